"""Cost of the YSF frame decoding (--find-ysf) by the method of profiles/layer_timing.py, with a YSF
channel at -3.6 MHz: the test script of tests/ysf_model.py (a transmission of 13 frames: header, V/D mode 2, V/D mode 1, data FR,
voice FR, terminator) in a loop.  The whole second pass with ``identify`` alone and with ``ysf`` beside it, then the three entry
points on their own.  Prints one JSON line (kept as profiles/ysf_timing.json).  Kernel resources: ``make -C
iq-to-audio_amd/csrc asm F=ysf``."""
from __future__ import annotations

import layer_timing as T
from iq_to_audio_amd import ysf as X

YM = T.load("ysf_model", "tests")
FC = 433.0e6


def add_ysf(capture) -> int:
    """The script's symbols in a loop, every symbol one entry of the level table.  Returns the frames sent."""
    table = YM.station(YM.SCRIPT)
    assert len(table) == 480 * len(YM.SCRIPT)
    T.add_channel(capture, table, 4800, YM.DEV)
    return int(capture.numel() // 2 * 4800 // (int(T.FT.FS) * 480))


def summary(ch) -> dict:
    return dict(offset_hz=ch.offset_hz, note=ch.note, frames=ch.frames, no_level=ch.no_level, cut=ch.cut, fich_failed=ch.fich_failed,
                golay_refused=ch.golay_refused, dch_failed=ch.dch_failed, fixed=ch.fixed, inverted=ch.inverted,
                transmissions=len(ch.transmissions), terminated=sum(t.terminated for t in ch.transmissions),
                conflicts=sum(t.conflicts for t in ch.transmissions))


def entry_points(st, entry) -> dict:
    entry.update(samples=int(st["v"].numel()), frames=len(st["rows"]))
    entry["slice_ms"] = T.entry_ms(lambda: X.slice_frames(st["v"], st["rows"], st["plan"]))
    entry["fich_ms"] = T.entry_ms(lambda: X.decode_fich(st["bits"]))
    entry["decode_ms"] = T.entry_ms(lambda: X.decode_frames(st["bits"], st["classes"]))
    return entry


if __name__ == "__main__":
    T.run("ysf", FC, "a YSF channel", add_ysf, "frames_sent", summary, 3, entry_points)
