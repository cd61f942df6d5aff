"""Cost of the NXDN frame decoding (--find-nxdn) by the method of profiles/layer_timing.py, with an NXDN
channel at -3.6 MHz: the test script of tests/nxdn_model.py (a call of 11 frames: a header with a VCALL, two voice superframes, a
frame with a FACCH1 in its second half, the release) in a loop at 4800 symbols/s.  The whole second pass with ``identify``
alone and with ``nxdn`` beside it, then the two entry points on their own.  Prints one JSON line (kept as
profiles/nxdn_timing.json).  Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=nxdn``."""
from __future__ import annotations

import layer_timing as T
from iq_to_audio_amd import nxdn as X

NM = T.load("nxdn_model", "tests")
FC = 433.0e6


def add_nxdn(capture) -> int:
    """The script's symbols in a loop, every symbol one entry of the level table.  Returns the frames sent."""
    table = NM.station(NM.SCRIPT)
    assert len(table) == 192 * len(NM.SCRIPT)
    T.add_channel(capture, table, 4800, NM.DEV)
    return int(capture.numel() // 2 * 4800 // (int(T.FT.FS) * 192))


def summary(ch) -> dict:
    return dict(offset_hz=ch.offset_hz, note=ch.note, rate=ch.rate, frames=ch.frames, inverted=ch.inverted, calls=len(ch.calls),
                released=sum(c.released for c in ch.calls), late=sum(c.late for c in ch.calls), conflicts=sum(c.conflicts for c in ch.calls),
                control=len(ch.control), **{k: getattr(ch, k) for k in X.new_counts()})


def entry_points(st, entry) -> dict:
    entry.update(samples=int(st["v"].numel()), frames=len(st["rows"]))
    entry["slice_ms"] = T.entry_ms(lambda: X.slice_frames(st["v"], st["rows"], st["plan"]))
    entry["decode_ms"] = T.entry_ms(lambda: X.decode_frames(st["bits"], st["classes"]))
    return entry


if __name__ == "__main__":
    T.run("nxdn", FC, "an NXDN channel", add_nxdn, "frames_sent", summary, 3, entry_points)
