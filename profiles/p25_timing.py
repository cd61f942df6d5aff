"""Cost of the P25 frame decoding (--find-p25) by the method of profiles/layer_timing.py, with a P25
channel at -3.6 MHz: the test script of tests/p25_model.py (a call of four LDUs with its header and terminator, then six TSBK
frames) in a loop.  The whole second pass with ``identify`` alone and with ``p25`` beside it, then the three entry points on
their own.  Prints one JSON line (kept as profiles/p25_timing.json).  Kernel resources: ``make -C iq-to-audio_amd/csrc asm
F=p25``."""
from __future__ import annotations

import layer_timing as T
from iq_to_audio_amd import p25 as X

PM = T.load("p25_model", "tests")
FC = 145.0e6


def add_p25(capture) -> int:
    """The script's symbols in a loop, every symbol one entry of the level table.  Returns the frames sent."""
    table = PM.station(PM.SCRIPT)
    assert len(table) % 36 == 0
    T.add_channel(capture, table, 4800, PM.DEV)
    return int(capture.numel() // 2 * 4800 // (int(T.FT.FS) * len(table))) * len(PM.SCRIPT)


def summary(ch) -> dict:
    return dict(offset_hz=ch.offset_hz, note=ch.note, nacs=ch.nacs, frames=ch.frames, no_level=ch.no_level, cut=ch.cut,
                nid_refused=ch.nid_refused, nid_fixed=ch.nid_fixed, lc_failed=ch.lc_failed, crc_failed=ch.crc_failed,
                golay_refused=ch.golay_refused, hamming_unmatched=ch.hamming_unmatched, inverted=ch.inverted, calls=len(ch.calls),
                terminated=sum(c.terminated for c in ch.calls), tsbks=[(t.opcode, t.count) for t in ch.tsbks])


def entry_points(st, entry) -> dict:
    duids = X.decoder_duids(st["nid"])
    entry.update(samples=int(st["v"].numel()), frames=len(st["rows"]))
    entry["slice_ms"] = T.entry_ms(lambda: X.slice_frames(st["v"], st["rows"], st["plan"]))
    entry["nid_ms"] = T.entry_ms(lambda: X.decode_nids(st["bits"]))
    entry["decode_ms"] = T.entry_ms(lambda: X.decode_frames(st["bits"], duids))
    return entry


if __name__ == "__main__":
    T.run("p25", FC, "a P25 channel", add_p25, "frames_sent", summary, 7, entry_points)
