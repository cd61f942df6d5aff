"""Cost of the DMR burst decoding (--find-dmr) by the method of profiles/layer_timing.py, with a DMR base
channel at -3.6 MHz: the test script of tests/dmr_model.py (idle bursts, a header, three superframes, a terminator, a CSBK) in a
loop of 48 slots.  The whole second pass with ``identify`` alone and with ``dmr`` beside it, then the two entry points on their
own.  Prints one JSON line (kept as profiles/dmr_timing.json).  Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=dmr``."""
from __future__ import annotations

import layer_timing as T
from iq_to_audio_amd import dmr as X

DM = T.load("dmr_model", "tests")
FC = 145.0e6
LOOP_SLOTS = 48


def add_dmr(capture) -> int:
    """The script's symbols in a loop, every symbol one entry of the level table.  Returns the slots sent."""
    table = DM.base_station(list(DM.SCRIPT) + [None] * (LOOP_SLOTS - len(DM.SCRIPT)))
    assert len(table) == 144 * LOOP_SLOTS
    T.add_channel(capture, table, 4800, DM.DEV)
    return int(capture.numel() // 2 * 4800 // (int(T.FT.FS) * 144))


def summary(ch) -> dict:
    return dict(offset_hz=ch.offset_hz, note=ch.note, kinds=ch.kinds, no_level=ch.no_level, cut=ch.cut, slot_refused=ch.slot_refused,
                bptc_failed=ch.bptc_failed, check_failed=ch.check_failed, tact_fixed=ch.tact_fixed, idle=ch.idle,
                calls=len(ch.calls), terminated=sum(c.terminated for c in ch.calls), bursts=len(ch.bursts))


def entry_points(st, entry) -> dict:
    entry.update(samples=int(st["v"].numel()), bursts=len(st["rows"]))
    entry["slice_ms"] = T.entry_ms(lambda: X.slice_bursts(st["v"], st["rows"], st["plan"]))
    entry["decode_ms"] = T.entry_ms(lambda: X.decode_bursts(st["bits"], st["rows"][:, 2]))
    return entry


if __name__ == "__main__":
    T.run("dmr", FC, "a DMR base channel", add_dmr, "slots_sent", summary, 3, entry_points)
