"""Cost of the FLEX page decoding (--find-flex) by the method of profiles/layer_timing.py, with a FLEX
channel at -3.6 MHz: 32 frames of 3200/2, back to back.  The whole second pass with ``identify`` alone and with ``flex`` beside
it, then the two entry points on their own, on the FLEX lane's planes.  Prints one JSON line (kept as
profiles/flex_timing.json).  Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=flex``."""
from __future__ import annotations

import layer_timing as T
import numpy as np
from iq_to_audio_amd import flex as X

FM = T.load("flex_model", "tests")
FC = 145.0e6
FLEX_MODE = "3200/2"
PAGES = {"A": [dict(kind="alpha", capcode=1234567, text="TIMING CAPTURE"), dict(kind="numeric", capcode=4242, text="555-0199")],
         "C": [dict(kind="alpha", capcode=99, text="PHASE C", fragment=0, more=True)]}


def add_flex(capture) -> int:
    """Frames of 3000 bits of the 1600 bit/s grid back to back, every half bit one entry of the level table.  Returns the frames
    sent."""
    segments, _ = FM.make_frame(FLEX_MODE, 3, 45, PAGES)
    table = []
    for lev, length in segments:
        table += [lev] * int(round(2 * length))
    assert len(table) == 6000
    T.add_channel(capture, table, 3200, 1600.0)
    return int(capture.numel() // 2 * 1600 // (int(T.FT.FS) * 3000))


def summary(ch) -> dict:
    return dict(offset_hz=ch.offset_hz, note=ch.note, frames=ch.frames, unknown_mode=ch.unknown_mode, no_level=ch.no_level,
                fiw_failed=ch.fiw_failed, biw_lost=ch.biw_lost, biw_bad=ch.biw_bad, vectors_dropped=ch.vectors_dropped,
                words=ch.words, shifts=ch.shifts, pages=len(ch.pages))


def entry_points(st, entry) -> dict:
    fplan = st["plan"]
    ms = np.array([(m, s) for m, s, _ in st["rows"]], dtype=np.int64)
    entry.update(samples=int(st["v16"].numel()), frames=len(st["rows"]))
    entry["frames_ms"] = T.entry_ms(lambda: X.frames(st["v16"], ms, fplan))
    for mode, (u, levels) in X.MODE_SHAPE.items():
        sel = [j for j, row in enumerate(st["rows"]) if row[2] == mode and st["ok"][j]]
        if not sel:
            continue
        plane = st["v16"] if u == 1 else st["v32"]
        recs = np.concatenate([ms[sel], (st["rec16"] if u == 1 else st["rec32"])[sel, :2]], axis=1)
        entry[f"words_{mode}_ms"] = T.entry_ms(lambda: X.words(plane, recs, levels, u, fplan))
        entry[f"words_{mode}_frames"] = len(sel)
    return entry


if __name__ == "__main__":
    T.run("flex", FC, "a FLEX 3200/2 channel", add_flex, "frames_sent", summary, 3, entry_points)
