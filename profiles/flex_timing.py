"""Cost of the FLEX page decoding (--find-flex) on the device-resident capture of profiles/find_timing.py
(60 s at 10 MS/s int16, the capture and the method of profiles/ident_timing.py) with a FLEX channel added: 32 frames of 3200/2,
back to back, at -3.6 MHz, written into the capture on the device.  The finder runs once; its channels then go through
``ChannelDescriber`` in the blocks ``find_channels`` uses, with ``identify`` alone (the yardstick) and with ``flex`` beside it,
alternating in one process.  By device events behind one warm-up each: the whole second pass with its results (median of
REPEATS).  Then the two entry points on their own, on the FLEX lane's planes: median of REPEATS each.  Prints one JSON line (kept
as profiles/flex_timing.json).  Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=flex``."""
from __future__ import annotations

import importlib.util
import json
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from iq_to_audio_amd import describe as DS  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd import find as FD  # noqa: E402
from iq_to_audio_amd import flex as X  # noqa: E402


def _load(name, folder):
    spec = importlib.util.spec_from_file_location(name, ROOT / folder / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


FT = _load("find_timing", "profiles")
FM = _load("flex_model", "tests")

REPEATS = FT.REPEATS
FC = 145.0e6
FLEX_OFFSET, FLEX_AMP, FLEX_MODE = -3.6e6, 0.01, "3200/2"  # (at 0.05 the sidelobes of the rectangular symbols read as a wide FM channel)
PAGES = {"A": [dict(kind="alpha", capcode=1234567, text="TIMING CAPTURE"), dict(kind="numeric", capcode=4242, text="555-0199")],
         "C": [dict(kind="alpha", capcode=99, text="PHASE C", fragment=0, more=True)]}


def add_flex(capture) -> int:
    """Adds the FLEX channel to the device capture in place, a second at a time: frames of 3000 bits of the 1600 bit/s grid
    back to back, every half bit one entry of a level table.  Returns the frames sent."""
    segments, _ = FM.make_frame(FLEX_MODE, 3, 45, PAGES)
    table = []
    for lev, length in segments:
        table += [lev] * int(round(2 * length))
    assert len(table) == 6000
    levels = torch.tensor(table, dtype=torch.float64, device="cuda")
    fs, n = FT.FS, int(capture.numel()) // 2
    phase = 0.0
    for a in range(0, n, int(fs)):
        b = min(n, a + int(fs))
        k = torch.arange(a, b, dtype=torch.int64, device="cuda")
        half = torch.div(k * 3200, int(fs), rounding_mode="floor") % 6000
        turns = torch.cumsum(levels[half] * (1600.0 / fs), 0) + phase
        phase = float(turns[-1]) % 1.0
        angle = 2.0 * math.pi * ((turns + (k.to(torch.float64) * (FLEX_OFFSET / fs))) % 1.0)
        z = torch.stack([torch.cos(angle), torch.sin(angle)], dim=1) * (FLEX_AMP * 32768.0)
        capture[2 * a : 2 * b] += torch.round(z).to(torch.int16).reshape(-1)
    return int(n * 1600 // (int(fs) * 3000))


def second_pass(capture, plan, fin, channels, flex: bool):
    """One whole second pass -> (device ms by events, wall ms, the describer)."""
    describer = DS.ChannelDescriber(plan, fin, channels, "s16", "iq", keying=True, identify=True, flex=flex)
    n = plan.n_samples
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e[0].record()
    for a in range(0, n, FD.BLOCK_FRAMES):
        describer.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    describer.keying_result(FC)
    describer.protocol_result(FC)
    if flex:
        describer.flex_result(FC)
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), (time.perf_counter() - t0) * 1e3, describer


def timed(fn) -> float:
    """Device ms of one call of ``fn`` by events."""
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    e[0].record()
    fn()
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1])


def main():
    torch.cuda.set_device(0)
    capture = FT.make_capture()
    sent = add_flex(capture)
    n = int(capture.numel()) // 2
    plan = P.plan_find(FT.FS, n)
    out = dict(capture=f"{FT.SECS:.0f} s @ {FT.FS / 1e6:.0f} MS/s cs16, device-resident, with a FLEX {FLEX_MODE} channel at {FLEX_OFFSET:+.0f} Hz",
               device=torch.cuda.get_device_name(0), repeats=REPEATS, frames_sent=sent)
    finder = FD.ChannelFinder(plan, "s16")
    for a in range(0, n, FD.BLOCK_FRAMES):
        finder.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    fin, found = finder.finish(), finder.result(FC)
    runs = {False: [], True: []}
    for flex in (False, True):
        second_pass(capture, plan, fin, found.channels, flex)  # warm-up: tap fragments, code objects, pools
    last = None
    for _ in range(REPEATS):  # alternating
        for flex in (False, True):
            r = second_pass(capture, plan, fin, found.channels, flex)
            runs[flex].append(r)
            last = r[2] if flex else last
    for flex, tag in ((False, "identify"), (True, "flex")):
        out[f"{tag}_device_ms"], out[f"{tag}_wall_ms"] = FT.med([r[0] for r in runs[flex]]), FT.med([r[1] for r in runs[flex]])
    out["keying"] = [line.strip() for line in last.keying_result(FC).lines()]
    out["protocols"] = [line.strip() for line in last.protocol_result(FC).lines()]
    result = last.flex_result(FC)
    out["channels"] = [dict(offset_hz=ch.offset_hz, note=ch.note, frames=ch.frames, unknown_mode=ch.unknown_mode, no_level=ch.no_level,
                            fiw_failed=ch.fiw_failed, biw_lost=ch.biw_lost, biw_bad=ch.biw_bad, vectors_dropped=ch.vectors_dropped,
                            words=ch.words, shifts=ch.shifts, pages=len(ch.pages)) for ch in result.channels]
    out["first_lines"] = result.lines()[:3]
    entries = []
    for ch, lane, st in zip(found.channels, last.lanes(), last.finish_flex()):
        if "rows" not in st or not st["rows"]:
            continue
        fplan = st["plan"]
        ms = np.array([(m, s) for m, s, _ in st["rows"]], dtype=np.int64)
        entry = dict(offset_hz=ch.offset_hz, fs_ch=lane.plan.fs_ch, sps=fplan.sps, samples=int(st["v16"].numel()), frames=len(st["rows"]))
        X.frames(st["v16"], ms, fplan)  # warm-up
        entry["frames_ms"] = FT.med([timed(lambda: X.frames(st["v16"], ms, fplan)) for _ in range(REPEATS)])
        for mode, (u, levels) in X.MODE_SHAPE.items():
            sel = [j for j, row in enumerate(st["rows"]) if row[2] == mode and st["ok"][j]]
            if not sel:
                continue
            plane = st["v16"] if u == 1 else st["v32"]
            rec = (st["rec16"] if u == 1 else st["rec32"])[sel, :2]
            recs = np.concatenate([ms[sel], rec], axis=1)
            X.words(plane, recs, levels, u, fplan)  # warm-up
            entry[f"words_{mode}_ms"] = FT.med([timed(lambda: X.words(plane, recs, levels, u, fplan)) for _ in range(REPEATS)])
            entry[f"words_{mode}_frames"] = len(sel)
        entries.append(entry)
    out["entry_points"] = entries
    print(json.dumps(out))


if __name__ == "__main__":
    main()
