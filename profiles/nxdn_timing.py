"""Cost of the NXDN frame decoding (--find-nxdn) on the device-resident capture of profiles/find_timing.py
(60 s at 10 MS/s int16, the capture and the method of profiles/ysf_timing.py) with an NXDN channel in place of the YSF one: the
test script of tests/nxdn_model.py (a call of 11 frames: a header with a VCALL, two voice superframes, a frame with a FACCH1 in
its second half, the release) in a loop at 4800 symbols/s, at -3.6 MHz, written into the capture on the device.  The finder
runs once; its channels then go through ``ChannelDescriber`` in the blocks ``find_channels`` uses, with ``identify`` alone (the
yardstick) and with ``nxdn`` beside it, alternating in one process.  By device events behind one warm-up each: the whole second
pass with its results (median of REPEATS).  Then the two entry points on their own, on the NXDN lane's plane: median of REPEATS
each.  Prints one JSON line (kept as profiles/nxdn_timing.json).  Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=nxdn``."""
from __future__ import annotations

import importlib.util
import json
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from iq_to_audio_amd import describe as DS  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd import find as FD  # noqa: E402
from iq_to_audio_amd import nxdn as X  # noqa: E402


def _load(name, folder):
    spec = importlib.util.spec_from_file_location(name, ROOT / folder / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


FT = _load("find_timing", "profiles")
NM = _load("nxdn_model", "tests")

REPEATS = FT.REPEATS
FC = 433.0e6
NXDN_OFFSET, NXDN_AMP = -3.6e6, 0.01  # (the place and the amplitude of profiles/dmr_timing.py's added channel)


def add_nxdn(capture) -> int:
    """Adds the NXDN channel to the device capture in place, a second at a time: the script's symbols in a loop, every symbol one
    entry of a level table.  Returns the frames sent."""
    table = NM.station(NM.SCRIPT)
    assert len(table) == 192 * len(NM.SCRIPT)
    levels = torch.tensor(table, dtype=torch.float64, device="cuda")
    fs, n = FT.FS, int(capture.numel()) // 2
    phase = 0.0
    for a in range(0, n, int(fs)):
        b = min(n, a + int(fs))
        k = torch.arange(a, b, dtype=torch.int64, device="cuda")
        symbol = torch.div(k * 4800, int(fs), rounding_mode="floor") % len(table)
        turns = torch.cumsum(levels[symbol] * (NM.DEV / fs), 0) + phase
        phase = float(turns[-1]) % 1.0
        angle = 2.0 * math.pi * ((turns + (k.to(torch.float64) * (NXDN_OFFSET / fs))) % 1.0)
        z = torch.stack([torch.cos(angle), torch.sin(angle)], dim=1) * (NXDN_AMP * 32768.0)
        capture[2 * a : 2 * b] += torch.round(z).to(torch.int16).reshape(-1)
    return int(n * 4800 // (int(fs) * 192))


def second_pass(capture, plan, fin, channels, nxdn: bool):
    """One whole second pass -> (device ms by events, wall ms, the describer)."""
    describer = DS.ChannelDescriber(plan, fin, channels, "s16", "iq", keying=True, identify=True, nxdn=nxdn)
    n = plan.n_samples
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e[0].record()
    for a in range(0, n, FD.BLOCK_FRAMES):
        describer.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    describer.keying_result(FC)
    describer.protocol_result(FC)
    if nxdn:
        describer.nxdn_result(FC)
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
    sent = add_nxdn(capture)
    n = int(capture.numel()) // 2
    plan = P.plan_find(FT.FS, n)
    out = dict(capture=f"{FT.SECS:.0f} s @ {FT.FS / 1e6:.0f} MS/s cs16, device-resident, with an NXDN channel at {NXDN_OFFSET:+.0f} Hz",
               device=torch.cuda.get_device_name(0), repeats=REPEATS, frames_sent=sent)
    finder = FD.ChannelFinder(plan, "s16")
    for a in range(0, n, FD.BLOCK_FRAMES):
        finder.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    fin, found = finder.finish(), finder.result(FC)
    runs = {False: [], True: []}
    for nxdn in (False, True):
        second_pass(capture, plan, fin, found.channels, nxdn)  # warm-up: tap fragments, code objects, pools
    last = None
    for _ in range(REPEATS):  # alternating
        for nxdn in (False, True):
            r = second_pass(capture, plan, fin, found.channels, nxdn)
            runs[nxdn].append(r)
            last = r[2] if nxdn else last
    for nxdn, tag in ((False, "identify"), (True, "nxdn")):
        out[f"{tag}_device_ms"], out[f"{tag}_wall_ms"] = FT.med([r[0] for r in runs[nxdn]]), FT.med([r[1] for r in runs[nxdn]])
    out["keying"] = [line.strip() for line in last.keying_result(FC).lines()]
    out["protocols"] = [line.strip() for line in last.protocol_result(FC).lines()]
    result = last.nxdn_result(FC)
    counters = tuple(X.new_counts())
    out["channels"] = [dict(offset_hz=ch.offset_hz, note=ch.note, rate=ch.rate, frames=ch.frames, inverted=ch.inverted, calls=len(ch.calls),
                            released=sum(c.released for c in ch.calls), late=sum(c.late for c in ch.calls), conflicts=sum(c.conflicts for c in ch.calls),
                            control=len(ch.control), **{k: getattr(ch, k) for k in counters}) for ch in result.channels]
    out["first_lines"] = result.lines()[:3]
    entries = []
    for ch, lane, st in zip(found.channels, last.lanes(), last.finish_nxdn()):
        if "rows" not in st or not len(st["rows"]):
            continue
        nplan, rows = st["plan"], st["rows"]
        entry = dict(offset_hz=ch.offset_hz, fs_ch=lane.plan.fs_ch, sps=nplan.sps, samples=int(st["v"].numel()), frames=len(rows))
        X.slice_frames(st["v"], rows, nplan)  # warm-up
        entry["slice_ms"] = FT.med([timed(lambda: X.slice_frames(st["v"], rows, nplan)) for _ in range(REPEATS)])
        X.decode_frames(st["bits"], st["classes"])  # warm-up
        entry["decode_ms"] = FT.med([timed(lambda: X.decode_frames(st["bits"], st["classes"])) for _ in range(REPEATS)])
        entries.append(entry)
    out["entry_points"] = entries
    print(json.dumps(out))


if __name__ == "__main__":
    main()
