"""Cost of the protocol identification (--find-identify) on the device-resident capture of
profiles/find_timing.py: 60 s at 10 MS/s int16, the capture and the method of profiles/keying_timing.py.  The finder runs once;
its channels then go through ``ChannelDescriber`` in the blocks ``find_channels`` uses, with ``keying`` alone (the yardstick) and
with ``identify`` beside it, in one process.  By device events behind one warm-up each: the whole second pass with its result
(median of REPEATS).  Then the two entry points on their own, on every lane's stored discriminator stream at every family whose
rate fits it, whatever the lane's label (the capture's channels need not be keyed): median of REPEATS each.  Prints one JSON
line (kept as profiles/ident_timing.json).  Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=ident``."""
from __future__ import annotations

import importlib.util
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from iq_to_audio_amd import describe as DS  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd import find as FD  # noqa: E402
from iq_to_audio_amd import identify as I  # noqa: E402

_spec = importlib.util.spec_from_file_location("find_timing", ROOT / "profiles" / "find_timing.py")
FT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FT)

REPEATS = FT.REPEATS
FC = 145.0e6


def second_pass(capture, plan, fin, channels, identify: bool):
    """One whole second pass -> (device ms by events, wall ms, the describer)."""
    describer = DS.ChannelDescriber(plan, fin, channels, "s16", "iq", keying=True, identify=identify)
    n = plan.n_samples
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e[0].record()
    for a in range(0, n, FD.BLOCK_FRAMES):
        describer.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    describer.keying_result(FC)
    if identify:
        describer.protocol_result(FC)
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
    n = int(capture.numel()) // 2
    plan = P.plan_find(FT.FS, n)
    out = dict(capture=f"{FT.SECS:.0f} s @ {FT.FS / 1e6:.0f} MS/s cs16, device-resident", device=torch.cuda.get_device_name(0), repeats=REPEATS)
    finder = FD.ChannelFinder(plan, "s16")
    for a in range(0, n, FD.BLOCK_FRAMES):
        finder.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    fin, found = finder.finish(), finder.result(FC)
    last = None
    for identify, tag in ((False, "keying"), (True, "identify")):
        second_pass(capture, plan, fin, found.channels, identify)  # warm-up: tap fragments, code objects, pools
        runs = [second_pass(capture, plan, fin, found.channels, identify) for _ in range(REPEATS)]
        out[f"{tag}_device_ms"], out[f"{tag}_wall_ms"] = FT.med([r[0] for r in runs]), FT.med([r[1] for r in runs])
        last = runs[-1][2]
    out["lines"] = [line.strip() for line in last.protocol_result(FC).lines()]
    out["stored_bytes"] = sum(4 * sum(int(t.numel()) for t in lane.stored) for lane in last.lanes())
    entries = []
    for ch, lane in zip(found.channels, last.lanes()):
        if lane.centre is None or not lane.stored:
            continue
        theta = torch.cat(lane.stored)
        for rate in (4800, 2400, 1600):
            try:
                iplan = P.plan_ident(lane.plan.fs_ch, rate)
            except ValueError:
                continue
            pats = I.patterns_for(rate)
            v = I.integrate(theta, iplan, lane.centre)  # warm-up
            _, hits = I.search(v, iplan, pats)
            entries.append(dict(offset_hz=ch.offset_hz, fs_ch=lane.plan.fs_ch, samples=int(theta.numel()), rate=rate, sps=iplan.sps,
                                patterns=len(pats), kept=int(hits.shape[0]),
                                integrate_ms=FT.med([timed(lambda: I.integrate(theta, iplan, lane.centre)) for _ in range(REPEATS)]),
                                search_ms=FT.med([timed(lambda: I.search(v, iplan, pats)) for _ in range(REPEATS)])))
    out["entry_points"] = entries
    print(json.dumps(out))


if __name__ == "__main__":
    main()
