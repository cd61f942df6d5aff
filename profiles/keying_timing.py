"""Cost of the keying measurement (--find-decode) on the device-resident capture of
profiles/find_timing.py: 60 s at 10 MS/s int16, the capture and the method of profiles/describe_timing.py.  The finder runs
once; its channels then go through ``ChannelDescriber`` in the blocks ``find_channels`` uses, without and with ``keying``.  By
device events behind one warm-up each: the whole second pass with its result (median of REPEATS), then REPEATS more passes with
events around every native call for the time of ``iqa_quadrature`` plus ``iqa_keying_accumulate`` beside
``iqa_describe_accumulate``.  Prints one JSON line (kept as profiles/keying_timing.json).
Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=keying``."""
from __future__ import annotations

import importlib.util
import json
import statistics
import sys
import time
from collections import defaultdict
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from iq_to_audio_amd import describe as DS  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd import find as FD  # noqa: E402

_spec = importlib.util.spec_from_file_location("find_timing", ROOT / "profiles" / "find_timing.py")
FT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FT)

REPEATS = FT.REPEATS
FC = 145.0e6


def second_pass(capture, plan, fin, channels, keying: bool):
    """One whole second pass -> (device ms by events, wall ms, the describer)."""
    describer = DS.ChannelDescriber(plan, fin, channels, "s16", "iq", keying=keying)
    n = plan.n_samples
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e[0].record()
    for a in range(0, n, FD.BLOCK_FRAMES):
        describer.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    if keying:
        describer.keying_result(FC)
    else:
        describer.result(FC)
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), (time.perf_counter() - t0) * 1e3, describer


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
    for keying, tag in ((False, "describe"), (True, "keying")):
        second_pass(capture, plan, fin, found.channels, keying)  # warm-up: tap fragments, code objects, pools
        runs = [second_pass(capture, plan, fin, found.channels, keying) for _ in range(REPEATS)]
        out[f"{tag}_device_ms"], out[f"{tag}_wall_ms"] = FT.med([r[0] for r in runs]), FT.med([r[1] for r in runs])
        if keying:
            out["lines"] = [line.strip() for line in runs[-1][2].keying_result(FC).lines()]
            out["channels"] = [dict(offset_hz=ch.offset_hz, fs_ch=lane.plan.fs_ch, samples=lane.pos, keyed_from=lane.keyed_from)
                               for ch, lane in zip(found.channels, runs[-1][2].lanes())]
    split, counts = defaultdict(list), {}
    for _ in range(REPEATS):
        with FT.CallTimes(("iqa_",)) as ct:
            second_pass(capture, plan, fin, found.channels, True)
        for name, ms in ct.ms.items():
            split[name].append(ms)
        counts = dict(ct.counts)
    out["per_call_ms"] = {name: statistics.median(v) for name, v in split.items()}
    out["per_call_count"] = counts
    out["describe_kernel_ms"] = out["per_call_ms"].get("iqa_describe_accumulate", 0.0)
    out["keying_kernels_ms"] = out["per_call_ms"].get("iqa_quadrature", 0.0) + out["per_call_ms"].get("iqa_keying_accumulate", 0.0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
