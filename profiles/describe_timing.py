"""Cost of the channel description (--find-describe) on the device-resident capture of
profiles/find_timing.py: 60 s at 10 MS/s int16.  The finder runs once; its channels then go through ``ChannelDescriber`` in the
blocks ``find_channels`` uses.  By device events behind one warm-up: the whole second pass with ``result()`` (median of
REPEATS), then REPEATS more passes with events around every native call for the split into the channelizer's entry points, the
one ``iqa_mean_power`` per channel and the new ``iqa_describe_accumulate``.  Beside it the finder's own pass, measured the same
way in the same process.  Prints one JSON line (kept as profiles/describe_timing.json).
Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=describe``."""
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


def describe_run(capture, plan, fin, channels):
    """One whole second pass -> (device ms by events, wall ms, the result)."""
    describer = DS.ChannelDescriber(plan, fin, channels, "s16", "iq")
    n = plan.n_samples
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e[0].record()
    for a in range(0, n, FD.BLOCK_FRAMES):
        describer.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    res = describer.result(FC)
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), (time.perf_counter() - t0) * 1e3, res


def main():
    torch.cuda.set_device(0)
    capture = FT.make_capture()
    n = int(capture.numel()) // 2
    plan = P.plan_find(FT.FS, n)
    out = dict(capture=f"{FT.SECS:.0f} s @ {FT.FS / 1e6:.0f} MS/s cs16, device-resident", device=torch.cuda.get_device_name(0), repeats=REPEATS)
    FT.find_run(capture, plan)  # warm-up
    out["find_device_ms"] = FT.med([FT.find_run(capture, plan)[0] for _ in range(REPEATS)])
    finder = FD.ChannelFinder(plan, "s16")
    for a in range(0, n, FD.BLOCK_FRAMES):
        finder.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    fin, found = finder.finish(), finder.result(FC)
    plans = [P.plan_describe(FT.FS, ch.offset_hz, ch.width_hz) for ch in found.channels]
    out["channels"] = [dict(offset_hz=ch.offset_hz, width_hz=ch.width_hz, bw=p.bw, decimation=p.decimation, fs_ch=p.fs_ch, taps=len(p.taps))
                       for ch, p in zip(found.channels, plans)]
    describe_run(capture, plan, fin, found.channels)  # warm-up: tap fragments, code objects, pools
    runs = [describe_run(capture, plan, fin, found.channels) for _ in range(REPEATS)]
    out["describe_device_ms"], out["describe_wall_ms"] = FT.med([r[0] for r in runs]), FT.med([r[1] for r in runs])
    out["lines"] = [line.strip() for line in runs[-1][2].lines()]
    split, counts = defaultdict(list), {}
    for _ in range(REPEATS):
        with FT.CallTimes(("iqa_",)) as ct:
            describe_run(capture, plan, fin, found.channels)
        for name, ms in ct.ms.items():
            split[name].append(ms)
        counts = dict(ct.counts)
    out["per_call_ms"] = {name: statistics.median(v) for name, v in split.items()}
    out["per_call_count"] = counts
    out["describe_kernel_ms"] = out["per_call_ms"].get("iqa_describe_accumulate", 0.0)
    out["channelizer_ms"] = sum(ms for name, ms in out["per_call_ms"].items() if name.startswith(("iqa_channelize", "iqa_mfma", "iqa_history")))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
