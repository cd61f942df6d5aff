"""Cost of the channel finder (--find-channels) on a device-resident capture: 60 s at 10 MS/s int16
(one second of four FM channels and noise, made on the host and tiled on the device), handed to ``ChannelFinder.process`` in
the blocks ``find_channels`` uses, then ``finish``.  By device events behind one warm-up: the whole run (median of REPEATS),
then REPEATS more runs with events around every entry point for the split into the existing ``iqa_psd_frames`` calls and the
new ``iqa_find_*`` ones.  For scale only, the one-channel NFM step (channelizer and demodulator, block by block) over the same
resident capture.  Prints one JSON line (kept as profiles/find_timing.json).
Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=find``."""
from __future__ import annotations

import importlib.util
import json
import statistics
import sys
import time
from collections import defaultdict
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from iq_to_audio_amd import _native as N  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd import find as FD  # noqa: E402
from iq_to_audio_amd.processing import ChannelDemod, Channelizer, ProcessingPipeline  # noqa: E402

_spec = importlib.util.spec_from_file_location("find_model", ROOT / "tests" / "find_model.py")
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

FS, SECS = 10e6, 60.0
CHANNELS = ((1.0e6, 1000.0, 3.0, 0.05), (-2.2e6, 700.0, 2.5, 0.005), (3.4e6, 5000.0, 15.0, 0.05))  # offset, tone, index, amplitude
BURST = (-0.6e6, 400.0, 3.0, 0.05, 0.3, 0.5)  # ... keyed from 0.3 to 0.5 s of every second
REPEATS = 5


def make_capture():
    """device int16[2 n]: one second made on the host, tiled SECS times."""
    n = int(FS)
    t = np.arange(n) / FS
    rng = np.random.default_rng(3)
    x = (0.05 * 10 ** -1.5 / np.sqrt(2.0)) * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + 0.01
    for offset, tone, index, amp in CHANNELS:
        x += M._fm(t, offset, tone, index, amp)
    offset, tone, index, amp, t0, t1 = BURST
    x += M._fm(t, offset, tone, index, amp) * ((t >= t0) & (t < t1))
    raw = np.empty((n, 2), dtype=np.int16)
    raw[:, 0], raw[:, 1] = np.rint(x.real * 32768.0), np.rint(x.imag * 32768.0)
    return torch.from_numpy(raw.reshape(-1)).cuda().repeat(int(SECS))


class CallTimes:
    """Device events around every native call whose name starts with one of ``prefixes`` (summed per name on exit)."""

    def __init__(self, prefixes):
        self.prefixes, self.events, self.ms, self.counts = tuple(prefixes), [], defaultdict(float), defaultdict(int)

    def __enter__(self):
        self.real = N.call

        def timed(name, *args):
            if not name.startswith(self.prefixes):
                return self.real(name, *args)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            try:
                return self.real(name, *args)
            finally:
                e[1].record()
                self.events.append((name, e))

        N.call = timed
        return self

    def __exit__(self, *exc):
        N.call = self.real
        torch.cuda.synchronize()
        for name, e in self.events:
            self.ms[name] += e[0].elapsed_time(e[1])
            self.counts[name] += 1
        return False


def find_run(capture, plan):
    """One whole run -> (device ms by events, wall ms, the result)."""
    finder = FD.ChannelFinder(plan, "s16")
    n = plan.n_samples
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e[0].record()
    for a in range(0, n, FD.BLOCK_FRAMES):
        finder.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    res = finder.result(145.0e6)
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), (time.perf_counter() - t0) * 1e3, res


def nfm_step(capture, n):
    """The one-channel NFM step over the same capture, block by block -> device ms by events."""
    d, fs_ch = P.choose_decimation(FS, 96_000.0)
    chan = Channelizer(P.design_channel_filter(FS, 12_500.0, d), sample_rate=FS, freq_offset=CHANNELS[0][0], mix_sign=1, decimation=d)
    chan.plan_ahead()
    dem = ChannelDemod("nfm", fs_ch, deemph_us=300.0, agc_enabled=True)
    audio = torch.empty(-(-n // d) + 16, dtype=torch.float32, device="cuda")
    block = ProcessingPipeline.block_frames_target
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    e[0].record()
    pos = 0
    for lo in range(0, n, block):
        z = chan.process(capture[2 * lo : 2 * min(n, lo + block)])
        m = int(z.numel())
        dem.process(z, np.array([0], dtype=np.int64), audio[pos : pos + m])
        pos += m
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1])


def med(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values), runs=len(values))


def main():
    torch.cuda.set_device(0)
    capture = make_capture()
    n = int(capture.numel()) // 2
    plan = P.plan_find(FS, n)
    out = dict(capture=f"{SECS:.0f} s @ {FS / 1e6:.0f} MS/s cs16, device-resident", device=torch.cuda.get_device_name(0), repeats=REPEATS,
               plan=dict(nfft=plan.nfft, frames=plan.frames, slice_frames=plan.slice_frames, slices=plan.slices, half=plan.half, gap=plan.gap))
    find_run(capture, plan)  # warm-up: FFT plans, code objects, pools
    runs = [find_run(capture, plan) for _ in range(REPEATS)]
    out["find_device_ms"], out["find_wall_ms"] = med([r[0] for r in runs]), med([r[1] for r in runs])
    out["channels"] = runs[-1][2].lines()
    split, counts = defaultdict(list), {}
    for _ in range(REPEATS):
        with CallTimes(("iqa_psd_frames", "iqa_find_")) as ct:
            find_run(capture, plan)
        for name, ms in ct.ms.items():
            split[name].append(ms)
        counts = dict(ct.counts)
    out["per_call_ms"] = {name: statistics.median(v) for name, v in split.items()}
    out["per_call_count"] = counts
    out["psd_frames_ms"] = out["per_call_ms"]["iqa_psd_frames"]
    out["find_kernels_ms"] = sum(ms for name, ms in out["per_call_ms"].items() if name.startswith("iqa_find_"))
    nfm_step(capture, n)
    out["nfm_one_channel_step_ms"] = med([nfm_step(capture, n) for _ in range(REPEATS)])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
