"""Cost of the carrier squelch (--squelch) on the device-resident capture of profiles/find_timing.py:
60 s at 10 MS/s int16, one NFM target (the burst channel, keyed 0.2 s of every second).  The target's run -- channelizer and
demodulator block by block, then the 48 kHz resampler to PCM16 -- without the squelch and with it, alternating in one process.
By device events behind one warm-up each: the whole run (median of REPEATS), then REPEATS more gated runs with events around
every new entry point.  The yardstick is the run without the flag on the same build: that path is unchanged.  Prints one JSON
line (kept as profiles/gate_timing.json).
Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=gate``."""
from __future__ import annotations

import importlib.util
import json
import statistics
import sys
from collections import defaultdict
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd.gate import CarrierGate, CarrierSquelch  # noqa: E402
from iq_to_audio_amd.processing import ChannelDemod, Channelizer, ProcessingPipeline, Resampler48k  # noqa: E402

_spec = importlib.util.spec_from_file_location("find_timing", ROOT / "profiles" / "find_timing.py")
FT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FT)

REPEATS = FT.REPEATS


def target_run(capture, n, squelch: bool):
    """One whole run of the target -> (device ms by events, the PCM16 tensor, the gate's result or None)."""
    d, fs_ch = P.choose_decimation(FT.FS, 96_000.0)
    chan = Channelizer(P.design_channel_filter(FT.FS, 12_500.0, d), sample_rate=FT.FS, freq_offset=FT.BURST[0], mix_sign=1, decimation=d)
    chan.plan_ahead()
    dem = ChannelDemod("nfm", fs_ch, deemph_us=300.0, agc_enabled=True)
    gate = CarrierGate(P.plan_gate(fs_ch, CarrierSquelch())) if squelch else None
    rs = Resampler48k(fs_ch)
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
        if gate is not None:
            gate.process(z)
        pos += m
    out, res = audio[:pos], None
    if gate is not None:
        gate.finish(pos)
        out = gate.apply(out)
        res = gate.result(145.0e6 + FT.BURST[0])
    pcm = rs.process(out, want="pcm16")
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), pcm, res


def main():
    torch.cuda.set_device(0)
    capture = FT.make_capture()
    n = int(capture.numel()) // 2
    out = dict(capture=f"{FT.SECS:.0f} s @ {FT.FS / 1e6:.0f} MS/s cs16, device-resident", device=torch.cuda.get_device_name(0), repeats=REPEATS)
    for flag in (False, True):
        target_run(capture, n, flag)  # warm-up: tap fragments, code objects, pools
    plain, gated, res, pcm = [], [], None, None
    for _ in range(REPEATS):  # alternating: the same machine state for both
        plain.append(target_run(capture, n, False)[0])
        ms, pcm, res = target_run(capture, n, True)
        gated.append(ms)
    out["plain_device_ms"], out["squelch_device_ms"] = FT.med(plain), FT.med(gated)
    out["channel_samples"], out["frames"], out["sh"], out["floor_dbfs"], out["duty"] = res.samples, -(-res.samples // res.frame), res.sh, res.floor_dbfs, res.duty
    out["transmissions"] = len(res.transmissions)
    out["lines"] = res.lines()[:3]
    out["pcm_zero_share"] = float((pcm == 0).float().mean().item())
    split, counts = defaultdict(list), {}
    for _ in range(REPEATS):
        with FT.CallTimes(("iqa_gate_",)) as ct:
            target_run(capture, n, True)
        for name, ms in ct.ms.items():
            split[name].append(ms)
        counts = dict(ct.counts)
    out["per_call_ms"] = {name: statistics.median(v) for name, v in split.items()}
    out["per_call_count"] = counts
    out["gate_kernels_ms"] = sum(out["per_call_ms"].values())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
