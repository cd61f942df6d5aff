"""Cost of ADS-B beside the AM path (--demod am --adsb): 60 s of int16 I/Q at 10 MS/s with --fs-ch 2e6 and
at 20 MS/s with --fs-ch 4e6, one target.  One second of capture (100 squitters on a carrier offset, noise) is made on the
host once and run 60 times through the channelizer and the AM block path, so nothing is read from a file.  By device events,
with and without ADS-B in the same process, alternating: the block demodulator (iqa_demodulate, and with ADS-B also
iqa_envelope and iqa_adsb_quantise), the finish stage (iqa_adsb_search, read-backs, parser) split into device calls and host
time, and one more pass with events around every entry point for the per-call split.  The yardstick is the same run without
the flag on the same build: the parent's AM path.  Prints one JSON line (kept as profiles/adsb_timing.json).  Every entry
point here is one kernel (iqa_adsb_search adds a small memset), so the per-call events are the per-kernel times.
Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=adsb``."""
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

import iq_to_audio_amd as A  # noqa: E402,F401
from iq_to_audio_amd import _native as N  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd.processing import ChannelBank, ChannelDemod, Channelizer  # noqa: E402

_spec = importlib.util.spec_from_file_location("adsb_model", ROOT / "tests" / "adsb_model.py")
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

SECS = 60
CONFIGS = ((10e6, 2e6), (20e6, 4e6))  # input rate, --fs-ch
OFFSET = 2.5e6
REPEATS = 3


def one_second(fs: float) -> np.ndarray:
    """int16 I/Q, one second: 100 squitters (the oracle's four, in turn) at +2.5 MHz and noise."""
    n = int(fs)
    rng = np.random.default_rng(5)
    per_chip = int(round(fs / 2e6))
    env = np.zeros(n, dtype=np.float32)
    for k in range(100):
        a = np.repeat(M.chips_of(M.FOUR[k % 4]), per_chip).astype(np.float32)
        at = 1000 + k * (n // 100) + k % per_chip
        env[at : at + a.size] = a
    t = np.arange(n, dtype=np.float64) / fs
    x = 0.5 * env * np.exp(2j * np.pi * OFFSET * t)
    x += 0.002 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    return np.rint(np.clip(np.column_stack((x.real, x.imag)), -0.999, 0.999) * 32767.0).astype(np.int16).reshape(-1)


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


def stage_times(raw, fs: float, fs_ch_target: float, adsb: bool) -> dict:
    d, fs_ch = P.choose_decimation(fs, fs_ch_target)
    taps = P.design_channel_filter(fs, 2e6, d)
    chan = Channelizer(taps, sample_rate=fs, freq_offset=OFFSET, mix_sign=1, decimation=d)
    chan.plan_ahead()
    bank = ChannelBank([chan])
    dem = ChannelDemod("am", fs_ch, deemph_us=300.0, agc_enabled=True, adsb=adsb)
    m_blk = -(-(raw.numel() // 2) // d)
    audio = torch.empty(m_blk, dtype=torch.float32, device="cuda")  # (reused: the audio is not what is measured)
    t_blk = 0.0
    for _ in range(SECS):
        z = bank.process(raw)[0]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        dem.process(z, np.array([0], dtype=np.int64), audio[: int(z.numel())])
        e[1].record()
        torch.cuda.synchronize()
        t_blk += e[0].elapsed_time(e[1])
    out = dict(adsb=adsb, block_ms=t_blk, channel_rate=fs_ch, decimation=d, blocks=SECS)
    if adsb:
        out["channel_samples"] = dem.side["adsb"].pos
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with CallTimes(("iqa_adsb_",)) as ct:
            res = dem.side_result("adsb")
            torch.cuda.synchronize()
            out["finish_ms"] = (time.perf_counter() - t0) * 1e3
        out["finish_device_ms"] = sum(ct.ms.values())
        out["finish_host_ms"] = out["finish_ms"] - out["finish_device_ms"]
        out["messages"] = 0 if res is None else len(res.messages)
        out["candidates_crc_ok"] = None if res is None else [res.candidates, res.crc_ok]
    return out


def med(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values), runs=len(values))


def main():
    torch.cuda.set_device(0)
    out = dict(capture=f"{SECS} s cs16, 100 squitters per second at +2.5 MHz, one target", device=torch.cuda.get_device_name(0), repeats=REPEATS,
               yardstick="the same run without adsb, same build", stages=[])
    for fs, fs_ch in CONFIGS:
        raw = torch.from_numpy(one_second(fs)).cuda()
        stage_times(raw, fs, fs_ch, False)  # warm-up: plans, tables, code objects
        stage_times(raw, fs, fs_ch, True)
        plain, with_ad, fin, fin_dev, fin_host, last = [], [], [], [], [], None
        for _ in range(REPEATS):  # alternating
            plain.append(stage_times(raw, fs, fs_ch, False)["block_ms"])
            last = stage_times(raw, fs, fs_ch, True)
            with_ad.append(last["block_ms"])
            fin.append(last["finish_ms"])
            fin_dev.append(last["finish_device_ms"])
            fin_host.append(last["finish_host_ms"])
        with CallTimes(("iqa_adsb_", "iqa_envelope", "iqa_demodulate")) as ct:
            stage_times(raw, fs, fs_ch, True)
        n_ch = last["channel_samples"]
        pl = P.plan_adsb(last["channel_rate"])
        search_bytes = 2 * n_ch * (1.0 + pl.span / 2048.0)  # q once, plus span halfwords per tile
        out["stages"].append(dict(input_rate=fs, channel_rate=last["channel_rate"], decimation=last["decimation"], channel_samples=n_ch,
                                  am_block_ms=med(plain), am_block_with_adsb_ms=med(with_ad),
                                  adsb_block_launches_ms=statistics.median(with_ad) - statistics.median(plain), adsb_finish_ms=med(fin),
                                  adsb_finish_device_ms=med(fin_dev), adsb_finish_host_ms=med(fin_host), messages=last["messages"],
                                  candidates_crc_ok=last["candidates_crc_ok"], search_bytes_by_count=search_bytes,
                                  per_call_ms=dict(ct.ms), per_call_count=dict(ct.counts)))
        del raw
    print(json.dumps(out))


if __name__ == "__main__":
    main()
