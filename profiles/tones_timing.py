"""Cost of CTCSS / DTMF detection beside the NFM path (--demod nfm --tones), in the shape of
profiles/ax25_timing.py: 60 s of a 10 MS/s int16 capture with five 25 kHz voice channels (a CTCSS tone each, a DTMF digit
every 0.5 s, a few voice-band sines), one target then five.  By device events, with and without tones in the same process,
alternating: the block demodulator (iqa_demodulate, and with tones also iqa_quadrature + iqa_tones_decimate), the tone
launches alone (the difference), the finish stage (two bank calls, the decision call, read-back, parser) split into device
calls and host time; one more pass with events around every entry point for the per-call split; then the file -> WAV wall
time through MultiChannelPipeline with and without tones.  Prints one JSON line (kept as profiles/tones_timing.json).
Every entry point here is one kernel, so the per-call events are the per-kernel times.
Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=tones``."""
from __future__ import annotations

import importlib.util
import json
import math
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import iq_to_audio_amd as A  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd import iqio  # noqa: E402
from iq_to_audio_amd.processing import ChannelBank, ChannelDemod, Channelizer, ProcessingPipeline  # noqa: E402

_spec = importlib.util.spec_from_file_location("ax25_timing", ROOT / "profiles" / "ax25_timing.py")
_AX = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_AX)
CallTimes, med = _AX.CallTimes, _AX.med

FS, SECS, FC = 10e6, 60.0, 455.0e6
OFFSETS = (1.0e6, -2.2e6, 2.6e6, -0.6e6, 3.4e6)  # channel offsets (Hz); the first is the one-target run
TONES = (67.0, 100.0, 131.8, 203.5, 254.1)  # CTCSS, per channel
DIGITS = "159D#0A7*"  # one every 0.5 s (50 ms on), round and round
VOICE = ((430.0, 350.0), (1130.0, 400.0), (2310.0, 300.0))  # (Hz, peak deviation) of the voice-band sines
REPEATS = 5


def make_capture(path: Path, block: int = 10_000_000) -> int:
    """int16 I/Q of five voice channels and noise, generated on the device.  Returns the number of digits sent per channel."""
    n = int(FS * SECS)
    dev = torch.device("cuda", 0)
    rows = torch.tensor([P.DTMF_TONES[P.DTMF_KEYS.index(k) // 4] for k in DIGITS], dtype=torch.float64, device=dev)
    cols = torch.tensor([P.DTMF_TONES[4 + P.DTMF_KEYS.index(k) % 4] for k in DIGITS], dtype=torch.float64, device=dev)
    phase = torch.zeros(len(OFFSETS), dtype=torch.float64, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    with path.open("wb") as fh:
        fh.write(b"\0" * 44)
        for lo in range(0, n, block):
            idx = torch.arange(lo, min(lo + block, n), dtype=torch.float64, device=dev)
            t = idx / FS
            slot = torch.floor(t / 0.5)
            into = t - 0.5 * slot
            key = torch.remainder(slot, len(DIGITS)).to(torch.int64)
            on = (into >= 0.2) & (into < 0.25)
            dtmf = torch.where(on, 1000.0 * (torch.sin(2 * math.pi * rows[key] * into) + torch.sin(2 * math.pi * cols[key] * into)), 0.0)
            voice = sum(a * torch.sin(2 * math.pi * f * t) for f, a in VOICE)
            x = torch.zeros(t.numel(), dtype=torch.complex128, device=dev)
            for i, (f, tone) in enumerate(zip(OFFSETS, TONES)):
                dev_hz = 500.0 * torch.sin(2 * math.pi * tone * t) + voice + dtmf
                ph = phase[i] + 2 * math.pi / FS * torch.cumsum(dev_hz, 0)
                x += 0.15 * torch.exp(1j * (2 * math.pi * f * t + ph))
                phase[i] = torch.remainder(ph[-1], 2 * math.pi)
            x += 0.002 * torch.complex(torch.randn(t.numel(), generator=g, device=dev, dtype=torch.float64),
                                       torch.randn(t.numel(), generator=g, device=dev, dtype=torch.float64))
            iq = torch.stack([x.real, x.imag], 1).clamp(-0.999, 0.999).mul(32767.0).round().to(torch.int16)
            fh.write(iq.cpu().numpy().tobytes())
    data = path.stat().st_size - 44
    stub = path.with_suffix(".hdr.wav")
    iqio.write_wav_iq(stub, np.zeros(0, np.int16), int(FS), "s16")
    head = bytearray(stub.read_bytes()[:44])
    head[4:8] = (36 + data).to_bytes(4, "little")
    head[40:44] = data.to_bytes(4, "little")
    with path.open("r+b") as fh:
        fh.write(bytes(head))
    stub.unlink()
    return int(SECS / 0.5)


def summary(res) -> dict | None:
    if res is None:
        return None
    return dict(ctcss=[[e.tone_hz, round(e.start_s, 2), round(e.end_s, 2)] for e in res.ctcss], digits=len(res.dtmf),
                sequences=[s.digits[:12] for s in res.sequences])


def stage_times(path: Path, n_targets: int, tones: bool) -> dict:
    info = iqio.probe_capture(path)
    frames = iqio.map_frames(info)
    n = info.n_frames
    d, fs_ch = P.choose_decimation(FS, 96_000.0)
    taps = P.design_channel_filter(FS, 12_500.0, d)
    chans = [Channelizer(taps, sample_rate=FS, freq_offset=f, mix_sign=1, decimation=d) for f in OFFSETS[:n_targets]]
    for c in chans:
        c.plan_ahead()
    bank = ChannelBank(chans)
    dems = [ChannelDemod("nfm", fs_ch, deemph_us=300.0, agc_enabled=True, tones=tones) for _ in chans]
    n_dec = -(-n // d)
    audio = [torch.empty(n_dec, dtype=torch.float32, device="cuda") for _ in chans]
    block = ProcessingPipeline.block_frames_target
    t_blk, pos, blocks = 0.0, 0, 0
    for lo in range(0, n, block):
        hi = min(lo + block, n)
        raw = torch.from_numpy(np.ascontiguousarray(frames[2 * lo : 2 * hi])).cuda()
        zs = bank.process(raw)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        m = int(zs[0].numel())
        for dem, z, a in zip(dems, zs, audio):
            dem.process(z, np.array([0], dtype=np.int64), a[pos : pos + m])
        e[1].record()
        torch.cuda.synchronize()
        t_blk += e[0].elapsed_time(e[1])
        pos += m
        blocks += 1
    out = dict(targets=n_targets, tones=tones, block_ms=t_blk, channel_rate=fs_ch, blocks=blocks)
    if tones:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with CallTimes(("iqa_tones_bank", "iqa_tones_decide")) as ct:
            results = [dem.side_result("tones") for dem in dems]
            torch.cuda.synchronize()
            out["finish_ms"] = (time.perf_counter() - t0) * 1e3
        out["finish_device_ms"] = sum(ct.ms.values())
        out["finish_host_ms"] = out["finish_ms"] - out["finish_device_ms"]
        out["finish_per_call_ms"] = dict(ct.ms)
        out["results"] = [summary(r) for r in results]
        out["stored_u"] = [int(dem.side["tones"].joined()["u"].numel()) for dem in dems]
    return out


def end_to_end(path: Path, n_targets: int, out_dir: Path, tones: bool) -> dict:
    cfgs = [A.ProcessingConfig(in_path=path, target_freq=FC + f, center_freq=FC, demod_mode="nfm", output_path=out_dir / f"t{i}.wav")
            for i, f in enumerate(OFFSETS[:n_targets])]
    t0 = time.perf_counter()
    multi = A.MultiChannelPipeline(cfgs, tones=tones)
    multi.run()
    wall = time.perf_counter() - t0
    return dict(wall_s=wall, results=[summary(r) for r in multi.tones])


def main():
    torch.cuda.set_device(0)
    out = dict(capture=f"{SECS:.0f} s @ {FS / 1e6:.0f} MS/s cs16, five voice channels, CTCSS {TONES}, a DTMF digit every 0.5 s",
               device=torch.cuda.get_device_name(0), repeats=REPEATS)
    with tempfile.TemporaryDirectory() as d:
        path = Path(d) / "voice_455000000Hz.wav"
        out["digits_sent"] = make_capture(path)
        out["stages"] = []
        for k in (1, 5):
            stage_times(path, k, False)  # warm-up: plans, tables, code objects
            stage_times(path, k, True)
            plain, with_t, fin, fin_dev, fin_host, last = [], [], [], [], [], None
            for _ in range(REPEATS):  # alternating
                plain.append(stage_times(path, k, False)["block_ms"])
                last = stage_times(path, k, True)
                with_t.append(last["block_ms"])
                fin.append(last["finish_ms"])
                fin_dev.append(last["finish_device_ms"])
                fin_host.append(last["finish_host_ms"])
            with CallTimes(("iqa_tones_", "iqa_quadrature", "iqa_demodulate")) as ct:
                stage_times(path, k, True)
            out["stages"].append(dict(targets=k, channel_rate=last["channel_rate"], blocks=last["blocks"], nfm_block_ms=med(plain),
                                      nfm_block_with_tones_ms=med(with_t),
                                      tones_block_launches_ms=statistics.median(with_t) - statistics.median(plain),
                                      tones_finish_ms=med(fin), tones_finish_device_ms=med(fin_dev), tones_finish_host_ms=med(fin_host),
                                      finish_per_call_ms=last["finish_per_call_ms"], results=last["results"], stored_u=last["stored_u"],
                                      per_call_ms=dict(ct.ms), per_call_count=dict(ct.counts)))
            print(json.dumps(out), flush=True)  # (progress: the last line printed is the complete one)
        out["end_to_end"] = []
        for k in (1, 5):
            end_to_end(path, k, Path(d), False)  # warm-up (page cache, pinned pools)
            end_to_end(path, k, Path(d), True)
            plain, with_t, results = [], [], None
            for _ in range(REPEATS):
                plain.append(end_to_end(path, k, Path(d), False)["wall_s"])
                r = end_to_end(path, k, Path(d), True)
                with_t.append(r["wall_s"])
                results = r["results"]
            out["end_to_end"].append(dict(targets=k, wall_s=med(plain), wall_with_tones_s=med(with_t),
                                          realtime_factor=SECS / statistics.median(plain),
                                          realtime_factor_with_tones=SECS / statistics.median(with_t), results=results))
            print(json.dumps(out), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
