"""Cost of RDS beside the wideband FM stereo path (--demod wfm --rds), in the shape of
profiles/wfm_timing.py: 60 s of a 10 MS/s int16 capture with five stereo stations that carry RDS, one station then five.
By device events, with and without RDS in the same process, alternating: the block demodulator (discriminator + stereo
matrix, and with RDS also iqa_rds_baseband + iqa_rds_clock), the RDS launches alone (the difference), the RDS finish
(timing, symbols, syndromes, the read-back and the group parser); then the file -> WAV wall time through
MultiChannelPipeline with and without rds.  Prints one JSON line (kept as profiles/rds_timing.json).
Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=rds``."""
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
from iq_to_audio_amd.decoders.rds import result_from  # noqa: E402
from iq_to_audio_amd.processing import ChannelBank, Channelizer, ProcessingPipeline, WfmDemod  # noqa: E402

_spec = importlib.util.spec_from_file_location("rds_model", ROOT / "tests" / "rds_model.py")
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

FS, SECS, FC = 10e6, 60.0, 100e6
OFFSETS = (1.0e6, -2.2e6, 2.6e6, -0.6e6, 3.4e6)  # station offsets (Hz); the first is the one-station run
PARENT = dict(source="profiles/wfm_timing.json (the parent commit's run)", wfm_block_ms={"1": 6.58, "5": 32.7})
REPEATS = 5


def make_capture(path: Path, block: int = 10_000_000) -> None:
    """int16 I/Q of five stereo stations (10 % pilot 30 ppm high, L = 1 kHz, R = 2.5 kHz, 4 % RDS: the model's group
    schedule) and noise, generated on the device."""
    n = int(FS * SECS)
    dev = torch.device("cuda", 0)
    e = torch.from_numpy(M.differential(M.bits_of(M.schedule(int(SECS * 1187.5 / 104) + 2)))).to(dev)
    phase = torch.zeros(len(OFFSETS), dtype=torch.float64, device=dev)
    k = 2 * math.pi * P.WFM_DEVIATION / FS
    g = torch.Generator(device=dev).manual_seed(7)

    def symbol(x):  # dsp_plan.rds_symbol on the device
        def s(v):
            return 4.0 * torch.sinc(4.0 * v)

        def h(v):
            return 0.5 * (s(v + 0.125) + s(v - 0.125))

        return h(x + 0.25) - h(x - 0.25)

    with path.open("wb") as fh:
        fh.write(b"\0" * 44)
        for lo in range(0, n, block):
            t = torch.arange(lo, min(lo + block, n), dtype=torch.float64, device=dev) / FS
            th = 2 * math.pi * P.WFM_PILOT_HZ * (1.0 + 30e-6) * t + 0.7
            lv, rv = 0.5 * torch.sin(2 * math.pi * 1000.0 * t), 0.5 * torch.sin(2 * math.pi * 2500.0 * t)
            psi = th / (32.0 * math.pi) - 0.37
            k0 = torch.floor(psi).to(torch.int64)
            bb = torch.zeros_like(t)
            for dk in range(-4, 5):
                kk = k0 + dk
                ok = (kk >= 0) & (kk < e.numel())
                a = torch.where(ok, 2 * e[kk.clamp(0, e.numel() - 1)] - 1, torch.zeros_like(kk)).to(torch.float64)
                bb += a * symbol(psi - kk.to(torch.float64) - 0.5)
            m = 0.45 * (lv + rv) + 0.45 * (lv - rv) * torch.sin(2 * th) + 0.1 * torch.sin(th) + 0.04 / 2.884 * bb * torch.cos(3 * th)
            x = torch.zeros(t.numel(), dtype=torch.complex128, device=dev)
            for i, f in enumerate(OFFSETS):
                ph = phase[i] + k * torch.cumsum(m, 0)
                x += 0.15 * torch.exp(1j * (2 * math.pi * f * t + ph))
                phase[i] = ph[-1]
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


def stage_times(path: Path, n_stations: int, rds: bool) -> dict:
    info = iqio.probe_capture(path)
    frames = iqio.map_frames(info)
    n = info.n_frames
    d, fs_ch = P.choose_decimation(FS, 480_000.0)
    taps = P.design_channel_filter(FS, 250_000.0, d)
    chans = [Channelizer(taps, sample_rate=FS, freq_offset=f, mix_sign=1, decimation=d) for f in OFFSETS[:n_stations]]
    for c in chans:
        c.plan_ahead()
    bank = ChannelBank(chans)
    dems = [WfmDemod(fs_ch, deemph_us=50.0, rds=rds) for _ in chans]
    n_dec = -(-n // d)
    planes = [torch.empty((2, n_dec), dtype=torch.float32, device="cuda") for _ in chans]
    block = ProcessingPipeline.block_frames_target
    t_wfm = 0.0
    pos = 0
    for lo in range(0, n, block):
        hi = min(lo + block, n)
        raw = torch.from_numpy(np.ascontiguousarray(frames[2 * lo : 2 * hi])).cuda()
        zs = bank.process(raw)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        m = int(zs[0].numel())
        for dem, z, pl in zip(dems, zs, planes):
            dem.process(z, np.array([0], dtype=np.int64), pl[:, pos : pos + m])
        e[1].record()
        torch.cuda.synchronize()
        t_wfm += e[0].elapsed_time(e[1])
        pos += m
    out = dict(stations=n_stations, rds=rds, block_ms=t_wfm, channel_rate=fs_ch)
    if rds:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        results = [result_from(dem.rds_core.finish()) for dem in dems]
        torch.cuda.synchronize()
        out["rds_finish_ms"] = (time.perf_counter() - t0) * 1e3
        out["stations_decoded"] = [r.line() for r in results]
        out["strength"] = [r.timing["strength"] for r in results]
    return out


def end_to_end(path: Path, n_stations: int, out_dir: Path, rds: bool) -> dict:
    cfgs = [A.ProcessingConfig(in_path=path, target_freq=FC + f, center_freq=FC, demod_mode="wfm", bandwidth=250_000.0,
                               fs_ch_target=480_000.0, deemph_us=50.0, output_path=out_dir / f"s{i}.wav")
            for i, f in enumerate(OFFSETS[:n_stations])]
    t0 = time.perf_counter()
    multi = A.MultiChannelPipeline(cfgs, rds=rds)
    multi.run()
    wall = time.perf_counter() - t0
    return dict(wall_s=wall, groups=[None if r is None else r.groups for r in multi.rds])


def med(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values), runs=len(values))


def main():
    torch.cuda.set_device(0)
    out = dict(capture=f"{SECS:.0f} s @ {FS / 1e6:.0f} MS/s cs16, five stereo stations with RDS",
               device=torch.cuda.get_device_name(0), repeats=REPEATS, parent=PARENT)
    with tempfile.TemporaryDirectory() as d:
        path = Path(d) / "fm_100000000Hz.wav"
        make_capture(path)
        out["stages"] = []
        for k in (1, 5):
            stage_times(path, k, False)  # warm-up: plans, tables, code objects
            stage_times(path, k, True)
            plain, with_rds, fin, last = [], [], [], None
            for _ in range(REPEATS):  # alternating
                plain.append(stage_times(path, k, False)["block_ms"])
                last = stage_times(path, k, True)
                with_rds.append(last["block_ms"])
                fin.append(last["rds_finish_ms"])
            out["stages"].append(dict(stations=k, channel_rate=last["channel_rate"], wfm_block_ms=med(plain),
                                      wfm_block_with_rds_ms=med(with_rds),
                                      rds_block_launches_ms=statistics.median(with_rds) - statistics.median(plain),
                                      rds_finish_ms=med(fin), decoded=last["stations_decoded"], strength=last["strength"]))
        out["end_to_end"] = []
        for k in (1, 5):
            end_to_end(path, k, Path(d), False)  # warm-up (page cache, pinned pools)
            end_to_end(path, k, Path(d), True)
            plain, with_rds, groups = [], [], None
            for _ in range(3):
                plain.append(end_to_end(path, k, Path(d), False)["wall_s"])
                r = end_to_end(path, k, Path(d), True)
                with_rds.append(r["wall_s"])
                groups = r["groups"]
            out["end_to_end"].append(dict(stations=k, wall_s=med(plain), wall_with_rds_s=med(with_rds),
                                          realtime_factor=SECS / statistics.median(plain),
                                          realtime_factor_with_rds=SECS / statistics.median(with_rds), groups=groups))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
