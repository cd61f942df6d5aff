"""Time of the wideband FM stereo path (--demod wfm): 60 s of a 10 MS/s int16 capture with one
stereo station, then five.  By device events: the channelizer (one ChannelBank pass per 64 Mi-frame block), the wfm
block demodulator (discriminator + stereo matrix kernel), the tail (stereo decision, matrix, de-emphasis, clip, 48 kHz
PCM16 with its copy to the host); then the file -> WAV run through MultiChannelPipeline, as a realtime factor.
Prints one JSON line.  Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=wfm``."""
from __future__ import annotations

import json
import math
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
from iq_to_audio_amd.processing import ChannelBank, Channelizer, ProcessingPipeline, WfmDemod  # noqa: E402

FS, SECS, FC = 10e6, 60.0, 100e6
OFFSETS = (1.0e6, -2.2e6, 2.6e6, -0.6e6, 3.4e6)  # station offsets (Hz); the first is the one-station run


def make_capture(path: Path, block: int = 10_000_000) -> None:
    """int16 I/Q of five stereo stations (10 % pilot, L = 1 kHz, R = 2.5 kHz) and noise, generated on the device."""
    n = int(FS * SECS)
    dev = torch.device("cuda", 0)
    phase = torch.zeros(len(OFFSETS), dtype=torch.float64, device=dev)
    k = 2 * math.pi * P.WFM_DEVIATION / FS
    g = torch.Generator(device=dev).manual_seed(7)
    with path.open("wb") as fh:
        fh.write(b"\0" * 44)
        for lo in range(0, n, block):
            t = torch.arange(lo, min(lo + block, n), dtype=torch.float64, device=dev) / FS
            th = 2 * math.pi * P.WFM_PILOT_HZ * t
            lv, rv = 0.5 * torch.sin(2 * math.pi * 1000.0 * t), 0.5 * torch.sin(2 * math.pi * 2500.0 * t)
            m = 0.45 * (lv + rv) + 0.45 * (lv - rv) * torch.sin(2 * th) + 0.1 * torch.sin(th)
            x = torch.zeros(t.numel(), dtype=torch.complex128, device=dev)
            for i, f in enumerate(OFFSETS):
                ph = phase[i] + k * torch.cumsum(m, 0)
                x += 0.15 * torch.exp(1j * (2 * math.pi * f * t + ph))
                phase[i] = ph[-1]
            x += 0.002 * torch.complex(torch.randn(t.numel(), generator=g, device=dev, dtype=torch.float64),
                                       torch.randn(t.numel(), generator=g, device=dev, dtype=torch.float64))
            iq = torch.stack([x.real, x.imag], 1).clamp(-0.999, 0.999).mul(32767.0).round().to(torch.int16)
            fh.write(iq.cpu().numpy().tobytes())
    # the header: the project's own writer on an empty stub, with the data size patched in
    data = path.stat().st_size - 44
    stub = path.with_suffix(".hdr.wav")
    iqio.write_wav_iq(stub, np.zeros(0, np.int16), int(FS), "s16")
    head = bytearray(stub.read_bytes()[:44])
    head[4:8] = (36 + data).to_bytes(4, "little")
    head[40:44] = data.to_bytes(4, "little")
    with path.open("r+b") as fh:
        fh.write(bytes(head))
    stub.unlink()


def stage_times(path: Path, n_stations: int) -> dict:
    info = iqio.probe_capture(path)
    frames = iqio.map_frames(info)
    n = info.n_frames
    d, fs_ch = P.choose_decimation(FS, 480_000.0)
    taps = P.design_channel_filter(FS, 250_000.0, d)
    chans = [Channelizer(taps, sample_rate=FS, freq_offset=f, mix_sign=1, decimation=d) for f in OFFSETS[:n_stations]]
    for c in chans:
        c.plan_ahead()
    bank = ChannelBank(chans)
    dems = [WfmDemod(fs_ch, deemph_us=50.0) for _ in chans]
    n_dec = -(-n // d)
    planes = [torch.empty((2, n_dec), dtype=torch.float32, device="cuda") for _ in chans]
    block = ProcessingPipeline.block_frames_target
    t_chan = t_wfm = 0.0
    pos = 0
    for lo in range(0, n, block):
        hi = min(lo + block, n)
        raw = torch.from_numpy(np.ascontiguousarray(frames[2 * lo : 2 * hi])).cuda()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        zs = bank.process(raw)
        e[1].record()
        m = int(zs[0].numel())
        for dem, z, pl in zip(dems, zs, planes):
            dem.process(z, np.array([0], dtype=np.int64), pl[:, pos : pos + m])
        e[2].record()
        torch.cuda.synchronize()
        t_chan += e[0].elapsed_time(e[1])
        t_wfm += e[1].elapsed_time(e[2])
        pos += m
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stereo = []
    for dem, pl in zip(dems, planes):
        dem.finish(pl[:, :pos])
        stereo.append(dem.stereo)
    torch.cuda.synchronize()
    t_tail = (time.perf_counter() - t0) * 1e3
    return dict(stations=n_stations, channelizer_ms=t_chan, wfm_block_ms=t_wfm, tail_ms=t_tail, stereo=stereo,
                channel_rate=fs_ch, kernel=chans[0]._kernel.last_kernel)


def end_to_end(path: Path, n_stations: int, out_dir: Path) -> dict:
    cfgs = [A.ProcessingConfig(in_path=path, target_freq=FC + f, center_freq=FC, demod_mode="wfm", bandwidth=250_000.0,
                               fs_ch_target=480_000.0, deemph_us=50.0, output_path=out_dir / f"s{i}.wav")
            for i, f in enumerate(OFFSETS[:n_stations])]
    t0 = time.perf_counter()
    multi = A.MultiChannelPipeline(cfgs)
    multi.run()
    wall = time.perf_counter() - t0
    return dict(stations=n_stations, wall_s=wall, realtime_factor=SECS / wall, stereo=multi.wfm_stereo)


def main():
    torch.cuda.set_device(0)
    out = dict(capture=f"{SECS:.0f} s @ {FS / 1e6:.0f} MS/s cs16", device=torch.cuda.get_device_name(0))
    with tempfile.TemporaryDirectory() as d:
        path = Path(d) / "fm_100000000Hz.wav"
        make_capture(path)
        stage_times(path, 1)  # warm-up: plans, tables, code objects
        out["stages"] = [stage_times(path, k) for k in (1, 5)]
        end_to_end(path, 1, Path(d))  # warm-up (page cache, pinned pools)
        out["end_to_end"] = [end_to_end(path, k, Path(d)) for k in (1, 5)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
