"""Cost of AIS beside the NFM path (--demod nfm --ais), in the shape of profiles/ax25_timing.py: 60 s
of a 10 MS/s int16 capture with five 25 kHz channels that each carry AIS bursts (a position report, a two-sentence static
report and a class-B report in turn, 0.1 s of carrier between them), one target then five, at 10e6 / 104 = 96 153.8 Hz.  By
device events, with and without AIS in the same process on the same build, alternating, as medians of five: the block
demodulator (iqa_demodulate, and with AIS also iqa_quadrature + iqa_ais_filter), the AIS launches alone (the difference),
the finish stage (symbol planes, frame walk, read-back, parser) split into device calls and host time; one more pass with
events around every entry point for the per-call split.  The yardstick is the unflagged run of the same build, which is the
parent's path.  Prints one JSON line (kept as profiles/ais_timing.json).  Every entry point here is one kernel
(iqa_ais_frames adds a 16-byte memset), so the per-call events are the per-kernel times.
Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=ais``."""
from __future__ import annotations

import importlib.util
import json
import math
import statistics
import sys
import tempfile
import time
from collections import defaultdict
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from iq_to_audio_amd import _native as N  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd import iqio  # noqa: E402
from iq_to_audio_amd.processing import ChannelBank, ChannelDemod, Channelizer, ProcessingPipeline  # noqa: E402

_spec = importlib.util.spec_from_file_location("ais_model", ROOT / "tests" / "ais_model.py")
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

FS, SECS, FC = 10e6, 60.0, 161.0e6
OFFSETS = (0.975e6, -2.2e6, 2.6e6, -0.6e6, 3.4e6)  # channel offsets (Hz); the first (161.975 MHz) is the one-target run
OVERSAMPLE = 8  # samples per bit of the host-made frequency trajectory the device interpolates
GAP_BITS = 960  # 0.1 s of carrier between bursts
REPEATS = 5


def messages() -> list:
    return [M.frame_bytes(M.dearmour(M.REFERENCE_PAYLOAD)),
            M.frame_bytes(M.static_data(235_087_654, imo=9_321_483, callsign="2ABC5", name="EVER GIVEN TWO", destination="ROTTERDAM")),
            M.frame_bytes(M.class_b_report(338_000_001, speed=61, lon=-70.25, lat=43.5, course=1805))]


def trajectory() -> tuple:
    """(frequency in units of the deviation at OVERSAMPLE samples per bit over the whole capture, bursts sent)."""
    total = int(SECS * M.BAUD)
    levels, sent = [], 0
    frames = messages()
    while True:
        burst = 2.0 * M.nrzi(M.burst_bits(frames[sent % len(frames)], first=sent & 1)).astype(np.float64) - 1.0
        if sum(x.size for x in levels) + burst.size + GAP_BITS > total:
            break
        levels += [burst, np.zeros(GAP_BITS)]
        sent += 1
    lv = np.concatenate(levels + [np.zeros(total + 8 - sum(x.size for x in levels))])
    sg = math.sqrt(math.log(2.0)) / (2.0 * math.pi * M.BT) * OVERSAMPLE
    k = np.arange(-4 * OVERSAMPLE, 4 * OVERSAMPLE + 1, dtype=np.float64)
    g = np.exp(-0.5 * (k / sg) ** 2)
    return np.convolve(np.repeat(lv, OVERSAMPLE), g / g.sum(), mode="same"), sent


def make_capture(path: Path, block: int = 10_000_000) -> int:
    """int16 I/Q of five GMSK channels (the same bursts on each) and noise, generated on the device: the frequency
    trajectory is interpolated linearly to the capture rate.  Returns the number of bursts per channel."""
    n = int(FS * SECS)
    dev = torch.device("cuda", 0)
    traj, sent = trajectory()
    table = torch.from_numpy(traj).to(dev)
    phase = torch.zeros((), dtype=torch.float64, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    with path.open("wb") as fh:
        fh.write(b"\0" * 44)
        for lo in range(0, n, block):
            idx = torch.arange(lo, min(lo + block, n), dtype=torch.float64, device=dev)
            t = idx / FS
            # sample k of the trajectory sits at the middle of its eighth of a bit
            pos = torch.clamp(idx * (M.BAUD * OVERSAMPLE / FS) - 0.5, min=0.0)
            i0 = torch.floor(pos).to(torch.int64)
            frac = pos - i0
            f = table[i0] * (1.0 - frac) + table[i0 + 1] * frac
            ph = phase + 2 * math.pi * M.DEVIATION / FS * torch.cumsum(f, 0)
            phase = torch.remainder(ph[-1], 2 * math.pi)
            x = torch.zeros(t.numel(), dtype=torch.complex128, device=dev)
            for off in OFFSETS:
                x += 0.15 * torch.exp(1j * (2 * math.pi * off * t + ph))
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
    return sent


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


def stage_times(path: Path, n_targets: int, ais: bool) -> dict:
    info = iqio.probe_capture(path)
    frames = iqio.map_frames(info)
    n = info.n_frames
    d, fs_ch = P.choose_decimation(FS, 96_000.0)
    taps = P.design_channel_filter(FS, 25_000.0, d)
    chans = [Channelizer(taps, sample_rate=FS, freq_offset=f, mix_sign=1, decimation=d) for f in OFFSETS[:n_targets]]
    for c in chans:
        c.plan_ahead()
    bank = ChannelBank(chans)
    dems = [ChannelDemod("nfm", fs_ch, deemph_us=300.0, agc_enabled=True, ais=ais) for _ in chans]
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
    out = dict(targets=n_targets, ais=ais, block_ms=t_blk, channel_rate=fs_ch, blocks=blocks)
    if ais:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with CallTimes(("iqa_ais_symbols", "iqa_ais_frames")) as ct:
            results = [dem.side_result("ais", frequency=FC + f) for dem, f in zip(dems, OFFSETS)]
            torch.cuda.synchronize()
            out["finish_ms"] = (time.perf_counter() - t0) * 1e3
        out["finish_device_ms"] = sum(ct.ms.values())
        out["finish_host_ms"] = out["finish_ms"] - out["finish_device_ms"]
        out["messages"] = [0 if r is None else len(r.messages) for r in results]
        out["hits"] = [None if r is None else [min(m.hits for m in r.messages), max(m.hits for m in r.messages)] for r in results]
        out["candidates"] = [None if r is None else [r.candidates, r.crc_ok] for r in results]
        out["stored_bytes_per_sample"] = 4
    return out


def med(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values), runs=len(values))


def main():
    torch.cuda.set_device(0)
    out = dict(capture=f"{SECS:.0f} s @ {FS / 1e6:.0f} MS/s cs16, five GMSK channels with AIS bursts", device=torch.cuda.get_device_name(0),
               repeats=REPEATS, yardstick="the unflagged run of the same build")
    with tempfile.TemporaryDirectory() as d:
        path = Path(d) / "marine_161000000Hz.wav"
        out["bursts_sent"] = make_capture(path)
        out["stages"] = []
        for k in (1, 5):
            stage_times(path, k, False)  # warm-up: plans, tables, code objects
            stage_times(path, k, True)
            plain, with_ais, fin, fin_dev, fin_host, last = [], [], [], [], [], None
            for _ in range(REPEATS):  # alternating
                plain.append(stage_times(path, k, False)["block_ms"])
                last = stage_times(path, k, True)
                with_ais.append(last["block_ms"])
                fin.append(last["finish_ms"])
                fin_dev.append(last["finish_device_ms"])
                fin_host.append(last["finish_host_ms"])
            with CallTimes(("iqa_ais_", "iqa_quadrature", "iqa_demodulate")) as ct:
                stage_times(path, k, True)
            out["stages"].append(dict(targets=k, channel_rate=last["channel_rate"], blocks=last["blocks"], nfm_block_ms=med(plain),
                                      nfm_block_with_ais_ms=med(with_ais),
                                      ais_block_launches_ms=statistics.median(with_ais) - statistics.median(plain),
                                      ais_finish_ms=med(fin), ais_finish_device_ms=med(fin_dev), ais_finish_host_ms=med(fin_host),
                                      messages=last["messages"], hits=last["hits"], candidates_crc_ok=last["candidates"],
                                      stored_bytes_per_sample=last["stored_bytes_per_sample"],
                                      per_call_ms=dict(ct.ms), per_call_count=dict(ct.counts)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
