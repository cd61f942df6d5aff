"""Cost of POCSAG beside the NFM path (--demod nfm --pocsag), in the shape of profiles/rds_timing.py:
60 s of a 10 MS/s int16 capture with five 25 kHz channels that carry pager traffic (1200, 512, 2400, 1200, 512 baud, back
to back transmissions), one target then five.  By device events, with and without POCSAG in the same process, alternating:
the block demodulator (iqa_demodulate, and with POCSAG also iqa_quadrature + iqa_pocsag_integrate), the POCSAG launches
alone (the difference), the finish stage (sync search per baud, codewords, read-back, parser); one more pass with events
around every POCSAG entry point for the per-call split; then the file -> WAV wall time through MultiChannelPipeline with
and without pocsag.  Prints one JSON line (kept as profiles/pocsag_timing.json).
Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=pocsag``."""
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

import iq_to_audio_amd as A  # noqa: E402
from iq_to_audio_amd import _native as N  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd import iqio  # noqa: E402
from iq_to_audio_amd.processing import ChannelBank, ChannelDemod, Channelizer, ProcessingPipeline  # noqa: E402

_spec = importlib.util.spec_from_file_location("pocsag_model", ROOT / "tests" / "pocsag_model.py")
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

FS, SECS, FC = 10e6, 60.0, 150e6
OFFSETS = (1.0e6, -2.2e6, 2.6e6, -0.6e6, 3.4e6)  # channel offsets (Hz); the first is the one-target run
BAUDS = (1200, 512, 2400, 1200, 512)
MESSAGES = [(1234567, 3, "Pump 4 pressure low, call 0171 5550123"), (424242, 0, "0123456789"), (77, 1, "ok")]
PARENT = dict(source="DESIGN.md section 6 (the parent commit's NFM numbers)")
REPEATS = 5


def make_capture(path: Path, block: int = 10_000_000) -> list:
    """int16 I/Q of five 2-FSK channels (+-4.5 kHz, transmissions back to back with 0.25 s of bare carrier between them) and
    noise, generated on the device.  Returns the number of transmissions per channel."""
    n = int(FS * SECS)
    dev = torch.device("cuda", 0)
    one = M.transmission_bits(MESSAGES)
    sent, bit_tables = [], []
    for baud in BAUDS:
        gap = np.zeros(int(0.25 * baud), dtype=np.uint8)
        reps = int(SECS * baud // (one.size + gap.size))
        sent.append(reps)
        bits = np.concatenate([np.concatenate([one, gap])] * reps + [np.zeros(int(SECS * baud) + 8, dtype=np.uint8)])
        bit_tables.append(torch.from_numpy(bits[: int(SECS * baud) + 8].astype(np.int64)).to(dev))
    phase = torch.zeros(len(OFFSETS), dtype=torch.float64, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    with path.open("wb") as fh:
        fh.write(b"\0" * 44)
        for lo in range(0, n, block):
            idx = torch.arange(lo, min(lo + block, n), dtype=torch.float64, device=dev)
            t = idx / FS
            x = torch.zeros(t.numel(), dtype=torch.complex128, device=dev)
            for i, (f, baud) in enumerate(zip(OFFSETS, BAUDS)):
                bit = bit_tables[i][torch.floor(idx * (baud / FS)).to(torch.int64)]
                dev_hz = torch.where(bit == 1, -M.DEVIATION, M.DEVIATION)
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


def stage_times(path: Path, n_targets: int, pocsag: bool) -> dict:
    info = iqio.probe_capture(path)
    frames = iqio.map_frames(info)
    n = info.n_frames
    d, fs_ch = P.choose_decimation(FS, 96_000.0)
    taps = P.design_channel_filter(FS, 12_500.0, d)
    chans = [Channelizer(taps, sample_rate=FS, freq_offset=f, mix_sign=1, decimation=d) for f in OFFSETS[:n_targets]]
    for c in chans:
        c.plan_ahead()
    bank = ChannelBank(chans)
    dems = [ChannelDemod("nfm", fs_ch, deemph_us=300.0, agc_enabled=True, pocsag=pocsag) for _ in chans]
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
    out = dict(targets=n_targets, pocsag=pocsag, block_ms=t_blk, channel_rate=fs_ch, blocks=blocks)
    if pocsag:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        results = [dem.side_result("pocsag") for dem in dems]
        torch.cuda.synchronize()
        out["finish_ms"] = (time.perf_counter() - t0) * 1e3
        out["messages"] = [0 if r is None else len(r.messages) for r in results]
        out["syncs"] = [None if r is None else r.syncs for r in results]
        out["codewords"] = [None if r is None else r.codewords for r in results]
    return out


def end_to_end(path: Path, n_targets: int, out_dir: Path, pocsag: bool) -> dict:
    cfgs = [A.ProcessingConfig(in_path=path, target_freq=FC + f, center_freq=FC, demod_mode="nfm", output_path=out_dir / f"t{i}.wav")
            for i, f in enumerate(OFFSETS[:n_targets])]
    t0 = time.perf_counter()
    multi = A.MultiChannelPipeline(cfgs, pocsag=pocsag)
    multi.run()
    wall = time.perf_counter() - t0
    return dict(wall_s=wall, messages=[None if r is None else len(r.messages) for r in multi.pocsag])


def med(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values), runs=len(values))


def main():
    torch.cuda.set_device(0)
    out = dict(capture=f"{SECS:.0f} s @ {FS / 1e6:.0f} MS/s cs16, five 2-FSK pager channels {BAUDS}",
               device=torch.cuda.get_device_name(0), repeats=REPEATS, parent=PARENT)
    with tempfile.TemporaryDirectory() as d:
        path = Path(d) / "pager_150000000Hz.wav"
        out["transmissions_sent"] = make_capture(path)
        out["messages_per_transmission"] = len(MESSAGES)
        out["stages"] = []
        for k in (1, 5):
            stage_times(path, k, False)  # warm-up: plans, tables, code objects
            stage_times(path, k, True)
            plain, with_pg, fin, last = [], [], [], None
            for _ in range(REPEATS):  # alternating
                plain.append(stage_times(path, k, False)["block_ms"])
                last = stage_times(path, k, True)
                with_pg.append(last["block_ms"])
                fin.append(last["finish_ms"])
            with CallTimes(("iqa_pocsag_", "iqa_quadrature", "iqa_demodulate")) as ct:
                stage_times(path, k, True)
            out["stages"].append(dict(targets=k, channel_rate=last["channel_rate"], blocks=last["blocks"], nfm_block_ms=med(plain),
                                      nfm_block_with_pocsag_ms=med(with_pg),
                                      pocsag_block_launches_ms=statistics.median(with_pg) - statistics.median(plain),
                                      pocsag_finish_ms=med(fin), messages=last["messages"], syncs=last["syncs"],
                                      codewords=last["codewords"], per_call_ms=dict(ct.ms), per_call_count=dict(ct.counts)))
        out["end_to_end"] = []
        for k in (1, 5):
            end_to_end(path, k, Path(d), False)  # warm-up (page cache, pinned pools)
            end_to_end(path, k, Path(d), True)
            plain, with_pg, messages = [], [], None
            for _ in range(REPEATS):
                plain.append(end_to_end(path, k, Path(d), False)["wall_s"])
                r = end_to_end(path, k, Path(d), True)
                with_pg.append(r["wall_s"])
                messages = r["messages"]
            out["end_to_end"].append(dict(targets=k, wall_s=med(plain), wall_with_pocsag_s=med(with_pg),
                                          realtime_factor=SECS / statistics.median(plain),
                                          realtime_factor_with_pocsag=SECS / statistics.median(with_pg), messages=messages))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
