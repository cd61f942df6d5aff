"""Cost of ACARS beside the AM path (--demod am --acars), in the shape of profiles/ax25_timing.py: 30 s
of a 10 MS/s int16 capture with five AM airband channels (transmissions of two blocks back to back on a carrier that stays
keyed), one target then five.  By device events, with and without ACARS in the same process, alternating: the block
demodulator (iqa_demodulate, and with ACARS also iqa_envelope into the decoder's store), the ACARS launch alone (the
difference), the finish stage (maximum, detector, symbol streams, frame walk, read-backs, parser) split into device calls and
host time; one more pass with events around every entry point for the per-call split; then the file -> WAV wall time through
MultiChannelPipeline with and without acars.  The yardstick is the same run without the flag on the same build: the parent's
AM path.  Prints one JSON line (kept as profiles/acars_timing.json).  Every entry point here is one kernel (iqa_acars_max and
iqa_acars_frames add a small memset), so the per-call events are the per-kernel times.
Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=acars``."""
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

_spec = importlib.util.spec_from_file_location("acars_model", ROOT / "tests" / "acars_model.py")
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

FS, SECS, FC = 10e6, 30.0, 131.5e6
OFFSETS = (1.0e6, -2.2e6, 2.6e6, -0.6e6, 3.4e6)  # channel offsets (Hz); the first is the one-target run
DEPTH = 0.5
REPEATS = 5


def make_capture(path: Path, block: int = 10_000_000) -> int:
    """int16 I/Q of five AM channels carrying the same ACARS transmissions (0.2 s of unmodulated carrier between them) and
    noise, generated on the device.  Returns the number of blocks sent per channel."""
    n = int(FS * SECS)
    dev = torch.device("cuda", 0)
    bodies = [M.body_bytes(**M.FIRST), M.body_bytes(**M.SECOND, etb=True)]
    one = np.concatenate([M.transitions(M.bits_of(M.message_bytes(b))) for b in bodies])
    gap = np.full(int(0.2 * M.BAUD), 2, dtype=np.uint8)  # 2: no modulation
    reps = int(SECS * M.BAUD // (one.size + gap.size))
    sym = np.concatenate([np.concatenate([one, gap])] * reps + [np.full(int(SECS * M.BAUD) + 8, 2, dtype=np.uint8)])
    table = torch.from_numpy(sym[: int(SECS * M.BAUD) + 8].astype(np.int64)).to(dev)
    audio_phase = torch.zeros((), dtype=torch.float64, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    with path.open("wb") as fh:
        fh.write(b"\0" * 44)
        for lo in range(0, n, block):
            idx = torch.arange(lo, min(lo + block, n), dtype=torch.float64, device=dev)
            t = idx / FS
            s = table[torch.floor(idx * (M.BAUD / FS)).to(torch.int64)]
            aph = audio_phase + 2 * math.pi / FS * torch.cumsum(torch.where(s == 1, 2400.0, 1200.0).to(torch.float64), 0)
            audio_phase = torch.remainder(aph[-1], 2 * math.pi)
            env = 1.0 + DEPTH * torch.where(s == 2, torch.zeros_like(aph), torch.cos(aph))
            x = torch.zeros(t.numel(), dtype=torch.complex128, device=dev)
            for f in OFFSETS:
                x += 0.12 * env * torch.exp(1j * (2 * math.pi * f * t))
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
    return reps * len(bodies)


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


def stage_times(path: Path, n_targets: int, acars: bool) -> dict:
    info = iqio.probe_capture(path)
    frames = iqio.map_frames(info)
    n = info.n_frames
    d, fs_ch = P.choose_decimation(FS, 96_000.0)
    taps = P.design_channel_filter(FS, 12_500.0, d)
    chans = [Channelizer(taps, sample_rate=FS, freq_offset=f, mix_sign=1, decimation=d) for f in OFFSETS[:n_targets]]
    for c in chans:
        c.plan_ahead()
    bank = ChannelBank(chans)
    dems = [ChannelDemod("am", fs_ch, deemph_us=300.0, agc_enabled=True, acars=acars) for _ in chans]
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
    out = dict(targets=n_targets, acars=acars, block_ms=t_blk, channel_rate=fs_ch, blocks=blocks)
    if acars:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with CallTimes(("iqa_acars_",)) as ct:
            results = [dem.side_result("acars") for dem in dems]
            torch.cuda.synchronize()
            out["finish_ms"] = (time.perf_counter() - t0) * 1e3
        out["finish_device_ms"] = sum(ct.ms.values())
        out["finish_host_ms"] = out["finish_ms"] - out["finish_device_ms"]
        out["finish_per_call_ms"] = dict(ct.ms)
        out["messages"] = [0 if r is None else len(r.messages) for r in results]
        out["hits"] = [None if r is None else [min(m.hits for m in r.messages), max(m.hits for m in r.messages)] for r in results]
        out["candidates"] = [None if r is None else [r.candidates, r.crc_ok] for r in results]
        out["stored_bytes_per_sample"] = 4
    return out


def end_to_end(path: Path, n_targets: int, out_dir: Path, acars: bool) -> dict:
    cfgs = [A.ProcessingConfig(in_path=path, target_freq=FC + f, center_freq=FC, demod_mode="am", output_path=out_dir / f"t{i}.wav")
            for i, f in enumerate(OFFSETS[:n_targets])]
    t0 = time.perf_counter()
    multi = A.MultiChannelPipeline(cfgs, acars=acars)
    multi.run()
    wall = time.perf_counter() - t0
    return dict(wall_s=wall, messages=[None if r is None else len(r.messages) for r in multi.acars])


def med(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values), runs=len(values))


def main():
    torch.cuda.set_device(0)
    out = dict(capture=f"{SECS:.0f} s @ {FS / 1e6:.0f} MS/s cs16, five AM channels with ACARS at depth {DEPTH}",
               device=torch.cuda.get_device_name(0), repeats=REPEATS, yardstick="the same run without acars, same build")
    with tempfile.TemporaryDirectory() as d:
        path = Path(d) / "airband_131500000Hz.wav"
        out["blocks_sent_per_channel"] = make_capture(path)
        out["stages"] = []
        for k in (1, 5):
            stage_times(path, k, False)  # warm-up: plans, tables, code objects
            stage_times(path, k, True)
            plain, with_ac, fin, fin_dev, fin_host, last = [], [], [], [], [], None
            for _ in range(REPEATS):  # alternating
                plain.append(stage_times(path, k, False)["block_ms"])
                last = stage_times(path, k, True)
                with_ac.append(last["block_ms"])
                fin.append(last["finish_ms"])
                fin_dev.append(last["finish_device_ms"])
                fin_host.append(last["finish_host_ms"])
            with CallTimes(("iqa_acars_", "iqa_envelope", "iqa_demodulate")) as ct:
                stage_times(path, k, True)
            out["stages"].append(dict(targets=k, channel_rate=last["channel_rate"], blocks=last["blocks"], am_block_ms=med(plain),
                                      am_block_with_acars_ms=med(with_ac),
                                      acars_block_launches_ms=statistics.median(with_ac) - statistics.median(plain),
                                      acars_finish_ms=med(fin), acars_finish_device_ms=med(fin_dev), acars_finish_host_ms=med(fin_host),
                                      messages=last["messages"], hits=last["hits"], candidates_crc_ok=last["candidates"],
                                      stored_bytes_per_sample=last["stored_bytes_per_sample"],
                                      per_call_ms=dict(ct.ms), per_call_count=dict(ct.counts)))
        out["end_to_end"] = []
        for k in (1, 5):
            end_to_end(path, k, Path(d), False)  # warm-up (page cache, pinned pools)
            end_to_end(path, k, Path(d), True)
            plain, with_ac, messages = [], [], None
            for _ in range(REPEATS):
                plain.append(end_to_end(path, k, Path(d), False)["wall_s"])
                r = end_to_end(path, k, Path(d), True)
                with_ac.append(r["wall_s"])
                messages = r["messages"]
            out["end_to_end"].append(dict(targets=k, wall_s=med(plain), wall_with_acars_s=med(with_ac),
                                          realtime_factor=SECS / statistics.median(plain),
                                          realtime_factor_with_acars=SECS / statistics.median(with_ac), messages=messages))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
