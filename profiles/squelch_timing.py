"""Device and end-to-end time of the squelch chain (--audio-post): one 60-s 48 kHz mono file, and a 40-file batch of
60-s 48 kHz files through process_audio_batch.  Prints one JSON line.  Launch count: run under
``rocprofv3 --kernel-trace --stats -- python profiles/squelch_timing.py --once``."""
from __future__ import annotations

import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

import iq_to_audio_amd.squelch as S  # noqa: E402
from iq_to_audio_amd import iqio  # noqa: E402


def signal(rate, secs, seed):
    rng = np.random.default_rng(seed)
    n = int(rate * secs)
    x = rng.standard_normal(n).astype(np.float32) * np.float32(0.003)
    t = np.arange(n) / rate
    for _ in range(60):
        a = int(rng.integers(0, n - 100_000))
        ln = int(rng.integers(2_000, 100_000))
        x[a:a + ln] += (0.3 * np.sin(2 * np.pi * 700 * t[a:a + ln])).astype(np.float32)
    return x


def device_ms(x_dev, cfg, reps):
    S.apply_squelch(x_dev, 48000.0, cfg)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        S.squelch_device([(x_dev, 48000.0)], cfg)  # includes the result read-back (one sync)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    once = "--once" in sys.argv
    torch.cuda.set_device(0)
    out = {}
    x = signal(48000, 60.0, 0)
    x_dev = torch.from_numpy(x).cuda()
    for method in ("adaptive", "static", "transient"):
        out[f"one_file_{method}_ms"] = device_ms(x_dev, S.SquelchConfig(method=method), 1 if once else 20)
    if not once:
        files = [signal(48000, 60.0, k) for k in range(40)]
        batch_dev = [(torch.from_numpy(f).cuda(), 48000.0) for f in files]
        S.squelch_device(batch_dev, S.SquelchConfig())
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        S.squelch_device(batch_dev, S.SquelchConfig())
        b.record()
        torch.cuda.synchronize()
        out["batch40_device_ms"] = a.elapsed_time(b)
        with tempfile.TemporaryDirectory() as d:
            paths = []
            for k, f in enumerate(files):
                p = Path(d) / f"ch{k:02d}.wav"
                iqio.write_wav_audio(p, f, 48000, "PCM_16")
                paths.append(p)
            opts = S.AudioPostOptions(config=S.SquelchConfig())
            t0 = time.perf_counter()
            summary = S.process_audio_batch(paths, opts)
            out["batch40_end_to_end_s"] = time.perf_counter() - t0
            out["batch40_files_ok"] = summary.processed
    print(json.dumps(out))


if __name__ == "__main__":
    main()
