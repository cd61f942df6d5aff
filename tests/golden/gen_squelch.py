"""Regenerate tests/golden/squelch.npz and tests/golden/squelch_edges.npz from the reference's squelch module (CPU only).

    python tests/golden/gen_squelch.py /path/to/iq-to-audio/src [squelch|squelch_edges|all] [out directory]

``squelch`` holds nine cases at audio rates and default hold and fade; ``squelch_edges`` holds short cases at 1000 Hz,
where a configuration's seconds are exact sample counts, at the edges the first file cannot reach (window 1 and n, the
int8 wrap at hold 127 / 128, fade 1 and beyond n, three channels, a float input above full scale, percentile 0 and 1,
a one-sample transient window, a burst at sample 0 with no trim padding).  A case whose ``{name}__kind`` is ``"f32"``
stores its input as ``{name}__f32`` (float32 [n, C]); every other case stores PCM16 byte planes.

Imports ``iq_to_audio.squelch`` from the given source tree with ``soundfile`` stubbed (no file I/O is used) and
records, per case: the PCM16 input (as high and low byte planes, ``pcm = hi << 8 | lo``), the parameters (JSON), the noise floor and threshold, the trim bounds, the
pre-dilation mask (np.packbits) and the gain (float32).  Asserts that input[start:stop] * gain reproduces
apply_squelch's output bit for bit.  Needs numpy (and scipy, which the reference imports)."""
from __future__ import annotations

import importlib.util
import json
import sys
import types
from pathlib import Path

import numpy as np


def load_reference(src: Path):
    sys.modules.setdefault("soundfile", types.ModuleType("soundfile"))
    spec = importlib.util.spec_from_file_location("ref_squelch", src / "iq_to_audio" / "squelch.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def bursts(rate: int, secs: float, channels: int, spans, noise: float, seed: int) -> np.ndarray:
    """Noise with sine bursts at (start s, length s, amplitude) -> PCM16 [n, channels].  The bursts are on a grid of
    256 LSB, so the low byte carries only the noise (a smaller fixture)."""
    rng = np.random.default_rng(seed)
    n = int(rate * secs)
    x = np.rint(rng.standard_normal((n, channels)) * noise * 32768.0)
    t = np.arange(n) / rate
    for k, (s0, ln, amp) in enumerate(spans):
        a, b = int(s0 * rate), int((s0 + ln) * rate)
        for c in range(channels):
            x[a:b, c] += 256.0 * np.rint(amp * 128.0 * np.sin(2 * np.pi * (400 + 150 * k + 37 * c) * t[a:b]))
    return np.clip(x, -32768, 32767).astype(np.int16)


CASES = [
    # name, rate, secs, channels, bursts, noise, config overrides.  Short, quiet cases keep the fixture small; windows:
    # 1920 at 48 kHz and 640 at 16 kHz (even), 441 at 11 025 Hz (odd).
    ("adaptive_mono_48k", 48000, 1.0, 1, [(0.25, 0.2, 0.3), (0.6, 0.03, 0.2), (0.8, 0.15, 0.5)], 0.00006, {}),
    ("adaptive_stereo_11k", 11025, 2.0, 2, [(0.4, 0.4, 0.25), (1.3, 0.2, 0.4)], 0.00006, {}),
    ("static_mono_16k_notrim", 16000, 1.2, 1, [(0.4, 0.3, 0.3)], 0.00006, {"method": "static", "trim_silence": False}),
    ("static_stereo_11k_manual", 11025, 1.5, 2, [(0.5, 0.4, 0.3)], 0.00006,
     {"method": "static", "auto_noise_floor": False, "manual_noise_floor_db": -45.0}),
    ("transient_mono_16k", 16000, 1.5, 1, [(0.4, 0.005, 0.6), (0.8, 0.008, 0.5), (1.1, 0.2, 0.3)], 0.00006,
     {"method": "transient"}),
    ("transient_stereo_11k_nofade", 11025, 1.5, 2, [(0.5, 0.006, 0.6), (1.0, 0.004, 0.5)], 0.00006,
     {"method": "transient", "fade_seconds": 0.0}),
    ("adaptive_all_noise", 11025, 1.0, 1, [], 0.0002, {}),
    ("static_trims_to_empty", 11025, 1.0, 1, [], 0.0002,
     {"method": "static", "auto_noise_floor": False, "manual_noise_floor_db": -10.0}),
    ("adaptive_fade0_short_bursts", 16000, 1.2, 2, [(0.2, 0.004, 0.5), (0.7, 0.01, 0.4)], 0.00006,
     {"fade_seconds": 0.0, "hold_seconds": 0.05}),
]


def bursts_f32(rate: int, secs: float, channels: int, spans, noise: float, seed: int) -> np.ndarray:
    """The same as float32 samples, not clipped: amplitudes above 1.0 stay (a FLOAT WAV above full scale)."""
    rng = np.random.default_rng(seed)
    n = int(rate * secs)
    x = rng.standard_normal((n, channels)) * noise
    t = np.arange(n) / rate
    for k, (s0, ln, amp) in enumerate(spans):
        a, b = int(s0 * rate), int((s0 + ln) * rate)
        for c in range(channels):
            x[a:b, c] += amp * np.sin(2 * np.pi * (40 + 15 * k + 3 * c) * t[a:b] + 0.5)
    return x.astype(np.float32)


_STATIC = {"method": "static", "auto_noise_floor": False, "manual_noise_floor_db": -45.0, "window_seconds": 0.008,
           "fade_seconds": 0.005}

EDGE_CASES = [
    # all at 1000 Hz: seconds * 1000 are the sample counts.  (name, rate, secs, channels, bursts, noise, overrides)
    ("hold_127", 1000, 3.0, 1, [(0.5, 0.3, 0.3), (1.5, 0.1, 0.3), (2.2, 0.129, 0.3)], 0.00006, dict(_STATIC, hold_seconds=0.127)),
    ("hold_128", 1000, 3.0, 1, [(0.5, 0.3, 0.3), (1.5, 0.1, 0.3), (2.2, 0.129, 0.3)], 0.00006, dict(_STATIC, hold_seconds=0.128)),
    ("fade_beyond_n", 1000, 1.2, 1, [(0.3, 0.2, 0.3)], 0.00006, dict(_STATIC, hold_seconds=0.02, fade_seconds=1.5)),
    ("fade_1", 1000, 1.2, 2, [(0.3, 0.2, 0.3), (0.9, 0.05, 0.2)], 0.00006, dict(_STATIC, hold_seconds=0.02, fade_seconds=0.001)),
    ("window_n", 1000, 2.0, 1, [(0.7, 0.5, 0.4)], 0.00006,
     {"method": "static", "window_seconds": 2.0, "threshold_margin_db": 0.5, "hold_seconds": 0.05}),
    ("window_1", 1000, 1.5, 1, [(0.4, 0.3, 0.3)], 0.0002, {"window_seconds": 0.001, "hold_seconds": 0.03}),
    ("three_channels", 1000, 2.0, 3, [(0.5, 0.4, 0.3), (1.4, 0.2, 0.5)], 0.00006, {}),
    ("float_above_full_scale", 1000, 1.5, 2, [(0.3, 0.3, 4.0), (0.9, 0.2, 0.5)], 0.0005, {"kind": "f32"}),
    ("percentile_0", 1000, 1.5, 1, [(0.5, 0.4, 0.3)], 0.0002, {"method": "static", "noise_floor_percentile": 0.0}),
    ("percentile_1", 1000, 1.5, 1, [(0.5, 0.4, 0.3)], 0.0002,
     {"method": "static", "noise_floor_percentile": 1.0, "threshold_margin_db": -3.0}),
    ("transient_short_1", 1000, 2.0, 1, [(0.5, 0.004, 0.6), (1.2, 0.003, 0.5), (1.6, 0.2, 0.3)], 0.00006,
     {"method": "transient", "transient_window_seconds": 0.001}),
    ("burst_at_0_no_padding", 1000, 1.5, 1, [(0.0, 0.3, 0.3), (1.3, 0.2, 0.3)], 0.00006,
     dict(_STATIC, hold_seconds=0.02, trim_lead_seconds=0.0, trim_trail_seconds=0.0)),
]

SETS = {"squelch": CASES, "squelch_edges": EDGE_CASES}


def main() -> None:
    src = Path(sys.argv[1])
    which = sys.argv[2] if len(sys.argv) > 2 else "all"
    out_dir = Path(sys.argv[3]) if len(sys.argv) > 3 else Path(__file__).parent
    ref = load_reference(src)
    for set_name, cases in SETS.items():
        if which in ("all", set_name):
            write_set(ref, cases, out_dir / f"{set_name}.npz")


def write_set(ref, cases, out: Path) -> None:
    blob = {}
    for k, (name, rate, secs, ch, spans, noise, over) in enumerate(cases):
        over = dict(over)
        kind = over.pop("kind", "pcm16")
        cfg = ref.SquelchConfig(**over)
        if kind == "f32":
            x = bursts_f32(rate, secs, ch, spans, noise, seed=k)
        else:
            pcm = bursts(rate, secs, ch, spans, noise, seed=k)
            x = pcm.astype(np.float32) / np.float32(32768.0)
        cleaned, floor_db, thr_db = ref.apply_squelch(x, float(rate), cfg)
        # the same stages again, to record the mask and the gain
        samples = ref._ensure_2d(np.asarray(x, dtype=np.float32))
        window = max(1, int(round(cfg.window_seconds * rate)))
        env_db = ref._dbfs(ref._envelope(samples, window))
        if cfg.method == "transient":
            mask = ref._transient_mask(samples, rate, cfg)
        elif cfg.method == "adaptive":
            mask = ref._adaptive_mask(env_db, thr_db)
        else:
            mask = ref._static_mask(env_db, thr_db)
        head = int(round(rate * cfg.hold_seconds))
        gain = ref._smooth_gain(ref._dilate_mask(mask, head=head, tail=head), int(round(rate * cfg.fade_seconds)))
        n = samples.shape[0]
        if cfg.trim_silence:
            act = np.flatnonzero(gain > 1e-3)
            if act.size == 0:
                start = stop = 0
            else:
                start = max(0, int(act[0]) - int(max(0, round(rate * cfg.trim_lead_seconds))))
                stop = min(n, int(act[-1]) + int(max(0, round(rate * cfg.trim_trail_seconds))) + 1)
        else:
            start, stop = 0, n
        again = (samples * gain[:, None])[start:stop]
        assert again.shape == cleaned.shape and np.array_equal(again, cleaned), name
        params = dict(over, sample_rate=rate)
        if kind == "f32":
            blob[f"{name}__f32"] = x
        else:
            u = pcm.view(np.uint16)  # byte planes: the high bytes of quiet noise are nearly constant and deflate well
            blob[f"{name}__pcm_hi"] = (u >> 8).astype(np.uint8)
            blob[f"{name}__pcm_lo"] = (u & 0xFF).astype(np.uint8)
        blob[f"{name}__kind"] = np.array(kind)
        blob[f"{name}__params"] = np.array(json.dumps(params))
        blob[f"{name}__scalars"] = np.array([floor_db, thr_db, start, stop], dtype=np.float64)
        blob[f"{name}__mask"] = np.packbits(mask)
        blob[f"{name}__gain"] = gain.astype(np.float32)
        print(f"{name}: n={n} C={ch} floor={floor_db:.3f} thr={thr_db:.3f} out=[{start},{stop}) mask={int(mask.sum())}")
    blob["cases"] = np.array([c[0] for c in cases])
    np.savez_compressed(out, **blob)
    print(f"wrote {out} ({out.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
