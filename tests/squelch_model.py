"""A per-stage numpy oracle of the squelch chain (csrc/squelch.hip), one function per stage.

Every function takes the previous stage's array, so a GPU stage can be judged against the oracle applied to the GPU's
own previous stage.  The stages are written from their definitions -- direct window sums (``np.correlate`` is a plain
O(n w) sum), ``np.percentile``, explicit edge padding -- and use none of the kernel's devices: no prefix sums, no
radix select, no closed-form edge terms.  ``tests/test_squelch_model_host.py`` binds this file to the reference's
recorded results and to numpy's own int8 / float32 convolutions before it judges a kernel.
"""
from __future__ import annotations

import numpy as np

MIN_DBFS = -160.0
EPS = 1e-10


def windows(rate: float, cfg) -> dict:
    """The sample counts of a configuration, as the reference rounds them."""
    short = max(1, int(round(cfg.transient_window_seconds * rate)))
    window = max(1, int(round(cfg.window_seconds * rate)))
    return dict(window=window, short_window=short, long_window=max(short * 4, int(round(cfg.window_seconds * rate))),
                hold=int(round(rate * cfg.hold_seconds)), fade=int(round(rate * cfg.fade_seconds)),
                lead=int(max(0, round(rate * cfg.trim_lead_seconds))),
                trail=int(max(0, round(rate * cfg.trim_trail_seconds))))


def magnitude(x: np.ndarray) -> np.ndarray:
    """Channel mean of |x| ([n, C] float32), accumulated in float64, as float32."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[:, None]
    return np.mean(np.abs(x), axis=1, dtype=np.float64).astype(np.float32)


def box(mag: np.ndarray, w: int) -> np.ndarray:
    """Moving average of w taps centred as np.convolve(mode="same"): taps i - w//2 .. i - w//2 + w - 1, zero outside.
    Direct float64 window sums, divided by w, as float32."""
    mag = np.asarray(mag, dtype=np.float32)
    if w == 1:
        return mag
    left = w // 2
    padded = np.concatenate((np.zeros(left), mag.astype(np.float64), np.zeros(w - 1 - left)))
    sums = np.correlate(padded, np.ones(w, dtype=np.float64), mode="valid")
    assert sums.size == mag.size
    return (sums / w).astype(np.float32)


def dbfs(v: np.ndarray) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    return np.maximum(MIN_DBFS, 20.0 * np.log10(np.maximum(v, EPS))).astype(np.float32)


def envelope_db(mag: np.ndarray, w: int) -> np.ndarray:
    return dbfs(box(mag, w))


def envelope_bound(want: np.ndarray) -> np.ndarray:
    """How far a correct float32 envelope (dB) may lie from the oracle's.  The two float64 window sums differ by far
    less than half a float32 ulp, so the float32 averages differ by at most one ulp (a factor 1 + 2^-23: the first
    term); each side's final cast to float32 rounds by half an ulp of the result (the second term)."""
    want = np.asarray(want, dtype=np.float32)
    return 20.0 * np.log10(1.0 + 2.0 ** -23) + np.spacing(np.abs(want)).astype(np.float64)


def noise_floor(env_db: np.ndarray, percentile: float) -> float:
    pct = float(np.clip(percentile, 0.0, 1.0)) * 100.0
    return float(np.percentile(np.asarray(env_db, dtype=np.float32), pct))


def relative(env_db: np.ndarray) -> np.ndarray:
    """The adaptive method's level: the envelope above its running minimum."""
    env_db = np.asarray(env_db, dtype=np.float32)
    return env_db - np.minimum.accumulate(env_db)


def span(level: np.ndarray):
    """(low, span) of the adaptive score: 5th percentile and max(95th - 5th, 1e-6), float32 steps."""
    level = np.asarray(level, dtype=np.float32)
    low = np.percentile(level, 0.05 * 100.0)
    high = np.percentile(level, 0.95 * 100.0)
    return low, max(high - low, 1e-6)


def adaptive_threshold(env_db: np.ndarray, level: np.ndarray, threshold_db: float) -> np.ndarray:
    """The per-sample threshold of the adaptive method; the plain threshold where nothing is above it (the reference
    returns the all-false mask there and has no threshold array)."""
    env_db = np.asarray(env_db, dtype=np.float32)
    if not np.any(env_db >= threshold_db):
        return np.full(env_db.shape, np.float32(threshold_db), dtype=np.float32)
    level = np.asarray(level, dtype=np.float32)
    low, sp = span(level)
    score = np.asarray((level - low) / sp, dtype=np.float32)
    thr = np.clip(threshold_db + 6.0 * (1.0 - score), threshold_db - 6.0, threshold_db + 6.0)
    assert thr.dtype == np.float32
    return thr


def adaptive_mask(env_db: np.ndarray, thr: np.ndarray, threshold_db: float) -> np.ndarray:
    env_db = np.asarray(env_db, dtype=np.float32)
    above = env_db >= threshold_db
    if not np.any(above):
        return above
    return env_db >= thr


def static_mask(env_db: np.ndarray, threshold_db: float) -> np.ndarray:
    return np.asarray(env_db, dtype=np.float32) >= threshold_db


def transient_level(mag: np.ndarray, short: int, long_: int) -> np.ndarray:
    short_env = box(mag, short)
    long_env = box(mag, long_)
    lifted = long_env + EPS
    assert lifted.dtype == np.float32  # the float32 addition the reference makes
    return dbfs(short_env) - dbfs(lifted)


def transient_mask(level: np.ndarray, margin_db: float) -> np.ndarray:
    return np.asarray(np.asarray(level, dtype=np.float32) >= margin_db, dtype=bool)


def window_counts(mask: np.ndarray, h: int):
    """int64 counts of the set samples in [i - h, i] and in [i, i + h], both clipped to the array."""
    m = np.asarray(mask).astype(np.int64)
    n = m.size
    he = min(int(h), n - 1)  # a window that reaches past the array sees nothing more
    ones = np.ones(he + 1, dtype=np.int64)
    pad = np.zeros(he, dtype=np.int64)
    tail = np.correlate(np.concatenate((pad, m)), ones, mode="valid")
    head = np.correlate(np.concatenate((m, pad)), ones, mode="valid")
    assert tail.size == n and head.size == n
    return tail, head


def int8_positive(count: np.ndarray) -> np.ndarray:
    return (np.asarray(count, dtype=np.int64) % 256).astype(np.uint8).view(np.int8) > 0


def dilate(mask: np.ndarray, h: int, wrap: bool = True) -> np.ndarray:
    """Hold: a sample is kept when a window of h samples before or after it holds a set sample -- counted as the
    reference counts, in int8 (``wrap=False``: the plain count, to show where the wrap matters)."""
    mask = np.asarray(mask, dtype=bool)
    if h <= 0:
        return mask.copy()
    tail, head = window_counts(mask, h)
    if wrap:
        return mask | int8_positive(tail) | int8_positive(head)
    return mask | (tail > 0) | (head > 0)


def burst_mask(lengths=(100, 128, 129, 256, 400), gap=600) -> np.ndarray:
    """Test input: bursts of the given lengths with `gap` clear samples before, between and after them.  A clear
    sample d <= h places after a burst of L >= h + 1 - d set samples has h + 1 - d of them in [i - h, i], so the
    int8 count first fails to be positive at h = 128 (d = 1, 128 set samples); at h <= 127 no clear sample can have
    128 set samples in a window that contains itself, so the wrap cannot show before h = 128."""
    parts = [np.zeros(gap, dtype=bool)]
    for ln in lengths:
        parts += [np.ones(ln, dtype=bool), np.zeros(gap, dtype=bool)]
    return np.concatenate(parts)


def gain(dil: np.ndarray, f: int) -> np.ndarray:
    """Fade: the edge-padded 0/1 mask correlated with the integer numerators of the reference's fade kernel
    [0, 1/f, .., (f-1)/f, 1, 1, (f-1)/f, .., 1/f], as float32(min(W / f, 1))."""
    dil = np.asarray(dil, dtype=bool)
    if f <= 0:
        return dil.astype(np.float32)
    d = dil.astype(np.int64)
    padded = np.concatenate((np.full(f, d[0]), d, np.full(f, d[-1])))
    kernel = np.concatenate((np.arange(0, f), [f], np.arange(f, 0, -1))).astype(np.int64)
    assert kernel.size == 2 * f + 1
    # np.convolve(padded, kernel, "same")[f:-f][i] = sum_k kernel[k] * padded[i + 2f - k]
    w = np.correlate(padded, kernel[::-1], mode="valid")
    assert w.size == d.size
    return np.minimum(w / f, 1.0).astype(np.float32)


def bounds(g: np.ndarray, n: int, lead: int, trail: int, trim: bool):
    if not trim:
        return 0, n
    active = np.flatnonzero(np.asarray(g, dtype=np.float32) > 1e-3)
    if active.size == 0:
        return 0, 0
    return max(0, int(active[0]) - lead), min(n, int(active[-1]) + trail + 1)


def output_f32(x: np.ndarray, g: np.ndarray, start: int, stop: int) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[:, None]
    return (x * np.asarray(g, dtype=np.float32)[:, None])[start:stop]


def output_pcm16(x: np.ndarray, g: np.ndarray, start: int, stop: int) -> np.ndarray:
    y = output_f32(x, g, start, stop)
    return np.clip(np.rint(y.astype(np.float64) * 32767.0), -32768.0, 32767.0).astype(np.int16)


def chain(x: np.ndarray, rate: float, cfg) -> dict:
    """The whole chain on the oracle's own stages (for the fixture tests)."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[:, None]
    w = windows(rate, cfg)
    n = x.shape[0]
    mag = magnitude(x)
    env = envelope_db(mag, w["window"])
    floor_db = noise_floor(env, cfg.noise_floor_percentile) if cfg.auto_noise_floor else float(cfg.manual_noise_floor_db)
    thr_db = floor_db + cfg.threshold_margin_db
    if cfg.method == "transient":
        level = transient_level(mag, w["short_window"], w["long_window"])
        thr = np.full(n, np.float32(cfg.transient_margin_db), dtype=np.float32)
        mask = transient_mask(level, cfg.transient_margin_db)
    elif cfg.method == "adaptive":
        level = relative(env)
        thr = adaptive_threshold(env, level, thr_db)
        mask = adaptive_mask(env, thr, thr_db)
    else:
        level = env
        thr = np.full(n, np.float32(thr_db), dtype=np.float32)
        mask = static_mask(env, thr_db)
    dil = dilate(mask, w["hold"])
    g = gain(dil, w["fade"])
    start, stop = bounds(g, n, w["lead"], w["trail"], cfg.trim_silence)
    return dict(w, envelope_db=env, noise_floor_db=floor_db, threshold_db=thr_db, level=level, threshold=thr, mask=mask,
                dilated=dil, gain=g, start=start, stop=stop, output=output_f32(x, g, start, stop))


def fixture_cases(z):
    """The cases of a reference fixture (tests/golden/gen_squelch.py): (name, input float32 [n, C], sample rate,
    configuration overrides, [floor, threshold, start, stop], packed mask, gain)."""
    import json

    for name in z["cases"]:
        name = str(name)
        params = json.loads(str(z[f"{name}__params"]))
        rate = params.pop("sample_rate")
        kind = str(z[f"{name}__kind"]) if f"{name}__kind" in z.files else "pcm16"
        if kind == "f32":
            x = np.asarray(z[f"{name}__f32"], dtype=np.float32)
        else:
            pcm = ((z[f"{name}__pcm_hi"].astype(np.uint16) << 8) | z[f"{name}__pcm_lo"]).view(np.int16)
            x = pcm.astype(np.float32) / np.float32(32768.0)
        yield name, x, rate, params, z[f"{name}__scalars"], z[f"{name}__mask"], z[f"{name}__gain"]
