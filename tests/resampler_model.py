"""Float64 model of the 48 kHz resampler (csrc/demod.hip: k_resample, k_resample_long, iqa_resample), for the tests
only; the product never imports it.

* ``y64`` evaluates the defining sum ``y[j] = sum_t table[p][t] * x[q - (t - T)]``, ``q, p = divmod(j * down, up)``,
  zeros outside ``[0, n)``, directly in float64 on the prototype of ``oracle.cpu_ref.resampler_prototype`` (no
  ``upfirdn``).  ``y64_upfirdn`` is the same sum through scipy, for the one stream that is too long for the gather.
* ``check`` holds a kernel's float32 output to "float64 accumulate, ONE rounding to float32": equal to
  ``float32(y64)`` bit for bit, except where y64 lies so close to a float32 rounding midpoint that two correct
  float64 evaluations may round to different sides.  ``bound`` is that distance.
* ``paths`` restates the launch arithmetic of ``iqa_resample`` and the wave set-up of ``k_resample``: which kernel and
  build a shape reaches, how many steps its waves run, how many of them leave the staged path.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import cpu_ref as O

CHUNK = 16_384  # outputs per gather (at most 65 536: the index matrix of a 321-tap row stays below 50 MB)

# Restated from csrc/demod.hip; tests/test_resampler_model_host.py pins the shapes of tests/test_gpu_resampler_shapes.py
# to the paths these give, so retuning one of them there fails here until the shapes are chosen again.
RS_TARGET_WAVES = 8192  # IQA_RS_TARGET_WAVES (demod.hip:269-271)
RS_GROUP = 4            # RS_GROUP (demod.hip:277)
RS_AHEAD = 8            # IQA_RS_AHEAD / RS_AHEAD (demod.hip:278-281)
RS_RING = RS_AHEAD + 2  # RS_RING (demod.hip:283)
RS_LONG_ROW = 192       # rows longer than this go to k_resample_long (demod.hip:678)
RS_BUILDS = (17, 24, 32, 48)  # taps per lane of the k_resample builds (demod.hip:720-723)


def spread(ni: int) -> int:
    """RsGeo<NI>::SPREAD (demod.hip:295)."""
    return min(2 * ni + 2, 253 - 4 * ni)


@functools.lru_cache(maxsize=4)
def _table(up: int, down: int):
    """(T, table[up, 2T+1]): row p holds h[p + t*up], t = -T..T, zero outside the prototype's support."""
    h = O.resampler_prototype(up, down)
    half = (h.size - 1) // 2
    t_half = -(-half // up)
    idx = np.arange(up, dtype=np.int64)[:, None] + np.arange(-t_half, t_half + 1, dtype=np.int64)[None, :] * up
    table = np.where(np.abs(idx) <= half, h[np.clip(idx + half, 0, 2 * half)], 0.0)
    table.setflags(write=False)
    return t_half, table


def geometry(fs: float):
    """(up, down, T, row length) of a channel rate."""
    _, up, down = O.resampler_plan(fs)
    half = O.RS_ZERO_CROSSINGS * max(up, down)
    t_half = -(-half // up)
    return up, down, t_half, 2 * t_half + 1


def n_out_of(fs: float, n_in: int) -> int:
    up, down, _, _ = geometry(fs)
    return -(-n_in * up // down)


def y64(x: np.ndarray, fs: float, j0: int = 0, n_out: int | None = None):
    """(y, a, row): outputs j0 .. j0 + n_out - 1 of the defining sum in float64, a[j] = sum |h| |x| (the scale of the
    sum's rounding error) and the row length 2T + 1."""
    up, down, t_half, row = geometry(fs)
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    if n_out is None:
        n_out = -(-n * up // down) - j0
    y = np.zeros(n_out, dtype=np.float64)
    a = np.zeros(n_out, dtype=np.float64)
    if up == 1 and down == 1:
        y[:] = x[j0:j0 + n_out]
        return y, np.abs(y), 1
    _, table = _table(up, down)
    # x between two blocks of zeros: position i of the stream is xp[i + row], everything outside it reads a zero
    xp = np.concatenate([np.zeros(row), x, np.zeros(row)])
    back = np.arange(row, dtype=np.int64) - t_half  # t - T
    for lo in range(0, n_out, CHUNK):
        j = np.arange(j0 + lo, j0 + min(lo + CHUNK, n_out), dtype=np.int64)
        q, p = np.divmod(j * down, up)
        xs = xp[np.clip(q[:, None] - back[None, :] + row, 0, xp.size - 1)]
        rows = table[p]
        y[lo:lo + j.size] = np.sum(rows * xs, axis=1)
        a[lo:lo + j.size] = np.sum(np.abs(rows) * np.abs(xs), axis=1)
    return y, a, row


def y64_upfirdn(x: np.ndarray, fs: float):
    """(y, a, row) of a whole stream as y64 gives them, through scipy's upfirdn (oracle.cpu_ref.resample_48k before its
    rounding): for streams of millions of samples."""
    from scipy import signal

    up, down, _, row = geometry(fs)
    x = np.asarray(x, dtype=np.float64)
    n_out = -(-x.size * up // down)
    h = O.resampler_prototype(up, down)
    half = (h.size - 1) // 2
    pad = (-half) % down
    hp = np.concatenate([np.zeros(pad), h])
    first = (half + pad) // down

    def run(taps, sig):
        v = signal.upfirdn(taps, sig, up, down)[first:first + n_out]
        return np.concatenate([v, np.zeros(n_out - v.size)])

    return run(hp, x), run(np.abs(hp), np.abs(x)), row


def bound(a: np.ndarray, row: int) -> np.ndarray:
    """Largest distance between two float64 evaluations of the sum, whatever their order of additions and with or
    without fused multiply-adds: each is within (row + 3) 2^-53 a of the exact value (row products and row - 1 additions
    at most per path, first-order, with room for the higher orders)."""
    return 2.0 * (row + 3) * 2.0 ** -53 * np.asarray(a, dtype=np.float64)


def _rounded(y: np.ndarray) -> np.ndarray:
    return (np.asarray(y, dtype=np.float64) + 0.0).astype(np.float32)  # (+ 0.0: a sum of -0.0 products is +0.0 in the kernel)


def near_midpoint(y: np.ndarray, a: np.ndarray, row: int):
    """(below, above): outputs whose float64 value lies within `bound` of the rounding midpoint between float32(y) and
    the float32 below / above it."""
    f = _rounded(y)
    lim = bound(a, row)
    dn = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
    upw = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    f64 = f.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        below = np.abs(y - 0.5 * (f64 + dn)) <= lim
        above = np.abs(y - 0.5 * (f64 + upw)) <= lim
    return below, above


def midpoint_cap(n_out: int) -> int:
    return max(2, int(1e-4 * n_out))


def midpoint_count(y: np.ndarray, a: np.ndarray, row: int) -> int:
    below, above = near_midpoint(y, a, row)
    return int(np.count_nonzero(below | above))


def check(y_gpu: np.ndarray, y: np.ndarray, a: np.ndarray, row: int) -> int:
    """y_gpu == float32(y) bit for bit; where y lies within `bound` of a rounding midpoint the float32 on the other side
    of that midpoint passes too.  The share of such outputs is a condition on y alone, asserted first.  Returns it."""
    y_gpu = np.asarray(y_gpu)
    assert y_gpu.dtype == np.float32 and y_gpu.shape == y.shape == a.shape, (y_gpu.dtype, y_gpu.shape, y.shape)
    assert np.all(np.isfinite(y)), "check() is for finite streams"
    below, above = near_midpoint(y, a, row)
    excepted = int(np.count_nonzero(below | above))
    assert excepted <= midpoint_cap(y.size), (excepted, y.size)
    want = _rounded(y)
    same = y_gpu.view(np.uint32) == want.view(np.uint32)
    other = (below & (y_gpu == np.nextafter(want, np.float32(-np.inf)))) | (above & (y_gpu == np.nextafter(want, np.float32(np.inf))))
    bad = ~(same | other)
    if bad.any():
        j = int(np.argmax(bad))
        ulp = np.abs(y_gpu.astype(np.float64) - want.astype(np.float64)) / np.maximum(np.spacing(np.abs(want)).astype(np.float64), 2.0 ** -149)
        raise AssertionError(f"{int(bad.sum())} of {y.size} outputs are not float32(y64); first at j = {j}: got {y_gpu[j]!r}, "
                             f"want {want[j]!r} (y64 {y[j]!r}); largest distance {float(np.nanmax(ulp[bad])):.3g} ulp")
    return excepted


def paths(fs: float, n_in: int, j0: int = 0, n_out: int | None = None) -> dict:
    """What iqa_resample (demod.hip:659-727) launches for this call and what its waves do (k_resample, demod.hip:391-433)."""
    up, down, t_half, row = geometry(fs)
    if n_out is None:
        n_out = -(-n_in * up // down) - j0
    if row > RS_LONG_ROW:
        return {"kernel": "long", "row": row, "up": up, "down": down, "n_out": n_out}
    ni = next(b for b in RS_BUILDS if -(-row // 4) <= b)
    g_all = -(-n_out // up)
    groups = -(-up // 16)
    split = max(1, min(g_all // RS_GROUP, -(-RS_TARGET_WAVES // groups)))
    g_per = -(-g_all // split)
    parts = -(-g_all // g_per) if g_all else 0  # parts with g_lo < g_hi
    # a wave's sixteen residues: first outputs jj0, their input positions q0
    res = np.arange(groups * 16, dtype=np.int64).reshape(groups, 16)
    ok = res < up
    jj0 = np.where(ok, (res - j0 % up) % up, 0)
    q0 = j0 * down // up + (j0 * down % up + jj0 * down) // up
    far = np.where(ok, q0, -(1 << 62)).max(axis=1) - np.where(ok, q0, 1 << 62).min(axis=1) > spread(ni)
    return {
        "kernel": "staged", "row": row, "NI": ni, "SPREAD": spread(ni), "up": up, "down": down, "n_out": n_out, "groups": groups,
        "split": split, "g_per": g_per, "parts": parts, "last_steps": g_all - (parts - 1) * g_per if parts else 0,
        "unstaged_groups": int(np.count_nonzero(far)),  # residue groups whose waves (one per part) read straight from memory
        "staged_groups": int(np.count_nonzero(~far)),
        "partial_last_wave": bool(up % 16),  # quads with res >= up
    }


# ---------------------------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_resampler_shapes.py; tests/test_resampler_model_host.py asserts the path of each

RATE_C2 = 2.5e6 / 26  # 96 154 Hz: up/down = 24000/48077, 1500 groups of residues
# (fs, n_in): waves of 11 to 14 steps -- more than RS_RING, a partial last group -- in every build
LONG_WAVES = [(96_000.0, 200_003), (24_000.0, 110_001), (120_000.0, 520_003), (144_000.0, 300_001), (192_000.0, 400_003),
              (240_000.0, 500_001), (RATE_C2, 2_950_003)]
CLASS_LIMITS = [99_000.0, 102_000.0, 141_000.0, 189_000.0, 285_000.0, 288_000.0]  # n_in = 30 011
# (fs, n_in, j0, cnt)
LATER_STRETCHES = [(131_071.0, 30_011, 7_001, 3_001), (150_000.0, 30_011, 1_003, 5_001), (250_000.0, 30_011, 1_003, 3_001),
                   (96_000.0, 200_003, 33_331, 60_001), (44_100.0, 30_011, 10_007, 20_001), (RATE_C2, 50_000, 24_959, 1),
                   (RATE_C2, 50_000, 23_999, 15), (288_000.0, 30_011, 1_003, 2_001)]
END_RATES = [120_000.0, 144_000.0, 192_000.0, 288_000.0]
END_LENGTHS = [30_009, 30_010, 30_011, 50, 1, 2, 3]  # n % 4 = 1, 2, 3; shorter than every row here; less than a DMA lane
SATURATING_N = 20_001  # at 96 kHz
UPFIRDN_FROM = 1_000_000  # inputs: the gather for shorter streams, scipy's upfirdn from here on
_REFS: dict = {}


def stream(n: int, seed: int = 7) -> np.ndarray:
    """Uniform noise in (-0.9, 0.9): no tone and no period, so a stale or shifted window is an O(1) error."""
    return np.random.default_rng(seed).uniform(-0.9, 0.9, n).astype(np.float32)


def saturating_stream(n: int) -> np.ndarray:
    """Blocks of 250 samples: +1.5, noise of 1e-3, -1.5, noise -- y saturates on both sides and crosses zero between."""
    x = np.random.default_rng(11).uniform(-1e-3, 1e-3, n)
    block = (np.arange(n) // 250) % 4
    x[block == 0] = 1.5
    x[block == 2] = -1.5
    return x.astype(np.float32)


def reference(fs: float, n: int):
    """(x, y64, a, row) of the seeded stream of n samples; computed once, read-only."""
    key = (fs, n)
    if key not in _REFS:
        x = stream(n)
        ref = (x,) + (y64_upfirdn(x, fs) if n >= UPFIRDN_FROM else y64(x, fs))
        for v in ref[:3]:
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]
