"""Models of the stand-alone stage kernels (csrc/stages.hip: k_oscillator_mix, k_trickle_copy; csrc/demod.hip:
k_decimate), for the tests only; the product never imports it.  The decimator and the trickle copy are exact copies:
their model is a numpy slice.  The mixer has a bound.

The mixer's bound.  out[i] = x[i] * (cf + j sf), cf = float32(cos(ph)), sf = float32(sin(ph)), ph = fma(step, i, phase0)
in float64, x the ingest conversion (exact in float32).  ``mix_exact`` is x * exp(j ph) with the ramp step * i + phase0
and the product carried in np.longdouble.  Per component, u = 2^-24 (float32 unit roundoff):

* the oscillator: float64 cos / sin (an error of 2^-52, below everything here) rounded once to float32, u |c| and u |s|;
* the product: re = xr cf - xi sf is two products and a subtraction, 3 roundings, of which each term passes through two
  (its own product, the subtraction) -- one fewer under fma contraction.  Each term therefore carries at most 3 u of its
  magnitude (oscillator + 2), and |xr||c| + |xi||s| <= |xr| + |xi|;
* the phase: ph is the float64 nearest to step * i + phase0, off by at most ulp64(|ph|) / 2, the model's own ramp (long
  double) by less; d/dph of either component is at most |xr| + |xi| in magnitude.

Hence |got - exact| <= (|xr| + |xi|) (3 * 2^-24 + ulp64(|ph|)) per component: one float32 rounding of the oscillator and
at most two in the product, plus the phase.  Derived, not tuned.  At ph ~ 1e6 the phase term is 1.2e-10: a float32 ramp
(ulp32(1e6) = 0.06 rad) or a dropped phase0 misses it by orders of magnitude.
"""
from __future__ import annotations

import numpy as np

import spectrum_model as SM

U32 = 2.0 ** -24
MIX_LENGTHS = (1, 255, 256, 257, 70_001)
#: (phase0, step): a small step from 0; a large phase with both signs of a large step -- 2.0, whose ramp 1e6 + 2 i is made of
#: integers below 2^24 and so survives even a float32 ramp, and a step that is no integer, whose ramp does not
MIX_SETTINGS = ((0.0, 0.0123456789), (0.0, -0.0123456789), (1e6, 2.0), (1e6, -2.0), (1e6, 1.9876543210987), (1e6, -1.9876543210987))
MIX_EXTREMES = {"s16": (-32768, 32767, 0, -1), "u8": (0, 255, 128, 127),
                "f32": (-0.0, 1e-40, float(np.finfo(np.float32).max), -float(np.finfo(np.float32).tiny))}

DECIM_LENGTHS = (1, 255, 256, 257)
TRICKLE_BYTES = (0, 1, 15, 16, 17, 4096, 4096 + 15, (1 << 20) + 3)


def mix_raw(fmt: str, n: int, seed: int = 3, plant: bool = True) -> np.ndarray:
    """Interleaved raw values of n samples over the format's whole range, its extremes at the front and at the end
    (``plant``).  The bound is one of relative roundings: it is run without the float32 extremes, whose products
    underflow (a rounding of 2^-150, not of u |x|) or overflow; the identity at step 0 takes them."""
    rng = np.random.default_rng(seed + n)
    if fmt == "s16":
        raw = rng.integers(-32768, 32768, size=2 * n).astype(np.int16)
    elif fmt == "u8":
        raw = rng.integers(0, 256, size=2 * n).astype(np.uint8)
    else:
        raw = rng.normal(size=2 * n).astype(np.float32)
    if not plant:
        return raw
    e = np.array(MIX_EXTREMES[fmt], dtype=raw.dtype)
    k = min(4, 2 * n)
    raw[:k] = e[:k]
    if n >= 4:
        raw[-4:] = e[::-1]
    return raw


def ingest_c64(raw, fmt: str, order: str) -> np.ndarray:
    xr, xi = SM.ingest(raw, fmt, order)
    out = np.empty(xr.size, dtype=np.complex64)
    out.real, out.imag = xr, xi  # (float32 values widened: the narrowing is exact)
    return out


def phases(n: int, phase0: float, step: float) -> np.ndarray:
    """step * i + phase0 in np.longdouble."""
    return np.longdouble(step) * np.arange(n, dtype=np.longdouble) + np.longdouble(phase0)


def mix_exact(x, phase0: float, step: float):
    """(re, im) of x * exp(j (phase0 + step i)) as float64, evaluated in np.longdouble."""
    x = np.asarray(x, dtype=np.complex64)
    ph = phases(x.size, phase0, step)
    c, s = np.cos(ph), np.sin(ph)
    xr, xi = x.real.astype(np.longdouble), x.imag.astype(np.longdouble)
    return (xr * c - xi * s).astype(np.float64), (xr * s + xi * c).astype(np.float64)


def mix_bound(x, phase0: float, step: float) -> np.ndarray:
    """(|xr| + |xi|) (3 * 2^-24 + ulp64(|ph|)) per sample."""
    x = np.asarray(x, dtype=np.complex64)
    ph = np.abs(phases(x.size, phase0, step).astype(np.float64))
    mag = np.abs(x.real.astype(np.float64)) + np.abs(x.imag.astype(np.float64))
    return mag * (3.0 * U32 + np.spacing(ph))


def mix_ratio(got, x, phase0: float, step: float, *, factor: float = 1.0) -> float:
    """Asserts the bound (times ``factor``) on both components of every sample; returns the largest |err| / bound."""
    got = np.asarray(got)
    assert got.dtype == np.complex64 and got.shape == np.asarray(x).shape
    re, im = mix_exact(x, phase0, step)
    bound = factor * mix_bound(x, phase0, step)
    err = np.maximum(np.abs(got.real.astype(np.float64) - re), np.abs(got.imag.astype(np.float64) - im))
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (f"{bad.size} of {got.size} samples outside the mixer's bound; first at {bad[0]}: "
                           f"|err| = {err[bad[0]]:.3e}, bound = {bound[bad[0]]:.3e}")
    live = bound > 0
    return float(np.max(err[live] / bound[live])) if live.any() else 0.0


def same_values(got, want) -> bool:
    """Equal as numbers everywhere and bit for bit wherever the value is not a zero (a zero's sign depends on the signs
    of the vanishing products: -0 * 1 - x * 0 is -0 for x > 0 and +0 for x < 0)."""
    g = np.ascontiguousarray(got).view(np.float32)
    w = np.ascontiguousarray(want).view(np.float32)
    if g.shape != w.shape or not np.array_equal(g, w):
        return False
    nz = w != 0
    return bool(np.array_equal(g[nz].view(np.uint32), w[nz].view(np.uint32)))


def decimate_cases():
    """(n, D, first, n_out): D in {1, 2, 3, 26, n, n + 5}, first in {0, D - 1}, every output the input has -- the last read
    is the last sample that first + i D reaches -- and n_out = 0."""
    out = []
    for n in DECIM_LENGTHS:
        for d in sorted({1, 2, 3, 26, n, n + 5}):
            for first in sorted({0, d - 1}):
                full = 0 if first >= n else -(-(n - first) // d)
                for n_out in sorted({full, 0}):
                    out.append((n, d, first, n_out))
    return out


def decimate_input(n: int) -> np.ndarray:
    """complex64[n] as raw bits: every value distinct, with NaN payloads, infinities, -0.0 and denormals among them."""
    rng = np.random.default_rng(40 + n)
    words = rng.integers(0, 1 << 32, size=2 * n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x807FFFFF],
                       dtype=np.uint32)
    k = min(special.size, words.size)
    words[:k] = special[:k]
    words[-1] = special[0] if n > 1 else words[-1]
    return words


def trickle_workgroups(nbytes: int):
    """0 (the default of 8), 1, 8, 64 and more workgroups than the copy has 16-byte words."""
    return (0, 1, 8, 64, nbytes // 16 + 1)
