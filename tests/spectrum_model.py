"""Float64 model of the spectrum kernels (csrc/spectrum.hip: k_psd_window, rocFFT, k_psd_finish, k_pair_average behind
iqa_psd_frames and iqa_pair_average_rows), for the tests only; the product never imports it.  The caller supplies the
window and the scale, as the C ABI does.

* ``windowed`` is the exact image k_psd_window writes: the ingest conversion is exact in float32 (integers below 2^16
  times a power of two), the widening to float64 is exact, and each component takes one float64 multiply by the window.
  numpy reproduces that bit for bit.
* ``power`` is |FFT|^2 / scale in float64 through scipy's pocketfft, in output (fftshift-ed) order; ``exact_power`` the
  same through a direct ``np.longdouble`` DFT (O(nfft^2), for nfft <= 1024).
* ``db`` is 10 log10(|p| + 1e-18); ``shift_index(k, nfft)`` is the FFT bin that output bin k shows.
* ``power_bound`` bounds |p_gpu - p| per bin in linear power, where p_gpu = 10^(db_gpu / 10) - 1e-18.
* ``pair_average`` is the waterfall's pairwise row reduction.
* The case tables of tests/test_gpu_spectrum_shapes.py live here; tests/test_spectrum_model_host.py asserts their
  conditions and measures the constant of the bound.

The bound.  A float64 FFT of length n returns X + dX with ||dX||_2 <= k eps log2(n) ||X||_2, eps = 2^-52, k of order one
for any factorisation into small radices (Bluestein: three such transforms of a length >= 2n - 1, a few times larger).
||X||_2 = sqrt(n) ||x||_2 for the windowed frame x, and a bin's power p = |X_k|^2 / scale moves by at most
(2 |X_k| |dX_k| + |dX_k|^2) / scale.  The form used is

    fft_term = c eps log2(n) ||x||_2^2 / scale

with one constant c for every length and bin.  c is not reasoned out: C_MEASURED is the largest ratio
|p_pocketfft - p_exact| / (eps log2(n) ||x||_2^2 / scale) over every bin of every case of the tables below (measured by
tests/test_spectrum_model_host.py, which fails if the tables or numpy give a larger one), and C = 8 C_MEASURED: rocFFT
may factor a length differently from pocketfft, and 8 times covers another factorisation of the same order of accuracy.
The largest ratios come from the single exponentials (all of ||x||^2 n in one bin: the ratio grows like n / log2 n) at the
Bluestein lengths.  A GPU value outside the bound is a finding to explain, never a reason to raise C.

The second term is the round trip through dB.  The kernel returns d = 10 log10(q), q = p + 1e-18, with the 1e-18 added
in float64 (0.5 ulp of q), log10 to 2 ulp of its value and the product by 10 to 0.5 ulp: |delta d| <= 3 eps |d| (eps as
the unit, twice the unit roundoff: generous).  The test forms 10^(d / 10): the division (0.5 ulp of d / 10) and pow
(1 ulp of its result).  A change delta d moves 10^(d/10) by the factor ln(10) / 10 * delta d, so

    log_term = q eps (2 + 4 (ln(10) / 10) |d|),      |d| <= 180:  at most 170 eps q,

and the subtraction of 1e-18 adds 0.5 ulp of q, inside the leading 2.  power_bound = fft_term + log_term.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
from scipy import fft as _sfft

EPS64 = 2.0 ** -52
FLOOR = 1e-18
FMT_CODE = {"s16": 0, "u8": 1, "f32": 2}
FMT_DTYPE = {"s16": np.int16, "u8": np.uint8, "f32": np.float32}
FORMATS = ("s16", "u8", "f32")
ORDER_CODE = {"iq": 0, "qi": 1, "iq_inv": 2, "qi_inv": 3}
ORDERS = tuple(ORDER_CODE)
#: values behind the samples of a call, inside the allocation: a read past n_samples meets them
HOSTILE = {"s16": 32767, "u8": 255, "f32": np.nan}


def ingest(raw, fmt: str, iq_order: str):
    """(re, im) as float64: load_sample of spectrum.hip (and of k_oscillator_mix), exact."""
    flat = np.asarray(raw).reshape(-1)
    assert flat.dtype == FMT_DTYPE[fmt] and flat.size % 2 == 0
    if fmt == "s16":
        f = flat.astype(np.float32) * np.float32(1.0 / 32768.0)
    elif fmt == "u8":
        f = (flat.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 128.0)
    else:
        f = flat
    a, b = f[0::2], f[1::2]
    code = ORDER_CODE[iq_order]
    xr, xi = (b, a) if code & 1 else (a, b)
    if code & 2:
        xi = -xi
    return xr.astype(np.float64), xi.astype(np.float64)


def windowed(raw, fmt, iq_order, first, hop, n_frames, nfft, use, window) -> np.ndarray:
    """complex128[n_frames][nfft]: what k_psd_window leaves in the work buffer."""
    xr, xi = ingest(raw, fmt, iq_order)
    w = np.asarray(window, dtype=np.float64)
    assert w.size >= use and 1 <= use <= nfft and first + (n_frames - 1) * hop + use <= xr.size
    out = np.zeros((n_frames, nfft), dtype=np.complex128)
    for f in range(n_frames):
        lo = first + f * hop
        out[f, :use].real = xr[lo:lo + use] * w[:use]
        out[f, :use].imag = xi[lo:lo + use] * w[:use]
    return out


def shift_index(k, nfft: int):
    """The FFT bin shown at output bin k: numpy's fftshift, out[k] = X[(k - nfft // 2) mod nfft]."""
    return (np.asarray(k) + (nfft + 1) // 2) % nfft


def power(raw, fmt, iq_order, first, hop, n_frames, nfft, use, window, scale) -> np.ndarray:
    """float64[n_frames][nfft], fftshift-ed: |FFT(windowed)|^2 / scale."""
    spec = _sfft.fft(windowed(raw, fmt, iq_order, first, hop, n_frames, nfft, use, window), axis=1)
    spec = spec[:, shift_index(np.arange(nfft), nfft)]
    return (spec.real * spec.real + spec.imag * spec.imag) / scale


_TWIDDLES: dict = {}


def _twiddles(nfft: int):
    if nfft not in _TWIDDLES:
        pi = np.longdouble(4) * np.arctan(np.longdouble(1))
        ang = (np.longdouble(2) * pi / np.longdouble(nfft)) * np.arange(nfft, dtype=np.longdouble)
        _TWIDDLES[nfft] = (np.cos(ang), -np.sin(ang))
    return _TWIDDLES[nfft]


def exact_power(raw, fmt, iq_order, first, hop, n_frames, nfft, use, window, scale) -> np.ndarray:
    """``power`` through a direct DFT in np.longdouble (only the rows i < use of the matrix: the rest meet zeros)."""
    assert nfft <= 1024
    x = windowed(raw, fmt, iq_order, first, hop, n_frames, nfft, use, window)[:, :use]
    xr, xi = x.real.astype(np.longdouble), x.imag.astype(np.longdouble)
    c, s = _twiddles(nfft)
    idx = np.outer(np.arange(use), shift_index(np.arange(nfft), nfft)) % nfft
    wr, wi = c[idx], s[idx]
    re = xr @ wr - xi @ wi
    im = xr @ wi + xi @ wr
    return ((re * re + im * im) / np.longdouble(scale)).astype(np.float64)


def db(p) -> np.ndarray:
    return 10.0 * np.log10(np.abs(np.asarray(p, dtype=np.float64)) + FLOOR)


def from_db(d) -> np.ndarray:
    """The linear power a dB value stands for (what the bound is stated on)."""
    return 10.0 ** (np.asarray(d, dtype=np.float64) / 10.0) - FLOOR


def fft_form(raw, fmt, iq_order, first, hop, n_frames, nfft, use, window, scale) -> np.ndarray:
    """eps log2(nfft) ||frame w||_2^2 / scale per frame (float64[n_frames][1])."""
    x = windowed(raw, fmt, iq_order, first, hop, n_frames, nfft, use, window)
    return EPS64 * np.log2(nfft) * np.sum(x.real * x.real + x.imag * x.imag, axis=1, keepdims=True) / scale


def power_bound(raw, fmt, iq_order, first, hop, n_frames, nfft, use, window, scale, *, p=None, c=None) -> np.ndarray:
    """Per bin: c eps log2(nfft) ||frame w||^2 / scale + (p + 1e-18) eps (2 + 4 ln(10) / 10 |dB(p)|)."""
    if p is None:
        p = power(raw, fmt, iq_order, first, hop, n_frames, nfft, use, window, scale)
    q = np.abs(p) + FLOOR
    log_term = q * EPS64 * (2.0 + 4.0 * (np.log(10.0) / 10.0) * np.abs(10.0 * np.log10(q)))
    return (C if c is None else c) * fft_form(raw, fmt, iq_order, first, hop, n_frames, nfft, use, window, scale) + log_term


def db_tolerance(p, bound) -> np.ndarray:
    """The dB distance that a linear deviation of ``bound`` allows at power p (bound < p + 1e-18)."""
    r = bound / (np.abs(p) + FLOOR)
    assert np.all(r < 0.5)
    return -10.0 * np.log10(1.0 - r)


def pair_average(rows) -> np.ndarray:
    """float32[ceil(n / 2)][cols]: float64 mean of neighbouring rows rounded to float32, an odd last row copied."""
    rows = np.asarray(rows, dtype=np.float32)
    n = rows.shape[0]
    out = np.empty(((n + 1) // 2, rows.shape[1]), dtype=np.float32)
    for r in range(out.shape[0]):
        if 2 * r + 1 < n:
            out[r] = ((rows[2 * r].astype(np.float64) + rows[2 * r + 1].astype(np.float64)) / 2.0).astype(np.float32)
        else:
            out[r] = rows[2 * r]
    return out


# ---------------------------------------------------------------------------------------------------------------
# inputs


def positive_window(use: int) -> np.ndarray:
    """A Hamming-shaped window on half-sample points: no zero at any length (np.hanning(2) is all zeros)."""
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * (np.arange(use, dtype=np.float64) + 0.5) / use)


def scale_of(window, sample_rate: float) -> float:
    """spectrum.py:39,167: use * fs * mean(w^2) + 1e-18."""
    w = np.asarray(window, dtype=np.float64)
    return float(w.size * sample_rate * (np.sum(w * w) / w.size) + FLOOR)


SAMPLE_RATE = 48_000.0
SIGMA = 0.15  # white noise per component: no bin of a frame is a deep null
EXTREMES = {"s16": (-32768, 32767, 0, -1), "u8": (0, 255, 128, 127),
            "f32": (-0.0, 1e-40, -1e-45, float(np.finfo(np.float32).tiny))}


def noisy(fmt: str, n: int, seed: int, plant: bool = True) -> np.ndarray:
    """Interleaved raw values of n samples: two tones of unequal strength at +0.1234 fs and -0.31 fs over white noise of
    sigma 0.15, Q at half the gain of I (a swap or a lost negation moves power to the mirror bin and changes every
    noise bin), the format's extreme values planted at samples 1, 2 and n - 1 (``plant``; not where a frame is a single
    sample: a frame that is one denormal has no power to compare)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = 0.15 * np.exp(2j * np.pi * 0.1234 * t) + 0.1 * np.exp(-2j * np.pi * 0.31 * t)
    x = x + rng.normal(scale=SIGMA, size=n) + 1j * rng.normal(scale=SIGMA, size=n)
    v = np.empty(2 * n, dtype=np.float64)
    v[0::2], v[1::2] = x.real, 0.5 * x.imag
    if fmt == "s16":
        raw = np.clip(np.rint(v * 32767.0), -32768, 32767).astype(np.int16)
    elif fmt == "u8":
        raw = np.clip(np.rint(128.0 + 127.0 * v), 0, 255).astype(np.uint8)
    else:
        raw = v.astype(np.float32)
    e = np.array(EXTREMES[fmt], dtype=raw.dtype)
    if plant and n >= 4:
        raw[2:6] = e
        raw[2 * n - 2:] = e[:2]
    return raw


def exponential(nfft: int, b: int, n: int | None = None) -> np.ndarray:
    """float32 interleaved: 0.5 exp(2 pi j b t / nfft)."""
    t = np.arange(nfft if n is None else n, dtype=np.float64)
    x = 0.5 * np.exp(2j * np.pi * b * t / nfft)
    return x.astype(np.complex64).view(np.float32).copy()


# ---------------------------------------------------------------------------------------------------------------
# case tables


@dataclass(frozen=True)
class Case:
    name: str
    fmt: str
    order: str
    nfft: int
    use: int
    n_frames: int
    hop: int
    first: int
    kind: str = "noisy"  # "noisy": every bin compared in dB terms (no mask); "tone" / "zeros": linear power only
    bin: int = 0
    seed: int = 1

    @property
    def n_samples(self) -> int:
        return self.first + (self.n_frames - 1) * self.hop + self.use

    def raw(self) -> np.ndarray:
        if self.kind == "tone":
            return exponential(self.nfft, self.bin, self.n_samples)
        if self.kind == "zeros":
            return np.zeros(2 * self.n_samples, dtype=FMT_DTYPE[self.fmt]) + (128 if self.fmt == "u8" else 0)
        return noisy(self.fmt, self.n_samples, self.seed, plant=self.use >= 8)

    def window(self) -> np.ndarray:
        return np.ones(self.use) if self.kind == "tone" else positive_window(self.use)

    def scale(self) -> float:
        return float(self.nfft) if self.kind == "tone" else scale_of(self.window(), SAMPLE_RATE)

    def args(self):
        """The model functions' arguments."""
        return (self.raw(), self.fmt, self.order, self.first, self.hop, self.n_frames, self.nfft, self.use, self.window(),
                self.scale())


NFFTS = (2, 3, 255, 256, 257, 999, 1024)


def _size_cases():
    out = []
    for nfft in NFFTS:
        for use in sorted({1, nfft - 1, nfft}):
            for n_frames in (1, 3):
                out.append(Case(f"nfft{nfft}-use{use}-x{n_frames}", "f32", "iq", nfft, use, n_frames, max(1, nfft // 4), 0,
                                seed=100 + nfft + use))
    return tuple(out)


SIZE_CASES = _size_cases()
FORMAT_CASES = tuple(Case(f"{fmt}-{order}-nfft{nfft}", fmt, order, nfft, nfft, 2, nfft // 4, 3, seed=7)
                     for fmt in FORMATS for order in ORDERS for nfft in (256, 257))
GEOMETRY_NFFT = 260  # two thread blocks per frame, a multiple of 4, no power of two
GEOMETRY_CASES = tuple(Case(f"x{n_frames}-hop{hop}-first{first}", FORMATS[i % 3], "iq", GEOMETRY_NFFT, GEOMETRY_NFFT, n_frames, hop,
                            first, seed=11)
                       for i, (n_frames, hop, first) in enumerate((nf, h, f0) for nf in (1, 2, 65)
                                                                  for h in (1, GEOMETRY_NFFT // 4, GEOMETRY_NFFT, GEOMETRY_NFFT + 7)
                                                                  for f0 in (0, 5)))
TONE_CASES = tuple(Case(f"tone-nfft{nfft}-bin{b}", "f32", "iq", nfft, nfft, 1, nfft, 0, kind="tone", bin=b)
                   for nfft in (256, 257) for b in (0, 1, nfft // 2 - 1, nfft // 2, nfft // 2 + 1, nfft - 1))
ZERO_CASES = tuple(Case(f"zeros-{fmt}", fmt, "iq", 257, 200, 2, 57, 1, kind="zeros") for fmt in FORMATS)
OUTPUT_CASE = Case("outputs", "s16", "qi_inv", 257, 200, 3, 64, 2, seed=21)
#: ten distinct plans (the library keeps 8), small, of two lengths (a plan's cost is its length's first use): the first is
#: evicted and made again
PLAN_CASES = tuple(Case(f"plan-{nfft}x{n_frames}", "f32", "iq", nfft, nfft, n_frames, nfft // 4, 0, seed=31 + nfft)
                   for nfft in (8, 16) for n_frames in (1, 2, 3, 4, 5))
NOISY_CASES = SIZE_CASES + FORMAT_CASES + GEOMETRY_CASES + (OUTPUT_CASE,) + PLAN_CASES
ALL_CASES = NOISY_CASES + TONE_CASES + ZERO_CASES

PAIR_ROWS = (1, 2, 3, 8, 9)
PAIR_COLS = (1, 255, 256, 257)


def pair_rows(n_rows: int, n_cols: int) -> np.ndarray:
    """dB-like float32 rows; planted in the first columns of rows 0 | 1 (where there are two rows): neighbours in float32
    (their float64 mean is a rounding tie, to even: once with an even lower neighbour, once with an odd one), values of
    opposite sign (mean 0 and mean of one ulp), denormals (a tie among denormals, the smallest one halved)."""
    rng = np.random.default_rng(1000 * n_rows + n_cols)
    rows = rng.uniform(-180.0, 10.0, size=(n_rows, n_cols)).astype(np.float32)
    if n_rows >= 2:
        one = np.float32(-73.25)
        up = np.nextafter(one, np.float32(0))
        tiny = np.float32(1e-45)
        plant = [(one, up), (up, np.nextafter(up, np.float32(0))), (np.float32(41.5), np.float32(-41.5)),
                 (np.float32(-3.0), np.nextafter(np.float32(3.0), np.float32(4.0))), (tiny, np.float32(2e-45)),
                 (tiny, np.float32(0.0)), (np.float32(-1e-40), np.float32(1e-40))]
        for c, (a, b) in enumerate(plant[:n_cols]):
            rows[0, c], rows[1, c] = a, b
    return rows


# streaming_waterfall (Python layer): (name, nfft, hop, max_slices, chunk sizes; None / 0 = a None / an empty chunk)
WATERFALL_CASES = (
    ("max_slices=1", 64, 64, 1, (500, 524)),
    ("hop>nfft", 64, 100, 400, (333, 1, 700, 90, 1000)),
    ("split inside a block", 32, 8, 40, (1000, 300)),  # 122 windows in the first block, room() = 41
    ("chunks of 1", 32, 8, 400, (1,) * 200),
    ("None and empty chunks", 64, 16, 400, (None, 300, 0, None, 500, 0)),
)


def waterfall_chunks(sizes, seed: int = 5):
    total = sum(s for s in sizes if s)
    x = noisy("f32", total, seed).view(np.complex64)
    out, lo = [], 0
    for s in sizes:
        if s is None:
            out.append(None)
        else:
            out.append(x[lo:lo + s].copy())
            lo += s
    return out


def reductions(frames: int, max_slices: int) -> int:
    """How often the waterfall's pairwise reduction runs (row 0 takes part every time: its depth)."""
    n = count = 0
    for _ in range(frames):
        n += 1
        while n > max(1, max_slices):
            n = (n + 1) // 2
            count += 1
    return count


#: the largest |p_pocketfft - p_exact| / (eps log2(n) ||x||^2 / scale) over ALL_CASES (63.955, the exponentials at nfft = 257;
#: tests/test_spectrum_model_host.py measures it again and holds this figure to it)
C_MEASURED = 63.96
C = 8.0 * C_MEASURED
