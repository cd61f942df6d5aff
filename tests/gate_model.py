"""Numpy oracle of the carrier squelch, written from the specification alone, one function per step,
and the model channel stream of its tests.  Every decision step is also written as a plain Python loop (``*_loops``); the
vectorised forms are held to the loops on small inputs (tests/test_gate_host.py)."""
from __future__ import annotations

import math

import numpy as np

CELL = 256
DEFAULTS = dict(frame_ms=10.0, open_db=6.0, hyst_db=2.0, hang_ms=300.0, min_ms=40.0, lead_ms=20.0, ramp_ms=5.0)


# ---- 1. plan ------------------------------------------------------------------------------------------------------------------

def plan(fs: float, **opts) -> dict:
    o = {**DEFAULTS, **opts}
    if not (o["hyst_db"] < o["open_db"] <= 30.0) or o["hyst_db"] < 0.0:
        raise ValueError("hyst_db < open_db <= 30 and hyst_db >= 0")
    for k in ("frame_ms", "hang_ms", "min_ms", "lead_ms", "ramp_ms"):
        if not 0.0 <= o[k] <= 10_000.0:
            raise ValueError(f"{k} outside 0 .. 10000 ms")
    Lf = 256 * max(1, int(fs * o["frame_ms"] / 1000 / 256))
    if Lf > 2**20:
        raise ValueError("Lf > 2^20")

    def fr(ms):
        return int(math.ceil(ms / 1000 * fs / Lf))

    R = int(np.rint(o["ramp_ms"] / 1000 * fs))
    return dict(fs=float(fs), Lf=Lf, H=fr(o["hang_ms"]), M=max(1, fr(o["min_ms"])), A=fr(o["lead_ms"]), R=R,
                num_open=int(np.rint(1024 * 10 ** (o["open_db"] / 10))),
                num_close=int(np.rint(1024 * 10 ** ((o["open_db"] - o["hyst_db"]) / 10))),
                ramp=np.array([np.float32((k + 1) / (R + 1)) for k in range(R)], dtype=np.float32))


# ---- 2. quantiser -------------------------------------------------------------------------------------------------------------

def choose_shift(mean_power: float) -> int:
    if not (mean_power > 0.0):
        return 15
    if math.isinf(mean_power):
        return -30
    return int(min(max(8 - math.ceil(math.log2(math.sqrt(mean_power))), -30), 30))


def quantise(x, sh: int) -> np.ndarray:
    """clamp(rintf(ldexpf(x, sh)), -32767, 32767) in float32, half-even; NaN -> 0, +-inf -> +-32767."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        v = np.rint(np.ldexp(x, np.int32(sh)).astype(np.float32))
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, -32767, 32767).astype(np.int64)


def power(z, sh: int) -> np.ndarray:
    z = np.asarray(z, dtype=np.complex64)
    qi, qq = quantise(z.real, sh), quantise(z.imag, sh)
    return qi * qi + qq * qq


# ---- 3. cells -----------------------------------------------------------------------------------------------------------------

def n_cells(pos: int, n: int) -> int:
    return 0 if n <= 0 else (pos + n - 1) // CELL - pos // CELL + 1


def cells(z, pos: int, sh: int) -> np.ndarray:
    """int64[n_cells(pos, n)]: one call's sums, the first entry being cell pos // 256."""
    p = power(z, sh)
    out = np.zeros(n_cells(pos, p.size), dtype=np.int64)
    np.add.at(out, (pos + np.arange(p.size, dtype=np.int64)) // CELL - pos // CELL, p)
    return out


def add_cells(parts, n: int) -> np.ndarray:
    """The cells of the whole stream: the calls' sums ((first cell, cells) each) added by cell number."""
    out = np.zeros(-(-n // CELL), dtype=np.int64)
    for first, part in parts:
        out[first : first + len(part)] += np.asarray(part, dtype=np.int64)
    return out


# ---- 4. frames ----------------------------------------------------------------------------------------------------------------

def frames(cell_sums, n: int, Lf: int) -> np.ndarray:
    F, K = max(1, n // Lf), Lf // CELL
    v = np.zeros(F, dtype=np.int64)
    for f in range(F):
        last = f == F - 1
        E = int(sum(int(c) for c in cell_sums[f * K : (len(cell_sums) if last else (f + 1) * K)]))
        N = n - f * Lf if last else Lf
        v[f] = (16 * E) // N
    return v


# ---- 5. floor -----------------------------------------------------------------------------------------------------------------

def floor_of(v) -> int:
    v = np.asarray(v, dtype=np.int64)
    return max(1, int(np.sort(v)[(v.size - 1) // 10]))


# ---- 6. state -----------------------------------------------------------------------------------------------------------------

def state(v, floor: int, num_open: int, num_close: int) -> np.ndarray:
    s, prev = np.zeros(len(v), dtype=np.uint8), 0
    for f, x in enumerate(v):
        x = 1024 * int(x)
        if x >= num_open * floor:
            prev = 1
        elif not x >= num_close * floor:
            prev = 0
        s[f] = prev
    return s


# ---- 7. minimum duration ------------------------------------------------------------------------------------------------------

def runs(bits) -> list:
    """The maximal runs of ones: (first, last) each."""
    out, start = [], None
    for f, b in enumerate(bits):
        if b and start is None:
            start = f
        if not b and start is not None:
            out.append((start, f - 1))
            start = None
    if start is not None:
        out.append((start, len(bits) - 1))
    return out


def min_duration(s, M: int) -> np.ndarray:
    s2 = np.zeros(len(s), dtype=np.uint8)
    for a, b in runs(s):
        if b - a + 1 >= M:
            s2[a : b + 1] = 1
    return s2


# ---- 8. hang and lead ---------------------------------------------------------------------------------------------------------

def hang_lead(s2, H: int, A: int) -> np.ndarray:
    F = len(s2)
    g = np.zeros(F, dtype=np.uint8)
    for f in range(F):
        a, b = max(0, f - H), min(F - 1, f + A)
        g[f] = 1 if np.any(s2[a : b + 1]) else 0
    return g


def bounds(g):
    lo, hi = np.full(len(g), -1, dtype=np.int32), np.full(len(g), -1, dtype=np.int32)
    for a, b in runs(g):
        lo[a : b + 1], hi[a : b + 1] = a, b + 1
    return lo, hi


def decide(cell_sums, n: int, p: dict) -> dict:
    """Steps 4 to 8 from the cells of a stream of n samples."""
    v = frames(cell_sums, n, p["Lf"])
    fl = floor_of(v)
    s = state(v, fl, p["num_open"], p["num_close"])
    s2 = min_duration(s, p["M"])
    g = hang_lead(s2, p["H"], p["A"])
    lo, hi = bounds(g)
    return dict(v=v, floor=fl, s=s, s2=s2, g=g, lo=lo, hi=hi)


def transmissions(g, n: int, Lf: int) -> list:
    """(first sample, one behind the last) of every transmission."""
    F = len(g)
    return [(a * Lf, n if b == F - 1 else (b + 1) * Lf) for a, b in runs(g)]


# ---- 9. apply -----------------------------------------------------------------------------------------------------------------

def gain(g, lo, hi, n: int, p: dict) -> np.ndarray:
    """float32[n]: the factor of every sample (0 where closed, the ramp value or 1 where open), by a loop per transmission."""
    Lf, R, F = p["Lf"], p["R"], len(g)
    out = np.zeros(n, dtype=np.float32)
    for a, b in transmissions(g, n, Lf):
        m = np.arange(a, b, dtype=np.int64)
        k = np.minimum(m - a, b - 1 - m)
        out[a:b] = np.where(k < R, p["ramp"][np.minimum(k, max(R - 1, 0))] if R else np.float32(1), np.float32(1))
    return out


def gain_loops(g, lo, hi, n: int, p: dict) -> np.ndarray:
    """The same by the text of step 9, a sample at a time."""
    Lf, R, F = p["Lf"], p["R"], len(g)
    out = np.zeros(n, dtype=np.float32)
    for m in range(n):
        f = min(m // Lf, F - 1)
        if not g[f]:
            continue
        b = n if hi[f] == F else int(hi[f]) * Lf
        k = min(m - int(lo[f]) * Lf, b - 1 - m)
        out[m] = p["ramp"][k] if k < R else np.float32(1)
    return out


def apply(a, g, lo, hi, p: dict) -> np.ndarray:
    """float32: a[m] gain[m] where open and exactly 0.0 where closed (whatever a holds there)."""
    a = np.asarray(a, dtype=np.float32)
    gn = gain(g, lo, hi, a.size, p)
    open_ = np.asarray(g, dtype=bool)[np.minimum(np.arange(a.size, dtype=np.int64) // p["Lf"], len(g) - 1)]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(open_, a * gn, np.float32(0)).astype(np.float32)


# ---- 10. result ---------------------------------------------------------------------------------------------------------------

def result(d: dict, n: int, sh: int, p: dict) -> dict:
    fl, F = d["floor"], len(d["g"])
    out, covered = [], 0
    for a, b in runs(d["g"]):
        start, end = a * p["Lf"], n if b == F - 1 else (b + 1) * p["Lf"]
        vs = [int(x) for x in d["v"][a : b + 1]]
        held = [int(x) for x, k in zip(d["v"][a : b + 1], d["s2"][a : b + 1]) if k]
        out.append(dict(start=start, end=end, start_s=start / p["fs"], end_s=end / p["fs"], peak_db=10 * math.log10(max(vs) / fl),
                        mean_db=10 * math.log10(sum(held) / len(held) / fl)))
        covered += end - start
    return dict(floor_dbfs=10 * math.log10(fl / 16) - 20 * sh * math.log10(2), duty=covered / n if n else 0.0, transmissions=out)


# ---- the whole gate on a stream ---------------------------------------------------------------------------------------------

def run(z, p: dict, sh: int | None = None, cuts=None) -> dict:
    """The gate of a whole stream; ``cuts``: the call lengths (None: one call)."""
    z = np.asarray(z, dtype=np.complex64)
    n = z.size
    if sh is None:
        head = z[:65536]
        sh = choose_shift(float(np.mean(head.real.astype(np.float64) ** 2 + head.imag.astype(np.float64) ** 2))) if n else 15
    parts, pos = [], 0
    for k in cuts or [n]:
        parts.append((pos // CELL, cells(z[pos : pos + k], pos, sh)))
        pos += k
    assert pos == n
    c = add_cells(parts, n)
    d = decide(c, n, p)
    d.update(cells=c, sh=sh, n=n)
    return d


# ---- the model channel stream -------------------------------------------------------------------------------------------------

MODEL_FS = 96_000.0
MODEL_SECONDS = 3.0
MODEL_KEYED = ((0.5, 1.1), (1.8, 2.0), (2.5, 2.52))


def model_noise(seed: int, n: int, fs: float = MODEL_FS) -> np.ndarray:
    """Complex noise low-passed to 6.25 kHz, scaled to an RMS of 0.01 (complex128)."""
    from scipy.signal import firwin, lfilter

    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n + 256) + 1j * rng.standard_normal(n + 256)
    y = lfilter(firwin(257, 6250.0, fs=fs), 1.0, w)[256:]
    return y * (0.01 / np.sqrt(np.mean(np.abs(y) ** 2)))


def model_carrier(n: int, fs: float = MODEL_FS, keyed=MODEL_KEYED) -> np.ndarray:
    """A unit two-tone FM carrier (700 and 1900 Hz, 2.5 kHz deviation) keyed over ``keyed`` (seconds), zero elsewhere."""
    t = np.arange(n, dtype=np.float64) / fs
    msg = 0.5 * (np.sin(2 * np.pi * 700.0 * t) + np.sin(2 * np.pi * 1900.0 * t))
    phase = 2 * np.pi * 2500.0 * np.cumsum(msg) / fs
    key = np.zeros(n)
    for a, b in keyed:
        key[int(round(a * fs)) : int(round(b * fs))] = 1.0
    return key * np.exp(1j * phase)


def model_stream(cn_db: float | None, seed: int, fs: float = MODEL_FS, seconds: float = MODEL_SECONDS) -> np.ndarray:
    """complex64: the noise and, unless ``cn_db`` is None, the keyed carrier ``cn_db`` over it."""
    n = int(round(fs * seconds))
    z = model_noise(seed, n, fs)
    if cn_db is not None:
        z = z + 0.01 * 10.0 ** (cn_db / 20.0) * model_carrier(n, fs)
    return z.astype(np.complex64)
