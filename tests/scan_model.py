"""Per-sample float64 oracle of the demodulator's scan engine (csrc/demod_fused.hip) and of the stand-alone sink
(k_writer_clip in csrc/demod.hip).  TEST INFRASTRUCTURE ONLY: numpy, scipy and oracle/cpu_ref.py; nothing is imported from
the product.

Every recurrence is evaluated sequentially in float64 and handed out BEFORE the float32 rounding; the float32 roundings are
the ones include/iqa_hotpath.h documents (the DC blocker's input difference and radius, the AGC's threshold test and
target/|x|).  tests/test_scan_model_host.py checks these against the same recurrences in np.longdouble and against the
reference's float32 loops; tests/test_gpu_scan_exact.py compares the kernels with them sample by sample.
"""
from __future__ import annotations

import ctypes
import functools
from dataclasses import dataclass, field

import numpy as np
import scipy.signal as _ssig

from oracle import cpu_ref as O

TILE = 2048            # SC_TILE: samples per workgroup of the reduce / apply passes
CARRY_THREADS = 1024   # FC_THREADS: the carry pass walks ceil(tiles / 1024) tiles per thread
SLOTS = 8              # IQA_SUMSQ_SLOTS
CLIP = np.float32(0.99)
AGC_THRESHOLD = np.float32(1e-6)
EPS32 = 2.0 ** -24     # half a float32 ulp, relative: one rounding to float32
DC_RADIUS = 0.995
AGC_TARGET, AGC_DECAY = O.AGC_TARGET, O.AGC_DECAY

_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        lib = O._seq_lib()
        fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
        lib.dc_block_f64_wide.argtypes = [fp, dp, ctypes.c_size_t, ctypes.c_double, dp, dp]
        lib.dc_block_f64_wide.restype = None
        lib.agc_gain_f64.argtypes = [fp, dp, ctypes.POINTER(ctypes.c_ubyte), ctypes.c_size_t, ctypes.c_double, ctypes.c_double]
        lib.agc_gain_f64.restype = None
        _LIB = lib
    return _LIB


def floor_term(S: float, pole: float) -> float:
    """F = 64 * 2^-53 * S / (1 - A): fewer than 64 roundings of affine compositions lie between a result and the inputs
    (8 in the thread, 6 in the wave, 4 across a tile's waves, a run of at most 3 tiles, 6 + 16 in the carry pass, the same
    again in the apply pass), each amplified by at most the filter's memory 1 / (1 - A)."""
    return 64.0 * 2.0 ** -53 * float(S) / (1.0 - float(pole))


def per_thread_tiles(n: int) -> int:
    """``per`` of k_fused_carry."""
    tiles = (n + TILE - 1) // TILE
    return (tiles + CARRY_THREADS - 1) // CARRY_THREADS


# ---- the three recurrences -------------------------------------------------------------------------


def deemphasis(x: np.ndarray, alpha: float, y_prev: float = 0.0) -> np.ndarray:
    """y = (1-a) x + a y_prev in float64 (lfilter's direct form II transposed: the same two roundings per sample as the
    sequential loop, as O.deemphasis runs it).  Returns the float64 values; the state after the block is y[-1]."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.size == 0:
        return np.empty(0, dtype=np.float64)
    b = np.array([1.0 - alpha], dtype=np.float64)
    a = np.array([1.0, -alpha], dtype=np.float64)
    y, _ = _ssig.lfilter(b, a, x.astype(np.float64), zi=np.array([alpha * float(y_prev)]))
    return y


def dc_block(x: np.ndarray, radius: float = DC_RADIUS, x_prev: float = 0.0, y_prev: float = 0.0) -> np.ndarray:
    """dc_block_f64 of oracle/seq_f32.c with the float64 values handed out: the difference x[n] - x[n-1] in float32, r
    rounded to float32, the recurrence in float64.  State after the block: {float32 x[-1], y[-1]}."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty(x.size, dtype=np.float64)
    if x.size == 0:
        return y
    xp, yp = ctypes.c_double(float(np.float32(x_prev))), ctypes.c_double(float(y_prev))
    _lib().dc_block_f64_wide(x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), y.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                             x.size, radius, ctypes.byref(xp), ctypes.byref(yp))
    return y


def restart_bounds(n: int, restarts) -> np.ndarray:
    """[0, the restart indices inside (0, n), n]: the AGC segments of a block."""
    r = np.asarray(restarts if restarts is not None else [], dtype=np.int64)
    r = r[(r > 0) & (r < n)]
    return np.concatenate(([0], np.unique(r), [n])).astype(np.int64)


def agc_gain(x: np.ndarray, restarts=None, target: float = AGC_TARGET, decay: float = AGC_DECAY):
    """The AGC's float64 gain per sample and the mask of held samples: agc_f64 of oracle/seq_f32.c once per restart segment
    (the gain restarts at 1.0 at index 0 and at every restart index, a sample holds the gain when the float32
    |x| <= float32(1e-6), desired = float32(target) / |x| in float32)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    g = np.empty(x.size, dtype=np.float64)
    held = np.empty(x.size, dtype=np.uint8)
    fp, dp, bp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte)
    b = restart_bounds(x.size, restarts)
    for lo, hi in zip(b[:-1], b[1:]):
        xs, gs, hs = x[lo:hi], g[lo:hi], held[lo:hi]
        _lib().agc_gain_f64(xs.ctypes.data_as(fp), gs.ctypes.data_as(dp), hs.ctypes.data_as(bp), hi - lo, target, decay)
    return g, held.astype(bool)


# ---- the sink ------------------------------------------------------------------------------------


def segment_of(n: int, seg_starts) -> np.ndarray:
    """Segment of every sample: the last start <= index (of equal starts the last one takes the samples)."""
    s = np.asarray(seg_starts, dtype=np.int64)
    return np.searchsorted(s, np.arange(n, dtype=np.int64), side="right") - 1


@dataclass
class Sink:
    audio: np.ndarray   # float32, clipped to +-0.99
    peak: np.float32    # max |v| before the clip
    sums: np.ndarray    # float64 per segment: sum of v*v before the clip (0 for a segment without samples)


def sink(v: np.ndarray, seg_starts=None) -> Sink:
    """AudioWriter.write on the pre-clip float32 values ``v``."""
    v = np.asarray(v, dtype=np.float32)
    peak = np.float32(np.max(np.abs(v))) if v.size else np.float32(0)
    audio = np.minimum(np.maximum(v, -CLIP), CLIP)
    if seg_starts is None or len(seg_starts) == 0:
        return Sink(audio, peak, np.zeros(0))
    v64 = v.astype(np.float64)
    sums = np.bincount(segment_of(v.size, seg_starts), weights=v64 * v64, minlength=len(seg_starts))
    return Sink(audio, peak, sums)


# ---- the source stages ---------------------------------------------------------------------------


def quadrature(z: np.ndarray, prev=np.complex64(1 + 0j)) -> np.ndarray:
    """arctan2 of the float32 products of z * conj(z_prev) as numpy forms them."""
    z = np.asarray(z, dtype=np.complex64)
    lag = np.concatenate((np.array([prev], dtype=np.complex64), z[:-1]))
    p = z * np.conj(lag)
    return np.arctan2(p.imag, p.real).astype(np.float32)


def envelope(z: np.ndarray) -> np.ndarray:
    return np.abs(np.asarray(z, dtype=np.complex64)).astype(np.float32)


def real_part(z: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(z, dtype=np.complex64).real, dtype=np.float32)


SOURCE = {"nfm": "quad", "am": "env", "usb": "real", "lsb": "real"}


def source(mode: str, z: np.ndarray, prev=np.complex64(1 + 0j)) -> np.ndarray:
    kind = SOURCE[mode]
    return quadrature(z, prev) if kind == "quad" else envelope(z) if kind == "env" else real_part(z)


def near_pi(want: np.ndarray) -> np.ndarray:
    """Discriminator values compared modulo 2 pi: a product rounded across the negative real axis may land on either
    sign of pi."""
    return np.abs(want.astype(np.float64)) > np.pi - 1e-5


# ---- the decoder state and one block through a mode --------------------------------------------------


@dataclass
class State:
    """The 32-byte state block: float2 prev | double deemph y_last | double dc x_last, y_last."""

    prev: np.complex64 = np.complex64(1 + 0j)
    de_y: float = 0.0
    dc_x: float = 0.0
    dc_y: float = 0.0

    def image(self) -> np.ndarray:
        img = np.zeros(32, dtype=np.uint8)
        img[:8] = np.array([self.prev], dtype=np.complex64).view(np.uint8)
        img[8:] = np.array([self.de_y, self.dc_x, self.dc_y], dtype=np.float64).view(np.uint8)
        return img


@dataclass
class Block:
    """One block through the scan, from the source stage's float32 values ``u``."""

    y64: np.ndarray          # the recurrence in float64 (AGC: x * gain, x the float32 input of the AGC)
    v: np.ndarray            # float32(y64): the oracle's pre-clip audio (AGC: x * float32(gain) in float32)
    S: float                 # the largest |state|
    F: float                 # the floor term
    # the bound on |got - y64| is rel * 2^-24 * |y64| + floor per sample; extra["floor"] where it is not F itself
    extra: dict = field(default_factory=dict)


def stage_deemphasis(u: np.ndarray, alpha: float, y_prev: float = 0.0) -> Block:
    y = deemphasis(u, alpha, y_prev)
    S = max(float(np.max(np.abs(y))), abs(float(y_prev)))
    F = floor_term(S, alpha)
    return Block(y, y.astype(np.float32), S, F)


def stage_dc(u: np.ndarray, radius: float = DC_RADIUS, x_prev: float = 0.0, y_prev: float = 0.0) -> Block:
    y = dc_block(u, radius, x_prev, y_prev)
    S = max(float(np.max(np.abs(y))), abs(float(y_prev)))
    F = floor_term(S, float(np.float32(radius)))
    return Block(y, y.astype(np.float32), S, F)


def stage_agc(x: np.ndarray, restarts=None, target: float = AGC_TARGET, decay: float = AGC_DECAY) -> Block:
    """The kernel rounds the gain to float32 and multiplies in float32: three roundings' worth on x * g64, and the
    gain's floor term scaled by |x|."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    g, held = agc_gain(x, restarts, target, decay)
    y = x.astype(np.float64) * g
    S = max(float(np.max(g)), 1.0)
    F = floor_term(S, 1.0 - float(np.float32(decay)))
    v = x * g.astype(np.float32)
    return Block(y, v, S, F, {"gain": g, "held": held, "rel": 3.0, "floor": np.abs(x.astype(np.float64)) * F})


def demod_block(mode: str, u: np.ndarray, st: State, alpha: float) -> Block:
    """The linear filter of a fused mode over one block of source values ``u``, from the state ``st`` (not changed).
    SSB with AGC runs ``stage_agc`` behind it on the float32 scratch values."""
    if mode == "nfm":
        return stage_deemphasis(u, alpha, st.de_y)
    return stage_dc(u, DC_RADIUS, st.dc_x, st.dc_y)


def advance(mode: str, st: State, z: np.ndarray, u: np.ndarray, blk: Block) -> State:
    """The state block after a call: prev = z[n-1] (nfm), de-emphasis y_last, DC {x_last (float32 value), y_last}.
    Fields of other modes are left as they were."""
    out = State(st.prev, st.de_y, st.dc_x, st.dc_y)
    if mode == "nfm":
        out.prev = np.complex64(z[-1])
        out.de_y = float(blk.y64[-1])
    else:
        out.dc_x = float(np.float32(u[-1]))
        out.dc_y = float(blk.y64[-1])
    return out


# ---- the inputs of the case matrix (seeded; every seed is kept here) ----------------------------------------

FS_CH = 96_153.84615384616
ALPHA = O.deemph_alpha(300.0, FS_CH)
SEEDS = {"a": 1101, "b": 1102, "c": 1103, "d": 1104, "e": 1105, "f": 1106}
CLASSES_Z = ("a", "b", "c", "e", "f")
QUIET = np.complex64(0.25 + 0.125j)  # the samples next to a stretch of zeros: z * conj(0) is then +0 +0j, not -0


def zero_stretches(n: int):
    """Class (c): (start, length) of the stretches of exact zeros -- lengths 1, 8, 2048 and 5000 where they fit, one
    starting at index 0 and one ending at n - 1; the 2048 one lies over two tile edges (4096 and 6138 -> restarts at tile
    multiples and at +-1 land on held samples)."""
    if n < 3:
        return [(0, 1)]
    if n < 64:
        return [(0, 1), (n - min(8, n // 3), min(8, n // 3))]
    if n < 20_000:
        return [(0, 8), (n // 2, 1), (n - min(2048, n // 4), min(2048, n // 4))]
    return [(0, 8), (4091, 2048), (n // 2, 1), (n - 5000, 5000)]


def _fm_am(n: int, rng) -> np.ndarray:
    t = np.arange(n, dtype=np.float64) / FS_CH
    return (0.3 * np.exp(2j * np.pi * (900.0 * t + 2.0 * np.sin(2 * np.pi * 3.0 * t))) * (1.0 + 0.4 * np.sin(2 * np.pi * 440.0 * t))
            + 0.01 * (rng.normal(size=n) + 1j * rng.normal(size=n)))


@functools.lru_cache(maxsize=6)
def make_z(cls: str, n: int) -> np.ndarray:
    """complex64 channel samples of input class ``cls`` (a, b, c, e, f of the case matrix); shared, not to be written to."""
    rng = np.random.default_rng(SEEDS[cls] + 7919 * (n % 1009))
    k = np.arange(n, dtype=np.float64)
    if cls == "a":      # an FM tone with AM and noise
        z = _fm_am(n, rng)
    elif cls == "b":    # white noise
        z = 0.3 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    elif cls == "c":    # (a) with stretches of exact zeros
        z = _fm_am(n, rng).astype(np.complex64)
        for lo, ln in zero_stretches(n):
            z[lo:lo + ln] = 0
            if lo > 0 and z[lo - 1] != 0:
                z[lo - 1] = QUIET
            if lo + ln < n:
                z[lo + ln] = QUIET
        return z
    elif cls == "e":    # a carrier of 0.5 under a slow envelope: a large offset in front of the DC blocker
        z = (0.5 + 0.2 * np.sin(2 * np.pi * 440.0 * k / FS_CH)) * np.exp(2j * np.pi * 0.01 * k) + 0.01 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    elif cls == "f":    # past the clip: 2.5 rad per sample for the discriminator, an envelope that jumps 0.3 <-> 3.0
        amp = np.where((np.arange(n) // 700) % 2 == 0, 3.0, 0.3)
        z = amp * np.exp(2.5j * k) + 0.01 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    else:
        raise ValueError(cls)
    return z.astype(np.complex64)


def threshold_values() -> np.ndarray:
    """Class (d): float32(1e-6), its two float32 neighbours, both signs."""
    t = AGC_THRESHOLD
    v = np.array([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))], dtype=np.float32)
    return np.concatenate((v, -v))


def make_x(op: str, cls: str, n: int) -> np.ndarray:
    """float32 input of a stage entry point (``op`` in deemph, dc, agc, clip) of class ``cls``: the source stage of the
    mode that feeds that stage, applied on the CPU to ``make_z``; (d) plants the AGC's threshold values into (a)."""
    if cls == "d":
        x = real_part(make_z("a", n)).copy()
        vals = threshold_values()
        pos = np.unique(np.concatenate((np.arange(0, n, 37), [n - 1], np.arange(TILE - 1, n, TILE), np.arange(TILE, n, TILE))))
        x[pos] = vals[np.arange(pos.size) % vals.size]
        return x
    z = make_z(cls, n)
    if op == "deemph":
        return quadrature(z)
    if op == "dc":
        return envelope(z) if cls in ("e", "f") else real_part(z)
    if op == "agc":
        return real_part(z)
    if op == "clip":  # pre-clip audio: the de-emphasised discriminator, |v| up to 2.5 in class (f)
        return stage_deemphasis(quadrature(z), ALPHA).v
    raise ValueError(op)


# ---- the segment / restart layouts ----------------------------------------------------------------------------

STAIRCASE = (1, 7, 8, 9, 63, 64, 65, 511, 512, 513)
LAYOUTS = ("single", "tile", "tile-1", "tile+1", "c5", "stair", "s100", "last", "prod", "dup")


def layout(name: str, n: int) -> np.ndarray:
    """Sorted int64 starts inside [0, n), the first one 0."""
    if name == "single":
        s = [0]
    elif name in ("tile", "tile-1", "tile+1"):
        # every tile edge up to 64 tiles, every 37th beyond (tiles without a boundary in between: `uniform`)
        k = np.arange(1, (n + TILE - 1) // TILE + 1, dtype=np.int64)
        k = k[(k <= 64) | (k % 37 == 0)]
        s = np.concatenate(([0], k * TILE + {"tile": 0, "tile-1": -1, "tile+1": 1}[name]))
    elif name == "c5":      # BASELINE config 5: 50 MS/s, D = 521, reference chunks of 1 048 576 input samples
        s = [-((-k * 1_048_576) // 521) for k in range(n * 521 // 1_048_576 + 2)]
    elif name == "stair":
        reps = n // sum(STAIRCASE) + 2
        s = np.concatenate(([0], np.cumsum(np.tile(STAIRCASE, reps))))
    elif name == "s100":    # 1000 segments of 100 samples: n_segs > 256 (where n allows)
        s = np.arange(1000, dtype=np.int64) * 100
    elif name == "last":
        s = [0, n - 1]
    elif name == "prod":    # the layout of test_demodulate_from_reset_equals_reset_then_demodulate
        s = np.arange(0, n, 40_330, dtype=np.int64)
    elif name == "dup":     # a segment without samples: two equal starts (the last of them takes the samples)
        return np.array([0, min(5, n - 1), min(5, n - 1), min(3000, n - 1)], dtype=np.int64) if n > 1 else np.array([0], dtype=np.int64)
    else:
        raise ValueError(name)
    s = np.unique(np.asarray(s, dtype=np.int64))
    return s[(s >= 0) & (s < n)]


STREAM_CUTS = (1, 1, 2047, 2049, 8, 100_003)


def stream_blocks(n: int):
    """(lo, hi) of the streaming test's blocks: lengths 1, 1, 2047, 2049, 8, 100 003 and the rest."""
    edges = np.concatenate(([0], np.cumsum(STREAM_CUTS), [n]))
    assert edges[-2] < n
    return list(zip(edges[:-1].tolist(), edges[1:].tolist()))


# ---- the one-launch (windowed) form of the de-emphasis scan: its window, layouts on its geometry, its sink plan -----------

SPAN = 8192            # FW_SPAN: positions per workgroup of k_fused_windowed, four rounds of 2048
WINDOW_STEP = 512
FORGET = 2.0 ** -64    # what a warm-up leaves of the state it ignores
WINDOWS = tuple(range(WINDOW_STEP, SPAN // 2 + 1, WINDOW_STEP))

# (tau in microseconds, channel rate in Hz, W or None): the de-emphasis settings the product runs and the window each takes
PRODUCT_WINDOWS = (
    (50.0, FS_CH, 512),
    (1.0, 480_000.0, 512),
    (75.0, 250_000.0, 1024),
    (300.0, FS_CH, 1536),
    (75.0, 480_000.0, 2048),
    (300.0, 192_000.0, 2560),
    (300.0, 225_000.0, 3072),
    (300.0, 250_000.0, 3584),
    (300.0, 288_000.0, 4096),
    (300.0, 384_000.0, None),
    (750.0, 131_071.0, None),
)


def product_alpha(tau_us: float, fs: float) -> float:
    """DeemphasisFilter's pole: exp(-1 / (fs tau)), tau = max(tau_us, 1) microseconds."""
    return float(np.exp(-1.0 / (fs * max(tau_us * 1e-6, 1e-6))))


def alpha_for_need(need: float) -> float:
    """The pole with alpha^need = 2^-64."""
    return float(np.exp(-64.0 * np.log(2.0) / need))


def window(alpha: float, span: int = SPAN):
    """The specification of scan_window: the smallest multiple of 512, at least 512, with alpha^W <= 2^-64 and 2 W <= span;
    None where there is none (no pole in (0, 1), a pole that forgets too slowly): the three launches are kept."""
    if not (alpha > 0.0 and alpha < 1.0):
        return None
    for w in range(WINDOW_STEP, span // 2 + 1, WINDOW_STEP):
        if alpha ** w <= FORGET:
            return w
    return None


WINDOWED_LAYOUTS = ("own", "own-1", "own+1", "own-last", "two-in-one", "fifty", "dup-own", "dup-own-1", "warmup-only")


def windowed_layout(name: str, n: int, W: int, span: int = SPAN) -> np.ndarray:
    """Sorted int64 starts inside [0, n), the first one 0, placed on the geometry of the one-launch form: block k owns
    [k own, min((k + 1) own, n)), own = span - W, and warms up over the W positions in front."""
    own = span - W
    edges = np.arange(own, n, own, dtype=np.int64)  # own0 of every block but the first
    if name in ("own", "own-1", "own+1"):
        s = edges + {"own": 0, "own-1": -1, "own+1": 1}[name]
    elif name == "own-last":     # the last sample of every own range (the last block's is n - 1)
        s = np.append(edges - 1, n - 1)
    elif name == "two-in-one":   # two starts strictly inside every own range: the general path in every block
        first = np.arange(0, n, own, dtype=np.int64)
        s = np.concatenate((first + 1, first + own // 2))
    elif name == "fifty":        # more than 512 starts above n = 25 600, more than 100 boundaries in a block
        s = np.arange(0, n, 50, dtype=np.int64)
    elif name == "dup-own":      # chunk 1 has no samples; block 1's first sample belongs to chunk 2
        return np.array([0, own, own], dtype=np.int64)
    elif name == "dup-own-1":    # block 0 crosses two starts at once, the chunk between them empty
        return np.array([0, own - 1, own - 1], dtype=np.int64)
    elif name == "warmup-only":  # inside block 0's own range and inside block 1's warm-up
        s = [own - W // 2]
    else:
        raise ValueError(name)
    s = np.unique(np.concatenate(([0], np.asarray(s, dtype=np.int64))))
    return s[(s >= 0) & (s < n)]


@dataclass
class BlockPlan:
    """What sink_count_segments and sink_plan decide for one workgroup of k_fused_windowed."""

    own0: int
    own1: int
    seg0: int            # the chunk of the block's first own sample: the last start <= own0
    seg1: int            # the chunk of its last own sample: the last start <= own1 - 1
    kind: str            # "uniform" (seg0 == seg1), "simple" (seg1 == seg0 + 1) or "general"
    bnd: int             # simple: the first index of the high part, segs[seg1]
    at_own0: bool        # a start (other than index 0) on the first own sample
    after_own0: bool     # ... on own0 + 1
    before_own0: bool    # ... on own0 - 1: the last sample of the block in front
    at_last: bool        # ... on own1 - 1
    warmup_only: bool    # starts inside [own0 - W, own0) and none inside [own0, own1)


def windowed_plan_classes(n: int, W: int, span: int, segs) -> list:
    """The restatement of the kernel's conditions, block by block (the counts are `start <= index`, so of equal starts
    the last one takes the samples)."""
    s = np.asarray(segs, dtype=np.int64)
    inner = s[1:]
    own = span - W
    plans = []
    for own0 in range(0, n, own):
        own1 = min(own0 + own, n)
        seg0 = int(np.count_nonzero(s <= own0)) - 1
        seg1 = int(np.count_nonzero(s <= own1 - 1)) - 1
        kind = "uniform" if seg0 == seg1 else "simple" if seg1 == seg0 + 1 else "general"
        in_warmup = bool(own0 > 0 and np.any((inner >= own0 - W) & (inner < own0)))
        in_own = bool(np.any((inner >= own0) & (inner < own1)))
        plans.append(BlockPlan(own0, own1, seg0, seg1, kind, int(s[seg1]) if kind == "simple" else n,
                               bool(np.any(inner == own0)), bool(np.any(inner == own0 + 1)), bool(np.any(inner == own0 - 1)),
                               bool(np.any(inner == own1 - 1)), in_warmup and not in_own))
    return plans


def windowed_chunk_of(n: int, W: int, span: int, segs) -> np.ndarray:
    """The chunk every sample's square is credited to by the one-launch form, from the plans above: a uniform block's go to
    seg0, a simple block's to seg0 below ``bnd`` and to seg1 from it on, a general block looks every sample up."""
    s = np.asarray(segs, dtype=np.int64)
    out = np.empty(n, dtype=np.int64)
    for p in windowed_plan_classes(n, W, span, s):
        idx = np.arange(p.own0, p.own1, dtype=np.int64)
        if p.kind == "general":
            out[p.own0:p.own1] = np.searchsorted(s, idx, side="right") - 1
        else:
            out[p.own0:p.own1] = np.where(idx < p.bnd, p.seg0, p.seg1)
    return out


FIFTY_STARTS = 512  # `fifty` must hold more starts than this in one call: sink_count_segments' loop then runs twice for some threads


def windowed_chunk_cases(W: int, span: int = SPAN) -> list:
    """(layout, n, input class) of the chunk-boundary tests at window W.  Every layout at n = 3 own + W + 5 with class (a),
    `own` and `own-last` with class (c) as well; `fifty` also at 4 own + 3 and, where that is not above 25 600 samples
    (own < 6400), at the first own multiple + 3 that is: more than 512 starts at every window."""
    own = span - W
    n = 3 * own + W + 5
    cases = []
    for lay in WINDOWED_LAYOUTS:
        cases.append((lay, n, "a"))
        if lay in ("own", "own-last"):
            cases.append((lay, n, "c"))
        if lay == "fifty":
            cases.append((lay, 4 * own + 3, "a"))
            if 4 * own + 3 <= 50 * FIFTY_STARTS:
                cases.append((lay, (50 * FIFTY_STARTS // own + 1) * own + 3, "a"))
    return cases


# ---- iqa_raw_level ---------------------------------------------------------------------------------------------------

RAW_LEVEL_FORMATS = {"s16": (0, 8, np.int16), "u8": (1, 16, np.uint8), "f32": (2, 4, np.float32)}  # fmt -> (code, values per 16-byte vector, dtype)


def raw_level_want(fmt: str, raw: np.ndarray) -> float:
    """Mean of value^2 over the eight documented stretches: vectors r * max(1024, n_vec // 8) + [0, 1024), cut at n_vec."""
    _, per_vec, _ = RAW_LEVEL_FORMATS[fmt]
    n_vec = raw.size // per_vec
    step = max(1024, n_vec // 8)
    v = raw[:n_vec * per_vec].astype(np.float64).reshape(n_vec, per_vec) - (128.0 if fmt == "u8" else 0.0)
    rows = np.concatenate([np.arange(r * step, min(r * step + 1024, n_vec)) for r in range(8)]).astype(np.int64) if n_vec else np.zeros(0, np.int64)
    rows = rows[rows < n_vec]
    assert np.unique(rows).size == rows.size
    return float(np.mean(v[rows] ** 2)) if rows.size else 0.0
