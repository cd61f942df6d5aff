"""Float64 model of the float32 channelizer (csrc/channelize.hip: k_channelize_v1 in its two forms, k_history_update,
iqa_channelize), for the tests only; the product never imports it.

* ``direct`` evaluates the header's defining sum per output in float64,
  ``z[m] = scale * rot(m) * conj_if(sum_i taps[i] * x[m*D - consumed - (L-1) + i])`` over the virtual stream
  ``(hist | raw)`` with zeros in front of it, from the arguments of the C entry point.  The phase of ``rot`` is formed in
  Python integers modulo 2^64, ``>> 11``, ``* 2**-53``, as the kernel states it.  ``method="fft"`` is the same sum through
  scipy's overlap-add convolution, for the streams of millions of frames that are too long for the gather.
* An *exact case* (``exact_data``) has integer-valued taps and frames with ``2 * L * max|g| * max|x| < 2**24``: every
  partial sum of either component, in any order, is an integer below 2^24 and so exact in float32.  With ``rotate = 0``
  and a scale of 1, j or -j the kernel's output must then equal ``direct`` bit for bit (``same_bits``).
* ``error_bound`` bounds, per output and component, what the kernel's own summation order can lose on real taps.
* ``classify`` restates the launch arithmetic of ``iqa_channelize`` and the block set-up of ``k_channelize_v1``: which
  form runs, the tile permutation, which blocks are interior, which tap slices the ``continue`` and the ``break`` skip,
  how many 4-frame groups take the guarded scalar path and what they touch.
* The case tables of tests/test_gpu_channelizer_shapes.py live here; tests/test_channelizer_model_host.py asserts the
  path of each.

The bound.  With u = 2^-24 and float32 taps g, frames x (exact in float32 in every format), write
B_re = sum_i |g_re||x_re| + |g_im||x_im|, B_im = sum_i |g_re||x_im| + |g_im||x_re| and B = B_re + B_im =
sum_i (|g_re| + |g_im|)(|x_re| + |x_im|).  A component of the tap sum is a sum of 2 Lpad products, each formed inside
an fma (not rounded on its own).  A product enters one lane's accumulator and from there passes through the remaining
fmas of that accumulator, the 6 adds of the wave butterfly and, in split-K, the 8 adds of the fixed-order sum over the
waves: at most ``depth`` roundings, depth = 8 ceil(Lpad / 256) + 6 (throughput form: 256 taps per wave step, 4 taps
and 2 fmas per tap and component per lane) or 8 ceil(Lpad / 2048) + 6 + 8 (split-K: 2048 taps per block step).  To first
order the component errors are e_re <= depth u B_re, e_im <= depth u B_im.  The rotation by (c, s), c^2 + s^2 = 1, mixes
them: |e_re c - e_im s| <= max(|c|, |s|)(e_re + e_im) <= depth u B, which is why the bound carries B and not B_re.
Epilogue, c_epi = 6: cos and sin rounded to float32 (1 rounding on each term of y_re = S_re c - S_im s), the product
(1) and the subtraction (1) -- 3, or 2 under fma contraction -- on terms whose magnitudes sum to
|S_re||c| + |S_im||s| <= |S_re| + |S_im| <= B; the scale's product and add (2; both exact for 1, j, -j, where one
factor is 1 and the other 0) on |y_re||sc_re| + |y_im||sc_im| <= (|sc_re| + |sc_im|) B; and 1 for everything of second
order: (depth + 5)^2 u <= 1043^2 2^-24 = 0.065 at the longest filter (Lpad = 33024, throughput form), the float64
sincospi (2^-53), and the float64 model's own (L + 3) 2^-53 B <= 6.2e-5 u B.  Hence
|z_gpu - z_model| <= (depth + c_epi) u B (|sc_re| + |sc_im|) per component.  Derived, not tuned.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

# Restated from csrc/channelize.hip; tests/test_channelizer_model_host.py pins the cases below to the paths these give.
CH_WAVES = 8
CH_R = 4  # outputs per wave (throughput form) and per block (split-K)
CH_TCH = 2048  # taps per LDS slice
CH_OUT_PER_BLOCK = CH_WAVES * CH_R
CH_TAP_ALIGN = 256
SPLITK_BELOW = 16384  # iqa_channelize: n_out < this runs the split-K form
XCDS = 8

U = 2.0 ** -24
C_EPI = 6
MASK64 = (1 << 64) - 1
FMT_CODE = {"s16": 0, "u8": 1, "f32": 2}
FMT_DTYPE = {"s16": np.int16, "u8": np.uint8, "f32": np.float32}
FRAME_BYTES = {"s16": 4, "u8": 2, "f32": 8}
FORMATS = ("s16", "u8", "f32")


def padded_len(ntaps: int) -> int:
    return -(-ntaps // CH_TAP_ALIGN) * CH_TAP_ALIGN


def frames(raw, fmt: str) -> np.ndarray:
    """Interleaved raw values -> complex128 frames as the kernel's loaders read them (no ingest scale: the taps carry it)."""
    flat = np.asarray(raw)
    if np.iscomplexobj(flat):
        flat = flat.astype(np.complex64).view(np.float32)
    f = flat.reshape(-1).astype(np.float64)
    if fmt == "u8":
        f = f - 128.0
    return f[0::2] + 1j * f[1::2]


def refusal(ntaps: int, decimation: int, n_frames: int, consumed: int, m_first: int, n_out: int) -> str | None:
    """The argument checks of iqa_channelize, in its order; None where it launches."""
    if ntaps <= 0:
        return "ntaps must be positive"
    if decimation < 1:
        return "decimation must be >= 1"
    if n_out < 0 or n_frames < 0 or consumed < 0 or m_first < 0:
        return "negative size"
    if n_out == 0:
        return None
    newest = (m_first + n_out - 1) * decimation - consumed
    oldest = m_first * decimation - consumed - (ntaps - 1)
    if newest >= n_frames:
        return "outputs requested beyond the frames supplied"
    if newest < 0:
        return "outputs requested before this block"
    if oldest < -(ntaps - 1):
        return "outputs need frames older than the history"
    return None


def _dot(v: np.ndarray, g: np.ndarray, first: int, step: int, n_out: int, method: str) -> np.ndarray:
    """out[o] = sum_i g[i] v[first + o step + i], float64 / complex128."""
    L = g.size
    assert first >= 0 and first + (n_out - 1) * step + L <= v.size, (first, step, n_out, L, v.size)
    if method == "fft":
        from scipy import signal

        return signal.oaconvolve(v[first:first + (n_out - 1) * step + L], g[::-1], mode="valid")[::step]
    assert method == "gather", method
    win = np.lib.stride_tricks.sliding_window_view(v, L)[first::step][:n_out]
    out = np.empty(n_out, dtype=np.result_type(v, g))
    rows = max(1, (1 << 21) // L)
    for lo in range(0, n_out, rows):
        out[lo:lo + rows] = np.ascontiguousarray(win[lo:lo + rows]) @ g
    return out


def _stream(raw, fmt: str, hist, ntaps: int, n_frames: int | None = None) -> np.ndarray:
    x = frames(raw, fmt)
    if n_frames is not None:
        assert x.size >= n_frames
        x = x[:n_frames]
    h = np.zeros(ntaps - 1, dtype=np.complex128) if hist is None else frames(hist, fmt)
    assert h.size == ntaps - 1, (h.size, ntaps)
    return np.concatenate([h, x])


def rotation(m_first: int, n_out: int, rot_step: int, rot_base: int) -> np.ndarray:
    """exp(j 2 pi frac(m)), frac = ((rot_base + m rot_step) mod 2^64 >> 11) 2^-53, for m = m_first ..; the quarter turns
    are taken out exactly first (frac is a multiple of 2^-53, so frac - k/4 is exact), as a sincospi does."""
    ph = np.array([((rot_base + (m_first + i) * rot_step) & MASK64) >> 11 for i in range(n_out)], dtype=np.uint64)
    frac = ph.astype(np.float64) * 2.0 ** -53
    k = np.floor(frac * 4.0 + 0.5)
    r = frac - 0.25 * k
    small = np.cos(2.0 * np.pi * r) + 1j * np.sin(2.0 * np.pi * r)
    return small * np.array([1.0, 1j, -1.0, -1j])[k.astype(np.int64) & 3]


def direct(taps, raw, fmt: str, hist, consumed: int, m_first: int, n_out: int, *, ntaps: int, decimation: int,
           n_frames: int | None = None, conj_sum: int = 0, rotate: int = 0, rot_step: int = 0, rot_base: int = 0,
           scale: complex = 1.0 + 0j, method: str = "gather") -> np.ndarray:
    """z[m_first .. m_first + n_out) of the defining sum, complex128.  ``taps``: window order, at least ``ntaps`` of them,
    taken as the float32 values the kernel sees."""
    v = _stream(raw, fmt, hist, ntaps, n_frames)
    why = refusal(ntaps, decimation, v.size - (ntaps - 1), consumed, m_first, n_out)
    if why is not None:
        raise ValueError(why)
    if n_out == 0:
        return np.zeros(0, dtype=np.complex128)
    g = np.asarray(taps).astype(np.complex64)[:ntaps].astype(np.complex128)
    s = _dot(v, g, m_first * decimation - consumed, decimation, n_out, method)
    if conj_sum:
        s = np.conj(s)
    if rotate:
        s = rotation(m_first, n_out, rot_step, rot_base) * s
    return complex(scale) * s


def abs_sum(taps, raw, fmt: str, hist, consumed: int, m_first: int, n_out: int, *, ntaps: int, decimation: int,
            n_frames: int | None = None, method: str = "gather") -> np.ndarray:
    """B_m = sum_i (|g_re| + |g_im|)(|x_re| + |x_im|) of each output, float64."""
    v = _stream(raw, fmt, hist, ntaps, n_frames)
    g = np.asarray(taps).astype(np.complex64)[:ntaps].astype(np.complex128)
    b = _dot(np.abs(v.real) + np.abs(v.imag), np.abs(g.real) + np.abs(g.imag), m_first * decimation - consumed, decimation,
             n_out, method)
    return np.abs(b)  # (the fft's own rounding may leave -1e-20 where B is 0)


def form_of(n_out: int) -> str:
    return "splitk" if n_out < SPLITK_BELOW else "throughput"


def depth(ntaps: int, form: str) -> int:
    """Roundings a product can pass through before the epilogue."""
    lpad = padded_len(ntaps)
    if form == "throughput":
        return 8 * -(-lpad // (64 * 4)) + 6
    assert form == "splitk", form
    return 8 * -(-lpad // CH_TCH) + 6 + CH_WAVES


def error_bound(taps, raw, fmt: str, hist, consumed: int, m_first: int, n_out: int, *, ntaps: int, decimation: int,
                n_frames: int | None = None, form: str | None = None, scale: complex = 1.0 + 0j,
                method: str = "gather") -> np.ndarray:
    """Per output, the bound on either component of z_gpu - direct (module docstring)."""
    b = abs_sum(taps, raw, fmt, hist, consumed, m_first, n_out, ntaps=ntaps, decimation=decimation, n_frames=n_frames, method=method)
    sc = abs(complex(scale).real) + abs(complex(scale).imag)
    return (depth(ntaps, form or form_of(n_out)) + C_EPI) * U * sc * b


def epilogue_bound(b: np.ndarray) -> np.ndarray:
    """The c_epi part alone: what remains where the tap sum itself is exact."""
    return C_EPI * U * np.asarray(b, dtype=np.float64)


def within(z_gpu, z, bound) -> np.ndarray:
    """|err| / bound per output, the larger of the two components (0 where both are 0)."""
    z_gpu = np.asarray(z_gpu).astype(np.complex128)
    err = np.maximum(np.abs(z_gpu.real - z.real), np.abs(z_gpu.imag - z.imag))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, err / bound)


def same_bits(z_gpu, z) -> bool:
    """complex64(z) == z_gpu bit for bit, the sign of a zero aside (a conjugated or scaled zero sum is -0 in the kernel)."""
    want = np.asarray(z).astype(np.complex64).view(np.float32) + np.float32(0.0)
    got = np.asarray(z_gpu).astype(np.complex64, copy=False).view(np.float32) + np.float32(0.0)
    return want.shape == got.shape and np.array_equal(want.view(np.uint32), got.view(np.uint32))


def history_next(hist, raw, fmt: str, keep: int, n_frames: int) -> np.ndarray:
    """The numpy statement of iqa_history_update, in raw bytes: next = (hist | raw)[n_frames : n_frames + keep]; a missing
    history is the format's zero level (128 / 128 for u8)."""
    fb = FRAME_BYTES[fmt]
    zero = np.full(keep * fb, 128 if fmt == "u8" else 0, dtype=np.uint8)
    h = zero if hist is None else np.ascontiguousarray(hist).view(np.uint8).reshape(-1)
    r = np.zeros(0, dtype=np.uint8) if raw is None else np.ascontiguousarray(raw).view(np.uint8).reshape(-1)[:n_frames * fb]
    assert h.size == keep * fb and r.size == n_frames * fb
    return np.concatenate([h, r])[n_frames * fb:(n_frames + keep) * fb].copy()


# ---------------------------------------------------------------------------------------------------------------
# launch arithmetic


def tile_permutation(nblk: int) -> list[int]:
    """tile of block b (k_channelize_v1: per = nblk >> 3; identity for the last nblk % 8 blocks)."""
    per = nblk >> 3
    return [(b & 7) * per + (b >> 3) if b < per * XCDS else b for b in range(nblk)]


def classify(ntaps: int, decimation: int, n_frames: int, consumed: int, m_first: int, n_out: int, has_hist: bool) -> dict:
    """What iqa_channelize launches for this call and what the blocks of k_channelize_v1 do with it."""
    why = refusal(ntaps, decimation, n_frames, consumed, m_first, n_out)
    if why is not None or n_out == 0:
        return {"refused": why, "launched": False}
    L, D, lpad = ntaps, decimation, padded_len(ntaps)
    form = form_of(n_out)
    opb = CH_R if form == "splitk" else CH_OUT_PER_BLOCK
    nblk = -(-n_out // opb)
    slices = [(tc, min(CH_TCH, lpad - tc)) for tc in range(0, lpad, CH_TCH)]
    tiles = np.arange(nblk, dtype=np.int64)
    blk_first = (m_first + tiles * opb) * D - consumed - (L - 1)
    blk_last = blk_first + (opb - 1) * D
    interior = (blk_first >= 0) & (blk_last + lpad <= n_frames) & ((tiles + 1) * opb <= n_out)
    res = {
        "refused": None, "launched": True, "form": form, "outputs_per_block": opb, "blocks": nblk, "slices": len(slices),
        "permutation": tile_permutation(nblk), "interior": interior, "interior_blocks": int(interior.sum()),
        "edge_blocks": int((~interior).sum()), "continue_slices": {}, "break_slices": {},
        "guarded": 0, "guarded_hist": 0, "guarded_front_zero": 0, "guarded_behind": 0, "guarded_straddle": 0,
        "guarded_pad_only": 0, "vector_in_edge": 0,
    }
    for t in range(nblk):
        active, skipped, broken = [], [], []
        for k, (tc, cnt) in enumerate(slices):
            if not has_hist and blk_last[t] + tc + cnt <= 0:
                skipped.append(k)
                continue
            if blk_first[t] + tc >= n_frames:
                broken = list(range(k, len(slices)))
                break
            active.append((tc, cnt))
        if skipped:
            res["continue_slices"][t] = skipped
        if broken:
            res["break_slices"][t] = broken
        if interior[t] or not active:
            continue
        outs = np.arange(t * opb, min((t + 1) * opb, n_out), dtype=np.int64)
        start = (m_first + outs) * D - consumed - (L - 1)
        grp = np.concatenate([np.arange(tc, tc + cnt, 4, dtype=np.int64) for tc, cnt in active])
        f = start[:, None] + grp[None, :]  # first frame of every 4-frame group of every output
        guarded = ~((f >= 0) & (f + 4 <= n_frames))
        j = np.arange(4, dtype=np.int64)
        fj = f[:, :, None] + j  # the frames, where the tap is a real one
        real = (grp[None, :, None] + j) < L
        in_hist = real & (fj < 0) & (fj >= -(L - 1)) & has_hist
        front = real & (fj < 0) & ~in_hist
        behind = fj >= n_frames  # (an accepted call has only pad taps there: the group is guarded so that they are not read)
        in_raw = real & (fj >= 0) & (fj < n_frames)
        g3 = guarded
        res["guarded"] += int(g3.sum())
        res["vector_in_edge"] += int((~g3).sum())
        res["guarded_hist"] += int((g3 & in_hist.any(axis=2)).sum())
        res["guarded_front_zero"] += int((g3 & front.any(axis=2)).sum())
        res["guarded_behind"] += int((g3 & behind.any(axis=2)).sum())
        res["guarded_straddle"] += int((g3 & in_hist.any(axis=2) & in_raw.any(axis=2)).sum())
        res["guarded_pad_only"] += int((g3 & ~real.any(axis=2)).sum())
    return res


def tags(c: dict) -> set:
    """The paths of a classified call, as the names the case tables use."""
    if not c["launched"]:
        return {"refused"} if c["refused"] else {"nothing"}
    t = {c["form"]}
    if c["interior_blocks"]:
        t.add("interior")
    if c["edge_blocks"]:
        t.add("edge")
    if c["continue_slices"]:
        t.add("continue")
    if c["break_slices"]:
        t.add("break")
    if c["slices"] > 1:
        t.add("multi_slice")
    for key in ("guarded", "guarded_hist", "guarded_front_zero", "guarded_behind", "guarded_straddle", "guarded_pad_only", "vector_in_edge"):
        if c[key]:
            t.add(key)
    nblk = c["blocks"]
    t.add("perm_identity" if nblk < XCDS else ("perm_tail" if nblk % XCDS else "perm_whole"))
    return t


# ---------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_channelizer_shapes.py; tests/test_channelizer_model_host.py asserts the paths of each


@dataclass(frozen=True)
class Case:
    name: str
    ntaps: int
    decimation: int
    n_out: int
    m_first: int
    consumed: int
    n_frames: int
    has_hist: bool
    paths: frozenset  # what `tags(classify(...))` must contain
    fmts: tuple = FORMATS

    def classify(self) -> dict:
        return classify(self.ntaps, self.decimation, self.n_frames, self.consumed, self.m_first, self.n_out, self.has_hist)


def at_start(name: str, L: int, D: int, n_out: int, paths=(), fmts=FORMATS, tail: int = 0) -> Case:
    """From the start of a stream: no history, zeros in front; the last output's newest frame is n_frames - 1 - tail."""
    return Case(name, L, D, n_out, 0, 0, (n_out - 1) * D + 1 + tail, False, frozenset(paths), fmts)


def mid_stream(name: str, L: int, D: int, n_out: int, paths=(), fmts=FORMATS, consumed: int = 1001, skip: int = 0, tail: int = 0,
               n_frames: int | None = None) -> Case:
    """With a history: the first output is the first one of this block (+ skip), the last one's newest frame is
    n_frames - 1 - tail."""
    m_first = -(-consumed // D) + skip
    newest = (m_first + n_out - 1) * D - consumed
    return Case(name, L, D, n_out, m_first, consumed, newest + 1 + tail if n_frames is None else n_frames, True, frozenset(paths), fmts)


TAP_LIMIT_L = (1, 3, 4, 5, 255, 256, 257, 2047, 2048, 2049, 4097)
TAP_LIMIT_N_OUT = (1, 3, 4, 5, 29, 33, 37, 130)  # split-K blocks: 1, 1, 1, 2, 8, 9, 10, 33
TAP_LIMIT_BLOCKS = {1: 1, 3: 1, 4: 1, 5: 2, 29: 8, 33: 9, 37: 10, 130: 33}


def tap_limit_cases(L: int) -> list[Case]:
    """D = 1 around the padding (256) and slice (2048) limits, from the stream's start and with a history."""
    out = []
    for n_out in TAP_LIMIT_N_OUT:
        blocks = TAP_LIMIT_BLOCKS[n_out]
        perm = "perm_identity" if blocks < 8 else ("perm_tail" if blocks % 8 else "perm_whole")
        multi = {"multi_slice"} if L > CH_TCH else set()
        skipped = {"continue"} if L >= 4097 else set()  # (2049 taps: the first slice still reaches frame 3 of block 0)
        zeros = {"guarded_front_zero"} if L > 1 else set()
        hist = {"guarded_hist"} if L > 1 else set()
        out.append(at_start(f"start-L{L}-n{n_out}", L, 1, n_out, {"splitk", "edge", perm} | multi | skipped | zeros))
        out.append(mid_stream(f"hist-L{L}-n{n_out}", L, 1, n_out, {"splitk", "edge", perm} | multi | hist))
    return out


THROUGHPUT_L = (5, 257, 2049)
THROUGHPUT_D = (1, 3)
THROUGHPUT_N_OUT = (16383, 16384, 16384 + 32 * 3 + 5)


def throughput_cases(L: int, D: int) -> list[Case]:
    """Around the form switch: the same placement for the three lengths (m_first > 0, consumed no multiple of D, the first
    output one or two frames into the block, the last output's newest frame the block's last)."""
    head = {"guarded_hist", "guarded_straddle"}
    shared = {"edge", "interior", "guarded_behind", "vector_in_edge"} | head
    return [
        mid_stream(f"tp-L{L}-D{D}-n16383", L, D, 16383, {"splitk", "perm_whole"} | shared),
        mid_stream(f"tp-L{L}-D{D}-n16384", L, D, 16384, {"throughput", "perm_whole"} | shared),
        mid_stream(f"tp-L{L}-D{D}-n16485", L, D, 16485, {"throughput", "perm_tail"} | shared),
    ]


PLACEMENT_CASES = [
    mid_stream("place-L257-D2", 257, 2, 37, {"splitk", "guarded_hist", "guarded_straddle", "guarded_behind"}, skip=3),
    mid_stream("place-L5-D7", 5, 7, 29, {"splitk", "guarded_hist", "guarded_behind"}, consumed=1000),  # D > L: frames never read
    mid_stream("place-L257-D104", 257, 104, 33, {"splitk", "guarded_straddle", "perm_tail"}, skip=1, tail=3),
    mid_stream("place-L257-D521", 257, 521, 5, {"splitk", "guarded_straddle"}, tail=1),  # D > L
    mid_stream("place-L2049-D104", 2049, 104, 29, {"splitk", "multi_slice", "guarded_straddle", "perm_whole"}, skip=2),
    mid_stream("short-L2049-D7", 2049, 7, 100, {"splitk", "multi_slice", "guarded_hist", "guarded_straddle", "guarded_behind"}, n_frames=700),
    mid_stream("short-L4097-D2", 4097, 2, 130, {"splitk", "multi_slice", "guarded_hist", "guarded_behind"}, n_frames=300),
    mid_stream("one-frame-L255-D1", 255, 1, 1, {"splitk", "guarded_straddle"}, consumed=1000),
    mid_stream("one-frame-L2047-D7", 2047, 7, 1, {"splitk", "guarded_straddle"}),
    mid_stream("one-frame-L1-D1", 1, 1, 1, {"splitk", "guarded"}, consumed=1000),
]

LONG_CASES = [
    at_start("long-L6401-D104-start", 6401, 104, 41, {"splitk", "multi_slice", "continue", "guarded_front_zero"}),
    mid_stream("long-L6401-D104-hist", 6401, 104, 41, {"splitk", "multi_slice", "guarded_hist", "guarded_straddle"}),
    at_start("long-L32769-D208-start", 32769, 208, 41, {"splitk", "multi_slice", "continue", "guarded_front_zero"}, fmts=("s16", "f32")),
    mid_stream("long-L32769-D208-hist", 32769, 208, 41, {"splitk", "multi_slice", "guarded_hist", "guarded_straddle"}, fmts=("s16", "f32")),
]

CONJ_SCALE_CASE = mid_stream("conj-scale-L4097-D3", 4097, 3, 37, {"splitk", "multi_slice", "guarded_straddle", "perm_tail"})
SCALES = (1.0 + 0j, 1j, -1j)

ROTATION_M_FIRST = (0, 1, 2 ** 31 - 1, 2 ** 40 + 3)


def rotation_case(L: int, m_first: int) -> Case:
    """D = 3, 37 outputs from m_first on, one frame into the block (consumed = 3 m_first - 1 where m_first > 0)."""
    D, n_out = 3, 37
    consumed = max(0, m_first * D - 1)
    newest = (m_first + n_out - 1) * D - consumed
    return Case(f"rot-L{L}-m{m_first}", L, D, n_out, m_first, consumed, newest + 1, True, frozenset({"splitk"}))


def all_cases() -> list[Case]:
    out = [c for L in TAP_LIMIT_L for c in tap_limit_cases(L)]
    out += [c for L in THROUGHPUT_L for D in THROUGHPUT_D for c in throughput_cases(L, D)]
    out += PLACEMENT_CASES + LONG_CASES + [CONJ_SCALE_CASE]
    out += [rotation_case(L, m) for L in (1, 5) for m in ROTATION_M_FIRST]
    return out


# exact data ------------------------------------------------------------------------------------------------------

X_MAX = {"s16": 100, "f32": 100, "u8": 128}  # |x| of the generated frames (u8: whatever a byte holds)
HOSTILE = {"s16": (32767, -32767), "u8": (255, 255), "f32": (np.nan, np.nan)}  # (I, Q) around the views


def tap_limit(ntaps: int, fmt: str) -> int:
    """Largest |g| <= 3 with 2 L |g| |x| < 2^24."""
    return int(min(3, (2 ** 24 - 1) // (2 * ntaps * X_MAX[fmt])))


def assert_exact(taps: np.ndarray, ntaps: int, *streams_c128) -> None:
    """The condition of an exact case, on the data itself: integers, dense taps, zero pad, 2 L max|g| max|x| < 2^24."""
    g = np.asarray(taps)
    assert g.dtype == np.complex64 and g.size == padded_len(ntaps)
    assert not g[ntaps:].any(), "pad taps must be zero"
    assert np.all(g.real[:ntaps] != 0) and np.all(g.imag[:ntaps] != 0), "taps must be dense"
    assert np.array_equal(g.real, np.rint(g.real)) and np.array_equal(g.imag, np.rint(g.imag))
    gmax = float(max(np.abs(g.real).max(), np.abs(g.imag).max()))
    xmax = 0.0
    for v in streams_c128:
        if v is None or v.size == 0:
            continue
        assert np.array_equal(v.real, np.rint(v.real)) and np.array_equal(v.imag, np.rint(v.imag))
        xmax = max(xmax, float(np.abs(v.real).max()), float(np.abs(v.imag).max()))
    assert 2 * ntaps * gmax * xmax < 2 ** 24, (ntaps, gmax, xmax)


def exact_data(case: Case, fmt: str, seed: int = 5):
    """(taps complex64[Lpad], raw, hist or None) of an exact case, the 2^24 condition asserted."""
    rng = np.random.default_rng([seed, case.ntaps, case.decimation, case.n_out, FMT_CODE[fmt]])
    L, gmax = case.ntaps, tap_limit(case.ntaps, fmt)
    assert gmax >= 1, (L, fmt)
    taps = np.zeros(padded_len(L), dtype=np.complex64)
    mag = rng.integers(1, gmax + 1, size=(2, L))
    sign = rng.integers(0, 2, size=(2, L)) * 2 - 1
    taps[:L] = (mag[0] * sign[0]) + 1j * (mag[1] * sign[1])

    def block(n):
        if fmt == "u8":
            return rng.integers(0, 256, size=2 * n).astype(np.uint8)
        return rng.integers(-X_MAX[fmt], X_MAX[fmt] + 1, size=2 * n).astype(FMT_DTYPE[fmt])

    raw = block(case.n_frames)
    hist = block(L - 1) if case.has_hist else None
    assert_exact(taps, L, frames(raw, fmt), None if hist is None else frames(hist, fmt))
    return taps, raw, hist
