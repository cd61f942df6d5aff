"""Exact host model of the int8 matrix-core channelizer kernels (csrc/channelize_mfma.hip, csrc/channelize_ring.hip,
csrc/mfma_common.h).

Every output of those kernels is an exact integer sum followed by a fixed, explicitly rounded float64 emission, so with
``rotate = 0`` a correct kernel's output is determined bit for bit by its inputs.  This module states that arithmetic:

  data rows        X[b][kap] = v[2 (b D + 1 - consumed) + kap]      (raw interleaved values; row b = frames bD+1 .. bD+D)
  tap rows         T[row][kap] = 256 q1 + q2 (dsp_plan.plan_mfma: ``group.tq``), row = comp*64 + (qq - 1)
  int16 data       v = 256 hi + lo' + 128:   S1 = sum q1 hi,   S2 = sum q1 lo' + q2 hi   (q2 lo' dropped, as the kernels do)
  uint8 data       one piece d = u ^ 0x80 = u - 128:   S1 = sum q1 d,   S2 = sum q2 d
  output m         tap row qq of group q meets data row m - 64 q - qq, qq = 1..64

The sums are a float64 GEMM of data rows x tap rows followed by a diagonal gather.  That is exact: every product
(|q| <= 128, |data byte| <= 128) and every partial sum is an integer far below 2^53, in any summation order.

Emission (``mfma_scaled_sum``): v = 256 S1 + S2 -- kept in one int32 by the ring kernels with int32 sums (which wrap on
overflow; ``dsp_plan.plan_mfma(acc32=True)`` guarantees they never do), formed in double from the separate sums by the
per-lane kernel and the ring kernels with 64-bit sums -- then (256 v + c) * unit: 256 v + c is an exact integer (< 2^53),
so the three forms are one rounding of the same value.  uint8: unit = tap LSB / 256, c = 0.  Passes chain with one
float64 add each, in pass order; ``iqa_mfma_combine`` scales raw int32 partials the same way and adds them in group
order.  Then conjugation, rotation by the exact uint64 phase rot_base + m rot_step ((ph >> 11) / 2^53 turns, float64),
out_scale (1, j or -j: exact) and one float32 rounding (``mfma_finish``).

Test infrastructure only: the package never imports it.
"""
from __future__ import annotations

import numpy as np

Q = 64  # tap rows per group and output component
TWO53 = float(2**53)
_CHUNK = 8192  # outputs per GEMM (bounds the host memory of the data-row matrix)


def split_taps(tq: np.ndarray):
    """(q1, q2): T = 256 q1 + q2 with both bytes signed (the fragments' two pieces)."""
    t = np.asarray(tq, dtype=np.int64)
    q2 = ((t + 128) & 255) - 128
    return (t - q2) >> 8, q2


def data_pieces(raw: np.ndarray, fmt: str):
    """The kernels' int8 data pieces of the interleaved raw values: int16 -> (hi, lo'), uint8 -> (u - 128,)."""
    if fmt == "s16":
        v = np.asarray(raw).astype(np.int64)
        lo = (v & 255) - 128
        hi = (v - lo - 128) >> 8
        return hi, lo
    if fmt == "u8":
        return (np.asarray(raw).astype(np.int64) - 128,)
    raise ValueError(f"the matrix-core kernels take s16 and u8 captures, not {fmt!r}")


def pass_sums(tq: np.ndarray, raw: np.ndarray, fmt: str, decimation: int, q: int, k_first: int, k_count: int,
              consumed: int, m_first: int, n_out: int):
    """(S1, S2): int64 [n_out, 2] (columns re, im) -- the integer sums one pass of tap-row group ``q`` over k steps
    [k_first, k_first + k_count) forms for outputs m_first .. m_first + n_out - 1.  ``raw``: the interleaved values the
    kernel reads, frame 0 of which has global index ``consumed``.  Values outside ``raw`` only ever meet zero taps (the K
    padding of a row's last k step); a non-zero tap that reaches outside raises ValueError."""
    D = int(decimation)
    pieces = data_pieces(raw, fmt)
    q1, q2 = split_taps(np.asarray(tq)[:, 32 * k_first : 32 * (k_first + k_count)])
    K = q1.shape[1]
    real_cols = max(0, min(K, 2 * D - 32 * k_first))  # columns that carry taps (the rest of the last k step is padding)
    if np.any(q1[:, real_cols:]) or np.any(q2[:, real_cols:]):
        raise ValueError("taps in the K padding")
    # weights of one GEMM [X_hi | X_lo] @ W: columns 0..127 -> S1 rows, 128..255 -> S2 rows (uint8: [X_d] @ [q1 | q2])
    if fmt == "s16":
        w = np.zeros((2 * K, 256))
        w[:K, :128] = q1.T
        w[:K, 128:] = q2.T
        w[K:, 128:] = q1.T
    else:
        w = np.concatenate([q1.T, q2.T], axis=1).astype(np.float64)
    n_vals = int(np.asarray(raw).size)
    b0 = m_first - Q * q - Q  # data row of relative row 0
    first = 2 * (b0 * D + 1 - consumed) + 32 * k_first  # value index of row 0, column 0
    last_row = b0 + n_out + Q - 2
    hi_val = 2 * (last_row * D + 1 - consumed) + 32 * k_first + max(real_cols, 1) - 1
    if n_out > 0 and (first < 0 or hi_val >= n_vals):
        raise ValueError(f"pass reads values [{first}, {hi_val}] outside the capture [0, {n_vals})")
    pad_back = max(0, 2 * (last_row * D + 1 - consumed) + 32 * k_first + K - n_vals)
    padded = [np.concatenate([p.astype(np.float64), np.zeros(pad_back)]) for p in pieces]
    s1 = np.zeros((n_out, 2), dtype=np.int64)
    s2 = np.zeros((n_out, 2), dtype=np.int64)
    for i0 in range(0, n_out, _CHUNK):
        n = min(_CHUNK, n_out - i0)
        rows = n + Q - 1
        start = first + 2 * D * i0
        views = [np.lib.stride_tricks.as_strided(p[start:], shape=(rows, K), strides=(2 * D * 8, 8)) for p in padded]
        g = np.concatenate(views, axis=1) @ w  # [rows, 256]; every entry an exact integer
        acc = np.zeros((n, 4))
        for qq in range(1, Q + 1):
            sl = g[Q - qq : Q - qq + n]
            acc += sl[:, [qq - 1, Q + qq - 1, 128 + qq - 1, 128 + Q + qq - 1]]
        assert np.all(np.abs(acc) < TWO53)
        acc = acc.astype(np.int64)
        s1[i0 : i0 + n] = acc[:, 0:2]
        s2[i0 : i0 + n] = acc[:, 2:4]
    return s1, s2


def wrap32(v: np.ndarray) -> np.ndarray:
    """int64 -> the int32 a 32-bit accumulator holds (two's complement wrap)."""
    return ((np.asarray(v, dtype=np.int64) + 2**31) % 2**32) - 2**31


def ring_value(s1: np.ndarray, s2: np.ndarray, acc32: bool) -> np.ndarray:
    """v = 256 S1 + S2 per component, int64 [n, 2]: what the kernels hand to the emission (``acc32``: the one int32 of
    the ring kernels with int32 sums -- also what a lane with raw_partials stores)."""
    v = 256 * np.asarray(s1, dtype=np.int64) + np.asarray(s2, dtype=np.int64)
    return wrap32(v) if acc32 else v


def scaled_sum(v: np.ndarray, c: float, unit: float) -> np.ndarray:
    """``mfma_scaled_sum``: (256 v + c) * unit, float64 -- exact up to the one rounding of the product."""
    x = np.asarray(v, dtype=np.int64).astype(np.float64) * 256.0 + float(c)
    assert np.all(np.abs(x) < TWO53)
    return x * float(unit)


def lane_unit(mp, gi: int, fmt: str) -> float:
    """The ``unit`` a lane / pass of group ``gi`` takes (uint8: the tap LSB / 256, as the host passes it)."""
    return float(mp.groups[gi].unit) / (256.0 if fmt == "u8" else 1.0)


def pass_partial(mp, ps, raw, fmt: str, decimation: int, consumed: int, m_first: int, n_out: int, acc32: bool,
                 afrag_tq=None):
    """(v int64 [n, 2], d float64 [n, 2]): one pass's integer sums and their emission ``(256 v + c) * unit``.
    ``afrag_tq``: taps to use instead of the group's own (a test may perturb what it uploads)."""
    grp = mp.groups[ps.group]
    tq = grp.tq if afrag_tq is None else afrag_tq
    s1, s2 = pass_sums(tq, raw, fmt, decimation, grp.q, ps.k_first, ps.k_count, consumed, m_first, n_out)
    v = ring_value(s1, s2, acc32)
    d = np.stack([scaled_sum(v[:, 0], ps.c_re, lane_unit(mp, ps.group, fmt)),
                  scaled_sum(v[:, 1], ps.c_im, lane_unit(mp, ps.group, fmt))], axis=1)
    return v, d


def chain(parts) -> np.ndarray:
    """Partials added one float64 add at a time, in the given order (``partial_in`` chaining, ``iqa_mfma_combine``)."""
    parts = list(parts)
    d = parts[0].copy()
    for p in parts[1:]:
        d = p + d
    return d


def plan_sums(mp, raw, fmt: str, decimation: int, consumed: int, m_first: int, n_out: int, acc32: bool) -> np.ndarray:
    """float64 [n, 2]: every pass of the plan emitted and chained in pass order (the single-channel passes)."""
    return chain(pass_partial(mp, ps, raw, fmt, decimation, consumed, m_first, n_out, acc32)[1] for ps in mp.passes)


def rotation(m: np.ndarray, rot_step: int, rot_base: int):
    """(cos, sin) of the output rotation, float64: the exact uint64 phase rot_base + m rot_step, (ph >> 11) / 2^53 turns."""
    m = np.asarray(m, dtype=np.uint64)
    ph = np.uint64(int(rot_base) % 2**64) + m * np.uint64(int(rot_step) % 2**64)  # wraps mod 2^64
    turns = (ph >> np.uint64(11)).astype(np.float64) * (1.0 / TWO53)
    return np.cos(2.0 * np.pi * turns), np.sin(2.0 * np.pi * turns)


def finish(d: np.ndarray, m_first: int, conj_sum: int, rotate: int, rot_step: int = 0, rot_base: int = 0,
           out_scale: complex = 1.0, cast: bool = True) -> np.ndarray:
    """``mfma_finish``: conjugation, rotation, out_scale (1, j, -j), then ONE rounding to complex64 (``cast=False``:
    complex128, for comparisons with an unquantised reference)."""
    re, im = d[:, 0].copy(), d[:, 1].copy()
    if conj_sum:
        im = -im
    if rotate:
        cw, sw = rotation(np.arange(m_first, m_first + len(re), dtype=np.uint64), rot_step, rot_base)
        re, im = re * cw - im * sw, re * sw + im * cw
    sr, si = float(np.float32(np.real(out_scale))), float(np.float32(np.imag(out_scale)))
    if (sr, si) not in ((1.0, 0.0), (0.0, 1.0), (0.0, -1.0)):
        raise ValueError("out_scale is one of 1, j, -j")
    zr, zi = re * sr - im * si, re * si + im * sr
    if not cast:
        return zr + 1j * zi
    z = np.empty(len(zr), dtype=np.complex64)
    z.real = zr.astype(np.float32)
    z.imag = zi.astype(np.float32)
    return z
