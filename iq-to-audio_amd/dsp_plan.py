"""Host-side planning for the hot path (float64 / exact-integer scalar logic, no device work).

Mirrors the scalar rules of the reference's ``processing.py`` (chunk tuning, decimation
choice, Kaiser channel filter) and adds what the fused GPU channelizer needs: complex
taps pre-rotated by the NCO, the 64-bit fixed-point output rotation, and the folding
of ``iq_order`` into taps/flags so that the kernel's inner loop is a plain dot product.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

MAX_CHUNK = 4_194_304
TWO64 = 1 << 64
IQ_ORDERS = ("iq", "qi", "iq_inv", "qi_inv")
INGEST_SCALE = {"s16": 1.0 / 32768.0, "u8": 1.0 / 128.0, "f32": 1.0}
FMT_CODE = {"s16": 0, "u8": 1, "f32": 2}
FMT_NUMPY = {"s16": np.int16, "u8": np.uint8, "f32": np.float32}


#: (minimum sample rate, seconds of signal a chunk should hold), highest rate first -- reference processing.py:69-72
_CHUNK_SECONDS = ((5_000_000.0, 0.50), (2_000_000.0, 0.40), (0.0, 0.25))


def tune_chunk_size(sample_rate: float, requested: int) -> int:
    """Effective chunk length (reference processing.py:65-81): the requested one unless the rate calls for more --
    then the next power of two holding 0.25 s of signal (0.40 s from 2 MS/s, 0.50 s from 5 MS/s), never below the
    request and never above 4 Mi frames.

    The result is *semantic*, not a memory knob here: it fixes where the SSB AGC gain
    restarts and which prefix ``choose_mix_sign`` inspects.
    """
    floor = max(1, requested)
    if sample_rate <= 0:
        return floor
    seconds = next(s for rate, s in _CHUNK_SECONDS if sample_rate >= rate)
    wanted = int(round(sample_rate * seconds))
    if wanted <= floor:
        return floor
    wanted = min(wanted, MAX_CHUNK)
    return int(min(max(1 << (wanted - 1).bit_length(), floor), MAX_CHUNK))


def choose_decimation(sample_rate: float, fs_ch_target: float) -> tuple[int, float]:
    """(D, fs_channel) (reference processing.py:885-890; Python round = half-to-even)."""
    decimation = max(1, int(round(sample_rate / fs_ch_target)))
    fs_channel = sample_rate / decimation
    if fs_channel > fs_ch_target * 1.5:
        decimation = max(int(math.floor(sample_rate / fs_ch_target)), 1)
        fs_channel = sample_rate / decimation
    return decimation, fs_channel


def kaiser_beta(atten_db: float) -> float:
    """Kaiser's empirical beta(A) formula (what scipy.signal.kaiser_beta evaluates)."""
    a = abs(atten_db)
    if a > 50:
        return 0.1102 * (a - 8.7)
    if a > 21:
        return 0.5842 * (a - 21) ** 0.4 + 0.07886 * (a - 21)
    return 0.0


def design_channel_filter(sample_rate: float, bandwidth: float, decimation: int) -> np.ndarray:
    """Kaiser-windowed low-pass, float64, unity DC gain (reference processing.py:599-620).

    Same design rule as the reference (taps = clip(4*fs/max(1000, bw/2), 1024, 32768) made
    odd; cutoff = min(0.525*bw, 0.9*fs/(2D)); 80 dB Kaiser), evaluated directly with NumPy:
    h[n] = 2fc/fs * sinc(2fc/fs * (n - (N-1)/2)) * kaiser(N, beta), normalised to sum 1 --
    the windowed-sinc construction scipy.signal.firwin documents for a single low-pass band.
    """
    guard = max(1_000.0, bandwidth * 0.5)
    cutoff = min(bandwidth * 0.5 * 1.05, (sample_rate / (2.0 * max(decimation, 1))) * 0.9)
    if cutoff <= 0:
        raise ValueError("Invalid cutoff frequency for channel filter.")
    width = guard / sample_rate
    num_taps = int(np.clip(4.0 / max(width, 1e-8), 1024, 32768))
    if num_taps % 2 == 0:
        num_taps += 1
    beta = kaiser_beta(80.0)
    fc = cutoff / (0.5 * sample_rate)  # relative to Nyquist
    m = np.arange(num_taps, dtype=np.float64) - (num_taps - 1) / 2.0
    h = fc * np.sinc(fc * m) * np.kaiser(num_taps, beta)
    return np.asarray(h / h.sum(), dtype=np.float64)


def freq_ratio_turns(freq_offset: float, sample_rate: float, sign: int) -> int:
    """NCO phase advance per input sample as a 64-bit fraction of a turn.

    The reference mixes with exp(j*sign*inc*n), inc = -2*pi*f_off/fs (processing.py:287,293),
    i.e. -sign*f_off/fs turns per sample.  Floats are exact rationals, so the ratio is
    formed exactly and rounded once to 2^-64 turn.
    """
    theta = -sign * Fraction(freq_offset) / Fraction(sample_rate)
    theta -= math.floor(theta)
    return int(round(theta * TWO64)) % TWO64


@dataclass
class ChannelPlan:
    """Everything the fused channelizer kernel needs for one channel."""

    fmt: str
    ntaps: int
    decimation: int
    taps_window: np.ndarray  # complex64 [Lpad], window order, ingest scale folded in
    conj_sum: int
    rotate: int
    rot_step: int
    rot_base: int
    out_scale: complex
    taps_natural: np.ndarray | None = None  # complex128 [L], natural order g[k] (same folding), for the MFMA planner
    nco_step: int = 0  # NCO advance per input sample, 2^-64 turns: g[k] = h[k] e^{-+j 2 pi nco_step k / 2^64} (the MFMA planner's in-band gain)


def plan_channel(
    taps: np.ndarray,
    *,
    sample_rate: float,
    freq_offset: float,
    mix_sign: int,
    decimation: int,
    fmt: str = "s16",
    iq_order: str = "iq",
    padded_len: int | None = None,
) -> ChannelPlan:
    """Fold NCO + iq_order + ingest scale into complex taps and output-rotation constants.

    mix -> filter -> decimate of the reference equals
        z[m] = e^{-j 2 pi theta m D} * sum_k (h[k] e^{+j 2 pi theta k}) x[mD - k],
    theta = -sign*f_off/fs turns/sample ... with the sign convention below:
    the mixer multiplies sample n by e^{+j 2 pi W n / 2^64}; pulling e^{+j 2 pi W (mD)}
    out of the sum leaves taps g[k] = h[k] e^{-j 2 pi W k / 2^64}.
    """
    if iq_order not in IQ_ORDERS:
        raise ValueError(f"Unsupported iq_order '{iq_order}'")
    if fmt not in FMT_CODE:
        raise ValueError(f"unsupported sample format {fmt!r}")
    h = np.asarray(taps, dtype=np.float64)
    ntaps = h.size
    w = freq_ratio_turns(freq_offset, sample_rate, mix_sign)
    k = np.arange(ntaps, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ph = np.uint64(w) * k  # wraps mod 2^64 == mod one turn
    turns = (ph >> np.uint64(11)).astype(np.float64) * (2.0**-53)
    g = h * np.exp(-2j * np.pi * turns)
    # raw frame r = a + jb (a = first value of the pair).  x = c*r or c*conj(r):
    #   iq: r | qi: j*conj(r) | iq_inv: conj(r) | qi_inv: -j*r      (IQReader._extract_iq)
    conj = iq_order in ("qi", "iq_inv")
    c = {"iq": 1.0 + 0j, "qi": 1j, "iq_inv": 1.0 + 0j, "qi_inv": -1j}[iq_order]
    if conj:
        g = np.conj(g)  # sum g*conj(r) = conj(sum conj(g)*r)
    g = g * INGEST_SCALE[fmt]
    lpad = padded_len if padded_len is not None else -(-ntaps // 256) * 256
    win = np.zeros(lpad, dtype=np.complex64)
    win[:ntaps] = g[::-1].astype(np.complex64)  # window order: win[i] multiplies x[n0-(L-1)+i]
    return ChannelPlan(
        fmt=fmt, ntaps=ntaps, decimation=int(decimation), taps_window=win, conj_sum=int(conj), rotate=1,
        rot_step=(w * int(decimation)) % TWO64, rot_base=0, out_scale=c, taps_natural=g.astype(np.complex128), nco_step=w,
    )


MFMA_Q = 64  # q slots (tap rows) per pass and output component in the int8-MFMA kernel
MFMA_KSTEP_BYTES = 8192  # tap fragments per k step: 4 row tiles x 2 pieces x 64 lanes x 16 B
MFMA_MAX_KSTEPS_PER_PASS = 16  # 128 KiB of fragments leaves room for >= 1888 outputs of accumulators in LDS


@dataclass
class MfmaGroup:
    """Tap rows 64*q+1 .. 64*q+64 of the filter (or, ``residual``, what an earlier group left of them), quantised on
    their own scale."""

    afrag: np.ndarray  # int8 [ksteps, 4, 2, 64, 16] tap fragments in MFMA lane order
    unit: float  # value of one tap LSB
    tq: np.ndarray  # int32 [128, Kpad] quantised taps T = 256*q1 + q2
    q: int = 0  # tap-row group (the data rows a lane of this group streams start 64*q rows earlier)
    residual: bool = False  # the taps of this group are the quantisation residue of the group in front of it
    high_only: bool = False  # every low tap byte q2 is zero: the ring kernels skip the q2*hi product (two MFMAs per k step)
    #: ``rot`` != 0 (int32-sum groups of int16 plans, ``zero_high_rotation``): ``afrag_rot`` holds the same fragments with the
    #: rows of either component rotated by ``rot`` slots -- slot s holds tap row (s - rot) mod 64 -- so that slots 0..15 are
    #: rows whose high tap byte q1 is zero throughout; the half-step ring kernel then skips their q1 products.
    rot: int = 0
    afrag_rot: np.ndarray | None = None


@dataclass
class MfmaPass:
    group: int  # index into MfmaPlan.groups
    k_first: int
    k_count: int
    c_re: float  # 128 * sum(T) over the real-output rows and this pass's k range (low-byte bias)
    c_im: float


@dataclass
class MfmaPlan:
    """Host-side operands of ``iqa_channelize_mfma`` (see csrc/channelize_mfma.hip)."""

    ksteps: int
    groups: list
    passes: list
    err_norm: float = 0.0  # sqrt(sum_k |T_k u - g_k|^2) per unit of full scale: the z error for a white input of unit RMS
    #: The part of the z error that does NOT scale with the input: the q2*lo' products the int16 kernels drop (low tap
    #: byte x low data byte; uint8 captures drop nothing: all three are 0).  Three figures, fractions of full scale:
    #: ``floor_rms`` -- its RMS for data whose low bytes are uniform and independent of the taps (noise of some tens of LSB
    #: and more: measured 1.0x at 300 and 3000 LSB, 1.4x at 30 LSB).
    floor_rms: float = 0.0
    #: ``zero_rms`` -- |z| of the zero-input response, EXACT: an all-zero capture has lo' = -128 everywhere, so the kernels
    #: emit the constant 128 * unit * sum(q2) per output component (summed over the plan's groups) where the filter gives
    #: 0.  It is what any stretch of a capture costs whose values stand still within one byte -- silence, a DC offset, the
    #: quiet half of a keyed signal, a clean carrier whose phase turns slowly against the filter length -- at ANY level
    #: estimate, so ``z_error_rms`` and the precision guard always apply it.  sum(q2) is the DC gain of the low tap bytes:
    #: where |T| < 128 (the tails of a Kaiser design) q2 IS the tap, so at offset 0 it is ~18x ``floor_rms``; away from
    #: offset 0 the NCO turns the taps and it is of the order of ``floor_rms`` or below.
    zero_rms: float = 0.0
    #: ``coherent_rms`` -- the bound for a QUIET capture (see ``QUIET_WIDEBAND``) whose content is a clean signal in the
    #: channel: for |v| < 128 the low byte is lo' = v - 128 sgn(v), i.e. the signal itself minus a square wave of 128 LSB
    #: in step with it, whose fundamental (4/pi * 128) the low tap bytes pass with their gain at the channel centre:
    #: (4/pi) * 128 * |sum_k unit * g2[k] e^{+-j 2 pi nco_step k}|, g2 the complex low-byte taps.  A constant-envelope
    #: signal of A LSB measures |1 - A / 163| of it (D = 104, +1 MHz: 1.10e-5 at 46 LSB, 6.4e-6 at 100 against 1.16e-5 and
    #: 6.2e-6 predicted).
    coherent_rms: float = 0.0

    # single-pass conveniences (tests, and the common ceil(L/D) <= 64, D <= 256 case)
    @property
    def afrag(self):
        return self.groups[0].afrag

    @property
    def unit(self):
        return self.groups[0].unit

    @property
    def tq(self):
        return self.groups[0].tq

    @property
    def c_re(self):
        return sum(p.c_re for p in self.passes if p.group == 0)

    @property
    def c_im(self):
        return sum(p.c_im for p in self.passes if p.group == 0)

    def floors(self) -> tuple:
        """(floor_rms, zero_rms, coherent_rms): the operands of ``dropped_floor``."""
        return float(self.floor_rms), float(self.zero_rms), float(self.coherent_rms)

    def z_error_rms(self, wideband_rms: float) -> float:
        """Expected RMS error of z for a capture of the given wideband RMS (fraction of full scale): tap rounding x level
        and the level-independent floor of the dropped products (``dropped_floor``)."""
        return math.hypot(self.err_norm * wideband_rms, dropped_floor(self.floors(), wideband_rms))


#: Wideband RMS (fraction of the KERNEL's full scale) below which a capture counts as quiet: 128 LSB of an int16.  A
#: constant-envelope signal of that level is the largest whose I and Q never leave the two bytes around zero, which is
#: what makes lo' = v - 128 sgn(v) coherent with it.  Exact-model sweep (tests/test_guard_model_host.py; D = 104, clean NFM,
#: 1 LSB of noise; audio RMS error of "fast" against the float64 chain, bar 1e-4), at offset 0 / +1 MHz:
#:   46 LSB 2.2e-4 / 1.7e-4, 64 LSB 1.3e-4 / 1.0e-4, 80 LSB 9.3e-5, 100 LSB 6.2e-5 / 4.6e-5, 128 LSB 3.7e-5 / 2.5e-5,
#:   160 LSB 2.5e-5 / 1.5e-5, 200 LSB 2.7e-5 / 1.7e-5.
#: D = 521 at +2.2 MHz (the plan of the sweep whose zero-input response is smallest, so that nothing else catches it):
#:   64 LSB 1.5e-4, 80 LSB 1.1e-4, 100 LSB 8.1e-5, 128 LSB 5.8e-5, 160 LSB 4.4e-5, 200 LSB 3.7e-5.
#: The bar is crossed between 64 and 100 LSB; at 128 LSB and above "fast" keeps it with a margin of 1.7 and more.
QUIET_WIDEBAND = 2.0**-8


def dropped_floor(floors, kernel_wideband_rms: float) -> float:
    """The level-independent part of the int16 kernels' z error, in units of the kernel's full scale, for a capture of
    wideband RMS ``kernel_wideband_rms`` (same units).  ``floors``: ``MfmaPlan.floors()``.  The uniform-low-byte RMS and
    the zero-input response hold at every level (a level estimate says nothing about the quiet stretches of a capture);
    the coherent bound joins them below ``QUIET_WIDEBAND``."""
    floor_rms, zero_rms, coherent_rms = floors
    worst = max(floor_rms, zero_rms)
    return max(worst, coherent_rms) if kernel_wideband_rms < QUIET_WIDEBAND else worst


def mfma_supported(plan: ChannelPlan) -> bool:
    """int16 captures (every matrix-core kernel) and uint8 captures (the row-staged ring kernel only)."""
    return plan.fmt in ("s16", "u8") and plan.taps_natural is not None


@functools.lru_cache(maxsize=32)
def _mfma_layout(ntaps: int, decimation: int, group: int):
    """Index tables of the tap-fragment layout; they depend only on (L, D, q-group)."""
    L, D = ntaps, decimation
    ksteps = -(-2 * D // 32)
    q = np.arange(1, MFMA_Q + 1, dtype=np.int64)[:, None] + MFMA_Q * group
    rho = np.arange(D, dtype=np.int64)[None, :]
    k = q * D - 1 - rho
    ok = (k >= 0) & (k < L)
    kc = np.clip(k, 0, L - 1)
    lane = np.arange(64)
    rows = (np.arange(4) * 32)[:, None] + (lane & 31)[None, :]  # [rt, lane]
    cols = (32 * np.arange(ksteps))[:, None, None] + (16 * (lane >> 5))[None, :, None] + np.arange(16)[None, None, :]
    flat = (rows[None, :, :, None] * (32 * ksteps) + cols[:, None, :, :]).astype(np.int64)  # [ks, rt, lane, j]
    return ksteps, kc, ok, flat


_LOW_BYTE_VAR = (256.0 * 256.0 - 1.0) / 12.0  # variance of a uniform low data byte lo' in [-128, 127]


def _quantise_rows(a: np.ndarray, acc32: bool, high_byte_only: bool, col_ranges=None):
    """(unit, T, q1, q2) for one 128-row tap matrix: T = rint(a / unit) = 256*q1 + q2 with both bytes signed,
    unit = max|a| / 32639 -- enlarged, with ``acc32``, until 256*S1 + S2 of a component cannot overflow an int32
    for ANY int16 input (``col_ranges``: the column ranges that are summed into one int32 -- a pass of the kernel covers
    one k-step range and hands its sum on in float64).  ``high_byte_only``: q2 = 0 (T a multiple of 256): the int16
    kernels then drop nothing -- their q2*lo' term is identically zero -- at the price of taps of ~6 bits."""
    amax = float(np.abs(a).max())
    unit = amax / 32639.0 if amax > 0 else 1.0
    while True:
        if high_byte_only:
            q1 = np.clip(np.rint(a * (1.0 / (256.0 * unit))), -127, 127).astype(np.int32)
            q2 = np.zeros_like(q1)
            t = q1 << 8
        else:
            t = np.rint(a * (1.0 / unit)).astype(np.int32)
            q2 = ((t + 128) & 255) - 128
            q1 = (t - q2) >> 8
        if not acc32:
            break
        # |256*S1 + S2| <= sum 128*(257|q1| + |q2|) over one component's rows (|hi|, |lo'| <= 128)
        w = 128 * (257 * np.abs(q1).astype(np.int64) + np.abs(q2))
        bound = max(int(w[r, c0:c1].sum()) for r in (slice(0, MFMA_Q), slice(MFMA_Q, 2 * MFMA_Q))
                    for c0, c1 in (col_ranges or [(0, a.shape[1])]))
        if bound < 2**31 - 1:
            break
        unit *= max(1.02, bound / (2**31 - 1) * 1.001)
    return unit, t, q1, q2


def zero_high_runs(q1: np.ndarray) -> list:
    """Per component (re, im) of a 128-row high-byte matrix: (first row, length) of the largest CYCLIC run of rows whose q1
    is zero throughout (rows past the filter's end are such rows); (0, 64) if all are, (0, 0) if none is."""
    runs = []
    for comp in range(2):
        z = ~np.any(q1[comp * MFMA_Q : (comp + 1) * MFMA_Q], axis=1)
        if z.all():
            runs.append((0, MFMA_Q))
            continue
        best, start, length = (0, 0), 0, 0
        for i in range(2 * MFMA_Q):  # twice around: a run that wraps is met whole
            if z[i % MFMA_Q]:
                if length == 0:
                    start = i % MFMA_Q
                length += 1
                if length > best[1]:
                    best = (start, length)
            else:
                length = 0
        runs.append(best)
    return runs


def zero_high_rotation(q1: np.ndarray) -> int:
    """The slot shift that puts the first 16 rows of the largest cyclic zero-q1 run into slots 0..15 of either component
    (slot s holds tap row (s - rot) mod 64); 0 = not rotated: the run is shorter than 16 rows in a component, the two
    components' runs differ, or the run starts at row 0 already."""
    (s_re, n_re), (s_im, n_im) = zero_high_runs(q1)
    if min(n_re, n_im) < 16 or (s_re, n_re) != (s_im, n_im):
        return 0
    return (MFMA_Q - s_re) % MFMA_Q


def rotate_rows(x: np.ndarray, rot: int) -> np.ndarray:
    """Rows of a [128, ...] tap matrix with either component rotated by ``rot`` slots: out[comp*64 + s] = x[comp*64 + (s - rot) % 64]."""
    s = (np.arange(MFMA_Q) - rot) % MFMA_Q
    return x[np.concatenate([s, MFMA_Q + s])]


def plan_mfma(plan: ChannelPlan, acc32: bool = False, max_ksteps: int | None = None, residual: bool = False) -> MfmaPlan:
    """Quantise the (already NCO-rotated, scaled) taps to 16-bit fixed point and lay them out as
    the A operand of v_mfma_i32_32x32x32_i8.

    ``acc32``: the ring kernel keeps 256*S1 + S2 of an output component in ONE int32.  The tap unit is then
    enlarged (taps of ~14 bits for the standard 12.5 kHz filters) until
    sum_k 128*(257|q1_k| + |q2_k|) < 2^31 over the rows of a component, so that the sum cannot overflow for
    ANY int16 input; everything stays exact integer arithmetic.

    ``residual`` (the "fine" precision of the pipeline): every tap-row group becomes TWO groups that stream the same data
    rows -- the taps themselves and what their quantisation left over, quantised again on a unit of its own (~1/20 of
    the first one's LSB under the int32 bound) -- whose partial sums ``iqa_mfma_combine`` adds.  For int16 captures the
    first of the two keeps the high tap byte only: the kernels drop the (low tap byte) x (low data byte) products, an
    error of the same size as the tap rounding itself, and with q2 = 0 there is nothing to drop; its result is then the
    EXACT product of its (coarse) taps and the residual group carries everything else.  Twice the matrix work, ~20x
    less error, same kernels.

    Rows: row = comp*64 + (q-1) within a q-group of 64 tap rows; columns kap = 2*rho + c over one
    data row of D frames:
        A[(re,q)][2rho] = Re g[qD-1-rho]   A[(re,q)][2rho+1] = -Im g[qD-1-rho]
        A[(im,q)][2rho] = Im g[qD-1-rho]   A[(im,q)][2rho+1] =  Re g[qD-1-rho]
    T = rint(A/u), u = max|A|/32639 per group; T = 256*q1 + q2 with both bytes signed.
    Fragment order (verified on hardware): lane l holds row l&31, k = 16*(l>>5) + j.
    Filters with ceil(L/D) > 64 get several q-groups, decimations whose fragments exceed LDS get
    several k-step ranges; every (group, range) is one pass of the kernel.
    """
    if not mfma_supported(plan):
        raise ValueError("MFMA channelizer needs an int16 or uint8 capture")
    g = plan.taps_natural
    D = plan.decimation
    n_groups = max(1, -(-(-(-plan.ntaps // D)) // MFMA_Q))
    groups, passes = [], []
    err_sq = floor_sq = 0.0
    zero_re = zero_im = 0.0  # the zero-input response: 128 * unit * sum(q2) per output component, over every group
    inband = np.zeros(2, dtype=np.complex128)  # sum_k unit * g2[k] e^{+-j 2 pi nco_step k}: the low tap bytes' gain at the channel centre
    with np.errstate(over="ignore"):
        nco_turns = ((np.uint64(plan.nco_step % TWO64) * np.arange(plan.ntaps, dtype=np.uint64)) >> np.uint64(11)).astype(np.float64) * 2.0**-53
    nco = np.exp(2j * np.pi * nco_turns)
    ksteps = -(-2 * D // 32)
    n_chunks = -(-ksteps // (max_ksteps or MFMA_MAX_KSTEPS_PER_PASS))  # k-step ranges: one pass each
    bounds = [round(i * ksteps / n_chunks) for i in range(n_chunks + 1)]
    s16 = plan.fmt == "s16"
    for gi in range(n_groups):
        _, kc, ok, flat = _mfma_layout(plan.ntaps, D, gi)
        kpad = 32 * ksteps
        gk = g[kc]
        gre = np.where(ok, gk.real, 0.0)
        gim = np.where(ok, gk.imag, 0.0)
        a = np.zeros((2 * MFMA_Q, kpad), dtype=np.float64)
        a[:MFMA_Q, 0 : 2 * D : 2] = gre
        a[:MFMA_Q, 1 : 2 * D : 2] = -gim
        a[MFMA_Q:, 0 : 2 * D : 2] = gim
        a[MFMA_Q:, 1 : 2 * D : 2] = gre
        left = a
        for part in range(2 if residual else 1):
            # (uint8 data are one piece: the kernels' T*v is exact whatever the low tap byte holds)
            unit, t, q1, q2 = _quantise_rows(left, acc32, high_byte_only=residual and part == 0 and s16,
                                             col_ranges=[(32 * bounds[i], 32 * bounds[i + 1]) for i in range(n_chunks)])
            left = left - t * unit
            if s16:
                floor_sq += unit * unit * _LOW_BYTE_VAR * float((q2.astype(np.float64) ** 2).sum())
                zero_re += 128.0 * unit * float(q2[:MFMA_Q].sum(dtype=np.int64))
                zero_im += 128.0 * unit * float(q2[MFMA_Q:].sum(dtype=np.int64))
                g2 = (q2[:MFMA_Q, 0 : 2 * D : 2] - 1j * q2[:MFMA_Q, 1 : 2 * D : 2])[ok] * unit  # (the layout of ``a`` above)
                inband += [np.sum(g2 * nco[kc[ok]]), np.sum(g2 * np.conj(nco[kc[ok]]))]
            frag = np.empty((ksteps, 4, 2, 64, 16), dtype=np.int8)
            frag[:, :, 0] = q1.reshape(-1)[flat]
            frag[:, :, 1] = q2.reshape(-1)[flat]
            groups.append(MfmaGroup(frag, unit, t, q=gi, residual=part == 1, high_only=bool(s16 and not np.any(q2))))
            if acc32 and s16 and not residual:  # (the "fine" groups are not covered)
                rot = zero_high_rotation(q1)
                if rot:
                    frag_rot = np.empty_like(frag)
                    frag_rot[:, :, 0] = rotate_rows(q1, rot).reshape(-1)[flat]
                    frag_rot[:, :, 1] = rotate_rows(q2, rot).reshape(-1)[flat]
                    groups[-1].rot, groups[-1].afrag_rot = rot, frag_rot
            for ci in range(n_chunks):
                k0, k1 = bounds[ci], bounds[ci + 1]
                sl = t[:, 32 * k0 : 32 * k1]
                # int16 data are split v = 256*hi + lo' + 128: the 128 makes a constant 128*sum(T); uint8 data have one piece
                bias = 128.0 if s16 else 0.0
                passes.append(MfmaPass(len(groups) - 1, k0, k1 - k0, bias * float(sl[:MFMA_Q].sum(dtype=np.int64)),
                                       bias * float(sl[MFMA_Q:].sum(dtype=np.int64))))
        err_sq += 0.5 * float((left**2).sum())  # every complex tap sits in the matrix twice (re and im rows)
    # (which of the two turns is the channel's depends on the sample order's conjugation: the other one finds no gain)
    coherent = 4.0 / math.pi * 128.0 * float(np.abs(inband).max())
    return MfmaPlan(ksteps, groups, passes, math.sqrt(err_sq) / INGEST_SCALE[plan.fmt], math.sqrt(floor_sq),
                    math.hypot(zero_re, zero_im), coherent)


def mfma_interior(consumed: int, n_frames: int, m_first: int, n_out: int, decimation: int, ksteps: int,
                  n_groups: int = 1):
    """(m_a, m_b): the sub-range of outputs [m_first, m_first+n_out) whose whole MFMA read range
    (columns m-64*n_groups .. m+29, each 16*ksteps frames from frame b*D+1) lies inside this block's frames."""
    d = decimation
    m_a = max(m_first, MFMA_Q * n_groups + -(-(consumed - 1) // d))  # consumed < 0: a lead-in in front of frame 0
    m_b = min(m_first + n_out, (n_frames + consumed - 16 * ksteps) // d - 30)
    return (m_a, m_b) if m_b > m_a else (m_first, m_first)


def plan_plain_fir(taps: np.ndarray, padded_len: int | None = None) -> ChannelPlan:
    """Real taps, complex64 in/out, no decimation, no rotation (the OverlapSaveFIR stage)."""
    h = np.asarray(taps, dtype=np.float64)
    lpad = padded_len if padded_len is not None else -(-h.size // 256) * 256
    win = np.zeros(lpad, dtype=np.complex64)
    win[: h.size] = h[::-1].astype(np.complex64)
    return ChannelPlan("f32", h.size, 1, win, 0, 0, 0, 0, 1.0 + 0j)


def chunk_output_starts(chunk: int, decimation: int, first_frame: int, n_frames: int) -> np.ndarray:
    """Indices (relative to the first output of the block) of the first decimated sample of
    every reference chunk that starts inside frames [first_frame, first_frame+n_frames).

    ``first_frame`` must be a multiple of ``chunk``.  These are the points where the SSB AGC
    gain restarts (decoders/ssb.py:72) and where per-chunk statistics are cut.
    """
    if first_frame % chunk:
        raise ValueError("blocks must start on a chunk boundary")
    d = decimation
    m_first = -(-first_frame // d)
    starts = np.arange(first_frame, first_frame + n_frames, chunk, dtype=np.int64)
    return (-(-starts // d) - m_first).astype(np.int64)


# ---- wideband FM stereo plan (--demod wfm) --------------------------------

WFM_DEVIATION = 75_000.0  # Hz of deviation that reads as composite 1.0
WFM_PILOT_HZ = 19_000.0
WFM_ATTEN_DB = 70.0
WFM_TRANSITION_HZ = 3_000.0
WFM_AUDIO_CUTOFF = 16_500.0
WFM_PILOT_CUTOFF = 1_500.0
WFM_MIN_RATE = 128_000.0  # below it the 38 kHz stereo subcarrier's upper band (53 kHz) does not fit the channel
WFM_MAX_TAPS = 2047  # IQA_WFM_MAX_TAPS
WFM_STEREO_LEVEL = 0.01  # sqrt(mean |p|^2) at or above which the output is stereo (a 10 % pilot reads 0.05)


@dataclass(frozen=True)
class WfmPlan:
    fs: float
    ntaps: int  # N
    delay: int  # (N - 1) / 2
    h_audio: np.ndarray  # float64[N], the 16.5 kHz low-pass h_a
    h_pilot: np.ndarray  # complex128[N], the analytic pilot filter h_p
    m_scale: float  # composite per radian of the discriminator: fs / (2 pi 75 000)
    taps_packed: np.ndarray  # float32[3 (delay + 1)]: h_a[0..delay], Re h_p[0..delay], Im h_p[0..delay] (iqa_wfm_stereo)


def wfm_num_taps(fs_channel: float) -> int:
    """N = ceil((70 - 7.95) / (2.285 * 2 pi * 3000 / fs)) (Kaiser's length rule), rounded up to odd: 347 at 240 kHz, 693 at 480."""
    n = int(math.ceil((WFM_ATTEN_DB - 7.95) / (2.285 * 2.0 * math.pi * WFM_TRANSITION_HZ / float(fs_channel))))
    return n + 1 if n % 2 == 0 else n


def _kaiser_lowpass(n: int, cutoff: float, fs: float, beta: float) -> np.ndarray:
    """The windowed-sinc construction of ``design_channel_filter``, normalised to sum 1."""
    fc = cutoff / (0.5 * fs)
    m = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    h = fc * np.sinc(fc * m) * np.kaiser(n, beta)
    return h / h.sum()


@functools.lru_cache(maxsize=16)
def plan_wfm(fs_channel: float) -> WfmPlan:
    """The stereo matrix's filters at channel rate ``fs_channel`` (float64; shared, read-only)."""
    fs = float(fs_channel)
    if not fs >= WFM_MIN_RATE:
        raise ValueError(f"wfm needs a channel rate of at least {WFM_MIN_RATE:.0f} Hz (--fs-ch), not {fs:.0f} Hz")
    n = wfm_num_taps(fs)
    if n > WFM_MAX_TAPS:
        raise ValueError(f"wfm channel rate {fs:.0f} Hz needs {n} taps; at most {WFM_MAX_TAPS} are supported (lower --fs-ch)")
    beta = kaiser_beta(WFM_ATTEN_DB)
    delay = (n - 1) // 2
    h_a = _kaiser_lowpass(n, WFM_AUDIO_CUTOFF, fs, beta)
    k = np.arange(n, dtype=np.float64) - delay
    h_p = _kaiser_lowpass(n, WFM_PILOT_CUTOFF, fs, beta) * np.exp(2j * np.pi * WFM_PILOT_HZ * k / fs)
    packed = np.concatenate([h_a[: delay + 1], h_p.real[: delay + 1], h_p.imag[: delay + 1]]).astype(np.float32)
    for arr in (h_a, h_p, packed):
        arr.setflags(write=False)
    return WfmPlan(fs, n, delay, h_a, h_p, float(np.float32(fs / (2.0 * math.pi * WFM_DEVIATION))), packed)


# ---- RDS plan (--demod wfm --rds) ------------------------------------------

RDS_SUBCARRIER_HZ = 57_000.0  # three times the pilot
RDS_BIT_RATE = 1_187.5  # the pilot divided by 16
RDS_SPAN_SYMBOLS = 2  # the matched filter covers +-2 symbols
RDS_MAX_HALF = 2400  # IQA_RDS_MAX_HALF
RDS_MAX_DECIM = 80  # IQA_RDS_MAX_DECIM
RDS_PHASE_BITS = 44  # q = rint(dev / 2 pi * 2^44)


@dataclass(frozen=True)
class RdsPlan:
    fs: float
    wfm: WfmPlan  # N, delay and the analytic pilot filter are the stereo matrix's
    decim: int  # R = round(fs / 19 000)
    half: int  # M: the matched filter has 2M + 1 taps
    h_matched: np.ndarray  # float64[2M + 1], antisymmetric about M, sum of squares 1
    f_mix: float  # 57 000 / fs, cycles per sample
    clock_step: float  # 19 000 R / fs, pilot cycles per decimated sample
    j0: int  # first decimated index past every filter's start-up: ceil((2 (N - 1) + 2M) / R)
    hist_len: int  # discriminator values carried in front of a block: 2M + 2 (N - 1)
    mf_packed: np.ndarray  # float32[M]: h_r[0 .. M-1] (iqa_rds_baseband)
    pilot_packed: np.ndarray  # float32[2 (delay + 1)]: Re h_p[0..delay], Im h_p[0..delay]


def _rds_s(v: np.ndarray) -> np.ndarray:
    """s(v) = sin(4 pi v) / (pi v), s(0) = 4."""
    return 4.0 * np.sinc(4.0 * v)


def rds_pulse(x) -> np.ndarray:
    """h(x) = (s(x + 1/8) + s(x - 1/8)) / 2, x in symbols: the inverse transform of H(f) = cos(pi f td / 4), |f| <= 2 / td."""
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * (_rds_s(x + 0.125) + _rds_s(x - 0.125))


def rds_symbol(x) -> np.ndarray:
    """The centred biphase symbol g(x) = h(x + 1/4) - h(x - 1/4) (antisymmetric), x in symbols."""
    x = np.asarray(x, dtype=np.float64)
    return rds_pulse(x + 0.25) - rds_pulse(x - 0.25)


@functools.lru_cache(maxsize=16)
def plan_rds(fs_channel: float) -> RdsPlan:
    """The RDS demodulator's constants and matched filter at channel rate ``fs_channel`` (float64; shared, read-only)."""
    wfm = plan_wfm(fs_channel)
    fs = wfm.fs
    decim = int(round(fs / WFM_PILOT_HZ))
    spp = fs / RDS_BIT_RATE  # samples per symbol
    half = int(math.ceil(RDS_SPAN_SYMBOLS * spp))
    if decim > RDS_MAX_DECIM or half > RDS_MAX_HALF:
        raise ValueError(f"RDS at a channel rate of {fs:.0f} Hz needs decimation {decim} and {2 * half + 1} taps; at most "
                         f"{RDS_MAX_DECIM} and {2 * RDS_MAX_HALF + 1} are supported (lower --fs-ch)")
    k = np.arange(2 * half + 1, dtype=np.float64)
    h = rds_symbol(-(k - half) / spp)
    h[half] = 0.0
    h = 0.5 * (h - h[::-1])  # (antisymmetric to the last bit)
    h /= math.sqrt(float(np.sum(h * h)))
    d = wfm.delay
    pilot = np.concatenate([wfm.h_pilot.real[: d + 1], wfm.h_pilot.imag[: d + 1]]).astype(np.float32)
    mf = h[:half].astype(np.float32)
    for arr in (h, pilot, mf):
        arr.setflags(write=False)
    j0 = -(-(2 * (wfm.ntaps - 1) + 2 * half) // decim)
    return RdsPlan(fs, wfm, decim, half, h, RDS_SUBCARRIER_HZ / fs, WFM_PILOT_HZ * decim / fs, j0,
                   2 * half + 2 * (wfm.ntaps - 1), mf, pilot)


# ---- POCSAG plan (--demod nfm --pocsag) -------------------------------------

POCSAG_BAUDS = (512, 1200, 2400)
POCSAG_MIN_SPS = 8.0  # below this the bit integrator is too coarse for a half-bit timing search
POCSAG_MAX_SPS = 384  # IQA_POCSAG_MAX_SPS: what the sync kernel's LDS window admits
POCSAG_THETA_BITS = 20  # t = rint(theta 2^20)
POCSAG_BATCH_BITS = 544  # sync word + 16 codewords


@dataclass(frozen=True)
class PocsagBaud:
    baud: int
    sps: float  # fs / baud (float64)
    L: int  # rint(sps): the bit integrator's window
    h: int  # floor(sps / 2): the local-maximum radius and the batch continuation tolerance
    offsets: np.ndarray  # int32[545]: rint(i sps), i = 0 .. 544, half-even in float64 (bit i of a batch; [544] = the next sync)


@dataclass(frozen=True)
class PocsagPlan:
    fs: float
    bauds: tuple  # the PocsagBaud entries that run, in POCSAG_BAUDS order
    skipped: tuple  # the baud rates that do not fit this channel rate
    hist_len: int  # quantised discriminator values carried in front of a block: max L - 1

    def lengths(self) -> tuple:
        """(L at 512, L at 1200, L at 2400), 0 for a skipped baud: what ``iqa_pocsag_integrate`` takes."""
        by = {b.baud: b.L for b in self.bauds}
        return tuple(by.get(b, 0) for b in POCSAG_BAUDS)


@functools.lru_cache(maxsize=16)
def plan_pocsag(fs_channel: float) -> PocsagPlan:
    """The POCSAG decoder's per-baud constants at channel rate ``fs_channel``; ``ValueError`` when no baud rate fits."""
    fs = float(fs_channel)
    if not math.isfinite(fs) or fs <= 0.0:
        raise ValueError("the channel rate must be positive")
    bauds, skipped = [], []
    for baud in POCSAG_BAUDS:
        sps = fs / baud
        if sps < POCSAG_MIN_SPS or sps > POCSAG_MAX_SPS:
            skipped.append(baud)
            continue
        offsets = np.rint(np.arange(POCSAG_BATCH_BITS + 1, dtype=np.float64) * sps).astype(np.int32)
        offsets.setflags(write=False)
        bauds.append(PocsagBaud(baud, sps, int(np.rint(sps)), int(math.floor(sps / 2.0)), offsets))
    if not bauds:
        raise ValueError(f"POCSAG needs {POCSAG_MIN_SPS:.0f} to {POCSAG_MAX_SPS} samples per bit at 512, 1200 or 2400 baud; "
                         f"a channel rate of {fs:.0f} Hz gives none of them (--fs-ch between about 20 000 and 190 000)")
    return PocsagPlan(fs, tuple(bauds), tuple(skipped), max(b.L for b in bauds) - 1)


# ---- AFSK / AX.25 plan (--demod nfm --ax25) ---------------------------------

AFSK_BAUD = 1200
AFSK_TONES = (1200, 2200)  # mark, space (Bell 202)
AFSK_MIN_SPS = 8.0  # below this eight sampling phases per bit are not distinct
AFSK_MAX_SPS = 400  # IQA_AFSK_MAX_SPS
AFSK_THETA_BITS = 12  # t = rint(theta 2^12)
AFSK_TAP_SCALE = 256.0
AFSK_PHASES = 8  # IQA_AFSK_PHASES
AFSK_GAINS = ((1, 1), (1, 4), (4, 1))  # (a, b) of d = a E_1200 - b E_2200: flat, de-emphasised and pre-emphasised space tone


@dataclass(frozen=True)
class AfskPlan:
    fs: float
    sps: float  # fs / 1200 (float64)
    L: int  # rint(sps): the tone correlators' window
    step: float  # sps / 8: the spacing of the sampling phases
    taps: np.ndarray  # int16[4, L]: c_1200, s_1200, c_2200, s_2200

    def instant(self, i, p: int):
        """The instant of bit ``i`` (an int or an integer array) at phase ``p``: L - 1 + rint((8 i + p) step)."""
        return self.L - 1 + np.rint((8.0 * np.asarray(i, dtype=np.float64) + p) * self.step).astype(np.int64)

    def bit_count(self, p: int, n: int) -> int:
        """How many bits of phase ``p`` have their instant inside a stream of ``n`` samples."""
        i = max(int((n - self.L) / self.sps) - 2, 0)
        while int(self.instant(i, p)) < n:
            i += 1
        return i


@functools.lru_cache(maxsize=16)
def plan_afsk(fs_channel: float) -> AfskPlan:
    """The Bell-202 decoder's constants at channel rate ``fs_channel``; ``ValueError`` when 1200 baud does not fit it."""
    fs = float(fs_channel)
    if not math.isfinite(fs) or fs <= 0.0:
        raise ValueError("the channel rate must be positive")
    sps = fs / AFSK_BAUD
    if sps < AFSK_MIN_SPS or sps > AFSK_MAX_SPS:
        raise ValueError(f"AFSK at 1200 baud needs {AFSK_MIN_SPS:.0f} to {AFSK_MAX_SPS} samples per bit; a channel rate of {fs:.0f} Hz "
                         f"gives {sps:.1f} (--fs-ch between 9 600 and 480 000)")
    L = int(np.rint(sps))
    k = np.arange(L, dtype=np.float64)
    rows = []
    for f in AFSK_TONES:
        rows.append(np.rint(AFSK_TAP_SCALE * np.cos(2.0 * np.pi * f * k / fs)))
        rows.append(np.rint(AFSK_TAP_SCALE * np.sin(2.0 * np.pi * f * k / fs)))
    taps = np.ascontiguousarray(np.stack(rows).astype(np.int16))
    taps.setflags(write=False)
    return AfskPlan(fs, sps, L, sps / 8.0, taps)


# ---- CTCSS / DTMF plan (--demod nfm --tones) --------------------------------

TONES_RATE = 8000.0  # the tone banks run at fd = fs / floor(fs / 8000), in [8000, 16000)
TONES_MAX_R = 64  # IQA_TONES_MAX_R
TONES_THETA_BITS = 12  # t = rint(theta 2^12)
TONES_TAP_SCALE = 256.0
TONES_NONE = 255  # IQA_TONES_NONE
CTCSS_TONES = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0,
               127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5, 186.2,
               189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1)
DTMF_TONES = (697.0, 770.0, 852.0, 941.0, 1209.0, 1336.0, 1477.0, 1633.0)  # rows, then columns
DTMF_KEYS = "123A456B789C*0#D"  # the key of (row r, column c) is DTMF_KEYS[4 r + c]
CTCSS_HOP_S, DTMF_HOP_S = 0.2, 0.01  # a frame is two hops


def _tone_taps(tones, n: int, fd: float) -> np.ndarray:
    k = np.arange(n, dtype=np.float64)
    rows = [[np.rint(TONES_TAP_SCALE * np.cos(2.0 * np.pi * f * k / fd)), np.rint(TONES_TAP_SCALE * np.sin(2.0 * np.pi * f * k / fd))]
            for f in tones]
    taps = np.ascontiguousarray(np.array(rows).astype(np.int16))
    taps.setflags(write=False)
    return taps


@dataclass(frozen=True)
class TonesPlan:
    fs: float
    R: int  # floor(fs / 8000): the decimation in front of the banks
    fd: float  # fs / R (float64)
    Hd: int  # DTMF hop, rint(0.01 fd)
    Nd: int  # DTMF frame, 2 Hd
    Hc: int  # CTCSS hop, rint(0.2 fd)
    Nc: int  # CTCSS frame, 2 Hc
    ctcss_taps: np.ndarray  # int16[50, 2, Nc]: c_f, s_f
    dtmf_taps: np.ndarray  # int16[8, 2, Nd]

    def frames(self, n_frame: int, hop: int, m: int) -> int:
        """How many frames of a bank fit ``m`` decimated samples."""
        return 0 if m < n_frame else (m - n_frame) // hop + 1


@functools.lru_cache(maxsize=16)
def plan_tones(fs_channel: float) -> TonesPlan:
    """The tone detectors' constants at channel rate ``fs_channel``; ``ValueError`` outside 8000 <= fs < 520 000."""
    fs = float(fs_channel)
    if not math.isfinite(fs) or fs <= 0.0:
        raise ValueError("the channel rate must be positive")
    R = int(math.floor(fs / TONES_RATE))
    if R < 1 or R > TONES_MAX_R:
        raise ValueError(f"tone detection decimates by floor(fs / 8000), which must be 1 to {TONES_MAX_R}; a channel rate of {fs:.0f} Hz "
                         f"gives {R} (--fs-ch from 8 000 to below 520 000)")
    fd = fs / R
    Hd, Hc = int(np.rint(DTMF_HOP_S * fd)), int(np.rint(CTCSS_HOP_S * fd))
    return TonesPlan(fs, R, fd, Hd, 2 * Hd, Hc, 2 * Hc, _tone_taps(CTCSS_TONES, 2 * Hc, fd), _tone_taps(DTMF_TONES, 2 * Hd, fd))


# ---- ACARS plan (--demod am --acars) ----------------------------------------

ACARS_BAUD = 2400
ACARS_CENTRE = 1800.0  # MSK: 1200 Hz (the bit changes) and 2400 Hz (the bit stays) around it
ACARS_MIN_SPS = 8.0  # below this eight sampling phases per bit are not distinct
ACARS_MAX_SPS = 400  # IQA_ACARS_MAX_SPS
ACARS_TAP_SCALE = 256.0
ACARS_PHASES = 8  # IQA_ACARS_PHASES
ACARS_Q_BITS = 15  # 0 <= q <= 2^15


@dataclass(frozen=True)
class AcarsPlan:
    fs: float
    sps: float  # fs / 2400 (float64)
    L: int  # rint(sps): the differential detector's delay
    W: int  # rint(fs / 1800): the correlator's window, one cycle of the centre frequency
    step: float  # sps / 8: the spacing of the sampling phases
    taps: np.ndarray  # int16[2, W]: c, s
    cr: int  # rint(256 cos psi), psi = 2 pi 1800 L / fs
    sr: int  # rint(256 sin psi)

    def instant(self, i, p: int):
        """The instant of symbol ``i`` (an int or an integer array) at phase ``p``: W - 1 + rint((8 i + p) step)."""
        return self.W - 1 + np.rint((8.0 * np.asarray(i, dtype=np.float64) + p) * self.step).astype(np.int64)

    def bit_count(self, p: int, n: int) -> int:
        """How many symbols of phase ``p`` have their instant inside a stream of ``n`` samples."""
        i = max(int((n - self.W) / self.sps) - 2, 0)
        while int(self.instant(i, p)) < n:
            i += 1
        return i


@functools.lru_cache(maxsize=16)
def plan_acars(fs_channel: float) -> AcarsPlan:
    """The ACARS decoder's constants at channel rate ``fs_channel``; ``ValueError`` when 2400 bit/s does not fit it."""
    fs = float(fs_channel)
    if not math.isfinite(fs) or fs <= 0.0:
        raise ValueError("the channel rate must be positive")
    sps = fs / ACARS_BAUD
    if sps < ACARS_MIN_SPS or sps > ACARS_MAX_SPS:
        raise ValueError(f"ACARS at 2400 bit/s needs {ACARS_MIN_SPS:.0f} to {ACARS_MAX_SPS} samples per bit; a channel rate of {fs:.0f} Hz "
                         f"gives {sps:.1f} (--fs-ch between 19 200 and 960 000)")
    L, W = int(np.rint(sps)), int(np.rint(fs / ACARS_CENTRE))
    k = np.arange(W, dtype=np.float64)
    rows = np.stack([np.rint(ACARS_TAP_SCALE * np.cos(2.0 * np.pi * ACARS_CENTRE * k / fs)),
                     np.rint(ACARS_TAP_SCALE * np.sin(2.0 * np.pi * ACARS_CENTRE * k / fs))])
    # q >= 0: a correlator sum is at most 2^15 times the positive (or the negative) taps of its table: inside int32
    assert 2 ** ACARS_Q_BITS * max(np.maximum(rows, 0).sum(axis=1).max(), -np.minimum(rows, 0).sum(axis=1).min()) < 2 ** 31
    taps = np.ascontiguousarray(rows.astype(np.int16))
    taps.setflags(write=False)
    psi = 2.0 * np.pi * ACARS_CENTRE * L / fs
    return AcarsPlan(fs, sps, L, W, sps / 8.0, taps, int(np.rint(ACARS_TAP_SCALE * np.cos(psi))), int(np.rint(ACARS_TAP_SCALE * np.sin(psi))))


# ---- AIS plan (--demod nfm --ais) -------------------------------------------

AIS_BAUD = 9600
AIS_BT = 0.4  # the transmitter's Gaussian filter
AIS_MIN_SPS = 5.0  # below this the pulse filter has too few taps to tell eight sampling phases apart
AIS_MAX_SPS = 100  # IQA_AIS_MAX_SPS
AIS_THETA_BITS = 12  # t = rint(theta 2^12)
AIS_T_MAX = 12_868  # rint(float32(pi) 4096)
AIS_TAP_SCALE = 256.0
AIS_PHASES = 8  # IQA_AIS_PHASES


@dataclass(frozen=True)
class AisPlan:
    fs: float
    sps: float  # fs / 9600 (float64)
    L: int  # rint(sps)
    W: int  # 3 L - 1: the pulse filter's taps
    step: float  # sps / 8: the spacing of the sampling phases
    taps: np.ndarray  # int16[W]

    def instant(self, i, p: int):
        """The instant of symbol ``i`` (an int or an integer array) at phase ``p``: W - 1 + rint((8 i + p) step)."""
        return self.W - 1 + np.rint((8.0 * np.asarray(i, dtype=np.float64) + p) * self.step).astype(np.int64)

    def symbol_count(self, p: int, n: int) -> int:
        """How many symbols of phase ``p`` have their instant inside a stream of ``n`` samples."""
        i = max(int((n - self.W) / self.sps) - 2, 0)
        while int(self.instant(i, p)) < n:
            i += 1
        return i


@functools.lru_cache(maxsize=16)
def plan_ais(fs_channel: float) -> AisPlan:
    """The AIS decoder's constants at channel rate ``fs_channel``; ``ValueError`` when 9600 bit/s does not fit it."""
    fs = float(fs_channel)
    if not math.isfinite(fs) or fs <= 0.0:
        raise ValueError("the channel rate must be positive")
    sps = fs / AIS_BAUD
    if sps < AIS_MIN_SPS or sps > AIS_MAX_SPS:
        raise ValueError(f"AIS at 9600 bit/s needs {AIS_MIN_SPS:.0f} to {AIS_MAX_SPS} samples per bit; a channel rate of {fs:.0f} Hz "
                         f"gives {sps:.1f} (--fs-ch between 48 000 and 960 000)")
    L = int(np.rint(sps))
    W = 3 * L - 1
    sigma = math.sqrt(math.log(2.0)) / (2.0 * math.pi * AIS_BT) * sps
    k = np.arange(2 * L, dtype=np.float64)
    gauss = np.exp(-((k - (2 * L - 1) / 2.0) ** 2) / (2.0 * sigma * sigma))
    pulse = np.convolve(gauss, np.ones(L, dtype=np.float64))  # the Gaussian over one bit of the NRZ waveform
    h = np.rint(AIS_TAP_SCALE * pulse / pulse.max())
    assert h.size == W and AIS_T_MAX * int(np.abs(h).sum()) < 2 ** 31
    taps = np.ascontiguousarray(h.astype(np.int16))
    taps.setflags(write=False)
    return AisPlan(fs, sps, L, W, sps / 8.0, taps)


# ---- ADS-B / Mode S plan (--demod am --adsb) --------------------------------

ADSB_CHIP_RATE = 2e6  # half-microsecond chips: a bit is two of them (pulse position modulation)
ADSB_MIN_SPS = 2.0  # samples per microsecond: one sample per chip at least
ADSB_MAX_SPS = 20  # IQA_ADSB_MAX_SPS
ADSB_CHIPS = 240  # 16 of the 8 us preamble, 224 of 112 bits (IQA_ADSB_CHIPS)
ADSB_Q_MAX = 65535  # q is uint16


@dataclass(frozen=True)
class AdsbPlan:
    fs: float
    sps: float  # fs / 1e6 (float64): samples per microsecond
    h: int  # floor(sps / 2): the samples summed per chip
    offsets: np.ndarray  # int32[240]: o[k] = rint(k sps / 2)
    span: int  # o[239] + h: the samples a candidate position reads
    L: int  # rint(sps): the reach within which identical frames are one message


@functools.lru_cache(maxsize=16)
def plan_adsb(fs_channel: float) -> AdsbPlan:
    """The Mode S decoder's constants at channel rate ``fs_channel``; ``ValueError`` when half-microsecond chips do not fit it."""
    fs = float(fs_channel)
    if not math.isfinite(fs) or fs <= 0.0:
        raise ValueError("the channel rate must be positive")
    sps = fs / 1e6
    if sps < ADSB_MIN_SPS or sps > ADSB_MAX_SPS:
        raise ValueError(f"Mode S on 1090 MHz needs {ADSB_MIN_SPS:.0f} to {ADSB_MAX_SPS} samples per microsecond; a channel rate of "
                         f"{fs:.0f} Hz gives {sps:.2f} (--fs-ch between 2 000 000 and 20 000 000)")
    h = int(math.floor(sps / 2.0))
    offsets = np.rint(np.arange(ADSB_CHIPS, dtype=np.float64) * (sps / 2.0)).astype(np.int32)
    # P is a sum of 4 chips and is compared with 6 chips: both stay inside int32
    assert h >= 1 and 6 * h * ADSB_Q_MAX < 2 ** 31
    offsets.setflags(write=False)
    return AdsbPlan(fs, sps, h, offsets, int(offsets[-1]) + h, int(np.rint(sps)))


# ---- channel finder plan (--find-channels) --------------------------------

FIND_MIN_NFFT, FIND_MAX_NFFT = 256, 1 << 18
FIND_MIN_FRAMES = 8  # the default nfft is halved while fewer frames fit
FIND_MAX_HALF = 8191  # IQA_FIND_MAX_HALF
FIND_MAX_GAP = 255  # IQA_FIND_MAX_GAP
FIND_MAX_SLICE_FRAMES = 65536  # IQA_FIND_MAX_SLICE_FRAMES
FIND_C_MIN, FIND_C_MAX = -30000, 30000  # centi-dB range of the quantiser (IQA_FIND_C_MIN)
FIND_RANK = (1, 4)  # the local floor is the lower quartile of its window


@dataclass(frozen=True)
class FindPlan:
    fs: float
    n_samples: int
    nfft: int
    hop: int  # nfft // 2
    frames: int  # F = (n - nfft) // hop + 1
    scale: float  # of the rows, as spectrum._PsdEngine makes it
    bin_hz: float
    dc_bin: int
    max_slices: int
    slice_frames: int  # T = ceil(F / max_slices)
    slices: int  # S = ceil(F / T)
    half: int  # h: bins on either side in the floor's window
    num: int
    den: int
    thr: int  # centi-dB, mean over its floor
    thr_peak: int  # centi-dB, max over its floor
    thr_act: int  # centi-dB, a slice's mean over the floor of the mean
    gap: int  # cold bins between two hot ones that are closed
    dc_guard: int  # bins on either side of dc_bin that are never hot (negative: none)
    min_hot: int
    threshold_db: float
    peak_threshold_db: float

    def slice_len(self, s: int) -> int:
        """T_s: the frames of slice ``s`` (the last one may be shorter)."""
        return min(self.slice_frames, self.frames - s * self.slice_frames)


def find_default_nfft(sample_rate: float, n_samples: int) -> int:
    """The power of two with fs / nfft in (250, 500] Hz, clipped to [256, 2^18] and halved while fewer than 8 frames fit."""
    nfft = 1 << max(0, math.ceil(math.log2(sample_rate / 500.0)))
    while nfft < sample_rate / 500.0:  # (log2 of an exact power of two may land a hair low)
        nfft *= 2
    nfft = min(max(nfft, FIND_MIN_NFFT), FIND_MAX_NFFT)
    while nfft > FIND_MIN_NFFT and (n_samples - nfft) // (nfft // 2) + 1 < FIND_MIN_FRAMES:
        nfft //= 2
    return nfft


def plan_find(sample_rate: float, n_samples: int, *, nfft: int | None = None, threshold_db: float = 6.0,
              peak_threshold_db: float = 10.0, floor_hz: float = 1e6, gap_hz: float = 5000.0, dc_guard_hz: float = 1000.0,
              max_slices: int = 256, min_hot: int = 2) -> FindPlan:
    """The channel finder's constants for a capture of ``n_samples`` frames at ``sample_rate``; ``ValueError`` where the capture
    holds no frame, a slice would be longer than 65536 frames or an option is out of range."""
    fs, n = float(sample_rate), int(n_samples)
    if not math.isfinite(fs) or fs <= 0.0:
        raise ValueError("the sample rate must be positive")
    for name, value in (("threshold_db", threshold_db), ("peak_threshold_db", peak_threshold_db), ("floor_hz", floor_hz)):
        if not math.isfinite(value) or value <= 0.0:
            raise ValueError(f"{name} must be positive")
    if not math.isfinite(gap_hz) or gap_hz < 0.0 or not math.isfinite(dc_guard_hz):
        raise ValueError("gap_hz must not be negative and dc_guard_hz must be finite")
    if max_slices < 1 or min_hot < 1:
        raise ValueError("max_slices and min_hot must be at least 1")
    if nfft is None:
        if n < FIND_MIN_NFFT:
            raise ValueError(f"the capture holds {n} samples: not one frame of {FIND_MIN_NFFT}")
        nfft = find_default_nfft(fs, n)
    nfft = int(nfft)
    if nfft < 16 or nfft > FIND_MAX_NFFT or nfft & (nfft - 1):
        raise ValueError(f"nfft must be a power of two between 16 and {FIND_MAX_NFFT}")
    if n < nfft:
        raise ValueError(f"the capture holds {n} samples: not one frame of {nfft}")
    hop = nfft // 2
    frames = (n - nfft) // hop + 1
    slice_frames = -(-frames // int(max_slices))
    if slice_frames > FIND_MAX_SLICE_FRAMES:
        raise ValueError(f"{frames} frames in {max_slices} slices are {slice_frames} per slice: more than {FIND_MAX_SLICE_FRAMES}")
    window = np.hanning(nfft).astype(np.float64)
    scale = (nfft * fs * float(np.sum(window ** 2) / nfft)) + 1e-18
    bin_hz = fs / nfft
    thr = int(np.rint(100.0 * threshold_db))
    if thr >= 1 << 20 or int(np.rint(100.0 * peak_threshold_db)) >= 1 << 20:
        raise ValueError("a threshold must stay below 10 485 dB")
    return FindPlan(fs=fs, n_samples=n, nfft=nfft, hop=hop, frames=frames, scale=scale, bin_hz=bin_hz, dc_bin=nfft // 2,
                    max_slices=int(max_slices), slice_frames=slice_frames, slices=-(-frames // slice_frames),
                    half=min(int(floor_hz / 2.0 / bin_hz), FIND_MAX_HALF), num=FIND_RANK[0], den=FIND_RANK[1], thr=thr,
                    thr_peak=int(np.rint(100.0 * peak_threshold_db)), thr_act=thr // 2, gap=min(int(gap_hz / bin_hz), FIND_MAX_GAP),
                    dc_guard=int(dc_guard_hz / bin_hz) if dc_guard_hz >= 0.0 else -1, min_hot=int(min_hot),
                    threshold_db=float(threshold_db), peak_threshold_db=float(peak_threshold_db))


# ---- channel description plan (--find-describe) ----------------------------

DESCRIBE_MIN_BW = 6000.0  # Hz: the narrowest channel filter
DESCRIBE_MIN_RATE = 12000.0  # Hz: the lowest channel rate asked for
DESCRIBE_MAX_SHIFT = 30  # IQA_DESCRIBE_MAX_SHIFT
DESCRIBE_TILE = 2048  # samples to a row of iqa_describe_accumulate


@dataclass(frozen=True)
class DescribePlan:
    fs: float
    offset_hz: float
    width_hz: float
    bw: float  # the channel filter's bandwidth
    decimation: int
    fs_ch: float
    taps: np.ndarray  # float64, read-only
    delay: int  # (L - 1) // 2 raw frames


def plan_describe(sample_rate: float, offset_hz: float, width_hz: float) -> DescribePlan:
    """The channelizer of one found channel: twice its occupied width (6 kHz at least, a quarter of the capture's rate at
    most), at twice that rate (12 kHz at least)."""
    fs, offset, width = float(sample_rate), float(offset_hz), float(width_hz)
    if not math.isfinite(fs) or fs <= 0.0:
        raise ValueError("the sample rate must be positive")
    if not math.isfinite(width) or width <= 0.0:
        raise ValueError("the channel's width must be positive")
    if not math.isfinite(offset) or abs(offset) > fs / 2.0:
        raise ValueError("the channel's offset must lie inside the capture")
    bw = min(max(2.0 * width, DESCRIBE_MIN_BW), fs / 4.0)
    decimation, fs_ch = choose_decimation(fs, max(2.0 * bw, DESCRIBE_MIN_RATE))
    taps = design_channel_filter(fs, bw, decimation)
    taps.setflags(write=False)
    return DescribePlan(fs=fs, offset_hz=offset, width_hz=width, bw=bw, decimation=decimation, fs_ch=fs_ch, taps=taps,
                        delay=(len(taps) - 1) // 2)


# ---- keying plan (--find-decode) -------------------------------------------

KEYING_BAUDS = (512, 1200, 1600, 2400, 3200, 4800, 9600)
KEYING_WINDOW = 2048  # samples to a row of iqa_keying_accumulate, counted on the absolute position
KEYING_SUMS = 16  # int32 values of a row: P, K, then (C_k, Q_k) per candidate
KEYING_TABLE = 1024  # entries of the cos / sin table
KEYING_SCALE = 4096.0  # the quantiser's: t = rint(theta 4096)
KEYING_T_MAX = 32767


@dataclass(frozen=True)
class KeyingPlan:
    fs_ch: float
    bauds: tuple  # KEYING_BAUDS
    incs: tuple  # rint(B 2^32 / fs_ch) per candidate; 0 for a skipped one
    skipped: tuple  # bool per candidate: B >= fs_ch / 4
    table: np.ndarray  # int16[1024][2]: rint(1024 cos), rint(1024 sin); read-only


def keying_table() -> np.ndarray:
    """int16[1024][2]: (rint(1024 cos(2 pi i / 1024)), rint(1024 sin(2 pi i / 1024))), float64 on the host."""
    turn = 2.0 * np.pi * np.arange(KEYING_TABLE, dtype=np.float64) / KEYING_TABLE
    table = np.stack((np.rint(1024.0 * np.cos(turn)), np.rint(1024.0 * np.sin(turn))), axis=1).astype(np.int16)
    table.setflags(write=False)
    return table


def plan_keying(fs_ch: float) -> KeyingPlan:
    """The clock steps of the candidate bauds at the channel rate ``fs_ch``: inc = rint(B 2^32 / fs_ch) in float64, and 0 for a
    candidate of a quarter of the rate or more (skipped: fewer than four samples to a symbol)."""
    fs_ch = float(fs_ch)
    if not math.isfinite(fs_ch) or fs_ch <= 0.0:
        raise ValueError("the channel rate must be positive")
    skipped = tuple(b >= fs_ch / 4.0 for b in KEYING_BAUDS)
    incs = tuple(0 if skip else int(np.rint(b * 4294967296.0 / fs_ch)) for b, skip in zip(KEYING_BAUDS, skipped))
    return KeyingPlan(fs_ch=fs_ch, bauds=KEYING_BAUDS, incs=incs, skipped=skipped, table=keying_table())


# ---- protocol identification plan (--find-identify) -------------------------

IDENT_MIN_SPS, IDENT_MAX_SPS = 4.0, 224.0  # samples to a symbol
IDENT_LEAD = 16  # o[i] sits at index 16 + i of ``offsets``: i = -16 .. 47
IDENT_OFFSETS = 64
IDENT_MAX_SYMBOLS = 32
IDENT_MAX_N = 1 << 30  # samples of one stored stream
IDENT_RECORD = 6  # int64 values of a kept hit: pattern, m, C, E, pre, post


@dataclass(frozen=True)
class IdentPlan:
    fs_ch: float
    rate: int  # R: the family's symbol rate
    sps: float  # fs_ch / R
    window: int  # L = rint(sps)
    half: int  # h = floor(sps / 2)
    shift: int  # sh = max(0, bit_length(L - 1) - 6)
    offsets: tuple  # o[i] = rint(i sps), i = -16 .. 47 (half-even, float64)

    def o(self, i: int) -> int:
        return self.offsets[IDENT_LEAD + i]


def plan_ident(fs_ch: float, rate: int) -> IdentPlan:
    """The integrator's window and the sample offsets of the symbols of a family of ``rate`` symbols/s at the channel rate
    ``fs_ch``.  ``ValueError`` unless 4 <= sps <= 224."""
    fs_ch, rate = float(fs_ch), int(rate)
    if not math.isfinite(fs_ch) or fs_ch <= 0.0 or rate <= 0:
        raise ValueError("the channel rate and the symbol rate must be positive")
    sps = fs_ch / rate
    if not IDENT_MIN_SPS <= sps <= IDENT_MAX_SPS:
        raise ValueError(f"{sps:.2f} samples to a symbol at {fs_ch:.0f} Hz and {rate} symbols/s: must be 4 .. 224")
    window = int(np.rint(sps))
    offsets = tuple(int(np.rint(i * sps)) for i in range(-IDENT_LEAD, IDENT_OFFSETS - IDENT_LEAD))
    return IdentPlan(fs_ch=fs_ch, rate=rate, sps=sps, window=window, half=int(math.floor(sps / 2.0)),
                     shift=max(0, (window - 1).bit_length() - 6), offsets=offsets)


# ---- FLEX page decoding plan (--find-flex) ---------------------------------

FLEX_MIN_SPS, FLEX_MAX_SPS = 8.0, 224.0  # samples to a 1600 bit/s bit: 3200 symbols/s keeps 4 samples to a symbol
FLEX_LEAD = 16  # o16[i] sits at index 16 + i of ``header``: i = -16 .. 95
FLEX_HEADER_OFFSETS = 112
FLEX_DATA_BIT = 135  # the data begin where bit 135 of the 1600 bit/s grid ends
FLEX_SYMBOLS = 2816  # data symbols of a frame at 1600 symbols/s: 11 blocks of 256
FLEX_BLOCKS, FLEX_SHIFTS, FLEX_PHASES, FLEX_WORDS = 11, 5, 4, 88


@dataclass(frozen=True)
class FlexPlan:
    fs_ch: float
    sps: float  # fs_ch / 1600
    header: tuple  # o16[i] = rint(i sps), i = -16 .. 95 (half-even, float64)
    data: tuple  # per u = 1, 2: int32[2816 u], data symbol q ends at m + rint((135 + (q + 1) / u) sps)
    steps: tuple  # per u = 1, 2: max(1, floor(sps / (8 u)))
    ident: tuple  # the IdentPlans at 1600 and 3200 symbols/s

    def o16(self, i: int) -> int:
        return self.header[FLEX_LEAD + i]


def plan_flex(fs_ch: float) -> FlexPlan:
    """The sample offsets of a FLEX frame behind its first sync word at the channel rate ``fs_ch``: the 1600 bit/s grid of the
    header, the data symbols at 1600 and 3200 symbols/s, the timing steps and the integrator plans of both rates.
    ``ValueError`` unless 8 <= sps <= 224."""
    fs_ch = float(fs_ch)
    if not math.isfinite(fs_ch) or fs_ch <= 0.0:
        raise ValueError("the channel rate must be positive")
    sps = fs_ch / 1600.0
    if not FLEX_MIN_SPS <= sps <= FLEX_MAX_SPS:
        raise ValueError(f"{sps:.2f} samples to a bit at {fs_ch:.0f} Hz and 1600 bit/s: must be 8 .. 224")
    header = tuple(int(np.rint(i * sps)) for i in range(-FLEX_LEAD, FLEX_HEADER_OFFSETS - FLEX_LEAD))
    data, steps = [], []
    for u in (1, 2):
        q = np.arange(FLEX_SYMBOLS * u, dtype=np.float64)
        off = np.rint((FLEX_DATA_BIT + (q + 1.0) / u) * sps).astype(np.int32)
        off.setflags(write=False)
        data.append(off)
        steps.append(max(1, int(math.floor(sps / (8.0 * u)))))
    return FlexPlan(fs_ch=fs_ch, sps=sps, header=header, data=tuple(data), steps=tuple(steps),
                    ident=(plan_ident(fs_ch, 1600), plan_ident(fs_ch, 3200)))


# ---- DMR burst decoding plan (--find-dmr) ----------------------------------

DMR_LEAD = 66  # o[i] sits at index 66 + i of ``offsets``: i = -66 .. 77
DMR_OFFSETS = 144
DMR_WORDS = 9  # uint32 words of a sliced burst: 24 CACH bits, then 264 burst bits
DMR_RECORD = 8  # int32 values of a decoded burst


@dataclass(frozen=True)
class DmrPlan:
    fs_ch: float
    sps: float  # fs_ch / 4800
    offsets: tuple  # o[i] = rint(i sps), i = -66 .. 77 (half-even, float64)
    ident: IdentPlan  # section 25's plan at 4800 symbols/s

    def o(self, i: int) -> int:
        return self.offsets[DMR_LEAD + i]


def plan_dmr(fs_ch: float) -> DmrPlan:
    """The sample offsets of a DMR burst and its CACH around sync symbol 0 at the channel rate ``fs_ch``, and section 25's plan at
    4800 symbols/s.  ``ValueError`` unless 4 <= sps <= 224 (``plan_ident``'s limits)."""
    ident = plan_ident(fs_ch, 4800)
    offsets = tuple(int(np.rint(i * ident.sps)) for i in range(-DMR_LEAD, DMR_OFFSETS - DMR_LEAD))
    return DmrPlan(fs_ch=ident.fs_ch, sps=ident.sps, offsets=offsets, ident=ident)


# ---- P25 frame decoding plan (--find-p25) ----------------------------------

P25_OFFSETS = 864  # o[i], i = 0 .. 863: the symbols of one LDU, the longest frame read
P25_WORDS = 54  # uint32 words of a sliced frame: symbol i the frame bits 2 i, 2 i + 1
P25_INFO = 9  # uint32 words of a decoded frame's information
P25_RECORD = 8  # int32 values of a decoded frame


@dataclass(frozen=True)
class P25Plan:
    fs_ch: float
    sps: float  # fs_ch / 4800
    offsets: tuple  # o[i] = rint(i sps), i = 0 .. 863 (half-even, float64)
    ident: IdentPlan  # section 25's plan at 4800 symbols/s

    def o(self, i: int) -> int:
        return self.offsets[i]


def plan_p25(fs_ch: float) -> P25Plan:
    """The sample offsets of the symbols of a P25 frame behind the end of sync symbol 0 at the channel rate ``fs_ch``, and section
    25's plan at 4800 symbols/s.  ``ValueError`` unless 4 <= sps <= 224 (``plan_ident``'s limits)."""
    ident = plan_ident(fs_ch, 4800)
    offsets = tuple(int(np.rint(i * ident.sps)) for i in range(P25_OFFSETS))
    return P25Plan(fs_ch=ident.fs_ch, sps=ident.sps, offsets=offsets, ident=ident)


# ---- YSF frame decoding plan (--find-ysf) ----------------------------------

YSF_OFFSETS = 480  # o[i], i = 0 .. 479: the symbols of one frame
YSF_WORDS = 30  # uint32 words of a sliced frame: symbol i the frame bits 2 i, 2 i + 1
YSF_FICH_RECORD = 5  # int32 values of a decoded FICH
YSF_INFO = 12  # uint32 words of a frame's decoded data channels: six to a block
YSF_RECORD = 4  # int32 values of a frame's decoded data channels


@dataclass(frozen=True)
class YsfPlan:
    fs_ch: float
    sps: float  # fs_ch / 4800
    offsets: tuple  # o[i] = rint(i sps), i = 0 .. 479 (half-even, float64)
    ident: IdentPlan  # section 25's plan at 4800 symbols/s

    def o(self, i: int) -> int:
        return self.offsets[i]


def plan_ysf(fs_ch: float) -> YsfPlan:
    """The sample offsets of the symbols of a YSF frame behind the end of sync symbol 0 at the channel rate ``fs_ch``, and section
    25's plan at 4800 symbols/s.  ``ValueError`` unless 4 <= sps <= 224 (``plan_ident``'s limits)."""
    ident = plan_ident(fs_ch, 4800)
    offsets = tuple(int(np.rint(i * ident.sps)) for i in range(YSF_OFFSETS))
    return YsfPlan(fs_ch=ident.fs_ch, sps=ident.sps, offsets=offsets, ident=ident)


# ---- NXDN frame decoding plan (--find-nxdn) --------------------------------

NXDN_OFFSETS = 192  # o[i], i = 0 .. 191: the symbols of one frame
NXDN_WORDS = 12  # uint32 words of a sliced frame: symbol i the frame bits 2 i, 2 i + 1
NXDN_INFO = 14  # uint32 words of a frame's decoded blocks: SACCH 0 .. 1, FACCH1-a 2 .. 4, FACCH1-b 5 .. 7, CAC 8 .. 13
NXDN_RECORD = 4  # int32 values of a frame's decoded blocks
NXDN_RATES = (4800, 2400)  # symbols/s


@dataclass(frozen=True)
class NxdnPlan:
    fs_ch: float
    rate: int  # 4800 or 2400 symbols/s
    sps: float  # fs_ch / rate
    offsets: tuple  # o[i] = rint(i sps), i = 0 .. 191 (half-even, float64)
    ident: IdentPlan  # section 25's plan at ``rate``

    def o(self, i: int) -> int:
        return self.offsets[i]


def plan_nxdn(fs_ch: float, rate: int = 4800) -> NxdnPlan:
    """The sample offsets of the symbols of an NXDN frame behind the end of sync symbol 0 at the channel rate ``fs_ch`` and
    ``rate`` symbols/s (4800 or 2400), and section 25's plan at that rate.  ``ValueError`` for another rate and unless
    4 <= sps <= 224 (``plan_ident``'s limits)."""
    if rate not in NXDN_RATES:
        raise ValueError(f"NXDN is sent at 4800 or 2400 symbols/s, not {rate}")
    ident = plan_ident(fs_ch, int(rate))
    offsets = tuple(int(np.rint(i * ident.sps)) for i in range(NXDN_OFFSETS))
    return NxdnPlan(fs_ch=ident.fs_ch, rate=int(rate), sps=ident.sps, offsets=offsets, ident=ident)


# ---- carrier squelch plan (--squelch) --------------------------------------

GATE_CELL = 256  # IQA_GATE_CELL: samples to a cell, counted on the absolute position
GATE_MAX_FRAME = 1 << 20  # IQA_GATE_MAX_FRAME
GATE_MAX_FRAMES = 1 << 24  # IQA_GATE_MAX_FRAMES
GATE_MAX_SHIFT = 30  # IQA_GATE_MAX_SHIFT
GATE_MAX_OPEN_DB = 30.0
GATE_MAX_MS = 10_000.0
GATE_RANK = (1, 10)  # the floor is the run's tenth percentile: rank (F - 1) // 10
GATE_DEFAULTS = dict(frame_ms=10.0, open_db=6.0, hyst_db=2.0, hang_ms=300.0, min_ms=40.0, lead_ms=20.0, ramp_ms=5.0)


@dataclass(frozen=True)
class GatePlan:
    fs: float
    frame: int  # Lf: samples to a frame, a multiple of GATE_CELL
    hang: int  # H frames
    min_frames: int  # M
    lead: int  # A frames
    ramp_len: int  # R samples
    num_open: int  # rint(1024 10^(open_db / 10))
    num_close: int  # rint(1024 10^((open_db - hyst_db) / 10))
    ramp: np.ndarray  # float32[R]: (k + 1) / (R + 1); read-only

    def frames(self, n: int) -> int:
        """F = max(1, n // Lf) of a stream of ``n`` samples."""
        return max(1, int(n) // self.frame)


def plan_gate(fs: float, opts=None) -> GatePlan:
    """The carrier squelch at the channel rate ``fs`` (float64 on the host).  ``opts``: anything with the attributes of
    ``GATE_DEFAULTS`` (``gate.CarrierSquelch``); None takes the defaults."""
    fs = float(fs)
    if not math.isfinite(fs) or fs <= 0.0:
        raise ValueError("the channel rate must be positive")
    o = {k: float(getattr(opts, k, v)) if opts is not None else v for k, v in GATE_DEFAULTS.items()}
    for k, v in o.items():
        if not math.isfinite(v):
            raise ValueError(f"{k} must be finite")
    for k in ("frame_ms", "hang_ms", "min_ms", "lead_ms", "ramp_ms"):
        if not 0.0 <= o[k] <= GATE_MAX_MS:
            raise ValueError(f"{k} must lie in 0 .. {GATE_MAX_MS:.0f} ms")
    if not (0.0 <= o["hyst_db"] < o["open_db"] <= GATE_MAX_OPEN_DB):
        raise ValueError(f"open_db and hyst_db must satisfy 0 <= hyst_db < open_db <= {GATE_MAX_OPEN_DB:.0f}")
    frame = GATE_CELL * max(1, int(fs * o["frame_ms"] / 1000.0 / GATE_CELL))
    if frame > GATE_MAX_FRAME:
        raise ValueError(f"a frame of {frame} samples exceeds {GATE_MAX_FRAME}")

    def fr(ms: float) -> int:
        return int(math.ceil(ms / 1000.0 * fs / frame))

    ramp_len = int(np.rint(o["ramp_ms"] / 1000.0 * fs))
    ramp = ((np.arange(ramp_len, dtype=np.float64) + 1.0) / (ramp_len + 1.0)).astype(np.float32)
    ramp.setflags(write=False)
    return GatePlan(fs=fs, frame=frame, hang=fr(o["hang_ms"]), min_frames=max(1, fr(o["min_ms"])), lead=fr(o["lead_ms"]),
                    ramp_len=ramp_len, num_open=int(np.rint(1024.0 * 10.0 ** (o["open_db"] / 10.0))),
                    num_close=int(np.rint(1024.0 * 10.0 ** ((o["open_db"] - o["hyst_db"]) / 10.0))), ramp=ramp)


# ---- 48 kHz resampler plan (build-defined spec; see DESIGN.md "48 kHz stage") -----------------

RS_ZERO_CROSSINGS = 16
RS_CUTOFF = 0.97
RS_KAISER_BETA = 9.0
RS_OUT_RATE = 48_000


@dataclass
class ResamplerPlan:
    in_rate: int
    up: int
    down: int
    half_taps: int  # T: table rows hold taps t = -T..T
    table: np.ndarray  # float64 [up, 2T+1]

    def n_out(self, n_in: int) -> int:
        return -(-n_in * self.up // self.down)


def plan_resampler(fs_channel: float, out_rate: int = RS_OUT_RATE) -> ResamplerPlan:
    """Polyphase table of the zero-phase Kaiser-sinc prototype (planned once per declared input rate: the table of
    the 96 154 -> 48 000 Hz case has 1.6 M entries and its Bessel window costs ~55 ms of host NumPy -- most of a file ->
    WAV run on the reference's own 5 s benchmark capture before it was cached).  The plan and its table are shared: do
    not modify them.

    The declared input rate is round(fs_channel), exactly what the reference tells ffmpeg
    (processing.py:389-397).  Prototype (common rate up*in_rate): h[i] = sinc(0.97*i/M) *
    kaiser(beta=9) over |i| <= 16*M, M = max(up, down), scaled to sum(h) = up.
    Row p of the table holds h[p + t*up] for t = -T..T (zero outside the support).
    """
    return _plan_resampler(max(1, int(round(fs_channel))), int(out_rate))


@functools.lru_cache(maxsize=16)
def _plan_resampler(rin: int, out_rate: int) -> ResamplerPlan:
    g = math.gcd(out_rate, rin)
    up, down = out_rate // g, rin // g
    m = max(up, down)
    half = RS_ZERO_CROSSINGS * m
    i = np.arange(-half, half + 1, dtype=np.float64)
    u = i / half
    win = np.i0(RS_KAISER_BETA * np.sqrt(np.clip(1.0 - u * u, 0.0, 1.0))) / np.i0(RS_KAISER_BETA)
    h = np.sinc(RS_CUTOFF * i / m) * win
    h *= up / h.sum()
    t_half = -(-half // up)
    idx = np.arange(up, dtype=np.int64)[:, None] + np.arange(-t_half, t_half + 1, dtype=np.int64)[None, :] * up
    ok = np.abs(idx) <= half
    table = np.ascontiguousarray(np.where(ok, h[np.clip(idx + half, 0, 2 * half)], 0.0), dtype=np.float64)
    table.setflags(write=False)
    return ResamplerPlan(rin, up, down, int(t_half), table)
