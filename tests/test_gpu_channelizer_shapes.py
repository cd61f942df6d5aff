"""The float32 channelizer (csrc/channelize.hip: k_channelize_v1 in its throughput and split-K forms, k_history_update)
against the float64 model of tests/channelizer_model.py, at the shapes where the kernel's own structure changes: tap
counts around the padding (256) and slice (2048) limits, block counts with and without a tail of the XCD tile
permutation, the form switch at 16384 outputs, windows that straddle hist | raw, blocks shorter than the history,
slices skipped at the start of a stream, D > L, conj_sum, the three scales and the 64-bit phase wrap.
tests/test_channelizer_model_host.py asserts that every case here reaches the path it is named for.

Every call goes through the C ABI.  The output carries 16 float2 of a fill pattern behind n_out, which must survive.  Raw
and history frames are views, at odd frame offsets (so every 16-byte load is unaligned), into allocations whose
surroundings hold NaN (f32), +-32767 (s16) or 255 (u8): a read outside [0, n_frames) or outside the L - 1 history frames
that meets a non-zero tap poisons or changes an exact sum.  Nothing reads outside an allocation.

Exact cases (integer taps and frames, 2 L max|g| max|x| < 2^24, dense taps, rotate = 0, scale 1 / j / -j): every float32
partial sum is an exact integer whatever the order, so the output must equal the model bit for bit (the sign of a zero
aside).  Rotation cases: the tap sum is exact, what remains is the epilogue, c_epi u B.  Designed filters: every output
of both forms within M.error_bound of M.direct, per component.

The bound (derivation: the docstring of tests/channelizer_model.py): u = 2^-24,
B = sum_i (|g_re| + |g_im|)(|x_re| + |x_im|); a product passes through at most depth = 8 ceil(Lpad / 256) + 6 roundings
in the throughput form (the fmas behind it on its lane's accumulator, 6 adds of the wave butterfly) and
8 ceil(Lpad / 2048) + 6 + 8 in split-K (+ the fixed-order sum over the 8 waves); the rotation mixes the two components'
errors, depth u B_re and depth u B_im, into at most depth u (B_re + B_im) = depth u B; c_epi = 6 = 3 (float32 cos / sin,
product, add of the rotation) + 2 (product, add of the scale) + 1 (second order, float64 sincospi, the model's own
error), with or without fma contraction.  |err| <= (depth + c_epi) u B per component: derived, not tuned.
"""
from __future__ import annotations

from ctypes import byref, c_int32, c_int64

import numpy as np
import pytest
import channelizer_model as M

from iq_to_audio_amd import _dev as D
from iq_to_audio_amd import _native as N
from iq_to_audio_amd import dsp_plan as P

pytestmark = pytest.mark.gpu

GUARD = 16  # float2 behind n_out
FILL = 0x7FC5A5A5  # a NaN pattern no sum produces
MARGIN = 512  # hostile frames on either side of a view
RAW_LEAD, HIST_LEAD = 3, 5  # odd frame offsets: 12 / 6 / 24 and 20 / 10 / 40 bytes past a 16-byte boundary
NEXT_FILL = 0xA5
RATIOS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    N.lib()
    N.require_gpu()
    yield
    for name, ratio in RATIOS.items():
        print(f"\nchannelizer [{name}]: largest |err| / bound = {ratio:.4f}")


def hostile_view(data, fmt: str, lead: int):
    """(allocation, view): `data` (interleaved values) on the device, `MARGIN + lead` frames into an allocation whose
    other frames hold the format's hostile values.  Keep the allocation alive while the view is in use."""
    data = np.zeros(0, dtype=M.FMT_DTYPE[fmt]) if data is None else np.ascontiguousarray(data).reshape(-1)
    assert data.dtype == M.FMT_DTYPE[fmt] and data.size % 2 == 0
    host = np.empty(2 * (2 * MARGIN + lead) + data.size, dtype=data.dtype)
    host[0::2], host[1::2] = M.HOSTILE[fmt]
    lo = 2 * (MARGIN + lead)
    host[lo:lo + data.size] = data
    dev = D.from_numpy(host)
    # (an empty slice has a NULL data_ptr: a view of no frames -- the history of one tap -- keeps one hostile frame, so that
    # the call still gets a pointer; none of it may be read)
    view = dev[lo:lo + max(data.size, 2)]
    assert (view.data_ptr() - dev.data_ptr()) % 16 != 0 and dev.data_ptr() % 16 == 0
    return dev, view


def chan_params(fmt, ntaps, decimation, conj_sum=0, rotate=0, rot_step=0, rot_base=0, scale=1.0 + 0j):
    return N.ChanParams(fmt=M.FMT_CODE.get(fmt, fmt), ntaps=ntaps, decimation=decimation, conj_sum=conj_sum, rotate=rotate, reserved=0,
                        rot_step=rot_step, rot_base=rot_base, out_scale_re=float(complex(scale).real),
                        out_scale_im=float(complex(scale).imag))


class Device:
    """The buffers of one call: taps, the hostile allocations around raw and hist."""

    def __init__(self, taps, raw, hist, fmt):
        self.fmt = fmt
        self.taps = D.from_numpy(np.asarray(taps, dtype=np.complex64))
        assert self.taps.data_ptr() % 16 == 0
        self.raw_all, self.raw = hostile_view(raw, fmt, RAW_LEAD)
        self.hist_all, self.hist = (None, None) if hist is None else hostile_view(hist, fmt, HIST_LEAD)

    def call(self, params, n_frames, consumed, m_first, n_out, *, taps=True, raw=True, out=True):
        """iqa_channelize into a guarded output.  Returns (complex64[n_out], whole buffer as uint32) -- the latter for the
        refusals, which must leave all of it alone."""
        torch = D.torch_mod()
        z = torch.full((2 * (max(n_out, 0) + GUARD),), FILL, dtype=torch.int32, device=D.device())
        try:
            N.call("iqa_channelize", byref(params), N.ptr(self.taps if taps else None), N.ptr(self.raw if raw else None),
                   c_int64(n_frames), c_int64(consumed), N.ptr(self.hist), c_int64(m_first), c_int64(n_out),
                   N.ptr(z if out else None), N.stream_ptr())
        finally:
            self.words = z.cpu().numpy().view(np.uint32)
        assert np.all(self.words[2 * max(n_out, 0):] == FILL), "a store landed behind n_out"
        return self.words[:2 * max(n_out, 0)].view(np.complex64).copy()


def run_case(case: M.Case, fmt: str, taps, raw, hist, **kw):
    dev = Device(taps, raw[:2 * case.n_frames], hist, fmt)
    return dev.call(chan_params(fmt, case.ntaps, case.decimation, **kw), case.n_frames, case.consumed, case.m_first, case.n_out)


def model(case: M.Case, fmt: str, taps, raw, hist, **kw):
    return M.direct(taps, raw, fmt, hist, case.consumed, case.m_first, case.n_out, ntaps=case.ntaps, decimation=case.decimation,
                    n_frames=case.n_frames, **kw)


def assert_bits(z, want, name):
    assert not (np.asarray(z).view(np.uint32) == FILL).any(), f"{name}: an output was not written"
    if not M.same_bits(z, want):
        w = np.asarray(want).astype(np.complex64)
        bad = np.flatnonzero(z != w)
        raise AssertionError(f"{name}: {bad.size} of {z.size} outputs differ from the exact model; first at {bad[0]}: "
                             f"got {z[bad[0]]!r}, want {w[bad[0]]!r}")


def exact(case: M.Case, fmt: str, **kw):
    taps, raw, hist = M.exact_data(case, fmt)
    z = run_case(case, fmt, taps, raw, hist, **kw)
    assert_bits(z, model(case, fmt, taps, raw, hist, **kw), f"{case.name} {fmt}")
    return z


# ---------------------------------------------------------------------------------------------------------------
# exact, bit for bit


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("L", M.TAP_LIMIT_L)
def test_tap_counts_around_the_padding_and_slice_limits(L, fmt):
    """D = 1, split-K with 1, 2, 8, 9, 10 and 33 blocks (the permutation without and with a tail), from the start of a
    stream (zeros in front; 4097 taps: the first slice of block 0 is skipped) and with a history."""
    for case in M.tap_limit_cases(L):
        exact(case, fmt)


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("D_", M.THROUGHPUT_D)
@pytest.mark.parametrize("L", M.THROUGHPUT_L)
def test_throughput_form_and_the_form_switch(L, D_, fmt):
    """16383 outputs (split-K, 4096 blocks), 16384 (throughput form, 512 blocks) and 16485 (516 blocks: a tail of the
    permutation and a ragged last block) of one stream at one placement: the head blocks straddle the history, the middle
    is interior, the last output's newest frame is n_frames - 1 so that the pad taps' frames lie behind the block.  All
    three equal the model, hence each other on the outputs they share."""
    cases = M.throughput_cases(L, D_)
    taps, raw, hist = M.exact_data(cases[-1], fmt)
    want = model(cases[-1], fmt, taps, raw, hist)
    got = {}
    for case in cases:
        got[case.n_out] = z = run_case(case, fmt, taps, raw, hist)
        assert_bits(z, want[:case.n_out], f"{case.name} {fmt}")
    assert np.array_equal(got[16383].view(np.uint32), got[16384][:16383].view(np.uint32))
    assert np.array_equal(got[16384].view(np.uint32), got[16485][:16384].view(np.uint32))


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("case", M.PLACEMENT_CASES, ids=lambda c: c.name)
def test_decimation_and_placement(case, fmt):
    """D = 2, 7, 104, 521 with D > L (frames never read), consumed no multiple of D, m_first > 0, slack behind the last
    window, blocks shorter than the history (every window mostly hist) and a block of one frame."""
    exact(case, fmt)


@pytest.mark.parametrize("case,fmt", [(c, f) for c in M.LONG_CASES for f in c.fmts], ids=lambda v: getattr(v, "name", v))
def test_long_filters(case, fmt):
    """6401 taps (4 slices) and 32769 taps (17 slices) at their decimations, at the start of a stream (2 of 4 and 15 of 17 slices of
    block 0 skipped) and mid-stream with a history."""
    exact(case, fmt)


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_conj_sum_and_scale(fmt):
    """conj_sum x scale in exact complex arithmetic at a three-slice shape."""
    case = M.CONJ_SCALE_CASE
    taps, raw, hist = M.exact_data(case, fmt)
    dev = Device(taps, raw, hist, fmt)
    plain = model(case, fmt, taps, raw, hist)
    seen = set()
    for conj in (0, 1):
        for scale in M.SCALES:
            z = dev.call(chan_params(fmt, case.ntaps, case.decimation, conj_sum=conj, scale=scale), case.n_frames, case.consumed,
                         case.m_first, case.n_out)
            want = model(case, fmt, taps, raw, hist, conj_sum=conj, scale=scale)
            assert np.array_equal(want, scale * (np.conj(plain) if conj else plain))
            assert_bits(z, want, f"{case.name} {fmt} conj {conj} scale {scale}")
            seen.add(z.tobytes())
    assert len(seen) == 6  # six different answers


# ---------------------------------------------------------------------------------------------------------------
# refusals


def test_argument_refusals_launch_nothing():
    """Every refused call returns the invalid-argument code (ValueError through the binding) and leaves the whole output
    buffer alone; n_out = 0 is fine with NULL pointers."""
    case = M.mid_stream("refuse", 5, 2, 20, consumed=11)
    taps, raw, hist = M.exact_data(case, "s16")
    dev = Device(taps, raw, hist, "s16")
    ok = dict(n_frames=case.n_frames, consumed=case.consumed, m_first=case.m_first, n_out=case.n_out)
    good = chan_params("s16", 5, 2)
    assert_bits(dev.call(good, **ok), model(case, "s16", taps, raw, hist), "the accepted call")
    refused = [
        ("beyond the frames", good, {**ok, "n_out": case.n_out + 1}, {}),
        ("beyond the frames", good, {**ok, "n_frames": case.n_frames - 1}, {}),
        ("before this block", good, {**ok, "consumed": 1000, "m_first": 0, "n_out": 3}, {}),
        ("older than the history", good, {**ok, "m_first": case.m_first - 1}, {}),
        ("ntaps", chan_params("s16", 0, 2), ok, {}),
        ("ntaps", chan_params("s16", -3, 2), ok, {}),
        ("decimation", chan_params("s16", 5, 0), ok, {}),
        ("format", chan_params(7, 5, 2), ok, {}),
        ("NULL", good, ok, {"taps": False}),
        ("NULL", good, ok, {"raw": False}),
        ("NULL", good, ok, {"out": False}),
        ("negative", good, {**ok, "consumed": -1}, {}),
    ]
    for what, params, args, nulls in refused:
        with pytest.raises(ValueError, match=what):
            dev.call(params, **args, **nulls)
        assert np.all(dev.words == FILL), what
    # nothing to do
    assert dev.call(good, 0, 0, 0, 0, taps=False, raw=False, out=False).size == 0


# ---------------------------------------------------------------------------------------------------------------
# rotation


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("m_first", M.ROTATION_M_FIRST)
def test_rotation_with_a_wrapping_64_bit_phase(m_first, fmt):
    """Exact tap sums, rotate = 1, random 64-bit rot_step and rot_base: m rot_step wraps 2^64 up to 2^40 times.  What
    remains is the epilogue: every output within c_epi u B of the model's float64 rotation (L = 1: B <= 2 |S|, so a phase
    wrong by 12 u = 7e-7 turns is caught)."""
    rng = np.random.default_rng([17, m_first % 1000])
    worst = 0.0
    for L in (1, 5):
        case = M.rotation_case(L, m_first)
        taps, raw, hist = M.exact_data(case, fmt)
        step, base = (int(v) for v in rng.integers(0, 2 ** 64, size=2, dtype=np.uint64))
        kw = dict(rotate=1, rot_step=step, rot_base=base)
        z = run_case(case, fmt, taps, raw, hist, **kw)
        want = model(case, fmt, taps, raw, hist, **kw)
        b = M.abs_sum(taps, raw, fmt, hist, case.consumed, case.m_first, case.n_out, ntaps=L, decimation=case.decimation)
        ratio = M.within(z, want, M.epilogue_bound(b))
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), (case.name, fmt, float(ratio.max()))
        plain = model(case, fmt, taps, raw, hist)
        assert np.abs(want).max() > 1.0 and np.ptp(np.angle(want[plain != 0] / plain[plain != 0])) > 1.0  # it does rotate
    RATIOS[f"rotation m_first {m_first} {fmt} (of c_epi u B)"] = worst


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_quarter_turns_are_exact(fmt):
    """rot_step = 0 and rot_base = 0, 2^62, 2^63, 3 2^62: the float32 cos and sin are exactly (1, 0), (0, 1), (-1, 0),
    (0, -1), each component of y = S (c + j s) is one exact product plus a zero, and BOTH components of every output must
    equal the model's 1, j, -1, -j times the exact sum bit for bit (the sign of a zero aside)."""
    case = M.rotation_case(5, 1)
    taps, raw, hist = M.exact_data(case, fmt)
    plain = model(case, fmt, taps, raw, hist)
    for k, turn in enumerate((1, 1j, -1, -1j)):
        kw = dict(rotate=1, rot_step=0, rot_base=k << 62)
        want = model(case, fmt, taps, raw, hist, **kw)
        assert np.array_equal(want, turn * plain)
        assert_bits(run_case(case, fmt, taps, raw, hist, **kw), want, f"{case.name} {fmt} rot_base {k} / 4")


# ---------------------------------------------------------------------------------------------------------------
# designed filters

DESIGNED = [  # (fs, bandwidth, D, f_off, mix_sign, fmt, iq_order): the filter shapes of tests/test_gpu_parity.py
    (1e6, 12500.0, 10, 31250.0, 1, "s16", "qi"),
    (1e6, 12500.0, 10, 31250.0, 1, "u8", "iq_inv"),
    (1e6, 12500.0, 10, 31250.0, 1, "f32", "qi_inv"),
    (10e6, 12500.0, 104, 1.2e6, 1, "s16", "iq"),
    (20e6, 2800.0, 208, -3.3e6, 1, "f32", "iq"),
    (50e6, 12500.0, 521, 7.7e6, 1, "u8", "iq"),
]
DESIGNED_N_OUT = 16384 + 37  # the throughput form; its first DESIGNED_SPLITK outputs again in split-K
DESIGNED_SPLITK = 1003


def noise_and_tone(fmt: str, n: int, cycles_per_frame: float, seed: int = 2):
    rng = np.random.default_rng(seed)
    tone = np.exp(2j * np.pi * cycles_per_frame * np.arange(n))
    iq = np.empty(2 * n)
    if fmt == "s16":
        iq[0::2], iq[1::2] = 8000 * tone.real, 8000 * tone.imag
        return (rng.integers(-12000, 12000, size=2 * n) + np.rint(iq)).astype(np.int16)
    if fmt == "u8":
        iq[0::2], iq[1::2] = 40 * tone.real, 40 * tone.imag
        return (rng.integers(48, 208, size=2 * n) + np.rint(iq)).astype(np.uint8)
    iq[0::2], iq[1::2] = 0.25 * tone.real, 0.25 * tone.imag
    return (rng.normal(scale=0.3, size=2 * n) + iq).astype(np.float32)


@pytest.mark.parametrize("fs,bw,d,f_off,sign,fmt,order", DESIGNED, ids=lambda v: str(v))
def test_designed_filters_within_the_derived_bound(fs, bw, d, f_off, sign, fmt, order):
    """The 1025-, 6401-, 32769- and 32001-tap channel filters, pre-rotated as Channelizer does it (dsp_plan.plan_channel:
    NCO, iq_order and ingest scale folded in, rotate = 1), on noise plus an in-band tone, mid-stream with a history: every
    output of the throughput form and of split-K within error_bound of direct, per component."""
    taps = P.design_channel_filter(fs, bw, d)
    plan = P.plan_channel(taps, sample_rate=fs, freq_offset=f_off, mix_sign=sign, decimation=d, fmt=fmt, iq_order=order)
    L = plan.ntaps
    case = M.mid_stream(f"designed-L{L}-D{d}", L, d, DESIGNED_N_OUT, consumed=1001)
    stream = noise_and_tone(fmt, L - 1 + case.n_frames, (f_off + 900.0) / fs * (1 if order in ("iq", "qi_inv") else -1))
    hist, raw = stream[:2 * (L - 1)], stream[2 * (L - 1):]
    method = "fft" if L * case.n_out > (1 << 26) else "gather"
    kw = dict(conj_sum=plan.conj_sum, rotate=plan.rotate, rot_step=plan.rot_step, rot_base=plan.rot_base, scale=plan.out_scale)
    want = model(case, fmt, plan.taps_window, raw, hist, method=method, **kw)
    b = M.abs_sum(plan.taps_window, raw, fmt, hist, case.consumed, case.m_first, case.n_out, ntaps=L, decimation=d,
                  n_frames=case.n_frames, method=method)
    assert np.sqrt(np.mean(np.abs(want[L // d + 1:]) ** 2)) > 0.05  # the tone is in the pass band
    dev = Device(plan.taps_window, raw, hist, fmt)
    params = chan_params(fmt, L, d, **kw)
    for form, n_out in (("throughput", case.n_out), ("splitk", DESIGNED_SPLITK)):
        assert M.form_of(n_out) == form
        z = dev.call(params, case.n_frames, case.consumed, case.m_first, n_out)
        bound = (M.depth(L, form) + M.C_EPI) * M.U * b[:n_out]
        ratio = M.within(z, want[:n_out], bound)
        RATIOS[f"designed L {L} D {d} {fmt} {order} {form}"] = float(ratio.max())
        print(f"designed L {L} D {d} {fmt} {order} {form}: largest |err| / bound = {float(ratio.max()):.4f}")
        assert np.all(ratio <= 1.0), (form, int(np.argmax(ratio)), float(ratio.max()))


# ---------------------------------------------------------------------------------------------------------------
# the history


def history_update(fmt, ntaps, hist_view, raw_view, n_frames, keep, *, alias=False):
    torch = D.torch_mod()
    fb = M.FRAME_BYTES[fmt]
    nxt = torch.full((keep * fb + 64,), NEXT_FILL, dtype=torch.uint8, device=D.device())
    target = hist_view if alias else nxt
    try:
        N.call("iqa_history_update", c_int32(M.FMT_CODE[fmt]), c_int32(ntaps), N.ptr(hist_view), N.ptr(raw_view), c_int64(n_frames),
               N.ptr(target), N.stream_ptr())
    finally:
        got = nxt.cpu().numpy()
    assert np.all(got[keep * fb:] == NEXT_FILL), "a store landed behind the next history"
    return got[:keep * fb]


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("keep", [1, 255, 256, 257, 6400])
def test_history_update_byte_for_byte(keep, fmt):
    """next = (hist | raw)[n_frames : n_frames + L - 1] in raw bytes, with a history and with NULL (zeros; 128 / 128 for
    u8), for blocks of 0, 1, keep - 1, keep, keep + 1 and 3 keep frames; one or two grid blocks (keep <= 256 | 257) and 26."""
    rng = np.random.default_rng([3, keep])
    dt = M.FMT_DTYPE[fmt]

    def block(n):
        if fmt == "f32":
            return rng.normal(size=2 * n).astype(dt)
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, size=2 * n, endpoint=True).astype(dt)

    hist = block(keep)
    hist_all, hist_view = hostile_view(hist, fmt, HIST_LEAD)
    for n_frames in sorted({0, 1, keep - 1, keep, keep + 1, 3 * keep}):
        raw = block(n_frames)
        raw_all, raw_view = hostile_view(raw, fmt, RAW_LEAD)
        for h_np, h_dev in ((hist, hist_view), (None, None)):
            got = history_update(fmt, keep + 1, h_dev, raw_view if n_frames else None, n_frames, keep)
            want = M.history_next(h_np, raw, fmt, keep, n_frames)
            assert np.array_equal(got, want), (fmt, keep, n_frames, h_np is None)
            if h_np is None and n_frames < keep:
                assert got[0] == (128 if fmt == "u8" else 0)


@pytest.mark.parametrize("fmt", M.FORMATS)
def test_history_update_edges(fmt):
    hist = np.arange(2 * 4, dtype=M.FMT_DTYPE[fmt])
    hist_all, hist_view = hostile_view(hist, fmt, HIST_LEAD)
    raw_all, raw_view = hostile_view(hist[:4], fmt, RAW_LEAD)
    # ntaps = 1: nothing to keep, nothing written, NULL is fine
    assert history_update(fmt, 1, None, None, 5, 0).size == 0
    with pytest.raises(ValueError, match="alias"):
        history_update(fmt, 5, hist_view, raw_view, 2, 4, alias=True)
    with pytest.raises(ValueError, match="format"):
        N.call("iqa_history_update", c_int32(7), c_int32(5), N.ptr(hist_view), N.ptr(raw_view), c_int64(2), N.ptr(hist_view), N.stream_ptr())
    assert np.array_equal(hist_view.cpu().numpy(), hist)  # the refused calls wrote nothing
