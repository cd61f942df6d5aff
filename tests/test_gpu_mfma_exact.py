"""The int8 matrix-core channelizer kernels held to an exact integer model (oracle/mfma_model.py).

Every output of ``k_channelize_mfma_s16`` and of the ring kernels of channelize_ring.hip is an exact integer sum followed
by a fixed, explicitly rounded float64 emission (csrc/mfma_common.h), so with ``rotate = 0`` it must equal the model bit
for bit (``torch.equal``).  With ``rotate = 1`` the kernels evaluate the rotation with ``sincospi`` or the ring's float64
recurrence: each component must lie within one float32 ulp of |z| of the model and fewer than 1 in 1000 outputs may
differ at all.  Taps are random and full scale (every tap row weighs the same), so a kernel that drops a k step, a tap
row, a frame or a product cannot hide in the weak outer rows of a Kaiser design.  Every launch asserts the documented
read bounds on the host, before the call.  Which kernel a launch reaches: oracle/mfma_dispatch.py restates the dispatch
of ring_launch_multi / ring_launch_pairs, and each case checks the part of it the ABI can report (iqa_mfma_ring_mode /
_lanes / _pairs: slot form and pair availability).  The SKIPK / HALF / 64-bit choice inside a form is not observable
through the ABI; the host suite checks that the sweep names every instantiation once or more, and a kernel trace of the
sweep launched exactly those 129 kernels, each as often as the sweep names it.
"""
from __future__ import annotations

import functools
import hashlib
from ctypes import byref, c_double, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from oracle import cpu_ref as O
from oracle import mfma_dispatch as X
from oracle import mfma_model as M

pytestmark = pytest.mark.gpu

RG_PACE_WORDS = 16384  # channelize_ring.hip: pacing words of the lane-pair launches


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _P():
    from iq_to_audio_amd import dsp_plan as P

    return P


def _N():
    from iq_to_audio_amd import _native as N

    return N


def _check_abi_selects(A, entry, fmt, d, k_first, k_count, acc64, name):
    X.abi_agrees(A.native.lib(), entry, fmt, d, k_first, k_count, acc64, name)


# ---- plans, captures, bounds -------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=64)
def random_plan(L: int, d: int, fmt: str, acc32: bool, residual: bool, max_ks, seed: int):
    """An MFMA plan of random full-scale complex taps (every tap row carries the same weight)."""
    P = _P()
    rng = np.random.default_rng(seed)
    g = (rng.uniform(-1.0, 1.0, L) + 1j * rng.uniform(-1.0, 1.0, L)) * P.INGEST_SCALE[fmt]
    plan = P.ChannelPlan(fmt=fmt, ntaps=L, decimation=d, taps_window=None, conj_sum=0, rotate=0, rot_step=0, rot_base=0,
                         out_scale=1.0 + 0j, taps_natural=g)
    return P.plan_mfma(plan, acc32=acc32, max_ksteps=max_ks, residual=residual)


def capture(fmt: str, n_frames: int, seed: int, data=None) -> np.ndarray:
    """Uniform full-range interleaved values, the extremes included.  ``data(fmt, n_frames)``: the 2 n_frames values to
    use instead (tests/test_gpu_mfma_data_classes.py), which must be legal for the format."""
    if data is not None:
        lo, hi, dt = (-32768, 32767, np.int16) if fmt == "s16" else (0, 255, np.uint8)
        v = np.asarray(data(fmt, n_frames))
        assert v.shape == (2 * n_frames,) and v.dtype.kind in "iu" and v.min() >= lo and v.max() <= hi
        return v.astype(dt)
    rng = np.random.default_rng(seed)
    if fmt == "s16":
        v = rng.integers(-32768, 32768, 2 * n_frames, dtype=np.int64)
        v[rng.integers(0, v.size, 64)] = -32768
        v[rng.integers(0, v.size, 64)] = 32767
        return v.astype(np.int16)
    return rng.integers(0, 256, 2 * n_frames, dtype=np.int64).astype(np.uint8)


def ring_frames_needed(mode: int, d: int, k_first: int, k_count: int, q_min: int, m_first: int, n_out: int, opb: int,
                       consumed: int) -> int:
    """Frames [0, n) a multi-lane ring launch may read (channelize_mfma.hip, channelize_mfma_lanes)."""
    blocks = -(-n_out // opb)
    last_cnt = n_out - (blocks - 1) * opb
    last_tiles, full_tiles = (last_cnt + 94) // 32, (opb + 94) // 32
    tail = 512 * k_count if mode == 1 else 16 * (k_first + k_count)
    b_last = m_first - 64 - 64 * q_min
    t_last = b_last + (blocks - 1) * opb + (last_tiles - 1) * 32
    t_full = b_last + (blocks - 2) * opb + (full_tiles - 1) * 32 if blocks > 1 else t_last
    span = 0 if mode == 1 else 31
    return max(t_last + span, t_full + span) * d + 1 - consumed + tail


def assert_read_bounds(mode: int, d: int, k_first: int, k_count: int, q_min: int, q_max: int, m_first: int, n_out: int,
                       opb: int, consumed: int, n_frames: int) -> None:
    """The documented read bounds of a ring launch, asserted before the call: the first row of the largest tap-row
    group starts inside the block; contiguous slots (mode 1) fetch 512 ceil(2D/32) frames from a tile's first frame,
    (m_last - 1) D + 512 ceil(2D/32) < consumed + n_frames; row-staged slots read exactly their rows' k-step ranges."""
    assert (m_first - 64 - 64 * q_max) * d + 1 - consumed >= 0
    assert ring_frames_needed(mode, d, k_first, k_count, q_min, m_first, n_out, opb, consumed) <= n_frames
    if mode == 1:
        ks_all = -(-2 * d // 32)
        assert (m_first + n_out - 2) * d + 512 * ks_all < consumed + n_frames


def perlane_frames_needed(d, k_first, k_count, q, m_first, n_out, opb, consumed) -> int:
    """Frames [0, n) the per-lane kernel reads (iqa_channelize_mfma, reserved = 0)."""
    blocks = -(-n_out // opb)
    last_cnt = n_out - (blocks - 1) * opb
    b_max = m_first + (blocks - 1) * opb - 64 - 64 * q + (last_cnt + 94) // 32 * 32 - 1
    b_max_full = m_first + (blocks - 2) * opb - 64 - 64 * q + (opb + 94) // 32 * 32 - 1 if blocks > 1 else b_max
    return max(b_max, b_max_full) * d + 1 - consumed + 16 * (k_first + k_count)


# ---- comparisons --------------------------------------------------------------------------------------------------


def assert_exact(got, want: np.ndarray, what=""):
    import torch

    w = torch.from_numpy(np.ascontiguousarray(want)).to(got.device)
    if not torch.equal(got, w):
        g = got.cpu().numpy()
        bad = np.flatnonzero((g != want).reshape(len(want), -1).any(axis=1))
        raise AssertionError(f"{what}: {bad.size} of {len(want)} outputs differ from the exact model, first at {bad[:8]}: "
                             f"got {g[bad[:3]]} want {want[bad[:3]]}")


def assert_rotation_bar(got, want: np.ndarray, what=""):
    """Each component within one float32 ulp of |z|, fewer than 1 in 1000 outputs differing at all."""
    g = got.cpu().numpy()
    ulp = np.spacing(np.abs(want.astype(np.complex128)).astype(np.float32)).astype(np.float64)
    dr = np.abs(g.real.astype(np.float64) - want.real)
    di = np.abs(g.imag.astype(np.float64) - want.imag)
    assert np.all(dr <= ulp) and np.all(di <= ulp), (what, float(np.max(dr / ulp)), float(np.max(di / ulp)))
    assert float(np.mean(g != want)) < 1e-3, (what, float(np.mean(g != want)))


def check_z(got, want, rotate, what=""):
    (assert_rotation_bar if rotate else assert_exact)(got, want, what)


# ---- lane tables --------------------------------------------------------------------------------------------------


class Lane:
    """One entry of a lane table and what the model says it must write."""

    def __init__(self, mp, gi, *, rotate=0, conj=0, scale=1.0 + 0j, rot_step=0, rot_base=0, finalize=1, raw_partials=0,
                 partial_in=None, fmt="s16"):
        self.mp, self.gi, self.fmt = mp, gi, fmt
        self.rotate, self.conj, self.scale = rotate, conj, scale
        self.rot_step, self.rot_base = rot_step % 2**64, rot_base % 2**64
        self.finalize, self.raw_partials, self.partial_in = finalize, raw_partials, partial_in
        self.out = None

    def pass_of(self, k_first):
        return next(p for p in self.mp.passes if p.group == self.gi and p.k_first == k_first)

    def fill(self, entry, k_first, n_out, device_afrag):
        import torch

        N = _N()
        P = _P()
        ps = self.pass_of(k_first)
        e = N.MfmaLane()
        e.afrag_dev = device_afrag[self.gi][ps.k_first * P.MFMA_KSTEP_BYTES :].data_ptr()
        if self.finalize:
            self.out = torch.full((n_out,), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda")
            e.z_out_dev = self.out.data_ptr()
        else:
            dt = torch.int32 if self.raw_partials else torch.float64
            self.out = torch.full((2 * n_out,), -7, dtype=dt, device="cuda")
            e.partial_out_dev = self.out.data_ptr()
        e.partial_in_dev = self.partial_in.data_ptr() if self.partial_in is not None else None
        e.unit = M.lane_unit(self.mp, self.gi, self.fmt)
        e.c_re, e.c_im = ps.c_re, ps.c_im
        e.rot_step, e.rot_base = self.rot_step, self.rot_base
        e.out_scale_re, e.out_scale_im = float(np.real(self.scale)), float(np.imag(self.scale))
        e.q_group, e.finalize, e.conj_sum, e.rotate = self.mp.groups[self.gi].q, self.finalize, self.conj, self.rotate
        e.raw_partials = self.raw_partials
        acc64 = not _acc32(self.mp, self.fmt)
        e.reserved = (1 if acc64 else 0) | (2 if self.mp.groups[self.gi].high_only else 0)
        return e


def _acc32(mp, fmt) -> bool:
    """Whether the lanes of this plan run with int32 sums: uint8 captures always do (row-staged slots only), int16 plans
    as ``make_plan`` / the test recorded (``plan_mfma(acc32=...)``)."""
    if fmt == "u8":
        assert getattr(mp, "_acc32", True), "uint8 lanes have int32 sums only"
        return True
    return bool(mp._acc32)


def make_plan(L, d, fmt, acc32, residual=False, max_ks=None, seed=0):
    mp = random_plan(L, d, fmt, acc32, residual, max_ks, seed)
    mp._acc32 = acc32
    return mp


_AFRAG = {}


def device_afrag(mp):
    from iq_to_audio_amd import _dev as D

    key = id(mp)
    if key not in _AFRAG:
        _AFRAG[key] = (mp, [D.from_numpy(g.afrag.reshape(-1).view(np.uint8)) for g in mp.groups])
    return _AFRAG[key][1]


def launch(entry, fmt, d, k_first, k_count, opb, lanes, x_dev, n_frames, consumed, m_first, n_out):
    """One call of iqa_channelize_mfma_multi / _pairs (``None`` in ``lanes``: a pair without a second lane)."""
    N = _N()
    P = _P()
    table = (N.MfmaLane * len(lanes))()
    for i, ln in enumerate(lanes):
        if ln is not None:
            table[i] = ln.fill(entry, k_first, n_out, device_afrag(ln.mp))
    name = "iqa_channelize_mfma_pairs" if entry == "pairs" else "iqa_channelize_mfma_multi"
    N.call(name, c_int32(P.FMT_CODE[fmt]), c_int32(d), c_int32(k_first), c_int32(k_count), c_int32(opb), table,
           c_int32(len(lanes)), N.ptr(x_dev), c_int64(n_frames), c_int64(consumed), c_int64(m_first), c_int64(n_out),
           N.stream_ptr())


_SUMS = {}


def _digest(a: np.ndarray) -> bytes:
    return hashlib.blake2b(np.ascontiguousarray(a).view(np.uint8), digest_size=16).digest()


def model_pass(ln, k_first, raw, d, consumed, m_first, n_out):
    """(v, d) of lane ``ln``'s pass starting at ``k_first``, memoised on the contents of the taps and the capture (lanes
    of one plan group share them)."""
    ps = ln.pass_of(k_first)
    key = (_digest(ln.mp.groups[ln.gi].tq), ln.fmt, ps.c_re, ps.c_im, M.lane_unit(ln.mp, ln.gi, ln.fmt), _acc32(ln.mp, ln.fmt),
           k_first, ps.k_count, ln.mp.groups[ln.gi].q, _digest(raw), raw.dtype.str, d, consumed, m_first, n_out)
    if key not in _SUMS:
        if len(_SUMS) > 64:
            _SUMS.clear()
        _SUMS[key] = M.pass_partial(ln.mp, ps, raw, ln.fmt, d, consumed, m_first, n_out, _acc32(ln.mp, ln.fmt))
    return _SUMS[key]


def model_lane_out(ln, k_first, raw, d, consumed, m_first, n_out, partial_in_model=None):
    """What lane ``ln`` writes: z (complex64), raw int32 partials, or double2 partials."""
    v, dd = model_pass(ln, k_first, raw, d, consumed, m_first, n_out)
    if ln.finalize == 0 and ln.raw_partials:
        return M.wrap32(v).astype(np.int32).reshape(-1)
    if partial_in_model is not None:
        dd = M.chain([partial_in_model.reshape(-1, 2), dd])
    if not ln.finalize:
        return dd.reshape(-1)
    return M.finish(dd, m_first, ln.conj, ln.rotate, ln.rot_step, ln.rot_base, ln.scale)


def check_lane(ln, k_first, raw, d, consumed, m_first, n_out, what, partial_in_model=None):
    import torch

    want = model_lane_out(ln, k_first, raw, d, consumed, m_first, n_out, partial_in_model)
    if ln.finalize:
        check_z(ln.out, want, ln.rotate, what)
    else:
        assert torch.equal(ln.out, torch.from_numpy(want).to(ln.out.device)), what
    return want


def _rot(rng):
    return int(rng.integers(0, 2**63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 2**63)) * 2


def setup_capture(fmt, d, mode, k_first, k_count, q_min, q_max, m_first, n_out, opb, seed, consumed=None, extra=0, data=None):
    """Device capture that holds exactly what the launch may read (+ ``extra`` frames), with random values behind it
    that a read past the bound would pick up.  ``data(fmt, n_frames)``: the values of the readable part (default: uniform
    full range, see ``capture``).  Returns (raw numpy, x_dev, n_frames, consumed)."""
    from iq_to_audio_amd import _dev as D

    if consumed is None:
        consumed = (m_first - 64 - 64 * q_max) * d + 1 - 3  # a mid-capture block: 3 frames before the first row
    n_frames = ring_frames_needed(mode, d, k_first, k_count, q_min, m_first, n_out, opb, consumed) + extra
    if mode == 1:  # the header's form of the contiguous bound
        n_frames = max(n_frames, (m_first + n_out - 2) * d + 512 * (-(-2 * d // 32)) - consumed + 1)
    raw = capture(fmt, n_frames + 4096, seed)
    if data is not None:
        raw[: 2 * n_frames] = capture(fmt, n_frames, seed, data=data)
    x_dev = D.to_device(raw, "int16" if fmt == "s16" else "uint8")
    assert_read_bounds(mode, d, k_first, k_count, q_min, q_max, m_first, n_out, opb, consumed, n_frames)
    return raw[: 2 * n_frames], x_dev, n_frames, consumed


# ---- every instantiation ------------------------------------------------------------------------------------------


SWEEP = X.sweep_cases()


@pytest.mark.parametrize("kind,ks,d", SWEEP, ids=[f"{k}-ks{ks}-d{d}" for k, ks, d in SWEEP])
def test_ring_instantiation_equals_model(A, kind, ks, d):
    """One launch of the named instantiation with two lanes of random full-scale taps: one exact (rotate 0), one
    rotated, conjugated and scaled by j; a mid-capture block (m_first, consumed > 0), ranges not a multiple of 8, a
    ragged last range.  Skip variants (SKIPK) mix a high-byte-only lane with a full-tap lane (the residual lanes of
    "fine" / "full").  64-bit sums: 16-bit taps without the int32 bound."""
    entry, fmt, acc64, skip = X.case_launch(kind, ks, d)
    name = X.sweep_kernel(kind, ks, d)
    assert -(-2 * d // 32) == ks
    _check_abi_selects(A, entry, fmt, d, 0, ks, acc64, name)
    L = 64 * d - d // 3 - 1  # 64 tap rows, not a multiple of D
    rng = np.random.default_rng(ks * 1000 + d)
    step, base = _rot(rng)
    if skip:
        mp = make_plan(L, d, fmt, not acc64, residual=True, seed=ks)
        assert mp.groups[0].high_only and not mp.groups[1].high_only
        lanes = [Lane(mp, 0, fmt=fmt), Lane(mp, 1, rotate=1, conj=1, scale=1j, rot_step=step, rot_base=base, fmt=fmt)]
    else:
        mp_a = make_plan(L, d, fmt, not acc64, seed=ks)
        mp_b = make_plan(L - 5, d, fmt, not acc64, seed=ks + 100)
        lanes = [Lane(mp_a, 0, fmt=fmt), Lane(mp_b, 0, rotate=1, conj=1, scale=1j, rot_step=step, rot_base=base, fmt=fmt)]
    mode = 2 if "rows" in name else 1
    opb, n_out = 256, 256 * 11 + 37 + ks
    m_first = 64 + 1000 + ks
    raw, x, n_frames, consumed = setup_capture(fmt, d, mode, 0, ks, 0, 0, m_first, n_out, opb, seed=ks + d)
    launch(entry, fmt, d, 0, ks, opb, lanes, x, n_frames, consumed, m_first, n_out)
    for i, ln in enumerate(lanes):
        check_lane(ln, 0, raw, d, consumed, m_first, n_out, f"{name} lane {i}")


# ---- per-lane kernel ----------------------------------------------------------------------------------------------


def _perlane_run(mp, raw_dev, n_frames, consumed, m_first, n_out, opb, fin_params):
    """Every pass of ``mp`` through iqa_channelize_mfma (reserved = 0), chained through double2 partials."""
    import torch

    N = _N()
    P = _P()
    afr = device_afrag(mp)
    z = torch.full((n_out,), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda")
    partial = torch.zeros(2 * n_out, dtype=torch.float64, device="cuda")
    for i, ps in enumerate(mp.passes):
        last = i == len(mp.passes) - 1
        grp = mp.groups[ps.group]
        assert perlane_frames_needed(fin_params.decimation, ps.k_first, ps.k_count, grp.q, m_first, n_out, opb, consumed) <= n_frames
        assert (m_first - 64 - 64 * grp.q) * fin_params.decimation + 1 - consumed >= 0
        prm = N.MfmaParams(outputs_per_block=opb, reserved=0, unit=grp.unit, c_re=ps.c_re, c_im=ps.c_im, debug_stamps=None,
                           q_group=grp.q, k_first=ps.k_first, k_count=ps.k_count, finalize=int(last),
                           partial_in_dev=partial.data_ptr() if i > 0 else None,
                           partial_out_dev=None if last else partial.data_ptr())
        N.call("iqa_channelize_mfma", byref(fin_params), byref(prm), N.ptr(afr[ps.group][ps.k_first * P.MFMA_KSTEP_BYTES :]),
               N.ptr(raw_dev), c_int64(n_frames), c_int64(consumed), c_int64(m_first), c_int64(n_out), N.ptr(z), N.stream_ptr())
    return z


@pytest.mark.parametrize("shape", ["d521_chained_ksteps", "d208_three_groups_kaiser", "d208_three_groups_random"])
def test_per_lane_kernel_equals_model(A, shape):
    """k_channelize_mfma_s16 (the per-lane kernel, reserved = 0): D = 521 as three chained k-step passes (partial_in /
    partial_out), and three tap-row groups at D = 208 (32769 taps: the Kaiser design of the 2.8 kHz filter, and random
    taps), 16-bit taps (the "full" precision's form off the contiguous slots), ragged last block."""
    from iq_to_audio_amd import _dev as D

    N = _N()
    P = _P()
    if shape == "d521_chained_ksteps":
        d, opb, n_out = 521, 1024, 3 * 1024 + 77
        L = 64 * d - 200
        mp = make_plan(L, d, "s16", False, max_ks=11, seed=521)
        assert [(p.k_first, p.k_count) for p in mp.passes] == [(0, 11), (11, 11), (22, 11)]
        rotate, rot_step, conj, scale = 0, 0, 0, 1.0 + 0j
    else:
        d, opb, n_out = 208, 512, 4 * 512 + 301
        if shape.endswith("kaiser"):
            taps = P.design_channel_filter(20e6, 2_800.0, d)
            L = len(taps)
            assert L == 32769
            plan = P.plan_channel(taps, sample_rate=20e6, freq_offset=-0.21 * 20e6, mix_sign=1, decimation=d, fmt="s16",
                                  iq_order="qi")
            mp = P.plan_mfma(plan)
            mp._acc32 = False
            rotate, rot_step, conj, scale = 1, plan.rot_step, plan.conj_sum, plan.out_scale
        else:
            L = 32769
            mp = make_plan(L, d, "s16", False, seed=208)
            rotate, rot_step, conj, scale = 0, 0, 1, -1j
        assert [g.q for g in mp.groups] == [0, 1, 2] and len(mp.passes) == 3
    q_max = max(g.q for g in mp.groups)
    m_first = 64 + 64 * q_max + 500
    consumed = (m_first - 64 - 64 * q_max) * d + 1 - 11
    n_frames = max(perlane_frames_needed(d, ps.k_first, ps.k_count, mp.groups[ps.group].q, m_first, n_out, opb, consumed)
                   for ps in mp.passes)
    raw = capture("s16", n_frames + 4096, seed=d)
    x = D.to_device(raw, "int16")
    raw = raw[: 2 * n_frames]
    prm = N.ChanParams(fmt=0, ntaps=L, decimation=d, conj_sum=conj, rotate=rotate, reserved=0,
                       rot_step=rot_step, rot_base=12345, out_scale_re=float(np.real(scale)), out_scale_im=float(np.imag(scale)))
    z = _perlane_run(mp, x, n_frames, consumed, m_first, n_out, opb, prm)
    want = M.finish(M.plan_sums(mp, raw, "s16", d, consumed, m_first, n_out, False), m_first, conj, rotate, rot_step, 12345, scale)
    check_z(z, want, rotate, shape)


# ---- 16-lane tables, partials, combine ----------------------------------------------------------------------------


def _combine(A, lanes_of_channel, m_first, n_out, raw_scale: bool, conj, rotate, step, base, scale):
    import torch

    N = _N()
    z = torch.full((n_out,), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda")
    ptrs = (c_void_p * len(lanes_of_channel))(*[ln.out.data_ptr() for ln in lanes_of_channel])
    sc = None
    if raw_scale:
        vals = []
        for ln in lanes_of_channel:
            ps = ln.mp.passes[[p.group for p in ln.mp.passes].index(ln.gi)]
            vals += [M.lane_unit(ln.mp, ln.gi, ln.fmt), ps.c_re, ps.c_im]
        sc = (c_double * len(vals))(*vals)
    prm = N.ChanParams(fmt=0, ntaps=1, decimation=1, conj_sum=conj, rotate=rotate, reserved=0, rot_step=step % 2**64,
                       rot_base=base % 2**64, out_scale_re=float(np.real(scale)), out_scale_im=float(np.imag(scale)))
    N.call("iqa_mfma_combine", byref(prm), ptrs, c_int32(len(lanes_of_channel)), sc, c_int64(m_first), c_int64(n_out), N.ptr(z),
           N.stream_ptr())
    return z


SIXTEEN_LANE_SHAPES = {  # shape -> (format, D, the kernel of every k-step range)
    "d104_raw_partials": ("s16", 104, "k_channelize_mfma_s16_ring_multi_half<7>"),
    "d521_chained_double_partials": ("s16", 521, "k_channelize_mfma_s16_ring_rows_multi<11>"),
    "u8_d25_raw_partials": ("u8", 25, "k_channelize_mfma_u8_ring_rows_multi<2>"),
    "u8_d521_chained_double_partials": ("u8", 521, "k_channelize_mfma_u8_ring_rows_multi<11>"),
}


@pytest.mark.parametrize("shape", list(SIXTEEN_LANE_SHAPES))
def test_sixteen_lanes_with_partials_and_combine(A, shape):
    """16 lanes (the maximum) in one table: five channels of three tap-row groups (finalize 0, q-groups 0..2 mixed in one
    launch) + one single-group channel that finishes z itself; every lane its own taps, unit, c, rotation, conjugation
    and out_scale.  D = 104 (the half-step kernel): the groups' raw int32 sums go to iqa_mfma_combine with raw_scale.
    D = 521 (row-staged, three k-step ranges (0,11), (11,11), (22,11): the later ones start 11 and 22 k steps into every
    row): three launches chained through double2 partial_in / partial_out, the combine adds the groups' double2 sums.
    The same for uint8 captures (the cu8 shapes: D = 25, an odd row of 50 bytes, and D = 521).  All against the model:
    the raw int32 and double2 partials bit for bit."""
    fmt, d, kernel = SIXTEEN_LANE_SHAPES[shape]
    rng = np.random.default_rng(d)
    max_ks = 11 if d == 521 else None
    ch_plans = [make_plan(64 * d * 2 + 1 + 37 * c, d, fmt, True, max_ks=max_ks, seed=50 + c) for c in range(5)]
    single = make_plan(40 * d + 3, d, fmt, True, max_ks=max_ks, seed=99)
    for mp in ch_plans:
        assert [g.q for g in mp.groups] == [0, 1, 2]
    kranges = [(p.k_first, p.k_count) for p in single.passes if p.group == 0]
    assert len(kranges) == (3 if d == 521 else 1)
    chans = []
    for c, mp in enumerate(ch_plans):
        step, base = _rot(rng)
        chans.append(dict(mp=mp, conj=c & 1, rotate=int(c % 3 != 0), scale=(1.0 + 0j, 1j, -1j)[c % 3], step=step, base=base))
    step1, base1 = _rot(rng)
    n_out, opb = 2 * 1000 + 3 if d == 521 else 6 * 640 + 5, 128
    m_first = 64 * 3 + 77
    mode = X.ring_mode(fmt, d, *kranges[0], False)
    raw_mode = len(kranges) == 1
    assert all(X.expected_kernel("multi", fmt, d, kf, kc, False, False) == kernel for kf, kc in kranges)
    consumed = (m_first - 64 - 64 * 2) * d + 1 - 2
    n_frames = max(ring_frames_needed(mode, d, kf, kc, 0, m_first, n_out, opb, consumed) for kf, kc in kranges)
    if mode == 1:  # the header's form of the contiguous bound
        n_frames = max(n_frames, (m_first + n_out - 2) * d + 512 * kranges[0][1] - consumed + 1)
    from iq_to_audio_amd import _dev as D

    raw = capture(fmt, n_frames + 4096, seed=d + 1)
    x = D.to_device(raw, "int16" if fmt == "s16" else "uint8")
    raw = raw[: 2 * n_frames]
    prev = {}
    final_lanes = None
    for ri, (kf, kc) in enumerate(kranges):
        last = ri == len(kranges) - 1
        _check_abi_selects(A, "multi", fmt, d, kf, kc, False, X.expected_kernel("multi", fmt, d, kf, kc, False, False))
        assert_read_bounds(mode, d, kf, kc, 0, 2, m_first, n_out, opb, consumed, n_frames)
        lanes = []
        for c, ch in enumerate(chans):
            for gi in range(3):
                lanes.append(Lane(ch["mp"], gi, finalize=0, raw_partials=int(raw_mode), partial_in=prev.get((c, gi)), fmt=fmt))
        lanes.append(Lane(single, 0, finalize=int(last), rotate=1, conj=1, scale=-1j, rot_step=step1, rot_base=base1,
                          partial_in=prev.get((5, 0)), fmt=fmt))
        assert len(lanes) == 16
        launch("multi", fmt, d, kf, kc, opb, lanes, x, n_frames, consumed, m_first, n_out)
        models = {}
        for i, ln in enumerate(lanes):
            key = (i // 3, i % 3) if i < 15 else (5, 0)
            pin = prev.get(key)
            pin_model = None if pin is None else prev_model[key]
            models[key] = check_lane(ln, kf, raw, d, consumed, m_first, n_out, f"{shape} range {ri} lane {i}", pin_model)
        prev = {((i // 3, i % 3) if i < 15 else (5, 0)): ln.out for i, ln in enumerate(lanes)}
        prev_model = models
        final_lanes = lanes
    for c, ch in enumerate(chans):
        group_lanes = final_lanes[3 * c : 3 * c + 3]
        z = _combine(A, group_lanes, m_first, n_out, raw_mode, ch["conj"], ch["rotate"], ch["step"], ch["base"], ch["scale"])
        if raw_mode:
            parts = [M.scaled_sum(prev_model[(c, gi)].reshape(-1, 2)[:, k], [p.c_re, p.c_im][k], M.lane_unit(ch["mp"], gi, fmt))
                     for gi in range(3) for p in [ch["mp"].passes[gi]] for k in (0, 1)]
            parts = [np.stack([parts[2 * gi], parts[2 * gi + 1]], axis=1) for gi in range(3)]
        else:
            parts = [prev_model[(c, gi)].reshape(-1, 2) for gi in range(3)]
        want = M.finish(M.chain(parts), m_first, ch["conj"], ch["rotate"], ch["step"], ch["base"], ch["scale"])
        check_z(z, want, ch["rotate"], f"{shape} channel {c} combined")


# ---- lane pairs ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("acc64", [False, True])
def test_lane_pairs_equal_multi_and_model(A, acc64):
    """iqa_channelize_mfma_pairs at D = 208 (13 k steps): pairs of descending tap-row groups (2,1), (1,0), (0,0), a pair
    without a second lane, and a first lane that is not high-byte-only (the kernel must not skip); equal to
    iqa_channelize_mfma_multi on the same lanes bit for bit, as the header promises, and to the model.  Two pair launches
    back to back (the pacing words are reused under a new token)."""
    fmt, d, ks = "s16", 208, 13
    mp3 = make_plan(64 * d * 3 - 41, d, fmt, not acc64, seed=7)
    mpr = make_plan(64 * d - 7, d, fmt, not acc64, residual=True, seed=8)
    assert [g.q for g in mp3.groups] == [0, 1, 2]
    rng = np.random.default_rng(3)

    def lanes_():
        out = []
        # pairs (2,1), (1,0), (0,0) -- the last with a first lane that is not high-byte-only --, (2, none), and the
        # residual plan's high-byte-only lane with its residue lane
        for i, (mp, gi) in enumerate([(mp3, 2), (mp3, 1), (mp3, 1), (mp3, 0), (mp3, 0), (mpr, 1), (mp3, 2), (None, None),
                                      (mpr, 0), (mpr, 1)]):
            if i == 7:  # the second lane of the fourth pair: none
                out.append(None)
                continue
            step, base = _rot(rng)
            out.append(Lane(mp, gi, rotate=i % 2, conj=(i // 2) % 2, scale=(1.0 + 0j, 1j, -1j)[i % 3], rot_step=step, rot_base=base))
        return out

    n_out, opb, m_first = 3 * 1024 + 19, 256, 64 * 3 + 300
    _check_abi_selects(A, "pairs", fmt, d, 0, ks, acc64, X.expected_kernel("pairs", fmt, d, 0, ks, acc64, False))
    raw, x, n_frames, consumed = setup_capture(fmt, d, 1, 0, ks, 0, 2, m_first, n_out, opb, seed=11)
    first = lanes_()
    launch("pairs", fmt, d, 0, ks, opb, first, x, n_frames, consumed, m_first, n_out)
    for i, ln in enumerate(first):
        if ln is not None:
            check_lane(ln, 0, raw, d, consumed, m_first, n_out, f"pairs lane {i}")
    # the same lanes (same rotations) once more as pairs, and as one lane per workgroup
    again = [None if ln is None else Lane(ln.mp, ln.gi, rotate=ln.rotate, conj=ln.conj, scale=ln.scale, rot_step=ln.rot_step,
                                          rot_base=ln.rot_base) for ln in first]
    launch("pairs", fmt, d, 0, ks, opb, again, x, n_frames, consumed, m_first, n_out)
    single = [Lane(ln.mp, ln.gi, rotate=ln.rotate, conj=ln.conj, scale=ln.scale, rot_step=ln.rot_step, rot_base=ln.rot_base)
              for ln in first if ln is not None]
    launch("multi", fmt, d, 0, ks, opb, single, x, n_frames, consumed, m_first, n_out)
    import torch

    for a_, b_ in zip([ln for ln in first if ln is not None], single):
        assert torch.equal(a_.out, b_.out)
    for a_, b_ in zip(first, again):
        if a_ is not None:
            assert torch.equal(a_.out, b_.out)
    # a pair table whose first lanes are all high-byte-only: the SKIPK variant
    sk = [Lane(mpr, 0), Lane(mpr, 1, rotate=1, rot_step=12345678901, rot_base=2**63 + 5)]
    _check_abi_selects(A, "pairs", fmt, d, 0, ks, acc64, X.expected_kernel("pairs", fmt, d, 0, ks, acc64, True))
    launch("pairs", fmt, d, 0, ks, opb, sk, x, n_frames, consumed, m_first, n_out)
    for i, ln in enumerate(sk):
        check_lane(ln, 0, raw, d, consumed, m_first, n_out, f"skip pair lane {i}")


def test_lane_pairs_without_pacing_buffer(A):
    """More pacing words than the library's buffer holds (16 lanes = 8 pairs, 32 outputs per range: > RG_PACE_WORDS):
    the kernel runs without pacing and must still equal the model.  D = 160 (10 k steps)."""
    fmt, d, ks = "s16", 160, 10
    opb = 32
    n_out = RG_PACE_WORDS // 8 * 32 + 32 * 9 + 1  # ranges past 2048 + a last range of one output
    groups = -(-(-(-n_out // opb)) // 8)
    assert groups * 8 * 8 > RG_PACE_WORDS
    plans = [make_plan(64 * d - 1 - 3 * i, d, fmt, True, seed=300 + i) for i in range(4)]
    rng = np.random.default_rng(4)
    lanes = []
    for i in range(16):
        step, base = _rot(rng)
        lanes.append(Lane(plans[i % 4], 0, rotate=int(i % 4 == 3), conj=i & 1, scale=(1.0 + 0j, 1j, -1j)[i % 3], rot_step=step,
                          rot_base=base))
    m_first = 64 + 5
    _check_abi_selects(A, "pairs", fmt, d, 0, ks, False, X.expected_kernel("pairs", fmt, d, 0, ks, False, False))
    raw, x, n_frames, consumed = setup_capture(fmt, d, 1, 0, ks, 0, 0, m_first, n_out, opb, seed=12)
    launch("pairs", fmt, d, 0, ks, opb, lanes, x, n_frames, consumed, m_first, n_out)
    for i, ln in enumerate(lanes):
        check_lane(ln, 0, raw, d, consumed, m_first, n_out, f"unpaced lane {i}")


# ---- launch geometry ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", ["lead_in_d104", "lead_in_rows_d25", "phase_wrap_d208", "opb32_d100", "opb64_rows_d75", "opb32_u8_d104"])
def test_launch_geometry(A, case):
    """A zero lead-in (consumed < 0, m_first = 0); m around 2^33 (m * rot_step is reduced mod 2^64 many times over)
    with rot_base chosen so that the phase rot_base + m rot_step wraps past 2^64 once inside the launch, at a chosen
    output; and small outputs_per_block (32, 64): launches of one, two and many ring rounds per workgroup, a last range
    of one output."""
    from iq_to_audio_amd import _dev as D

    fmt = "u8" if "u8" in case else "s16"
    d = int(case.rsplit("_d", 1)[1])
    ks = -(-2 * d // 32)
    mode = 1 if (fmt == "s16" and d % 4 == 0) else 2
    mp = make_plan(64 * d - 13, d, fmt, True, seed=d)
    step, base = 0x9E3779B97F4A7C15, 0
    rotate = 1
    if case.startswith("lead_in"):
        m_first, n_out, opb = 0, 5000, 512
        consumed = -(64 * d) + 1  # raw starts 64 D - 1 frames before global frame 0: zeros
    elif case.startswith("phase_wrap"):
        m_first, n_out, opb = 2**33 + 12345, 4000 + 3, 256
        consumed = (m_first - 64) * d - 5
        step = 0x123456789ABD  # ~9e5 outputs per turn: one wrap in the launch
        i_wrap = 977
        base = (3 - (m_first + i_wrap) * step) % 2**64  # the phase of output m_first + i_wrap is 3, of the one before 2^64 - step + 3
    else:
        opb = int(case.split("_")[0][3:])
        m_first, n_out = 64 + 3, opb * 37 + 1
        consumed = 0
    n_frames = ring_frames_needed(mode, d, 0, ks, 0, m_first, n_out, opb, consumed)
    if mode == 1:
        n_frames = max(n_frames, (m_first + n_out - 2) * d + 512 * ks - consumed + 1)
    assert_read_bounds(mode, d, 0, ks, 0, 0, m_first, n_out, opb, consumed, n_frames)
    raw = capture(fmt, n_frames + 4096, seed=d + 5)
    if consumed < 0:
        raw[: 2 * (-consumed)] = 0 if fmt == "s16" else 128  # the filter's zero initial state (uint8: 128 is zero)
    x = D.to_device(raw, "int16" if fmt == "s16" else "uint8")
    raw = raw[: 2 * n_frames]
    lanes = [Lane(mp, 0, fmt=fmt), Lane(mp, 0, rotate=rotate, conj=1, scale=1j, rot_step=step, rot_base=base, fmt=fmt)]
    launch("multi", fmt, d, 0, ks, opb, lanes, x, n_frames, consumed, m_first, n_out)
    for i, ln in enumerate(lanes):
        check_lane(ln, 0, raw, d, consumed, m_first, n_out, f"{case} lane {i}")
    if case.startswith("phase_wrap"):  # exactly one wrap, where it was put
        ph = [(base + (m_first + i) * step) % 2**64 for i in range(n_out)]
        assert [i for i in range(1, n_out) if ph[i] < ph[i - 1]] == [i_wrap]
        assert ph[i_wrap] == 3 and ph[i_wrap - 1] > 2**64 - 2 * step


@pytest.mark.parametrize("d,acc64", [(104, False), (104, True), (75, False)], ids=["contiguous-int32", "contiguous-int64", "rows-int32"])
def test_single_channel_ring_entry_equals_one_lane_launch(A, d, acc64):
    """The ring branch of iqa_channelize_mfma (reserved = 64 | 128: int32 sums, 64: 64-bit sums) is a one-lane launch of
    iqa_channelize_mfma_multi: the package's own driver calls only the latter, callers of the C ABI may use either.  The
    same rotated, conjugated, scaled lane through both entries: z byte for byte the same (and the model's)."""
    import torch

    N, P = _N(), _P()
    ks = -(-2 * d // 32)
    mode = X.ring_mode("s16", d, 0, ks, acc64)
    assert mode == (1 if d % 4 == 0 else 2)
    L = 64 * d - 13
    mp = make_plan(L, d, "s16", not acc64, seed=d + 1)
    step, base = _rot(np.random.default_rng(d))
    opb, n_out, m_first = 256, 256 * 5 + 37, 64 + 500
    raw, x, n_frames, consumed = setup_capture("s16", d, mode, 0, ks, 0, 0, m_first, n_out, opb, seed=d + 2)
    ln = Lane(mp, 0, rotate=1, conj=1, scale=1j, rot_step=step, rot_base=base)
    launch("multi", "s16", d, 0, ks, opb, [ln], x, n_frames, consumed, m_first, n_out)
    check_lane(ln, 0, raw, d, consumed, m_first, n_out, f"one lane, d={d}, acc64={acc64}")
    ps = ln.pass_of(0)
    chan = N.ChanParams(fmt=P.FMT_CODE["s16"], ntaps=L, decimation=d, conj_sum=1, rotate=1, reserved=0, rot_step=ln.rot_step,
                        rot_base=ln.rot_base, out_scale_re=0.0, out_scale_im=1.0)
    prm = N.MfmaParams(outputs_per_block=opb, reserved=64 | (0 if acc64 else 128), unit=M.lane_unit(mp, 0, "s16"), c_re=ps.c_re,
                       c_im=ps.c_im, debug_stamps=None, q_group=0, k_first=0, k_count=ks, finalize=1, partial_in_dev=None,
                       partial_out_dev=None)
    z = torch.full((n_out,), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda")
    N.call("iqa_channelize_mfma", byref(chan), byref(prm), N.ptr(device_afrag(mp)[0]), N.ptr(x), c_int64(n_frames),
           c_int64(consumed), c_int64(m_first), c_int64(n_out), N.ptr(z), N.stream_ptr())
    assert torch.equal(torch.view_as_real(z).view(torch.int32), torch.view_as_real(ln.out).view(torch.int32))


SINGLE_ROW = [("s16", 104, 104), ("s16", 104, 37), ("s16", 521, 521), ("s16", 521, 300), ("u8", 25, 25), ("u8", 521, 200)]


@pytest.mark.parametrize("fmt,d,L", SINGLE_ROW, ids=[f"{f}-d{d}-L{L}" for f, d, L in SINGLE_ROW])
def test_single_tap_row_filters(A, fmt, d, L):
    """L <= D: tap row 1 is the only one with taps (the other 63 rows, and the K padding, are zero).  D = 104 in one
    contiguous-slot launch; D = 521 as three row-staged k-step ranges chained through double2 partials (with L = 300
    the first range holds no tap at all); uint8 at D = 25 and 521.  An exact lane and a rotated one, against the model."""
    from iq_to_audio_amd import _dev as D

    max_ks = 11 if d == 521 else None
    mp = make_plan(L, d, fmt, True, max_ks=max_ks, seed=L)
    tq = mp.groups[0].tq
    assert [g.q for g in mp.groups] == [0]
    assert np.any(tq[0]) and np.any(tq[64]) and not np.any(tq[1:64]) and not np.any(tq[65:])
    kranges = [(p.k_first, p.k_count) for p in mp.passes]
    assert len(kranges) == (3 if d == 521 else 1)
    mode = X.ring_mode(fmt, d, *kranges[0], False)
    opb, n_out, m_first = 128, 2500 + 3, 64 + 21
    consumed = (m_first - 64) * d + 1 - 7
    n_frames = max(ring_frames_needed(mode, d, kf, kc, 0, m_first, n_out, opb, consumed) for kf, kc in kranges)
    if mode == 1:  # the header's form of the contiguous bound
        n_frames = max(n_frames, (m_first + n_out - 2) * d + 512 * kranges[0][1] - consumed + 1)
    raw = capture(fmt, n_frames + 4096, seed=L + d)
    x = D.to_device(raw, "int16" if fmt == "s16" else "uint8")
    raw = raw[: 2 * n_frames]
    prev, prev_model = [None, None], [None, None]
    for ri, (kf, kc) in enumerate(kranges):
        last = ri == len(kranges) - 1
        _check_abi_selects(A, "multi", fmt, d, kf, kc, False, X.expected_kernel("multi", fmt, d, kf, kc, False, False))
        assert_read_bounds(mode, d, kf, kc, 0, 0, m_first, n_out, opb, consumed, n_frames)
        lanes = [Lane(mp, 0, finalize=int(last), partial_in=prev[0], fmt=fmt),
                 Lane(mp, 0, finalize=int(last), rotate=1, conj=1, scale=-1j, rot_step=0x0F1E2D3C4B5A6978, rot_base=2**63 + 1,
                      partial_in=prev[1], fmt=fmt)]
        launch("multi", fmt, d, kf, kc, opb, lanes, x, n_frames, consumed, m_first, n_out)
        prev_model = [check_lane(ln, kf, raw, d, consumed, m_first, n_out, f"L={L} range {ri} lane {i}", prev_model[i])
                      for i, ln in enumerate(lanes)]
        prev = [ln.out for ln in lanes]


# ---- the int32 bound, reached -------------------------------------------------------------------------------------


def test_adversarial_capture_reaches_the_int32_bound(A):
    """32767 sign(tap) aligned to one output's window, per component: the "fast" plan's one-int32 sums (C2 shape:
    6401 random full-scale taps at D = 104) reach >= 90 % of 2^31 -- the bound plan_mfma(acc32=True) guarantees -- and
    the kernel still equals the model (nothing wrapped)."""
    from iq_to_audio_amd import _dev as D

    fmt, d, ks = "s16", 104, 7
    mp = make_plan(6401, d, fmt, True, seed=6401)
    opb, n_out, m_first = 256, 2048 + 7, 64 + 40
    raw, _, n_frames, consumed = setup_capture(fmt, d, 1, 0, ks, 0, 0, m_first, n_out, opb, seed=13)
    raw = raw.copy()
    t = mp.groups[0].tq
    targets = {0: m_first + 300, 1: m_first + 1300}  # component -> output (windows far apart)
    for comp, m in targets.items():
        for qq in range(1, 65):
            b = m - qq
            base = 2 * (b * d + 1 - consumed)
            row = t[comp * 64 + qq - 1, : 2 * d]
            raw[base : base + 2 * d] = np.where(row > 0, 32767, np.where(row < 0, -32767, 0)).astype(np.int16)
    x = D.to_device(raw, "int16")
    s1, s2 = M.pass_sums(t, raw, fmt, d, 0, 0, ks, consumed, m_first, n_out)
    v64, v32 = M.ring_value(s1, s2, False), M.ring_value(s1, s2, True)
    assert np.array_equal(v64, v32)
    for comp, m in targets.items():
        assert abs(int(v64[m - m_first, comp])) >= 0.9 * 2**31, (comp, int(v64[m - m_first, comp]))
    lanes = [Lane(mp, 0), Lane(mp, 0, finalize=0, raw_partials=1)]
    launch("multi", fmt, d, 0, ks, opb, lanes, x, n_frames, consumed, m_first, n_out)
    for i, ln in enumerate(lanes):
        check_lane(ln, 0, raw, d, consumed, m_first, n_out, f"adversarial lane {i}")


# ---- the gap this file closes -------------------------------------------------------------------------------------


def test_one_lsb_in_an_outer_tap_row_is_caught_by_the_exact_bar_only(A):
    """A Kaiser filter at the C2 shape (6401 taps, D = 104, "fast" plan): one low tap byte of the outermost tap row
    changed by one LSB in the fragments uploaded to the GPU.  The exact comparison with the model catches it on the
    outputs it touches; the float32 VALU kernel comparison the suite used so far (2e-5 RMS, 1.2e-4 max of full scale)
    does not."""
    import torch

    from iq_to_audio_amd import _dev as D

    N = _N()
    P = _P()
    fs, d, ks = 10e6, 104, 7
    taps = P.design_channel_filter(fs, 12_500.0, d)
    assert len(taps) == 6401
    plan = P.plan_channel(taps, sample_rate=fs, freq_offset=0.113 * fs, mix_sign=1, decimation=d, fmt="s16", iq_order="iq",
                          padded_len=int(N.lib().iqa_taps_padded_len(len(taps))))
    mp = P.plan_mfma(plan, acc32=True)
    mp._acc32 = True
    rows = -(-len(taps) // d)
    assert rows == 62
    # the outermost tap row (qq = 62, real-output component), a column whose tap is non-zero and whose low byte can grow
    r = rows - 1
    tq = mp.groups[0].tq.copy()
    q1, q2 = M.split_taps(tq)
    col = int(next(c for c in range(2 * d) if tq[r, c] != 0 and q2[r, c] < 127))
    frag = mp.groups[0].afrag.copy()
    # fragment layout [kstep][rowtile][piece][lane][16]: row r -> rowtile r // 32, lane (r % 32) + 32 * ((col % 32) // 16)
    kst, j = col // 32, col % 16
    lane = (r % 32) + 32 * ((col % 32) // 16)
    assert frag[kst, r // 32, 1, lane, j] == q2[r, col]
    frag[kst, r // 32, 1, lane, j] += 1
    tq_bad = tq.copy()
    tq_bad[r, col] += 1
    opb, n_out, m_first = 512, 8192 + 5, 64 + 10
    s16 = O.synth_capture_s16(fs, 0.2, 25e3).reshape(-1)
    consumed = 0
    n_frames = max(ring_frames_needed(1, d, 0, ks, 0, m_first, n_out, opb, consumed),
                   (m_first + n_out - 2) * d + 512 * ks - consumed + 1)
    assert_read_bounds(1, d, 0, ks, 0, 0, m_first, n_out, opb, consumed, n_frames)
    raw = s16[: 2 * n_frames]
    x = D.to_device(s16, "int16")
    bad_dev = [D.from_numpy(frag.reshape(-1).view(np.uint8))]
    good, bad = Lane(mp, 0), Lane(mp, 0)
    launch("multi", "s16", d, 0, ks, opb, [good], x, n_frames, consumed, m_first, n_out)
    _AFRAG[id(mp)] = (mp, bad_dev)
    try:
        launch("multi", "s16", d, 0, ks, opb, [bad], x, n_frames, consumed, m_first, n_out)
    finally:
        _AFRAG.pop(id(mp))
    exact = model_lane_out(good, 0, raw, d, consumed, m_first, n_out)
    assert_exact(good.out, exact, "unperturbed")
    ps = mp.passes[0]
    vb = M.ring_value(*M.pass_sums(tq_bad, raw, "s16", d, 0, 0, ks, consumed, m_first, n_out), True)
    perturbed = M.finish(np.stack([M.scaled_sum(vb[:, 0], ps.c_re, mp.groups[0].unit), M.scaled_sum(vb[:, 1], ps.c_im, mp.groups[0].unit)], 1),
                         m_first, 0, 0)
    assert_exact(bad.out, perturbed, "perturbed kernel vs perturbed model")
    got = bad.out.cpu().numpy()
    touched = perturbed != exact
    assert touched.mean() > 0.5  # the data's high byte is zero only at the tone's zero crossings
    assert np.array_equal(got != exact, touched)  # the exact bar fails precisely on the outputs the byte reaches
    # the VALU kernel on the same outputs (rotate 0, as the lanes above), with the bar of test_ring_kernel_every_kstep_count
    prm = N.ChanParams(fmt=0, ntaps=plan.ntaps, decimation=d, conj_sum=0, rotate=0, reserved=0, rot_step=0, rot_base=0,
                       out_scale_re=1.0, out_scale_im=0.0)
    taps_dev = D.from_numpy(plan.taps_window)
    valu = torch.empty(n_out, dtype=torch.complex64, device="cuda")
    N.call("iqa_channelize", byref(prm), N.ptr(taps_dev), N.ptr(x), c_int64(n_frames), c_int64(consumed), None, c_int64(m_first),
           c_int64(n_out), N.ptr(valu), N.stream_ptr())
    v = valu.cpu().numpy()
    err = got.astype(np.complex128) - v
    rms_err = float(np.sqrt(np.mean(np.abs(err) ** 2)))
    assert rms_err < 2e-5 and float(np.abs(err).max()) < 1.2e-4, (rms_err, float(np.abs(err).max()))


# ---- the pipeline -------------------------------------------------------------------------------------------------


def _direct(plan, raw, m_first, n_out):
    """float64 direct convolution with the unquantised taps, rotated in float64: z[m] for m_first .. m_first + n_out - 1."""
    g = plan.taps_natural  # (conjugated on the host for conjugating sample orders; finish() conjugates the sum)
    xc = raw[0::2].astype(np.float64) + 1j * raw[1::2].astype(np.float64)
    d = plan.decimation
    lo = max(0, m_first * d - (len(g) - 1))
    seg = xc[lo : (m_first + n_out - 1) * d + 1]
    nfft = 1 << int(np.ceil(np.log2(seg.size + g.size)))
    conv = np.fft.ifft(np.fft.fft(seg, nfft) * np.fft.fft(g, nfft))
    s = conv[np.arange(m_first, m_first + n_out) * d - lo]
    dd = np.stack([s.real, s.imag], axis=1)
    return M.finish(dd, m_first, plan.conj_sum, plan.rotate, plan.rot_step, plan.rot_base, plan.out_scale, cast=False)


def _check_channel_blocks(ch, mp, blocks_out, raw, cuts, wide, acc32, what):
    """The matrix-core interior of every block against the model (rotation bar) and the float64 direct convolution (the
    plan's own z_error_rms)."""
    k = ch._kernel
    plan = k.plan
    checked = 0
    for (c0, c1), z in zip(cuts, blocks_out):
        m_first = -(-c0 // plan.decimation)
        n_out = z.numel()
        m_a, m_b = k._interior(c0, c1 - c0, m_first, n_out)
        n_int = m_b - m_a
        assert n_int >= 4096, (what, n_int)
        want = M.finish(M.plan_sums(mp, raw, plan.fmt, plan.decimation, 0, m_a, n_int, acc32), m_a, plan.conj_sum, plan.rotate,
                        plan.rot_step, plan.rot_base, plan.out_scale)
        got = z[m_a - m_first : m_b - m_first]
        assert_rotation_bar(got, want, what)
        ref = _direct(plan, raw, m_a, n_int)
        g = got.cpu().numpy().astype(np.complex128)
        err = float(np.sqrt(np.mean(np.abs(g - ref) ** 2)))
        f32 = 2.0**-24 * float(np.sqrt(np.mean(np.abs(ref) ** 2)))  # the float32 rounding of z itself
        bar = 2.0 * mp.z_error_rms(wide) + f32
        assert err < bar, (what, err, mp.z_error_rms(wide), f32)
        checked += n_int
    return checked


@pytest.mark.parametrize("precision", ["fast", "fine", "full"])
def test_channelizer_interior_equals_model(A, precision):
    """Channelizer at the C2 shape (10 MS/s, D = 104, 6401 taps) over two ragged blocks: the outputs the matrix cores
    produce equal the model (rotation bar) and stay within the plan's own z_error_rms of a float64 direct convolution
    with the unquantised taps, over tens of thousands of outputs."""
    import torch

    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import processing as PR

    fs, d = 10e6, 104
    n = 60_000 * d + 777
    f_off = 0.113 * fs
    raw = O.synth_capture_s16(fs, n / fs, 25e3, seed=9).reshape(-1)[: 2 * n]
    wide = float(np.sqrt(np.mean((raw.astype(np.float64) / 32768.0) ** 2) * 2.0))
    x = D.to_device(raw, "int16")
    taps = A.design_channel_filter(fs, 12_500.0, d)
    cut = 31_000 * d + 55
    old = PR._ChannelKernel.mfma_min_outputs
    try:
        PR._ChannelKernel.mfma_min_outputs = 4096
        ch = A.Channelizer(taps, sample_rate=fs, freq_offset=f_off, mix_sign=1, decimation=d, precision=precision)
        outs = [ch.process(x[: 2 * cut])]
        assert ch._kernel.last_kernel == "k_channelize_mfma_s16_ring", ch._kernel.last_kernel
        outs.append(ch.process(x[2 * cut :]))
        assert ch._kernel.last_kernel == "k_channelize_mfma_s16_ring", ch._kernel.last_kernel
        torch.cuda.synchronize()
    finally:
        PR._ChannelKernel.mfma_min_outputs = old
    mp = ch._kernel.mfma
    assert len(mp.groups) == (1 if precision == "fast" else 2)
    n_checked = _check_channel_blocks(ch, mp, outs, raw, [(0, cut), (cut, n)], wide, ch._kernel.acc32, precision)
    assert n_checked > 50_000


def test_channel_bank_c3_like_interior_equals_model(A):
    """A ChannelBank of C3-like targets (20 MS/s, D = 208: two 12.5 kHz channels and a 2.8 kHz one of three tap-row groups,
    mixed mixer signs, one launch of lane pairs + the combine) over two ragged blocks: every channel's matrix-core interior
    equals the model (rotation bar) and stays within its plan's z_error_rms of a float64 direct convolution."""
    import torch

    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import processing as PR

    fs, d = 20e6, 208
    n = 40_000 * d + 1234
    specs = [(-3.1e6, 12_500.0, 1), (4.2e6, 2_800.0, -1), (0.9e6, 12_500.0, -1)]
    raw = O.synth_capture_s16(fs, n / fs, specs[0][0], seed=3).reshape(-1)[: 2 * n]
    wide = float(np.sqrt(np.mean((raw.astype(np.float64) / 32768.0) ** 2) * 2.0))
    x = D.to_device(raw, "int16")
    cut = 19_000 * d + 321
    old = PR._ChannelKernel.mfma_min_outputs
    try:
        PR._ChannelKernel.mfma_min_outputs = 4096
        chans = [A.Channelizer(A.design_channel_filter(fs, bw, d), sample_rate=fs, freq_offset=off, mix_sign=sign, decimation=d)
                 for off, bw, sign in specs]
        bank = A.ChannelBank(chans)
        first = bank.process(x[: 2 * cut])
        info = dict(bank.last_launch)
        second = bank.process(x[2 * cut :])
        torch.cuda.synchronize()
    finally:
        PR._ChannelKernel.mfma_min_outputs = old
    assert info["lanes"] == 5 and info["pairs"] == 3 and info["combines"] == 1, info
    total = 0
    for i, c in enumerate(chans):
        assert c._kernel.last_kernel == "k_channelize_mfma_s16_ring"
        k = c._kernel
        # the bank's interior is the one common to its channels: compare each channel over that span
        spans = [[kk._interior(c0, c1 - c0, -(-c0 // d), z.numel()) for kk in (ch_._kernel for ch_ in chans)]
                 for (c0, c1), z in zip([(0, cut), (cut, n)], [first[i], second[i]])]
        for (c0, c1), z, sp in zip([(0, cut), (cut, n)], [first[i], second[i]], spans):
            m_first = -(-c0 // d)
            m_a, m_b = max(s[0] for s in sp), min(s[1] for s in sp)
            want = M.finish(M.plan_sums(k.mfma, raw, "s16", d, 0, m_a, m_b - m_a, True), m_a, k.plan.conj_sum, k.plan.rotate,
                            k.plan.rot_step, k.plan.rot_base, k.plan.out_scale)
            got = z[m_a - m_first : m_b - m_first]
            assert_rotation_bar(got, want, f"bank channel {i}")
            ref = _direct(k.plan, raw, m_a, m_b - m_a)
            g = got.cpu().numpy().astype(np.complex128)
            err = float(np.sqrt(np.mean(np.abs(g - ref) ** 2)))
            bar = 2.0 * k.mfma.z_error_rms(wide) + 2.0**-24 * float(np.sqrt(np.mean(np.abs(ref) ** 2)))
            assert err < bar, (i, err, bar)
            total += m_b - m_a
    assert total > 100_000
