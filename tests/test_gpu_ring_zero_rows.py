"""The half-step ring kernel on rotated tap fragments (k_channelize_mfma_s16_ring_multi_half<KS, ONCE, ZEDGE>: the all-zero
high tap bytes of a filter's edge rows are not multiplied) against the exact integer model of
tests/channelizer_model.py and against the unrotated launch of the same data: integer sums, so z is equal bit for bit.

One lane per launch (the launches that take the variant).  Shapes: D = 104 with the 6401-tap Kaiser filter of the headline
(7 k steps, folded odd step, rot 12: the wrap inside slots 0..15) at mixer sign +1 and -1; D = 40 (3 k steps, rot 8); D = 8
(1 k step: the folded step alone; rot 20: the wrap inside slots 16..31); D = 100 (7 k steps, 8 values in the last one, rot 4) --
the last three with random full-scale taps whose edge rows are scaled down until their high byte is zero.  A range of 704
outputs and a ragged one of 37: more than the 512 positions of the sliding window, so its slots are reused.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_mfma_exact import Lane, _N, _P, _rot, assert_exact, device_afrag, launch, model_lane_out, setup_capture

pytestmark = pytest.mark.gpu

FMT, OPB, N_OUT, M_FIRST = "s16", 704, 704 + 37, 64 + 1000
ZEDGE, PLAIN = b"k_channelize_mfma_s16_ring_multi_half<KS, ONCE, ZEDGE>", b"k_channelize_mfma_s16_ring_multi_half<KS, ONCE>"


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _ks(d):
    return -(-2 * d // 32)


_PLANS = {}


def _kaiser_plan(sign):
    P = _P()
    fs, d = 10e6, 104
    taps = P.design_channel_filter(fs, 12_500.0, d)
    assert len(taps) == 6401
    plan = P.plan_channel(taps, sample_rate=fs, freq_offset=0.113 * fs, mix_sign=sign, decimation=d, fmt=FMT, iq_order="iq",
                          padded_len=int(_N().lib().iqa_taps_padded_len(len(taps))))
    return P.plan_mfma(plan, acc32=True)


def _edge_plan(d, rot, seed):
    """Random full-scale taps over 64 tap rows; the last ``rot`` rows and the first 20 - rot (at least 2) a thousandth of that."""
    P = _P()
    rng = np.random.default_rng(seed)
    L = 64 * d - d // 3 - 1
    g = rng.uniform(-1.0, 1.0, L) + 1j * rng.uniform(-1.0, 1.0, L)
    row = np.arange(L) // d
    g[(row >= 64 - rot) | (row < max(20 - rot, 2))] *= 1e-3
    plan = P.ChannelPlan(fmt=FMT, ntaps=L, decimation=d, taps_window=None, conj_sum=0, rotate=0, rot_step=0, rot_base=0,
                         out_scale=1.0 + 0j, taps_natural=g * P.INGEST_SCALE[FMT])
    return P.plan_mfma(plan, acc32=True)


SHAPES = {  # name -> (D, rot, plan)
    "d104-kaiser-sign+": (104, 12, lambda: _kaiser_plan(1)),
    "d104-kaiser-sign-": (104, 12, lambda: _kaiser_plan(-1)),
    "d40-ks3": (40, 8, lambda: _edge_plan(40, 8, 40)),
    "d8-ks1": (8, 20, lambda: _edge_plan(8, 20, 8)),
    "d100-ks7": (100, 4, lambda: _edge_plan(100, 4, 100)),
}


def _plan(shape):
    if shape not in _PLANS:
        d, rot, make = SHAPES[shape]
        mp = make()
        mp._acc32 = True
        assert mp.ksteps == _ks(d) and mp.groups[0].rot == rot and mp.groups[0].afrag_rot is not None, (shape, mp.groups[0].rot)
        _PLANS[shape] = mp
    return _PLANS[shape]


_ROT_DEV = {}


class RotLane(Lane):
    """The same lane on the rotated fragments: afrag_rot and its rot in bits 8..13 of ``reserved``."""

    def fill(self, entry, k_first, n_out, device_afrag):
        from iq_to_audio_amd import _dev as D

        g = self.mp.groups[self.gi]
        key = id(self.mp)
        if key not in _ROT_DEV:
            _ROT_DEV[key] = (self.mp, D.from_numpy(g.afrag_rot.reshape(-1).view(np.uint8)))
        e = super().fill(entry, k_first, n_out, device_afrag)
        e.afrag_dev = _ROT_DEV[key][1].data_ptr()
        e.reserved |= g.rot << 8
        return e


def _both(A, shape, consumed=None, data=None, seed=0, rotate=False, what=""):
    """The rotated and the unrotated launch of one lane over the same capture: each against the model (exact; a rotated
    output within the rotation's own bar is not asked for here: the lanes do not rotate unless ``rotate``), and against each other."""
    import torch

    d = SHAPES[shape][0]
    mp = _plan(shape)
    kw = {}
    if rotate:
        step, base = _rot(np.random.default_rng(d))
        kw = dict(rotate=1, conj=1, scale=1j, rot_step=step, rot_base=base)
    raw, x, n_frames, consumed = setup_capture(FMT, d, 1, 0, _ks(d), 0, 0, M_FIRST, N_OUT, OPB, seed=d + seed, consumed=consumed, data=data)
    lib = _N().lib()
    assert lib.iqa_mfma_ring_zero_rows(0, d, 0, _ks(d), 1) == 1
    new, old = RotLane(mp, 0, **kw), Lane(mp, 0, **kw)
    launch("multi", FMT, d, 0, _ks(d), OPB, [new], x, n_frames, consumed, M_FIRST, N_OUT)
    assert lib.iqa_mfma_ring_last_kernel() == ZEDGE
    launch("multi", FMT, d, 0, _ks(d), OPB, [old], x, n_frames, consumed, M_FIRST, N_OUT)
    assert lib.iqa_mfma_ring_last_kernel() == PLAIN
    assert torch.equal(new.out, old.out), f"{shape} {what}: rotated and unrotated launch differ"
    if not rotate:
        assert_exact(new.out, model_lane_out(new, 0, raw, d, consumed, M_FIRST, N_OUT), f"{shape} {what}")
    return new.out


def _first_row_frame(d):
    return (M_FIRST - 64) * d + 1


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rotated_launch_equals_model_and_unrotated_launch(A, shape):
    """A mid-capture block (consumed > 0: the launch continues a previous block), uniform full-range data."""
    _both(A, shape, what="mid-capture")


@pytest.mark.parametrize("phase", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", ["d104-kaiser-sign+", "d8-ks1"])
def test_stream_phases(A, shape, phase):
    d = SHAPES[shape][0]
    _both(A, shape, consumed=_first_row_frame(d) - 4 - phase, seed=phase, what=f"phase {phase}")


@pytest.mark.parametrize("shape", ["d104-kaiser-sign+", "d104-kaiser-sign-", "d40-ks3"])
def test_full_scale_alternating_capture(A, shape):
    """+-32767 alternating from value to value: the largest sums the int32 bound of the plan allows."""
    out = _both(A, shape, data=lambda fmt, n: np.where(np.arange(2 * n) & 1, -32767, 32767), what="+-32767")
    assert bool(out.isfinite().all())


@pytest.mark.parametrize("shape", ["d104-kaiser-sign+", "d100-ks7"])
def test_all_zero_capture(A, shape):
    _both(A, shape, data=lambda fmt, n: np.zeros(2 * n, dtype=np.int64), what="zeros")


def test_rotated_lane_with_output_rotation(A):
    """The emission is untouched: a lane that conjugates, rotates and scales by j gives the same bits either way."""
    _both(A, "d104-kaiser-sign-", rotate=True, what="rotating lane")


def test_filter_without_a_run_takes_todays_kernel(A):
    """Random full-scale taps: rot = 0, the launch is today's; and the package's own launcher sends no rot for it."""
    from test_gpu_mfma_exact import make_plan

    d = 104
    mp = make_plan(64 * d - d // 3 - 1, d, FMT, True, seed=3)
    assert mp.groups[0].rot == 0 and mp.groups[0].afrag_rot is None
    raw, x, n_frames, consumed = setup_capture(FMT, d, 1, 0, _ks(d), 0, 0, M_FIRST, N_OUT, OPB, seed=5)
    ln = Lane(mp, 0)
    launch("multi", FMT, d, 0, _ks(d), OPB, [ln], x, n_frames, consumed, M_FIRST, N_OUT)
    assert _N().lib().iqa_mfma_ring_last_kernel() == PLAIN
    assert_exact(ln.out, model_lane_out(ln, 0, raw, d, consumed, M_FIRST, N_OUT), "rot 0")


def test_rot_is_refused_where_no_kernel_takes_it(A):
    """Two lanes, a rot that is no multiple of 4, a decimation of the 32x32x32 kernels: IQA_EINVAL, nothing launched."""
    mp = _plan("d104-kaiser-sign+")
    raw, x, n_frames, consumed = setup_capture(FMT, 104, 1, 0, 7, 0, 0, M_FIRST, N_OUT, OPB, seed=9)
    with pytest.raises(Exception, match="rotated tap fragments"):
        launch("multi", FMT, 104, 0, 7, OPB, [RotLane(mp, 0), Lane(mp, 0)], x, n_frames, consumed, M_FIRST, N_OUT)

    class OddRot(RotLane):
        def fill(self, *a):
            e = super().fill(*a)
            e.reserved = (e.reserved & 255) | (13 << 8)
            return e

    with pytest.raises(Exception, match="rotated tap fragments"):
        launch("multi", FMT, 104, 0, 7, OPB, [OddRot(mp, 0)], x, n_frames, consumed, M_FIRST, N_OUT)
    assert _N().lib().iqa_mfma_ring_zero_rows(0, 208, 0, 13, 1) == 0 and _N().lib().iqa_mfma_ring_zero_rows(0, 104, 0, 7, 0) == 0


def test_channelizer_sends_the_rotated_fragments(A):
    """The package's own path at the headline's shape: Channelizer with and without ``use_zero_rows``, same z bit for bit,
    and the kernel each launch took."""
    import torch

    from iq_to_audio_amd import channelizer as C

    P = _P()
    fs, d = 10e6, 104
    taps = P.design_channel_filter(fs, 12_500.0, d)
    from iq_to_audio_amd import _dev as D

    rng = np.random.default_rng(11)
    n, m_first, n_out = 1 << 20, 64 + 1000, 4096 + 37
    x = D.to_device(rng.integers(-20000, 20000, 2 * n).astype(np.int16), "int16")
    outs, names = [], []
    for use in (True, False):
        C._ChannelKernel.use_zero_rows = use
        C._KERNEL_CACHE.clear()
        try:
            ch = C.Channelizer(taps, sample_rate=fs, freq_offset=25e3, mix_sign=1, decimation=d, fmt=FMT)
            out = torch.full((n_out,), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda")
            # (the interior launch by itself, on the calling thread: the thread whose last kernel the library reports)
            assert ch._kernel.run_interior_only(x, n, m_first, n_out, out)
            names.append(_N().lib().iqa_mfma_ring_last_kernel())
            outs.append(out)
        finally:
            C._ChannelKernel.use_zero_rows = True
            C._KERNEL_CACHE.clear()
    assert names == [ZEDGE, PLAIN]
    assert bool(outs[0].isfinite().all()) and torch.equal(outs[0], outs[1])
