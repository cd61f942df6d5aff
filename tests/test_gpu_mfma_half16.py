"""The 16x16x64 tile body of the half-step ring kernels (k_channelize_mfma_s16_ring_multi_half<KS>, ring_main_h16 in
csrc/channelize_ring.hip) against the exact integer model (oracle/mfma_model.py), ``torch.equal``, at the smallest shapes
where this body can go wrong -- one axis at a time around D = 104, 64 tap rows, a mid-capture block:

  * row shapes: D = 4 (the row is only a remainder: one 16x16x32), 8, 20 (first even KS, 8 values in the last step),
    100 and 104 (KS = 7: 8 and 16 values), 116 and 120 (KS = 8);
  * output counts 1, 31, 33 (both tile parities), 63, 64, 65 (an emission-group edge) in one range; nine ranges (not a
    multiple of 8) with a ragged last one;
  * 64 full-scale random tap rows, 17 (the second 16-row half of a tile nearly empty), a single tap row;
  * a sign-matched capture at D = 104 that drives one output per component to the int32 bound: the two off-diagonal
    16x16 blocks of a tile share one accumulator, whose partial sums must stay inside int32 as the planner promises.

The helpers are those of tests/test_gpu_mfma_exact.py, whose sweep already runs every KS of this family once.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import mfma_dispatch as X
from oracle import mfma_model as M
from test_gpu_mfma_exact import Lane, _check_abi_selects, _rot, check_lane, launch, make_plan, setup_capture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _half_kernel(A, d):
    ks = -(-2 * d // 32)
    name = X.expected_kernel("multi", "s16", d, 0, ks, False, False)
    assert name == f"k_channelize_mfma_s16_ring_multi_half<{ks}>", name
    _check_abi_selects(A, "multi", "s16", d, 0, ks, False, name)
    return ks


def _run(A, d, L, opb, n_out, m_first, seed, what):
    """Two lanes of one launch -- an exact one and a rotated, conjugated, scaled one -- against the model."""
    ks = _half_kernel(A, d)
    mp = make_plan(L, d, "s16", True, seed=seed)
    step, base = _rot(np.random.default_rng(seed))
    lanes = [Lane(mp, 0), Lane(mp, 0, rotate=1, conj=1, scale=1j, rot_step=step, rot_base=base)]
    raw, x, n_frames, consumed = setup_capture("s16", d, 1, 0, ks, 0, 0, m_first, n_out, opb, seed=seed + 1)
    assert consumed > 0  # a mid-capture block
    launch("multi", "s16", d, 0, ks, opb, lanes, x, n_frames, consumed, m_first, n_out)
    for i, ln in enumerate(lanes):
        check_lane(ln, 0, raw, d, consumed, m_first, n_out, f"{what} lane {i}")


@pytest.mark.parametrize("d", [4, 8, 20, 100, 104, 116, 120])
def test_row_shapes(A, d):
    """64 full-scale tap rows (L no multiple of D), three ranges with a ragged last one."""
    _run(A, d, 64 * d - d // 3 - 1, 128, 2 * 128 + 37, 64 + 500 + d, 7000 + d, f"d={d}")


@pytest.mark.parametrize("n_out", [1, 31, 33, 63, 64, 65])
def test_output_counts_in_one_range(A, n_out):
    _run(A, 104, 64 * 104 - 35, 256, n_out, 64 + 777, 7200 + n_out, f"n_out={n_out}")


def test_nine_ranges_mid_capture(A):
    """Nine ranges: two groups of workgroups, the second with one range; the last range holds 17 outputs."""
    _run(A, 104, 64 * 104 - 35, 64, 8 * 64 + 17, 64 + 12345, 7300, "nine ranges")


@pytest.mark.parametrize("rows", [17, 1])
def test_few_tap_rows(A, rows):
    """17 tap rows: the second 16-row half of the first row tile holds one row, the other tiles none; one row: L <= D."""
    d = 104
    L = rows * d - 67
    mp = make_plan(L, d, "s16", True, seed=7400 + rows)
    tq = mp.groups[0].tq
    assert np.any(tq[rows - 1]) and np.any(tq[64 + rows - 1]) and not np.any(tq[rows:64]) and not np.any(tq[64 + rows:])
    _run(A, d, L, 128, 2 * 128 + 37, 64 + 333, 7400 + rows, f"{rows} tap rows")


def test_sign_matched_capture_reaches_the_int32_bound(A):
    """32767 sign(tap) over one output's 64 data rows, per component (6401 full-scale taps at D = 104): the one-int32 sum
    256 S1 + S2 reaches >= 90 % of 2^31, every accumulator of the tile body -- the shared one of the off-diagonal blocks
    included -- holds a partial sum of it, and the kernel equals the model: nothing wrapped."""
    from iq_to_audio_amd import _dev as D

    d, ks = 104, _half_kernel(A, 104)
    mp = make_plan(6401, d, "s16", True, seed=6401)
    opb, n_out, m_first = 128, 2 * 128 + 9, 64 + 40
    raw, _, n_frames, consumed = setup_capture("s16", d, 1, 0, ks, 0, 0, m_first, n_out, opb, seed=7500)
    raw = raw.copy()
    t = mp.groups[0].tq
    targets = {0: m_first + 50, 1: m_first + 200}  # component -> output; windows of 64 rows that do not overlap
    for comp, m in targets.items():
        for qq in range(1, 65):
            at = 2 * ((m - qq) * d + 1 - consumed)
            row = t[comp * 64 + qq - 1, : 2 * d]
            raw[at : at + 2 * d] = np.where(row > 0, 32767, np.where(row < 0, -32767, 0)).astype(np.int16)
    x = D.to_device(raw, "int16")
    s1, s2 = M.pass_sums(t, raw, "s16", d, 0, 0, ks, consumed, m_first, n_out)
    v64, v32 = M.ring_value(s1, s2, False), M.ring_value(s1, s2, True)
    assert np.array_equal(v64, v32)
    for comp, m in targets.items():
        assert abs(int(v64[m - m_first, comp])) >= 0.9 * 2**31, (comp, int(v64[m - m_first, comp]))
    lanes = [Lane(mp, 0), Lane(mp, 0, finalize=0, raw_partials=1)]
    launch("multi", "s16", d, 0, ks, opb, lanes, x, n_frames, consumed, m_first, n_out)
    for i, ln in enumerate(lanes):
        check_lane(ln, 0, raw, d, consumed, m_first, n_out, f"sign-matched lane {i}")
