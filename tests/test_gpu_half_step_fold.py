"""The folded odd last k step of the half-step ring kernels (k_channelize_mfma_s16_ring_multi_half<KS>, KS odd:
ring_main_h16 in csrc/channelize_ring.hip) against the exact integer model (oracle/mfma_model.py), ``torch.equal``.

The odd step's twelve products of 16 values (tap pieces q1, q2 of tap-row half 0 / 1 against the byte planes hi, lo of
data-row half 0 / 1) run as seven v_mfma_i32_16x16x32_i8 whose K halves hold two products of one accumulator each.  A
tap or data operand gathered from the wrong piece, plane, row half or K half leaves every 64-value chunk right, so the
lanes here isolate the odd step: full-scale taps that are non-zero ONLY in the last k step's values --

  * all pieces (q1 and q2: every one of the seven instructions contributes),
  * high tap bytes only (q2 = 0: the q1 halves of every operand, S1 and the q1 * lo part of S2),
  * low tap bytes only (q1 = 0: the q2 halves, the q2 * hi part of S2),

and one lane of 64 full random tap rows, rotated, conjugated and scaled, in the same launch.  Row shapes: D = 8 (KS 1: the
odd step is the only step, every accumulator's first use must clear it), D = 36 and 100 (KS 3, 7: the last step holds 8
values, values 8..15 are the next row's data and must meet zero taps), D = 40 and 104 (KS 3, 7: 16 values).  Three ranges
of 256 outputs with a ragged last one, a mid-capture block, random values behind the readable bound.

The helpers are those of tests/test_gpu_mfma_exact.py.
"""
from __future__ import annotations

import dataclasses

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


def _last_step_plan(L: int, d: int, seed: int):
    """A plan of random full-scale complex taps that are zero outside the row's last k step (frames rho >= 16 (KS - 1) of a
    data row: tap k sits at rho = D - 1 - k mod D)."""
    from iq_to_audio_amd import dsp_plan as P

    ks = -(-2 * d // 32)
    rng = np.random.default_rng(seed)
    g = (rng.uniform(-1.0, 1.0, L) + 1j * rng.uniform(-1.0, 1.0, L)) * P.INGEST_SCALE["s16"]
    g[(d - 1 - np.arange(L) % d) < 16 * (ks - 1)] = 0.0
    plan = P.ChannelPlan(fmt="s16", ntaps=L, decimation=d, taps_window=None, conj_sum=0, rotate=0, rot_step=0, rot_base=0,
                         out_scale=1.0 + 0j, taps_natural=g)
    mp = P.plan_mfma(plan, acc32=True)
    mp._acc32 = True
    tq = mp.groups[0].tq
    assert not np.any(tq[:, : 32 * (ks - 1)]) and not np.any(tq[:, 2 * d :])
    assert np.any(tq[:64, 32 * (ks - 1) : 2 * d]) and np.any(tq[64:, 32 * (ks - 1) : 2 * d])
    return mp


def _with_taps(mp, tq: np.ndarray, L: int, d: int):
    """``mp`` with the taps of its one group replaced by ``tq`` (a subset of their bytes: the int32 bound still holds):
    fragments in the planner's layout, the low-byte bias of the pass recomputed.  Never flagged high-byte-only, so the
    launch stays on the half-step kernel."""
    from iq_to_audio_amd import dsp_plan as P

    (grp,), (ps,) = mp.groups, mp.passes
    _, _, _, flat = P._mfma_layout(L, d, 0)
    q1, q2 = M.split_taps(tq)
    frag = np.empty_like(grp.afrag)
    frag[:, :, 0] = q1.reshape(-1)[flat]
    frag[:, :, 1] = q2.reshape(-1)[flat]
    tq = np.asarray(tq, dtype=grp.tq.dtype)
    out = dataclasses.replace(mp, groups=[dataclasses.replace(grp, afrag=frag, tq=tq, high_only=False)],
                              passes=[dataclasses.replace(ps, c_re=128.0 * float(tq[:64].sum(dtype=np.int64)),
                                                          c_im=128.0 * float(tq[64:].sum(dtype=np.int64)))])
    out._acc32 = True
    return out


@pytest.mark.parametrize("d", [8, 36, 40, 100, 104])
def test_odd_last_step_isolated(A, d):
    ks = -(-2 * d // 32)
    assert ks & 1 and 0 < (2 * d) % 32 <= 16
    name = X.expected_kernel("multi", "s16", d, 0, ks, False, False)
    assert name == f"k_channelize_mfma_s16_ring_multi_half<{ks}>", name
    _check_abi_selects(A, "multi", "s16", d, 0, ks, False, name)
    L = 64 * d - d // 3 - 1  # 64 tap rows, not a multiple of D
    both = _last_step_plan(L, d, 9000 + d)
    # the planner's own fragments and bias are what _with_taps rebuilds
    same = _with_taps(both, both.groups[0].tq, L, d)
    assert np.array_equal(same.groups[0].afrag, both.groups[0].afrag)
    assert (same.passes[0].c_re, same.passes[0].c_im) == (both.passes[0].c_re, both.passes[0].c_im)
    q1, q2 = M.split_taps(both.groups[0].tq)
    assert np.any(q1) and np.any(q2)
    high = _with_taps(both, 256 * q1, L, d)
    low = _with_taps(both, q2, L, d)
    full = make_plan(L, d, "s16", True, seed=9100 + d)
    step, base = _rot(np.random.default_rng(9200 + d))
    lanes = [Lane(both, 0), Lane(high, 0), Lane(low, 0),
             Lane(full, 0, rotate=1, conj=1, scale=1j, rot_step=step, rot_base=base)]
    opb, n_out, m_first = 256, 2 * 256 + 37, 64 + 500 + d
    raw, x, n_frames, consumed = setup_capture("s16", d, 1, 0, ks, 0, 0, m_first, n_out, opb, seed=9300 + d)
    assert consumed > 0  # a mid-capture block
    launch("multi", "s16", d, 0, ks, opb, lanes, x, n_frames, consumed, m_first, n_out)
    for ln, what in zip(lanes, ["all pieces", "high tap bytes", "low tap bytes", "64 rows, rotated"]):
        check_lane(ln, 0, raw, d, consumed, m_first, n_out, f"d={d} {what}")
