"""The rotated tap fragments of dsp_plan.plan_mfma(acc32=True): rows whose high tap byte is zero, and the rotation that puts
16 of them into slots 0..15 of either component.  Host only.

The first and last tap rows of a Kaiser design are tiny; with T = 256 q1 + q2 a row whose |T| stays below 128 has q1 = 0.
Figures of the benchmark's plans (one NFM channel of 12.5 kHz at +25 kHz, int16 capture):
  config 1   (2.5 MS/s, D = 26, 1601 taps):   26 of 128 rows, cyclic run of 12 per component          -> rot 0
  config 2   (10 MS/s, D = 104, 6401 taps):   44 of 128 rows, rows 52..63 and 0..9 of either component -> rot 12
  config 4's unit (20 MS/s, D = 208, 12 801 taps): 52 of 128 rows, rows 51..63 and 0..10              -> rot 13
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

from iq_to_audio_amd import dsp_plan as P

BENCH = {  # name -> (sample rate, zero-q1 rows of 128, (first row, length) of a component's cyclic run, rot)
    "config1": (2.5e6, 26, (57, 12), 0),
    "config2": (10e6, 44, (52, 22), 12),
    "config4-unit": (20e6, 52, (51, 24), 13),
}


def _bench_plan(fs, sign=1):
    d, _ = P.choose_decimation(fs, 96_000.0)
    taps = P.design_channel_filter(fs, 12_500.0, d)
    plan = P.plan_channel(taps, sample_rate=fs, freq_offset=25e3, mix_sign=sign, decimation=d, fmt="s16", iq_order="iq",
                          padded_len=-(-len(taps) // 256) * 256)
    return plan, P.plan_mfma(plan, acc32=True)


def _bytes(tq):
    q2 = ((tq + 128) & 255) - 128
    return (tq - q2) >> 8, q2


def _rows_of(frag):
    """[128, 32 ksteps] of either piece of a fragment array, undoing the lane order (lane l: row l & 31, values 16 (l >> 5) + j)."""
    ks = frag.shape[0]
    out = np.zeros((2, 128, 32 * ks), dtype=np.int64)
    for pc in range(2):
        f = frag[:, :, pc].reshape(ks, 4, 2, 32, 16)  # [ks, rt, half, row, j]
        out[pc] = f.transpose(1, 3, 0, 2, 4).reshape(128, 32 * ks)
    return out


@pytest.mark.parametrize("name", list(BENCH))
@pytest.mark.parametrize("sign", [1, -1])
def test_benchmark_plans(name, sign):
    fs, zero_rows, run, rot = BENCH[name]
    plan, mp = _bench_plan(fs, sign)
    g = mp.groups[0]
    q1, q2 = _bytes(g.tq)
    assert int((~np.any(q1, axis=1)).sum()) == zero_rows
    assert P.zero_high_runs(q1) == [run, run]
    assert g.rot == rot == P.zero_high_rotation(q1)
    if rot == 0:
        assert g.afrag_rot is None
        return
    assert g.afrag_rot.shape == g.afrag.shape and g.afrag_rot.dtype == np.int8
    # a pure row permutation of afrag: slot s of either component holds tap row (s - rot) mod 64
    rows, rows_rot = _rows_of(g.afrag), _rows_of(g.afrag_rot)
    assert np.array_equal(rows[0], q1) and np.array_equal(rows[1], q2)
    for comp in range(2):
        for s in range(64):
            assert np.array_equal(rows_rot[:, comp * 64 + s], rows[:, comp * 64 + (s - rot) % 64]), (comp, s)
    assert sorted(map(bytes, rows_rot.transpose(1, 0, 2).astype(np.int8))) == sorted(map(bytes, rows.transpose(1, 0, 2).astype(np.int8)))
    assert not rows_rot[0, :16].any() and not rows_rot[0, 64:80].any()  # slots 0..15: no high tap byte
    # the fields that were there before are what the planner without the rotation gives
    before = _plan_without_rotation(plan)
    for a, b in zip(mp.groups, before.groups):
        for f in dataclasses.fields(a):
            if f.name in ("rot", "afrag_rot"):
                continue
            va, vb = getattr(a, f.name), getattr(b, f.name)
            assert np.array_equal(va, vb) if isinstance(va, np.ndarray) else va == vb, f.name
    assert [dataclasses.astuple(p) for p in mp.passes] == [dataclasses.astuple(p) for p in before.passes]
    assert mp.floors() == before.floors() and mp.err_norm == before.err_norm and mp.ksteps == before.ksteps


def _plan_without_rotation(plan):
    saved = P.zero_high_rotation
    P.zero_high_rotation = lambda q1: 0
    try:
        return P.plan_mfma(plan, acc32=True)
    finally:
        P.zero_high_rotation = saved


def _plan_of(g, d):
    plan = P.ChannelPlan(fmt="s16", ntaps=len(g), decimation=d, taps_window=None, conj_sum=0, rotate=0, rot_step=0, rot_base=0,
                         out_scale=1.0 + 0j, taps_natural=np.asarray(g) * P.INGEST_SCALE["s16"])
    return plan


def test_short_run_is_not_rotated():
    """Short filters with large taps: every row inside the filter has a high byte, so the run is the rows past its end --
    24 of them are rotated to the front, 15, 14 or none are not."""
    d = 8
    rng = np.random.default_rng(1)
    for rows, rot in ((40, 24), (49, 15), (50, 0), (64, 0)):
        L = rows * d
        mp = P.plan_mfma(_plan_of(rng.uniform(0.5, 1.0, L) * np.exp(2j * np.pi * rng.uniform(0, 1, L)), d), acc32=True)
        run = P.zero_high_runs(_bytes(mp.groups[0].tq)[0])
        assert run == [(rows % 64, 64 - rows)] * 2
        assert mp.groups[0].rot == (rot if 64 - rows >= 16 else 0)
        assert (mp.groups[0].afrag_rot is None) == (mp.groups[0].rot == 0)


def test_components_with_different_runs_are_not_rotated():
    """Both components of a planned filter hold Re and Im of every tap, so their runs differ only in a hand-made matrix:
    zero_high_rotation on q1 itself."""
    q1 = np.zeros((128, 64), dtype=np.int32)
    q1[20:40] = 1
    q1[64 + 20 : 64 + 40] = 1
    assert P.zero_high_runs(q1) == [(40, 44), (40, 44)] and P.zero_high_rotation(q1) == 24
    q1[64 + 41] = 1  # the imaginary component's run now starts a row later and is shorter
    assert P.zero_high_runs(q1) == [(40, 44), (42, 42)] and P.zero_high_rotation(q1) == 0
    q1[:] = 0
    assert P.zero_high_runs(q1) == [(0, 64), (0, 64)] and P.zero_high_rotation(q1) == 0  # (nothing to rotate: rot 0 is "as it is")
    q1[:] = 1
    assert P.zero_high_runs(q1) == [(0, 0), (0, 0)] and P.zero_high_rotation(q1) == 0


def test_residual_and_wide_sum_groups_carry_no_rotation():
    plan, _ = _bench_plan(10e6)
    for kw in (dict(acc32=False), dict(acc32=True, residual=True)):
        assert all(g.rot == 0 and g.afrag_rot is None for g in P.plan_mfma(plan, **kw).groups)
