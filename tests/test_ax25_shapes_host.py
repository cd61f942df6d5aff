"""The crafted inputs of tests/test_gpu_ax25_shapes.py through the oracle alone (tests/ax25_model.py): every branch the GPU
test means to reach is reached by the oracle, and ``plan_afsk`` is the oracle's plan at every rate used.  No GPU needed."""
from __future__ import annotations

import ax25_model as M
import numpy as np
import pytest

import iq_to_audio_amd.dsp_plan as P

PLAN_RATES = sorted(set(M.EDGE_RATES) | {1200.0 * L for L in M.EDGE_WINDOWS})


@pytest.mark.parametrize("fs", PLAN_RATES)
def test_the_plan_is_the_oracles_at_every_edge_rate(fs):
    plan, pl = P.plan_afsk(fs), M.plan(fs)
    assert (plan.sps, plan.L, plan.step) == (pl["sps"], pl["L"], pl["step"])
    assert plan.taps.dtype == np.int16 and plan.taps.shape == (4, pl["L"])
    want = np.stack([pl["taps"][1200][0], pl["taps"][1200][1], pl["taps"][2200][0], pl["taps"][2200][1]])
    assert np.array_equal(plan.taps, want) and int(np.abs(want).max()) == 256
    n = 40 * pl["L"] + 5
    for p in range(M.PHASES):
        at = M.instants(pl, p, n)
        assert np.array_equal(plan.instant(np.arange(at.size), p), at)
        assert plan.bit_count(p, n) == at.size and plan.bit_count(p, 0) == 0
        assert int(plan.instant(at.size, p)) >= n


def test_the_edge_rates_are_the_edges():
    got = {fs: (M.plan(fs)["L"], M.plan(fs)["step"]) for fs in M.EDGE_RATES}
    assert got == {9_600.0: (8, 1.0), 12_600.0: (10, 21.0 / 16.0), 97_200.0: (81, 10.125), 100_800.0: (84, 10.5)}
    assert M.plan(480_000.0)["step"] == 50.0 and P.AFSK_MAX_SPS == 400
    assert sorted(M.plan(1200.0 * L)["L"] for L in M.EDGE_WINDOWS) == list(M.EDGE_WINDOWS)


@pytest.mark.parametrize("fs", M.EDGE_RATES)
def test_instant_ties_are_where_the_step_puts_them(fs):
    pl = M.plan(fs)
    ties = M.tie_instants(pl, 40 * pl["L"])
    assert bool(ties) == (fs in M.TIE_RATES)
    for i, p in ties[:50]:
        x = (8.0 * i + p) * pl["step"]
        assert np.rint(x) % 2 == 0 and abs(np.rint(x) - x) == 0.5
    if ties:  # half of them round down: floor(x + 0.5) would move those instants
        assert any(np.rint((8.0 * i + p) * pl["step"]) != np.floor((8.0 * i + p) * pl["step"] + 0.5) for i, p in ties)


@pytest.mark.parametrize("fs", M.EDGE_RATES)
def test_the_oracle_decodes_the_edge_streams(fs):
    z = M.edge_stream(fs)
    want = M.oracle(M.theta_of(z), fs)
    assert [M.tnc2(f) for f in want["frames"]] == ["N0CALL-7>APRS,WIDE1-1*,WIDE2-1:!4903.50N/07201.75W-edge rates"]
    assert 12 <= len(want["records"]) <= 15 and want["rejected"] == 0
    assert bool(M.tie_instants(M.plan(fs), z.size)) == (fs in M.TIE_RATES)


def test_crafted_theta_reaches_the_correlators_full_scale():
    pl = M.plan(480_000.0)
    th = M.crafted_theta(400, 2055, seed=1)
    t, E, sign, sums = M.correlate_block(th, M.crafted_history(400, seed=2), pl)
    assert int(np.abs(t).max()) == M.T_PI and M.T_PI * 256 * 400 < 2 ** 31
    for f in (1200, 2200):
        assert max(int(np.abs(x).max()) for x in sums[f]) > M.T_PI * 256 * 400 // 2, f
        assert int(E[f].max()) < 2 ** 59  # 4 E stays inside int64
    assert set(np.unique(sign).tolist()) == {0, 4, 5, 7}  # E1 > 4 E2 implies E1 > E2 implies 4 E1 > E2: all four decisions occur
    for L in M.EDGE_WINDOWS:
        assert M.crafted_history(L, 0).size == L - 1 and M.crafted_theta(L, 7, 0).size == 7


@pytest.mark.parametrize("fs", M.EDGE_RATES + (480_000.0,))
def test_the_bit_plane_ends_on_the_last_sample(fs):
    pl = M.plan(fs)
    plane, n = M.bits_case(pl)
    assert plane.size == n and set(np.unique(plane).tolist()) == set(range(8))
    assert int(M.instants(pl, 3, n)[-1]) == n - 1 and M.instants(pl, 3, n).size == 38
    assert M.instants(pl, 3, n - 1).size == 37
    full, short = M.bits_plane(plane, pl, 38 + 3), M.bits_plane(plane[: n - 1], pl, 38 + 3)
    assert (full[:, 38:] == 0).all() and (short[3::8, 37] == 0).all()
    assert np.array_equal(full[:, :37], short[:, :37]) and 0 < int(full.sum()) < full.size
