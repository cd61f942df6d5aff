"""The resampler model (tests/resampler_model.py) before it judges a kernel (tests/test_gpu_resampler_shapes.py): its
direct float64 sum against the oracle's upfirdn evaluation, the path every GPU shape is meant to reach against the
restated launch arithmetic, and the near-midpoint cap for every stream the GPU tests use.  No GPU needed."""
from __future__ import annotations

import numpy as np
import pytest
import resampler_model as M

from oracle import cpu_ref as O


@pytest.mark.parametrize("fs,n", [(96_000.0, 200_003), (192_000.0, 400_003), (288_000.0, 30_011), (44_100.0, 30_011), (M.RATE_C2, 50_000)])
def test_the_direct_sum_and_upfirdn_round_to_the_same_float32(fs, n):
    """Two independent float64 evaluations of the specification: the gather of y64 and scipy's polyphase upfirdn."""
    x, y, a, row = M.reference(fs, n)
    want = O.resample_48k(x, fs)
    assert y.size == want.size == M.n_out_of(fs, n)
    assert np.array_equal(M._rounded(y).view(np.uint32), want.view(np.uint32))
    yu, au, _ = M.y64_upfirdn(x, fs)
    assert np.all(np.abs(yu - y) <= M.bound(a, row)) and np.allclose(au, a, rtol=1e-12, atol=0.0)
    # a later stretch is the slice
    ys, as_, _ = M.y64(x, fs, j0=1_003, n_out=501)
    assert np.array_equal(ys, y[1_003:1_504]) and np.array_equal(as_, a[1_003:1_504])


def test_the_model_table_is_the_plan_the_kernel_reads():
    from iq_to_audio_amd import dsp_plan as P

    for fs in (M.RATE_C2, 99_000.0, 24_000.0, 288_000.0):
        plan = P.plan_resampler(fs)
        up, down, t_half, row = M.geometry(fs)
        assert (plan.up, plan.down, plan.half_taps) == (up, down, t_half) and plan.table.shape == (up, row)
        assert np.array_equal(plan.table, M._table(up, down)[1])


def test_check_passes_the_rounding_and_fails_its_neighbours():
    x, y, a, row = M.reference(96_000.0, 200_003)
    want = M._rounded(y)
    assert M.check(want, y, a, row) == M.midpoint_count(y, a, row)
    below, above = M.near_midpoint(y, a, row)
    j = int(np.argmin(below | above))  # an output away from every midpoint
    for wrong in (np.nextafter(want[j], np.float32(np.inf)), np.nextafter(want[j], np.float32(-np.inf)), np.float32(0.0)):
        bad = want.copy()
        bad[j] = wrong
        with pytest.raises(AssertionError):
            M.check(bad, y, a, row)
    # float32 accumulation, and a lost last tap, are far outside it
    with pytest.raises(AssertionError):
        M.check(np.float32(y.astype(np.float32) * np.float32(1 + 2 ** -23)), y, a, row)
    up, down, t_half, _ = M.geometry(96_000.0)
    lost = y - M._table(up, down)[1][0, -1] * np.concatenate([np.zeros(16), x.astype(np.float64)])[0:2 * y.size:2]
    with pytest.raises(AssertionError):
        M.check(lost.astype(np.float32), y, a, row)
    # at a midpoint both neighbours of it pass, the float beyond does not
    f = np.float32(0.3)
    g = np.nextafter(f, np.float32(1))
    mid = np.array([0.5 * (float(f) + float(g))])
    a1 = np.array([1.0])
    assert M.check(np.array([f]), mid, a1, 65) == M.check(np.array([g]), mid, a1, 65) == 1
    with pytest.raises(AssertionError):
        M.check(np.array([np.nextafter(g, np.float32(1))]), mid, a1, 65)


LONG_WAVE_PATHS = {  # (fs, n_in): (build, steps per wave, steps of the last part, groups, split)
    (96_000.0, 200_003): (17, 13, 6, 1, 8192),
    (24_000.0, 110_001): (17, 14, 3, 1, 8192),
    (120_000.0, 520_003): (24, 13, 1, 1, 8192),
    (144_000.0, 300_001): (32, 13, 5, 1, 8192),
    (192_000.0, 400_003): (48, 13, 5, 1, 8192),
    (240_000.0, 500_001): (48, 13, 5, 1, 8192),
    (M.RATE_C2, 2_950_003): (17, 11, 7, 1500, 6),
}


def test_long_wave_shapes_reach_their_paths():
    assert list(LONG_WAVE_PATHS) == M.LONG_WAVES
    rows = {192_000.0: 129, 240_000.0: 161}
    for (fs, n), (ni, steps, last, groups, split) in LONG_WAVE_PATHS.items():
        p = M.paths(fs, n)
        assert p["kernel"] == "staged", (fs, p)
        assert (p["NI"], p["g_per"], p["last_steps"], p["groups"], p["split"]) == (ni, steps, last, groups, split), (fs, p)
        assert p["unstaged_groups"] == 0 and steps > M.RS_RING and steps % M.RS_GROUP != 0
        assert fs not in rows or p["row"] == rows[fs]
        # the split is at its cap: these are the smallest streams whose waves run this many steps
        assert split == -(-M.RS_TARGET_WAVES // groups)
    assert M.paths(24_000.0, 110_001)["up"] > M.paths(24_000.0, 110_001)["down"]
    assert {p[0] for p in LONG_WAVE_PATHS.values()} == set(M.RS_BUILDS)


def test_class_limit_shapes_reach_their_paths():
    want = {99_000.0: (67, 17), 102_000.0: (69, 24), 141_000.0: (95, 24), 189_000.0: (127, 32), 285_000.0: (191, 48), 288_000.0: (193, None)}
    assert list(want) == M.CLASS_LIMITS
    for fs, (row, ni) in want.items():
        p = M.paths(fs, 30_011)
        assert p["row"] == row
        if ni is None:
            assert p["kernel"] == "long" and row == M.RS_LONG_ROW + 1
        else:
            assert p["kernel"] == "staged" and p["NI"] == ni
            assert -(-row // 4) == ni or row == 69  # the last row of its build; 69 is the first of the next
            assert (4 * ni - row) in (1, 27)  # the last row of a build leaves one lane's last tap masked
    p = M.paths(285_000.0, 30_011)
    assert (p["groups"], p["unstaged_groups"]) == (1, 1) and 15 * p["down"] // p["up"] > p["SPREAD"]
    for fs in (99_000.0, 102_000.0, 141_000.0, 189_000.0):
        assert M.paths(fs, 30_011)["unstaged_groups"] == 0


def test_later_stretch_shapes_reach_their_paths():
    want = [  # (kernel, NI, unstaged groups of all groups, steps per wave)
        ("staged", 24, (1, 3000), 1), ("staged", 32, (0, 1), 5), ("staged", 48, (2, 2), 5), ("staged", 17, (0, 1), 8),
        ("staged", 17, (1, 10), 5), ("staged", 17, (1, 1500), 1), ("staged", 17, (1, 1500), 1), ("long", None, None, None)]
    assert len(want) == len(M.LATER_STRETCHES)
    for (fs, n, j0, cnt), (kernel, ni, unstaged, steps) in zip(M.LATER_STRETCHES, want):
        p = M.paths(fs, n, j0, cnt)
        assert j0 > 0 and j0 + cnt <= M.n_out_of(fs, n) and p["kernel"] == kernel, (fs, p)
        if kernel == "staged":
            assert (p["NI"], (p["unstaged_groups"], p["groups"]), p["g_per"]) == (ni, unstaged, steps), (fs, p)
            # the wrapped wave is unstaged because of j0: the whole stream has none (250 kHz: the ratio alone takes its
            # full wave of 16 residues out of the window, the wrap the wave of the other 8)
            assert M.paths(fs, n)["unstaged_groups"] == (1 if fs == 250_000.0 else 0)
    # every build and the long kernel get a j0 > 0
    seen = {M.paths(fs, n, j0, cnt).get("NI") for fs, n, j0, cnt in M.LATER_STRETCHES}
    assert seen == set(M.RS_BUILDS) | {None}
    # fewer outputs than a wave's residues, across the wrap of (j0 + jj) mod up
    up = M.paths(M.RATE_C2, 50_000)["up"]
    assert 23_999 % up + 15 > up and 15 < 16


def test_stream_end_shapes_reach_their_paths():
    assert [n % 4 for n in M.END_LENGTHS[:3]] == [1, 2, 3] and M.END_LENGTHS[4:] == [1, 2, 3]
    want = {120_000.0: 24, 144_000.0: 32, 192_000.0: 48, 288_000.0: None}
    assert list(want) == M.END_RATES
    for fs, ni in want.items():
        for n in M.END_LENGTHS:
            p = M.paths(fs, n)
            assert p.get("NI") == ni and p["n_out"] >= 1 and (n >= 30_009 or n < p["row"])
            assert p["kernel"] == "long" or p["unstaged_groups"] == 0


def test_midpoint_cap_holds_for_every_gpu_stream():
    """The excepted share is a property of the float64 values alone; here for every stream the GPU tests pin."""
    streams = set(M.LONG_WAVES) | {(fs, 30_011) for fs in M.CLASS_LIMITS} | {(fs, n) for fs, n, _, _ in M.LATER_STRETCHES}
    for fs, n in sorted(streams):
        x, y, a, row = M.reference(fs, n)
        cnt = M.midpoint_count(y, a, row)
        print(f"{fs:.0f} Hz x {n}: {cnt} of {y.size} outputs within the bound of a rounding midpoint")
        assert cnt <= M.midpoint_cap(y.size), (fs, n, cnt)
    for fs in M.END_RATES:
        x_all = M.reference(fs, 30_011)[0]
        for n in M.END_LENGTHS:
            y, a, row = M.y64(x_all[:n], fs)
            assert M.midpoint_count(y, a, row) <= M.midpoint_cap(y.size), (fs, n)
    y, a, row = M.y64(M.saturating_stream(M.SATURATING_N), 96_000.0)
    assert M.midpoint_count(y, a, row) <= M.midpoint_cap(y.size)
