"""The crafted inputs of tests/test_gpu_tones_shapes.py through the oracle alone (tests/tones_model.py): the tile counts per
R, the negative sums that R does not divide, the extreme sums, and the GPU file's own comparisons run against numpy stand-ins
of the entry points -- whole, and broken one way at a time, which shows which comparison notices which break.  No GPU
needed."""
from __future__ import annotations

import numpy as np
import pytest
import tones_model as M

import iq_to_audio_amd.dsp_plan as P

STAGES = ("t", "u", "E_ctcss", "E_dtmf", "P", "ctcss", "dtmf")


def decimate_standin(**breaks):
    def call(theta, n, pos, hist, R, t_buf, u_buf):
        M.entry_decimate(theta, n, pos, hist, R, t_buf, u_buf, **breaks)
        return t_buf, u_buf

    return call


def bank_standin(**breaks):
    def call(u, m, frame, hop, ntones, taps, e_buf, p_buf):
        M.entry_bank(u, m, frame, hop, ntones, taps, e_buf, p_buf, **breaks)
        return e_buf, p_buf

    return call


def failing(cases, check, call) -> list:
    out = []
    for case in cases:
        try:
            check(case, call)
        except (AssertionError, RuntimeError):
            out.append(case)
    return out


# ---- the oracle's own facts -----------------------------------------------------------------------------------------------


def test_the_tiles_are_the_kernels():
    assert M.MAX_R == P.TONES_MAX_R == 64 and M.SHAPE_R == (1, 2, 31, 32, 33, 63, 64)
    assert [M.tile_outputs(R) for R in M.SHAPE_R] == [256, 256, 256, 256, 248, 130, 128]
    assert [M.tile_outputs(R) * R for R in M.SHAPE_R] == [256, 512, 7936, 8192, 8184, 8190, 8192]  # 33 and 63 leave a tile short of TN_SPAN
    assert M.tile_outputs(32) == 256 and M.tile_outputs(33) < 256  # the switch
    for R in M.SHAPE_R:
        cases = M.decimate_cases(R)
        tiles = {c["name"]: M.tiles_of(c) for c in cases}
        assert sorted(set(tiles.values())) == [1, 3, 4], R
        assert all(v == (1 if "one sample" in k else 3 if "last sample" in k else 4) for k, v in tiles.items())
        assert max(c["n"] for c in cases) == 3 * M.tile_outputs(R) * R + R + 1 < 25_000
        assert {c["pos"] % R for c in cases} >= ({0} if R == 1 else {0, R - 1, (7 * R + R // 2) % R}) and M.BIG_POS in {c["pos"] for c in cases}
        assert R == 1 or {c["hist"] for c in cases} == {False, True}


@pytest.mark.parametrize("R", [2, 12, 33, 64])
def test_the_block_oracle_is_the_stream_oracle(R):
    """``decimate_block`` (a window product per output, with a position and a history) against ``decimate`` (two running
    sums over the whole stream): equal at every cut, also where the block completes nothing."""
    t = M.quantise(M.shape_theta(40 * R + 5, R, seed=R))
    whole = M.decimate(t, R)
    u0, sums = M.decimate_block(t, R, 0)
    np.testing.assert_array_equal(u0, whole)
    assert ((sums < 0) & (sums % R != 0)).any() and int(np.abs(sums).max()) == R * R * M.T_PI
    for cut in (1, R - 1, R, R + 1, 7 * R + 3, t.size - 1):
        back = 2 * R - 2
        hist = np.concatenate([np.zeros(back, dtype=np.int32), t[:cut]])[-back:]
        u1, _ = M.decimate_block(t[cut:], R, cut, hist)
        np.testing.assert_array_equal(np.concatenate([M.decimate_block(t[:cut], R, 0)[0], u1]), whole)


# ---- the GPU file's comparisons on the stand-ins --------------------------------------------------------------------------


@pytest.mark.parametrize("R", list(M.SHAPE_R))
def test_decimate_cases_on_the_standin(R):
    stats: dict = {}
    cases = M.decimate_cases(R)
    for case in cases:
        M.check_decimate(case, decimate_standin(), stats)
    assert R == 1 or (stats["no output"] >= 2 and stats["from the history alone"] >= 2 and stats["negative, not divisible"] > 100)
    assert R > 1 or stats["no output"] == 0


def test_a_truncating_quotient_fails_every_multi_tile_case_with_R_above_1():
    for R in M.SHAPE_R:
        cases = M.decimate_cases(R)
        bad = failing(cases, M.check_decimate, decimate_standin(floor=False))
        assert {c["name"] for c in bad} >= {c["name"] for c in cases if c["n"] > 1 and R > 1}, R
        assert R > 1 or not bad  # R = 1: every sum is divisible


def test_a_tile_of_256_outputs_at_every_R():
    """MB fixed at 256 in the launcher: self-consistent wherever the tile still fits (R <= 63: 64 760 bytes), so only
    R = 64 notices, by a refused launch.  MB fixed at 256 inside the kernel alone: every case with R >= 33 fails."""
    for R in M.SHAPE_R:
        cases = M.decimate_cases(R)
        in_launcher = failing(cases, M.check_decimate, decimate_standin(mb_host=256))
        in_kernel = failing(cases, M.check_decimate, decimate_standin(mb_kernel=256))
        assert len(in_launcher) == (len(cases) if R == 64 else 0), R
        assert len(in_kernel) == (len(cases) if R >= 33 else 0), R


@pytest.mark.parametrize("R", [33, M.MAX_R])
def test_block_invariance_on_the_standin(R):
    fs, n, schedules = M.invariance_case(R)
    span = M.tile_outputs(R) * R
    assert P.plan_tones(fs).R == R and n < 240_000
    sizes = [b - a for cuts in schedules for a, b in zip(cuts[:-1], cuts[1:])]
    assert 1 in sizes and 2 * R - 3 in sizes and any(cuts[1] == span + d for cuts in schedules for d in (-1, 0, 1))
    theta = M.shape_stream(fs, n)
    assert np.abs(theta).max() < np.pi
    want = M.oracle(fs=fs, t=M.quantise(theta))

    def decimate(block, pos, hist, R):
        count = (pos + block.size) // R - pos // R
        t, u = np.full(block.size, M.SENT, dtype=np.int32), np.full(count, M.SENT, dtype=np.int32)
        M.entry_decimate(block, block.size, pos, hist, R, t, u)
        return t, u

    runs = []
    for cuts in schedules:
        st = M.run_blocks(theta, R, cuts, decimate)
        runs.append(dict(M.oracle(fs=fs, t=st["t"]), u=st["u"]))  # (the stages behind u from the oracle: the banks have their own test)
        np.testing.assert_array_equal(st["u"], want["u"])
    M.check_invariance(runs, want, STAGES)
    # a history that is dropped at a cut is noticed
    lost = M.run_blocks(theta, R, schedules[2], lambda block, pos, hist, R: decimate(block, pos, None, R))
    assert (lost["u"] != want["u"]).any()


def test_bank_cases_on_the_standin():
    cases = M.bank_cases()
    assert len(cases) == 20
    for fs in M.BANK_RATES:
        pl, mine = P.plan_tones(fs), M.plan(fs)
        assert (pl.R, pl.Nc, pl.Hc, pl.Nd, pl.Hd) == (mine["R"], mine["Nc"], mine["Hc"], mine["Nd"], mine["Hd"])
    assert P.plan_tones(519_999.0).R == 64 and M.plan(15_999.0)["Nc"] == M.MAX_FRAME
    with pytest.raises(ValueError):
        P.plan_tones(520_000.0)
    with pytest.raises(ValueError):
        P.plan_tones(7_999.0)
    for case in cases:
        M.check_bank(case, bank_standin())
    assert len(failing(cases, M.check_bank, bank_standin(shift=False))) == len(cases)  # / 4096 for >> 12


def test_the_refusal_tables_are_the_entries():
    for what, n, pos, R, has_theta, has_t, has_u, message in M.decimate_refusals():
        with pytest.raises(ValueError, match=message):
            M.entry_decimate(np.zeros(64, np.float32) if has_theta else None, n, pos, None, R, np.zeros(64, np.int32) if has_t else None,
                             np.zeros(64, np.int32) if has_u else None)
    for what, m, frame, hop, ntones, has_u, has_taps, has_e, message in M.bank_refusals():
        with pytest.raises(ValueError, match=message):
            M.entry_bank(np.zeros(8, np.int32) if has_u else None, m, frame, hop, ntones, np.zeros(8, np.int16) if has_taps else None,
                         np.zeros(8, np.int64) if has_e else None, None)
    for what, fc, fd, frame, has_ec, has_ed, has_p, has_c, has_d, message in M.decide_refusals():
        with pytest.raises(ValueError, match=message):
            M.entry_decide_checks(fc, fd, frame, *[0 if has else None for has in (has_ec, has_ed, has_p, has_c, has_d)])
    M.entry_decide_checks(2, 2, 160, 0, 0, 0, 0, 0)  # and a call that is in order passes
