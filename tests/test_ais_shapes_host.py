"""The crafted inputs of tests/test_gpu_ais_shapes.py through the oracle alone (tests/ais_model.py): the full-scale sums, the
tie instants, the kept counts behind every equality, the model's invariance under the affine map, and the GPU file's own
comparisons run against numpy stand-ins of the entry points -- whole, and broken one way at a time, which shows which
comparison notices which break.  No GPU needed."""
from __future__ import annotations

import ais_model as M
import numpy as np
import pytest

import iq_to_audio_amd.dsp_plan as P


def filter_standin(**breaks):
    def call(theta, th_at, n, hist, h_at, W, taps, t_alloc, t_at, s_alloc, s_at):
        M.entry_filter(theta, th_at, n, hist, h_at, W, taps, t_alloc, t_at, s_alloc, s_at, **breaks)
        return t_alloc, s_alloc

    return call


def symbols_standin(S, n, W, step, nsym, v_buf):
    M.entry_symbols(S, n, W, step, nsym, v_buf)
    return v_buf


def frames_standin(**breaks):
    def call(planes, nsym, count_of, W, step, capacity, lst, slots, counts):
        M.entry_frames(planes, nsym, count_of, W, step, capacity, lst, slots, counts, **breaks)
        return lst, slots, counts

    return call


# ---- the oracle's own facts -----------------------------------------------------------------------------------------------


def test_the_limits_are_the_plans():
    assert (M.MAX_TAPS, M.PHASES, int(M.MAX_SPS)) == (3 * P.AIS_MAX_SPS - 1, P.AIS_PHASES, P.AIS_MAX_SPS)
    assert M.T_PI * 256 * M.MAX_TAPS == 984_968_192 < 2 ** 31  # the bound the kernel's static_assert claims
    plan_windows = {3 * L - 1 for L in range(5, 101)}
    assert [W in plan_windows for W in M.FILTER_WINDOWS] == [False, False, False, False, False, True, False, True]  # six that no plan asks for
    assert [(W - 1 + 7) // 8 * 8 for W in M.FILTER_WINDOWS] == [0, 8, 8, 8, 16, 16, 304, 304]  # H: none, and both sides of a tap group
    offs = M.view_offsets()
    assert len(offs) == 8 and all({o[k] for o in offs} == {0, 1, 2, 3} for k in range(1, 4))
    assert {(o[3], o[0] == 0) for o in offs} == {(s, a) for s in range(4) for a in (True, False)}
    assert len({(o[0] - o[3]) % 4 for o in offs}) > 1 and len({(o[1] - o[2]) % 4 for o in offs}) > 1  # not in step


def test_the_mad24_model_is_exact_inside_its_range():
    x = np.array([0, 1, -1, M.T_PI, -M.T_PI, 256, 2 ** 23 - 1, -(2 ** 23)])
    assert (M.s24(x) == x).all() and int(M.s24(2 ** 23)) == -(2 ** 23)
    assert int(M.wrap32(2 ** 31)) == -(2 ** 31) and int(M.wrap32(M.T_PI * 256 * 299)) == M.T_PI * 256 * 299


def test_ties_occur_and_round_half_even():
    for sps, p, i, at in ((10.0, 2, 0, 2), (10.0, 2, 1, 12), (6.0, 2, 0, 2), (6.0, 6, 0, 4), (6.0, 2, 1, 8)):
        x = (8 * i + p) * (sps / 8.0)
        assert x % 1.0 == 0.5 and int(np.rint(x)) == at and at % 2 == 0
        assert M.instant_of(1, sps / 8.0, i, p) == at
    _, at, ties = M.symbols_block(np.arange(4000, dtype=np.int32), 4000, 29, 1.25, 257)
    assert ties[[2, 6]].all() and not ties[[0, 1, 3, 4, 5, 7]].any()  # phases 2 and 6 at sps 10: every instant is a tie
    assert (at[2] == 28 + 10 * np.arange(257) + 2).all() and (at[6] == 28 + 10 * np.arange(257) + 8).all()  # 2.5 -> 2, 7.5 -> 8


def test_the_affine_map_keeps_every_decision():
    assert (M.AFFINE_A, 9000 * M.AFFINE_A + M.AFFINE_B, -7000 * M.AFFINE_A + M.AFFINE_B) == (134_217, 2_147_472_001, 1)
    for name, v, count, kept in M.hand_made_planes():
        if min(v) < -7000 or max(v) > 9000:
            continue
        assert M.frames_of(M.affine(v)[:count]) == M.frames_of(v[:count]), name
        assert len(M.frames_of(v[:count])[0]) == kept


# ---- the GPU file's comparisons on the stand-ins --------------------------------------------------------------------------


@pytest.mark.parametrize("W", list(M.FILTER_WINDOWS))
def test_filter_cases_on_the_standin(W):
    cases = M.filter_cases(W)
    assert len(cases) == 86 and {c["n"] for c in cases} == set(M.FILTER_LENGTHS) == {7, 8, 9, 2056, 4101}
    for case in cases:
        M.check_filter(case, filter_standin())
    # the 16-byte store taken whatever the address: every case with a full run of 8 at an unaligned s_out, and no other
    for case in cases:
        hit = case["offsets"][3] != 0 and case["n"] >= 8
        if hit:
            with pytest.raises(AssertionError):
                M.check_filter(case, filter_standin(wide_store_always=True))
        else:
            M.check_filter(case, filter_standin(wide_store_always=True))


def test_symbol_cases_on_the_standin():
    stats: dict = {}
    cases = M.symbol_cases()
    assert {c["nsym"] for c in cases} == {0, 1, 255, 256, 257} and sum(1 for c in cases if c["n"] == c["W"] - 2) == 4
    for case in cases:
        M.check_symbols(case, symbols_standin, stats)
    assert stats == {"ties": 9097, "ties rounded down": 4550}


@pytest.mark.parametrize("nsym", list(M.FRAME_NSYM))
def test_frame_scenarios_on_the_standin(nsym):
    scenarios = M.frame_scenarios(nsym)
    assert [sc["kept"] for sc in scenarios] == [[1, 1, 0, 0, 0, 0, 0, 1], [1, 1, 1, 0, 0, 0, 1, 0]]
    for sc in scenarios:
        assert len(set(sc["count_of"])) >= 5 and sc["planes"].shape == (8, nsym) and sc["planes"].dtype == np.int32
        for mapped in (False, True):
            M.check_frames(sc, frames_standin(), mapped=mapped)
        # an int32 level sum, and 16 v in int32: the planes as made pass both, which is the gap; under the map both fail
        for breaks in (dict(level32=True), dict(mul32=True)):
            M.check_frames(sc, frames_standin(**breaks), mapped=False)
            with pytest.raises(AssertionError):
                M.check_frames(sc, frames_standin(**breaks), mapped=True)
    cuts = scenarios[0]
    want, kept, closed = M.frames_block(cuts["planes"], cuts["count_of"])
    assert cuts["count_of"] == [nsym, 163, 162, 0, 23, 24, 25, nsym]
    # phase 0: the frame ends with the plane (163 - 32 symbols behind its opener); phase 7: the first position there is
    assert [(p, s) for p, s, _at, _raw in want] == [(0, nsym - 131), (1, 32), (7, 24)] and (kept, closed) == (3, 3)
    walks = scenarios[1]
    assert M.frames_block(walks["planes"], walks["count_of"])[1:] == (4, 5)  # the damaged frame closes and fails its check


def test_a_list_shorter_than_the_kept_frames():
    sc = M.frame_scenarios(256)[0]
    lst, slots, counts = np.full(4 + M.GUARD, M.SENT, dtype=np.int64), np.full(M.SLOT_BYTES + M.GUARD, 0xAA, dtype=np.uint8), np.array([99, 99], dtype=np.int64)
    M.entry_frames(sc["planes"].reshape(-1), 256, sc["count_of"], M.FRAME_W, M.FRAME_STEP, 1, lst, slots, counts)
    assert counts.tolist() == [3, 3] and (lst[4:] == M.SENT).all() and (slots[M.SLOT_BYTES :] == 0xAA).all() and lst[:2].tolist() == [0, 125]


def test_the_refusal_tables_are_the_entries():
    z32, z16, z64 = np.zeros(64, np.int32), np.zeros(64, np.int16), np.zeros(64, np.int64)
    for what, n, W, has_theta, has_taps, has_s, message in M.filter_refusals():
        with pytest.raises(ValueError, match=message):
            M.entry_filter(np.zeros(64, np.float32) if has_theta else None, 0, n, None, 0, W, z16 if has_taps else None, z32.copy(), 0, z32.copy() if has_s else None, 0)
    for what, n, W, step, nsym, has_s, has_v, message in M.symbol_refusals():
        with pytest.raises(ValueError, match=message):
            M.entry_symbols(z32 if has_s else None, n, W, step, nsym, z32.copy() if has_v else None)
    for what, nsym, count_of, W, step, capacity, has_v, has_list, has_slots, has_counts, message in M.frame_refusals():
        counts = np.array([99, 99], dtype=np.int64)
        with pytest.raises(ValueError, match=message):
            M.entry_frames(z32 if has_v else None, nsym, count_of, W, step, capacity, z64.copy() if has_list else None,
                           np.zeros(512, np.uint8) if has_slots else None, counts if has_counts else None)
        assert counts.tolist() == [99, 99], what  # a refused call clears nothing
    for step in (5.0 / 8.0, 12.5):
        assert M.step_ok(step) and P.plan_ais(step * 8.0 * 9600.0).step == step
