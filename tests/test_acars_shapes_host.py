"""The crafted inputs of tests/test_gpu_acars_shapes.py through the oracle alone (tests/acars_model.py): the tap sums, the
2 139 095 040 bound, the quantiser's ties and extreme scales, the tie instants, the kept blocks behind every equality, and
the GPU file's own comparisons run against numpy stand-ins of the entry points -- whole, and broken one way at a time, which
shows which comparison notices which break.  No GPU needed."""
from __future__ import annotations

import acars_model as M
import numpy as np
import pytest

import iq_to_audio_amd.dsp_plan as P


def detect_standin(**breaks):
    def call(*args):
        return M.entry_detect(*args, **breaks)

    return call


def bits_standin(**breaks):
    def call(same, n, W, step, nbits, out):
        return M.entry_bits(same, n, W, step, nbits, out, **breaks)

    return call


def fails(check, *args, **kwargs) -> bool:
    try:
        check(*args, **kwargs)
    except AssertionError:
        return True
    return False


# ---- the oracle's own facts -----------------------------------------------------------------------------------------------


def test_the_limits_are_the_plans():
    assert (M.MAX_DELAY, M.PHASES) == (P.ACARS_MAX_SPS, P.ACARS_PHASES) and M.MAX_WINDOW >= P.plan_acars(2400.0 * 400).W == 533
    plans = {(pl.W, pl.L) for pl in (P.plan_acars(2400.0 * sps) for sps in np.arange(8.0, 400.25, 0.25))}
    assert not plans & set(M.DETECT_SHAPES)  # nine pairs that no plan asks for
    assert [M.round8(W - 1) for W, _ in M.DETECT_SHAPES] == [0, 8, 8, 8, 16, 16, 256, 536, 536]  # H: none, and both sides of a tap group
    assert [M.TILE - M.round8(L) for _, L in M.DETECT_SHAPES] == [2040, 2040, 2032, 2032, 2032, 1648, 2040, 2040, 1648]
    offs = [M.detect_offsets(k) for k in range(56)]
    assert {o["same"] for o in offs} == set(range(8)) and {o["y"] for o in offs} == {0, 1}
    assert all({o[k] for o in offs} == {0, 1, 2, 3} for k in ("e", "q", "I", "Q"))
    assert len({(o["e"] - o["same"]) % 4 for o in offs}) > 1 and len({(o["q"] - o["I"]) % 4 for o in offs}) > 1  # not in step
    assert (M.front_of(np.uint8), M.front_of(np.int32), M.front_of(np.int64)) == (16, 4, 4)


def test_the_mad24_model_is_exact_inside_its_range():
    x = np.array([0, 1, -1, 2 ** 15, 256, -256, 2 ** 23 - 1, -(2 ** 23)])
    assert (M.s24(x) == x).all() and int(M.s24(2 ** 23)) == -(2 ** 23) and int(M.s16(2 ** 15)) == -(2 ** 15)
    assert int(M.wrap32(2 ** 31)) == -(2 ** 31) and int(M.wrap32(M.FULL_SUM)) == M.FULL_SUM == 2_139_095_040
    assert round(100.0 * (1.0 - M.FULL_SUM / 2.0 ** 31), 1) == 0.4  # per cent under 2^31


def test_the_quantiser_cases_are_what_they_say():
    ties, tiny, small, big = M.quantiser_cases()
    q = M.detect_block(ties)["q"]
    assert q[:10].tolist() == [0, 2, 2, 4, 4, 6, 2 ** 15, 2 ** 15 - 1, 2 ** 15, 2 ** 15]  # half-even; 2^15 - 1/2 and either side
    x = ties["e"].astype(np.float64) * 2.0 ** 17
    assert int((x % 1.0 == 0.5).sum()) >= ties["n"] - 4 and {int(v) % 2 for v in np.floor(x[:100])} == {0, 1}
    for case, sh in ((tiny, 163), (small, 140), (big, -113)):
        blk = M.detect_block(case)
        assert blk["sh"] == sh and 2 ** 14 <= blk["q"].max() <= 2 ** 15 and blk["same"].any() and not blk["same"].all()
    assert sorted(set(M.detect_block(tiny)["q"].tolist())) == [0, 2 ** 14]
    q = M.detect_block(small)["q"]
    assert q[:8].tolist() == [0, 2, 6, 2 ** 14, 2 ** 14, 0, 1, 0] and len(set(q.tolist())) > 1000  # k 2^-9 at 1/2, 3/2, 11/2, ..., 255/512, 257/512
    q = M.detect_block(big)["q"]
    assert len(set(q.tolist())) > 1000 and q[3] == 2 ** 15  # the largest float is 2^15 - 2^-9 at sh = -113: the upper end itself


def test_ties_occur_and_round_half_even():
    for step, p, i, at in ((1.5, 1, 0, 2), (1.5, 3, 0, 4), (1.25, 2, 0, 2), (1.25, 6, 0, 8), (1.25, 2, 1, 12)):
        x = (8 * i + p) * step
        assert x % 1.0 == 0.5 and int(np.rint(x)) == at and at % 2 == 0
        assert M.instant_of(1, step, i, p) == at
    _, at, ties = M.bits_block(np.ones(4000, np.uint8), 4000, 16, 1.5, 257)
    assert ties[[1, 3, 5, 7]].all() and not ties[[0, 2, 4, 6]].any()


def test_the_17th_round_reads_one_element():
    assert M.MAX_LENGTHS[-3:] == (M.MAX_GRID * M.MAX_THREADS * 16 - 1, M.MAX_GRID * M.MAX_THREADS * 16, M.MAX_GRID * M.MAX_THREADS * 16 + 1)
    assert M.max_reader(4_194_305, 4_194_304) == (0, 0, 16) and M.max_reader(4_194_304, 4_194_303) == (1023, 255, 15)
    assert M.max_reader(257, 256) == (0, 0, 1)  # one block: its thread 0 goes round twice
    cases = M.max_cases()
    assert {c["n"] for c in cases} == set(M.MAX_LENGTHS) and {c["offset"] for c in cases} == {0, 1, 2, 3}
    assert any(c["n"] == 4_194_305 and c["at"] == 4_194_304 for c in cases) and {c["kind"] for c in cases} == {"denormal", "largest", "smallest"}
    assert sum(1 for c in cases if c["n"] > 4_000_000) == 7


# ---- the GPU file's comparisons on the stand-ins --------------------------------------------------------------------------


@pytest.mark.parametrize("W,L", list(M.DETECT_SHAPES))
def test_detect_cases_on_the_standin(W, L):
    cases = M.detect_cases(W, L)
    assert len(cases) == 57 + 6 * (W == 255) and {c["n"] for c in cases[:56]} == set(M.detect_lengths(L))
    assert {c["offsets"]["same"] for c in cases} == set(range(8)) and {c["outputs"] for c in cases} == set(M.DETECT_OUTPUTS)
    assert {(c["cr"], c["sr"]) for c in cases[:56]} == set(M.DETECT_CRSR) and cases[56]["outputs"] == "" and cases[56]["offsets"]["same"] == 3
    for case in cases:
        M.check_detect(case, detect_standin())
    # the breaks, on the cases of one length and the full-scale ones
    T = M.TILE - M.round8(L)
    for case in [c for c in cases if c["n"] == T + 1 or c["full"]]:
        # the 8-byte store taken whatever the address: every case with same off the boundary, and no other
        assert fails(M.check_detect, case, detect_standin(wide_store_always=True)) == (case["offsets"]["same"] % 8 != 0), case["name"]
        if case["full"]:  # q = 2^15 does not fit 16 bits; y = 2 . 256 . 8 355 840^2 does not fit 32
            assert fails(M.check_detect, case, detect_standin(operands16=True)) and fails(M.check_detect, case, detect_standin(y32=True)), case["name"]


def test_quantiser_cases_on_the_standin():
    for case in M.quantiser_cases():
        M.check_detect(case, detect_standin())


def test_max_cases_on_the_standin():
    for case in M.max_cases():
        if case["n"] < 4_000_000 or case["at"]:
            M.check_max(case, M.entry_max)


def test_bit_cases_on_the_standin():
    stats: dict = {}
    cases = M.bit_cases()
    assert {c["nbits"] for c in cases} == set(M.BIT_COUNTS) and sum(1 for c in cases if c["last"] is None) == 5 and len(cases) == 6 * 13 + 5
    for case in cases:
        M.check_bits(case, M.entry_bits, stats)
    assert stats[1.5] == dict(ties=10252, down=5126) and stats[1.25] == dict(ties=5126, down=2563)
    assert all(stats[s]["ties"] > 1000 and stats[s]["down"] > 1000 for s in (1.5, 1.25))
    broken = {c["step"] for c in cases if fails(M.check_bits, c, bits_standin(floor_half=True))}
    assert broken >= {1.5, 1.25} and not broken & {1.0, 5.0, 50.0}


def test_frame_scenarios_on_the_standin():
    scenarios = M.frame_scenarios()
    assert [sc["name"] for sc in scenarios] == ["counts", "walks 0", "walks 1"]
    assert scenarios[0]["kept"] == [1, 0, 0, 0, 0, 0, 1, 1]
    for sc in scenarios:
        assert sc["planes"].dtype == np.uint8 and sc["planes"].shape[0] == 8 and len(set(sc["count_of"])) >= 3
        for capacity in (16, 1, 0):
            M.check_frames(sc, M.entry_frames, capacity=capacity)
        for g, count in zip(sc["planes"], sc["count_of"]):
            assert M.standin_frames_of(g[:count]) == M.frames_of(g[:count])
    # kept, reached-not-kept and aborted blocks in one call
    kinds = [M.frames_block(sc["planes"], sc["count_of"])[1:] for sc in scenarios[1:]]
    assert all(reached > kept > 0 for kept, reached in kinds), kinds


def test_the_refusal_tables_are_the_entries():
    f32, i16, u8, i64 = np.zeros(64, np.float32), np.zeros(2 * 536 + 8, np.int16), np.zeros(4096, np.uint8), np.zeros(64, np.int64)
    for what, n, sh, W, L, cr, sr, has_e, has_taps, has_same, message in M.detect_refusals():
        with pytest.raises(ValueError, match=message):
            M.entry_detect(f32 if has_e else None, 0, n, sh, W, L, i16 if has_taps else None, cr, sr, dict(same=u8.copy() if has_same else None), dict(same=0))
    for what, n, has_e, has_out, message in M.max_refusals():
        out = np.array([99], dtype=np.uint32)
        with pytest.raises(ValueError, match=message):
            M.entry_max(f32 if has_e else None, 0, n, out if has_out else None, 0)
        assert out.tolist() == [99], what  # a refused call clears nothing
    for what, n, W, step, nbits, has_same, has_out, message in M.bit_refusals():
        with pytest.raises(ValueError, match=message):
            M.entry_bits(u8 if has_same else None, n, W, step, nbits, u8.copy() if has_out else None)
    for what, nbits, count_of, W, step, capacity, has_bits, has_list, has_slots, has_counts, message in M.frame_refusals():
        counts = np.array([99, 99], dtype=np.int64)
        with pytest.raises(ValueError, match=message):
            M.entry_frames(u8 if has_bits else None, nbits, count_of, W, step, capacity, i64.copy() if has_list else None, u8.copy() if has_slots else None,
                           counts if has_counts else None)
        assert counts.tolist() == [99, 99], what
    assert (len(M.detect_refusals()), len(M.max_refusals()), len(M.bit_refusals()), len(M.frame_refusals())) == (13, 4, 11, 14)
