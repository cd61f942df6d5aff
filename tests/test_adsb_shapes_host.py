"""The crafted inputs of tests/test_gpu_adsb_shapes.py through the oracle alone (tests/adsb_model.py): the tables' own
preconditions, the ties of sums without a tie of samples, at least 257 passing positions in a tile, the kept frames behind
every equality, and the GPU file's own comparisons run against numpy stand-ins of the entry points -- whole, and broken one
way at a time, which shows which comparison notices which break.  No GPU needed."""
from __future__ import annotations

import adsb_model as M
import numpy as np
import pytest

import iq_to_audio_amd.dsp_plan as P


def search_standin(**breaks):
    def call(*args):
        return M.entry_search(*args, **breaks)

    return call


def fails(case, **breaks) -> bool:
    try:
        M.check_search(case, search_standin(**breaks))
    except AssertionError:
        return True
    return False


CASES = M.search_cases()


# ---- the oracle's own facts -----------------------------------------------------------------------------------------------


def test_the_limits_and_the_tables():
    assert (M.MAX_H, M.MAX_SPAN, M.CHIPS, M.TILE) == (P.ADSB_MAX_SPS // 2, 2400, P.ADSB_CHIPS, 2048)
    T = M.tables()
    assert all(M.table_ok(t) for t in T.values())
    plans = [(pl.h, pl.span, pl.offsets.tolist()) for pl in (P.plan_adsb(fs) for fs in np.arange(2.0e6, 20.0e6 + 1, 0.1e6))]
    for name in ("wide", "slack", "equal at a 0 bit", "equal at a 1 bit", "equal at the preamble"):
        assert (T[name]["h"], T[name]["span"], T[name]["o"].tolist()) not in plans, name  # no plan's
    pl = P.plan_adsb(6.4e6)  # "h 3" is a plan's after all: 6.4 MHz, a rate class (h = 3, steps of 3 and 4) no other test runs
    assert (T["h 3"]["h"], T["h 3"]["span"], T["h 3"]["o"].tolist()) == (pl.h, pl.span, pl.offsets.tolist()) and 6.4e6 not in M.RATES
    for name, fs in (("2 MHz", 2e6), ("4 MHz", 4e6), ("20 MHz", 20e6)):
        pl = P.plan_adsb(fs)
        assert (T[name]["h"], T[name]["span"], T[name]["o"].tolist()) == (pl.h, pl.span, pl.offsets.tolist())
    assert (T["wide"]["span"], int(T["wide"]["o"][-1]), T["wide"]["h"]) == (2400, 2390, 1)  # the LDS size the static_assert is written for
    assert T["slack"]["span"] - int(T["slack"]["o"][-1]) - T["slack"]["h"] == 37
    assert (T["h 3"]["h"], int(T["h 3"]["o"][-1]), int(np.diff(T["h 3"]["o"]).min())) == (3, 765, 3)
    assert int((np.diff(T["equal at a 0 bit"]["o"]) == 0).sum()) == 1 and T["equal at the preamble"]["o"][:2].tolist() == [0, 0]
    assert {c["offsets"][0] for c in CASES} == {0, 1, 2, 3} == {c["offsets"][1] for c in CASES} and len({c["offsets"] for c in CASES}) == 16


def test_sums_tie_where_no_sample_does():
    for h in (2, 10):
        a, b = M.chip_values(h, 39_000 * h, 0), M.chip_values(h, 39_000 * h, 1)
        assert a.sum() == b.sum() and len(set(a.tolist()) | set(b.tolist())) == 2 * h
        cases = M.strict_cases(h)
        assert len(cases) == 2 * 13 + 2 * (h == 10) and sum(1 for c in cases if c["misses"]) == 13 + (h == 10)
        assert all(c["keep"] for c in cases if c["passes"])


def test_more_than_256_positions_of_a_tile_pass():
    q = M.period7_plane(3 * M.TILE + 239)
    got = M.search(q, M.tables()["2 MHz"])
    assert got["flags"][:14].tolist() == [1, 0, 0, 0, 0, 0, 0] * 2 and int(got["flags"][: M.TILE].sum()) == 293 and got["records"] == []
    crowded = M.crowded_cases()
    counts = [int(M.search(c["q"], c["table"])["flags"][: M.TILE].sum()) for c in crowded]
    assert counts == [293, 258, 258, 291, 272], counts
    # the frames across the tile edge are the last of tile 0's list: pass 2 reaches them in its second round
    for c in crowded[3:]:
        flags = M.search(c["q"], c["table"])["flags"][: M.TILE]
        assert int(flags[: c["keep"][-1][0]].sum()) >= 256


# ---- the GPU file's comparisons on the stand-ins --------------------------------------------------------------------------


def test_search_cases_on_the_standin():
    assert len(CASES) == 83
    for case in CASES:
        M.check_search(case, search_standin())
    assert sum(1 for c in CASES if not c["flags"]) == 2 and sum(1 for c in CASES if c["capacity"] == 0) == 2


def test_which_comparison_notices_which_break():
    # pass 2 limited to one round: the two planes whose frame lies behind 256 passing positions of its tile
    assert [c["name"] for c in CASES if fails(c, one_round=True)] == ["period 7 with IDENT across the edge at 2040",
                                                                      "period 7 with DF11 at 1900, POS_EVEN across the edge at 2044"]
    # the 112-bit register used for short frames: a DF11 with anything but ties behind it is lost, the DF11 whose 112 bits pass is
    # kept; a DF11 followed by a flat plane reads 56 zero bits behind it, which leave a zero register zero
    assert [c["name"] for c in CASES if fails(c, reg_for_short=True)] == ["period 7 with DF11 at 1900, POS_EVEN across the edge at 2044",
                                                                         "a DF11 whose 56 bits fail and whose 112 would pass", "a valid DF11 is kept"]
    # 6 C_4 <= P: the two planes where 6 C_4 equals P, at h = 2 and 10 and at full scale
    assert [c["name"] for c in CASES if fails(c, le_rule=4)] == ["h 2: 6 C4 against P, equal", "h 10: 6 C4 against P, equal",
                                                                  "h 10 at full scale: 6 C4 against P = 2 621 400, equal"]


def test_quantise_cases_on_the_standin():
    cases = M.quantise_cases()
    assert [c["n"] for c in cases] == list(M.QUANTISE_LENGTHS) and all(o % 2 == 1 for c in cases for o in c["offsets"])
    assert len(M.QUANTISE_WANT) == M.QUANTISE_VALUES.size == 40
    for case in cases:
        M.check_quantise(case, M.entry_quantise)


def test_the_refusal_tables_are_the_entries():
    q, o32, u8, i64 = np.zeros(4096, np.uint16), np.arange(240, dtype=np.int32), np.zeros(4096, np.uint8), np.zeros(64, np.int64)
    for what, n, o_host, h, span, capacity, has_q, has_o, has_list, has_slots, has_counts, message in M.search_refusals():
        counts = np.array([99, 99], dtype=np.int64)
        with pytest.raises(ValueError, match=message):
            M.entry_search(q if has_q else None, 0, n, o32 if has_o else None, o_host, h, span, u8.copy(), 0, i64.copy() if has_list else None,
                           u8.copy() if has_slots else None, capacity, counts if has_counts else None)
        assert counts.tolist() == [99, 99], what  # a refused call clears nothing
    for what, n, has_e, has_q, message in M.quantise_refusals():
        with pytest.raises(ValueError, match=message):
            M.entry_quantise(np.zeros(64, np.float32) if has_e else None, 0, n, q.copy() if has_q else None, 0)
    assert (len(M.search_refusals()), len(M.quantise_refusals())) == (16, 4)
