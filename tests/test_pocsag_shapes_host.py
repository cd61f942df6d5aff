"""The crafted inputs of tests/test_gpu_pocsag_shapes.py through the oracle alone (tests/pocsag_model.py): every branch the
GPU test means to reach is reached by the oracle, and ``plan_pocsag`` is the oracle's plan at every rate used.  No GPU
needed."""
from __future__ import annotations

from collections import Counter

import numpy as np
import pocsag_model as M
import pytest

import iq_to_audio_amd.dsp_plan as P

BP8 = M.baud_plan(4096.0, 512)  # sps 8: offsets 8 i, h 4
BP384 = M.baud_plan(196_608.0, 512)  # sps 384: the largest window


@pytest.mark.parametrize("fs", list(M.EDGE_RATES))
def test_the_plan_is_the_oracles_at_every_edge_rate(fs):
    skipped, ties = M.EDGE_RATES[fs]
    plan = P.plan_pocsag(fs)
    assert list(plan.skipped) == skipped == [b for b in M.BAUDS if M.baud_plan(fs, b) is None]
    assert [pb.baud for pb in plan.bauds] == [b for b in M.BAUDS if b not in skipped] == list(ties)
    for pb in plan.bauds:
        bp = M.baud_plan(fs, pb.baud)
        assert (pb.sps, pb.L, pb.h) == (bp["sps"], bp["L"], bp["h"])
        assert pb.offsets.dtype == np.int32 and np.array_equal(pb.offsets, bp["off"])
        assert M.tie_count(bp["sps"]) == ties[pb.baud], (fs, pb.baud)
    assert plan.hist_len == max(pb.L for pb in plan.bauds) - 1
    assert plan.lengths() == tuple(0 if b in skipped else M.baud_plan(fs, b)["L"] for b in M.BAUDS)


def test_the_edge_rates_are_the_edges():
    assert (BP8["sps"], BP8["L"], BP8["h"]) == (8.0, 8, 4)
    assert (BP384["sps"], BP384["L"], int(BP384["off"][31])) == (384.0, P.POCSAG_MAX_SPS, 11_904)
    assert M.baud_plan(196_609.0, 512) is None and M.baud_plan(921_600.0, 2400)["L"] == 384
    assert M.baud_plan(96_600.0, 1200)["L"] == 80  # 80.5: the tie is in L itself
    assert [M.baud_plan(9_600.0, 512)["L"], M.baud_plan(19_200.0, 512)["L"], M.baud_plan(96_600.0, 512)["L"]] == [19, 38, 189]
    # a tie rounds to even: rint differs from floor(x + 0.5) at those offsets
    bp = M.baud_plan(19_200.0, 512)
    up = np.floor(np.arange(545) * bp["sps"] + 0.5).astype(np.int64)
    assert int((up != bp["off"]).sum()) == 136  # the ties whose floor is even


@pytest.mark.parametrize("fs", list(M.EDGE_RATES))
def test_the_oracle_decodes_the_edge_streams(fs):
    """With numpy's theta: one kept sync and both messages per active baud."""
    want = M.oracle(M.theta_of(M.edge_stream(fs)), fs)
    active = [b for b in M.BAUDS if b not in M.EDGE_RATES[fs][0]]
    assert want["skipped"] == M.EDGE_RATES[fs][0]
    assert {b: len(k) for b, k in want["syncs"].items()} == {b: 1 for b in active}
    sent = [(a, f, M.shown(f, t)) for a, f, t in M.EDGE_MESSAGES]
    for baud in active:
        assert M.triples([m for m in want["messages"] if m["baud"] == baud]) == sent


def test_crafted_theta_reaches_the_integrators_full_scale():
    th = M.crafted_theta(2047, 384, seed=1)
    t, (S, _, _) = M.integrate_block(th, None, 383, (384, 0, 0))
    assert int(np.abs(t).max()) == M.T_PI and M.T_PI * 384 < 2 ** 31
    assert int(S.max()) >= 384 * 3_294_198 and int(S.min()) <= -384 * 3_294_198
    ties = th.astype(np.float64) * 2.0 ** 20
    assert int((np.mod(ties, 1.0) == 0.5).sum()) >= 2047 // 4 - 2 * 768 // 4 - 2
    h = M.crafted_history(384, seed=2)
    assert h.dtype == np.int32 and int(np.abs(h).max()) == M.T_PI
    _, (S8, _, _) = M.integrate_block(th[:7], h, 384, (8, 0, 0))
    assert int(S8[0]) == 7 * M.T_PI + int(t[0])  # the history reaches into the first outputs


@pytest.mark.parametrize("bp,start", [(BP8, 40), (BP8, 1020), (BP8, 252), (BP8, 2), (BP384, 832)])
def test_a_plateau_keeps_one_sync_at_the_smallest_index(bp, start):
    S = M.crafted_plane(bp, [start], [M.word_levels(M.SYNC)])
    stats: dict = {}
    assert M.sync_search(S, bp, stats) == [(start, 0, False, 0)]
    assert stats["near"] - stats["gated"] >= int(bp["off"][1])  # every position of the first bit period is a candidate


@pytest.mark.parametrize("inverted", [False, True])
def test_sync_errors_up_to_two_are_kept_three_are_refused(inverted):
    sign = -1 if inverted else 1
    for bp in (BP8, BP384):
        for k, sigma in ((0, 0), (1, 2000), (2, 4000)):
            S = M.crafted_plane(bp, [40], [M.word_levels(M.flipped(M.SYNC, (3, 4, 5)[:k]), inverted=inverted)])
            assert M.sync_search(S, bp) == [(40, sign * sigma, inverted, k)]
        S = M.crafted_plane(bp, [40], [M.word_levels(M.flipped(M.SYNC, (3, 4, 5)), inverted=inverted)])
        assert M.sync_search(S, bp) == []


def test_the_eye_gate_flips_and_can_sit_on_equality():
    level, kept, dropped = M.eye_gate_flip(BP8, 1000)
    assert level == 220 and len(M.sync_search(kept, BP8)) == 1 and M.sync_search(dropped, BP8) == []
    # 128 (31 l + A) >= 32 l + 992 A  <=>  41 l >= 9 A: equality at A = 1025, l = 225
    level, kept, dropped = M.eye_gate_flip(BP8, 1025)
    least, energy = M.eye_gate_terms(kept, BP8, 40)
    assert level == 225 and least == energy
    least, energy = M.eye_gate_terms(dropped, BP8, 40)
    assert least < energy


def test_the_stream_end_decides_the_last_position():
    last = 40 + int(BP8["off"][31])
    S = M.crafted_plane(BP8, [40], [M.word_levels(M.SYNC)])
    assert M.sync_search(S[: last + 1], BP8) == [(40, 0, False, 0)]
    assert M.sync_search(S[:last], BP8) == []
    assert M.sync_search(S[: int(BP8["off"][31])], BP8) == []
    wide = dict(BP8, h=384)  # a radius beyond both ends of the plane
    assert M.sync_search(S[: last + 1], wide) == [(40, 0, False, 0)]


def test_error_patterns_give_32_corrected_496_refused_and_no_triple_passes():
    cw = M.codeword(0x12345)
    e = M.error_words(cw)
    assert [len(e[k]) for k in ("clean", "single", "double", "triple")] == [1, 32, 496, 500]
    assert M.correct(cw) == (cw, 0)
    assert all(M.correct(w) == (cw, 1) for w in e["single"])
    assert all(M.correct(w) == (w, 2) for w in e["double"])
    assert all(M.correct(w) == (w, 2) for w in M.error_words(cw, triples=4960)["triple"])
    words = e["clean"] + e["single"] + e["double"] + e["triple"]
    S, starts, batches = M.batch_plane(BP8, words)
    kept = M.sync_search(S, BP8)
    assert [k[0] for k in kept] == starts and all(k[1:] == (0, False, 0) for k in kept)
    hist = Counter()
    for (n0, sigma, inv, _d), b in zip(kept, batches):
        fixed, raw, status = M.read_batch(S, BP8, n0, sigma, inv)
        assert raw == b
        hist.update(status)
    pad = -len(words) % 16
    assert hist == {0: 1 + pad, 1: 32, 2: 996}


def test_the_codeword_threshold_and_absence_sit_on_their_boundaries():
    S, starts, batches = M.batch_plane(BP8, [M.codeword(0x12345)] * 16)
    n0 = starts[0]
    at = int(S[n0 + int(BP8["off"][32])])
    assert at == 1000  # the first bit of the first codeword is a 0
    _, raw_eq, _ = M.read_batch(S, BP8, n0, 32 * at, False)
    _, raw_up, _ = M.read_batch(S, BP8, n0, 32 * at + 1, False)
    assert raw_eq[0] >> 31 == 0 and raw_up[0] >> 31 == 1
    for c in (0, 7, 15):
        end = n0 + int(BP8["off"][32 * (1 + c) + 31])
        assert M.read_batch(S[: end + 1], BP8, n0, 0, False)[2] == [0] * (c + 1) + [3] * (15 - c)
        assert M.read_batch(S[:end], BP8, n0, 0, False)[2] == [0] * c + [3] * (16 - c)
