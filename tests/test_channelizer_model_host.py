"""The channelizer model (tests/channelizer_model.py) before it judges a kernel (tests/test_gpu_channelizer_shapes.py):
its direct float64 sum against the oracle chain through Channelizer's own tap rotation, the 2^24 condition of every exact
case, the path every GPU case is meant to reach against the restated launch arithmetic, and the tile permutation.
No GPU needed."""
from __future__ import annotations

import numpy as np
import pytest
import channelizer_model as M

from iq_to_audio_amd import dsp_plan as P
from oracle import cpu_ref as O


def _capture(fmt: str, n: int, seed: int = 9):
    rng = np.random.default_rng(seed)
    if fmt == "s16":
        return rng.integers(-20000, 20000, size=2 * n).astype(np.int16)
    if fmt == "u8":
        return rng.integers(0, 255, size=2 * n).astype(np.uint8)
    return rng.normal(scale=0.3, size=2 * n).astype(np.float32)


def plan_args(plan) -> dict:
    return dict(ntaps=plan.ntaps, decimation=plan.decimation, conj_sum=plan.conj_sum, rotate=plan.rotate, rot_step=plan.rot_step,
                rot_base=plan.rot_base, scale=plan.out_scale)


@pytest.mark.parametrize("order", P.IQ_ORDERS)
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_direct_agrees_with_the_oracle_chain(fmt, order):
    """mix -> overlap-save -> decimate of the oracle against `direct` on dsp_plan's rotated taps, fed ragged blocks with
    the history carried in numpy.  The oracle rounds to complex64 after the mixer (2^-24 |x| per sample, through a filter
    of sum |h| ~ 1.3), after the filter and keeps the oscillator in complex64; `direct` sees float32 taps: a few 1e-7 at
    |z| <= 1, far inside 2e-6."""
    fs, f_off, d, n = 1e6, 31250.0, 10, 6000
    taps = P.design_channel_filter(fs, 12500.0, d)
    plan = P.plan_channel(taps, sample_rate=fs, freq_offset=f_off, mix_sign=-1, decimation=d, fmt=fmt, iq_order=order)
    assert plan.taps_window.size == M.padded_len(plan.ntaps) and plan.ntaps == 1025
    raw = _capture(fmt, n)
    nco, fir, dst = O.NcoState(f_off, fs), O.OverlapSaveState(taps, 4096), O.DecimState(d)
    hist, consumed, keep = None, 0, plan.ntaps - 1
    for lo, hi in zip([0, 7, 500, 1501, 1502], [7, 500, 1501, 1502, n]):
        blk = raw[2 * lo:2 * hi]
        want = O.decimate(O.overlap_save(O.nco_mix(O.ingest_to_complex64(blk, fmt, order), nco, -1), fir), dst)
        m_first = -(-consumed // d)
        n_out = -(-(consumed + hi - lo) // d) - m_first
        got = M.direct(plan.taps_window, blk, fmt, hist, consumed, m_first, n_out, **plan_args(plan))
        assert got.shape == want.shape, (lo, hi)
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
        assert hi < n or np.abs(want).max() > 1e-3  # (behind the filter's transient: a non-trivial comparison)
        nxt = M.history_next(hist, blk, fmt, keep, hi - lo).view(M.FMT_DTYPE[fmt])
        whole = np.concatenate([np.zeros(2 * keep, raw.dtype) + (128 if fmt == "u8" else 0), raw[:2 * hi]])
        assert np.array_equal(nxt, whole[2 * hi:2 * (hi + keep)])  # the carried history is the stream's last L - 1 frames
        hist, consumed = nxt, consumed + hi - lo


def test_the_fft_form_is_the_same_sum():
    fs, d = 10e6, 104
    taps = P.design_channel_filter(fs, 12500.0, d)
    plan = P.plan_channel(taps, sample_rate=fs, freq_offset=1.2e6, mix_sign=1, decimation=d)
    raw = _capture("s16", 60_000, seed=3)
    kw = dict(ntaps=plan.ntaps, decimation=d)
    a = M.direct(plan.taps_window, raw, "s16", None, 0, 0, 500, method="gather", **plan_args(plan))
    b = M.direct(plan.taps_window, raw, "s16", None, 0, 0, 500, method="fft", **plan_args(plan))
    ba = M.abs_sum(plan.taps_window, raw, "s16", None, 0, 0, 500, method="gather", **kw)
    bb = M.abs_sum(plan.taps_window, raw, "s16", None, 0, 0, 500, method="fft", **kw)
    assert np.all(np.abs(a - b) <= 1e-6 * M.U * ba.max())  # (the fft's error follows the stream's norm, not B_m)
    assert np.allclose(ba, bb, rtol=1e-9, atol=1e-9 * ba.max())
    assert ba.min() > 0 and np.all(np.abs(a.real) + np.abs(a.imag) <= ba * (1 + 1e-12))


def test_rotation_is_exact_at_the_quarter_turns_and_wraps():
    r = M.rotation(0, 3, 0, 0)
    assert np.array_equal(r, [1, 1, 1])
    for k, want in enumerate([1, 1j, -1, -1j]):
        assert np.array_equal(M.rotation(5, 2, 0, k << 62), [want, want])
    # a step of a quarter turn + 2^-64: the wrap of m * step is what keeps the phase small
    step = (1 << 62) + 1
    got = M.rotation(2 ** 40 + 3, 1, step, 0)[0]
    m = 2 ** 40 + 3
    assert abs(got - np.exp(2j * np.pi * ((m * step) % (1 << 64)) / 2.0 ** 64)) < 1e-12
    assert abs(got - (-1j)) < 1e-6  # m mod 4 = 3


def test_depth_and_bound_constants():
    assert M.depth(1025, "splitk") == 8 * 1 + 6 + 8 and M.depth(1025, "throughput") == 8 * 5 + 6
    assert M.depth(32769, "splitk") == 8 * 17 + 14 and M.depth(32769, "throughput") == 8 * 129 + 6
    assert (M.depth(32769, "throughput") + 5) ** 2 * M.U < 0.07  # the second-order share c_epi's last unit pays for
    assert M.form_of(16383) == "splitk" and M.form_of(16384) == "throughput"


def test_every_exact_case_satisfies_the_2_24_condition():
    """exact_data asserts it on the data (dense integer taps, zero pad, 2 L max|g| max|x| < 2^24); here for every case and
    format, and the limits the generator works with."""
    for fmt in M.FORMATS:
        for L in (1, 257, 4097, 6401):
            assert 2 * L * M.tap_limit(L, fmt) * M.X_MAX[fmt] < 2 ** 24 and M.tap_limit(L, fmt) >= 1
    assert M.tap_limit(32769, "u8") == 1 and M.tap_limit(32769, "s16") == 2 and M.tap_limit(6401, "u8") == 3
    seen = 0
    for case in M.all_cases():
        if case.n_frames > 5000 and case.ntaps < 2049:
            continue  # (the long streams of the short filters: the same generator and limits)
        for fmt in case.fmts:
            taps, raw, hist = M.exact_data(case, fmt)
            assert raw.size == 2 * case.n_frames and (hist is None) == (not case.has_hist)
            seen += 1
    assert seen > 500
    bad = np.zeros(256, dtype=np.complex64)
    bad[:5] = 3 + 3j
    with pytest.raises(AssertionError):
        M.assert_exact(bad, 5, np.array([2 ** 20 + 0j]))
    bad[2] = 3
    with pytest.raises(AssertionError):
        M.assert_exact(bad, 5, np.array([1 + 0j]))


def test_every_gpu_case_reaches_the_path_it_is_named_for():
    reached = set()
    names = set()
    for case in M.all_cases():
        assert case.name not in names, case.name
        names.add(case.name)
        assert M.refusal(case.ntaps, case.decimation, case.n_frames, case.consumed, case.m_first, case.n_out) is None, case
        t = M.tags(case.classify())
        assert case.paths <= t, (case.name, sorted(case.paths - t), sorted(t))
        reached |= t
    # over the whole table
    want = {"splitk", "throughput", "interior", "edge", "continue", "multi_slice", "guarded_hist", "guarded_front_zero",
            "guarded_behind", "guarded_straddle", "vector_in_edge", "perm_identity", "perm_whole", "perm_tail"}
    assert want <= reached, sorted(want - reached)
    # the slice `break` needs blk_first + tc >= n_frames at a slice start tc < Lpad.  The first output of a block exists
    # (o_blk < n_out), its newest frame blk_first + L - 1 is at most the launch's newest, and iqa_channelize refuses
    # newest >= n_frames ("outputs requested beyond the frames supplied"): so tc >= L.  tc is a multiple of 2048, hence of
    # 256, and Lpad is the smallest multiple of 256 that is >= L: tc >= Lpad.  Unreachable through the entry point.
    assert "break" not in reached
    print("reached:", sorted(reached), "| unreachable through iqa_channelize's argument checks: break (newest >= n_frames is refused)")


def test_the_break_is_unreachable_for_any_accepted_call():
    rng = np.random.default_rng(1)
    launched = 0
    for _ in range(600):
        L = int(rng.choice([1, 5, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 6401]))
        D = int(rng.choice([1, 2, 7, 104, 3000]))
        n_out = int(rng.integers(1, 70))
        consumed = int(rng.integers(0, 5000))
        m_first = -(-consumed // D) + int(rng.integers(0, 3))
        newest = (m_first + n_out - 1) * D - consumed
        n_frames = newest + 1 + int(rng.integers(0, 3)) * int(rng.integers(0, 5000))
        c = M.classify(L, D, n_frames, consumed, m_first, n_out, bool(rng.integers(0, 2)))
        assert c["launched"] and not c["break_slices"]
        launched += 1
    assert launched == 600


def test_named_blocks_of_the_form_switch():
    """16383 outputs are 4096 split-K blocks, 16384 are 512 throughput blocks, 16485 are 516 with a ragged last one; in
    each the head blocks straddle the history, the middle is interior and the last block's pad taps lie behind the
    frames."""
    for L in M.THROUGHPUT_L:
        for D in M.THROUGHPUT_D:
            a, b, c = (case.classify() for case in M.throughput_cases(L, D))
            assert (a["form"], a["blocks"]) == ("splitk", 4096) and (b["form"], b["blocks"]) == ("throughput", 512)
            assert (c["form"], c["blocks"]) == ("throughput", 516)
            for r in (a, b, c):
                inner = r["interior"]
                assert not inner[0] and not inner[-1] and inner[len(inner) // 2]
                head = int(np.argmax(inner))
                assert inner[head:len(inner) - 1 - int(np.argmax(inner[::-1]))].all()  # one interior stretch
            cases = M.throughput_cases(L, D)
            assert len({(k.m_first, k.consumed) for k in cases}) == 1 and cases[0].n_frames < cases[1].n_frames < cases[2].n_frames


def test_tap_limit_cases_have_the_named_block_counts():
    for L in M.TAP_LIMIT_L:
        for case in M.tap_limit_cases(L):
            c = case.classify()
            assert c["form"] == "splitk" and c["blocks"] == M.TAP_LIMIT_BLOCKS[case.n_out]
            assert c["slices"] == -(-M.padded_len(L) // M.CH_TCH)
            if not case.has_hist and L >= 4097:
                assert c["continue_slices"][0] == [0]
    assert sorted(set(M.TAP_LIMIT_BLOCKS.values())) == [1, 2, 8, 9, 10, 33]
    long_start = M.LONG_CASES[2].classify()
    assert long_start["slices"] == 17 and long_start["continue_slices"][0] == list(range(15))


def test_tile_permutation_is_a_bijection():
    counts = set(range(1, 41)) | {c.classify()["blocks"] for c in M.all_cases()}
    for nblk in sorted(counts):
        perm = M.tile_permutation(nblk)
        assert sorted(perm) == list(range(nblk)), nblk
        per = nblk >> 3
        assert perm[per * 8:] == list(range(per * 8, nblk))  # identity for the last nblk % 8
    assert {4096, 512, 516, 33, 10, 9, 8, 2, 1} <= counts
    assert M.tile_permutation(16) == [0, 2, 4, 6, 8, 10, 12, 14, 1, 3, 5, 7, 9, 11, 13, 15]
    assert M.tile_permutation(20) == [0, 2, 4, 6, 8, 10, 12, 14, 1, 3, 5, 7, 9, 11, 13, 15, 16, 17, 18, 19]
    assert M.tile_permutation(7) == list(range(7))


def test_refusals_follow_the_entry_point():
    ok = dict(ntaps=5, decimation=2, n_frames=100, consumed=10, m_first=5, n_out=20)
    assert M.refusal(**ok) is None
    assert "beyond" in M.refusal(**{**ok, "n_out": 60})
    assert "before" in M.refusal(**{**ok, "consumed": 60, "m_first": 0, "n_out": 5})
    assert "older" in M.refusal(**{**ok, "m_first": 4})
    assert "ntaps" in M.refusal(**{**ok, "ntaps": 0}) and "decimation" in M.refusal(**{**ok, "decimation": 0})
    assert M.refusal(**{**ok, "n_out": 0, "n_frames": 0}) is None
