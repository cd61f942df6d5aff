"""The POCSAG kernels (csrc/pocsag.hip) against the numpy oracle of tests/pocsag_model.py at their edge shapes, on the
MI355X: the channel rates at the plan's limits (sps 8 and 384, skipped bauds, half-integer sps), block cuts around the
carried history and the 2048-sample tile, and the three entry points called directly on crafted inputs -- full-scale and
tie-valued theta, integrator planes built from bit levels (plateaus of equal energy, 0 .. 3 sync errors, the eye gate on
and next to equality, the stream end on and next to the last evaluable position), every single and double error of a
codeword and 500 triple errors.  Integers throughout: no tolerance.  The oracle's own branch facts (kept counts, status
histograms, tie counts) are asserted before every comparison; tests/test_pocsag_shapes_host.py holds them without a GPU."""
from __future__ import annotations

import functools
import importlib.util
import sys
from collections import Counter
from ctypes import c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _load_model():
    name = "pocsag_model"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name("pocsag_model.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load_model()

MAX_SPS = 384  # IQA_POCSAG_MAX_SPS
SENT = -7_777_777  # what untouched output words hold
GUARD = 16  # sentinel words behind every output
BP8 = M.baud_plan(4096.0, 512)
BP384 = M.baud_plan(196_608.0, 512)
BATCH_KEYS = ("n0", "sigma", "inverted", "distance", "words", "raw", "status")


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


@functools.lru_cache(maxsize=None)
def _stream(fs: float) -> np.ndarray:
    z = M.edge_stream(fs)
    z.setflags(write=False)
    return z


def _same_batches(got: dict, want: dict, bauds) -> None:
    assert sorted(got) == sorted(bauds)
    for baud in bauds:
        g, kept = got[baud], want["syncs"][baud]
        assert [(int(a), int(b), bool(c), int(d)) for a, b, c, d in zip(g["n0"], g["sigma"], g["inverted"], g["distance"])] == kept, baud
        for key in ("words", "raw", "status"):
            np.testing.assert_array_equal(g[key], want["batches"][baud][key], err_msg=f"{key} {baud}")


# ---- a. rate classes through PocsagDecoder ------------------------------------------------------------------------------


@pytest.mark.parametrize("fs", list(M.EDGE_RATES))
def test_rate_classes(A, fs):
    """One transmission per active baud, fed in three blocks: t is the oracle's quantiser of the GPU's own theta; from that
    t the integrator planes, kept syncs, corrected and raw words, status and messages are the oracle's."""
    from iq_to_audio_amd.decoders.pocsag import PocsagDecoder

    skipped, ties = M.EDGE_RATES[fs]
    active = [b for b in M.BAUDS if b not in skipped]
    for baud in active:
        assert M.tie_count(fs / baud) == ties[baud], baud
    z = _stream(fs)
    dec = PocsagDecoder(fs)
    assert dec.plan.hist_len == max(M.baud_plan(fs, b)["L"] for b in active) - 1
    cuts = [0, z.size // 3, 2 * z.size // 3 + 1, z.size]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        dec.process(z[lo:hi])
    st = dec.stages()
    assert st["t"].dtype == np.int32 and st["t"].size == z.size
    np.testing.assert_array_equal(st["t"], M.quantise(st["theta"]))
    want = M.oracle(fs=fs, t=st["t"])
    assert want["skipped"] == skipped and {b: len(k) for b, k in want["syncs"].items()} == {b: 1 for b in active}
    assert sorted(st["S"]) == active
    for baud in active:
        np.testing.assert_array_equal(st["S"][baud], want["S"][baud], err_msg=f"S {baud}")
    _same_batches(st["batches"], want, active)
    res = dec.finish()
    assert res is not None and res.bauds_skipped == skipped
    sent = [(a, f, M.shown(f, t)) for a, f, t in M.EDGE_MESSAGES]
    assert M.triples(res.messages) == M.triples(want["messages"])
    for baud in active:
        assert M.triples([m for m in res.messages if m.baud == baud]) == sent, baud
    assert res.syncs == {b: 1 for b in active} and res.codewords["uncorrectable"] == 0 and res.codewords["absent"] == 0


# ---- b. block invariance at the limits ----------------------------------------------------------------------------------


@pytest.mark.parametrize("fs,hist_len", [(196_608.0, 383), (19_200.0, 37)])
def test_block_invariance_at_the_limits(A, fs, hist_len):
    """One block against a first block of one sample, blocks shorter than the history, and first blocks that end one
    before, on and one behind the first and the second tile edge: bit-identical t, S and batches."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.decoders.pocsag import PocsagDecoder

    z = D.to_device(_stream(fs), "complex64")
    n = int(z.numel())
    short = [0, 1, 1 + hist_len - 1, 1 + 2 * (hist_len - 1), 1 + 2 * (hist_len - 1) + 5, 2047, 2048, 2049, 4095, 4096, 4097, n - hist_len + 2, n]
    schedules = [[0, n], [0, 1, n], short] + [[0, c, n] for c in (2047, 2048, 2049, 4095, 4096, 4097)]
    runs = []
    for cuts in schedules:
        dec = PocsagDecoder(fs)
        assert dec.plan.hist_len == hist_len
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            assert lo < hi
            dec.process(z[lo:hi])
        assert dec.core.pos == n
        runs.append(dec.stages())
    assert min(b - a for a, b in zip(short[:-1], short[1:])) == 1 and hist_len - 1 in [b - a for a, b in zip(short[:-1], short[1:])]
    assert all(len(b["n0"]) == 1 for b in runs[0]["batches"].values()) and len(runs[0]["batches"]) == 3
    for st in runs[1:]:
        np.testing.assert_array_equal(st["theta"], runs[0]["theta"])
        np.testing.assert_array_equal(st["t"], runs[0]["t"])
        for baud in M.BAUDS:
            np.testing.assert_array_equal(st["S"][baud], runs[0]["S"][baud], err_msg=f"S {baud}")
            for key in BATCH_KEYS:
                np.testing.assert_array_equal(st["batches"][baud][key], runs[0]["batches"][baud][key], err_msg=f"{key} {baud}")


# ---- c. iqa_pocsag_integrate on crafted theta ---------------------------------------------------------------------------


def _integrate(theta, hist, hist_len, windows, n=None):
    """-> (t[n + GUARD], [S[n + GUARD] or None] * 3): every output pre-filled with SENT."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    n = theta.size if n is None else n
    th = D.from_numpy(theta)
    h = None if hist is None else D.from_numpy(hist)
    t = D.from_numpy(np.full(n + GUARD, SENT, dtype=np.int32))
    planes = [D.from_numpy(np.full(n + GUARD, SENT, dtype=np.int32)) if L else None for L in windows]
    outs = (c_void_p * 3)(*[None if p is None else p.data_ptr() for p in planes])
    N.call("iqa_pocsag_integrate", N.ptr(th), c_int64(n), N.ptr(h), c_int32(hist_len), (c_int32 * 3)(*windows), N.ptr(t), outs,
           N.stream_ptr())
    return t.cpu().numpy(), [None if p is None else p.cpu().numpy() for p in planes]


INT_WINDOWS = [(384, 164, 82), (8, 0, 0), (0, 0, 8), (38, 16, 8)]
INT_LENGTHS = [1, 7, 8, 9, 2047, 2048, 2049, 4097]


@pytest.mark.parametrize("windows", INT_WINDOWS)
def test_integrate_on_crafted_theta(A, windows):
    """Random, tie-valued and held +-pi theta, every tile-edge length, NULL and full-scale history, the shortest and the
    longest admitted history: t and S are the oracle's, NULL outputs of inactive bauds are never touched, nothing is
    written behind n."""
    l_max = max(windows)
    seen_full_scale = False
    for n in INT_LENGTHS:
        theta = M.crafted_theta(n, l_max, seed=n)
        for hist_len in (l_max - 1, MAX_SPS):
            for hist in (None, M.crafted_history(hist_len, seed=n + hist_len)):
                want_t, want_s = M.integrate_block(theta, hist, hist_len, windows)
                if l_max == MAX_SPS and n >= 2047:
                    assert max(int(np.abs(s).max()) for s in want_s if s is not None) >= 384 * 3_294_198
                    seen_full_scale = True
                if hist is not None:
                    assert int(want_s[windows.index(l_max)][0]) != int(M.integrate_block(theta, None, hist_len, windows)[1][windows.index(l_max)][0])
                t, planes = _integrate(theta, hist, hist_len, windows)
                tag = f"n {n} hist_len {hist_len} hist {'NULL' if hist is None else 'given'}"
                np.testing.assert_array_equal(t[:n], want_t, err_msg=tag)
                assert (t[n:] == SENT).all(), tag
                for L, got, want in zip(windows, planes, want_s):
                    assert (got is None) == (L == 0) == (want is None)
                    if L:
                        np.testing.assert_array_equal(got[:n], want, err_msg=f"S of window {L}, {tag}")
                        assert (got[n:] == SENT).all(), tag
    assert seen_full_scale == (l_max == MAX_SPS)


def test_integrate_rejects_before_it_launches(A):
    """A history shorter than the longest window - 1, a window or a history above IQA_POCSAG_MAX_SPS and a call without an
    active baud are refused with the error code, and no output word changes."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    th = D.from_numpy(M.crafted_theta(64, 8, seed=0))
    for windows, hist_len, what in (((38, 16, 8), 36, "hist_len"), ((385, 0, 0), 384, "window"), ((0, 0, 0), 384, "no active baud"),
                                    ((8, 0, 0), 385, "hist_len")):
        outs = [D.from_numpy(np.full(64, SENT, dtype=np.int32)) for _ in range(4)]
        table = (c_void_p * 3)(*[p.data_ptr() for p in outs[1:]])
        with pytest.raises(ValueError, match=what):
            N.call("iqa_pocsag_integrate", N.ptr(th), c_int64(64), c_void_p(0), c_int32(hist_len), (c_int32 * 3)(*windows), N.ptr(outs[0]),
                   table, N.stream_ptr())
        D.torch_mod().cuda.synchronize()
        assert all((p.cpu().numpy() == SENT).all() for p in outs), what


# ---- d. iqa_pocsag_sync on crafted integrator planes --------------------------------------------------------------------


def _sync(S, bp, half_bit=None, capacity=64):
    """-> (kept [(n0, Sigma, inverted, distance)] ascending, score plane int64[n], untouched list tail intact)."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    n = int(S.size)
    s = D.from_numpy(np.ascontiguousarray(S, dtype=np.int32))
    score = D.from_numpy(np.full(n + GUARD, SENT, dtype=np.int64))
    lst = D.from_numpy(np.full(4 * capacity, SENT, dtype=np.int64))
    count = D.from_numpy(np.array([99], dtype=np.int64))
    offs = (c_int32 * 32)(*[int(v) for v in bp["off"][:32]])
    N.call("iqa_pocsag_sync", N.ptr(s), c_int64(n), offs, c_int32(bp["h"] if half_bit is None else half_bit), N.ptr(score), N.ptr(lst),
           c_int64(capacity), N.ptr(count), N.stream_ptr())
    k = int(count.item())
    assert k <= capacity
    plane, entries = score.cpu().numpy(), lst.cpu().numpy().reshape(-1, 4)
    assert (plane[n:] == SENT).all() and (entries[k:] == SENT).all()
    kept = sorted((int(a), int(b), bool(c), int(d)) for a, b, c, d in entries[:k])
    return kept, plane[:n]


def _same_sync(S, bp, expect, half_bit=None):
    """The oracle gives ``expect``; the GPU's list is the oracle's and its score plane marks the oracle's candidates."""
    model_bp = bp if half_bit is None else dict(bp, h=half_bit)
    stats: dict = {}
    want = M.sync_search(S, model_bp, stats)
    assert want == expect, (want, expect)
    kept, score = _sync(S, bp, half_bit)
    assert kept == want
    assert int((score != 0).sum()) == stats.get("near", 0) - stats.get("gated", 0)
    assert (score >= 0).all()
    for n0, _s, inverted, _d in want:
        assert score[n0] == score.max() and bool(score[n0] & 1) == inverted
    return score


@pytest.mark.parametrize("start", [40, 1020, 252, 2])
def test_sync_plateau_keeps_the_smallest_index(A, start):
    """Eight candidates of identical energy: in one thread group, across the 1024-position tile of the score kernel, across a
    256-thread group of the keep kernel, and with a neighbourhood clipped at index 0."""
    S = M.crafted_plane(BP8, [start], [M.word_levels(M.SYNC)])
    score = _same_sync(S, BP8, [(start, 0, False, 0)])
    assert int((score == score.max()).sum()) == 8 and (score[start : start + 8] == score.max()).all()


@pytest.mark.parametrize("bp,start", [(BP8, 40), (BP384, 832)], ids=["sps8", "sps384"])
@pytest.mark.parametrize("inverted", [False, True])
def test_sync_errors_in_both_polarities(A, bp, start, inverted):
    """0, 1 and 2 wrong sync bits are kept with their distance and Sigma, 3 are refused; at sps 384 the plateau lies across
    the tile edge at 1024, so position 1023 reads the last word of the largest LDS window."""
    sign = -1 if inverted else 1
    for k, sigma in ((0, 0), (1, 2000), (2, 4000), (3, None)):
        S = M.crafted_plane(bp, [start], [M.word_levels(M.flipped(M.SYNC, (3, 4, 5)[:k]), inverted=inverted)])
        expect = [] if sigma is None else [(start, sign * sigma, inverted, k)]
        score = _same_sync(S, bp, expect)
        if sigma is not None:
            sps = int(bp["off"][1])
            assert int((score == score.max()).sum()) == sps
            assert start < 1024 < start + sps or sps == 8


@pytest.mark.parametrize("amplitude,level", [(1000, 220), (1025, 225)])
def test_sync_eye_gate_at_its_flip_point(A, amplitude, level):
    """The first sync bit shrunk until 128 min |x| >= E fails: the GPU keeps and drops where the oracle does.  At amplitude
    1025 the last kept level sits on equality (41 l = 9 A)."""
    found = M.eye_gate_flip(BP8, amplitude)
    assert found is not None and found[0] == level
    _lvl, kept, dropped = found
    least, energy = M.eye_gate_terms(kept, BP8, 40)
    assert least >= energy and (amplitude != 1025 or least == energy)
    least, energy = M.eye_gate_terms(dropped, BP8, 40)
    assert least < energy
    _same_sync(kept, BP8, [(40, level - amplitude, False, 0)])
    _same_sync(dropped, BP8, [])


def test_sync_at_the_stream_end(A):
    """A sync at the very last evaluable position is kept, one sample fewer and it is not; a plane no longer than off[31]
    gives a score plane of zeros and a count of 0; a radius beyond both ends of the plane clips the neighbourhood."""
    S = M.crafted_plane(BP8, [40], [M.word_levels(M.SYNC)])
    last = 40 + int(BP8["off"][31])
    _same_sync(S[: last + 1], BP8, [(40, 0, False, 0)])
    _same_sync(S[:last], BP8, [])
    for n in (int(BP8["off"][31]), int(BP8["off"][31]) - 1, 1):
        kept, score = _sync(S[40 : 40 + n], BP8)
        assert kept == [] and (score == 0).all()
    for n in (last + 1, last + 2, S.size):  # a + half_bit > n - 1 for every candidate, a - half_bit < 0 as well
        _same_sync(S[:n], BP8, [(40, 0, False, 0)], half_bit=MAX_SPS)
    two = M.crafted_plane(BP8, [2, 2 + 300], [M.word_levels(M.SYNC)] * 2, n=2 + 300 + int(BP8["off"][31]) + 1)
    _same_sync(two, BP8, [(2, 0, False, 0), (302, 0, False, 0)])
    _same_sync(two, BP8, [(2, 0, False, 0)], half_bit=MAX_SPS)  # the later one loses the tie at any distance inside the radius


# ---- e. iqa_pocsag_codewords on the plateau planes ----------------------------------------------------------------------


def _codewords(S, bp, entries, n=None):
    """entries [(m, Sigma, inverted)] -> (fixed, raw, status) as uint32 / uint32 / uint8 [k, 16]."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    n = int(S.size) if n is None else n
    k = len(entries)
    s = D.from_numpy(np.ascontiguousarray(S[:n], dtype=np.int32))
    lst = D.from_numpy(np.array([[m, sg, int(inv), 0] for m, sg, inv in entries], dtype=np.int64).reshape(-1))
    offs = D.from_numpy(np.ascontiguousarray(bp["off"], dtype=np.int32))
    fixed = D.from_numpy(np.full(16 * k + GUARD, SENT, dtype=np.int32))
    raw = D.from_numpy(np.full(16 * k + GUARD, SENT, dtype=np.int32))
    status = D.from_numpy(np.full(16 * k + GUARD, 0xAA, dtype=np.uint8))
    N.call("iqa_pocsag_codewords", N.ptr(s), c_int64(n), N.ptr(lst), c_int64(k), N.ptr(offs), N.ptr(fixed), N.ptr(raw), N.ptr(status),
           N.stream_ptr())
    f, r, st = fixed.cpu().numpy(), raw.cpu().numpy(), status.cpu().numpy()
    assert (f[16 * k :] == SENT).all() and (r[16 * k :] == SENT).all() and (st[16 * k :] == 0xAA).all()
    return f[: 16 * k].view(np.uint32).reshape(k, 16), r[: 16 * k].view(np.uint32).reshape(k, 16), st[: 16 * k].reshape(k, 16)


def _read(S, bp, entries):
    rows = [M.read_batch(S, bp, m, sg, inv) for m, sg, inv in entries]
    return tuple(np.array([r[i] for r in rows], dtype=dt).reshape(-1, 16) for i, dt in enumerate((np.uint32, np.uint32, np.uint8)))


@pytest.mark.parametrize("inverted", [False, True])
def test_codewords_of_every_error_pattern(A, inverted):
    """A clean word, its 32 single, 496 double and 500 triple errors, 65 batches in one plane: the sync search finds every
    batch at its plateau's first position, and the corrected words, raw words and status are the oracle's -- 32 restored,
    every double and triple error refused with its raw word kept."""
    cw = M.codeword(0x12345)
    e = M.error_words(cw)
    words = e["clean"] + e["single"] + e["double"] + e["triple"]
    S, starts, batches = M.batch_plane(BP8, words)
    if inverted:
        S = -S
    want_kept = M.sync_search(S, BP8)
    assert want_kept == [(a, 0, inverted, 0) for a in starts] and len(starts) == 65
    kept, _score = _sync(S, BP8, capacity=128)
    assert kept == want_kept
    entries = [(a, sg, inv) for a, sg, inv, _d in kept]
    want = _read(S, BP8, entries)
    assert want[1].reshape(-1).tolist() == [w for b in batches for w in b]
    hist = Counter(want[2].reshape(-1).tolist())
    assert hist == {0: 1 + (-len(words) % 16), 1: 32, 2: 996}
    flat_fixed, flat_status = want[0].reshape(-1), want[2].reshape(-1)
    assert (flat_fixed[1:33] == cw).all() and (flat_status[1:33] == 1).all()
    assert (flat_status[33 : 33 + 996] == 2).all() and (flat_fixed[33 : 33 + 996] == want[1].reshape(-1)[33 : 33 + 996]).all()
    got = _codewords(S, BP8, entries)
    for g, w, name in zip(got, want, ("corrected", "raw", "status")):
        np.testing.assert_array_equal(g, w, err_msg=name)


def test_codeword_threshold_absence_and_empty_entries(A):
    """Sigma on and one above 32 S at the first bit of the first codeword; planes that end on and one before the last bit of
    codeword c; a list entry with m = -1."""
    cw = M.codeword(0x12345)
    S, starts, _batches = M.batch_plane(BP8, [cw] * 16)
    n0 = starts[0]
    at = int(S[n0 + int(BP8["off"][32])])
    entries = [(n0, 32 * at, False), (n0, 32 * at + 1, False), (n0, 32 * at - 1, False), (n0, -32 * at, True), (n0, -32 * at - 1, True), (n0, 0, False)]
    want = _read(S, BP8, entries)
    assert [int(r[0]) >> 31 for r in want[1]] == [0, 1, 0, 1, 1, 0] and at == 1000
    assert want[1][0, 0] != want[1][1, 0] and (want[1][5] == cw).all() and (want[2][5] == 0).all()
    got = _codewords(S, BP8, entries)
    for g, w, name in zip(got, want, ("corrected", "raw", "status")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    for c in (0, 7, 15):
        end = n0 + int(BP8["off"][32 * (1 + c) + 31])
        for n, present in ((end + 1, c + 1), (end, c)):
            want = _read(S[:n], BP8, [(n0, 0, False)])
            assert want[2][0].tolist() == [0] * present + [3] * (16 - present)
            assert (want[0][0, present:] == 0).all() and (want[1][0, present:] == 0).all()
            got = _codewords(S, BP8, [(n0, 0, False)], n=n)
            for g, w, name in zip(got, want, ("corrected", "raw", "status")):
                np.testing.assert_array_equal(g, w, err_msg=f"{name}, codeword {c}, n {n}")
    fixed, raw, status = _codewords(S, BP8, [(-1, 0, False), (n0, 0, False)])
    assert (status[0] == 3).all() and (fixed[0] == 0).all() and (raw[0] == 0).all()
    assert (status[1] == 0).all() and (fixed[1] == cw).all()


def test_codewords_at_the_largest_window(A):
    """sps 384: the codeword offsets reach off[543] = 208 512 behind a sync found across the tile edge."""
    cw = M.codeword(0x12345)
    words = [M.flipped(cw, (k,)) for k in (0, 31)] + [M.flipped(cw, (3, 20))] + [cw] * 13
    S, starts, batches = M.batch_plane(BP384, words, lead=832)
    want_kept = M.sync_search(S, BP384)
    assert want_kept == [(832, 0, False, 0)]
    kept, score = _sync(S, BP384)
    assert kept == want_kept and int((score != 0).sum()) >= 384
    want = _read(S, BP384, [(832, 0, False)])
    assert want[2][0].tolist() == [1, 1, 2] + [0] * 13 and want[1][0].tolist() == batches[0]
    got = _codewords(S, BP384, [(832, 0, False)])
    for g, w, name in zip(got, want, ("corrected", "raw", "status")):
        np.testing.assert_array_equal(g, w, err_msg=name)


def test_sync_refuses_before_it_clears_the_count(A):
    """A call refused for a NULL plane, score or list pointer leaves the count, and every other buffer, as they were."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    offs = (c_int32 * 32)(*[int(v) for v in BP8["off"][:32]])
    for missing in ("s", "score", "list"):
        bufs = dict(s=D.from_numpy(np.full(1024, SENT, dtype=np.int32)), score=D.from_numpy(np.full(1024, SENT, dtype=np.int64)),
                    list=D.from_numpy(np.full(64, SENT, dtype=np.int64)), count=D.from_numpy(np.array([SENT, SENT], dtype=np.int64)))
        arg = {k: None if k == missing else v for k, v in bufs.items()}
        with pytest.raises(ValueError, match="NULL device pointer"):
            N.call("iqa_pocsag_sync", N.ptr(arg["s"]), c_int64(1024), offs, c_int32(BP8["h"]), N.ptr(arg["score"]), N.ptr(arg["list"]), c_int64(4),
                   N.ptr(arg["count"]), N.stream_ptr())
        D.torch_mod().cuda.synchronize()
        assert all((v.cpu().numpy() == SENT).all() for v in bufs.values()), missing
