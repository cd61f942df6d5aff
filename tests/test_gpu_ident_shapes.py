"""The kernels of the protocol identification on the MI355X at their edge shapes, on crafted theta streams
and crafted planes, the oracle's expectation asserted first and the comparison exact: the integrator at L = 4, 33 and 224 and at
lengths around its tile, at full scale, on quantiser ties and with every centre, nothing written behind n; the search at the
stream's end, on the threshold's equality, on plateaus across a score tile, a keep thread group and the stream's start, with a
word and its negation, with pre and post at the stream's ends, with two patterns at one position, at 4 and at 224 samples to a
symbol, and with a hit list of one entry."""
from __future__ import annotations

import importlib.util
import sys
from ctypes import c_int8, c_int32, c_int64
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


IM = _load("ident_model")
SENTINEL = -123456789
RATE_OF_L = {4: (19_200.0, 4800), 33: (158_400.0, 4800), 224: (358_400.0, 1600)}  # a channel rate and a family with sps = L


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _gpu_integrate(theta, L: int, sh: int, c: int) -> np.ndarray:
    """iqa_ident_integrate into a buffer with 64 sentinels behind n, which must stay."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    theta = np.ascontiguousarray(theta, dtype=np.float32)
    n = theta.size
    out = D.from_numpy(np.full(n + 64, SENTINEL, dtype=np.int32))
    N.call("iqa_ident_integrate", N.ptr(D.from_numpy(theta)), c_int64(n), c_int32(L), c_int32(sh), c_int32(c), N.ptr(out), N.stream_ptr())
    got = out.cpu().numpy()
    assert (got[n:] == SENTINEL).all()
    return got[:n]


def _pkg_patterns(pats):
    from iq_to_audio_amd import identify as I

    return tuple(I.SyncPattern(*p) for p in pats)


def _gpu_search(v, fs_ch: float, rate: int, pats, capacity: int):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd import identify as I

    score, hits = I.search(D.from_numpy(np.ascontiguousarray(v, dtype=np.int32)), P.plan_ident(fs_ch, rate), _pkg_patterns(pats), capacity)
    return score.cpu().numpy(), [tuple(h) for h in hits.tolist()]


def _search(v, fs_ch: float, rate: int, pats=None, capacity: int = 64):
    """The oracle's planes and kept hits of a crafted plane, the GPU held to both."""
    pats = IM.family(rate) if pats is None else pats
    pl = IM.plan(fs_ch, rate)
    planes, kept = IM.search(v, pl, pats)
    score, hits = _gpu_search(v, fs_ch, rate, pats, capacity)
    np.testing.assert_array_equal(score, planes)
    assert hits == kept
    return planes, kept


# ---- the integrator -----------------------------------------------------------------------------------------------------------


def _theta(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    theta = rng.uniform(-np.pi, np.pi, n).astype(np.float32)
    for at, value in ((0, np.nan), (3, np.inf), (5, -np.inf), (6, 9.0), (n - 1, -9.0), (n // 2, 2.5 / 4096), (n // 3, -1.5 / 4096)):
        if 0 <= at < n:
            theta[at] = value
    return theta


@pytest.mark.parametrize("L", [4, 33, 224])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2048, 2049, 4097])
def test_integrator_lengths_and_centres(A, L, n):
    sh = IM.plan(*RATE_OF_L[L])["sh"]
    theta = _theta(n, 100 * L + n)
    for c in (0, 300, -300, 32767, -32767):
        want = IM.integrate(theta, c, L, sh)
        assert np.abs(want).max() <= IM.V_MAX
        if n <= 9:
            assert want.tolist() == IM.integrate_by_loops(theta, c, L, sh)
        np.testing.assert_array_equal(_gpu_integrate(theta, L, sh, c), want, err_msg=f"c = {c}")


@pytest.mark.parametrize("L", [4, 33, 224])
def test_integrator_at_full_scale_and_on_ties(A, L):
    sh = IM.plan(*RATE_OF_L[L])["sh"]
    for value, c, t in ((np.pi, 0, 12868), (-np.pi, 0, -12868), (np.pi, -32767, 12868), (9.0, -32767, 32767), (-9.0, 32767, -32767)):
        theta = np.full(2 * L, value, dtype=np.float32)
        want = IM.integrate(theta, c, L, sh)
        assert int(want[-1]) == ((t - c) * L) >> sh and int(want[0]) == (t - c) >> sh and abs(int(want[-1])) <= IM.V_MAX  # the int32 and sh bound
        np.testing.assert_array_equal(_gpu_integrate(theta, L, sh, c), want)
    # exact .5 ties go to the even neighbour: t = 0, 2, 2, 4 and their negatives, one a sample, the rest zero
    ties = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5], dtype=np.float32) / np.float32(4096.0)
    theta = np.zeros(8 * (L + 1), dtype=np.float32)
    theta[:: L + 1] = ties
    want = IM.integrate(theta, 0, L, 0)
    assert want[:: L + 1].tolist() == [0, 2, 2, 4, 0, -2, -2, -4] and IM.K.quantise(ties).tolist() == [0, 2, 2, 4, 0, -2, -2, -4]
    np.testing.assert_array_equal(_gpu_integrate(theta, L, 0 if L <= 64 else sh, 0), IM.integrate(theta, 0, L, 0 if L <= 64 else sh))
    if L <= 64:
        np.testing.assert_array_equal(_gpu_integrate(theta, L, 0, 0), want)


# ---- the search ---------------------------------------------------------------------------------------------------------------

FLEX_FS = 19_200.0  # 12 samples to a bit at 1600
FS5 = 24_000.0  # 5 samples to a symbol at 4800


def test_stream_end():
    pl = IM.plan(FLEX_FS, 1600)
    flex = IM.symbols(IM.family(1600)[0])
    n = pl["o"][31] + 1
    v = IM.crafted_plane(n, pl, 0, flex)
    planes, kept = _search(v, FLEX_FS, 1600)
    assert [(m, C, E, pre, post) for _, m, C, E, pre, post in kept] == [(0, 32_000, 32_000_000, 0, 0)]  # exactly one evaluated position
    assert np.count_nonzero(planes) == 1 and planes[0, 0] == 64_000
    planes, kept = _search(v[:-1], FLEX_FS, 1600)  # one sample fewer: none
    assert not planes.any() and kept == []
    # the patterns of one family end at their own last symbol
    pl = IM.plan(FS5, 4800)
    lev = IM.symbols(IM.family(4800)[1])
    v = IM.crafted_plane(pl["o"][23] + 1, pl, 0, lev, amp=-40)
    planes, kept = _search(v, FS5, 4800)
    assert [(j, m, C) for j, m, C, *_ in kept if j == 1] == [(1, 0, -40 * 9 * 24)] and np.count_nonzero(planes[:3]) == 1


def test_threshold_on_equality():
    pl = IM.plan(FLEX_FS, 1600)
    sym = IM.symbols(IM.family(1600)[0])
    for k, stays in ((5, True), (6, True), (7, False)):  # 16 (32 - k) >= 416, on equality at k = 6
        lev = list(sym)
        for i in range(k):
            lev[3 * i + 1] = 0
        for amp in (1, -900, IM.V_MAX):
            planes, kept = _search(IM.crafted_plane(700, pl, 60, lev, amp=amp), FLEX_FS, 1600)
            assert [(m, C) for _, m, C, *_ in kept] == ([(60, amp * (32 - k))] if stays else []), (k, amp)
            assert bool(planes[0, 60]) == stays
    pl = IM.plan(FS5, 4800)
    p25 = IM.symbols(IM.family(4800)[2])
    for k, stays in ((4, True), (5, False)):  # a +-3 pattern: 16 * 9 (24 - k) >= 13 * 216 holds up to k = 4
        lev = [0 if i < k else s for i, s in enumerate(p25)]
        planes, kept = _search(IM.crafted_plane(400, pl, 20, lev, amp=IM.V_MAX // 3), FS5, 4800)
        assert bool(planes[2, 20]) == stays and [(j, m) for j, m, *_ in kept if j == 2] == ([(2, 20)] if stays else [])


@pytest.mark.parametrize("start", [0, 1, 254, 1022, 1023, 2046])
def test_plateaus_keep_their_first_position(A, start):
    """Symbols of constant level give a plateau of equal |C| as wide as a symbol: across a score tile's edge (1024), a keep thread
    group's edge (256) and at m < h the smallest index is kept, and no other."""
    for fs_ch, rate in ((FLEX_FS, 1600), (FS5, 4800)):
        pl = IM.plan(fs_ch, rate)
        pat = IM.family(rate)[0]
        v = IM.crafted_plane(start + 48 * pl["L"] + 1300, pl, start, IM.symbols(pat), amp=777)
        planes, kept = _search(v, fs_ch, rate)
        assert list(np.flatnonzero(planes[0])) == list(range(start, start + pl["L"])) and len(set(planes[0, start : start + pl["L"]].tolist())) == 1
        assert [(j, m) for j, m, *_ in kept] == [(0, start)]


def test_a_word_and_its_negation_give_both_names(A):
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd import identify as I

    pl = IM.plan(FS5, 4800)
    voice = IM.symbols(IM.family(4800)[0])
    v = IM.crafted_plane(3000, pl, 100, voice, amp=500)
    v = IM.crafted_plane(3000, pl, 100 + pl["o"][24] + 144 * 5 - 120, [-s for s in voice], amp=500, base=v)
    _, kept = _search(v, FS5, 4800)
    assert [(j, m, C > 0) for j, m, C, *_ in kept] == [(0, 100, True), (0, 820, False)]
    res = I.decide(np.array(kept, dtype=np.int64), I.patterns_for(4800), P.plan_ident(FS5, 4800))
    assert res["hits"] == {"dmr bs voice": 1, "dmr bs data": 1} and res["pairs"] == {"dmr": 1} and res["protocol"] == "dmr"


def test_pre_and_post_at_the_streams_ends(A):
    pl = IM.plan(FLEX_FS, 1600)
    flex = IM.symbols(IM.family(1600)[0])
    code, other = IM.bits_of(0xDEA0, 16), IM.bits_of(0xDEA0 ^ 0xFFFF, 16)
    time_bits = lambda bits: sum(1 << k for k, b in enumerate(bits) if b > 0)  # noqa: E731
    # whole: sixteen bits on either side
    v = IM.crafted_plane(1200, pl, 300, code + flex + other, first=-16)
    _, kept = _search(v, FLEX_FS, 1600)
    assert [(m, pre, post) for _, m, _, _, pre, post in kept] == [(300, time_bits(code), time_bits(other))]
    assert IM.flex_mode(*IM.flex_words(kept[0][4], kept[0][5], False)) == "3200/4"
    # the stream starts 5 bits in front of the marker: the eleven earlier positions read as 0
    start = pl["o"][5]
    v = IM.crafted_plane(1200, pl, start, code + flex + other, first=-16)
    _, kept = _search(v, FLEX_FS, 1600)
    assert [(m, pre, post) for _, m, _, _, pre, post in kept] == [(start, time_bits([-1] * 11 + code[11:]), time_bits(other))]
    # the stream ends 9 bits behind the marker, and right behind it
    for bits in (9, 0):
        n = 300 + pl["o"][32 + bits]
        v = IM.crafted_plane(n, pl, 300, code + flex + [1] * 16, first=-16)
        _, kept = _search(v, FLEX_FS, 1600)
        assert [(m, pre, post) for _, m, _, _, pre, post in kept] == [(300, time_bits(code), (1 << bits) - 1)]
    # the marker at the stream's first sample
    _, kept = _search(IM.crafted_plane(800, pl, 0, flex + other), FLEX_FS, 1600)
    assert [(m, pre, post) for _, m, _, _, pre, post in kept] == [(0, 0, time_bits(other))]


def test_two_patterns_at_one_position(A):
    word = 0x755FD7DF75F7
    pats = (("dmr", "whole", "whole-", word, 24, 144, (4800,), False), ("dmr", "head", "head-", word >> 28, 10, 144, (4800,), False),
            ("p25", "p25", "p25 inverted", 0x5575F5FF77FF, 24, 36, (4800,), False))
    pl = IM.plan(FS5, 4800)
    v = IM.crafted_plane(1500, pl, 640, [-s for s in IM.symbols(pats[0])], amp=321)
    planes, kept = _search(v, FS5, 4800, pats)
    assert [(j, m, C < 0) for j, m, C, *_ in kept if m == 640] == [(0, 640, True), (1, 640, True)] and planes[0, 640] and planes[1, 640]


@pytest.mark.parametrize("fs_ch, rate", [(19_200.0, 4800), (358_400.0, 1600), (1_075_200.0, 4800)])
def test_four_and_224_samples_to_a_symbol(A, fs_ch, rate):
    pl = IM.plan(fs_ch, rate)
    assert pl["L"] in (4, 224) and pl["o"][47] == 47 * pl["L"] and pl["o"][-16] == -16 * pl["L"]
    rng = np.random.default_rng(pl["L"] + rate)
    n = 80 * pl["L"] + 1500
    pat = IM.family(rate)[-1]
    lead, tail = list(2 * rng.integers(0, 2, 16) - 1), list(2 * rng.integers(0, 2, 16) - 1)
    v = IM.crafted_plane(n, pl, 20 * pl["L"] + 3, lead + IM.symbols(pat) + tail, first=-16, amp=(IM.V_MAX - 1000) // 3)
    v = v + rng.integers(-1000, 1000, n) * (v != 0)
    assert np.abs(v).max() <= IM.V_MAX
    planes, kept = _search(v, fs_ch, rate)
    mine = [(m, pre, post) for j, m, _, _, pre, post in kept if j == len(IM.family(rate)) - 1]
    want = sum(1 << k for k, b in enumerate(lead) if b > 0), sum(1 << k for k, b in enumerate(tail) if b > 0)
    # (under noise a plateau of 2 h samples may hold two maxima more than h apart: each is a hit of its own, with the same bits)
    assert 1 <= len(mine) <= 2 and all(0 <= m - (20 * pl["L"] + 3) < pl["L"] and (pre, post) == want for m, pre, post in mine)


def test_a_list_of_one_entry_is_never_taken_short(A, monkeypatch):
    from iq_to_audio_amd import _native

    pl = IM.plan(FS5, 4800)
    pats = IM.family(4800)
    v = IM.crafted_plane(2600, pl, 30, IM.symbols(pats[2]))
    v = IM.crafted_plane(2600, pl, 330, [-s for s in IM.symbols(pats[3])], base=v)
    v = IM.crafted_plane(2600, pl, 1500, IM.symbols(pats[2]), base=v)
    rooms = []
    real = _native.call

    def watching(name, *args):
        if name == "iqa_ident_search":
            rooms.append(args[9].value)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", watching)
    _, kept = _search(v, FS5, 4800, capacity=1)
    assert [(j, m) for j, m, *_ in kept] == [(2, 30), (2, 1500), (3, 330)] and rooms == [1, 3]
    rooms.clear()
    _search(v, FS5, 4800, capacity=3)
    assert rooms == [3]


def test_nothing_is_written_behind_the_planes_and_the_list(A):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N
    from iq_to_audio_amd import dsp_plan as P

    pl, plan = IM.plan(FS5, 4800), P.plan_ident(FS5, 4800)
    pats = IM.family(4800)
    n = 1031
    v = IM.crafted_plane(n, pl, 17, IM.symbols(pats[3]), amp=250)
    v = IM.crafted_plane(n, pl, 500, IM.symbols(pats[0]), amp=-250, base=v)
    planes, kept = IM.search(v, pl, pats)
    assert [(j, m) for j, m, *_ in kept] == [(0, 500), (3, 17)]
    table = np.zeros((5, 32), dtype=np.int8)
    for j, pat in enumerate(pats):
        table[j, : pat[4]] = IM.symbols(pat)
    score = D.from_numpy(np.full(5 * n + 64, SENTINEL, dtype=np.int32))
    lst = D.from_numpy(np.full(6 * 2 + 64, SENTINEL, dtype=np.int64))
    count = D.from_numpy(np.array([77, SENTINEL], dtype=np.int64))
    N.call("iqa_ident_search", N.ptr(D.from_numpy(v.astype(np.int32))), c_int64(n), (c_int32 * 64)(*plan.offsets), c_int32(5),
           (c_int8 * 160)(*table.reshape(-1).tolist()), (c_int32 * 5)(*[p[4] for p in pats]), c_int32(plan.half), N.ptr(score), N.ptr(lst),
           c_int64(2), N.ptr(count), N.stream_ptr())
    got = score.cpu().numpy()
    np.testing.assert_array_equal(got[: 5 * n].reshape(5, n), planes)
    assert (got[5 * n :] == SENTINEL).all() and count.cpu().numpy().tolist() == [2, SENTINEL]
    rows = lst.cpu().numpy()
    assert (rows[12:] == SENTINEL).all() and sorted(tuple(r) for r in rows[:12].reshape(2, 6).tolist()) == kept
