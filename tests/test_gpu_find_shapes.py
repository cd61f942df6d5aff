"""The six entry points of the channel finder on small hand-made integer planes against the numpy
oracle of tests/find_model.py, at their edge shapes: bin counts around the workgroup, batches that start and end inside a
slice, the quantiser's special values, windows wider than the plane, gaps of exactly gap and gap + 1, runs at the ends, the
bounded list, waves of 63, 64 and 65 bins, sums at the bound.  What the oracle must give is asserted first, so that no
equality is one of empty results."""
from __future__ import annotations

import importlib.util
import sys
from ctypes import c_int32, c_int64
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


M = _load("find_model")
TILE = 256  # FD_TILE: bins of one workgroup of the floor and mask kernels


@pytest.fixture(scope="module")
def G():
    """The entry points on numpy arrays."""
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    class Entries:
        @staticmethod
        def state(nbins, S):
            st = M.new_state(nbins, S)
            return {k: D.from_numpy(v.reshape(-1)) for k, v in st.items()}

        @staticmethod
        def accumulate(state, rows, first, T, S):
            rows = np.ascontiguousarray(rows, dtype=np.float32)
            n, nbins = rows.shape
            c, dev = D.from_numpy(np.full(n * nbins, 77, dtype=np.int16)), D.from_numpy(rows.reshape(-1))  # (held until the call is queued)
            N.call("iqa_find_accumulate", N.ptr(dev), c_int32(n), c_int32(nbins), c_int64(first), c_int32(T),
                   c_int32(S), N.ptr(state["sum"]), N.ptr(state["max"]), N.ptr(state["slice"]), N.ptr(c), N.stream_ptr())
            return c.cpu().numpy().reshape(n, nbins)

        @staticmethod
        def host(state, nbins):
            return dict(sum=state["sum"].cpu().numpy(), max=state["max"].cpu().numpy(), slice=state["slice"].cpu().numpy().reshape(-1, nbins))

        @staticmethod
        def mean(total, F):
            out, dev = D.from_numpy(np.full(total.size, 77, dtype=np.int32)), D.from_numpy(np.asarray(total, dtype=np.int64))
            N.call("iqa_find_mean", N.ptr(dev), c_int32(total.size), c_int64(F), N.ptr(out), N.stream_ptr())
            return out.cpu().numpy()

        @staticmethod
        def floor(plane, h, num, den):
            out, dev = D.from_numpy(np.full(plane.size, 77, dtype=np.int32)), D.from_numpy(np.asarray(plane, dtype=np.int32))
            N.call("iqa_find_floor", N.ptr(dev), c_int32(plane.size), c_int32(h), c_int32(num),
                   c_int32(den), N.ptr(out), N.stream_ptr())
            return out.cpu().numpy()

        @staticmethod
        def mask(mean, fmean, mx, fmax, *, thr, thr_peak, gap, dc_bin, dc_guard):
            n = mean.size
            x, mk = D.from_numpy(np.full(n, 77, dtype=np.int32)), D.from_numpy(np.full(n, 77, dtype=np.uint8))
            planes = [D.from_numpy(np.asarray(a, dtype=np.int32)) for a in (mean, fmean, mx, fmax)]
            N.call("iqa_find_mask", *(N.ptr(a) for a in planes), c_int32(n), c_int32(thr), c_int32(thr_peak), c_int32(gap), c_int32(dc_bin),
                   c_int32(dc_guard), N.ptr(x), N.ptr(mk), N.stream_ptr())
            return x.cpu().numpy(), mk.cpu().numpy()

        @staticmethod
        def runs(mean, fmean, mx, fmax, mk, min_hot, capacity):
            """(the list as written, int64[capacity + 1][8] with a guard record behind it; counts)"""
            planes = [D.from_numpy(np.asarray(a, dtype=np.int32)) for a in (mean, fmean, mx, fmax)]
            mk_dev = D.from_numpy(np.asarray(mk, dtype=np.uint8))
            lst = D.from_numpy(np.full((capacity + 1) * 8, -7, dtype=np.int64))
            counts = D.from_numpy(np.array([99, 99], dtype=np.int64))
            N.call("iqa_find_runs", *(N.ptr(a) for a in planes), N.ptr(mk_dev), c_int32(mean.size),
                   c_int32(min_hot), N.ptr(lst), c_int64(capacity), N.ptr(counts), N.stream_ptr())
            return lst.cpu().numpy().reshape(-1, 8), counts.cpu().numpy().tolist()

        @staticmethod
        def activity(slices, fmean, records, *, T, F, thr_act):
            S, nbins = slices.shape
            J = len(records)
            on = D.from_numpy(np.full(max(J * S, 1), 77, dtype=np.uint8))
            rec = D.from_numpy(np.asarray(records, dtype=np.int64).reshape(-1)) if J else None
            sl_dev, fm_dev = D.from_numpy(np.asarray(slices, dtype=np.int32).reshape(-1)), D.from_numpy(np.asarray(fmean, dtype=np.int32))
            N.call("iqa_find_activity", N.ptr(sl_dev), N.ptr(fm_dev), N.ptr(rec), c_int64(J), c_int32(nbins), c_int64(F), c_int32(T),
                   c_int32(S), c_int32(thr_act), N.ptr(on), N.stream_ptr())
            return on.cpu().numpy()[: J * S].reshape(J, S), on.cpu().numpy()

    return Entries


# ---- accumulate and mean -------------------------------------------------------------------------------------------------

SPECIAL = np.array([np.inf, -np.inf, np.nan, 300.005, -300.005, 300.0, -300.0, 299.995, 0.125, 0.375, -0.125, -0.375, 0.005, 0.015, 1e30],
                   dtype=np.float32)


@pytest.mark.parametrize("nbins", [1, 255, 256, 257])
def test_accumulate_shapes(G, nbins):
    """T = 3, F = 8: slices of 3, 3 and 2 frames.  Calls of 1 frame, of 4 frames from frame 1 (starts inside slice 0, crosses
    into slice 1) and of 3 frames from frame 5 (starts inside slice 1, fills the shorter last slice)."""
    T, F, S = 3, 8, 3
    rng = np.random.default_rng(nbins)
    rows = (rng.uniform(-320.0, 320.0, size=(F, nbins))).astype(np.float32)
    flat = rows.reshape(-1)
    at = rng.permutation(flat.size)[: min(SPECIAL.size, flat.size)]
    flat[at] = SPECIAL[: at.size]
    c_want = M.quantise(rows)
    want = M.accumulate_all(c_want, T, S)
    assert c_want.min() == -30000 and c_want.max() == 30000 and np.abs(want["slice"]).min(axis=1).tolist() != [0, 0, 0]
    if nbins > 1:
        assert sorted(c_want.reshape(-1)[at].tolist()) == sorted([30000, -30000, -30000, 30000, -30000, 30000, -30000, 30000, 12, 38, -12, -38, 0, 2,
                                                                 30000][: at.size])
    state = G.state(nbins, S)
    got_c = np.concatenate([G.accumulate(state, rows[a:b], a, T, S) for a, b in ((0, 1), (1, 5), (5, 8))])
    np.testing.assert_array_equal(got_c, c_want)
    got = G.host(state, nbins)
    for key in ("sum", "max", "slice"):
        assert got[key].dtype == want[key].dtype
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    # one call of everything, and one frame per call, land on the same planes
    for cuts in ([(0, 8)], [(f, f + 1) for f in range(F)]):
        state = G.state(nbins, S)
        for a, b in cuts:
            G.accumulate(state, rows[a:b], a, T, S)
        for key, value in G.host(state, nbins).items():
            np.testing.assert_array_equal(value, want[key], err_msg=key)


def test_accumulate_max_starts_at_the_bottom_and_mean_floors(G):
    rows = np.full((2, 5), -400.0, dtype=np.float32)  # under the range: c = -30000, the maximum stays at its start value
    state = G.state(5, 1)
    G.accumulate(state, rows, 0, 2, 1)
    got = G.host(state, 5)
    assert got["max"].tolist() == [-30000] * 5 and got["sum"].tolist() == [-60000] * 5 and got["slice"].tolist() == [[-60000] * 5]
    total = np.array([-7, -8, 7, 8, 0, -1, 1, -(1 << 31) + 3, (1 << 31) - 3, -29999 * 1170 - 1], dtype=np.int64)
    for F in (1, 4, 1170):
        want = M.mean(total, F)
        assert want.tolist() == [int(v) // F for v in total.tolist()]
        np.testing.assert_array_equal(G.mean(total, F), want)
    assert M.mean(total, 4)[:2].tolist() == [-2, -2] and M.mean(total, 1170)[-1] == -30000


# ---- the local floor -----------------------------------------------------------------------------------------------------


def _plane(kind, nbins, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "constant":
        return np.full(nbins, -12345, dtype=np.int32)
    if kind == "descending":
        return (30000 - 3 * np.arange(nbins)).astype(np.int32) if nbins <= 20000 else None
    plane = rng.integers(-30000, 30001, size=nbins).astype(np.int32)
    plane[rng.integers(0, nbins, size=3)] = (-30000, 30000, 0)
    return plane


@pytest.mark.parametrize("nbins,h", [(300, 0), (300, 7), (300, 299), (300, 300), (300, 8191), (TILE - 1, 5), (TILE, 5), (TILE + 1, 5), (1, 0), (1, 8191),
                                     (3 * TILE + 17, 200)])
def test_floor_shapes(G, nbins, h):
    for kind in ("random", "constant", "descending"):
        plane = _plane(kind, nbins)
        for num, den in ((0, 1), (1, 4), (1, 1)):
            want = M.floor(plane, h, num, den)
            if h == 0:
                assert want.tolist() == plane.tolist()
            elif h >= nbins:
                assert want.tolist() == [sorted(plane.tolist())[((nbins - 1) * num) // den]] * nbins
            elif kind == "descending" and (num, den) == (0, 1):
                assert want.tolist() == [int(plane[min(nbins - 1, k + h)]) for k in range(nbins)]  # the window's minimum is its last bin
            np.testing.assert_array_equal(G.floor(plane, h, num, den), want, err_msg=f"{kind} {num}/{den}")


def test_floor_widest_window_on_a_long_plane(G):
    """h = 8191 with 20000 bins: 16383 halfwords of neighbours and a tile in LDS, 79 workgroups, clipped windows at both ends."""
    plane = _plane("random", 20_000, seed=8)
    want = M.floor(plane, 8191, 1, 4)
    assert len(set(want.tolist())) > 20 and want[0] == sorted(plane[:8192].tolist())[8191 // 4]
    np.testing.assert_array_equal(G.floor(plane, 8191, 1, 4), want)
    ramp = (30000 - 3 * np.arange(20_000)).astype(np.int32)  # all distinct, descending
    want = M.floor(ramp, 8191, 1, 4)
    assert want[10_000] == ramp[10_000 + 8191 - (2 * 8191) // 4]
    np.testing.assert_array_equal(G.floor(ramp, 8191, 1, 4), want)


# ---- the mask ------------------------------------------------------------------------------------------------------------


def _mask_planes(nbins, hot, thr=600, thr_peak=1000, by_peak=()):
    """Planes whose hot bins are exactly ``hot`` (through the mean) and ``by_peak`` (through the maximum alone)."""
    rng = np.random.default_rng(len(hot))
    fmean = rng.integers(-9000, -8000, size=nbins).astype(np.int32)
    fmax = rng.integers(-8000, -7000, size=nbins).astype(np.int32)
    mean = fmean + rng.integers(-50, thr, size=nbins).astype(np.int32)  # under the threshold by 1 at least
    mx = fmax + rng.integers(-50, thr_peak, size=nbins).astype(np.int32)
    for k in hot:
        mean[k] = fmean[k] + thr + (0 if k % 2 else 37)  # exactly at the threshold, or over it
    for k in by_peak:
        mx[k] = fmax[k] + thr_peak
    return mean, fmean, mx, fmax


@pytest.mark.parametrize("gap", [0, 1, 17, 254, 255])
def test_mask_gaps(G, gap):
    """Hot bins at 0, then behind exactly ``gap`` cold bins (closed), then behind ``gap + 1`` (left open), then the same pair of
    distances in front of the last bin: the stretches cross the workgroups' edges at 256 and 512."""
    nbins = 2 * (2 * gap + 5) + 300
    a = gap + 1
    b = a + gap + 2
    hot = [0, a, b, nbins - 1 - (gap + 1) - (gap + 2), nbins - 1 - (gap + 1), nbins - 1]
    planes = _mask_planes(nbins, hot)
    kw = dict(thr=600, thr_peak=1000, gap=gap, dc_bin=nbins // 2, dc_guard=3)
    x_want, mk_want = M.mask(*planes, **kw)
    assert np.flatnonzero(mk_want & 1).tolist() == hot
    closed = np.flatnonzero(mk_want & 2).tolist()
    assert closed == sorted(set(range(0, a + 1)) | {b, hot[3]} | set(range(hot[4], nbins)))
    x, mk = G.mask(*planes, **kw)
    np.testing.assert_array_equal(x, x_want)
    np.testing.assert_array_equal(mk, mk_want)


def test_mask_guard_and_second_term(G):
    nbins, dc = 700, 350
    hot = [0, 255, 256, 340, 347, 349, 350, 351, 353, 360, 699]
    planes = _mask_planes(nbins, hot, by_peak=(100, 352))
    for guard, live in ((-1, hot + [100, 352]), (-5, hot + [100, 352]), (0, [k for k in hot + [100, 352] if k != dc]),
                        (3, [k for k in hot + [100, 352] if abs(k - dc) > 3]), (349, [0]), (350, []), (100_000, [])):
        kw = dict(thr=600, thr_peak=1000, gap=4, dc_bin=dc, dc_guard=guard)
        x_want, mk_want = M.mask(*planes, **kw)
        assert np.flatnonzero(mk_want & 1).tolist() == sorted(live), guard
        x, mk = G.mask(*planes, **kw)
        np.testing.assert_array_equal(x, x_want)
        np.testing.assert_array_equal(mk, mk_want, err_msg=str(guard))
    # the second term alone: bins 100 and 352 are under the mean's threshold and at the maximum's
    x_want, _ = M.mask(*planes, thr=600, thr_peak=1000, gap=4, dc_bin=dc, dc_guard=-1)
    assert x_want[100] == 0 and x_want[352] == 0 and planes[0][100] - planes[1][100] < 600
    # a dc_bin outside the plane guards nothing inside it
    kw = dict(thr=600, thr_peak=1000, gap=0, dc_bin=5000, dc_guard=10)
    _, mk_want = M.mask(*planes, **kw)
    assert np.flatnonzero(mk_want & 1).tolist() == sorted(hot + [100, 352])
    np.testing.assert_array_equal(G.mask(*planes, **kw)[1], mk_want)


# ---- the runs ------------------------------------------------------------------------------------------------------------


def _run_planes(nbins, seed=2):
    rng = np.random.default_rng(seed)
    fmean = rng.integers(-9000, -8000, size=nbins).astype(np.int32)
    fmax = rng.integers(-8000, -7000, size=nbins).astype(np.int32)
    mean = fmean + rng.integers(-300, 4000, size=nbins).astype(np.int32)
    mx = fmax + rng.integers(0, 5000, size=nbins).astype(np.int32)
    return mean, fmean, mx, fmax


def _runs_equal(G, planes, mk, min_hot, capacity, kept, total):
    want, n_all = M.runs(*planes, mk, min_hot)
    assert (len(want), n_all) == (kept, total)
    lst, counts = G.runs(*planes, mk, min_hot, capacity)
    assert counts == [kept, total]
    assert (lst[capacity] == -7).all()  # nothing behind the list
    got = lst[: min(kept, capacity)]
    if kept <= capacity:
        assert (lst[kept:capacity] == -7).all()
        np.testing.assert_array_equal(got[np.argsort(got[:, 0])], want)
    else:  # a subset, each record whole and none twice
        rows = {tuple(r) for r in want.tolist()}
        assert len({tuple(r) for r in got.tolist()}) == capacity and all(tuple(r) in rows for r in got.tolist())
    return want


def test_runs_shapes(G):
    nbins = 700
    planes = _run_planes(nbins)
    none = np.zeros(nbins, dtype=np.uint8)
    _runs_equal(G, planes, none, 2, 4, 0, 0)
    whole = np.full(nbins, 3, dtype=np.uint8)  # one run covering every bin, across three workgroups
    want = _runs_equal(G, planes, whole, 2, 4, 1, 1)
    assert want[0, :3].tolist() == [0, nbins - 1, nbins]
    ends = none.copy()
    ends[[0, 1, 2]] = (1 | 2, 2, 1 | 2)
    ends[[255, 256]] = 3  # a run across the workgroups' edge
    ends[[400]] = 3  # one hot bin: a run, dropped at min_hot 2
    ends[[500, 501, 502, 503]] = (3, 2, 2, 3)
    ends[[697, 698, 699]] = (3, 3, 3)
    want = _runs_equal(G, planes, ends, 2, 8, 4, 5)
    assert want[:, :3].tolist() == [[0, 2, 2], [255, 256, 2], [500, 503, 2], [697, 699, 3]]
    want = _runs_equal(G, planes, ends, 3, 8, 1, 5)  # kept at exactly min_hot, dropped one below
    assert want[:, :3].tolist() == [[697, 699, 3]]
    _runs_equal(G, planes, ends, 1, 8, 5, 5)
    _runs_equal(G, planes, ends, 1, 5, 5, 5)  # a list that is exactly long enough
    # ties for the peak go to the lowest bin; a run whose e is negative throughout has no weight
    mean, fmean, mx, fmax = (a.copy() for a in planes)
    mean[500:504] = fmean[500:504] + np.array([5, 900, 900, 900])
    mean[697:700] = fmean[697:700] - np.array([3, 1, 1])
    want = _runs_equal(G, (mean, fmean, mx, fmax), ends, 2, 8, 4, 5)
    assert want[2, 3:7].tolist() == [501, 900, 2705, 900 * (1 + 2 + 3)] and want[3, 3:7].tolist() == [698, -1, 0, 0]


def test_runs_more_than_the_list_holds(G):
    nbins = 300 * 3
    planes = _run_planes(nbins, seed=4)
    mk = np.zeros(nbins, dtype=np.uint8)
    mk[0::3] = 3
    mk[1::3] = 3  # 300 runs of two hot bins
    _runs_equal(G, planes, mk, 2, 256, 300, 300)
    _runs_equal(G, planes, mk, 2, 300, 300, 300)
    _runs_equal(G, planes, mk, 3, 256, 0, 300)


# ---- the activity --------------------------------------------------------------------------------------------------------


def _at_the_bound(fmean, records, lens, thr_act, below):
    """Slices in which every run's sum equals its bound exactly; where ``below[j][s]``, one bin of run j is one lower."""
    slices = np.stack([Ts * (fmean.astype(np.int64) + thr_act) for Ts in lens])
    for j, (lo, hi) in enumerate(records):
        for s in range(len(lens)):
            if below[j][s]:
                slices[s, lo + (hi - lo) // 2] -= 1
    return slices.astype(np.int32)


def test_activity_shapes(G):
    nbins, T, F, thr_act = 1300, 3, 11, 300
    lens = [3, 3, 3, 2]
    fmean = np.random.default_rng(3).integers(-9000, -8000, size=nbins).astype(np.int32)
    spans = [(0, 0), (5, 5), (10, 72), (100, 163), (200, 264), (300, 1299)]  # 1, 1, 63, 64, 65 and 1000 bins
    assert [hi - lo + 1 for lo, hi in spans] == [1, 1, 63, 64, 65, 1000]
    records = np.zeros((len(spans), 8), dtype=np.int64)
    records[:, :2] = spans
    below = [[(j + s) % 2 == 1 for s in range(4)] for j in range(len(spans))]
    slices = _at_the_bound(fmean, spans, lens, thr_act, below)
    want = M.activity(slices, fmean, records, T=T, F=F, thr_act=thr_act)
    assert want.tolist() == [[0 if below[j][s] else 1 for s in range(4)] for j in range(len(spans))]  # at the bound: on; one below: off
    got, _ = G.activity(slices, fmean, records, T=T, F=F, thr_act=thr_act)
    np.testing.assert_array_equal(got, want)
    # records in any order, and a record that is no run of this plane
    order = [4, 0, 5, 2, 1, 3]
    got, _ = G.activity(slices, fmean, records[order], T=T, F=F, thr_act=thr_act)
    np.testing.assert_array_equal(got, want[order])
    bad = records.copy()
    bad[1, :2] = (-1, 5)
    bad[3, :2] = (100, nbins)
    bad[4, :2] = (264, 200)
    got, _ = G.activity(slices, fmean, bad, T=T, F=F, thr_act=thr_act)
    keep = [0, 2, 5]
    np.testing.assert_array_equal(got[keep], want[keep])
    assert not got[[1, 3, 4]].any()
    # random slices
    rnd = (slices.astype(np.int64) + np.random.default_rng(9).integers(-40, 41, size=slices.shape)).astype(np.int32)
    want = M.activity(rnd, fmean, records, T=T, F=F, thr_act=thr_act)
    assert 0 < want.sum() < want.size
    np.testing.assert_array_equal(G.activity(rnd, fmean, records, T=T, F=F, thr_act=thr_act)[0], want)


def test_activity_one_slice_one_frame_no_run(G):
    nbins, thr_act = 200, 300
    fmean = np.random.default_rng(6).integers(-9000, -8000, size=nbins).astype(np.int32)
    spans = [(0, 63), (64, 64), (100, 199)]
    records = np.zeros((3, 8), dtype=np.int64)
    records[:, :2] = spans
    # S = 1: the whole run is one slice of 7 frames
    slices = _at_the_bound(fmean, spans, [7], thr_act, [[False], [True], [False]])
    want = M.activity(slices, fmean, records, T=7, F=7, thr_act=thr_act)
    assert want.tolist() == [[1], [0], [1]]
    np.testing.assert_array_equal(G.activity(slices, fmean, records, T=7, F=7, thr_act=thr_act)[0], want)
    # a short only slice: T = 9 but 7 frames
    want = M.activity(slices, fmean, records, T=9, F=7, thr_act=thr_act)
    assert want.tolist() == [[1], [0], [1]]
    np.testing.assert_array_equal(G.activity(slices, fmean, records, T=9, F=7, thr_act=thr_act)[0], want)
    # T_s = 1: every frame its own slice
    below = [[False, True, False], [True, False, True], [False, False, True]]
    slices = _at_the_bound(fmean, spans, [1, 1, 1], thr_act, below)
    want = M.activity(slices, fmean, records, T=1, F=3, thr_act=thr_act)
    assert want.tolist() == [[0 if b else 1 for b in row] for row in below]
    np.testing.assert_array_equal(G.activity(slices, fmean, records, T=1, F=3, thr_act=thr_act)[0], want)
    # no run: nothing is written
    got, raw = G.activity(slices, fmean, records[:0], T=1, F=3, thr_act=thr_act)
    assert got.shape == (0, 3) and raw.tolist() == [77]


def test_runs_refuse_before_they_clear_the_counters(G):
    """A call refused for a NULL plane, mask or list pointer leaves the counters, and every other buffer, as they were."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    names = ("mean", "fmean", "max", "fmax", "mask", "list")
    for missing in names:
        bufs = {k: D.from_numpy(np.full(256, -7, dtype=np.int64)) for k in names + ("counts",)}
        arg = {k: None if k == missing else v for k, v in bufs.items()}
        with pytest.raises(ValueError, match="NULL device pointer"):
            N.call("iqa_find_runs", *(N.ptr(arg[k]) for k in names[:5]), c_int32(64), c_int32(1), N.ptr(arg["list"]), c_int64(4), N.ptr(arg["counts"]),
                   N.stream_ptr())
        D.torch_mod().cuda.synchronize()
        assert all((v.cpu().numpy() == -7).all() for v in bufs.values()), missing
