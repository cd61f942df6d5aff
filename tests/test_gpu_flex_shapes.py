"""The two entry points of the FLEX page decoding on the MI355X at their edge shapes, on crafted planes
(v written straight from symbol levels): the oracle's expectation is asserted first, then the kernels are held to the oracle
exactly.  Every call goes through buffers with sentinels behind them."""
from __future__ import annotations

import importlib.util
import sys
from ctypes import c_int32, c_int64, c_void_p
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


FM = _load("flex_model")
AMP = 1000
GUARD = 64
W0 = FM.codeword(0x12345)


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def gpu_frames(plane, hits, pl):
    """``iqa_flex_frames`` with sentinels behind the output: int64[K][6]."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    hits = np.asarray(hits, dtype=np.int64).reshape(-1, 2)
    k = hits.shape[0]
    out = D.from_numpy(np.full(6 * k + GUARD, -77, dtype=np.int64))
    off = (c_int32 * 112)(*[pl["o16"][i] for i in range(-16, 96)])
    v = D.from_numpy(np.asarray(plane, dtype=np.int32))
    hits_dev = D.from_numpy(hits)
    N.call("iqa_flex_frames", N.ptr(v) if v.numel() else c_void_p(0), c_int64(int(v.numel())), N.ptr(hits_dev) if k else c_void_p(0),
           c_int64(k), off, N.ptr(out), N.stream_ptr())
    got = out.cpu().numpy()
    assert (got[6 * k :] == -77).all()
    return got[: 6 * k].reshape(k, 6)


def gpu_words(plane, recs, levels, u, pl):
    """``iqa_flex_words`` with sentinels behind the three outputs."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    recs = np.asarray(recs, dtype=np.int64).reshape(-1, 4)
    f = recs.shape[0]
    count = f * 5 * 4 * 88
    fixed = D.from_numpy(np.full(count + GUARD, 0xDEADBEEF, dtype=np.uint32).view(np.int32))
    raw = D.from_numpy(np.full(count + GUARD, 0xDEADBEEF, dtype=np.uint32).view(np.int32))
    status = D.from_numpy(np.full(count + GUARD, 99, dtype=np.uint8))
    v = D.from_numpy(np.asarray(plane, dtype=np.int32))
    offs = D.from_numpy(np.asarray(pl["data"][u], dtype=np.int32))
    recs_dev = D.from_numpy(recs)
    N.call("iqa_flex_words", N.ptr(v) if v.numel() else c_void_p(0), c_int64(int(v.numel())), N.ptr(recs_dev) if f else c_void_p(0),
           c_int64(f), c_int32(levels), c_int32(u), c_int32(pl["step"][u]), N.ptr(offs), N.ptr(fixed), N.ptr(raw), N.ptr(status), N.stream_ptr())
    got = [t.cpu().numpy() for t in (fixed, raw, status)]
    assert (got[0][count:].view(np.uint32) == 0xDEADBEEF).all() and (got[1][count:].view(np.uint32) == 0xDEADBEEF).all() and (got[2][count:] == 99).all()
    shape = (f, 5, 4, 88)
    return got[0][:count].view(np.uint32).reshape(shape), got[1][:count].view(np.uint32).reshape(shape), got[2][:count].reshape(shape)


def craft(pl, mode, phases, fiw, start, n=None, centre=True):
    """(plane int64[n], m): a whole frame written straight from its levels at AMP, the first bit of the mode code (bit -16)
    beginning at sample ``start``.  m is the last sample of the marker's first bit, or (``centre``) half a data symbol in front
    of it, so that every instant lies in the middle of its symbol.  The default n ends exactly on the last data instant."""
    u = FM.SHAPE[mode][0]
    segments = FM.frame_segments(mode, fiw, phases)[32:]  # without the bit sync
    ends = np.cumsum([length for _, length in segments])
    edges = start + np.rint(np.concatenate(([0.0], ends)) * pl["sps"]).astype(np.int64)
    m = int(edges[17]) - 1 - (int(pl["sps"] / (2 * u)) if centre else 0)
    if n is None:
        n = m + pl["data"][u][-1] + 1
    v = np.zeros(n, dtype=np.int64)
    for (lev, _), a, b in zip(segments, edges[:-1], edges[1:]):
        v[max(min(a, n), 0) : max(min(b, n), 0)] = lev * AMP
    return v, m


def check(plane, rec, levels, u, pl):
    """The kernel against the oracle on one frame: (fixed, raw, status) of the oracle, [5][4][88]."""
    want = FM.words(plane, [rec], levels, u, pl)
    got = gpu_words(plane, [rec], levels, u, pl)
    for w, g, name in zip(want, got, ("fixed", "raw", "status")):
        assert g.dtype == w.dtype
        np.testing.assert_array_equal(g, w, err_msg=name)
    return want[0][0], want[1][0], want[2][0]


@pytest.mark.parametrize("fs_ch,mode", [(12_800.0, "3200/4"), (12_800.0, "1600/2"), (358_400.0, "3200/2"), (358_400.0, "1600/4")])
def test_whole_frames_at_the_ends_of_the_rate_range(A, fs_ch, mode):
    pl = FM.plan(fs_ch)
    u, levels = FM.SHAPE[mode]
    rng = np.random.default_rng(int(fs_ch) + u + levels)
    phases = {p: [FM.codeword(int(x)) for x in rng.integers(0, 1 << 21, 88)] for p in FM.ACTIVE[mode]}
    fiw = FM.codeword(FM.fiw_info(7, 100))
    plane, m = craft(pl, mode, phases, fiw, 5 * pl["o16"][1])  # the stream begins 5 bits in front of the mode code
    assert m + pl["o16"][-16] >= 0
    sent = np.array([phases.get(p, [0] * 88) for p in "ABCD"], dtype=np.uint32)
    for n in (plane.size, plane.size - 1):  # ending exactly on the last data instant, and one sample short
        v = plane[:n]
        recs = FM.frame_records(v, [(m, 1), (m, -1)], pl)
        assert recs[0].tolist() == [0, 96 * AMP, fiw, fiw, 0, 1] and recs[1, 1] == -96 * AMP
        np.testing.assert_array_equal(gpu_frames(v, [(m, 1), (m, -1)], pl), recs)
        fixed, raw, status = check(v, (m, 1, 0, 96 * AMP), levels, u, pl)
        active = ["ABCD".index(p) for p in FM.ACTIVE[mode]]
        idle = [p for p in range(4) if p not in active]
        assert (status[:, idle] == 4).all() and not fixed[:, idle].any() and not raw[:, idle].any()  # inactive phases read 0 / 0 / 4
        last_pair = [p for p in active if p // 2 == u - 1]
        if n == plane.size:
            assert (status[2, active] == 0).all() and (fixed[2] == sent).all() and (raw[2] == sent).all()
            if pl["sps"] / u >= 8:  # (at four samples to a symbol a shift of two leaves the symbol)
                assert (status[:2, active] == 0).all() and (fixed[:2] == sent).all()
            assert (status[3:, last_pair, 87] == 3).all() and (status[3:, :, :80] != 3).all()
        else:
            assert (status[2, last_pair, 87] == 3).all() and (np.delete(status[2], 87, axis=1)[active] == 0).all()
            assert not fixed[2, last_pair, 87].any() and not raw[2, last_pair, 87].any()
            assert (status[:, :, :80] != 3).all()  # status 3 in the last block only


def test_instants_in_front_of_the_stream(A):
    pl = FM.plan(12_800.0)
    mode, (u, levels) = "1600/2", FM.SHAPE["1600/2"]
    phases = {"A": [W0] * 88}
    fiw = FM.codeword(FM.fiw_info(1, 2))
    # the stream begins 5 bits in front of the marker: m + o[-16] < 0, and the record is complete
    plane, m = craft(pl, mode, phases, fiw, -11 * 8)
    assert m + pl["o16"][-16] < 0 <= m + pl["o16"][0]
    want = FM.frame_records(plane, [(m, 1)], pl)
    assert want[0].tolist() == [0, 96 * AMP, fiw, fiw, 0, 1]
    np.testing.assert_array_equal(gpu_frames(plane, [(m, 1)], pl), want)
    # a marker that begins in front of the stream, one that ends behind it, and a frame information word cut by the end
    hits = [(-1, 1), (m, 1), (plane.size - pl["o16"][31], -1), (plane.size - pl["o16"][95], 1), (plane.size - pl["o16"][95] - 1, 1)]
    want = FM.frame_records(plane, hits, pl)
    assert want[:, 5].tolist() == [0, 1, 0, 1, 1] and want[:, 4].tolist()[:4] == [3, 0, 3, 3] and want[0].tolist() == [0, 0, 0, 0, 3, 0]
    np.testing.assert_array_equal(gpu_frames(plane, hits, pl), want)
    # shifts reaching below 0: a frame whose first data instant is sample 1
    rec = (1 - pl["data"][1][0], 1, 0, 96 * AMP)
    fixed, raw, status = check(plane, rec, levels, u, pl)
    assert status[0, 0, 0] == 3 and status[1, 0, 0] != 3 and (status[0, 0, 1:] != 3).all()


def test_slicing_on_equality_and_either_side(A):
    pl = FM.plan(25_600.0)
    phases = {"A": [0] * 88, "B": [0] * 88}  # every symbol at -outer
    plane, m = craft(pl, "1600/4", phases, FM.codeword(FM.fiw_info(0, 0)), 400)
    amp = 96 * AMP
    # 3 |d| against 2 A at d = 32 y: y = 2 AMP is equality.  Bit 0 of words 0 .. 7 of block 0 are symbols 0 .. 7
    values = [2 * AMP, 2 * AMP - 1, 2 * AMP + 1, -2 * AMP, -2 * AMP + 1, -2 * AMP - 1, 0, 1]
    for q, y in enumerate(values):
        plane[m + pl["data"][1][q]] = y
    assert [FM.slice_symbol(y, 0, amp, 4) for y in values] == [(1, 0), (1, 1), (1, 0), (0, 0), (0, 1), (0, 0), (0, 1), (1, 1)]
    fixed, raw, status = check(plane, (m, 1, 0, amp), 4, 1, pl)
    assert [(int(raw[2, 0, q]) & 1, int(raw[2, 1, q]) & 1) for q in range(8)] == [(1, 0), (1, 1), (1, 0), (0, 0), (0, 1), (0, 0), (0, 1), (1, 1)]
    # a sigma that is not 0, both signs, and a frame without levels: A = 0 and A < 0 never read an inner level
    for rec in ((m, 1, 640, amp), (m, -1, -640, amp), (m, 1, 0, 0), (m, -1, 0, -amp), (m, 1, 7, 3 * 64 * AMP // 2)):
        fixed, raw, status = check(plane, rec, 4, 1, pl)
        if rec[3] <= 0:
            assert not raw[:, 1].any()
    # the records: a plane of zeros gives A = 0, the negated marker A < 0
    zeros = np.zeros(plane.size, dtype=np.int64)
    want = FM.frame_records(zeros, [(m, 1)], pl)
    assert want[0, :2].tolist() == [0, 0] and want[0, 5] == 1
    np.testing.assert_array_equal(gpu_frames(zeros, [(m, 1)], pl), want)
    want = FM.frame_records(plane, [(m, -1)], pl)
    assert want[0, 1] == -amp
    np.testing.assert_array_equal(gpu_frames(plane, [(m, -1)], pl), want)
    # the largest plane values stay exact
    big = np.where(plane > 0, 64 * 65534, -64 * 65534)
    want = FM.frame_records(big, [(m, 1), (m, -1)], pl)
    assert want[0, 1] == 32 * 64 * 65534
    np.testing.assert_array_equal(gpu_frames(big, [(m, 1), (m, -1)], pl), want)
    check(big, (m, 1, int(want[0, 0]), int(want[0, 1])), 4, 1, pl)


def test_single_errors_are_restored_and_double_errors_refused(A):
    pl = FM.plan(12_800.0)
    words = [W0 ^ (1 << w) for w in range(32)] + [W0 ^ (1 << w) ^ (1 << ((w + 5 + w // 8) % 32)) for w in range(32)]
    words += [W0] * 24
    assert all(bin(w ^ W0).count("1") == 2 for w in words[32:64])
    plane, m = craft(pl, "3200/2", {"A": words, "C": words[::-1]}, FM.codeword(FM.fiw_info(0, 1)), 100)
    fixed, raw, status = check(plane, (m, 1, 0, 96 * AMP), 2, 2, pl)
    assert raw[2, 0].tolist() == words and raw[2, 2].tolist() == words[::-1]
    assert status[2, 0].tolist() == [1] * 32 + [2] * 32 + [0] * 24 and fixed[2, 0].tolist() == [W0] * 32 + words[32:64] + [W0] * 24
    assert status[2, 2].tolist() == status[2, 0].tolist()[::-1]
    # the frame information word: one bit restored, two refused
    for bad, st in ((1 << 5, 1), (0b11 << 9, 2)):
        fiw = FM.codeword(FM.fiw_info(0, 1)) ^ bad
        plane, m = craft(pl, "1600/2", {"A": words}, fiw, 100)
        want = FM.frame_records(plane, [(m, 1)], pl)
        assert want[0, 2:].tolist() == [fiw, fiw ^ bad if st == 1 else fiw, st, 1]
        np.testing.assert_array_equal(gpu_frames(plane, [(m, 1)], pl), want)


def test_nothing_to_do(A):
    from iq_to_audio_amd import _native as N
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd import flex as X

    pl = FM.plan(25_600.0)
    plane = np.zeros(1000, dtype=np.int64)
    assert gpu_frames(plane, np.zeros((0, 2)), pl).shape == (0, 6)  # K = 0: the sentinels stay
    assert gpu_frames(np.zeros(0), [(5, 1)], pl).tolist() == [[-77] * 6]  # n = 0: nothing is written
    assert gpu_words(plane, np.zeros((0, 4)), 4, 2, pl)[2].shape == (0, 5, 4, 88)
    null = c_void_p(0)
    off = (c_int32 * 112)(*P.plan_flex(25_600.0).header)
    N.call("iqa_flex_frames", null, c_int64(0), null, c_int64(3), off, null, N.stream_ptr())
    N.call("iqa_flex_words", null, c_int64(1000), null, c_int64(0), c_int32(2), c_int32(1), c_int32(2), null, null, null, null, N.stream_ptr())
    # the package's wrappers
    from iq_to_audio_amd import _dev as D

    plan = P.plan_flex(25_600.0)
    v = D.zeros(1000, "int32")
    assert X.frames(v, np.zeros((0, 2), dtype=np.int64), plan).shape == (0, 6)
    assert [a.shape for a in X.words(v, np.zeros((0, 4), dtype=np.int64), 4, 2, plan)] == [(0, 5, 4, 88)] * 3
