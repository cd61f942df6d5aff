"""``iqa_ysf_slice``, ``iqa_ysf_fich`` and ``iqa_ysf_decode`` on the MI355X at their edge shapes, on crafted
planes and words, against the model of tests/ysf_model.py: a header frame at 4, 224 and 20.125 samples to a symbol, ``valid`` one
short of and at 20, 120 and 480, hits in front of and outside the plane, the slicing threshold on equality and one either side
of it for both signs, a DC under everything, the largest plane values, K = 1, 3, 4, 5 and 261 (a partial last wave of trellises,
more frames than a workgroup has threads), every class in one call, a FICH with Golay words at distance 0, 3 and 4, a burst on
which the tie rule matters, K = 0 and n = 0; every output lies in a buffer with sentinels behind it.  Every comparison is of
integers and exact."""
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


YM = _load("ysf_model")
IM = YM.IM
SENTINEL, TAIL = 0x5A5A5A5A, 64
V_MAX = 64 * 65534
S = YM.SCALE


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _guarded(torch, count, dtype):
    fill = SENTINEL if dtype == torch.int32 else SENTINEL << 32 | SENTINEL
    return torch.full((count + TAIL,), fill, dtype=dtype, device="cuda"), fill


def _slice(A, v, rows, pl):
    """``iqa_ysf_slice`` straight through the binding, the outputs in guarded buffers: (bits uint32[K][30], levels int64[K][3])."""
    import torch

    N = A.native
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    k = rows.shape[0]
    plane = torch.from_numpy(np.asarray(v, dtype=np.int32)).cuda()
    hits = torch.from_numpy(rows).cuda()
    (bits, fb), (levels, fl) = _guarded(torch, 30 * k, torch.int32), _guarded(torch, 3 * k, torch.int64)
    offsets = (c_int32 * 480)(*pl["o"])
    N.call("iqa_ysf_slice", N.ptr(plane), c_int64(plane.numel()), N.ptr(hits), c_int64(k), offsets, N.ptr(bits), N.ptr(levels), N.stream_ptr())
    torch.cuda.synchronize()
    assert (bits[30 * k :] == fb).all() and (levels[3 * k :] == fl).all(), "a sentinel behind an output was overwritten"
    return bits[: 30 * k].cpu().numpy().view(np.uint32).reshape(k, 30), levels[: 3 * k].cpu().numpy().reshape(k, 3)


def _fich(A, words):
    """``iqa_ysf_fich`` straight through the binding, the outputs in guarded buffers: (fich uint32[K][2], rec int32[K][5])."""
    import torch

    N = A.native
    words = np.asarray(words, dtype=np.uint32).reshape(-1, 30)
    k = words.shape[0]
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    (fich, ff), (rec, fr) = _guarded(torch, 2 * k, torch.int32), _guarded(torch, 5 * k, torch.int32)
    N.call("iqa_ysf_fich", N.ptr(bits), c_int64(k), N.ptr(fich), N.ptr(rec), N.stream_ptr())
    torch.cuda.synchronize()
    assert (fich[2 * k :] == ff).all() and (rec[5 * k :] == fr).all(), "a sentinel behind an output was overwritten"
    return fich[: 2 * k].cpu().numpy().view(np.uint32).reshape(k, 2), rec[: 5 * k].cpu().numpy().reshape(k, 5)


def _decode(A, words, classes):
    """``iqa_ysf_decode`` straight through the binding, the outputs in guarded buffers: (info uint32[K][12], rec int32[K][4])."""
    import torch

    N = A.native
    words = np.asarray(words, dtype=np.uint32).reshape(-1, 30)
    k = words.shape[0]
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    classes_dev = torch.from_numpy(np.asarray(classes, dtype=np.uint8)).cuda()
    (info, fi), (rec, fr) = _guarded(torch, 12 * k, torch.int32), _guarded(torch, 4 * k, torch.int32)
    N.call("iqa_ysf_decode", N.ptr(bits), N.ptr(classes_dev), c_int64(k), N.ptr(info), N.ptr(rec), N.stream_ptr())
    torch.cuda.synchronize()
    assert (info[12 * k :] == fi).all() and (rec[4 * k :] == fr).all(), "a sentinel behind an output was overwritten"
    return info[: 12 * k].cpu().numpy().view(np.uint32).reshape(k, 12), rec[: 4 * k].cpu().numpy().reshape(k, 4)


def _check_slice(A, v, rows, pl):
    bits, levels = _slice(A, v, rows, pl)
    want_bits, want_levels = YM.slice_all(v, rows, pl)
    np.testing.assert_array_equal(bits, want_bits)
    np.testing.assert_array_equal(levels, want_levels)
    return bits, levels


def _check_coders(A, bits, classes=None):
    """The FICHs and what lies behind them, held to the model: (fich, frec, info, rec)."""
    fich, frec = _fich(A, bits)
    want_fich, want_frec = YM.fich_all(bits)
    np.testing.assert_array_equal(fich, want_fich)
    np.testing.assert_array_equal(frec, want_frec)
    if classes is None:
        classes = [YM.frame_class(YM.word_bytes(two)) if YM.fich_ok(two) else 0 for two in fich.tolist()]
    info, rec = _decode(A, bits, classes)
    want_info, want_rec = YM.decode_all(bits, classes)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rec, want_rec)
    return fich, frec, info, rec


def _plane(pl, levels, lead=3, amp=1000, tail=1):
    """(v, m): symbol levels written straight into a plane, ``lead`` samples in front of symbol 0 and ``tail`` behind the last one's
    first; m is the first sample of sync symbol 0, so every instant m + o[i] is symbol i's first."""
    n = lead + int(round((len(levels) - 1) * pl["sps"])) + tail
    return IM.crafted_plane(n, pl["ident"], lead, levels, first=0, amp=amp), lead


def _levels(item, seed=3):
    return [YM.LEVEL[d] for d in YM.make_frame(item, np.random.default_rng(seed))]


HEADER_BYTES = [YM.CS["dst"] + YM.CS["src"], YM.CS["downlink"] + YM.CS["uplink"]]


def _blocks(info_row, cls):
    """The data bytes less the whitening of the blocks of one frame's information words, and whether each CRC holds."""
    out = []
    size = 10 if cls == 3 else 20
    for second in ((0, 1) if cls == 1 else (0,) if cls else ()):
        by = YM.word_bytes(info_row[6 * second : 6 * second + 6])
        out.append((YM.whiten(by[:size]), YM.crc16(by[:size]) == (by[size] << 8 | by[size + 1])))
    return out


@pytest.mark.parametrize("fs_ch", [19_200.0, 1_075_200.0, 96_600.0], ids=["sps4", "sps224", "sps20.125"])
def test_a_header_at_the_rate_limits(A, fs_ch):
    pl = YM.plan(fs_ch)
    v, m = _plane(pl, _levels(YM.header()))
    last = m + pl["o"][479]
    assert len(v) == last + 1  # the plane ends on the last symbol's instant: one sample fewer cuts it
    bits, levels = _check_slice(A, v, [(m, 1)], pl)
    assert levels[0].tolist() == [S * 3000, 0, 480]
    fich, frec, info, rec = _check_coders(A, bits)
    assert YM.word_bytes(fich[0])[:4] == YM.header()[0] and YM.fich_ok(fich[0]) and frec[0].tolist() == [0, 0, 0, 0, 0]
    assert rec[0].tolist() == [1, 0, 0, 0] and _blocks(info[0], 1) == [(HEADER_BYTES[0], True), (HEADER_BYTES[1], True)]
    short_bits, short_levels = _check_slice(A, v[:last], [(m, 1)], pl)
    assert short_levels[0].tolist() == [S * 3000, 0, 479] and short_bits[0, :29].tolist() == bits[0, :29].tolist()
    assert short_bits[0, 29] == bits[0, 29] & 0xFFFFFFFC  # symbol 479 alone reads 0
    # the same frame negated is the same frame at s = -1
    neg_bits, neg_levels = _check_slice(A, -v, [(m, -1)], pl)
    np.testing.assert_array_equal(neg_bits, bits)
    assert neg_levels[0].tolist() == [S * 3000, 0, 480]


def test_valid_on_either_side_of_what_is_needed(A):
    pl = YM.plan(25_000.0)  # sps 5.208...
    v, m = _plane(pl, _levels(YM.header()), lead=0)
    o = pl["o"]
    got = {}
    for valid in (480, 479, 120, 119, 20, 19):
        bits, levels = _check_slice(A, v[: m + o[valid - 1] + 1], [(m, 1)], pl)
        assert levels[0, 2] == valid
        got[valid] = (bits, levels) + _check_coders(A, bits)[:2]
    for valid in (480, 479, 120):  # the FICH is whole
        assert YM.fich_ok(got[valid][2][0]) and got[valid][3][0].tolist() == [0, 0, 0, 0, 0]
        assert YM.apply_flags(got[valid][3], got[valid][1])[0, 0] == 0 and A.ysf.apply_flags(got[valid][3], got[valid][1])[0, 0] == 0
    assert YM.apply_flags(got[119][3], got[119][1])[0, 0] == 3 and A.ysf.apply_flags(got[119][3], got[119][1])[0, 0] == 3
    assert YM.decoder_classes(got[480][2], got[480][3], got[480][1]) == [1] and YM.decoder_classes(got[479][2], got[479][3], got[479][1]) == [0]
    assert A.ysf.decoder_classes(got[480][2], got[480][3], got[480][1]).tolist() == [1]
    assert A.ysf.decoder_classes(got[479][2], got[479][3], got[479][1]).tolist() == [0]
    assert got[20][1][0].tolist() == [S * 3000, 0, 20] and got[20][0][0, 0] == YM.SYNC >> 8 and got[20][0][0, 1] == (YM.SYNC & 0xFF) << 24
    assert not got[20][0][0, 2:].any()
    assert got[19][1][0].tolist() == [0, 0, 19] and not got[19][0].any()
    # hits in front of the plane and far outside
    n = len(v)
    rows = [(-1, 1), (-5000, -1), (n + 5000, 1), (n - 1, 1), (n, -1), (m, 1)]
    bits, levels = _check_slice(A, v, rows, pl)
    assert levels[:, 2].tolist() == [0, 0, 0, 1, 0, 480] and not bits[:5].any() and not levels[:5, :2].any()


def test_thresholds_and_levels(A):
    pl = YM.plan(48_000.0)  # sps 10
    a = 1000
    sync = YM.sync_levels()
    # the sync word at a s_i: A = 584 * 3 a, Dc = 0, so d = 584 y and the second bit is (|y| >= 2 a)
    probes = [2 * a, 2 * a - 1, 2 * a + 1, -2 * a, -2 * a + 1, -2 * a - 1, 0, 1, -1, 3 * a, -3 * a, a, -a]
    values = [s * a for s in sync] + probes + [0] * (480 - 20 - len(probes))

    def plane_of(vals):
        return IM.crafted_plane(5000, pl["ident"], 100, vals, first=0, amp=1)

    def two(words, count=13, first=20):
        bits = YM.record_bits(words)
        return [(bits[2 * (first + j)], bits[2 * (first + j) + 1]) for j in range(count)]

    v = plane_of(values)
    bits, lev = _check_slice(A, v, [(100, 1), (100, -1)], pl)
    assert lev[0].tolist() == [S * 3 * a, 0, 480] and lev[1].tolist() == [-S * 3 * a, 0, 480]
    want = [(0, 1), (0, 0), (0, 1), (1, 1), (1, 0), (1, 1), (0, 0), (0, 0), (1, 0), (0, 1), (1, 1), (0, 0), (1, 0)]
    assert two(bits[0]) == want
    assert [YM.DIBIT[s] for s in sync] == [f << 1 | g for f, g in two(bits[0], 20, 0)]  # the word's own inner and outer symbols
    # A < 0 (the word read with the wrong sign): every second bit is set
    assert all(b == 1 for _, b in two(bits[1], 480, 0))
    # the negated plane at s = -1 reads as the plane at s = +1: equality and either side of it in the other sign
    neg_bits, neg_lev = _check_slice(A, -v, [(100, -1)], pl)
    assert two(neg_bits[0]) == want and neg_lev[0].tolist() == [S * 3 * a, 0, 480]
    # a DC under everything: Dc takes it out, so the thresholds sit at Dc +- 2 a on both sides of Dc
    dc = plane_of([x + 777 for x in values])
    bits_dc, lev_dc = _check_slice(A, dc, [(100, 1)], pl)
    assert lev_dc[0].tolist() == [S * 3 * a, S * 777, 480]
    np.testing.assert_array_equal(bits_dc[0], bits[0])
    bits_dc, lev_dc = _check_slice(A, plane_of([x - 123_456 for x in values]), [(100, 1)], pl)
    assert lev_dc[0].tolist() == [S * 3 * a, -S * 123_456, 480]
    np.testing.assert_array_equal(bits_dc[0], bits[0])
    # A = 0: a plane that is 0 under the sync word
    flat = plane_of([0] * 20 + probes + [0] * (460 - len(probes)))
    bits0, lev0 = _check_slice(A, flat, [(100, 1), (100, -1)], pl)
    assert lev0[:, :2].tolist() == [[0, 0], [0, 0]] and all(b == 1 for _, b in two(bits0[0], 480, 0))
    # the largest plane values, in the sync word and behind it: 15 Q reaches 15 * 124 / 3 * V_MAX
    big = plane_of([s * V_MAX // 3 if abs(s) == 3 else s * (V_MAX // 3) for s in sync] + [V_MAX if j % 3 else -V_MAX for j in range(460)])
    bits_big, lev_big = _check_slice(A, big, [(100, 1), (100, -1)], pl)
    assert lev_big[0, 0] == -lev_big[1, 0] and abs(int(lev_big[0, 0]) - S * V_MAX) < S * 3 and abs(int(lev_big[0, 1])) < S * 3
    assert two(bits_big[0], 6) == [(1, 1), (0, 1), (0, 1), (1, 1), (0, 1), (0, 1)]
    _check_slice(A, plane_of([V_MAX if s > 0 else -V_MAX for s in sync] + [-V_MAX, V_MAX] * 230), [(100, 1), (100, -1)], pl)
    _check_slice(A, plane_of([V_MAX] * 20 + [-V_MAX] * 460), [(100, 1), (100, -1)], pl)


@pytest.mark.parametrize("k", [1, 3, 4, 5, 261])
def test_frame_counts_around_a_wave_of_trellises(A, k):
    pl = YM.plan(19_200.0)
    items = [YM.header(), YM.vd2(1), YM.vd1(0), YM.voice_fr(), YM.data_fr(2), YM.header(fi=2), YM.vd2(7)]
    frames = [_levels(item, seed=j) for j, item in enumerate(items)]
    v, m = _plane(pl, [x for f in frames for x in f] + [1] * 480)
    rows = [(m + int(round(480 * (j % 7) * pl["sps"])) + (0 if j < 7 else (j % 5) - 2), 1 if j < 7 or j % 3 else -1) for j in range(k)]
    bits, lev = _check_slice(A, v, rows, pl)
    fich, frec, info, rec = _check_coders(A, bits)
    assert len(rec) == k and rec[: min(k, 7), 0].tolist() == [1, 3, 2, 0, 1, 1, 3][:k] and not frec[: min(k, 7)].any()
    # every class, given and not derived, on every frame: the last of an odd K sits alone in its wave
    classes = [(j * 3 + 1) % 4 for j in range(k)]
    info, rec = _decode(A, bits, classes)
    want_info, want_rec = YM.decode_all(bits, classes)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rec, want_rec)


def test_every_class_in_one_call(A):
    pl = YM.plan(48_000.0)
    script = [YM.header(), YM.vd1(0), YM.vd2(0), YM.voice_fr(), YM.data_fr(0), YM.header(fi=2), YM.vd2(3), YM.vd1(2)]
    frames = [_levels(item, seed=j) for j, item in enumerate(script)]
    v, m = _plane(pl, [x for f in frames for x in f] + [1] * 480)
    rows = [(m + 4800 * j, 1) for j in range(len(script))]
    bits, lev = _check_slice(A, v, rows, pl)
    assert (lev[:, 0] == S * 3000).all() and (lev[:, 1] == 0).all() and (lev[:, 2] == 480).all()
    fich, frec, info, rec = _check_coders(A, bits)
    assert rec.tolist() == [[c, 0, 0, 0] for c in (1, 2, 3, 0, 1, 1, 3, 2)] and not frec.any() and not info[3].any()
    assert [YM.word_bytes(two)[:4] for two in fich.tolist()] == [item[0] for item in script]
    for j, item in enumerate(script):
        want = [(list(d), True) for d in item[1:3] if d is not None]
        assert _blocks(info[j], int(rec[j, 0])) == want, j
    assert not info[1, 6:].any() and not info[2, 3:].any()  # nothing behind the one block of classes 2 and 3
    # a class over 3 reads nothing and is reported as 0
    info, rec = _decode(A, bits[:3], [4, 200, 255])
    assert not info.any() and not rec.any()
    # the package's wrappers give the same
    import torch

    plan = A.plan_ysf(48_000.0)
    x_bits, x_lev = A.ysf.slice_frames(torch.from_numpy(np.asarray(v, dtype=np.int32)).cuda(), rows, plan)
    np.testing.assert_array_equal(x_bits, bits)
    np.testing.assert_array_equal(x_lev, lev)
    x_fich, x_frec = A.ysf.decode_fich(x_bits)
    np.testing.assert_array_equal(x_fich, fich)
    np.testing.assert_array_equal(x_frec, frec)
    classes = A.ysf.decoder_classes(x_fich, x_frec, x_lev)
    assert classes.tolist() == [1, 2, 3, 0, 1, 1, 3, 2] == YM.decoder_classes(fich, frec, lev)
    x_info, x_rec = A.ysf.decode_frames(x_bits, classes)
    want_info, want_rec = YM.decode_all(bits, classes)
    np.testing.assert_array_equal(x_info, want_info)
    np.testing.assert_array_equal(x_rec, want_rec)


def test_the_coder_cases_of_the_host_test(A):
    cases = YM.coder_cases()
    names = list(cases)
    words, classes = [cases[n][0] for n in names], [cases[n][1] for n in names]
    want_fich, want_frec = YM.fich_all(words)
    want_info, want_rec = YM.decode_all(words, [c if c <= 3 else 0 for c in classes])
    at = names.index
    # the model's expectation (tests/test_ysf_host.py holds every case; here the kinds of outcome are all there)
    assert want_frec[at("golay-0000")].tolist() == [0, 0, 0, 0, 0] and want_frec[at("golay-3333")].tolist() == [1, 0, 4, 0, 12]
    assert want_frec[at("golay-4000")].tolist() == [2, 0, 0, 1, 0] and want_frec[at("golay-0403")].tolist() == [2, 0, 1, 1, 3]
    assert want_frec[at("golay-1234")].tolist() == [2, 0, 3, 1, 6] and want_frec[at("golay-4444")][3] == 4
    assert sorted(set(want_rec[:, 0].tolist())) == [0, 1, 2, 3] and len(names) > 60
    tie = YM.decode_frame(*cases["dch-tie"])
    assert tie[2] > 0 and tie[0] != YM.decode_frame(*cases["dch-tie"], smaller=False)[0]  # an equal-metric compare on the surviving path
    fich, frec = _fich(A, words)
    info, rec = _decode(A, words, classes)
    for j, name in enumerate(names):
        assert fich[j].tolist() == want_fich[j].tolist() and frec[j].tolist() == want_frec[j].tolist(), name
        assert rec[j].tolist() == want_rec[j].tolist() and info[j].tolist() == want_info[j].tolist(), name
    assert info[at("dch-tie")].tolist() == tie[0] and rec[at("dch-tie")].tolist() == tie[1]


def test_nothing_to_do(A):
    import torch

    pl = A.plan_ysf(48_000.0)
    empty = torch.empty(0, dtype=torch.int32, device="cuda")
    bits, lev = A.ysf.slice_frames(empty, [(10, 1)], pl)
    assert bits.shape == (1, 30) and lev.shape == (1, 3) and not bits.any() and not lev.any()
    plane = torch.zeros(100, dtype=torch.int32, device="cuda")
    bits, lev = A.ysf.slice_frames(plane, np.zeros((0, 2), dtype=np.int64), pl)
    assert bits.shape == (0, 30) and lev.shape == (0, 3)
    fich, frec = A.ysf.decode_fich(np.zeros((0, 30), dtype=np.uint32))
    assert fich.shape == (0, 2) and frec.shape == (0, 5)
    info, rec = A.ysf.decode_frames(np.zeros((0, 30), dtype=np.uint32), [])
    assert info.shape == (0, 12) and rec.shape == (0, 4)
    # straight through the binding with NULL pointers: K = 0 and n = 0 touch nothing
    N = A.native
    null = N.ptr(None)
    offsets = (c_int32 * 480)(*pl.offsets)
    N.call("iqa_ysf_slice", null, c_int64(0), null, c_int64(5), offsets, null, null, N.stream_ptr())
    N.call("iqa_ysf_slice", null, c_int64(100), null, c_int64(0), offsets, null, null, N.stream_ptr())
    N.call("iqa_ysf_fich", null, c_int64(0), null, null, N.stream_ptr())
    N.call("iqa_ysf_decode", null, null, c_int64(0), null, null, N.stream_ptr())
