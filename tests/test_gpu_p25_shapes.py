"""``iqa_p25_slice``, ``iqa_p25_nid`` and ``iqa_p25_decode`` on the MI355X at their edge shapes, on crafted
planes and words, against the numpy oracle of tests/p25_model.py: 4, 224 and 20.125 samples to a symbol, a plane that ends on
the last instant and one sample short, ``valid`` on either side of what the NID and the levels need, hits in front of and far
outside the plane, the slicing threshold on equality and one either side of it for both signs, d = 0, A = 0 and A < 0, a DC
under everything, the largest plane values, status symbols of every value, the host test's coder cases, every DUID class in
one call, K = 0 and n = 0, K = 1 and 257; every output lies in a buffer with sentinels behind it.  Every comparison is of
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


PM = _load("p25_model")
IM = PM.IM
SENTINEL, TAIL = 0x5A5A5A5A, 64
V_MAX = 64 * 65534


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
    """``iqa_p25_slice`` straight through the binding, the outputs in guarded buffers: (bits uint32[K][54], levels int64[K][3])."""
    import torch

    N = A.native
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    k = rows.shape[0]
    plane = torch.from_numpy(np.asarray(v, dtype=np.int32)).cuda()
    hits = torch.from_numpy(rows).cuda()
    (bits, fb), (levels, fl) = _guarded(torch, 54 * k, torch.int32), _guarded(torch, 3 * k, torch.int64)
    offsets = (c_int32 * 864)(*pl["o"])
    N.call("iqa_p25_slice", N.ptr(plane), c_int64(plane.numel()), N.ptr(hits), c_int64(k), offsets, N.ptr(bits), N.ptr(levels), N.stream_ptr())
    torch.cuda.synchronize()
    assert (bits[54 * k :] == fb).all() and (levels[3 * k :] == fl).all(), "a sentinel behind an output was overwritten"
    return bits[: 54 * k].cpu().numpy().view(np.uint32).reshape(k, 54), levels[: 3 * k].cpu().numpy().reshape(k, 3)


def _nid(A, words):
    """``iqa_p25_nid`` straight through the binding, the output in a guarded buffer: int32[K][4]."""
    import torch

    N = A.native
    words = np.asarray(words, dtype=np.uint32).reshape(-1, 54)
    k = words.shape[0]
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    nid, fn = _guarded(torch, 4 * k, torch.int32)
    N.call("iqa_p25_nid", N.ptr(bits), c_int64(k), N.ptr(nid), N.stream_ptr())
    torch.cuda.synchronize()
    assert (nid[4 * k :] == fn).all(), "a sentinel behind an output was overwritten"
    return nid[: 4 * k].cpu().numpy().reshape(k, 4)


def _decode(A, words, duids):
    """``iqa_p25_decode`` straight through the binding, the outputs in guarded buffers: (info uint32[K][9], rec int32[K][8])."""
    import torch

    N = A.native
    words = np.asarray(words, dtype=np.uint32).reshape(-1, 54)
    k = words.shape[0]
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    duids_dev = torch.from_numpy(np.asarray(duids, dtype=np.uint8)).cuda()
    (info, fi), (rec, fr) = _guarded(torch, 9 * k, torch.int32), _guarded(torch, 8 * k, torch.int32)
    N.call("iqa_p25_decode", N.ptr(bits), N.ptr(duids_dev), c_int64(k), N.ptr(info), N.ptr(rec), N.stream_ptr())
    torch.cuda.synchronize()
    assert (info[9 * k :] == fi).all() and (rec[8 * k :] == fr).all(), "a sentinel behind an output was overwritten"
    return info[: 9 * k].cpu().numpy().view(np.uint32).reshape(k, 9), rec[: 8 * k].cpu().numpy().reshape(k, 8)


def _check_slice(A, v, rows, pl, loops=True):
    """The kernel's output, held to both forms of the oracle."""
    bits, levels = _slice(A, v, rows, pl)
    want_bits, want_levels = PM.slice_all(v, rows, pl)
    np.testing.assert_array_equal(bits, want_bits)
    np.testing.assert_array_equal(levels, want_levels)
    if loops:
        for j, (m, s) in enumerate(np.asarray(rows).reshape(-1, 2).tolist()):
            w, lev = PM.slice_by_loops(v, len(v), m, s, pl)
            assert bits[j].tolist() == w and levels[j].tolist() == lev, j
    return bits, levels


def _check_coders(A, bits):
    """The NIDs and what lies behind them, held to the oracle: (nid, info, rec)."""
    nid = _nid(A, bits)
    np.testing.assert_array_equal(nid, PM.nid_all(bits))
    duids = PM.decoder_duids(nid)
    info, rec = _decode(A, bits, duids)
    want_info, want_rec = PM.decode_all(bits, duids)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rec, want_rec)
    return nid, info, rec


def _plane(pl, levels, lead=3, amp=1000, tail=1):
    """(v, m): symbol levels written straight into a plane, ``lead`` samples in front of symbol 0 and ``tail`` behind the last one's
    first; m is the first sample of sync symbol 0, so every instant m + o[i] is symbol i's first."""
    n = lead + int(round((len(levels) - 1) * pl["sps"])) + tail
    return IM.crafted_plane(n, pl["ident"], lead, levels, first=0, amp=amp), lead


def _levels(item, seed=3):
    return [PM.LEVEL[d] for d in PM.make_frame(item, PM.NAC, np.random.default_rng(seed))]


UNIT = PM.lc_hexbits(3, 1234, 5678)


@pytest.mark.parametrize("fs_ch", [19_200.0, 1_075_200.0, 96_600.0], ids=["sps4", "sps224", "sps20.125"])
def test_an_ldu1_at_the_rate_limits(A, fs_ch):
    pl = PM.plan(fs_ch)
    v, m = _plane(pl, _levels(("ldu1", UNIT)))
    last = m + pl["o"][863]
    assert len(v) == last + 1  # the plane ends on the last symbol's instant: one sample fewer cuts it
    bits, levels = _check_slice(A, v, [(m, 1)], pl)
    assert levels[0].tolist() == [286 * 3000, 0, 864]
    nid, info, rec = _check_coders(A, bits)
    assert nid[0].tolist() == [0, 0, PM.NAC << 4 | 5, 1] and rec[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert PM.info_hexbits(info[0]) == UNIT and PM.rs_check(PM.info_hexbits(info[0]))
    short_bits, short_levels = _check_slice(A, v[:last], [(m, 1)], pl)
    assert short_levels[0].tolist() == [286 * 3000, 0, 863] and short_bits[0, :53].tolist() == bits[0, :53].tolist()
    assert short_bits[0, 53] == bits[0, 53] & 0xFFFFFFFC  # symbol 863 alone reads 0
    # the same frame negated is the same frame at s = -1
    neg_bits, neg_levels = _check_slice(A, -v, [(m, -1)], pl, loops=False)
    np.testing.assert_array_equal(neg_bits, bits)
    assert neg_levels[0].tolist() == [286 * 3000, 0, 864]


def test_valid_on_either_side_of_what_is_needed(A):
    pl = PM.plan(25_000.0)  # sps 5.208...
    v, m = _plane(pl, _levels(("tdu",)), lead=0)
    o = pl["o"]
    planes = {valid: v[: m + o[valid - 1] + 1] for valid in (57, 56, 24, 23)}
    got = {}
    for valid, plane in planes.items():
        bits, levels = _check_slice(A, plane, [(m, 1)], pl)
        assert levels[0, 2] == valid
        got[valid] = (bits, levels, _nid(A, bits))
        np.testing.assert_array_equal(got[valid][2], PM.nid_all(bits))
    assert got[57][2][0].tolist() == [0, 0, PM.NAC << 4 | 3, 1] and PM.apply_flags(got[57][2], got[57][1])[0, 0] == 0
    assert PM.apply_flags(got[56][2], got[56][1])[0, 0] == 3 and A.p25.apply_flags(got[56][2], got[56][1])[0, 0] == 3
    assert got[56][2][0, 0] == 1 and got[56][2][0, 3] == 1  # the last NID symbol reads 00: one bit off, and the parity bit
    assert got[24][1][0].tolist() == [286 * 3000, 0, 24] and got[24][0][0, 1] >> 16 == PM.SYNC & 0xFFFF and not got[24][0][0, 2:].any()
    assert got[23][1][0].tolist() == [0, 0, 23] and not got[23][0].any()
    # hits in front of the plane and far outside
    n = len(v)
    rows = [(-1, 1), (-5000, -1), (n + 5000, 1), (n - 1, 1), (n, -1), (m, 1)]
    bits, levels = _check_slice(A, v, rows, pl)
    assert levels[:, 2].tolist() == [0, 0, 0, 1, 0, 72] and not bits[:5].any() and not levels[:5, :2].any()


def test_thresholds_and_levels(A):
    pl = PM.plan(48_000.0)  # sps 10
    a = 1000
    sync = PM.sync_levels()
    # the sync word at +-3 a: A = 286 * 3 a, Dc = 0, so d = 286 y and the second bit is (|y| >= 2 a)
    probes = [2 * a, 2 * a - 1, 2 * a + 1, -2 * a, -2 * a + 1, -2 * a - 1, 0, 1, -1, 3 * a, -3 * a, a, -a]
    values = [s * a for s in sync] + probes + [0] * (864 - 24 - len(probes))

    def plane_of(vals):
        return IM.crafted_plane(9000, pl["ident"], 100, vals, first=0, amp=1)

    def two(words, count=13, first=24):
        bits = PM.record_bits(words)
        return [(bits[2 * (first + j)], bits[2 * (first + j) + 1]) for j in range(count)]

    v = plane_of(values)
    bits, lev = _check_slice(A, v, [(100, 1), (100, -1)], pl)
    assert lev[0].tolist() == [286 * 3 * a, 0, 864] and lev[1].tolist() == [-286 * 3 * a, 0, 864]
    want = [(0, 1), (0, 0), (0, 1), (1, 1), (1, 0), (1, 1), (0, 0), (0, 0), (1, 0), (0, 1), (1, 1), (0, 0), (1, 0)]
    assert two(bits[0]) == want
    # A < 0 (the word read with the wrong sign): every second bit is set, and the first bits are those of -y
    assert all(b == 1 for _, b in two(bits[1], 864, 0))
    assert [f for f, _ in two(bits[1])] == [1, 1, 1, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0]
    # the negated plane at s = -1 reads as the plane at s = +1: equality and either side of it in the other sign
    neg_bits, neg_lev = _check_slice(A, -v, [(100, -1)], pl)
    assert two(neg_bits[0]) == want and neg_lev[0].tolist() == [286 * 3 * a, 0, 864]
    # A = 0: a plane that is 0 under the sync word
    flat = plane_of([0] * 24 + probes + [0] * (840 - len(probes)))
    bits0, lev0 = _check_slice(A, flat, [(100, 1), (100, -1)], pl)
    assert lev0[:, :2].tolist() == [[0, 0], [0, 0]] and all(b == 1 for _, b in two(bits0[0], 864, 0))
    # a DC under everything: Dc takes it out
    dc = plane_of([x + 777 for x in values])
    bits_dc, lev_dc = _check_slice(A, dc, [(100, 1)], pl)
    assert lev_dc[0].tolist() == [286 * 3 * a, 286 * 777, 864]
    np.testing.assert_array_equal(bits_dc[0], bits[0])
    # the largest plane values, in the sync word and behind it
    big = plane_of([s // 3 * V_MAX for s in sync] + [V_MAX if j % 3 else -V_MAX for j in range(840)])
    bits_big, lev_big = _check_slice(A, big, [(100, 1), (100, -1)], pl)
    assert lev_big[0].tolist() == [286 * V_MAX, 0, 864] and lev_big[1, 0] == -286 * V_MAX
    assert two(bits_big[0], 6) == [(1, 1), (0, 1), (0, 1), (1, 1), (0, 1), (0, 1)]
    big_dc = plane_of([V_MAX] * 24 + [-V_MAX] * 840)  # Dc = 286 V_MAX - 2 * 12 ... : the widest d
    _check_slice(A, big_dc, [(100, 1), (100, -1)], pl)


def test_status_symbols_of_every_value(A):
    pl = PM.plan(48_000.0)
    levels = _levels(PM.TSBK_THREE)
    inverse = {v: k for k, v in PM.LEVEL.items()}
    for k, i in enumerate(range(35, len(levels), 36)):
        levels[i] = PM.LEVEL[k % 4]
    v, m = _plane(pl, levels + [1] * (864 - len(levels)))
    bits, lev = _check_slice(A, v, [(m, 1)], pl)
    rec_bits = PM.record_bits(bits[0])
    assert [rec_bits[2 * i] << 1 | rec_bits[2 * i + 1] for i in range(35, 360, 36)] == [k % 4 for k in range(10)]  # sliced like the rest
    assert [inverse[x] for x in levels] == [rec_bits[2 * i] << 1 | rec_bits[2 * i + 1] for i in range(360)]
    nid, info, rec = _check_coders(A, bits)  # and skipped by every reader
    assert nid[0].tolist() == [0, 0, PM.NAC << 4 | 7, 1] and rec[0].tolist() == [3, 0, 0, 0, 0, 0, 0, 0]
    assert [PM.info_bytes(info[0][3 * b : 3 * b + 3]) for b in range(3)] == PM.TSBK_THREE[1]


def test_every_duid_class_in_one_call(A):
    pl = PM.plan(48_000.0)
    script = [("ldu1", UNIT), ("tdulc", PM.LC), PM.TSBK_THREE, ("hdu",), ("tdu",), ("ldu2",), PM.TSBK_ONE, ("raw", 0xC, [1, 0] * 50, 144), ("raw", 0x9, [], 72)]
    frames = [_levels(item, seed=j) for j, item in enumerate(script)]
    levels = [x for f in frames for x in f] + [1] * 864
    starts = np.cumsum([0] + [len(f) for f in frames])[:-1]
    v, m = _plane(pl, levels)
    rows = [(m + pl["o"][0] + int(round(int(at) * pl["sps"])), 1) for at in starts]
    bits, lev = _check_slice(A, v, rows, pl, loops=False)
    assert (lev[:, 0] == 286 * 3000).all() and (lev[:, 2] == 864).all()
    nid, info, rec = _check_coders(A, bits)
    assert (nid[:, 0] == 0).all() and (nid[:, 2] & 15).tolist() == [0x5, 0xF, 0x7, 0x0, 0x3, 0xA, 0x7, 0xC, 0x9] and (nid[:, 2] >> 4 == PM.NAC).all()
    assert rec[:, 0].tolist() == [1, 2, 3, 0, 0, 0, 3, 0, 0] and not rec[:3, 1:].any() and not info[[3, 4, 5, 7, 8]].any()
    assert PM.info_hexbits(info[0]) == UNIT and PM.info_hexbits(info[1]) == PM.LC and PM.info_bytes(info[6][:3]) == PM.TSBK_ONE[1][0]
    # the package's wrappers give the same
    import torch

    plan = A.plan_p25(48_000.0)
    x_bits, x_lev = A.p25.slice_frames(torch.from_numpy(np.asarray(v, dtype=np.int32)).cuda(), rows, plan)
    np.testing.assert_array_equal(x_bits, bits)
    np.testing.assert_array_equal(x_lev, lev)
    x_nid = A.p25.decode_nids(x_bits)
    np.testing.assert_array_equal(x_nid, nid)
    x_info, x_rec = A.p25.decode_frames(x_bits, A.p25.decoder_duids(x_nid))
    np.testing.assert_array_equal(x_info, info)
    np.testing.assert_array_equal(x_rec, rec)


def test_the_coder_cases_of_the_host_test(A):
    cases = PM.nid_cases()
    names = list(cases)
    words = [cases[n] for n in names]
    want = PM.nid_all(words)
    # the oracle's expectation (tests/test_p25_host.py holds every case; here the kinds of outcome are all there)
    assert sorted(set(want[:, 0].tolist())) == [0, 1, 2] and want[:, 1].max() == 12 and sorted(set(want[:, 3].tolist())) == [0, 1] and len(names) > 68
    nid = _nid(A, words)
    for j, name in enumerate(names):
        assert nid[j].tolist() == want[j].tolist(), name
    cases = PM.coder_cases()
    names = list(cases)
    words, duids = [cases[n][0] for n in names], [cases[n][1] for n in names]
    want_info, want_rec = PM.decode_all(words, duids)
    assert sorted(set(want_rec[:, 0].tolist())) == [0, 1, 2, 3] and want_rec[names.index("golay-four"), 2] == 1 and len(names) > 60
    assert want_rec[names.index("unmatched-1001"), 2] == 1 and want_rec[names.index("trellis-tie")].tolist()[:4] == [3, 3, 0, 0]
    info, rec = _decode(A, words, duids)
    for j, name in enumerate(names):
        assert rec[j].tolist() == want_rec[j].tolist() and info[j].tolist() == want_info[j].tolist(), name


def test_one_frame_and_more_frames_than_a_workgroup_has_threads(A):
    pl = PM.plan(19_200.0)
    v, m = _plane(pl, _levels(PM.TSBK_THREE) + [1] * 504)
    for k in (1, 257):
        rows = [(m + (j % 7) - 3 if j else m, 1 if j % 3 else -1 if j else 1) for j in range(k)]
        bits, lev = _check_slice(A, v, rows, pl, loops=False)
        nid, info, rec = _check_coders(A, bits)
        assert nid[0].tolist() == [0, 0, PM.NAC << 4 | 7, 1] and rec[0].tolist() == [3, 0, 0, 0, 0, 0, 0, 0] and len(rec) == k
    cases = PM.coder_cases()
    names = list(cases)
    words, duids = [cases[names[j % len(names)]][0] for j in range(257)], [cases[names[j % len(names)]][1] for j in range(257)]
    info, rec = _decode(A, words, duids)
    want_info, want_rec = PM.decode_all(words[: len(names)], duids[: len(names)])
    np.testing.assert_array_equal(info, np.concatenate([want_info] * 5)[:257])
    np.testing.assert_array_equal(rec, np.concatenate([want_rec] * 5)[:257])


def test_nothing_to_do(A):
    import torch

    pl = A.plan_p25(48_000.0)
    empty = torch.empty(0, dtype=torch.int32, device="cuda")
    bits, lev = A.p25.slice_frames(empty, [(10, 1)], pl)
    assert bits.shape == (1, 54) and lev.shape == (1, 3) and not bits.any() and not lev.any()
    plane = torch.zeros(100, dtype=torch.int32, device="cuda")
    bits, lev = A.p25.slice_frames(plane, np.zeros((0, 2), dtype=np.int64), pl)
    assert bits.shape == (0, 54) and lev.shape == (0, 3)
    assert A.p25.decode_nids(np.zeros((0, 54), dtype=np.uint32)).shape == (0, 4)
    info, rec = A.p25.decode_frames(np.zeros((0, 54), dtype=np.uint32), [])
    assert info.shape == (0, 9) and rec.shape == (0, 8)
