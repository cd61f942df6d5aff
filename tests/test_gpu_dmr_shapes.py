"""``iqa_dmr_slice`` and ``iqa_dmr_decode`` on the MI355X at their edge shapes, on crafted planes and
words, against the numpy oracle of tests/dmr_model.py: 4 and 224 samples to a symbol, a plane that ends on the last instant
and one sample short, a CACH or a burst outside the plane, the slicing threshold on equality and one either side of it, d = 0,
A = 0 and A < 0, the largest plane values, all four kinds in one call, the host test's coder cases, K = 0 and n = 0; every
output lies in a buffer with sentinels behind it.  Every comparison is of integers and exact."""
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


DM = _load("dmr_model")
IM = DM.IM
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
    """``iqa_dmr_slice`` straight through the binding, the outputs in guarded buffers: (bits uint32[K][9], levels int64[K][3])."""
    import torch

    N = A.native
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    k = rows.shape[0]
    plane = torch.from_numpy(np.asarray(v, dtype=np.int32)).cuda()
    hits = torch.from_numpy(rows).cuda()
    (bits, fb), (levels, fl) = _guarded(torch, 9 * k, torch.int32), _guarded(torch, 3 * k, torch.int64)
    offsets = (c_int32 * 144)(*[pl["o"][i] for i in range(-66, 78)])
    N.call("iqa_dmr_slice", N.ptr(plane), c_int64(plane.numel()), N.ptr(hits), c_int64(k), offsets, N.ptr(bits), N.ptr(levels), N.stream_ptr())
    torch.cuda.synchronize()
    assert (bits[9 * k :] == fb).all() and (levels[3 * k :] == fl).all(), "a sentinel behind an output was overwritten"
    return bits[: 9 * k].cpu().numpy().view(np.uint32).reshape(k, 9), levels[: 3 * k].cpu().numpy().reshape(k, 3)


def _decode(A, words, kinds):
    """``iqa_dmr_decode`` straight through the binding, the outputs in guarded buffers: (info uint32[K][3], rec int32[K][8])."""
    import torch

    N = A.native
    words = np.asarray(words, dtype=np.uint32).reshape(-1, 9)
    k = words.shape[0]
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    kinds_dev = torch.from_numpy(np.asarray(kinds, dtype=np.uint8)).cuda()
    (info, fi), (rec, fr) = _guarded(torch, 3 * k, torch.int32), _guarded(torch, 8 * k, torch.int32)
    N.call("iqa_dmr_decode", N.ptr(bits), N.ptr(kinds_dev), c_int64(k), N.ptr(info), N.ptr(rec), N.stream_ptr())
    torch.cuda.synchronize()
    assert (info[3 * k :] == fi).all() and (rec[8 * k :] == fr).all(), "a sentinel behind an output was overwritten"
    return info[: 3 * k].cpu().numpy().view(np.uint32).reshape(k, 3), rec[: 8 * k].cpu().numpy().reshape(k, 8)


def _check_slice(A, v, rows, pl):
    """The kernel's output, held to both forms of the oracle."""
    bits, levels = _slice(A, v, rows, pl)
    want_bits, want_levels = DM.slice_all(v, rows, pl)
    np.testing.assert_array_equal(bits, want_bits)
    np.testing.assert_array_equal(levels, want_levels)
    for j, (m, s, kind) in enumerate(np.asarray(rows).reshape(-1, 3).tolist()):
        w, lev = DM.slice_by_loops(v, len(v), m, s, kind, pl)
        assert bits[j].tolist() == w and levels[j].tolist() == lev, j
    return bits, levels


HEADER = ("header", 3, 1234, 5678)


def _slot_plane(pl, script, lead=3, amp=1000, kind_levels=None):
    """(v, the m of every slot): the levels of a base station's ``script`` written straight into a plane, ``lead`` samples in
    front of the first CACH symbol; m is the first sample of sync symbol 0, so every instant m + o[i] is symbol i's first."""
    levels = DM.base_station(script) if kind_levels is None else kind_levels
    sps = pl["sps"]
    start = lead - int(round(-66 * sps))  # symbol -66 of slot 0 begins at ``lead``
    n = start + int(round((len(levels) - 66) * sps)) + 1
    v = IM.crafted_plane(n, pl["ident"], start, levels, first=-66, amp=amp)
    ms = [start + int(round(144 * j * sps)) for j in range(len(levels) // 144)]
    return v, ms


@pytest.mark.parametrize("fs_ch", [19_200.0, 1_075_200.0, 96_600.0], ids=["sps4", "sps224", "sps20.125"])
def test_a_header_at_the_rate_limits(A, fs_ch):
    pl = DM.plan(fs_ch)
    v, (m,) = _slot_plane(pl, [HEADER])
    # the plane ends on the burst's last instant: one sample fewer cuts the burst
    last = m + pl["o"][77]
    assert len(v) > last
    v = v[: last + 1]
    bits, levels = _check_slice(A, v, [(m, -1, 1)], pl)
    assert levels[0].tolist() == [0, 72_000, 3]
    info, rec = _decode(A, bits, [1])
    want_info, want_rec = DM.decode_all(bits, [1])
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rec, want_rec)
    assert rec[0].tolist() == [0, 8, 0, 0, 0x11, 0, 0, 1]
    by = DM.info_bytes(info[0])
    assert DM.check_lc(by, 1) and (by[0] & 63, by[3] << 16 | by[4] << 8 | by[5], by[6] << 16 | by[7] << 8 | by[8]) == (3, 5678, 1234)
    short_bits, short_levels = _check_slice(A, v[:last], [(m, -1, 1)], pl)
    assert short_levels[0].tolist() == [0, 0, 2] and not short_bits.any()


def test_cuts_at_either_end(A):
    pl = DM.plan(25_000.0)  # sps 5.208...
    v, (m0, m1, m2) = _slot_plane(pl, [HEADER, None, HEADER], lead=0)
    o = pl["o"]
    front = m0 + o[-66]  # the first CACH instant of slot 0
    assert front == 0
    # dropping samples in front moves every m down: the CACH alone outside, then the burst cut by one sample
    only_cach = m0 + o[-54]  # samples to drop so that the burst's first instant is sample 0
    rows = []
    planes = []
    for drop in (0, 1, only_cach, only_cach + 1):
        planes.append(v[drop:])
        rows.append([(m0 - drop, -1, 1), (m1 - drop, -1, 1), (m2 - drop, -1, 1)])
    flags = []
    for plane, r in zip(planes, rows):
        bits, levels = _check_slice(A, plane, r, pl)
        flags.append(levels[:, 2].tolist())
        if levels[0, 2] == 1:  # the CACH outside: its bits are 0, the burst is read
            assert bits[0, 0] >> 8 == 0 and DM.decode_all(bits[:1], [1])[1][0][2:6].tolist() == [0, 0, 0x11, 0]
    assert flags == [[3, 3, 3], [1, 3, 3], [1, 3, 3], [0, 3, 3]]
    # the end: the last burst's last instant is the plane's last sample, then one short, then far short, then a hit far outside
    last = m2 + o[77]
    bits, levels = _check_slice(A, v[: last + 1], [(m2, -1, 1), (m2 + 1, -1, 1), (len(v) + 5000, 1, 0), (-5000, 1, 2), (m2, 1, 3)], pl)
    assert levels[:, 2].tolist() == [3, 2, 0, 0, 1] and not bits[1:4].any()


def test_thresholds_and_levels(A):
    pl = DM.plan(48_000.0)  # sps 10
    a = 1000
    sync = DM.sync_levels(DM.BS_VOICE)
    # the payload symbols -54 .. -1 carry the probes; Sigma = 0 and A = 72 a, so d = 24 y and the second bit is (|y| >= 2 a)
    probes = [2 * a, 2 * a - 1, 2 * a + 1, -2 * a, -2 * a + 1, -2 * a - 1, 0, 1, -1, 3 * a, -3 * a, a, -a]
    levels = [0] * 12 + (probes + [0] * 54)[:54] + [s * a for s in sync] + [0] * 54

    def plane_of(values):
        return IM.crafted_plane(2000, pl["ident"], 700, values, first=-66, amp=1)

    v = plane_of(levels)
    bits, lev = _check_slice(A, v, [(700, 1, 0), (700, -1, 1), (700, 1, 2)], pl)
    assert lev[0].tolist() == [0, 72 * a, 3] and lev[1].tolist() == [0, -72 * a, 3]
    two = [(b >> 1, b & 1) for b in [(DM.record_bits(bits[0])[24 + 2 * j] << 1 | DM.record_bits(bits[0])[24 + 2 * j + 1]) for j in range(13)]]
    assert two == [(0, 1), (0, 0), (0, 1), (1, 1), (1, 0), (1, 1), (0, 0), (0, 0), (1, 0), (0, 1), (1, 1), (0, 0), (1, 0)]
    # A < 0 (the voice word read as a data hit): every second bit is set, the first bits stay
    assert all(DM.record_bits(bits[1])[2 * j + 1] == 1 for j in range(144))
    assert [DM.record_bits(bits[1])[2 * j] for j in range(144)] == [DM.record_bits(bits[0])[2 * j] for j in range(144)]
    # A = 0: a plane that is 0 under the sync word
    flat = plane_of([0] * 12 + probes + [0] * (132 - len(probes)))
    bits, lev = _check_slice(A, flat, [(700, 1, 0)], pl)
    assert lev[0].tolist() == [0, 0, 3] and all(DM.record_bits(bits[0])[2 * j + 1] == 1 for j in range(144))
    # a DC under everything: Sigma takes it out
    dc = plane_of([x + 777 for x in levels])
    bits_dc, lev_dc = _check_slice(A, dc, [(700, 1, 0)], pl)
    assert lev_dc[0].tolist() == [24 * 777, 72 * a, 3]
    np.testing.assert_array_equal(bits_dc[0], _slice(A, v, [(700, 1, 0)], pl)[0][0])
    # the largest plane values, in the sync word and around it
    big = plane_of([V_MAX, -V_MAX] * 6 + [V_MAX if j % 3 else -V_MAX for j in range(54)] + [s // 3 * V_MAX for s in sync] + [-V_MAX, V_MAX] * 27)
    bits, lev = _check_slice(A, big, [(700, 1, 0), (700, -1, 1)], pl)
    assert lev[0].tolist() == [0, 24 * V_MAX, 3] and lev[1, 1] == -24 * V_MAX


def test_all_four_kinds_in_one_call(A):
    pl = DM.plan(48_000.0)
    rng = np.random.default_rng(4)
    info = rng.integers(0, 2, 96).tolist()
    slots = [DM.cach_bits(0, rng) + DM.voice_burst_bits(0, rng), DM.cach_bits(1, rng) + DM.data_burst_bits(1, 7, 3, DM.csbk_info(5, 16, [1, 2, 3, 4, 5, 6, 7, 8])),
             DM.cach_bits(0, rng) + DM.voice_burst_bits(2, rng), DM.cach_bits(1, rng) + DM.data_burst_bits(3, 2, 6, info)]
    levels = [lev for bits in slots for lev in DM.levels_of_bits(bits)]
    v, ms = _slot_plane(pl, None, kind_levels=levels)
    rows = [(ms[0], 1, 0), (ms[1], -1, 1), (ms[2], 1, 2), (ms[3], -1, 3)]
    bits, lev = _check_slice(A, v, rows, pl)
    assert lev[:, 2].tolist() == [3, 3, 1, 1] and (lev[:, 1] == 72_000).all()
    assert [DM.record_bits(w)[24:] for w in bits] == [s[24:] for s in slots]
    assert [DM.record_bits(w)[:24] for w in bits] == [slots[0][:24], slots[1][:24], [0] * 24, [0] * 24]
    got_info, rec = _decode(A, bits, [0, 1, 2, 3])
    want_info, want_rec = DM.decode_all(bits, [0, 1, 2, 3])
    np.testing.assert_array_equal(got_info, want_info)
    np.testing.assert_array_equal(rec, want_rec)
    assert rec.tolist() == [[0, 8, 4, 0, 0, 4, 0, 0], [0, 12, 0, 0, 0x73, 0, 0, 1], [4, 0, 4, 0, 0, 4, 0, 0], [4, 0, 0, 0, 0x26, 0, 0, 1]]
    assert DM.check_csbk(DM.info_bytes(got_info[1]), 3) and DM.record_bits(got_info[3]) == info
    # the package's wrappers give the same
    import torch

    x_bits, x_lev = A.dmr.slice_bursts(torch.from_numpy(np.asarray(v, dtype=np.int32)).cuda(), rows, A.plan_dmr(48_000.0))
    np.testing.assert_array_equal(x_bits, bits)
    np.testing.assert_array_equal(x_lev, lev)
    x_info, x_rec = A.dmr.decode_bursts(x_bits, [0, 1, 2, 3])
    np.testing.assert_array_equal(x_info, got_info)
    np.testing.assert_array_equal(x_rec, rec)


def test_the_coder_cases_of_the_host_test(A):
    cases = DM.coder_cases()
    names = list(cases)
    words, kinds = [cases[n][0] for n in names], [cases[n][1] for n in names]
    want_info, want_rec = DM.decode_all(words, kinds)
    # the oracle's expectation (tests/test_dmr_host.py holds every case; here the kinds of outcome are all there)
    assert sorted(set(want_rec[:, 5].tolist())) == [0, 1, 2, 4] and sorted(set(want_rec[:, 2].tolist())) == [0, 1, 2, 4]
    assert sorted(set(want_rec[:, 0].tolist())) == [0, 1, 4] and want_rec[:, 7].max() >= 3 and len(names) > 230
    info, rec = _decode(A, words, kinds)
    for j, name in enumerate(names):
        assert rec[j].tolist() == want_rec[j].tolist() and info[j].tolist() == want_info[j].tolist(), name


def test_nothing_to_do(A):
    import torch

    pl = A.plan_dmr(48_000.0)
    empty = torch.empty(0, dtype=torch.int32, device="cuda")
    bits, lev = A.dmr.slice_bursts(empty, [(10, 1, 0)], pl)
    assert bits.shape == (1, 9) and lev.shape == (1, 3) and not bits.any() and not lev.any()
    plane = torch.zeros(100, dtype=torch.int32, device="cuda")
    bits, lev = A.dmr.slice_bursts(plane, np.zeros((0, 3), dtype=np.int64), pl)
    assert bits.shape == (0, 9) and lev.shape == (0, 3)
    info, rec = A.dmr.decode_bursts(np.zeros((0, 9), dtype=np.uint32), [])
    assert info.shape == (0, 3) and rec.shape == (0, 8)
