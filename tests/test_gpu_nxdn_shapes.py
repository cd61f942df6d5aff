"""``iqa_nxdn_slice`` and ``iqa_nxdn_decode`` on the MI355X at their edge shapes, on crafted planes and
words, against the model of tests/nxdn_model.py: a header frame at 4, 224 and 20.125 samples to a symbol, ``valid`` one short of
and at 10, 18 and 192, hits in front of and outside the plane, the slicing threshold on equality and one either side of it for
both signs, a DC under everything, the largest plane values, a frame of +3 alone whose bits are the scrambler's mask, K = 1, 3,
4, 5 and 261, every class mask 0 .. 15 and values over 15 in one call, every block type clean, with one channel error and with
an input on which the tie rule matters, K = 0 and n = 0; every output lies in a buffer with sentinels behind it.  Every
comparison is of integers and exact."""
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


NM = _load("nxdn_model")
IM = NM.IM
SENTINEL, TAIL = 0x5A5A5A5A, 64
V_MAX = 64 * 65534
S = NM.SCALE
W, INFO = NM.WORDS, NM.INFO


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
    """``iqa_nxdn_slice`` straight through the binding, the outputs in guarded buffers: (bits uint32[K][12], levels int64[K][3])."""
    import torch

    N = A.native
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    k = rows.shape[0]
    plane = torch.from_numpy(np.asarray(v, dtype=np.int32)).cuda()
    hits = torch.from_numpy(rows).cuda()
    (bits, fb), (levels, fl) = _guarded(torch, W * k, torch.int32), _guarded(torch, 3 * k, torch.int64)
    offsets = (c_int32 * 192)(*pl["o"])
    N.call("iqa_nxdn_slice", N.ptr(plane), c_int64(plane.numel()), N.ptr(hits), c_int64(k), offsets, N.ptr(bits), N.ptr(levels), N.stream_ptr())
    torch.cuda.synchronize()
    assert (bits[W * k :] == fb).all() and (levels[3 * k :] == fl).all(), "a sentinel behind an output was overwritten"
    return bits[: W * k].cpu().numpy().view(np.uint32).reshape(k, W), levels[: 3 * k].cpu().numpy().reshape(k, 3)


def _decode(A, words, classes):
    """``iqa_nxdn_decode`` straight through the binding, the outputs in guarded buffers: (info uint32[K][14], rec int32[K][4])."""
    import torch

    N = A.native
    words = np.asarray(words, dtype=np.uint32).reshape(-1, W)
    k = words.shape[0]
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    classes_dev = torch.from_numpy(np.asarray(classes, dtype=np.uint8)).cuda()
    (info, fi), (rec, fr) = _guarded(torch, INFO * k, torch.int32), _guarded(torch, 4 * k, torch.int32)
    N.call("iqa_nxdn_decode", N.ptr(bits), N.ptr(classes_dev), c_int64(k), N.ptr(info), N.ptr(rec), N.stream_ptr())
    torch.cuda.synchronize()
    assert (info[INFO * k :] == fi).all() and (rec[4 * k :] == fr).all(), "a sentinel behind an output was overwritten"
    return info[: INFO * k].cpu().numpy().view(np.uint32).reshape(k, INFO), rec[: 4 * k].cpu().numpy().reshape(k, 4)


def _check_slice(A, v, rows, pl):
    bits, levels = _slice(A, v, rows, pl)
    want_bits, want_levels = NM.slice_all(v, rows, pl)
    np.testing.assert_array_equal(bits, want_bits)
    np.testing.assert_array_equal(levels, want_levels)
    return bits, levels


def _check_decode(A, bits, classes=None):
    """What lies behind the LICHs, held to the model: (classes, info, rec)."""
    if classes is None:
        classes = [NM.lich_mask(NM.lich_of(w)[0]) if NM.lich_parity_ok(NM.lich_of(w)[0]) else 0 for w in np.asarray(bits).tolist()]
    info, rec = _decode(A, bits, classes)
    want_info, want_rec = NM.decode_all(bits, classes)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rec, want_rec)
    return classes, info, rec


def _plane(pl, levels, lead=3, amp=1000, tail=1):
    """(v, m): symbol levels written straight into a plane, ``lead`` samples in front of symbol 0 and ``tail`` behind the last one's
    first; m is the first sample of sync symbol 0, so every instant m + o[i] is symbol i's first."""
    n = lead + int(round((len(levels) - 1) * pl["sps"])) + tail
    return IM.crafted_plane(n, pl["ident"], lead, levels, first=0, amp=amp), lead


def _levels(item, seed=3):
    return [NM.LEVEL[d] for d in NM.make_frame(item, np.random.default_rng(seed))]


def _messages(info_row, mask):
    """(the octets of the message, whether the CRC holds) of the FACCH1s that ``mask`` names."""
    out = []
    for bit, at in ((NM.FACCH1_A, 2), (NM.FACCH1_B, 5)):
        if mask & bit:
            b, ok = NM.block_ok(info_row[at : at + 3], "facch1")
            out.append((NM.bits_bytes(b), ok))
    return out


@pytest.mark.parametrize("fs_ch,rate", [(19_200.0, 4800), (537_600.0, 2400), (96_600.0, 4800)], ids=["sps4", "sps224", "sps20.125"])
def test_a_header_at_the_rate_limits(A, fs_ch, rate):
    pl = NM.plan(fs_ch, rate)
    v, m = _plane(pl, _levels(NM.header_frame()))
    last = m + pl["o"][191]
    assert len(v) == last + 1  # the plane ends on the last symbol's instant: one sample fewer cuts it
    bits, levels = _check_slice(A, v, [(m, 1)], pl)
    assert levels[0].tolist() == [S * 3000, 0, 192]
    assert NM.lich_of(bits[0]) == (NM.lich_byte(1, 0, 0), True)
    classes, info, rec = _check_decode(A, bits)
    assert classes == [7] and rec[0].tolist() == [7, 0, 0, 0] and _messages(info[0], 7) == [(NM.VCALL, True), (NM.VCALL, True)]
    sacch, ok = NM.block_ok(info[0, 0:2], "sacch")
    assert ok and sacch == NM.sacch_info(0, NM.RAN, NM.bytes_bits(NM.VCALL)[:18]) and not info[0, 8:].any()
    short_bits, short_levels = _check_slice(A, v[:last], [(m, 1)], pl)
    assert short_levels[0].tolist() == [S * 3000, 0, 191] and short_bits[0, :11].tolist() == bits[0, :11].tolist()
    assert short_bits[0, 11] == (bits[0, 11] & 0xFFFFFFFC)  # symbol 191 alone reads 0, its scrambler bit too
    # the same frame negated is the same frame at s = -1
    neg_bits, neg_levels = _check_slice(A, -v, [(m, -1)], pl)
    np.testing.assert_array_equal(neg_bits, bits)
    assert neg_levels[0].tolist() == [S * 3000, 0, 192]


def test_valid_on_either_side_of_what_is_needed(A):
    pl = NM.plan(25_000.0)  # sps 5.208...
    v, m = _plane(pl, _levels(NM.header_frame()), lead=0)
    o = pl["o"]
    got = {}
    for valid in (192, 191, 18, 17, 10, 9):
        bits, levels = _check_slice(A, v[: m + o[valid - 1] + 1], [(m, 1)], pl)
        assert levels[0, 2] == valid
        got[valid] = (bits, levels)
    for valid in (192, 191, 18):  # the LICH is whole
        assert NM.lich_of(got[valid][0][0]) == (NM.lich_byte(1, 0, 0), True)
    assert NM.lich_of(got[17][0][0])[1] is False  # symbol 17 reads 0 0
    assert NM.decoder_classes(*got[192]) == [7] and NM.decoder_classes(*got[191]) == [0]
    assert A.nxdn.decoder_classes(*got[192]).tolist() == [7] and A.nxdn.decoder_classes(*got[191]).tolist() == [0]
    rows = np.array([(m, 1)])
    for valid, cut in ((191, 1), (18, 1), (17, 1), (9, 1)):
        zeros = (np.zeros((1, INFO), dtype=np.uint32), np.zeros((1, 4), dtype=np.int32))
        frames, counts = A.nxdn.parse_frames(rows, *got[valid], *zeros, 25_000.0)
        want_frames, want_counts = NM.parse(rows, *got[valid], *zeros, 25_000.0)
        assert counts == want_counts and counts["cut"] == cut and len(frames) == len(want_frames) == (1 if valid >= 18 else 0)
    assert got[10][1][0].tolist() == [S * 3000, 0, 10] and got[10][0][0, 0] == NM.FSW << 12 and not got[10][0][0, 1:].any()
    assert got[9][1][0].tolist() == [0, 0, 9] and not got[9][0].any()
    # hits in front of the plane and far outside
    n = len(v)
    rows = [(-1, 1), (-5000, -1), (n + 5000, 1), (n - 1, 1), (n, -1), (m, 1)]
    bits, levels = _check_slice(A, v, rows, pl)
    assert levels[:, 2].tolist() == [0, 0, 0, 1, 0, 192] and not bits[:5].any() and not levels[:5, :2].any()


def test_thresholds_levels_and_the_scrambler(A):
    pl = NM.plan(48_000.0)  # sps 10
    a = 1000
    sync = NM.fsw_levels()
    mask = NM.scramble_mask()
    # the sync word at a s_i: A = 370 * 3 a, Dc = 0, so d = 370 y and the second bit is (|y| >= 2 a)
    probes = [2 * a, 2 * a - 1, 2 * a + 1, -2 * a, -2 * a + 1, -2 * a - 1, 0, 1, -1, 3 * a, -3 * a, a, -a]
    values = [s * a for s in sync] + probes + [0] * (192 - 10 - len(probes))

    def plane_of(vals):
        return IM.crafted_plane(2500, pl["ident"], 100, vals, first=0, amp=1)

    def two(words, count=13, first=10):
        """(sign bit less the scrambler, magnitude bit) of ``count`` symbols."""
        bits = NM.record_bits(words)
        return [(bits[2 * (first + j)] ^ mask[2 * (first + j)], bits[2 * (first + j) + 1]) for j in range(count)]

    v = plane_of(values)
    bits, lev = _check_slice(A, v, [(100, 1), (100, -1)], pl)
    assert lev[0].tolist() == [S * 3 * a, 0, 192] and lev[1].tolist() == [-S * 3 * a, 0, 192]
    want = [(0, 1), (0, 0), (0, 1), (1, 1), (1, 0), (1, 1), (0, 0), (0, 0), (1, 0), (0, 1), (1, 1), (0, 0), (1, 0)]
    assert two(bits[0]) == want
    assert [NM.DIBIT[s] for s in sync] == [f << 1 | g for f, g in two(bits[0], 10, 0)]  # the word's own inner and outer symbols
    # A < 0 (the word read with the wrong sign): every second bit is set
    assert all(b == 1 for _, b in two(bits[1], 192, 0))
    # the negated plane at s = -1 reads as the plane at s = +1: equality and either side of it in the other sign
    neg_bits, neg_lev = _check_slice(A, -v, [(100, -1)], pl)
    assert two(neg_bits[0]) == want and neg_lev[0].tolist() == [S * 3 * a, 0, 192]
    # a DC under everything: Dc takes it out, so the thresholds sit at Dc +- 2 a on both sides of Dc
    for dc in (777, -123_456):
        bits_dc, lev_dc = _check_slice(A, plane_of([x + dc for x in values]), [(100, 1)], pl)
        assert lev_dc[0].tolist() == [S * 3 * a, S * dc, 192]
        np.testing.assert_array_equal(bits_dc[0], bits[0])
    # A = 0: a plane that is 0 under the sync word
    flat = plane_of([0] * 10 + probes + [0] * (182 - len(probes)))
    bits0, lev0 = _check_slice(A, flat, [(100, 1), (100, -1)], pl)
    assert lev0[:, :2].tolist() == [[0, 0], [0, 0]] and all(b == 1 for _, b in two(bits0[0], 192, 0))
    # the largest plane values, in the sync word and behind it: 15 Q reaches 15 * 26 * V_MAX / 3
    big = plane_of([s * (V_MAX // 3) for s in sync] + [V_MAX if j % 3 else -V_MAX for j in range(182)])
    bits_big, lev_big = _check_slice(A, big, [(100, 1), (100, -1)], pl)
    assert lev_big[0].tolist() == [15 * 74 * (V_MAX // 3), 0, 192] and lev_big[1, 0] == -lev_big[0, 0]
    assert two(bits_big[0], 6) == [(1, 1), (0, 1), (0, 1), (1, 1), (0, 1), (0, 1)]
    _check_slice(A, plane_of([V_MAX if s > 0 else -V_MAX for s in sync] + [-V_MAX, V_MAX] * 91), [(100, 1), (100, -1)], pl)
    _check_slice(A, plane_of([V_MAX] * 10 + [-V_MAX] * 182), [(100, 1), (100, -1)], pl)
    # every scrambler bit matters: +3 alone behind the sync word is sent as 01 everywhere, and reads as 01 with the mask over it
    bits3, lev3 = _check_slice(A, plane_of([s * a for s in sync] + [3 * a] * 182), [(100, 1)], pl)
    sent = NM.word_bits(NM.FSW, 20) + [0, 1] * 182
    want_bytes = bytes(x ^ y for x, y in zip(NM.bits_bytes(sent), NM.MASK_BYTES))
    assert bits3[0].astype(">u4").tobytes() == want_bytes and lev3[0].tolist() == [S * 3 * a, 0, 192]
    assert sum(bin(x).count("1") for x in NM.MASK_BYTES) == 92


@pytest.mark.parametrize("k", [1, 3, 4, 5, 261])
def test_frame_counts(A, k):
    pl = NM.plan(19_200.0)
    items = [NM.header_frame(), NM.voice_frame(3), NM.second_half_frame(), NM.cac_frame(NM.SITE_INFO), NM.voice_frame(0), NM.header_frame(NM.TX_REL),
             NM.cac_frame(NM.IDLE)]
    frames = [_levels(item, seed=j) for j, item in enumerate(items)]
    v, m = _plane(pl, [x for f in frames for x in f] + [1] * 192)
    rows = [(m + int(round(192 * (j % 7) * pl["sps"])) + (0 if j < 7 else (j % 5) - 2), 1 if j < 7 or j % 3 else -1) for j in range(k)]
    bits, lev = _check_slice(A, v, rows, pl)
    classes, info, rec = _check_decode(A, bits)
    assert len(rec) == k and rec[: min(k, 7)].tolist() == [[c, 0, 0, 0] for c in (7, 1, 5, 8, 1, 7, 8)][:k]
    # every mask, given and not derived, on every frame
    classes = [(j * 5 + 1) % 9 for j in range(k)]
    _check_decode(A, bits, classes)


def test_every_class_mask_in_one_call(A):
    head = NM.frame_words(NM.header_frame())
    control = NM.frame_words(NM.cac_frame(NM.SRV_INFO))
    masks = list(range(16)) + [16, 17, 64, 200, 255]
    words = [control if c == 8 else head for c in masks]
    classes, info, rec = _check_decode(A, words, masks)
    for j, c in enumerate(masks):
        valid = c <= 8
        assert rec[j, 0] == (c if valid else 0) and not rec[j, 1:].any()  # clean words: every metric is 0
        assert info[j, 0:2].any() == (valid and bool(c & 1)) and info[j, 2:5].any() == (valid and bool(c & 2))
        assert info[j, 5:8].any() == (valid and bool(c & 4)) and info[j, 8:14].any() == (c == 8)
        if valid and c < 8:
            assert _messages(info[j], c) == [(NM.VCALL, True)] * bin(c & 6).count("1")
    b, ok = NM.block_ok(info[8, 8:14], "cac")
    assert ok and b == NM.cac_info(0, NM.RAN, NM.SRV_INFO)
    # the package's wrappers give the same, and refuse what the kernel would read as nothing
    x_info, x_rec = A.nxdn.decode_frames(np.array(words[:9], dtype=np.uint32), masks[:9])
    np.testing.assert_array_equal(x_info, info[:9])
    np.testing.assert_array_equal(x_rec, rec[:9])
    for bad in (9, 15, 16, 255, -1):
        with pytest.raises(ValueError):
            A.nxdn.decode_frames(np.array(words[:1], dtype=np.uint32), [bad])


def test_the_coder_cases_of_the_host_test(A):
    cases = NM.coder_cases()
    names = list(cases)
    words, classes = [cases[n][0] for n in names], [cases[n][1] for n in names]
    want_info, want_rec = NM.decode_all(words, classes)
    at = names.index
    # the model's expectation (tests/test_nxdn_host.py holds every case; here the kinds of outcome are all there)
    for name in NM.BLOCK_CASES:
        slot = {"sacch": 1, "cac": 1, "facch1-a": 2, "facch1-b": 3}[name]
        assert not want_rec[at(name), 1:].any() and want_rec[at(f"{name}-one-7"), slot] == 1
        assert want_info[at(f"{name}-one-7")].tolist() == want_info[at(name)].tolist()  # one flipped channel bit is restored
        tie = NM.decode_frame(*cases[f"{name}-tie"])
        assert tie[2] > 0 and tie[0] != NM.decode_frame(*cases[f"{name}-tie"], smaller=False)[0]  # an equal-metric compare on the surviving path
    assert len(names) > 100
    info, rec = _decode(A, words, classes)
    for j, name in enumerate(names):
        assert rec[j].tolist() == want_rec[j].tolist() and info[j].tolist() == want_info[j].tolist(), name
    for name in NM.BLOCK_CASES:
        tie = NM.decode_frame(*cases[f"{name}-tie"])
        assert info[at(f"{name}-tie")].tolist() == tie[0] and rec[at(f"{name}-tie")].tolist() == tie[1]


def test_nothing_to_do(A):
    import torch

    pl = A.plan_nxdn(48_000.0)
    empty = torch.empty(0, dtype=torch.int32, device="cuda")
    bits, lev = A.nxdn.slice_frames(empty, [(10, 1)], pl)
    assert bits.shape == (1, W) and lev.shape == (1, 3) and not bits.any() and not lev.any()
    plane = torch.zeros(100, dtype=torch.int32, device="cuda")
    bits, lev = A.nxdn.slice_frames(plane, np.zeros((0, 2), dtype=np.int64), pl)
    assert bits.shape == (0, W) and lev.shape == (0, 3)
    info, rec = A.nxdn.decode_frames(np.zeros((0, W), dtype=np.uint32), [])
    assert info.shape == (0, INFO) and rec.shape == (0, 4)
    # straight through the binding with NULL pointers: K = 0 and n = 0 touch nothing
    N = A.native
    null = N.ptr(None)
    offsets = (c_int32 * 192)(*pl.offsets)
    N.call("iqa_nxdn_slice", null, c_int64(0), null, c_int64(5), offsets, null, null, N.stream_ptr())
    N.call("iqa_nxdn_slice", null, c_int64(100), null, c_int64(0), offsets, null, null, N.stream_ptr())
    N.call("iqa_nxdn_decode", null, null, c_int64(0), null, null, N.stream_ptr())
