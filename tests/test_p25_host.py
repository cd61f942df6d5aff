"""The P25 phase 1 frame decoding (--find-p25) without a GPU: the constants of the package against the
oracle's own copy, the facts that section 31 states about the codes, the oracle's coders on crafted errors, ``plan_p25`` against
the oracle's plan, the needed ``valid`` numbers, the package's parser, call tracker and TSBK collapse against the oracle's on
crafted frames, the JSON round trip, the layer table's branches, the CLI's flags, the entry points' argument checks, the oracle
end to end on synthesised theta (clean, negated and at the noise level found here) and the model capture of the GPU test's CLI
run through the numpy pipeline."""
from __future__ import annotations

import heapq
import importlib.util
import json
import sys
from ctypes import c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest

import iq_to_audio_amd as A
from iq_to_audio_amd import cli
from iq_to_audio_amd import describe as DS
from iq_to_audio_amd import dsp_plan as P
from iq_to_audio_amd import find_layers as FL
from iq_to_audio_amd import p25 as X


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


PM = _load("p25_model")
FS = 160_000.0
#: radians of white noise on theta: the largest of 0.01, 0.02, ... at which the oracle alone still decodes every frame of the test
#: stream (found on the CPU: 0.06 loses one link control word to the Reed-Solomon check)
NOISE = 0.05
FREE_DISTANCE = 5  # of the trellis, in channel bits: found by the search below, recorded in section 31
SINGLE_FLIPS_RESTORED = 196  # of the 196 single flips of a block, those that the oracle restores: measured, recorded in section 31


# ---- constants and the codes ------------------------------------------------------------------------------------------------------


def test_constants_are_the_oracles():
    assert X.SYNC == PM.SYNC and [(p.protocol, p.word, p.symbols) for p in X.P25_PATTERNS] == [(p[0], p[3], p[4]) for p in PM.P25_PATTERNS]
    for name in ("GOLAY_POLY", "HAMMING_COLUMNS", "TRELLIS_PAIRS", "TRELLIS_POINTS", "INTERLEAVE", "GF_POLY", "DUIDS", "HANG_S", "STATUS_EVERY",
                 "NEED_NID", "NEED_TDULC", "NEED_LDU1", "NEED_TSBK"):
        assert getattr(X, name) == getattr(PM, name), name
    assert X.BCH_POLY == PM.bch_generator() and X.BCH_MAX_DISTANCE == 11 and X.GOLAY_MAX_DISTANCE == 3 and X.CRC_POLY == 0x1021
    assert (P.P25_OFFSETS, P.P25_WORDS, P.P25_INFO, P.P25_RECORD) == (PM.OFFSETS, PM.WORDS, 9, 8) == (864, 54, 9, 8)
    assert X.PLANE_RATES == (4800,) and X.NID_RECORD == 4 and X.RS_ROOTS == 12
    header = (Path(__file__).resolve().parent.parent / "include" / "iqa_hotpath.h").read_text()
    for text in ("#define IQA_P25_OFFSETS 864", "#define IQA_P25_WORDS 54", "#define IQA_P25_INFO 9", "#define IQA_P25_RECORD 8",
                 "#define IQA_ABI_VERSION 1"):
        assert text in header


def test_the_sync_word_and_the_level_identities():
    lev = PM.sync_levels()
    assert sorted(lev) == [-3] * 13 + [3] * 11 and lev == list(A.identify.symbols_of(X.P25_PATTERNS[0]))
    # x_i = s L sgn_i + c: 12 Q + P = 286 s L and 12 P + Q = 286 c, for both signs
    sgn = [1 if x > 0 else -1 for x in lev]
    for s in (1, -1):
        for level, dc in ((1000, 0), (1000, 77), (3, -5000), (4_000_000, 123_456)):
            x = [s * level * g + dc for g in sgn]
            p, q = sum(x), sum(g * xi for g, xi in zip(sgn, x))
            assert s * (12 * q + p) == 286 * level and 12 * p + q == 286 * dc


def test_the_bch_code():
    g = PM.bch_generator()
    assert g == 0o6331141367235453 and g.bit_length() - 1 == 47 and PM.poly2_mod((1 << 63) | 1, g) == 0
    words = PM.bch_codewords()
    assert words.shape == (65536,) and all(int(words[d]) == PM.bch_encode(d) for d in (0, 1, 2, 0x2935, 0x8000, 0xFFFF))
    assert (words >> np.uint64(47) == np.arange(65536, dtype=np.uint64)).all()  # systematic
    assert int(np.bitwise_count(words[1:]).min()) == 23
    cases = PM.nid_cases()
    nid = lambda name: PM.nid_decode(PM.data_bits_of(cases[name])[48:112])  # noqa: E731
    value = PM.NAC << 4 | 3
    assert nid("clean") == [0, 0, value, 1]
    for j in range(63):
        assert nid(f"single-{j}") == [1, 1, value, 0], j
    assert nid("single-63") == [0, 0, value, 0]  # the parity bit alone: reported, not used
    assert nid("eleven") == [1, 11, value, 0]
    other = nid("twelve-other")
    assert other[:2] == [1, 11] and other[2] != value  # twelve flips that land within 11 of another codeword
    refused = nid("twelve-refused")
    assert refused[0] == 2 and refused[1] == 12 and refused[2] == PM.bits_word(PM.data_bits_of(cases["twelve-refused"])[48:64])
    assert nid("zeros") == [0, 0, 0, 1]


def test_golay_and_hamming():
    assert min(bin(cw).count("1") for cw in PM.GOLAY[1:]) == 8 and all(cw >> 12 == d and bin(cw).count("1") % 2 == 0 for d, cw in enumerate(PM.GOLAY))
    assert all(PM.GOLAY[a ^ b] == PM.GOLAY[a] ^ PM.GOLAY[b] for a, b in ((1, 2), (0xABC, 0x123), (0xFFF, 0x800)))  # linear: weight = distance
    cases = PM.coder_cases()
    info, rec = PM.decode_frame(*cases["tdulc"])
    assert rec == [2, 0, 0, 0, 0, 0, 0, 0] and PM.info_hexbits(info) == PM.LC and PM.rs_check(PM.info_hexbits(info))
    for name, want in (("golay-single", [2, 12, 0, 12]), ("golay-double", [2, 2, 0, 4]), ("golay-triple", [2, 2, 0, 6])):
        got_info, got = PM.decode_frame(*cases[name])
        assert got_info == info and got[:4] == want, name
    got_info, got = PM.decode_frame(*cases["golay-four"])
    assert got[:4] == [2, 0, 1, 0] and got_info != info and not PM.rs_check(PM.info_hexbits(got_info))
    # Hamming: ten distinct nonzero columns, every flip restored, the five other syndromes leave the word alone
    cols = PM.HAMMING_ALL_COLUMNS
    assert len(set(cols)) == 10 and 0 not in cols and set(range(1, 16)) - set(cols) == {0b1111, 0b1010, 0b1001, 0b0110, 0b0101}
    info, rec = PM.decode_frame(*cases["ldu1"])
    assert rec == [1, 0, 0, 0, 0, 0, 0, 0] and PM.info_hexbits(info) == PM.lc_hexbits(3, 111, 222)
    for k in range(10):
        got_info, got = PM.decode_frame(*cases[f"hamming-{k}"])
        assert got_info == info and got[:4] == [1, 8, 0, 8], k
    for name in ("1111", "1010", "1001", "0110", "0101"):
        got_info, got = PM.decode_frame(*cases[f"unmatched-{name}"])
        assert got[:4] == [1, 0, 1, 0], name
    for six in range(64):
        word = PM.hamming_encode(PM.word_bits(six, 6))
        assert PM.hamming_decode(word) == (PM.word_bits(six, 6), 0)


def test_reed_solomon_and_the_crc():
    lc = PM.LC
    assert PM.rs_check(lc) and X.check_lc(lc) and len(PM.rs_generator()) == 13
    for j in range(24):
        for delta in (1, 0x20, 0x3F):
            bad = list(lc)
            bad[j] ^= delta
            assert not PM.rs_check(bad) and not X.check_lc(bad), (j, delta)
    assert all(X.gf_mul(a, b) == PM.gf_mul(a, b) for a in (0, 1, 2, 29, 33, 63) for b in range(64))
    assert X.lc_fields(lc) == dict(lco=0, mfid=0, src=PM.SRC, dst=PM.TG, hex="00000000000923cace")
    unit = X.lc_fields(PM.lc_hexbits(3, 111, 222, mfid=0x90))
    assert (unit["lco"], unit["mfid"], unit["src"], unit["dst"]) == (3, 0x90, 111, 222)
    assert X.lc_fields(PM.lc_hexbits(3, 1, 2)[:12][:0] + [5] + [0] * 11)["src"] is None  # another LCO is kept as hex
    assert PM.crc_ccitt(b"123456789") == X.crc_ccitt(b"123456789") == 0x31C3
    by = PM.tsbk_bytes(0x3B, 0, PM.NET)
    assert X.check_tsbk(by) and PM.check_tsbk(by) and not X.check_tsbk(PM.tsbk_bytes(0x3B, 0, PM.NET, break_crc=True))
    for j in range(96):
        bad = list(by)
        bad[j >> 3] ^= 0x80 >> (j & 7)
        assert not X.check_tsbk(bad)


def _free_distance() -> int:
    """The smallest distance in channel bits between two paths of the trellis that part in one state and meet again."""
    bits = lambda i, j: PM.TRELLIS_PAIRS[PM.TRELLIS_POINTS[i][j]][0] << 2 | PM.TRELLIS_PAIRS[PM.TRELLIS_POINTS[i][j]][1]  # noqa: E731
    heap = [(bin(bits(s, a) ^ bits(s, b)).count("1"), a, b) for s in range(4) for a in range(4) for b in range(a + 1, 4)]
    heapq.heapify(heap)
    done = set()
    while heap:
        d, a, b = heapq.heappop(heap)
        if a == b:
            return d
        if (a, b) in done:
            continue
        done.add((a, b))
        for x in range(4):
            for y in range(4):
                heapq.heappush(heap, (d + bin(bits(a, x) ^ bits(b, y)).count("1"), x, y))
    raise AssertionError


def test_the_trellis():
    assert sorted(PM.INTERLEAVE) == list(range(98)) and PM.INTERLEAVE[:4] == (0, 1, 8, 9) and PM.INTERLEAVE[26:30] == (2, 3, 10, 11)
    assert len(set(PM.TRELLIS_PAIRS)) == 16
    assert all(len(set(row)) == 4 for row in PM.TRELLIS_POINTS) and all(len({row[j] for row in PM.TRELLIS_POINTS}) == 4 for j in range(4))
    assert sorted(p for row in PM.TRELLIS_POINTS for p in row) == list(range(16))
    rng = np.random.default_rng(7)
    for _ in range(20):
        dibits = rng.integers(0, 4, 48).tolist()
        assert PM.trellis_decode(PM.trellis_encode(dibits)) == (dibits, 0)
    free = _free_distance()
    print("free distance", free)
    assert free == FREE_DISTANCE
    dibits = rng.integers(0, 4, 48).tolist()
    sent = PM.trellis_encode(dibits)
    restored = 0
    for k in range(196):
        bad = list(sent)
        bad[k >> 1] ^= 2 >> (k & 1)
        got, metric = PM.trellis_decode(bad)
        restored += got == dibits and metric == 1
    print("single flips restored", restored)
    assert restored == SINGLE_FLIPS_RESTORED
    # the tie rule: a word on which the two rules part; the specification's takes the smaller predecessor
    cases = PM.coder_cases()
    words, duid = cases["trellis-tie"]
    data = PM.data_bits_of(words)
    sent = [data[112 + 2 * j] << 1 | data[113 + 2 * j] for j in range(98)]
    small, large = PM.trellis_decode(sent), PM.trellis_decode(sent, smaller=False)
    assert small[1] == large[1] == 3 and small[0] != large[0]
    info, rec = PM.decode_frame(words, duid)
    assert PM.record_bits(info[:3]) == [b for d in small[0] for b in (d >> 1, d & 1)] and rec[:4] == [3, 3, 0, 0]
    info, rec = PM.decode_frame(*cases["tsbk"])
    assert rec == [3, 0, 0, 0, 0, 0, 0, 0] and [PM.info_bytes(info[3 * b : 3 * b + 3]) for b in range(3)] == PM.TSBK_THREE[1]
    assert all(PM.decode_frame(*cases[f"other-{d:x}"]) == ([0] * 9, [0] * 8) for d in (0x0, 0x3, 0xA, 0xC, 0x1, 0x9))


# ---- the plan and the needed lengths ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("fs_ch", [19_200.0, 160_000.0, 96_600.0, 1_075_200.0])
def test_plan_against_the_oracle(fs_ch):
    plan, want = P.plan_p25(fs_ch), PM.plan(fs_ch)
    assert plan.sps == want["sps"] == fs_ch / 4800.0 and len(plan.offsets) == 864
    assert list(plan.offsets) == want["o"] and plan.o(0) == 0 and plan.o(863) == want["o"][863]
    assert (plan.ident.window, plan.ident.half, plan.ident.shift) == (want["ident"]["L"], want["ident"]["h"], want["ident"]["sh"])
    assert plan.ident == P.plan_ident(fs_ch, 4800) and A.plan_p25 is P.plan_p25
    assert all(0 < b - a <= 225 for a, b in zip(plan.offsets, plan.offsets[1:]))
    if fs_ch == 96_600.0:  # sps 20.125: i = 4 and 12 fall on .5 and go to the even side
        assert (plan.o(4), plan.o(12), plan.o(20), plan.o(28)) == (80, 242, 402, 564)


def test_plan_refuses_rates_that_do_not_fit():
    for fs_ch in (19_199.0, 1_075_201.0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            P.plan_p25(fs_ch)
    for fs_ch in (19_199.0, 1_075_201.0):
        with pytest.raises(ValueError):
            PM.plan(fs_ch)
        with pytest.raises(ValueError):
            A.P25Decoder(fs_ch)


def test_the_needed_valid_numbers():
    q = PM.symbol_of
    assert (q(0), q(34), q(35), q(69), q(70)) == (0, 34, 36, 70, 72) and all(q(d) % 36 != 35 for d in range(840)) and q(839) == 862
    assert PM.NEED_NID == q(111 // 2) + 1 == 57
    assert PM.NEED_TDULC == q(399 // 2) + 1 == 205  # (a remembered 215 does not hold: data bit 399 lies in symbol 204)
    assert PM.NEED_LDU1 == q(1359 // 2) + 1 == 699
    assert PM.NEED_TSBK == tuple(q((112 + 196 * (b + 1) - 1) // 2) + 1 for b in range(3)) == (158, 259, 359)
    # the encoder's frames: a status symbol of value 2 at every i mod 36 = 35, and the data dibits where symbol_of says
    rng = np.random.default_rng(1)
    dibits = PM.make_frame(("ldu1", PM.LC), PM.NAC, rng)
    assert len(dibits) == 864 and all(dibits[i] == 2 for i in range(35, 864, 36))
    data = PM.data_bits_of(PM.words_of_dibits(dibits))
    assert len(data) == 1680 and data[:48] == PM.word_bits(PM.SYNC, 48) and data[48:112] == PM.nid_bits(PM.NAC, 5)
    assert [len(PM.make_frame(item, 1, rng)) for item in (("hdu",), ("ldu2",), ("tdu",), ("tdulc", PM.LC), PM.TSBK_ONE, PM.TSBK_THREE)] == [
        396, 864, 72, 216, 180, 360]


# ---- the parser, the call tracker and the blocks ------------------------------------------------------------------------------------


def _crafted(script, sps=100 / 3.0, valid=None, signs=None, **kwargs):
    """rows, levels, nid, info, rec of a station's ``script``, one frame behind the other, through the oracle's coders alone."""
    rng = np.random.default_rng(5)
    rows, words, at = [], [], 0
    for j, item in enumerate(script):
        dibits = PM.make_frame(item, kwargs.get("nac", PM.NAC), rng)
        words.append(PM.words_of_dibits(dibits))
        rows.append((int(round(at * sps)), 1 if signs is None else signs[j]))
        at += len(dibits) + (kwargs.get("gaps", {}).get(j, 0))
    rows = np.array(rows, dtype=np.int64).reshape(-1, 2)
    levels = np.array([[1000, 0, 864 if valid is None else valid[j]] for j in range(len(rows))], dtype=np.int64).reshape(-1, 3)
    nid = PM.apply_flags(PM.nid_all(words), levels)
    info, rec = PM.decode_all(words, PM.decoder_duids(nid))
    return rows, levels, nid, info, rec


def _both(script, **kwargs):
    """The package's frames, calls and blocks of ``script`` as objects, asserted equal to the oracle's."""
    rows, levels, nid, info, rec = _crafted(script, **kwargs)
    np.testing.assert_array_equal(nid, X.apply_flags(nid, levels))
    assert X.decoder_duids(nid).tolist() == PM.decoder_duids(nid)
    frames, counts = X.parse_frames(rows, levels, nid, info, rec, FS)
    want, want_counts = PM.parse(rows, levels, nid, info, rec, FS)
    assert [f.to_json() for f in frames] == want and counts == want_counts
    calls, tsbks = X.track_calls(frames), X.collapse_tsbks(frames)
    assert [c.to_json() for c in calls] == PM.track(want) and [t.to_json() for t in tsbks] == PM.collapse(want)
    return frames, counts, calls, tsbks


CLEAN = dict(no_level=0, cut=0, nid_refused=0, nid_fixed=0, lc_failed=0, crc_failed=0, golay_refused=0, hamming_unmatched=0)


def test_parser_calls_and_blocks_on_the_test_script():
    frames, counts, calls, tsbks = _both(PM.SCRIPT)
    assert counts == CLEAN and [f.name for f in frames] == ["hdu", "ldu1", "ldu2", "ldu1", "ldu2", "tdulc"] + ["tsbk"] * 6
    (call,) = calls
    assert (call.nac, call.group, call.src, call.dst, call.ldus, call.terminated) == (PM.NAC, True, PM.SRC, PM.TG, 4, True)
    assert call.line() == "P25 nac=0x293 group 2345678 -> 9 0.80 s (4 ldus)"
    assert [(t.opcode, t.mfid, t.count) for t in tsbks] == [(0x3D, 0, 1), (0x3B, 0, 3), (0x3A, 0, 3), (0x00, 0, 3), (0x29, 0x90, 2)]
    assert [t.line() for t in tsbks] == [
        "P25 nac=0x293 tsbk identifier update id 1 base 849.7625 MHz spacing 12.5 kHz x1",
        "P25 nac=0x293 tsbk network status wacn 0xbee00 system 0x293 ch 0x1001 (849.7750 MHz) x3",
        "P25 nac=0x293 tsbk rfss status system 0x293 rfss 1 site 2 ch 0x1001 (849.7750 MHz) x3",
        "P25 nac=0x293 tsbk group grant tg 9 src 2345678 ch 0x1064 (851.0125 MHz) x3",
        "P25 nac=0x293 tsbk o=0x29 mfid=0x90 0123456789abcdef x2"]
    assert tsbks[1].first_s < tsbks[1].last_s and frames[1].line() == "P25 nac=0x293 ldu1 group 2345678 -> 9"
    # without its identifier update a channel has no frequency
    _, _, _, tsbks = _both([PM.TSBK_THREE])
    assert [t.line() for t in tsbks][2] == "P25 nac=0x293 tsbk group grant tg 9 src 2345678 ch 0x1064 x1"


def test_tsbk_fields_and_frequencies():
    assert X.tsbk_fields(0x00, 0, PM.GRANT) == dict(kind="group grant", svc=0, channel=PM.VOICE, tgid=PM.TG, src=PM.SRC)
    assert X.tsbk_fields(0x02, 0, 0x1064_0009_1065_000A) == dict(kind="grant update", channel=0x1064, tgid=9, channel2=0x1065, tgid2=10)
    assert X.tsbk_fields(0x3A, 0, PM.RFSS_ARGS) == dict(kind="rfss status", lra=0, flags=0, system=PM.SYSTEM, rfss=PM.RFSS, site=PM.SITE,
                                                        channel=PM.CONTROL, svc=0x70)
    assert X.tsbk_fields(0x3B, 0, PM.NET) == dict(kind="network status", lra=0, wacn=PM.WACN, system=PM.SYSTEM, channel=PM.CONTROL, svc=0x70)
    assert X.tsbk_fields(0x3D, 0, PM.IDEN) == dict(kind="identifier update", id=1, bandwidth=100, tx_offset=180, spacing=100, base=169_952_500)
    assert X.tsbk_fields(0x3D, 0x90, PM.IDEN) == {} and X.tsbk_fields(0x29, 0, 5) == {}
    idens = {1: (169_952_500, 100)}
    assert X.channel_hz(0x1064, idens) == 851_012_500 and X.channel_hz(0x2064, idens) is None and X.channel_hz(0x1000, idens) == 849_762_500
    assert X.tsbk_text(0x02, 0, 0x1064_0009_2065_000A, idens) == "grant update tg 9 ch 0x1064 (851.0125 MHz), tg 10 ch 0x2065"
    for args in ((0x00, 0, PM.GRANT), (0x02, 0, 0x1064_0009_2065_000A), (0x3A, 0, PM.RFSS_ARGS), (0x3B, 0, PM.NET), (0x3D, 0, PM.IDEN), (0x29, 0x90, 7)):
        assert X.tsbk_text(*args, idens) == PM.tsbk_text(*args, idens) and X.tsbk_text(*args, {}) == PM.tsbk_text(*args, {})


def test_late_entry_hang_changed_ids_and_terminators():
    other = PM.lc_hexbits(3, 111, 222)
    # a late entry (LDU2s alone, then silence beyond the hang), then a call whose ids change, ended by a TDU
    script = [("ldu2",), ("ldu2",), ("ldu1", PM.LC), ("ldu2",), ("ldu1", other), ("ldu2",), ("tdu",), ("tdulc", PM.LC)]
    frames, counts, calls, _ = _both(script, gaps={1: int(0.4 * 4800)})
    assert counts == CLEAN and len(calls) == 3
    late, first, second = calls
    assert (late.group, late.src, late.dst, late.ldus, late.terminated) == (None, None, None, 2, False)
    assert late.end_s == frames[1].time_s and "late entry" in late.line() and late.line().endswith("(2 ldus, not terminated)")
    assert (first.group, first.src, first.dst, first.ldus, first.terminated) == (True, PM.SRC, PM.TG, 2, False) and first.end_s == frames[3].time_s
    assert (second.group, second.src, second.dst, second.ldus, second.terminated) == (False, 111, 222, 2, True) and second.end_s == frames[6].time_s
    assert second.line().startswith("P25 nac=0x293 unit 111 -> 222 ")  # the TDULC behind the TDU finds no call open and opens none
    # within the hang the call goes on: a gap of 0.17 s behind an LDU (0.18 s) is 0.35 s between sync words
    _, _, calls, _ = _both([("ldu1", PM.LC), ("ldu2",), ("tdulc", PM.LC)], gaps={0: int(0.17 * 4800)})
    assert len(calls) == 1 and (calls[0].ldus, calls[0].terminated) == (2, True)
    # a TDULC names the ids of a late entry before it closes it
    _, _, calls, _ = _both([("ldu2",), ("tdulc", PM.LC)])
    assert len(calls) == 1 and (calls[0].group, calls[0].src, calls[0].terminated) == (True, PM.SRC, True)


def test_failed_refused_cut_and_inverted_frames():
    bad = PM.lc_hexbits(0, 1, 2, break_rs=True)
    script = [("hdu",), ("ldu1", bad), ("ldu1", PM.LC), ("ldu1", PM.LC), ("tdulc", PM.LC), ("tsbk", [PM.tsbk_bytes(0x3B, 0, PM.NET, break_crc=True),
                                                                                                    PM.tsbk_bytes(0x3A, 0, PM.RFSS_ARGS, lb=1)]
                                                                                          + [PM.tsbk_bytes(0x00, 0, PM.GRANT)]), PM.TSBK_THREE, ("tdu",), ("hdu",)]
    valid = [864, 864, 698, 864, 204, 864, 258, 56, 864]
    rows, levels, nid, info, rec = _crafted(script, valid=valid, signs=[-1] * 9)
    levels[8] = (0, 5, 864)  # no level
    frames, counts = X.parse_frames(rows, levels, nid, info, rec, FS)
    want, want_counts = PM.parse(rows, levels, nid, info, rec, FS)
    assert [f.to_json() for f in frames] == want and counts == want_counts
    assert counts == dict(CLEAN, lc_failed=1, cut=4, crc_failed=1, no_level=1)
    assert [(f.name, f.checked) for f in frames] == [("hdu", None), ("ldu1", False), ("ldu1", None), ("ldu1", True), ("tdulc", None), ("tsbk", None), ("tsbk", None)]
    assert frames[1].src is None and frames[1].line() == "P25 nac=0x293 ldu1 (failed)"
    assert [ok for _, ok in frames[5].blocks] == [False, True] and len(frames[6].blocks) == 1  # the LB bit ends a frame; a cut one ends at the cut
    tsbks = X.collapse_tsbks(frames)
    assert [(t.opcode, t.count) for t in tsbks] == [(0x3A, 1), (0x3B, 1)]  # the failed block is left out
    (call,) = X.track_calls(frames)
    assert (call.group, call.src, call.ldus, call.terminated) == (True, PM.SRC, 3, True)  # the failed LC names nobody
    # a refused NID is counted and left out; a corrected one is counted and kept
    rows, levels, nid, info, rec = _crafted([("tdu",), ("tdu",)])
    nid[0] = (2, 14, 0x1234, 1)
    nid[1, :2] = (1, 3)
    frames, counts = X.parse_frames(rows, levels, nid, info, rec, FS)
    assert counts == dict(CLEAN, nid_refused=1, nid_fixed=1) and len(frames) == 1 and frames[0].corrected
    # the channel: inverted where most hits are negative
    st = dict(rows=rows, levels=levels, nid=PM.apply_flags(PM.nid_all([PM.words_of_dibits(PM.make_frame(("tdu",), 5, None))] * 2), levels), info=info, rec=rec)
    assert X.channel_of(st, FS, 0, 0.0, None).inverted is False and X.channel_of(st, FS, 0, 0.0, None).nacs == {"0x005": 2}
    st["rows"] = rows * np.array([1, -1])
    assert X.channel_of(st, FS, 0, 0.0, None).inverted is True and X.channel_of(st, FS, 0, 0.0, None).frames == {"tdu": 2}


def test_frame_hits_keeps_the_larger_of_two_near_hits():
    pats = A.identify.patterns_for(4800)
    p = [j for j, pat in enumerate(pats) if pat.protocol == "p25"][0]
    hits = [(p, 1000, -50, 9, 0, 0), (p, 1010, 40, 9, 0, 0), (p, 1016, 50, 9, 0, 0), (0, 1000, 999, 9, 0, 0), (p, 3000, 7, 9, 0, 0)]
    got = X.frame_hits(np.array(hits, dtype=np.int64), pats, 16)
    want = PM.frame_hits([(0,) + h[1:] for h in hits if h[0] == p], 16)
    assert got.tolist() == [list(r) for r in want] == [[1000, -1], [3000, 1]]
    assert X.frame_hits(np.array(hits, dtype=np.int64), pats, 15).tolist() == [[1000, -1], [1016, 1], [3000, 1]]
    assert X.frame_hits(np.zeros((0, 6), dtype=np.int64), pats, 16).shape == (0, 2)


def test_result_round_trips_through_json():
    frames, counts, calls, tsbks = _both(PM.SCRIPT)
    ch = X.P25Channel(offset_hz=200e3, freq_hz=851012500.0, nacs={"0x293": 12}, frames={"tsbk": 6}, calls=calls, tsbks=tsbks, inverted=True, **counts)
    res = X.P25Result(channels=[ch, X.P25Channel(offset_hz=1.0, freq_hz=None, note="no p25 channel")], sample_rate=2.4e6, center_freq=850812500.0)
    assert X.P25Result.from_json(json.loads(json.dumps(res.to_json()))) == res
    assert res.lines()[0] == "851012500 Hz: P25 nac=0x293 group 2345678 -> 9 0.80 s (4 ldus)" and len(res.lines()) == 6
    assert res.lines()[4] == "851012500 Hz: P25 nac=0x293 tsbk group grant tg 9 src 2345678 ch 0x1064 (851.0125 MHz) x3"
    assert res.calls == calls and ch.to_json()["tsbks"][1]["count"] == 3
    assert X.P25Frame.from_json(json.loads(json.dumps(frames[7].to_json()))) == frames[7]
    assert all(hasattr(cls, "to_json") and (hasattr(cls, "line") or hasattr(cls, "lines")) for cls in (X.P25Frame, X.P25Call, X.P25Tsbk, X.P25Channel, X.P25Result))


# ---- the layer table, the CLI, the package surface, the C ABI -----------------------------------------------------------------------


def test_the_branches_of_the_layer_table():
    assert [l.name for l in FL.FIND_BRANCHES[:2]] == ["dmr", "p25"]  # the rows before this one stay where they were
    (row,) = [l for l in FL.FIND_BRANCHES if l.name == "p25"]
    assert FL.FIND_BRANCHES.index(row) == 1
    assert (row.name, row.flag, row.section, row.suffix, row.inline, row.needs, row.option) == ("p25", "find_p25", 31, "p25", False, "identify", "--find-p25")
    on = dict(describe=True, keying=True, identify=True)
    assert [l.name for l in FL.active_layers({**on, "p25": True})] == ["describe", "keying", "identify", "p25"]
    assert [l.name for l in FL.active_layers({**on, "flex": True, "dmr": True, "p25": True})] == ["describe", "keying", "identify", "flex", "dmr", "p25"]
    assert [l.name for l in FL.active_layers(on)] == ["describe", "keying", "identify"]
    with pytest.raises(ValueError, match="p25=True needs identify=True"):
        FL.active_layers(dict(describe=True, keying=True, p25=True))
    with pytest.raises(ValueError, match="identify=True needs keying=True"):  # the chain's own errors come first
        FL.active_layers(dict(describe=True, identify=True, p25=True))
    plan = P.plan_find(2.4e6, 100_000)
    fin = dict(runs=np.zeros((0, 8), dtype=np.int64), on=np.zeros((0, plan.slices), dtype=np.uint8))
    with pytest.raises(ValueError, match="p25=True needs identify=True"):
        DS.ChannelDescriber(plan, fin, [], keying=True, p25=True)
    with pytest.raises(ValueError, match="p25=True needs identify=True"):
        A.find_channels("nothing.wav", describe=True, keying=True, p25=True)
    with pytest.raises(ValueError, match="the describer was made without p25=True"):
        DS.ChannelDescriber(plan, fin, [], keying=True, identify=True, dmr=True).finish_p25()
    assert DS.ChannelDescriber(plan, fin, [], keying=True, identify=True, dmr=True, p25=True)._names == ("describe", "keying", "identify", "dmr", "p25")


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        cli.main(argv)
    assert exc.value.code == 2
    return capsys.readouterr().err


def test_cli_flags(capsys):
    base = ["--in", "capture.wav"]
    args = cli.build_parser().parse_args(base + ["--find-p25"])
    assert (args.find_p25, args.find_identify, args.find_dmr) == (True, False, False)
    assert cli.check_find_args(cli.build_parser(), args) is True
    assert (args.find_p25, args.find_identify, args.find_decode, args.find_flex, args.find_dmr, args.find_describe) == (True, True, True, False, False, False)
    args = cli.build_parser().parse_args(base + ["--find-dmr"])
    assert cli.check_find_args(cli.build_parser(), args) is True and args.find_p25 is False
    args = cli.build_parser().parse_args(base + ["--find-flex", "--find-dmr", "--find-p25"])
    assert cli.check_find_args(cli.build_parser(), args) is True
    assert (args.find_p25, args.find_dmr, args.find_flex, args.find_identify) == (True, True, True, True)
    assert "--find-p25 cannot be combined with --ft." in _usage_error(base + ["--find-p25", "--ft", "455800000"], capsys)
    assert "--find-p25 needs --in." in _usage_error(["--find-p25"], capsys)
    assert "--find-auto needs --find-top." in _usage_error(base + ["--find-p25", "--find-auto"], capsys)
    text = "".join(cli.build_parser().format_help().split())
    (row,) = [l for l in FL.FIND_BRANCHES if l.name == "p25"]
    assert "--find-p25" in text and "".join(row.help.split()) in text


def test_package_surface():
    for name in ("P25Frame", "P25Call", "P25Tsbk", "P25Result", "P25Decoder"):
        assert getattr(A, name) is getattr(X, name)
    text = Path(X.__file__).read_text()
    assert "scipy" not in text and "import oracle" not in text and "from oracle" not in text
    for name in ("slice_frames", "decode_nids", "decode_frames", "frame_hits", "apply_flags", "check_lc", "check_tsbk", "parse_frames", "track_calls",
                 "collapse_tsbks", "decode_stream", "channel_of", "finish_p25", "p25_result", "stage_keys"):
        assert callable(getattr(X, name))


def test_c_abi_refuses_bad_arguments():
    """The library has the three entry points, and the argument checks come before the launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some = c_void_p(0), c_void_p(8)  # (never dereferenced: every call below is refused, or has nothing to do)
    for name in ("iqa_p25_slice", "iqa_p25_nid", "iqa_p25_decode"):
        assert hasattr(N.lib(), name) and name in N.EXPORTS
    assert N.lib().iqa_abi_version() == 1
    plan = P.plan_p25(FS)

    def slice_(plane=some, n=100_000, hits=some, k=2, offsets=plan.offsets, bits=some, levels=some):
        off = None if offsets is None else (c_int32 * 864)(*offsets)
        N.call("iqa_p25_slice", plane, c_int64(n), hits, c_int64(k), off, bits, levels, null)

    def offs(at, value):
        o = list(plan.offsets)
        o[at] = value
        return tuple(o)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(k=-1), "negative"), (dict(n=(1 << 30) + 1), "2\\^30"), (dict(k=(1 << 20) + 1), "2\\^20"),
                         (dict(offsets=None), "NULL offsets"), (dict(offsets=offs(0, 1)), "o\\[0\\]"), (dict(offsets=offs(40, -9000)), "ascend"),
                         (dict(offsets=offs(863, plan.offsets[862] + 226)), "step"), (dict(plane=null), "NULL"), (dict(hits=null), "NULL"),
                         (dict(bits=null), "NULL"), (dict(levels=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            slice_(**kwargs)
    slice_(plane=null, hits=null, bits=null, levels=null, n=0)  # nothing to do: no pointer is touched
    slice_(plane=null, hits=null, bits=null, levels=null, k=0)

    def nid(bits=some, k=2, out=some):
        N.call("iqa_p25_nid", bits, c_int64(k), out, null)

    for kwargs, what in ((dict(k=-1), "negative"), (dict(k=(1 << 20) + 1), "2\\^20"), (dict(bits=null), "NULL"), (dict(out=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            nid(**kwargs)
    nid(bits=null, out=null, k=0)

    def decode(bits=some, duids=some, k=2, info=some, rec=some):
        N.call("iqa_p25_decode", bits, duids, c_int64(k), info, rec, null)

    for kwargs, what in ((dict(k=-1), "negative"), (dict(k=(1 << 20) + 1), "2\\^20"), (dict(bits=null), "NULL"), (dict(duids=null), "NULL"),
                         (dict(info=null), "NULL"), (dict(rec=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            decode(**kwargs)
    decode(bits=null, duids=null, info=null, rec=null, k=0)

    # the sign of a hit and the DUID lie in device memory for the kernels: the package checks them before anything is launched
    class Plane:
        def numel(self):
            raise AssertionError("checked before the plane is looked at")

    for rows in ([(100, 0)], [(100, 2)], [(100, -3)]):
        with pytest.raises(ValueError, match="sign must be \\+-1"):
            X.slice_frames(Plane(), rows, plan)
    with pytest.raises(ValueError, match="a DUID must be 0 .. 15"):
        X.decode_frames(np.zeros((1, 54), dtype=np.uint32), [16])
    with pytest.raises(ValueError, match="one DUID to a frame"):
        X.decode_frames(np.zeros((2, 54), dtype=np.uint32), [1])


# ---- the oracle end to end ----------------------------------------------------------------------------------------------------------


def _strip(frames):
    return [{k: v for k, v in f.items() if k not in ("corrected", "time_s")} for f in frames]


@pytest.fixture(scope="module")
def clean():
    return PM.decode_theta(PM.test_stream(FS), FS)


@pytest.mark.parametrize("case", ["clean", "noise", "negated"])
def test_oracle_end_to_end(clean, case):
    out = clean if case == "clean" else PM.decode_theta(PM.test_stream(FS, noise=NOISE if case == "noise" else 0.0, negate=case == "negated"), FS)
    assert len(out["rows"]) == 12 and set(out["rows"][:, 1].tolist()) == ({-1} if case == "negated" else {1})
    assert case == "noise" or out["rows"][:, 0].tolist() == clean["rows"][:, 0].tolist()
    assert np.abs(out["rows"][:, 0] - clean["rows"][:, 0]).max() <= 1
    assert out["counts"] == dict(CLEAN, nid_fixed=out["counts"]["nid_fixed"]) and _strip(out["frames"]) == _strip(clean["frames"])
    assert [f["name"] for f in out["frames"]] == ["hdu", "ldu1", "ldu2", "ldu1", "ldu2", "tdulc"] + ["tsbk"] * 6
    (call,) = out["calls"]
    assert (call["nac"], call["group"], call["src"], call["dst"], call["ldus"], call["terminated"]) == (PM.NAC, True, PM.SRC, PM.TG, 4, True)
    assert [(t["opcode"], t["count"]) for t in out["tsbks"]] == [(0x3D, 1), (0x3B, 3), (0x3A, 3), (0x00, 3), (0x29, 2)]
    assert [len(f["blocks"]) for f in out["frames"][6:]] == [1, 3, 3, 1, 3, 1] and all(ok for f in out["frames"] for _, ok in f["blocks"])
    read = [j for j, d in enumerate(PM.decoder_duids(out["nid"])) if d in (0x5, 0xF)]
    nid_bits, words = int(out["nid"][:, 1].sum()), int(out["rec"][read, 1].sum())
    trellis = sum(int(out["rec"][j, 1 + b]) for j, f in enumerate(out["frames"]) for b in range(len(f["blocks"])))
    print(case, "nid bits", nid_bits, "nid fixed", out["counts"]["nid_fixed"], "hamming and golay words corrected", words, "trellis bits", trellis)
    if case == "noise":
        assert nid_bits > 0 and words > 0 and trellis > 0
    else:
        assert nid_bits == 0 and words == 0 and trellis == 0 and out["counts"]["nid_fixed"] == 0
    if case == "negated":
        np.testing.assert_array_equal(out["v"], -clean["v"])  # (no shift at this rate: the plane is the clean one negated)
        np.testing.assert_array_equal(out["bits"], clean["bits"])
        assert out["frames"] == clean["frames"] and out["calls"] == clean["calls"] and out["tsbks"] == clean["tsbks"]
    # the two forms of the slicing agree, here and at the stream's ends
    pl = out["plan"]
    n = len(out["v"])
    rows = np.concatenate([out["rows"], [(5, 1), (n - 3, -1), (n - pl["o"][56] - 1, 1), (n - pl["o"][56], -1), (-1, 1), (n + 5, 1)]])
    bits, levels = PM.slice_all(out["v"], rows, pl)
    for j, (m, s) in enumerate(rows.tolist()):
        w, lev = PM.slice_by_loops(out["v"], n, m, s, pl)
        assert bits[j].tolist() == w and levels[j].tolist() == lev, j
    assert levels[-6:, 2].tolist() == [864, 1, 57, 56, 0, 0]


def test_the_next_noise_level_loses_a_frame():
    out = PM.decode_theta(PM.test_stream(FS, noise=NOISE + 0.01), FS)
    c = out["counts"]
    assert c["lc_failed"] + c["crc_failed"] + c["nid_refused"] > 0 or _strip(out["frames"]) != _strip(PM.decode_theta(PM.test_stream(FS), FS)["frames"])


def test_model_capture_reads_fsk_4800_and_p25():
    """The model capture of the GPU test's CLI run, through the numpy finder, the float64 channelizer, section 23's keying and
    section 25's identification: it reads ``fsk 4800`` and ``p25``, and the oracle finds the call and the blocks."""
    p25, voice = PM.model_run()
    assert p25["keyed"]["label"] == "fsk 4800" and voice["keyed"]["label"] == "unkeyed" and voice["p25"] is None
    assert (p25["named"]["protocol"], p25["named"]["confirmed"]) == ("p25", True)
    assert 4.0 <= p25["described"]["plan"]["fs_ch"] / 4800.0 <= 224.0
    out = p25["p25"]
    (call,) = out["calls"]
    assert (call["nac"], call["group"], call["src"], call["dst"], call["ldus"], call["terminated"]) == (PM.NAC, True, PM.SRC, PM.TG, 4, True)
    # (the capture opens with the control channel's frame, so its blocks come first; the last frame is cut behind its second block)
    assert [(t["opcode"], t["mfid"], t["count"]) for t in out["tsbks"]] == [(0x3B, 0, 14), (0x3A, 0, 14), (0x00, 0, 13), (0x3D, 0, 1), (0x29, 0x90, 2)]
    assert out["tsbks"][2]["text"] == "group grant tg 9 src 2345678 ch 0x1064 (851.0125 MHz)"
    assert out["counts"] == dict(CLEAN, cut=1) and len(out["rows"]) == 23
    assert p25["named"]["hits"]["p25"] == 23 and p25["named"]["pairs"] == {"p25": 22}
