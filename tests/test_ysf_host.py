"""The YSF frame decoding (--find-ysf) without a GPU: the anchors that section 32 states (the sync word's
sums, the convolutional code's impulse, the Golay word of 1, the CRC vector, the whitening bytes), the properties of the codes on
the model's coders, the level rule, ``plan_ysf`` against the model's plan, the package's checks, fields, parser and transmission
tracker against the model's on hand-made frames, the JSON round trip, the layer table's branches, the CLI's flags, the package
surface, the entry points' argument checks, the model end to end on synthesised theta (clean, negated and at the noise level
found here) and the model capture of the GPU test's CLI run through the numpy pipeline."""
from __future__ import annotations

import importlib.util
import itertools
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
from iq_to_audio_amd import ysf as X


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


YM = _load("ysf_model")
FS = 160_000.0
#: radians of white noise on theta: the largest of 0.01, 0.02, ... at which the model alone still decodes every frame of the test
#: stream (found on the CPU: 0.13 loses five data channel blocks to their CRC)
NOISE = 0.12
CLEAN = dict(no_level=0, cut=0, fich_failed=0, golay_refused=0, dch_failed=0, fixed=0)
PN9_20 = bytes([0x93, 0xD7, 0x51, 0x21, 0x9C, 0x2F, 0x6C, 0xD0, 0xEF, 0x0F, 0xF8, 0x3D, 0xF1, 0x73, 0x20, 0x94, 0xED, 0x1E, 0x7C, 0xD8])


# ---- the anchors ----------------------------------------------------------------------------------------------------------------------


def test_constants_are_the_models():
    assert X.SYNC == YM.SYNC == 0xD471C9634D and [(p.protocol, p.word, p.symbols) for p in X.YSF_PATTERNS] == [(p[0], p[3], p[4]) for p in YM.YSF_PATTERNS]
    assert (X.SYNC_SYMBOLS, X.LEVEL_SCALE, X.GOLAY_POLY, X.HANG_S, X.NEED_FICH, X.NEED_DCH) == (20, YM.SCALE, YM.GOLAY_POLY, YM.HANG_S, YM.NEED_FICH, YM.NEED_DCH)
    assert (P.YSF_OFFSETS, P.YSF_WORDS, P.YSF_FICH_RECORD, P.YSF_INFO, P.YSF_RECORD) == (YM.OFFSETS, YM.WORDS, YM.FICH_RECORD, YM.INFO, YM.RECORD) == (480, 30, 5, 12, 4)
    assert X.PLANE_RATES == (4800,) and X.GOLAY_MAX_DISTANCE == 3 and X.CRC_POLY == 0x1021 and X.DT == YM.MODES and X.FIELDS == YM.FIELDS
    header = (Path(__file__).resolve().parent.parent / "include" / "iqa_hotpath.h").read_text()
    for text in ("#define IQA_YSF_OFFSETS 480", "#define IQA_YSF_WORDS 30", "#define IQA_YSF_FICH_RECORD 5", "#define IQA_YSF_INFO 12",
                 "#define IQA_YSF_RECORD 4", "#define IQA_ABI_VERSION 1"):
        assert text in header


def test_the_five_anchors():
    lev = YM.sync_levels()
    assert lev == [-3, 3, 3, 1, 3, -3, 1, 3, -3, 1, -1, 3, 3, -1, 1, -3, 3, 1, -3, 3] == list(A.identify.symbols_of(X.YSF_PATTERNS[0]))
    assert sum(lev) == 12 and sum(x * x for x in lev) == 124 and 20 * 124 - 12 * 12 == 4 * 584
    assert YM.conv_encode([1])[:10] == [1, 1, 0, 1, 0, 1, 1, 0, 1, 1]  # the dibits 11 01 01 10 11
    assert YM.golay(1) == 0x0018EB
    assert YM.crc16(b"123456789") == X.crc16(b"123456789") == 0xCE3C
    assert YM.pn9(20) == X.pn9(20) == PN9_20 == YM.PN9_20
    bits = YM.bytes_bits(PN9_20)
    assert bits[:9] == [1, 0, 0, 1, 0, 0, 1, 1, 1] == list(X.PN9_FIRST) and all(bits[n] == bits[n - 5] ^ bits[n - 9] for n in range(9, 160))
    data = bytes(range(40, 60))
    assert X.dewhiten(bytes(YM.whiten(data))) == data and X.dewhiten(data[:10]) == bytes(YM.whiten(data[:10]))


# ---- the properties of the codes ----------------------------------------------------------------------------------------------------------


def test_the_interleave_is_a_permutation():
    for rows in (5, 9):
        at = [YM.interleave_at(i, rows) for i in range(20 * rows)]
        assert sorted(at) == list(range(20 * rows)) and X.INTERLEAVE_ROWS[20 * rows] == rows
        bits = np.random.default_rng(rows).integers(0, 2, 40 * rows).tolist()
        assert YM.deinterleave(YM.interleave(bits, rows), rows) == bits
    assert [YM.interleave_at(i, 5) for i in (0, 1, 4, 5, 99)] == [0, 20, 80, 1, 99] and [YM.interleave_at(i, 9) for i in (1, 8, 9, 179)] == [20, 160, 1, 179]


def test_the_encoder_round_trips_every_class():
    cases = YM.coder_cases()
    for name, item in (("header", YM.header()), ("terminator", YM.header(fi=2)), ("vd1", YM.vd1(0)), ("vd2", YM.vd2(1)), ("data-fr", YM.data_fr(3)),
                       ("voice-fr", YM.voice_fr())):
        words, cls = cases[name]
        assert words[0] == YM.SYNC >> 8 and words[1] >> 24 == YM.SYNC & 0xFF
        two, frec = YM.fich_decode(words)
        assert frec == [0, 0, 0, 0, 0] and YM.word_bytes(two)[:4] == item[0] and YM.fich_ok(two) and X.check_fich(two)
        assert YM.frame_class(item[0]) == cls == X.frame_class(item[0][0] >> 6, item[0][2] & 3)
        info, rec, ties = YM.decode_frame(words, cls)
        assert rec == [cls, 0, 0, 0] and ties == 0
        size = 10 if cls == 3 else 20
        for second, data in enumerate(d for d in item[1:3] if d is not None and cls):
            block = info[6 * second : 6 * second + 6]
            by = YM.word_bytes(block)
            assert YM.whiten(by[:size]) == list(data) and X.check_dch(block, size) and X.dewhiten(by[:size]) == bytes(data)
            assert not any(by[size + 2 :])  # the tail bits and the rest of the block's words are 0
        if cls in (0, 2, 3):
            assert not any(info[6:]) and (cls or not any(info))
    assert all(YM.decode_frame(cases[f"class-{c}"][0], c if c <= 3 else 0)[:2] == ([0] * 12, [0, 0, 0, 0]) for c in (0, 4, 255))


def test_viterbi_corrects_any_two_flipped_channel_bits():
    rng = np.random.default_rng(7)
    for size, rows in ((96, 5), (176, 9)):
        bits = rng.integers(0, 2, size).tolist()
        coded = YM.conv_encode(bits)
        assert len(coded) == 2 * (size + 4) == 40 * rows
        assert YM.viterbi(coded) == (bits + [0] * 4, 0, 0)
        pairs = list(itertools.combinations(range(len(coded)), 2))
        picked = [pairs[k] for k in rng.choice(len(pairs), 150, replace=False)] + [(k, k + 1) for k in range(0, len(coded) - 1, 7)]
        for a, b in picked + [(0, 1), (len(coded) - 2, len(coded) - 1)]:
            bad = list(coded)
            bad[a] ^= 1
            bad[b] ^= 1
            got, metric, _ = YM.viterbi(bad)
            assert got == bits + [0] * 4 and metric == 2, (a, b)
    # the frames' own cases: two flips to a block, anywhere in the frame
    cases = YM.coder_cases()
    clean = YM.decode_frame(*cases["header"])[0]
    for name, (words, cls) in cases.items():
        if name.startswith("dch-two-"):
            info, rec, _ = YM.decode_frame(words, cls)
            assert info == clean and rec == [1, 2, 2, 0], name
        elif name.startswith("fich-two-"):
            assert YM.fich_decode(words) == (YM.fich_decode(cases["header"][0])[0], [1, 2, 0, 0, 0]), name
        elif name.startswith("vd2-two-"):
            assert YM.decode_frame(words, cls)[:2] == (YM.decode_frame(*cases["vd2"])[0], [3, 2, 0, 0]), name


def test_the_tie_rule_matters_on_the_crafted_burst():
    cases = YM.coder_cases()
    words, cls = cases["dch-tie"]
    first, rec, ties = YM.decode_frame(words, cls)
    other = YM.decode_frame(words, cls, smaller=False)
    assert ties > 0 and rec == [1, 4, 0, 0] and other[1] == rec and first != other[0]  # the same metric, other bits: the rule decides
    assert first == YM.decode_frame(*cases["header"])[0]  # here the smaller predecessor is the sent path
    assert YM.decode_frame(*cases["dch-burst"])[1][2] > 0


def test_golay_corrects_three_and_refuses_four():
    assert int(np.bitwise_count(YM.GOLAY[1:]).min()) == 8 and all(int(cw) >> 12 == d for d, cw in enumerate(YM.GOLAY.tolist()))
    rng = np.random.default_rng(3)
    for d in (0, 1, 0xABC, 0xFFF):
        cw = int(YM.GOLAY[d])
        assert YM.golay_decode(cw) == (0, d, False)
        for count in (1, 2, 3, 4):
            for _ in range(20):
                bad = cw
                for k in rng.choice(24, count, replace=False).tolist():
                    bad ^= 1 << k
                dist, value, refused = YM.golay_decode(bad)
                assert (dist, value, refused) == ((count, d, False) if count <= 3 else (4, bad >> 12, True))
    cases = YM.coder_cases()
    four = YM.fich_bytes(fi=1, dt=3, fn=5, ft=6, cm=3, sql=1, sq=99)
    want = {"golay-0000": [0, 0, 0, 0, 0], "golay-3333": [1, 0, 4, 0, 12], "golay-4000": [2, 0, 0, 1, 0], "golay-0403": [2, 0, 1, 1, 3],
            "golay-1234": [2, 0, 3, 1, 6], "golay-4444": [2, 0, 0, 4, 0]}
    for name, rec in want.items():
        two, got = YM.fich_decode(cases[name][0])
        assert got == rec, name
        assert (YM.word_bytes(two)[:4] == four and YM.fich_ok(two)) == (rec[3] == 0), name  # (these refused words lose a data bit)


# ---- the levels and the plan ------------------------------------------------------------------------------------------------------------


def test_the_level_rule_is_exact():
    lev = YM.sync_levels()
    for s in (1, -1):
        for a, dc in ((1000, 0), (1000, 77), (1, -5000), (64 * 65534 // 3, 0), (1_000_000, -123_456), (7, 64 * 65534 - 21)):
            x = [dc + a * s * g for g in lev]
            assert YM.levels_of(x, s) == (584 * 3 * a, 584 * dc)
            assert YM.levels_of(x, -s) == (-584 * 3 * a, 584 * dc)
    # 15 Q at the largest plane values leaves int32 and stays far inside int64
    big = [64 * 65534 if g > 0 else -64 * 65534 for g in lev]
    q = sum(g * x for g, x in zip(lev, big))
    assert 15 * q > 1 << 31 and abs(YM.levels_of(big, 1)[0]) < 1 << 40


@pytest.mark.parametrize("fs_ch", [19_200.0, 160_000.0, 96_600.0, 1_075_200.0])
def test_plan_against_the_model(fs_ch):
    plan, want = P.plan_ysf(fs_ch), YM.plan(fs_ch)
    assert plan.sps == want["sps"] == fs_ch / 4800.0 and len(plan.offsets) == 480
    assert list(plan.offsets) == want["o"] and plan.o(0) == 0 and plan.o(479) == want["o"][479]
    assert (plan.ident.window, plan.ident.half, plan.ident.shift) == (want["ident"]["L"], want["ident"]["h"], want["ident"]["sh"])
    assert plan.ident == P.plan_ident(fs_ch, 4800) and A.plan_ysf is P.plan_ysf
    assert all(0 < b - a <= 225 for a, b in zip(plan.offsets, plan.offsets[1:]))
    if fs_ch == 96_600.0:  # sps 20.125: i = 4 and 12 fall on .5 and go to the even side
        assert (plan.o(4), plan.o(12), plan.o(20), plan.o(28)) == (80, 242, 402, 564)


def test_plan_refuses_rates_that_do_not_fit():
    for fs_ch in (19_199.0, 1_075_201.0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            P.plan_ysf(fs_ch)
    for fs_ch in (19_199.0, 1_075_201.0):
        with pytest.raises(ValueError):
            YM.plan(fs_ch)
        with pytest.raises(ValueError):
            A.YsfDecoder(fs_ch)


# ---- the host rules on hand-made frames -------------------------------------------------------------------------------------------------


def test_fich_fields_frame_class_and_callsign():
    four = YM.fich_bytes(fi=1, cs=2, cm=3, bn=1, bt=2, fn=5, ft=6, dev=1, mr=4, voip=1, dt=2, sql=1, sq=0x55)
    crc = YM.crc16(four)
    words = [int.from_bytes(bytes(four), "big"), crc << 16]
    assert X.check_fich(words) and not X.check_fich([words[0] ^ 1, words[1]]) and not X.check_fich([words[0], words[1] ^ 0x10000])
    assert X.fich_fields(words) == dict(fi=1, cs=2, cm=3, bn=1, bt=2, fn=5, ft=6, dev=1, mr=4, voip=1, dt=2, sql=1, sq=0x55)
    want = {(0, 0): 1, (0, 3): 1, (2, 1): 1, (1, 1): 1, (1, 0): 2, (1, 2): 3, (1, 3): 0, (3, 0): 0, (3, 2): 0}
    for (fi, dt), cls in want.items():
        assert X.frame_class(fi, dt) == cls == YM.frame_class(YM.fich_bytes(fi=fi, dt=dt)), (fi, dt)
    assert X.callsign(b"JA1YOE    ") == "JA1YOE" == YM.callsign(list(b"JA1YOE    ")) and X.callsign(b"  AB  CD  ") == "AB  CD"
    assert X.callsign(b"**********") == "**********" and X.callsign(b"          ") == ""
    for bad in (b"JA1\x00OE    ", b"JA1YOE\x7f   ", bytes([0x80] + [0x20] * 9), b"\nA1YOE    "):
        assert X.callsign(bad) is None and YM.callsign(list(bad)) is None
    for cls, fi, fn, second in itertools.product(range(4), range(4), range(8), (False, True)):
        assert X.block_fields(cls, fi, fn, second) == YM.block_fields(cls, fi, fn, second)
    assert X.block_fields(1, 0, 5, True) == ("downlink", "uplink") and X.block_fields(1, 1, 1, False) == () and X.block_fields(3, 1, 6, False) == ()
    assert X.block_fields(2, 1, 2, False) == ("rem12", "rem34") and X.block_fields(3, 1, 1, False) == ("src",)


def _crafted(script, sps=100 / 3.0, valid=None, signs=None, gaps=None):
    """rows, levels, fich, frec, info, rec of a station's ``script``, one frame behind the other, through the model's coders alone."""
    rng = np.random.default_rng(5)
    rows, words, at = [], [], 0
    for j, item in enumerate(script):
        words.append(YM.words_of_dibits(YM.make_frame(item, rng)))
        rows.append((int(round(at * sps)), 1 if signs is None else signs[j]))
        at += 480 + (gaps or {}).get(j, 0)
    rows = np.array(rows, dtype=np.int64).reshape(-1, 2)
    levels = np.array([[1000, 0, 480 if valid is None else valid[j]] for j in range(len(rows))], dtype=np.int64).reshape(-1, 3)
    fich, frec = YM.fich_all(words)
    frec = YM.apply_flags(frec, levels)
    info, rec = YM.decode_all(words, YM.decoder_classes(fich, frec, levels))
    return rows, levels, fich, frec, info, rec


def _both(script, **kwargs):
    """The package's frames and transmissions of ``script`` as objects, asserted equal to the model's."""
    rows, levels, fich, frec, info, rec = _crafted(script, **kwargs)
    np.testing.assert_array_equal(frec, X.apply_flags(frec, levels))
    assert X.decoder_classes(fich, frec, levels).tolist() == YM.decoder_classes(fich, frec, levels)
    frames, counts = X.parse_frames(rows, levels, fich, frec, info, rec, FS)
    want, want_counts = YM.parse(rows, levels, fich, frec, info, rec, FS)
    assert [f.to_json() for f in frames] == want and counts == want_counts
    txs = X.track_transmissions(frames)
    assert [t.to_json() for t in txs] == YM.track(want) and [t.line() for t in txs] == [YM.tx_line(t) for t in YM.track(want)]
    return frames, counts, txs


def test_header_frames_terminator():
    frames, counts, txs = _both(YM.SCRIPT)
    assert counts == CLEAN and [X.frame_kind(f) for f in frames] == ["header"] + ["V/D2"] * 8 + ["V/D1", "data FR", "voice FR", "terminator"]
    (tx,) = txs
    assert (tx.src, tx.dst, tx.downlink, tx.uplink, tx.rem12, tx.rem34) == (YM.SRC, YM.DST, YM.DOWN, YM.UP, YM.REM12, YM.REM34)
    assert (tx.cm, tx.dt, tx.sq, tx.late, tx.terminated, tx.conflicts, tx.frames) == (0, 2, 42, False, True, 0, 13)
    assert tx.line() == YM.LINE == "YSF JA1YOE -> ALL via JP1YJQ/JP1YJQ-1 group V/D2 sq=42 1.20 s (13 frames)"
    assert frames[0].fields == dict(dst=YM.DST, src=YM.SRC, downlink=YM.DOWN, uplink=YM.UP) and frames[2].fields == dict(src=YM.SRC)
    assert frames[7].fields == {} and frames[7].blocks == [[(b"6" * 10).hex(), True]] and frames[11].blocks == [] and frames[11].cls == 0
    assert frames[2].line() == "YSF communication V/D2 fn=1/7 src=JA1YOE" and frames[12].line().startswith("YSF terminator V/D2 fn=0/7 dst=")


def test_a_late_join_fills_its_fields_from_the_rotation():
    frames, counts, txs = _both([YM.vd2(fn) for fn in (3, 4, 5, 6, 7, 0, 1, 2)])
    (tx,) = txs
    assert counts == CLEAN and (tx.late, tx.terminated, tx.frames) == (True, False, 8)
    assert (tx.src, tx.dst, tx.downlink, tx.uplink) == (YM.SRC, YM.DST, YM.DOWN, YM.UP)
    assert tx.line() == "YSF JA1YOE -> ALL via JP1YJQ/JP1YJQ-1 group V/D2 sq=42 0.70 s (8 frames)"
    # what is not known is left out, not invented
    _, _, (tx,) = _both([YM.vd2(1), YM.vd2(6)])
    assert tx.line() == "YSF JA1YOE group V/D2 sq=42 0.10 s (2 frames)"
    _, _, (tx,) = _both([YM.vd2(3), YM.vd2(0)])
    assert tx.line() == "YSF -> ALL via /JP1YJQ-1 group V/D2 sq=42 0.10 s (2 frames)"
    _, _, (tx,) = _both([(YM.fich_bytes(fi=1, dt=3, cm=3), None, None)])
    assert tx.line() == "YSF individual voice FR sq=off 0.00 s (1 frame)"
    _, _, (tx,) = _both([(YM.fich_bytes(fi=1, dt=0, cm=1, fn=0), YM.callsign_bytes("W1AW") + YM.callsign_bytes("K1ABC"), None)])
    assert tx.line() == "YSF K1ABC -> W1AW V/D1 sq=off 0.00 s (1 frame)"


def test_a_hang_closes_and_two_transmissions():
    script = [YM.header(), YM.vd2(0), YM.vd2(1), YM.header(), YM.vd2(0), YM.header(fi=2), YM.header(), YM.header(fi=2)]
    frames, counts, txs = _both(script, gaps={2: int(0.4 * 4800)})
    assert counts == CLEAN and [(t.frames, t.terminated, t.late) for t in txs] == [(3, False, False), (3, True, False), (2, True, False)]
    assert txs[0].end_s == frames[2].time_s and txs[1].start_s == frames[3].time_s and txs[2].start_s == frames[6].time_s
    # within the hang the transmission goes on: 0.25 s behind a frame (0.1 s) is 0.35 s between sync words
    _, _, txs = _both(script[:3], gaps={1: int(0.25 * 4800)})
    assert len(txs) == 1 and txs[0].frames == 3
    _, _, txs = _both(script[:3], gaps={1: int(0.27 * 4800)})
    assert len(txs) == 2


def test_a_conflict_keeps_the_first_value():
    other = (YM.fich_bytes(fi=1, dt=2, fn=1, ft=7, sql=1, sq=42), YM.callsign_bytes("JA1ZZZ"), None)
    frames, counts, (tx,) = _both([YM.header(), other, YM.vd2(1), other, YM.header(fi=2)])
    assert counts == CLEAN and tx.src == YM.SRC and tx.conflicts == 2 and tx.terminated
    # a field that is not printable is None, keeps its hex, and fills nothing
    ugly = (YM.fich_bytes(fi=1, dt=2, fn=1), [0x4A, 0x00] + [0x20] * 8, None)
    frames, counts, (tx,) = _both([ugly, YM.vd2(0)])
    assert frames[0].fields == dict(src=None) and frames[0].blocks == [["4a00" + "20" * 8, True]] and tx.src is None and tx.conflicts == 0


def test_failed_cut_and_no_level_frames():
    script = [YM.header(break_a=True), YM.vd2(1, break_fich=True), YM.vd2(1, break_a=True), YM.vd2(2), YM.vd2(3), YM.header(fi=2, break_b=True), YM.vd2(0),
              YM.voice_fr()]
    rows, levels, fich, frec, info, rec = _crafted(script, valid=[480, 480, 480, 479, 119, 480, 480, 120])
    levels[6] = (0, 5, 480)  # no level
    frec = YM.apply_flags(frec, levels)
    frames, counts = X.parse_frames(rows, levels, fich, frec, info, rec, FS)
    want, want_counts = YM.parse(rows, levels, fich, frec, info, rec, FS)
    assert [f.to_json() for f in frames] == want and counts == want_counts
    assert counts == dict(CLEAN, dch_failed=3, fich_failed=1, cut=2, no_level=1)
    assert [(X.frame_kind(f), [ok for _, ok in f.blocks]) for f in frames] == [("header", [False, True]), ("V/D2", [False]), ("V/D2", []),
                                                                              ("terminator", [True, False]), ("voice FR", [])]
    assert frames[0].fields == dict(downlink=YM.DOWN, uplink=YM.UP) and frames[3].fields == dict(dst=YM.DST, src=YM.SRC)
    tx, lone = X.track_transmissions(frames)  # (the voice FR frame behind the terminator opens a transmission of its own)
    assert (tx.src, tx.dst, tx.downlink, tx.frames, tx.terminated) == (YM.SRC, YM.DST, YM.DOWN, 4, True)
    assert (lone.src, lone.frames, lone.late, lone.terminated, lone.dt) == (None, 1, True, False, 3)
    assert X.decoder_classes(fich, frec, levels).tolist() == [1, 0, 3, 0, 0, 1, 0, 0]
    # the channel: inverted where most hits are negative; corrected frames are counted
    rows, levels, fich, frec, info, rec = _crafted([YM.header(), YM.header(fi=2)], signs=[-1, -1])
    frec[0, :3] = (1, 2, 0)
    rec[1, 2] = 3
    st = dict(rows=rows, levels=levels, fich=fich, frec=frec, info=info, rec=rec)
    ch = X.channel_of(st, FS, 0, 0.0, None)
    assert ch.inverted is True and ch.fixed == 2 and ch.frames == {"header": 1, "terminator": 1} and len(ch.transmissions) == 1
    st["rows"] = rows * np.array([1, -1])
    assert X.channel_of(st, FS, 0, 0.0, None).inverted is False


def test_frame_hits_keeps_the_larger_of_two_near_hits():
    pats = A.identify.patterns_for(4800)
    p = [j for j, pat in enumerate(pats) if pat.protocol == "ysf"][0]
    hits = [(p, 1000, -50, 9, 0, 0), (p, 1010, 40, 9, 0, 0), (p, 1016, 50, 9, 0, 0), (0, 1000, 999, 9, 0, 0), (p, 3000, 7, 9, 0, 0)]
    got = X.frame_hits(np.array(hits, dtype=np.int64), pats, 16)
    want = YM.frame_hits([(0,) + h[1:] for h in hits if h[0] == p], 16)
    assert got.tolist() == [list(r) for r in want] == [[1000, -1], [3000, 1]]
    assert X.frame_hits(np.array(hits, dtype=np.int64), pats, 15).tolist() == [[1000, -1], [1016, 1], [3000, 1]]
    assert X.frame_hits(np.zeros((0, 6), dtype=np.int64), pats, 16).shape == (0, 2)


def test_result_round_trips_through_json():
    frames, counts, txs = _both(YM.SCRIPT)
    ch = X.YsfChannel(offset_hz=200e3, freq_hz=433200000.0, frames={"header": 1}, transmissions=txs, inverted=True, **counts)
    res = X.YsfResult(channels=[ch, X.YsfChannel(offset_hz=1.0, freq_hz=None, note="no ysf channel")], sample_rate=2.4e6, center_freq=433.0e6)
    assert X.YsfResult.from_json(json.loads(json.dumps(res.to_json()))) == res
    assert res.lines() == ["433200000 Hz: " + YM.LINE] and res.transmissions == txs and ch.to_json()["transmissions"][0]["src"] == YM.SRC
    assert X.YsfFrame.from_json(json.loads(json.dumps(frames[3].to_json()))) == frames[3]
    assert X.YsfTransmission.from_json(json.loads(json.dumps(txs[0].to_json()))) == txs[0]
    assert all(hasattr(cls, "to_json") and (hasattr(cls, "line") or hasattr(cls, "lines")) for cls in (X.YsfFrame, X.YsfTransmission, X.YsfChannel, X.YsfResult))


# ---- the layer table, the CLI, the package surface, the C ABI -----------------------------------------------------------------------


def test_the_branches_of_the_layer_table():
    assert [l.name for l in FL.FIND_BRANCHES[:2]] == ["dmr", "p25"]  # a prefix: the rows before this one stay where they were
    (row,) = [l for l in FL.FIND_BRANCHES if l.name == "ysf"]
    assert FL.FIND_BRANCHES.index(row) == 2
    assert (row.flag, row.section, row.suffix, row.inline, row.needs, row.option) == ("find_ysf", 32, "ysf", False, "identify", "--find-ysf")
    on = dict(describe=True, keying=True, identify=True)
    assert [l.name for l in FL.active_layers({**on, "ysf": True})] == ["describe", "keying", "identify", "ysf"]
    assert [l.name for l in FL.active_layers({**on, "flex": True, "dmr": True, "p25": True, "ysf": True})] == [
        "describe", "keying", "identify", "flex", "dmr", "p25", "ysf"]
    assert [l.name for l in FL.active_layers({**on, "ysf": True, "dmr": True})] == ["describe", "keying", "identify", "dmr", "ysf"]
    assert [l.name for l in FL.active_layers(on)] == ["describe", "keying", "identify"]
    with pytest.raises(ValueError, match="ysf=True needs identify=True"):
        FL.active_layers(dict(describe=True, keying=True, ysf=True))
    with pytest.raises(ValueError, match="identify=True needs keying=True"):  # the chain's own errors come first
        FL.active_layers(dict(describe=True, identify=True, ysf=True))
    plan = P.plan_find(2.4e6, 100_000)
    fin = dict(runs=np.zeros((0, 8), dtype=np.int64), on=np.zeros((0, plan.slices), dtype=np.uint8))
    with pytest.raises(ValueError, match="ysf=True needs identify=True"):
        DS.ChannelDescriber(plan, fin, [], keying=True, ysf=True)
    with pytest.raises(ValueError, match="ysf=True needs identify=True"):
        A.find_channels("nothing.wav", describe=True, keying=True, ysf=True)
    with pytest.raises(ValueError, match="the describer was made without ysf=True"):
        DS.ChannelDescriber(plan, fin, [], keying=True, identify=True, p25=True).finish_ysf()
    assert DS.ChannelDescriber(plan, fin, [], keying=True, identify=True, p25=True, ysf=True)._names == ("describe", "keying", "identify", "p25", "ysf")


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        cli.main(argv)
    assert exc.value.code == 2
    return capsys.readouterr().err


def test_cli_flags(capsys):
    base = ["--in", "capture.wav"]
    args = cli.build_parser().parse_args(base + ["--find-ysf"])
    assert (args.find_ysf, args.find_identify, args.find_p25) == (True, False, False)
    assert cli.check_find_args(cli.build_parser(), args) is True
    assert (args.find_ysf, args.find_identify, args.find_decode, args.find_flex, args.find_dmr, args.find_p25, args.find_describe) == (
        True, True, True, False, False, False, False)
    args = cli.build_parser().parse_args(base + ["--find-p25"])
    assert cli.check_find_args(cli.build_parser(), args) is True and args.find_ysf is False
    args = cli.build_parser().parse_args(base + ["--find-flex", "--find-dmr", "--find-p25", "--find-ysf"])
    assert cli.check_find_args(cli.build_parser(), args) is True
    assert (args.find_ysf, args.find_p25, args.find_dmr, args.find_flex, args.find_identify) == (True, True, True, True, True)
    assert "--find-ysf cannot be combined with --ft." in _usage_error(base + ["--find-ysf", "--ft", "433200000"], capsys)
    assert "--find-ysf needs --in." in _usage_error(["--find-ysf"], capsys)
    assert "--find-auto needs --find-top." in _usage_error(base + ["--find-ysf", "--find-auto"], capsys)
    text = "".join(cli.build_parser().format_help().split())
    (row,) = [l for l in FL.FIND_BRANCHES if l.name == "ysf"]
    assert "--find-ysf" in text and "".join(row.help.split()) in text


def test_package_surface():
    for name in ("YsfFrame", "YsfTransmission", "YsfChannel", "YsfResult", "YsfDecoder"):
        assert getattr(A, name) is getattr(X, name)
    text = Path(X.__file__).read_text()
    assert "scipy" not in text and "import oracle" not in text and "from oracle" not in text
    doc = " ".join(X.__doc__.split())
    assert "from memory" in doc and "Not decoded: the voice" in doc and "DT1" in doc  # where the constants come from, and what is left out
    for name in ("slice_frames", "decode_fich", "decode_frames", "frame_hits", "apply_flags", "check_fich", "fich_fields", "frame_class", "check_dch",
                 "dewhiten", "callsign", "parse_frames", "track_transmissions", "decode_stream", "channel_of", "finish_ysf", "ysf_result", "stage_keys"):
        assert callable(getattr(X, name))


def test_c_abi_refuses_bad_arguments():
    """The library has the three entry points, and the argument checks come before the launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some = c_void_p(0), c_void_p(8)  # (never dereferenced: every call below is refused, or has nothing to do)
    for name in ("iqa_ysf_slice", "iqa_ysf_fich", "iqa_ysf_decode"):
        assert hasattr(N.lib(), name) and name in N.EXPORTS
    assert N.lib().iqa_abi_version() == 1
    plan = P.plan_ysf(FS)

    def slice_(plane=some, n=100_000, hits=some, k=2, offsets=plan.offsets, bits=some, levels=some):
        off = None if offsets is None else (c_int32 * 480)(*offsets)
        N.call("iqa_ysf_slice", plane, c_int64(n), hits, c_int64(k), off, bits, levels, null)

    def offs(at, value):
        o = list(plan.offsets)
        o[at] = value
        return tuple(o)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(k=-1), "negative"), (dict(n=(1 << 30) + 1), "2\\^30"), (dict(k=(1 << 20) + 1), "2\\^20"),
                         (dict(offsets=None), "NULL offsets"), (dict(offsets=offs(0, 1)), "o\\[0\\]"), (dict(offsets=offs(40, -9000)), "ascend"),
                         (dict(offsets=offs(479, plan.offsets[478] + 226)), "step"), (dict(plane=null), "NULL"), (dict(hits=null), "NULL"),
                         (dict(bits=null), "NULL"), (dict(levels=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            slice_(**kwargs)
    slice_(plane=null, hits=null, bits=null, levels=null, n=0)  # nothing to do: no pointer is touched
    slice_(plane=null, hits=null, bits=null, levels=null, k=0)

    def fich(bits=some, k=2, out=some, rec=some):
        N.call("iqa_ysf_fich", bits, c_int64(k), out, rec, null)

    for kwargs, what in ((dict(k=-1), "negative"), (dict(k=(1 << 20) + 1), "2\\^20"), (dict(bits=null), "NULL"), (dict(out=null), "NULL"),
                         (dict(rec=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            fich(**kwargs)
    fich(bits=null, out=null, rec=null, k=0)

    def decode(bits=some, classes=some, k=2, info=some, rec=some):
        N.call("iqa_ysf_decode", bits, classes, c_int64(k), info, rec, null)

    for kwargs, what in ((dict(k=-1), "negative"), (dict(k=(1 << 20) + 1), "2\\^20"), (dict(bits=null), "NULL"), (dict(classes=null), "NULL"),
                         (dict(info=null), "NULL"), (dict(rec=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            decode(**kwargs)
    decode(bits=null, classes=null, info=null, rec=null, k=0)

    # the sign of a hit and the class lie in device memory for the kernels: the package checks them before anything is launched
    class Plane:
        def numel(self):
            raise AssertionError("checked before the plane is looked at")

    for rows in ([(100, 0)], [(100, 2)], [(100, -3)]):
        with pytest.raises(ValueError, match="sign must be \\+-1"):
            X.slice_frames(Plane(), rows, plan)
    for bad in ([4], [-1], [255]):
        with pytest.raises(ValueError, match="a class must be 0 .. 3"):
            X.decode_frames(np.zeros((1, 30), dtype=np.uint32), bad)
    with pytest.raises(ValueError, match="one class to a frame"):
        X.decode_frames(np.zeros((2, 30), dtype=np.uint32), [1])


# ---- the model end to end ----------------------------------------------------------------------------------------------------------


def _strip(frames):
    return [{k: v for k, v in f.items() if k not in ("corrected", "time_s")} for f in frames]


@pytest.fixture(scope="module")
def clean():
    return YM.decode_theta(YM.test_stream(FS), FS)


@pytest.mark.parametrize("case", ["clean", "noise", "negated"])
def test_model_end_to_end(clean, case):
    out = clean if case == "clean" else YM.decode_theta(YM.test_stream(FS, noise=NOISE if case == "noise" else 0.0, negate=case == "negated"), FS)
    assert len(out["rows"]) == 13 and set(out["rows"][:, 1].tolist()) == ({-1} if case == "negated" else {1})
    assert np.abs(out["rows"][:, 0] - clean["rows"][:, 0]).max() <= (1 if case == "noise" else 0)
    assert _strip(out["frames"]) == _strip(clean["frames"]) and out["classes"].tolist() == [1] + [3] * 8 + [2, 1, 0, 1]
    (tx,) = out["txs"]
    assert YM.tx_line(tx) == YM.LINE and (tx["late"], tx["terminated"], tx["conflicts"]) == (False, True, 0)
    fich_bits, dch_bits = int(out["frec"][:, 1].sum()), int(out["rec"][:, 1:3].sum())
    print(case, "fich bits", fich_bits, "golay refused", out["counts"]["golay_refused"], "dch bits", dch_bits, "fixed", out["counts"]["fixed"])
    if case == "noise":
        assert fich_bits > 0 and dch_bits > 0 and out["counts"]["fixed"] > 0
        assert out["counts"] == dict(CLEAN, fixed=out["counts"]["fixed"], golay_refused=out["counts"]["golay_refused"])
    else:
        assert fich_bits == 0 and dch_bits == 0 and out["counts"] == CLEAN
    if case == "negated":
        np.testing.assert_array_equal(out["v"], -clean["v"])  # (no shift at this rate: the plane is the clean one negated)
        np.testing.assert_array_equal(out["bits"], clean["bits"])
        np.testing.assert_array_equal(out["levels"] * np.array([1, -1, 1]), clean["levels"])
        assert out["frames"] == clean["frames"] and out["txs"] == clean["txs"]
    # the slicing at the stream's ends
    pl = out["plan"]
    n = len(out["v"])
    rows = [(5, 1), (n - 3, -1), (n - pl["o"][119] - 1, 1), (n - pl["o"][119], -1), (-1, 1), (n + 5, 1)]
    _, levels = YM.slice_all(out["v"], rows, pl)
    assert levels[:, 2].tolist() == [480, 1, 120, 119, 0, 0]


def test_the_next_noise_level_loses_a_frame():
    out = YM.decode_theta(YM.test_stream(FS, noise=NOISE + 0.01), FS)
    c = out["counts"]
    assert c["fich_failed"] + c["dch_failed"] > 0 or _strip(out["frames"]) != _strip(YM.decode_theta(YM.test_stream(FS), FS)["frames"])


def test_model_capture_reads_fsk_4800_and_ysf():
    """The model capture of the GPU test's CLI run, through the numpy finder, the float64 channelizer, section 23's keying and
    section 25's identification: it reads ``fsk 4800`` and ``ysf``, and the model finds both transmissions."""
    ysf, voice = YM.model_run()
    assert ysf["keyed"]["label"] == "fsk 4800" and voice["keyed"]["label"] == "unkeyed" and voice["ysf"] is None
    assert (ysf["named"]["protocol"], ysf["named"]["confirmed"]) == ("ysf", True)
    assert 4.0 <= ysf["described"]["plan"]["fs_ch"] / 4800.0 <= 224.0
    out = ysf["ysf"]
    # (480 random symbols lead the capture; the last frame is cut behind its FICH)
    assert [YM.tx_line(t) for t in out["txs"]] == ["YSF JA1YOE -> ALL via JP1YJQ/JP1YJQ-1 group V/D2 sq=42 0.90 s (10 frames)",
                                                  "YSF JA1YOE -> ALL via JP1YJQ/JP1YJQ-1 group V/D2 sq=42 0.80 s (9 frames)"]
    assert [(t["late"], t["terminated"], t["conflicts"]) for t in out["txs"]] == [(False, True, 0), (False, False, 0)]
    assert out["counts"] == dict(CLEAN, cut=1, fixed=out["counts"]["fixed"]) and len(out["rows"]) == 19
    assert ysf["named"]["hits"]["ysf"] == 19 and ysf["named"]["pairs"] == {"ysf": 18}
