"""The FLEX page decoding (--find-flex) without a GPU: the constants of the package against the oracle's
own copy, ``plan_flex`` against the oracle's plan, the encoder of tests/flex_model.py against the package's parser in all four
modes and both polarities, ``choose_shifts`` on its ties, the oracle's two forms against each other, the oracle end to end on
synthesised theta (clean, under noise, with a sample-clock error), the usage errors and the entry points' argument checks."""
from __future__ import annotations

import functools
import importlib.util
import sys
from ctypes import c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest

import iq_to_audio_amd as A
from iq_to_audio_amd import cli
from iq_to_audio_amd import describe as DS
from iq_to_audio_amd import dsp_plan as P
from iq_to_audio_amd import flex as X


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


FM = _load("flex_model")
PM = _load("pocsag_model")
FS = 25_600.0  # sps 16
NOISE = 0.4  # radians of white noise on theta at which the oracle still decodes every page of every mode (found on the CPU)
PPM = 44.0  # the sender's clock error at which shift 0 alone fails in the last block of a 3200/4 frame (found on the CPU from +60 down)

PAGES = {"A": [dict(kind="alpha", capcode=1234567, text="HELLO FLEX"), dict(kind="numeric", capcode=4242, text="555-0199 U[3]")],
         "B": [dict(kind="tone", capcode=77), dict(kind="alpha", capcode=8, text="dropped", drop=True)],
         "C": [dict(kind="alpha", capcode=99, text="no signature", fragment=0, more=True)],
         "D": [dict(kind="numbered numeric", capcode=5, text="12345"), dict(kind="tone", address=(0x1F8000, 0x12345))]}
LONG_TEXT = "".join(chr(0x20 + (7 * i) % 95) for i in range(3 * 83 - 1))  # an alpha page that fills its phase to the last block


def _want(mode, inverted=False, pages=PAGES, cycle=3, frame=45):
    """What the parser must give for ``pages`` sent in ``mode``: (cycle, frame, phase, mode, inverted, capcode, kind, text,
    fragment, more, damaged), in order of phase and address."""
    out = []
    for p in FM.ACTIVE[mode]:
        for page in pages.get(p, []):
            if page.get("drop"):
                continue
            alpha = page["kind"] == "alpha"
            out.append((cycle, frame, p, mode, inverted, None if "address" in page else page["capcode"], page["kind"],
                        None if "address" in page else page.get("text"), page.get("fragment", 3) if alpha else None,
                        page.get("more", False) if alpha else None, False))
    return out


def _samples(frames=1):
    return int((0.05 + frames * FM.FRAME_BITS / 1600.0 + 0.05) * FS)


@functools.lru_cache(maxsize=None)
def _frame(mode):
    return FM.make_frame(mode, 3, 45, PAGES)


# ---- constants and the plan -----------------------------------------------------------------------------------------------------


def test_constants_are_the_oracles():
    assert (X.MARKER, X.SYNC_B, X.BCH_POLY, X.INFO_MASK) == (FM.MARKER, FM.SYNC_B, FM.G, FM.MASK) == (0xA6C6AAAA, 0x5939, 0x769, 0x1FFFFF)
    assert dict((name, code) for code, name in X.MODES) == FM.MODES and X.MODE_SHAPE == FM.SHAPE
    assert {m: "".join(X.PHASES[p] for p in ph) for m, ph in X.ACTIVE.items()} == FM.ACTIVE
    assert X.TYPES == FM.TYPES and X.DIGITS == FM.DIGITS and len(X.DIGITS) == 16 and tuple(e - 2 for e in X.SHIFT_ORDER) == FM.SHIFT_ORDER
    assert (P.FLEX_BLOCKS, P.FLEX_WORDS, P.FLEX_SYMBOLS, P.FLEX_DATA_BIT, P.FLEX_SHIFTS, P.FLEX_PHASES) == (FM.BLOCKS, FM.WORDS, FM.SYMBOLS,
                                                                                                              FM.DATA_BIT, 5, 4)
    assert bin(X.MARKER).count("1") == 16
    # a mode code lies within three bits of no other, negated or not; 0x5939 is no mode code
    codes = list(FM.MODES.values())
    for a in codes:
        for b in codes + [X.SYNC_B]:
            if a != b:
                assert bin(a ^ b).count("1") > 3 and bin(a ^ b ^ 0xFFFF).count("1") > 3, (hex(a), hex(b))


def test_codewords_and_check4():
    rng = np.random.default_rng(26)
    for info in [0, FM.MASK, 1, 1 << 20] + rng.integers(0, 1 << 21, 40).tolist():
        w = FM.codeword(info)
        assert w & FM.MASK == info and PM.syndrome(X.rev32(w)) == 0 and PM.parity(w) == 0 and X.is_codeword(w)
        assert FM.correct(w) == (w, 0) and PM.correct(X.rev32(w)) == (X.rev32(w), 0)
        for bit in range(32):
            assert FM.correct(w ^ (1 << bit)) == (w, 1)
        assert FM.correct(w ^ 0b101)[1] == 2 and not X.is_codeword(w ^ 1)
    assert X.rev32(0x7CD215D8) == 0x1BA84B3E and X.is_codeword(0x1BA84B3E)  # section 12's sync word
    assert X.syndrome(0x7CD215D8) == PM.syndrome(0x7CD215D8) == 0
    # check4: the nibbles of bits 0 .. 19 and bit 20
    assert X.check4(0xF) and X.check4(0x0000FF0 + 1) and X.check4((1 << 20) | 0xE) and not X.check4(0) and not X.check4((1 << 20) | 0xF)
    for x in rng.integers(0, 1 << 21, 50).tolist():
        y = FM.with_check4(x)
        assert X.check4(y) and FM.check4(y) and y >> 4 == x >> 4
        assert sum(X.check4((y & ~0xF) | nib) for nib in range(16)) == 1
    for a, long in ((0x8000, True), (0x8001, False), (0x1E0000, False), (0x1E0001, True), (0x1F0000, True), (0x1F0001, False),
                    (0x1F7FFE, False), (0x1F7FFF, True), (1, True)):
        assert X.is_long(a) is long and FM.is_long(a) is long


@pytest.mark.parametrize("fs_ch", [12_800.0, 53_333.0, 96_600.0, 358_400.0])
def test_plan_against_the_oracle(fs_ch):
    plan, pl = P.plan_flex(fs_ch), FM.plan(fs_ch)
    assert plan.sps == pl["sps"] and plan.header == tuple(pl["o16"][i] for i in range(-16, 96)) and plan.o16(0) == 0 and len(plan.header) == 112
    for u in (1, 2):
        assert plan.data[u - 1].dtype == np.int32 and plan.data[u - 1].tolist() == pl["data"][u] and plan.steps[u - 1] == pl["step"][u]
        assert len(pl["data"][u]) == 2816 * u
    assert plan.ident == (P.plan_ident(fs_ch, 1600), P.plan_ident(fs_ch, 3200))
    assert plan.header[:64] == plan.ident[0].offsets and plan.o16(-16) == plan.ident[0].o(-16)
    if fs_ch == 96_600.0:  # sps 60.375: i sps ends in .5 for i = 4, 12, ...: half-even
        assert pl["sps"] == 60.375 and (plan.o16(4), plan.o16(12), plan.o16(20)) == (242, 724, 1208)
        assert plan.data[1][0] == round(135.5 * 60.375) and plan.data[0][3] == 8392 and 139 * 60.375 == 8392.125
    if fs_ch == 12_800.0:
        assert plan.steps == (1, 1) and plan.ident[1].sps == 4.0
    if fs_ch == 358_400.0:
        assert plan.steps == (28, 14) and plan.data[1][-1] == round((135 + 2816) * 224.0)


def test_plan_refuses_rates_that_do_not_fit():
    for fs_ch in (12_799.0, 358_401.0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            P.plan_flex(fs_ch)
        with pytest.raises(ValueError):
            X.FlexDecoder(fs_ch)
    with pytest.raises(ValueError, match="rate does not fit"):
        FM.plan(12_799.0)
    P.plan_flex(12_800.0), P.plan_flex(358_400.0)


# ---- the parser against the encoder ---------------------------------------------------------------------------------------------


def _parse(mode, phases, fiw=None, inverted=False, spoil=None):
    """The package's parser on the words of one frame as sent (``spoil``: (phase index, word, status) entries)."""
    fixed = np.zeros((1, 4, 88), dtype=np.uint32)
    status = np.full((1, 4, 88), 4, dtype=np.uint8)
    for p, ws in phases.items():
        fixed[0, "ABCD".index(p)], status[0, "ABCD".index(p)] = ws, 0
    for ph, w, s in spoil or ():
        status[0, ph, w] = s
    head = dict(time_s=1.5, mode=mode, inverted=inverted, fiw=FM.codeword(FM.fiw_info(3, 45)) if fiw is None else fiw, fiw_status=0)
    return X.parse_frames([head], fixed, status)


@pytest.mark.parametrize("mode", list(FM.MODES))
@pytest.mark.parametrize("inverted", [False, True])
def test_round_trip_encoder_to_parser(mode, inverted):
    _, phases = _frame(mode)
    pages, counts = _parse(mode, phases, inverted=inverted)
    assert [FM.page_key(p) for p in pages] == _want(mode, inverted)
    assert counts == dict(fiw_failed=0, biw_lost=0, biw_bad=0, vectors_dropped=1 if "B" in FM.ACTIVE[mode] else 0)
    assert all(p.time_s == 1.5 and p.corrected == 0 for p in pages)
    first = pages[0]
    assert first.line() == f'FLEX {mode} 03.045.A cap=1234567 alpha "HELLO FLEX"' and first.words[0] == f"{phases['A'][1]:08x}"
    assert len(first.words) == 2 + 1 + 4  # address, vector, header and the signature with ten characters in four words
    if mode == "3200/4":
        long = pages[-1]
        assert (long.capcode, long.long, long.kind, long.text) == (None, True, "tone", None) and len(long.words) == 3
        assert long.line() == "FLEX 3200/4 03.045.D cap=long tone" and pages[-2].text == "12345" and pages[1].text == "555-0199 U[3]"
    # the oracle's own parser reads the same
    for p in FM.ACTIVE[mode]:
        state, got = FM.read_phase(phases[p], [0] * 88)
        assert state == "ok" and [(mode, inverted) + g for g in got if g != "dropped"] == [k[3:5] + k[5:] for k in _want(mode, inverted) if k[2] == p]


def test_parser_counts_what_it_cannot_read():
    mode = "3200/4"
    _, phases = _frame(mode)
    # the frame information word: status 2, or a failed check4
    assert _parse(mode, phases, fiw=FM.codeword(FM.fiw_info(3, 45) ^ 1)) == ([], dict(fiw_failed=1, biw_lost=0, biw_bad=0, vectors_dropped=0))
    head = dict(time_s=0.0, mode=mode, inverted=False, fiw=FM.codeword(FM.fiw_info(3, 45)), fiw_status=2)
    assert X.parse_frames([head], np.zeros((1, 4, 88), dtype=np.uint32), np.zeros((1, 4, 88), dtype=np.uint8))[1]["fiw_failed"] == 1
    assert FM.read_fiw(FM.codeword(FM.fiw_info(9, 127, 0x2A)), 1) == (9, 127) and FM.read_fiw(FM.codeword(FM.fiw_info(9, 127)), 2) is None
    # an idle phase, a lost and a bad block information word
    idle = dict(phases, C=[FM.codeword(x) for x in FM.phase_infos([])])
    pages, counts = _parse(mode, idle)
    assert [p.phase for p in pages] == ["A", "A", "B", "D", "D"] and counts["biw_bad"] == counts["biw_lost"] == 0
    assert FM.read_phase(idle["C"], [0] * 88) == ("idle", [])
    pages, counts = _parse(mode, phases, spoil=[(2, 0, 2)])
    assert [p.phase for p in pages] == ["A", "A", "B", "D", "D"] and counts["biw_lost"] == 1
    bad = dict(phases, A=[FM.codeword(x) for x in FM.phase_infos(PAGES["A"], break_biw=True)])
    pages, counts = _parse(mode, bad)
    assert [p.phase for p in pages] == ["B", "C", "D", "D"] and counts["biw_bad"] == 1 and FM.read_phase(bad["A"], [0] * 88)[0] == "biw_bad"
    # a damaged message word: three replacement characters; a corrected one is counted
    pages, _ = _parse(mode, phases, spoil=[(0, 7, 2), (0, 6, 1)])
    assert pages[0].text == "HE" + 3 * "\ufffd" + " FLEX" and pages[0].damaged and pages[0].corrected == 1
    # a message that would run past the frame, and one that starts inside the vector field
    for start, count in ((80, 9), (2, 4)):
        ws = list(phases["C"])
        ws[2] = FM.codeword(FM.with_check4((5 << 4) | (start << 7) | (count << 14)))
        assert _parse(mode, dict(phases, C=ws))[1]["vectors_dropped"] == 2
    # fragments are pages of their own
    assert [p.more for p in _parse(mode, phases)[0] if p.phase == "C"] == [True]


def test_result_round_trips_through_json():
    _, phases = _frame("3200/4")
    pages, counts = _parse("3200/4", phases)
    ch = X.FlexChannel(offset_hz=200e3, freq_hz=455.7e6, frames={"3200/4": 1}, words={"0": 352}, shifts={"0": 11}, pages=pages, **counts)
    res = X.FlexResult(channels=[ch, X.FlexChannel(offset_hz=-1e3, freq_hz=None, note="rate does not fit")], sample_rate=2.4e6, center_freq=455.5e6)
    assert X.FlexResult.from_json(__import__("json").loads(__import__("json").dumps(res.to_json()))) == res
    assert res.lines()[0] == '455700000 Hz: FLEX 3200/4 03.045.A cap=1234567 alpha "HELLO FLEX"' and len(res.lines()) == len(pages) == len(res.pages)


def test_choose_shifts_ties():
    status = np.zeros((2, 5, 4, 88), dtype=np.uint8)
    status[:, :, 1:] = 4  # 1600/2: phase A only
    assert X.choose_shifts(status, (0,)).tolist() == [[2] * 11] * 2  # all equal: shift 0
    status[0, 2, 0, 8:16] = 2  # block 1: shift 0 is the worst, -1 and +1 tie: the negative one
    status[0, 1, 0, 16] = status[0, 2, 0, 17] = 2  # block 2: -1 and 0 tie at one word, +1 is clean
    status[0, (1, 2, 3), 0, 24] = 3  # block 3: -2 and +2 tie
    status[1, :, 0, 80:88] = 2
    status[1, 4, 0, 87] = 1  # the last block of frame 1: +2 alone has a word less
    status[1, 0, 3, 0:8] = 2  # an inactive phase does not count
    got = X.choose_shifts(status, (0,))
    assert got.tolist() == [[2, 1, 3, 0, 2, 2, 2, 2, 2, 2, 2], [2] * 10 + [4]]
    for f in range(2):
        mode = "1600/2"
        assert FM.choose_shifts(status[f], mode) == got[f].tolist()
    fixed = np.arange(2 * 5 * 4 * 88, dtype=np.uint32).reshape(2, 5, 4, 88)
    took = X.take_shifts(fixed, got)
    assert took.shape == (2, 4, 88) and took[0, 0, 8] == fixed[0, 1, 0, 8] and took[1, 3, 87] == fixed[1, 4, 3, 87] and took[0, 2, 0] == fixed[0, 2, 2, 0]
    np.testing.assert_array_equal(took[1], FM.take_shifts(fixed[1], got[1]))
    # two active phases are added
    both = np.zeros((1, 5, 4, 88), dtype=np.uint8)
    both[0, 2, 0, 0] = both[0, 1, 2, 0] = both[0, 1, 2, 1] = 2
    assert X.choose_shifts(both, (0, 2))[0, 0] == 3 and X.choose_shifts(both, (0,))[0, 0] == 1 and FM.choose_shifts(both[0], "3200/2")[0] == 3


# ---- the oracle on synthesised theta ----------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _decoded(mode, inverted=False, noise=0.0, ppm=0.0, long=False):
    if long:
        pages = dict(PAGES, A=[dict(kind="alpha", capcode=1234567, text=LONG_TEXT)], C=[dict(kind="alpha", capcode=99, text=LONG_TEXT[::-1])])
        segments, phases = FM.make_frame(mode, 3, 45, pages)
    else:
        segments, phases = _frame(mode)
    theta = FM.synth_theta([(0.03, segments)], FS, _samples(), inverted=inverted, noise=noise, seed=7, ppm=ppm)
    return FM.decode_theta(theta, FS), phases


@pytest.mark.parametrize("mode", list(FM.MODES))
@pytest.mark.parametrize("inverted,noise", [(False, 0.0), (True, 0.0), (False, NOISE)])
def test_oracle_end_to_end(mode, inverted, noise):
    out, phases = _decoded(mode, inverted, noise)
    assert out["rows"] == [(out["rows"][0][0], -1 if inverted else 1, mode)] and out["unknown_mode"] == 0 and out["ok"].tolist() == [True]
    assert abs(out["rows"][0][0] - (0.03 * FS + 49 * 16 - 1)) <= 2  # the end of the marker's first bit
    assert out["rec16"][0, 3] == FM.codeword(FM.fiw_info(3, 45)) and out["rec16"][0, 4] <= (1 if noise else 0) and out["rec16"][0, 5] == 1
    assert [p[1:] for p in out["pages"]] == _want(mode, inverted)
    chosen = FM.take_shifts(out["status"][0], out["chosen"][0])
    for p in "ABCD":
        if p in FM.ACTIVE[mode]:
            assert (chosen["ABCD".index(p)] <= (2 if noise else 0)).all()
            if not noise:
                assert FM.take_shifts(out["fixed"][0], out["chosen"][0])["ABCD".index(p)].tolist() == phases[p]
        else:
            assert (out["status"][0][:, "ABCD".index(p)] == 4).all() and not out["fixed"][0][:, "ABCD".index(p)].any()
    if not noise:
        assert out["chosen"].tolist() == [[2] * 11]
    # the package's host logic on the oracle's arrays gives the same pages
    heads = [dict(time_s=m / FS, mode=md, inverted=s < 0, fiw=out["rec16"][j, 3], fiw_status=out["rec16"][j, 4]) for j, (m, s, md) in enumerate(out["rows"])]
    got = X.choose_shifts(out["status"], X.ACTIVE[mode])
    assert got.tolist() == out["chosen"].tolist()
    pages, _ = X.parse_frames(heads, X.take_shifts(out["fixed"], got), X.take_shifts(out["status"], got))
    assert [FM.page_key(p) for p in pages] == [p[1:] for p in out["pages"]]


def test_loops_and_vectorised_forms_agree():
    out, _ = _decoded("3200/4", False, NOISE)
    m, s, mode = out["rows"][0]
    n = m + out["plan"]["data"][2][-1]  # one sample short of the last instant: status 3 in the last word
    for u, levels, plane, rec in ((2, 4, out["v32"][:n], out["rec32"][0]), (1, 2, out["v16"], out["rec16"][0])):
        rec = (m, s, int(rec[0]), int(rec[1]))
        fixed, raw, status = FM.words(plane, [rec], levels, u, out["plan"])
        by = FM.words_by_loops(plane, rec, levels, u, out["plan"])
        assert fixed[0].tolist() == by[0] and raw[0].tolist() == by[1] and status[0].tolist() == by[2]
        if u == 2:  # at shift 0 the last symbol alone lies outside: the last word of phases C and D
            assert [by[2][2][ph][87] == 3 for ph in range(4)] == [False, False, True, True] and 3 not in by[2][2][2][:87]
            assert by[2][4][2][87] == 3 and by[2][4][0][87] != 3 and by[2][0][3][87] != 3
    assert FM.frame_record(out["v16"], m, s, out["plan"]) == out["rec16"][0].tolist()


def test_clock_error_needs_the_shifts():
    """A 3200/4 frame whose sender runs 44 ppm fast or slow (a quarter of a symbol at the frame's end), two alpha pages filling
    phases A and C to the last block: shift 0 alone leaves refused words in the last block, the chosen shifts decode all.  (From
    56 ppm on a phase of the last blocks reads its neighbour's words, which are codewords too, at shift 0: the count of refused
    words cannot see that, and the pages come out wrong.  DESIGN.md section 26 lists it under the known limits.)"""
    clean, phases = _decoded("3200/4", long=True)
    want = [p[1:] for p in clean["pages"]]
    assert [p[6] for p in want] == ["alpha", "tone", "alpha", "numbered numeric", "tone"] and want[0][7] == LONG_TEXT and want[2][7] == LONG_TEXT[::-1]
    sent = np.array([phases[p] for p in "ABCD"], dtype=np.uint32)
    for ppm, e in ((PPM, 1), (-PPM, 3)):
        out, _ = _decoded("3200/4", ppm=ppm, long=True)
        zero = (out["fixed"][0][2] != sent) | (out["status"][0][2] >= 2)
        print(ppm, "shift 0: refused or wrong words per block", zero.reshape(4, 11, 8).sum(axis=(0, 2)).tolist(), "chosen", out["chosen"].tolist())
        assert zero[:, 80:].any() and (out["status"][0][2][:, 80:] >= 2).any() and not zero[:, :80].any()
        assert out["chosen"][0].tolist() == [2] * 10 + [e]
        assert [p[1:] for p in out["pages"]] == want
    for ppm in (20.0, -20.0):
        assert [p[1:] for p in _decoded("3200/4", ppm=ppm, long=True)[0]["pages"]] == want


def test_model_capture_reads_fsk_3200_and_decodes():
    """The model capture of the GPU test's CLI run, through the numpy finder, the float64 channelizer and section 23's keying:
    a 3200/2 frame reads ``fsk 3200`` (1600/2 reads ``fsk 3200`` too; 1600/4 and 3200/4 read ``unkeyed`` and are not identified:
    DESIGN.md section 26), section 25 names it, and the oracle decodes its three pages."""
    flex, voice = FM.model_run("3200/2")
    assert flex["keyed"]["label"] == "fsk 3200" and voice["keyed"]["label"] == "unkeyed" and voice["flex"] is None
    assert (flex["named"]["protocol"], flex["named"]["mode"], flex["named"]["hits"]) == ("flex", "3200/2", {"flex": 1})
    assert 8.0 <= flex["described"]["plan"]["fs_ch"] / 1600.0 <= 224.0
    assert [p[1:] for p in flex["flex"]["pages"]] == _want("3200/2", pages=FM.CAPTURE_PAGES)
    assert flex["flex"]["chosen"].tolist() == [[2] * 11]


# ---- the CLI, the package surface, the C ABI ------------------------------------------------------------------------------------


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        cli.main(argv)
    assert exc.value.code == 2
    return capsys.readouterr().err


def test_cli_refuses_misuse(capsys):
    base = ["--in", "capture.wav"]
    assert "--find-flex cannot be combined with --ft." in _usage_error(base + ["--find-flex", "--ft", "455800000"], capsys)
    assert "--find-flex cannot be combined with --benchmark." in _usage_error(base + ["--find-flex", "--benchmark"], capsys)
    assert "--find-flex cannot be combined with --audio-post." in _usage_error(base + ["--find-flex", "--audio-post", "x"], capsys)
    assert "--find-flex cannot be combined with --probe-only." in _usage_error(base + ["--find-flex", "--probe-only"], capsys)
    assert "--find-flex needs --in." in _usage_error(["--find-flex"], capsys)
    assert "--find-auto needs --find-top." in _usage_error(base + ["--find-flex", "--find-auto"], capsys)
    assert "--find-identify cannot be combined with --ft." in _usage_error(base + ["--find-identify", "--find-flex", "--ft", "1e6"], capsys)
    args = cli.build_parser().parse_args(base + ["--find-flex", "--find-threshold", "8"])
    assert args.find_identify is False
    assert cli.check_find_args(cli.build_parser(), args) is True and (args.find_flex, args.find_identify, args.find_decode) == (True, True, True)
    args = cli.build_parser().parse_args(base + ["--find-identify"])
    assert cli.check_find_args(cli.build_parser(), args) is True and args.find_flex is False


def test_package_surface():
    for name in ("FlexPage", "FlexResult", "FlexDecoder"):
        assert getattr(A, name) is getattr(X, name)
    assert A.plan_flex is P.plan_flex
    text = Path(X.__file__).read_text()
    assert "scipy" not in text and "import oracle" not in text and "from oracle" not in text
    plan = P.plan_find(2.4e6, 100_000)
    fin = dict(runs=np.zeros((0, 8), dtype=np.int64), on=np.zeros((0, plan.slices), dtype=np.uint8))
    with pytest.raises(ValueError, match="flex=True needs identify=True"):
        DS.ChannelDescriber(plan, fin, [], keying=True, flex=True)
    with pytest.raises(ValueError, match="without flex=True"):
        DS.ChannelDescriber(plan, fin, [], keying=True, identify=True).finish_flex()
    with pytest.raises(ValueError, match="flex=True needs identify=True"):
        A.find_channels("nothing.wav", describe=True, keying=True, flex=True)


def test_c_abi_refuses_bad_arguments():
    """The library has the two entry points, and the argument checks come before the launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some = c_void_p(0), c_void_p(8)  # (never dereferenced: every call below is refused, or has nothing to do)
    for name in ("iqa_flex_frames", "iqa_flex_words"):
        assert hasattr(N.lib(), name) and name in N.EXPORTS
    assert N.lib().iqa_abi_version() == 1
    header = (Path(__file__).resolve().parent.parent / "include" / "iqa_hotpath.h").read_text()
    for text in ("#define IQA_FLEX_HEADER_OFFSETS 112", "#define IQA_FLEX_BLOCKS 11", "#define IQA_FLEX_SHIFTS 5", "#define IQA_FLEX_PHASES 4",
                 "#define IQA_FLEX_WORDS 88", "#define IQA_FLEX_SYMBOLS 2816", "#define IQA_FLEX_MAX_STEP 28", "#define IQA_ABI_VERSION 1"):
        assert text in header
    plan = P.plan_flex(FS)
    i32, i64 = c_int32, c_int64

    def frames(plane=some, n=100_000, hits=some, k=2, offsets=plan.header, out=some):
        off = None if offsets is None else (c_int32 * 112)(*offsets)
        N.call("iqa_flex_frames", plane, i64(n), hits, i64(k), off, out, null)

    def offs(at, value):
        o = list(plan.header)
        o[at] = value
        return tuple(o)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(k=-1), "negative"), (dict(n=(1 << 30) + 1), "2\\^30"), (dict(k=(1 << 20) + 1), "2\\^20"),
                         (dict(offsets=None), "NULL offsets"), (dict(offsets=offs(16, 1)), "o\\[0\\]"), (dict(offsets=offs(40, 0)), "ascend"),
                         (dict(offsets=offs(111, plan.header[110] + 226)), "step"), (dict(plane=null), "NULL"), (dict(hits=null), "NULL"),
                         (dict(out=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            frames(**kwargs)
    frames(plane=null, hits=null, out=null, n=0)  # nothing to do: no pointer is touched
    frames(plane=null, hits=null, out=null, k=0)

    def words(plane=some, n=100_000, recs=some, f=1, levels=4, u=2, step=1, offsets=some, fixed=some, raw=some, status=some):
        N.call("iqa_flex_words", plane, i64(n), recs, i64(f), i32(levels), i32(u), i32(step), offsets, fixed, raw, status, null)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(f=-1), "negative"), (dict(n=(1 << 30) + 1), "2\\^30"), (dict(f=(1 << 20) + 1), "2\\^20"),
                         (dict(levels=3), "levels"), (dict(levels=0), "levels"), (dict(u=0), "u must"), (dict(u=3), "u must"), (dict(step=0), "step"),
                         (dict(step=29), "step"), (dict(plane=null), "NULL"), (dict(recs=null), "NULL"), (dict(offsets=null), "NULL"),
                         (dict(fixed=null), "NULL"), (dict(raw=null), "NULL"), (dict(status=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            words(**kwargs)
    words(plane=null, recs=null, offsets=null, fixed=null, raw=null, status=null, n=0)
    words(plane=null, recs=null, offsets=null, fixed=null, raw=null, status=null, f=0, step=28, levels=2, u=1)
