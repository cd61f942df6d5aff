"""The DMR burst decoding (--find-dmr) without a GPU: the constants of the package against the oracle's own
copy, the facts that section 29 states about the codes, the oracle's coders on crafted errors, ``plan_dmr`` against the oracle's
plan, the package's parser and call tracker against the oracle's on crafted bursts, the JSON round trip, the layer table's
branch, the CLI's flags, the entry points' argument checks, the oracle end to end on synthesised theta (clean and at the noise
level found here) and the model capture of the GPU test's CLI run through the numpy pipeline."""
from __future__ import annotations

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
from iq_to_audio_amd import dmr as X
from iq_to_audio_amd import dsp_plan as P
from iq_to_audio_amd import find_layers as FL


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


DM = _load("dmr_model")
FS = 160_000.0
#: radians of white noise on theta: the largest of 0.01, 0.02, ... at which the oracle alone still decodes every burst of the test
#: stream (found on the CPU: 0.07 loses three bursts to the BPTC)
NOISE = 0.06


# ---- constants and the codes ------------------------------------------------------------------------------------------------------


def test_constants_are_the_oracles():
    assert X.SYNC_VOICE == (DM.BS_VOICE, DM.MS_VOICE) and X.SYNC_DATA == (DM.BS_DATA, DM.MS_DATA) and X.KINDS == DM.KINDS
    assert [(p.protocol, p.word, p.symbols) for p in X.PATTERNS] == [(p[0], p[3], p[4]) for p in DM.DMR_PATTERNS]
    for name in ("TACT_BITS", "TACT_CHECKS", "SLOT_TYPE_BITS", "GOLAY_POLY", "INTERLEAVE", "PAYLOAD_BITS", "ROW_CHECKS", "COLUMN_CHECKS",
                 "ROUNDS", "INFO_INDEX", "GF_POLY", "RS_GENERATOR", "RS_MASK", "CRC_MASK", "DATA_TYPES", "HANG_S"):
        assert getattr(X, name) == getattr(DM, name), name
    assert (X.FIRST, X.LAST, X.BURST_FIRST, X.CACH_FIRST) == (-66, 77, -54, -66) and X.LAST - X.FIRST + 1 == P.DMR_OFFSETS == 144
    assert (P.DMR_LEAD, P.DMR_WORDS, P.DMR_RECORD) == (66, 9, 8) and X.PLANE_RATES == (4800,) and X.CRC_POLY == 0x1021
    assert len(X.INFO_INDEX) == 96 and X.INFO_INDEX[:9] == (4, 5, 6, 7, 8, 9, 10, 11, 16) and X.INFO_INDEX[-1] == 131
    assert len(X.PAYLOAD_BITS) == 196 and len(X.SLOT_TYPE_BITS) == 20 and X.GOLAY_MAX_DISTANCE == 3
    header = (Path(__file__).resolve().parent.parent / "include" / "iqa_hotpath.h").read_text()
    for text in ("#define IQA_DMR_OFFSETS 144", "#define IQA_DMR_WORDS 9", "#define IQA_DMR_RECORD 8", "#define IQA_ABI_VERSION 1"):
        assert text in header


def test_the_facts_section_29_states():
    # the slot type's code
    assert (DM.GOLAY[1], DM.GOLAY[2], DM.GOLAY[4]) == (0x18EB, 0x293E, 0x4A97)
    assert min(bin(a ^ b).count("1") for i, a in enumerate(DM.GOLAY) for b in DM.GOLAY[i + 1 :]) == 8
    assert all(cw >> 12 == d and bin(cw).count("1") % 2 == 0 for d, cw in enumerate(DM.GOLAY))
    # the generator is (x + a)(x + a^2)(x + a^3) over GF(2^8) / 0x11D, a = 2
    prod = [1]
    for root in (2, 4, 8):
        prod = [x ^ y for x, y in zip(prod + [0], [0] + [DM.gf_mul(c, root) for c in prod])]
    assert tuple(prod) == DM.RS_GENERATOR == (1, 14, 56, 64)
    assert all(X.gf_mul(a, b) == DM.gf_mul(a, b) for a in (0, 1, 2, 29, 142, 255) for b in range(256))
    # the three check matrices: distinct nonzero columns; the column code leaves two syndromes unnamed
    for table, length in ((DM.H7, 7), (DM.H13, 13), (DM.H15, 15)):
        assert len(table) == length and not any(not any(syn) for syn in table)
    assert len(DM.H7) == 2 ** 3 - 1 and len(DM.H15) == 2 ** 4 - 1
    assert {(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)} - set(DM.H13) - {(0, 0, 0, 0)} == {(1, 0, 0, 1), (1, 1, 0, 1)}
    # the interleave is a bijection
    assert sorted((181 * k) % 196 for k in range(196)) == list(range(196))
    # both sync words hold twelve +3 and twelve -3, and the data words are their negations
    for voice, data in ((DM.BS_VOICE, DM.BS_DATA), (DM.MS_VOICE, DM.MS_DATA)):
        lev = DM.sync_levels(voice)
        assert sorted(lev) == [-3] * 12 + [3] * 12 and DM.sync_levels(data) == [-x for x in lev]
    assert [DM.sync_levels(w) for w in X.SYNC_VOICE] == [list(A.identify.symbols_of(p)) for p in X.PATTERNS]
    # the CRC: the usual check value of CRC-CCITT with a zero start
    assert DM.crc_ccitt(b"123456789") == X.crc_ccitt(b"123456789") == 0x31C3


# ---- the oracle's coders on crafted words -------------------------------------------------------------------------------------------


def _clean():
    words, kind = DM.coder_cases()["clean"]
    return DM.decode_burst(words, kind)


def test_bptc_round_trips():
    cases = DM.coder_cases()
    info, rec = _clean()
    assert rec == [0, 12, 0, 0, 0x53, 0, 0, 1]  # TACT clean (AT 1, TC 1), slot type clean (cc 5, CSBK), payload clean after one round
    _, burst = DM.crafted_burst()
    assert DM.bptc_decode([burst[j] for j in DM.PAYLOAD_BITS])[3] == np.random.default_rng(2).integers(0, 2, 96).tolist()
    for p in range(196):
        got_info, got = DM.decode_burst(*cases[f"single-{p}"])
        # (bit 0 of the matrix is unused: its flip goes unseen; every other one is restored by its column)
        assert got_info == info and got[5:] == ([0, 0, 1] if p == 0 else [1, 1, 2]), p
    got_info, got = DM.decode_burst(*cases["two-apart"])
    assert got_info == info and got[5:] == [1, 2, 2]
    got_info, got = DM.decode_burst(*cases["unmatched-column"])  # the column is left alone, its two rows restore a bit each
    assert got_info == info and got[5:] == [1, 2, 2]
    got_info, got = DM.decode_burst(*cases["two-rounds"])
    assert got_info == info and got[5] == 1 and got[7] == 3 and got[6] >= 3
    got_info, got = DM.decode_burst(*cases["fails"])
    assert got[5] == 2 and got[7] <= 5 and got[2] == 0
    assert DM.decode_burst(*cases["zeros"])[1][2:6] == [0, 0, 0, 0]  # (the zero word is a codeword of every code here)
    assert DM.decode_burst(*cases["ones"])[1][2] == 2 and DM.decode_burst(*cases["ones"])[1][5] == 4


def test_slot_type_and_tact_errors():
    cases = DM.coder_cases()
    info, rec = _clean()
    for name in [f"slot-single-{p}" for p in range(20)] + [n for n in cases if n.startswith("slot-triple-")]:
        got_info, got = DM.decode_burst(*cases[name])
        assert got_info == info and got[2:5] == [1, 3 if "triple" in name else 1, 0x53] and got[5:] == rec[5:], name
    got_info, got = DM.decode_burst(*cases["slot-four"])
    assert got[2] == 2 and got[3] == 4 and got[5:] == [4, 0, 0] and got_info == [0, 0, 0]
    assert got[4] == DM.bits_word(DM.record_bits(cases["slot-four"][0])[24:][j] for j in DM.SLOT_TYPE_BITS[:8])
    for j in range(7):
        got_info, got = DM.decode_burst(*cases[f"tact-{j}"])
        assert got_info == info and got[:2] == [1, 12] and got[2:] == rec[2:]
    assert DM.decode_burst(*cases["voice-bs"])[1] == [0, 12, 4, 0, 0, 4, 0, 0]
    assert DM.decode_burst(*cases["voice-ms"])[1] == [4, 0, 4, 0, 0, 4, 0, 0]
    assert DM.decode_burst(*cases["data-ms"])[1] == [4, 0, 0, 0, 0xF6, 0, 0, 1]


# ---- the plan ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("fs_ch", [19_200.0, 160_000.0, 96_600.0, 1_075_200.0, 25_000.0])
def test_plan_against_the_oracle(fs_ch):
    plan, want = P.plan_dmr(fs_ch), DM.plan(fs_ch)
    assert plan.sps == want["sps"] == fs_ch / 4800.0 and len(plan.offsets) == 144
    assert list(plan.offsets) == [want["o"][i] for i in range(-66, 78)] and plan.o(0) == 0 and plan.o(-66) == want["o"][-66]
    assert (plan.ident.window, plan.ident.half, plan.ident.shift) == (want["ident"]["L"], want["ident"]["h"], want["ident"]["sh"])
    assert plan.ident == P.plan_ident(fs_ch, 4800) and A.plan_dmr is P.plan_dmr
    assert all(0 < b - a <= 225 for a, b in zip(plan.offsets, plan.offsets[1:]))
    if fs_ch == 96_600.0:  # sps 20.125: i = 4 and 12 fall on .5 and go to the even side
        assert (plan.o(4), plan.o(12), plan.o(-4), plan.o(20)) == (80, 242, -80, 402)


def test_plan_refuses_rates_that_do_not_fit():
    for fs_ch in (19_199.0, 1_075_201.0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            P.plan_dmr(fs_ch)
    for fs_ch in (19_199.0, 1_075_201.0):
        with pytest.raises(ValueError):
            DM.plan(fs_ch)
        with pytest.raises(ValueError):
            A.DmrDecoder(fs_ch)


# ---- the parser and the call tracker ----------------------------------------------------------------------------------------------


def _crafted(script, sps=100 / 3.0, **kwargs):
    """rows, levels, info, rec of a base station's ``script``, a slot every 144 symbols, through the oracle's coders alone."""
    levels = DM.base_station(script, **kwargs)
    sym = {v: k for k, v in DM.LEVEL.items()}
    rows, words = [], []
    for j, item in enumerate(script):
        if item == "voice-":
            continue
        bits = [b for lev in levels[144 * j : 144 * j + 144] for b in (sym[lev] >> 1, sym[lev] & 1)]
        words.append(DM.words_of(bits[:24], bits[24:]))
        kind = 0 if item == "voice" else 1
        rows.append((int(round((144 * j + 66) * sps)), 1 if kind == 0 else -1, kind))
    rows = np.array(rows, dtype=np.int64).reshape(-1, 3)
    info, rec = DM.decode_all(words, rows[:, 2])
    return rows, np.array([[0, 1000, 3]] * len(rows), dtype=np.int64).reshape(-1, 3), info, rec


def _both(script, **kwargs):
    """The package's bursts and calls of ``script`` as dicts, asserted equal to the oracle's."""
    rows, levels, info, rec = _crafted(script, **kwargs)
    bursts, counts = X.parse_bursts(rows, levels, info, rec, FS)
    want, want_counts = DM.parse(rows, levels, info, rec, FS)
    assert [b.to_json() for b in bursts] == want and counts == want_counts
    calls = X.track_calls(bursts)
    assert [c.to_json() for c in calls] == DM.track(want)
    return bursts, counts, calls


SUPER = ["voice", None, "voice-", None, "voice-", None, "voice-", None, "voice-", None, "voice-", None]


def test_parser_and_calls_on_the_test_script():
    bursts, counts, calls = _both(DM.SCRIPT)
    assert counts == dict(no_level=0, cut=0, slot_refused=0, bptc_failed=0, check_failed=0, tact_fixed=0, idle=24)
    (call,) = calls  # the repeated header opens one call
    assert (call.slot, call.cc, call.group, call.src, call.dst, call.superframes, call.terminated) == (1, 1, True, DM.SRC, DM.DST, 3, True)
    assert abs((call.end_s - call.start_s) - 40 * 0.030) < 1e-3
    csbk = [b for b in bursts if b.data_type == 3]
    assert len(csbk) == 1 and (csbk[0].slot, csbk[0].csbko, csbk[0].fid, csbk[0].checked) == (2, 0x3D, 0, True)
    assert csbk[0].line() == "DMR cc=1 ts=2 csbk o=0x3d fid=0x00 0123456789abcdef"
    assert call.line() == "DMR cc=1 ts=1 group 2345678 -> 9 1.20 s (3 superframes)"


def test_late_entry_hang_and_an_unterminated_call():
    # late entry: voice without a header; then 25 empty slots (750 ms) on the air; then a private call that never ends
    script = SUPER + SUPER + ["voice-"] * 50 + [("header", 3, 111, 222), None] + SUPER
    bursts, counts, calls = _both([x if x is not None else "voice-" for x in script])  # (no idle bursts: the slots stay silent)
    assert len(calls) == 2
    late, private = calls
    assert (late.group, late.src, late.dst, late.cc, late.superframes, late.terminated) == (None, None, None, None, 2, False)
    assert late.end_s == bursts[1].time_s and "late entry" in late.line() and "not terminated" in late.line()
    assert (private.group, private.src, private.dst, private.cc, private.superframes, private.terminated) == (False, 111, 222, 1, 1, False)
    # within the hang the call goes on: the next voice sync of the slot comes 22 slots (660 ms) behind the last one
    script = [("header", 0, 1, 2), "voice-"] + SUPER + ["voice-"] * 10 + SUPER
    _, _, calls = _both([x if x is not None else "voice-" for x in script])
    assert len(calls) == 1 and calls[0].superframes == 2


def test_two_slots_interleaved_and_a_failed_check():
    a, b = ("header", 0, 10, 20), ("header", 3, 30, 40)
    script = [a, b, "voice", "voice", "voice-", "voice-", ("term", 0, 10, 20), "voice-", "voice-", ("term", 3, 30, 40, dict(break_rs=True)),
              "voice-", ("term", 3, 30, 40)]
    bursts, counts, calls = _both(script)
    assert counts["check_failed"] == 1 and [(c.slot, c.src, c.dst, c.group, c.superframes, c.terminated) for c in calls] == [
        (1, 10, 20, True, 1, True), (2, 30, 40, False, 1, True)]
    failed = [x for x in bursts if x.checked is False]
    assert len(failed) == 1 and failed[0].src is None and failed[0].line().endswith("(failed)")
    assert calls[1].end_s == bursts[-1].time_s  # the failed terminator closes nothing
    # a header whose check fails opens no call; a CSBK with a bad CRC is flagged
    bad = DM.csbk_info(1, 2, [0] * 8)
    bad[80] ^= 1
    bursts, counts, calls = _both([("header", 0, 1, 2, dict(break_rs=True)), ("raw", 3, bad), ("raw", 7, [1] * 96), ("raw", 6, DM.csbk_info(1, 2, [9] * 8, data_type=6))])
    assert calls == [] and counts["check_failed"] == 2 and [x.checked for x in bursts] == [False, False, None, True]
    assert bursts[2].hex == "ff" * 12 and bursts[2].type_name == "rate 1/2 data" and bursts[3].csbko is None


def test_dropped_bursts_are_counted():
    rows, levels, info, rec = _crafted([None, None, None, None, ("header", 0, 1, 2)])
    levels[0] = (0, 0, 2)  # cut
    levels[1] = (5, 0, 3)  # no level
    rec = DM.apply_flags(rec, levels, rows[:, 2])
    np.testing.assert_array_equal(rec, X.apply_flags(rec, levels, rows[:, 2]))
    assert rec[0, 5] == 3 and rec[1, 5] == 0
    rec[2, 2] = 2  # a refused slot type
    rec[3, 5] = 2  # a failed payload
    levels[4] = (0, 1000, 1)  # the CACH outside: no slot
    rec = X.apply_flags(rec, levels, rows[:, 2])
    bursts, counts = X.parse_bursts(rows, levels, info, rec, FS)
    want, want_counts = DM.parse(rows, levels, info, rec, FS)
    assert [b.to_json() for b in bursts] == want and counts == want_counts
    assert counts == dict(no_level=1, cut=1, slot_refused=1, bptc_failed=1, check_failed=0, tact_fixed=0, idle=0)
    assert [(b.checked, b.slot) for b in bursts] == [(False, 2), (True, None)]
    (call,) = X.track_calls(bursts)
    assert call.slot is None and "ts=?" in call.line()


def test_burst_hits_keeps_the_larger_of_two_near_hits():
    pats = A.identify.patterns_for(4800)
    hits = [(0, 1000, -50, 9, 0, 0), (1, 1010, 40, 9, 0, 0), (0, 1016, 50, 9, 0, 0), (1, 1016, -50, 9, 0, 0), (2, 1000, 999, 9, 0, 0), (0, 3000, 7, 9, 0, 0)]
    got = X.burst_hits(np.array(hits, dtype=np.int64), pats, 16)
    want = DM.burst_hits([h for h in hits if h[0] < 2], 16)
    assert got.tolist() == [list(r) for r in want] == [[1000, -1, 1], [3000, 1, 0]]
    assert X.burst_hits(np.array(hits, dtype=np.int64), pats, 15).tolist() == [[1000, -1, 1], [1016, 1, 0], [3000, 1, 0]]
    assert X.burst_hits(np.zeros((0, 6), dtype=np.int64), pats, 16).shape == (0, 3)


def test_result_round_trips_through_json():
    bursts, counts, calls = _both(DM.SCRIPT)
    ch = X.DmrChannel(offset_hz=200e3, freq_hz=439512500.0, kinds={"bs data": 28, "bs voice": 3}, calls=calls,
                      bursts=[b for b in bursts if b.data_type not in (None, 9)], **counts)
    res = X.DmrResult(channels=[ch, X.DmrChannel(offset_hz=1.0, freq_hz=None, note="no dmr channel")], sample_rate=2.4e6, center_freq=439312500.0)
    assert X.DmrResult.from_json(json.loads(json.dumps(res.to_json()))) == res
    assert res.lines() == ["439512500 Hz: DMR cc=1 ts=1 group 2345678 -> 9 1.20 s (3 superframes)",
                           "439512500 Hz: DMR cc=1 ts=2 csbk o=0x3d fid=0x00 0123456789abcdef"]
    assert res.calls == calls and ch.to_json()["calls"][0]["src"] == DM.SRC
    assert all(hasattr(cls, "to_json") and (hasattr(cls, "line") or hasattr(cls, "lines")) for cls in (X.DmrBurst, X.DmrCall, X.DmrChannel, X.DmrResult))


# ---- the layer table, the CLI, the package surface, the C ABI -----------------------------------------------------------------------


def test_the_branch_of_the_layer_table():
    (row,) = [l for l in FL.FIND_BRANCHES if l.name == "dmr"]
    assert FL.FIND_BRANCHES.index(row) == 0
    assert (row.name, row.flag, row.section, row.suffix, row.inline, row.needs, row.option) == ("dmr", "find_dmr", 29, "dmr", False, "identify", "--find-dmr")
    assert all(layer.needs is None for layer in FL.FIND_LAYERS)
    on = dict(describe=True, keying=True, identify=True)
    assert [l.name for l in FL.active_layers({**on, "dmr": True})] == ["describe", "keying", "identify", "dmr"]
    assert [l.name for l in FL.active_layers({**on, "flex": True, "dmr": True})] == ["describe", "keying", "identify", "flex", "dmr"]
    assert [l.name for l in FL.active_layers(on)] == ["describe", "keying", "identify"]
    with pytest.raises(ValueError, match="dmr=True needs identify=True"):
        FL.active_layers(dict(describe=True, keying=True, dmr=True))
    with pytest.raises(ValueError, match="identify=True needs keying=True"):  # the chain's own errors come first
        FL.active_layers(dict(describe=True, identify=True, dmr=True))
    plan = P.plan_find(2.4e6, 100_000)
    fin = dict(runs=np.zeros((0, 8), dtype=np.int64), on=np.zeros((0, plan.slices), dtype=np.uint8))
    with pytest.raises(ValueError, match="dmr=True needs identify=True"):
        DS.ChannelDescriber(plan, fin, [], keying=True, dmr=True)
    with pytest.raises(ValueError, match="dmr=True needs identify=True"):
        A.find_channels("nothing.wav", describe=True, keying=True, dmr=True)
    with pytest.raises(ValueError, match="the describer was made without dmr=True"):
        DS.ChannelDescriber(plan, fin, [], keying=True, identify=True).finish_dmr()
    assert DS.ChannelDescriber(plan, fin, [], keying=True, identify=True, dmr=True)._names == ("describe", "keying", "identify", "dmr")


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        cli.main(argv)
    assert exc.value.code == 2
    return capsys.readouterr().err


def test_cli_flags(capsys):
    base = ["--in", "capture.wav"]
    args = cli.build_parser().parse_args(base + ["--find-dmr"])
    assert (args.find_dmr, args.find_identify) == (True, False)
    assert cli.check_find_args(cli.build_parser(), args) is True
    assert (args.find_dmr, args.find_identify, args.find_decode, args.find_flex, args.find_describe) == (True, True, True, False, False)
    args = cli.build_parser().parse_args(base + ["--find-flex"])
    assert cli.check_find_args(cli.build_parser(), args) is True and args.find_dmr is False
    args = cli.build_parser().parse_args(base + ["--find-flex", "--find-dmr"])
    assert cli.check_find_args(cli.build_parser(), args) is True and (args.find_dmr, args.find_flex, args.find_identify) == (True, True, True)
    assert "--find-dmr cannot be combined with --ft." in _usage_error(base + ["--find-dmr", "--ft", "455800000"], capsys)
    assert "--find-dmr needs --in." in _usage_error(["--find-dmr"], capsys)
    assert "--find-auto needs --find-top." in _usage_error(base + ["--find-dmr", "--find-auto"], capsys)
    text = "".join(cli.build_parser().format_help().split())
    (row,) = [l for l in FL.FIND_BRANCHES if l.name == "dmr"]
    assert "--find-dmr" in text and "".join(row.help.split()) in text


def test_package_surface():
    for name in ("DmrBurst", "DmrCall", "DmrResult", "DmrDecoder"):
        assert getattr(A, name) is getattr(X, name)
    text = Path(X.__file__).read_text()
    assert "scipy" not in text and "import oracle" not in text and "from oracle" not in text
    for name in ("slice_bursts", "decode_bursts", "check_lc", "check_csbk", "parse_bursts", "track_calls", "decode_stream", "finish_dmr",
                 "dmr_result", "stage_keys"):
        assert callable(getattr(X, name))


def test_c_abi_refuses_bad_arguments():
    """The library has the two entry points, and the argument checks come before the launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some = c_void_p(0), c_void_p(8)  # (never dereferenced: every call below is refused, or has nothing to do)
    for name in ("iqa_dmr_slice", "iqa_dmr_decode"):
        assert hasattr(N.lib(), name) and name in N.EXPORTS
    assert N.lib().iqa_abi_version() == 1
    plan = P.plan_dmr(FS)

    def slice_(plane=some, n=100_000, hits=some, k=2, offsets=plan.offsets, bits=some, levels=some):
        off = None if offsets is None else (c_int32 * 144)(*offsets)
        N.call("iqa_dmr_slice", plane, c_int64(n), hits, c_int64(k), off, bits, levels, null)

    def offs(at, value):
        o = list(plan.offsets)
        o[at] = value
        return tuple(o)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(k=-1), "negative"), (dict(n=(1 << 30) + 1), "2\\^30"), (dict(k=(1 << 20) + 1), "2\\^20"),
                         (dict(offsets=None), "NULL offsets"), (dict(offsets=offs(66, 1)), "o\\[0\\]"), (dict(offsets=offs(40, -9000)), "ascend"),
                         (dict(offsets=offs(143, plan.offsets[142] + 226)), "step"), (dict(plane=null), "NULL"), (dict(hits=null), "NULL"),
                         (dict(bits=null), "NULL"), (dict(levels=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            slice_(**kwargs)
    slice_(plane=null, hits=null, bits=null, levels=null, n=0)  # nothing to do: no pointer is touched
    slice_(plane=null, hits=null, bits=null, levels=null, k=0)

    def decode(bits=some, kinds=some, k=2, info=some, rec=some):
        N.call("iqa_dmr_decode", bits, kinds, c_int64(k), info, rec, null)

    for kwargs, what in ((dict(k=-1), "negative"), (dict(k=(1 << 20) + 1), "2\\^20"), (dict(bits=null), "NULL"), (dict(kinds=null), "NULL"),
                         (dict(info=null), "NULL"), (dict(rec=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            decode(**kwargs)
    decode(bits=null, kinds=null, info=null, rec=null, k=0)

    # the sign and the kind of a hit lie in device memory for the kernels: the package checks them before anything is launched
    class Plane:
        def numel(self):
            raise AssertionError("checked before the plane is looked at")

    for rows in ([(100, 0, 1)], [(100, 2, 1)], [(100, 1, 4)], [(100, -1, -1)]):
        with pytest.raises(ValueError, match="sign must be \\+-1 and its kind 0 .. 3"):
            X.slice_bursts(Plane(), rows, plan)
    with pytest.raises(ValueError, match="a kind must be 0 .. 3"):
        X.decode_bursts(np.zeros((1, 9), dtype=np.uint32), [4])
    with pytest.raises(ValueError, match="one kind to a burst"):
        X.decode_bursts(np.zeros((2, 9), dtype=np.uint32), [1])


# ---- the oracle end to end ----------------------------------------------------------------------------------------------------------


def _strip(bursts):
    return [{k: v for k, v in b.items() if k not in ("corrected", "time_s")} for b in bursts]


@pytest.mark.parametrize("noise", [0.0, NOISE])
def test_oracle_end_to_end(noise):
    clean = DM.decode_theta(DM.test_stream(FS), FS)
    out = clean if not noise else DM.decode_theta(DM.test_stream(FS, noise=noise), FS)
    assert len(out["rows"]) == 31 and out["rows"][:, 2].tolist().count(0) == 3 and set(out["rows"][:, 2].tolist()) == {0, 1}
    assert out["counts"] == dict(no_level=0, cut=0, slot_refused=0, bptc_failed=0, check_failed=0, idle=24, tact_fixed=out["counts"]["tact_fixed"])
    assert _strip(out["bursts"]) == _strip(clean["bursts"])
    (call,) = out["calls"]
    assert (call["slot"], call["cc"], call["group"], call["src"], call["dst"], call["superframes"], call["terminated"]) == (1, 1, True, DM.SRC, DM.DST, 3, True)
    assert [b["data_type"] for b in out["bursts"] if b["data_type"] not in (None, 9)] == [1, 1, 3, 2]
    flips, distance = int(out["rec"][:, 6].sum()), int(out["rec"][:, 3].sum())
    print("noise", noise, "flips", flips, "slot-type distance", distance, "tact fixed", out["counts"]["tact_fixed"])
    assert (flips > 0 and distance > 0) if noise else (flips == 0 and distance == 0 and out["counts"]["tact_fixed"] == 0)
    # the two forms of the slicing agree, here and at the stream's ends
    pl = out["plan"]
    rows = np.concatenate([out["rows"], [(5, 1, 0), (len(out["v"]) - 3, -1, 3), (pl["o"][54] + 1, -1, 1)]])
    bits, levels = DM.slice_all(out["v"], rows, pl)
    for j, (m, s, kind) in enumerate(rows.tolist()):
        w, lev = DM.slice_by_loops(out["v"], len(out["v"]), m, s, kind, pl)
        assert bits[j].tolist() == w and levels[j].tolist() == lev, j
    assert levels[-3:, 2].tolist() == [0, 0, 1]


def test_the_next_noise_level_loses_a_burst():
    out = DM.decode_theta(DM.test_stream(FS, noise=NOISE + 0.01), FS)
    assert out["counts"]["bptc_failed"] + out["counts"]["slot_refused"] + out["counts"]["check_failed"] > 0


def test_model_capture_reads_fsk_4800_and_dmr():
    """The model capture of the GPU test's CLI run, through the numpy finder, the float64 channelizer, section 23's keying and
    section 25's identification: it reads ``fsk 4800`` and ``dmr``, and the oracle finds the call and the CSBK."""
    dmr, voice = DM.model_run()
    assert dmr["keyed"]["label"] == "fsk 4800" and voice["keyed"]["label"] == "unkeyed" and voice["dmr"] is None
    assert (dmr["named"]["protocol"], dmr["named"]["confirmed"]) == ("dmr", True)
    assert 4.0 <= dmr["described"]["plan"]["fs_ch"] / 4800.0 <= 224.0
    out = dmr["dmr"]
    (call,) = out["calls"]
    assert (call["slot"], call["cc"], call["group"], call["src"], call["dst"], call["superframes"], call["terminated"]) == (1, 1, True, DM.SRC, DM.DST, 3, True)
    assert [(b["data_type"], b["slot"], b["checked"]) for b in out["bursts"] if b["data_type"] not in (None, 9)] == [
        (1, 1, True), (1, 1, True), (3, 2, True), (2, 1, True)]
    assert out["counts"]["bptc_failed"] == out["counts"]["slot_refused"] == out["counts"]["check_failed"] == out["counts"]["no_level"] == 0
