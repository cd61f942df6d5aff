"""The NXDN frame decoding (--find-nxdn) without a GPU: the anchors that section 34 states (the frame sync
word's sums, the scrambler's mask, the convolutional code's impulse, the punctured counts, the three CRCs), the properties of the
codes on the model's coders, the level rule, ``plan_nxdn`` against the model's plan, the package's LICH reader, checks, parser,
superframe joiner, call tracker and control folder against the model's on hand-made frames, the JSON round trip, the layer
table's row, the CLI's flag, the package surface, the entry points' argument checks, the model end to end on synthesised theta
(clean, negated, at 2400 symbols/s, the control stream, and at the noise level found here) and the model capture of the GPU
test's CLI run through the numpy pipeline."""
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
from iq_to_audio_amd import dsp_plan as P
from iq_to_audio_amd import find_layers as FL
from iq_to_audio_amd import nxdn as X


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


NM = _load("nxdn_model")
FS = 160_000.0
#: radians of white noise on theta: the largest of 0.01, 0.02, ... at which the model alone still decodes every frame of the test
#: stream and nothing else (found on the CPU by ``test_the_noise_level_is_the_largest_that_decodes``: at 0.07 the ten-symbol
#: frame sync word is found once more in the noisy voice bits, a twelfth frame whose LICH fails its parity)
NOISE = 0.06
CLEAN = dict(no_level=0, cut=0, lich_inner=0, lich_failed=0, sacch_failed=0, facch_failed=0, cac_failed=0, superframe_broken=0, udch=0,
             inbound_cac=0, fixed=0)
ROOT = Path(__file__).resolve().parent.parent


# ---- the anchors ----------------------------------------------------------------------------------------------------------------------


def test_constants_are_the_models():
    assert X.SYNC == NM.FSW == 0xCDF59 and [(p.protocol, p.word, p.symbols) for p in X.NXDN_PATTERNS] == [(p[0], p[3], p[4]) for p in NM.NXDN_PATTERNS]
    assert (X.SYNC_SYMBOLS, X.LEVEL_SCALE, X.HANG_S, X.NEED_LICH, X.NEED_FRAME) == (10, NM.SCALE, NM.HANG_S, NM.NEED_LICH, NM.NEED_FRAME) == (10, 370, 0.36, 18, 192)
    assert (P.NXDN_OFFSETS, P.NXDN_WORDS, P.NXDN_INFO, P.NXDN_RECORD) == (NM.OFFSETS, NM.WORDS, NM.INFO, NM.RECORD) == (192, 12, 14, 4)
    assert X.PLANE_RATES == (4800, 2400) and (X.SACCH, X.FACCH1_A, X.FACCH1_B, X.CAC) == (1, 2, 4, 8) and X.MESSAGES == NM.NAMES and X.CALL_TYPES == NM.CALL_TYPES
    assert {k: v[:5] for k, v in NM.BLOCKS.items()} == X.CODES and NM.CRC == X.CRCS
    header = (ROOT / "include" / "iqa_hotpath.h").read_text()
    for text in ("#define IQA_NXDN_OFFSETS 192", "#define IQA_NXDN_WORDS 12", "#define IQA_NXDN_INFO 14", "#define IQA_NXDN_RECORD 4",
                 "#define IQA_NXDN_CAC 8", "#define IQA_ABI_VERSION 1"):
        assert text in header


def test_the_frame_sync_word_and_the_scrambler():
    s = NM.fsw_levels()
    assert s == [-3, 1, -3, 3, -3, -3, 3, 3, -1, 3] == list(A.identify.symbols_of(X.NXDN_PATTERNS[0]))
    assert sum(s) == 0 and sum(x * x for x in s) == 74
    assert NM.pn()[:9] == [0, 0, 1, 0, 0, 1, 1, 1, 0] and len(NM.pn()) == 182 and X.scrambler() == NM.pn()
    mask = NM.scramble_mask()
    assert bytes(NM.bits_bytes(mask)) == NM.MASK_BYTES and sum(mask) == 92 and not any(mask[1::2]) and not any(mask[:20])
    assert NM.MASK_BYTES.hex(" ").upper().startswith("00 00 00 82 A0 88 8A 00 A2 A8 82 8A") and NM.MASK_BYTES.hex().upper().endswith("08A0AA02")


def test_the_code_its_puncturing_and_its_interleavers():
    assert NM.conv_encode([1])[:10] == [1, 1, 0, 1, 0, 1, 1, 0, 1, 1]  # the impulse sends 11 01 01 10 11
    for kind, sent in (("sacch", 60), ("facch1", 144), ("cac", 300)):
        steps, _where, _period, depth, cols, _first = NM.BLOCKS[kind]
        width, _poly, _init, covered = NM.CRC[kind]
        assert covered + width + 4 == steps
        assert sum(1 for j in range(2 * steps) if not NM.punctured(j, kind)) == sent == depth * cols
        assert sorted(NM.channel_index(p, kind) for p in range(sent)) == list(range(sent))  # a permutation


def test_the_crc_anchors():
    for kind, size, zeros, first in (("sacch", 26, 0x2B, 0x25), ("facch1", 80, 0x891, 0xD99), ("cac", 155, 0xCBAD, 0x1D61)):
        width, poly, init, covered = X.CRCS[kind]
        assert covered == size
        for bits, want in (([0] * size, zeros), ([1] + [0] * (size - 1), first)):
            assert NM.crc(bits, kind) == want == X.crc_bits(bits, width, poly, init)
    text = NM.bytes_bits(b"123456789")
    assert NM.crc(text, "cac") == 0x29B1 == X.crc_bits(text, 16, 0x1021, 0xFFFF)


# ---- the coders -----------------------------------------------------------------------------------------------------------------------


def test_the_encoder_round_trips_every_class():
    cases = NM.coder_cases()
    for name, (item, mask, _first, _sent) in NM.BLOCK_CASES.items():
        words = cases[name][0]
        info, rec, _ = NM.decode_frame(words, mask)
        assert rec == [mask, 0, 0, 0]
        assert X.lich_of(words) == NM.lich_of(words) == (item["lich"], True) and NM.lich_mask(item["lich"]) & mask
    head = cases["facch1-a"][0]
    info, rec, _ = NM.decode_frame(head, 7)
    assert rec == [7, 0, 0, 0] and X.check_sacch(info[0:2]) and X.check_facch1(info[2:5]) and X.check_facch1(info[5:8]) and not any(info[8:])
    assert NM.block_ok(info[2:5], "facch1") == (NM.bytes_bits(NM.VCALL), True) == NM.block_ok(info[5:8], "facch1")
    assert NM.block_ok(info[0:2], "sacch") == (NM.sacch_info(0, NM.RAN, NM.bytes_bits(NM.VCALL)[:18]), True)
    info, rec, _ = NM.decode_frame(cases["cac"][0], 8)
    assert X.check_cac(info[8:14]) and NM.block_ok(info[8:14], "cac") == (NM.cac_info(0, NM.RAN, NM.SITE_INFO), True) and not any(info[:8])
    # a spoiled CRC is seen by both
    bad = NM.frame_words(NM.header_frame(**{"break": ("sacch", "fb")}))
    info = NM.decode_frame(bad, 7)[0]
    assert (X.check_sacch(info[0:2]), X.check_facch1(info[2:5]), X.check_facch1(info[5:8])) == (False, True, False)
    assert not X.check_cac(NM.decode_frame(NM.frame_words(NM.cac_frame(NM.IDLE, **{"break": ("cac",)})), 8)[0][8:14])
    # masks that read nothing
    for cls in (0, 9, 12, 15, 16, 255):
        info, rec, _ = NM.decode_frame(head, cls)
        assert not any(info) and rec == [0, 0, 0, 0]


@pytest.mark.parametrize("name", list(NM.BLOCK_CASES))
def test_one_flipped_channel_bit_is_restored_anywhere(name):
    item, mask, first, sent = NM.BLOCK_CASES[name]
    words = NM.frame_words(item)
    clean = NM.decode_frame(words, mask)
    slot = {"sacch": 1, "cac": 1, "facch1-a": 2, "facch1-b": 3}[name]
    for k in range(0, sent, 1 if sent <= 60 else 3):
        info, rec, _ = NM.decode_frame(NM.flipped_words(words, [first + k]), mask)
        assert info == clean[0] and rec[slot] == 1, k


@pytest.mark.parametrize("name", list(NM.BLOCK_CASES))
def test_the_tie_rule_matters_on_the_found_input(name):
    words, mask, flips = NM.tie_case(name)
    first, second = NM.decode_frame(words, mask), NM.decode_frame(words, mask, smaller=False)
    assert first[2] > 0 and first[0] != second[0] and first[1] == second[1] and len(flips) <= 3


def test_the_level_rule_is_exact():
    s = NM.fsw_levels()
    for a, dc, sign in ((1000, 0, 1), (1000, 777, 1), (1000, -123_456, -1), (1, 5, 1), (NM.IM.V_MAX // 3, 0, -1), (NM.IM.V_MAX // 6, NM.IM.V_MAX // 2, 1)):
        x = [sign * a * g + dc for g in s]
        assert max(abs(v) for v in x) <= NM.IM.V_MAX
        assert NM.levels_of(x, sign) == (370 * 3 * a, 370 * dc)
        assert NM.levels_of(x, -sign) == (-370 * 3 * a, 370 * dc)
    assert 15 * 26 * NM.IM.V_MAX * 3 < 1 << 50


def test_the_lich():
    for rf in range(4):
        for fn in range(4):
            for option in range(4):
                byte = NM.lich_byte(rf, fn, option, outbound=option & 1)
                f = X.lich_fields(byte)
                assert f == dict(NM.lich_parts(byte), parity_ok=True) and NM.lich_parity_ok(byte) and not X.lich_fields(byte ^ 1)["parity_ok"]
                assert not X.lich_fields(byte ^ 0x40)["parity_ok"] and X.lich_fields(byte ^ 0x0C)["parity_ok"]  # (the parity covers b7 .. b4 alone)
                assert X.lich_mask(rf, fn, option) == NM.lich_mask(byte)
    assert [X.lich_mask(1, 0, o) for o in range(4)] == [7, 5, 3, 1] and X.lich_mask(0, 0, 0) == 8
    assert [X.lich_mask(0, 1, 0), X.lich_mask(0, 3, 0), X.lich_mask(1, 1, 0), X.lich_mask(2, 2, 3), X.lich_mask(3, 3, 3)] == [0, 0, 0, 1, 1]
    inner = NM.frame_words(dict(NM.header_frame(), inner=3))
    assert X.lich_of(inner) == NM.lich_of(inner) == (NM.lich_byte(1, 0, 0), False)


@pytest.mark.parametrize("fs_ch,rate", [(19_200.0, 4800), (160_000.0, 4800), (160_000.0, 2400), (96_600.0, 4800), (537_600.0, 2400), (9_600.0, 2400)])
def test_plan_against_the_model(fs_ch, rate):
    plan, want = A.plan_nxdn(fs_ch, rate), NM.plan(fs_ch, rate)
    assert isinstance(plan, A.NxdnPlan) and list(plan.offsets) == want["o"] and len(plan.offsets) == 192 and plan.sps == want["sps"] and plan.rate == rate
    assert (plan.ident.rate, plan.ident.window, plan.ident.half, plan.ident.shift) == (rate, want["ident"]["L"], want["ident"]["h"], want["ident"]["sh"])
    assert plan.o(0) == 0 and plan.o(191) == plan.offsets[191]


def test_plan_refuses_what_does_not_fit():
    assert A.plan_nxdn(48_000.0).rate == 4800
    for fs_ch, rate in ((19_199.0, 4800), (1_075_201.0, 4800), (9_599.0, 2400), (537_601.0, 2400), (48_000.0, 1600), (48_000.0, 9600), (0.0, 4800)):
        with pytest.raises(ValueError):
            A.plan_nxdn(fs_ch, rate)
        with pytest.raises(ValueError):
            NM.plan(fs_ch, rate) if fs_ch else A.plan_nxdn(fs_ch, rate)
    with pytest.raises(ValueError):
        A.NxdnDecoder(48_000.0, rate=1200)


# ---- the host rules on hand-made frames ----------------------------------------------------------------------------------------------

STEP = 6400  # samples of a 40 ms frame at FS


def _arrays(items, at=None, valid=None, amp=None):
    """(rows, bits, levels, info, rec) of hand-made frames through the model's encoder and coders; ``at``: their frame slots."""
    at = list(range(len(items))) if at is None else at
    rows = np.array([(100 + int(STEP * t), 1) for t in at], dtype=np.int64).reshape(-1, 2)
    bits = np.array([NM.frame_words(item, seed=j) for j, item in enumerate(items)], dtype=np.uint32).reshape(-1, 12)
    levels = np.array([[1110 if amp is None else amp[j], 0, 192 if valid is None else valid[j]] for j in range(len(items))], dtype=np.int64).reshape(-1, 3)
    classes = NM.decoder_classes(bits, levels)
    assert X.decoder_classes(bits, levels).tolist() == classes
    info, rec = NM.decode_all(bits, classes)
    return rows, bits, levels, info, rec


def _both(arrays):
    """The package's frames, counts, calls and control lines, held to the model's."""
    frames, counts = X.parse_frames(*arrays, FS)
    want_frames, want_counts = NM.parse(*arrays, FS)
    assert [f.to_json() for f in frames] == want_frames and counts == want_counts
    calls, control = X.track_calls(frames), X.fold_control(frames)
    assert [c.to_json() for c in calls] == NM.track(want_frames) and [c.line() for c in calls] == [NM.call_line(c) for c in NM.track(want_frames)]
    assert [c.to_json() for c in control] == NM.fold(want_frames) and [c.line() for c in control] == [NM.control_line(c) for c in NM.fold(want_frames)]
    assert [f.kind() for f in frames] == [NM.frame_kind(f) for f in want_frames]
    return frames, counts, calls, control


SUPERFRAME = [NM.voice_frame(p) for p in (3, 2, 1, 0)]


def test_a_superframe_joined():
    frames, counts, calls, _ = _both(_arrays([NM.header_frame()] + SUPERFRAME))
    assert counts == CLEAN and [len(f.messages) for f in frames] == [3, 0, 0, 0, 1]
    msg = frames[4].messages[0]
    assert (msg["via"], msg["name"], msg["src"], msg["dst"], msg["hex"]) == ("sacch", "VCALL", 1234, 5678, bytes(NM.vcall(size=9)).hex())
    assert [m["via"] for m in frames[0].messages] == ["sacch", "facch1-a", "facch1-b"] and frames[0].messages[0] == dict(via="sacch", type=1, name="VCALL", hex="00400")
    assert [(f.structure, f.ran) for f in frames] == [(0, 5), (3, 5), (2, 5), (1, 5), (0, 5)]
    assert [c.line() for c in calls] == ["NXDN RAN 5 1234 -> 5678 group clear 0.16 s (5 frames)"] and calls[0].late is False and calls[0].conflicts == 0


def test_a_superframe_broken():
    spoiled = dict(NM.voice_frame(2), **{"break": ("sacch",)})
    other_ran = dict(NM.voice_frame(1), sacch=(1, 9, [0] * 18))
    cases = (([SUPERFRAME[0], spoiled, SUPERFRAME[2], SUPERFRAME[3]] + SUPERFRAME, None, 1, 1),  # a failed part: once, the rest passed over
             (SUPERFRAME[:2] + SUPERFRAME[3:], [0, 1, 3], 0, 1),  # a missing part
             (SUPERFRAME[:3] + SUPERFRAME, None, 0, 1),  # a new part 3 while one is open
             (SUPERFRAME[:2] + [other_ran, SUPERFRAME[3]], None, 0, 1),  # another RAN
             (SUPERFRAME[1:] + SUPERFRAME, None, 0, 1),  # joined in the middle: the first is dropped, the second whole
             (SUPERFRAME[:2] + [NM.header_frame(NM.TX_REL)], None, 0, 1),  # ended by a frame outside it
             (SUPERFRAME + SUPERFRAME[:3], None, 0, 1))  # cut by the end
    for items, at, failed, broken in cases:
        frames, counts, _, _ = _both(_arrays(items, at))
        assert counts == dict(CLEAN, sacch_failed=failed, superframe_broken=broken), (len(items), counts)
        joined = sum(1 for f in frames for m in f.messages if m["via"] == "sacch" and f.fn == 2)
        assert joined == (1 if len(items) >= 7 else 0)


def test_a_late_join_and_the_fields_it_learns():
    frames, counts, calls, _ = _both(_arrays(SUPERFRAME[2:] + SUPERFRAME + [NM.header_frame(NM.TX_REL)]))
    (call,) = calls
    assert (call.late, call.released, call.frames, call.ran, call.src, call.dst, call.conflicts) == (True, True, 7, 5, 1234, 5678, 0)
    assert counts == dict(CLEAN, superframe_broken=1)
    # without a VCALL the line keeps to what is known
    frames, counts, calls, _ = _both(_arrays(SUPERFRAME[2:]))
    assert [c.line() for c in calls] == ["NXDN RAN 5 0.04 s (2 frames)"] and calls[0].late is True
    # a header whose FACCH1s fail is no opening
    frames, counts, calls, _ = _both(_arrays([NM.header_frame(**{"break": ("fa", "fb")})] + SUPERFRAME))
    assert calls[0].late is True and counts == dict(CLEAN, facch_failed=2) and calls[0].src == 1234


def test_the_hang_on_either_side():
    below, above = 0.36 * FS / STEP, 0.36 * FS / STEP + 0.001  # exactly 0.36 s apart, and a little more
    _, _, calls, _ = _both(_arrays([NM.header_frame(), NM.voice_frame(3)], [0, below]))
    assert len(calls) == 1 and calls[0].frames == 2 and abs(calls[0].end_s - calls[0].start_s - 0.36) < 1e-9
    _, _, calls, _ = _both(_arrays([NM.header_frame(), NM.voice_frame(3)], [0, above]))
    assert [(c.frames, c.late, c.released) for c in calls] == [(1, False, False), (1, True, False)]


def test_a_conflict_keeps_the_first_value_and_two_calls():
    other = NM.vcall(src=4321, dst=5678, call_type=4, cipher=2, key=7)
    frames, counts, calls, _ = _both(_arrays([NM.header_frame(), NM.header_frame(other), NM.header_frame(NM.TX_REL), NM.header_frame(other),
                                              dict(NM.header_frame(NM.TX_REL), sacch=(0, 9, [0] * 18))]))
    assert [(c.src, c.dst, c.call_type, c.cipher, c.key, c.ran, c.conflicts, c.released, c.frames) for c in calls] == [
        (1234, 5678, 1, 0, 0, 5, 8, True, 3), (4321, 5678, 4, 2, 7, 5, 1, True, 2)]  # (src, type, cipher, key in both FACCH1s; then the RAN)
    assert [c.line() for c in calls] == ["NXDN RAN 5 1234 -> 5678 group clear 0.08 s (3 frames)", "NXDN RAN 5 4321 -> 5678 individual cipher 2 0.04 s (2 frames)"]
    assert X.NxdnCall(0.0, 1.0, 1, None, 7, 8, 5, 1, 0, 3, 1, True, False, 0).line() == "NXDN 7 -> 8 5 cipher 3 1.00 s (1 frame)"


def test_cac_folding():
    items = [NM.cac_frame(NM.SITE_INFO), NM.cac_frame(NM.SRV_INFO), NM.cac_frame(NM.IDLE), NM.cac_frame(NM.IDLE, ran=9), NM.cac_frame(NM.SITE_INFO),
             NM.cac_frame([0x2A, 1, 2]), NM.cac_frame(NM.IDLE, **{"break": ("cac",)})]
    frames, counts, calls, control = _both(_arrays(items))
    assert calls == [] and counts == dict(CLEAN, cac_failed=1)
    assert [(c.ran, c.name, c.count) for c in control] == [(5, "SITE_INFO", 2), (5, "SRV_INFO", 1), (5, "IDLE", 1), (9, "IDLE", 1), (5, "0x2A", 1)]
    assert control[0].line() == "NXDN RAN 5 SITE_INFO " + bytes(NM.SITE_INFO).hex() + " x2 0.00 .. 0.16 s"


def test_udch_inbound_cut_failed_and_no_level_frames():
    items = [dict(lich=NM.lich_byte(1, 1, 0)), dict(lich=NM.lich_byte(2, 1, 3)), dict(lich=NM.lich_byte(0, 1, 0, 0)), dict(lich=NM.lich_byte(0, 3, 0, 0)),
             dict(lich=NM.lich_byte(1, 0, 0, break_parity=True)), dict(NM.header_frame(), inner=5), NM.header_frame(), NM.header_frame(), NM.header_frame(),
             NM.cac_frame(NM.IDLE)]
    valid = [192, 192, 192, 192, 192, 192, 17, 18, 192, 191]
    amp = [1110] * 8 + [0, 1110]
    arrays = _arrays(items, valid=valid, amp=amp)
    assert NM.decoder_classes(arrays[1], arrays[2]) == [0, 0, 0, 0, 0, 7, 0, 0, 0, 0]
    frames, counts, calls, control = _both(arrays)
    assert counts == dict(CLEAN, udch=2, inbound_cac=2, lich_failed=1, lich_inner=1, cut=3, no_level=1)
    assert [f.kind() for f in frames] == ["RTCH UDCH", "RDCH UDCH", "RCCH long inbound", "RCCH short inbound", "RTCH non-superframe", "RTCH non-superframe",
                                          "RCCH outbound"]
    assert [f.blocks for f in frames[:4] + frames[5:]] == [[]] * 6 and len(frames[4].blocks) == 3  # seen, not read; cut behind the LICH
    assert control == [] and len(calls) == 1 and calls[0].frames == 4  # (the control frames belong to no call)


def test_frame_hits_keeps_the_larger_of_two_near_hits():
    pats = A.identify.patterns_for(4800)
    p = [j for j, pat in enumerate(pats) if pat.protocol == "nxdn"][0]
    hits = [(p, 1000, 500, 9, 0, 0), (p, 1005, -700, 9, 0, 0), (p, 3000, -400, 9, 0, 0), (0, 3002, 900, 9, 0, 0), (p, 5000, 300, 9, 0, 0), (p, 5016, 300, 9, 0, 0),
            (p, 5017, 300, 9, 0, 0)]
    assert X.frame_hits(hits, pats, 16).tolist() == [[1005, -1], [3000, -1], [5000, 1]]
    assert NM.frame_hits([(0,) + h[1:] for h in hits if h[0] == p], 16) == [(1005, -1), (3000, -1), (5000, 1)]
    assert X.frame_hits(np.zeros((0, 6)), pats, 16).shape == (0, 2)
    assert [pat.protocol for pat in A.identify.patterns_for(2400)] == ["nxdn"]


def test_result_round_trips_through_json():
    frames, counts, calls, control = _both(_arrays([NM.header_frame()] + SUPERFRAME + [NM.cac_frame(NM.IDLE)]))
    ch = X.NxdnChannel(offset_hz=12_500.0, freq_hz=None, rate=2400, frames={"RTCH superframe": 4}, calls=calls, control=control, **counts)
    res = X.NxdnResult(channels=[ch, X.NxdnChannel(offset_hz=-1.0, freq_hz=433e6, note="no nxdn channel")], sample_rate=2.4e6, center_freq=433e6)
    assert X.NxdnResult.from_json(json.loads(json.dumps(res.to_json()))) == res and res.calls == calls
    assert res.lines() == ["+12500 Hz: " + calls[0].line(), "+12500 Hz: " + control[0].line()]
    assert X.NxdnFrame.from_json(json.loads(json.dumps(frames[0].to_json()))) == frames[0]
    assert all(hasattr(cls, "to_json") and (hasattr(cls, "line") or hasattr(cls, "lines") or hasattr(cls, "kind"))
               for cls in (X.NxdnFrame, X.NxdnCall, X.NxdnControl, X.NxdnChannel, X.NxdnResult))


# ---- the layer table, the CLI, the package surface, the C ABI -----------------------------------------------------------------------


def test_the_row_of_the_layer_table():
    assert [l.name for l in FL.FIND_BRANCHES[:2]] == ["dmr", "p25"]  # still a prefix: the rows before this one stay where they were
    (row,) = [l for l in FL.FIND_BRANCHES if l.name == "nxdn"]
    assert FL.FIND_BRANCHES.index(row) == 3 > [l.name for l in FL.FIND_BRANCHES].index("ysf")
    assert (row.flag, row.section, row.suffix, row.inline, row.needs, row.option) == ("find_nxdn", 34, "nxdn", False, "identify", "--find-nxdn")
    on = dict(describe=True, keying=True, identify=True)
    assert [l.name for l in FL.active_layers({**on, "nxdn": True})] == ["describe", "keying", "identify", "nxdn"]
    assert [l.name for l in FL.active_layers({**on, "flex": True, "dmr": True, "p25": True, "ysf": True, "nxdn": True})] == [
        "describe", "keying", "identify", "flex", "dmr", "p25", "ysf", "nxdn"]
    assert [l.name for l in FL.active_layers(on)] == ["describe", "keying", "identify"]
    with pytest.raises(ValueError, match="nxdn=True needs identify=True"):
        FL.active_layers(dict(describe=True, keying=True, nxdn=True))
    plan = P.plan_find(2.4e6, 100_000)
    fin = dict(runs=np.zeros((0, 8), dtype=np.int64), on=np.zeros((0, plan.slices), dtype=np.uint8))
    with pytest.raises(ValueError, match="nxdn=True needs identify=True"):
        DS.ChannelDescriber(plan, fin, [], keying=True, nxdn=True)
    with pytest.raises(ValueError, match="nxdn=True needs identify=True"):
        A.find_channels("nothing.wav", describe=True, keying=True, nxdn=True)
    with pytest.raises(ValueError, match="the describer was made without nxdn=True"):
        DS.ChannelDescriber(plan, fin, [], keying=True, identify=True, ysf=True).finish_nxdn()
    assert DS.ChannelDescriber(plan, fin, [], keying=True, identify=True, ysf=True, nxdn=True)._names == ("describe", "keying", "identify", "ysf", "nxdn")


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        cli.main(argv)
    assert exc.value.code == 2
    return capsys.readouterr().err


def test_cli_flags(capsys):
    base = ["--in", "capture.wav"]
    args = cli.build_parser().parse_args(base + ["--find-nxdn"])
    assert (args.find_nxdn, args.find_identify, args.find_ysf) == (True, False, False)
    assert cli.check_find_args(cli.build_parser(), args) is True
    assert (args.find_nxdn, args.find_identify, args.find_decode, args.find_flex, args.find_dmr, args.find_p25, args.find_ysf, args.find_describe) == (
        True, True, True, False, False, False, False, False)
    args = cli.build_parser().parse_args(base + ["--find-ysf"])
    assert cli.check_find_args(cli.build_parser(), args) is True and args.find_nxdn is False
    args = cli.build_parser().parse_args(base + ["--find-flex", "--find-dmr", "--find-p25", "--find-ysf", "--find-nxdn"])
    assert cli.check_find_args(cli.build_parser(), args) is True
    assert (args.find_nxdn, args.find_ysf, args.find_p25, args.find_dmr, args.find_flex, args.find_identify) == (True,) * 6
    assert "--find-nxdn cannot be combined with --ft." in _usage_error(base + ["--find-nxdn", "--ft", "433200000"], capsys)
    assert "--find-nxdn needs --in." in _usage_error(["--find-nxdn"], capsys)
    text = "".join(cli.build_parser().format_help().split())
    (row,) = [l for l in FL.FIND_BRANCHES if l.name == "nxdn"]
    assert "--find-nxdn" in text and "".join(row.help.split()) in text


def test_package_surface():
    for name in ("NxdnFrame", "NxdnCall", "NxdnControl", "NxdnChannel", "NxdnResult", "NxdnDecoder"):
        assert getattr(A, name) is getattr(X, name)
    assert A.plan_nxdn is P.plan_nxdn and A.NxdnPlan is P.NxdnPlan
    text = Path(X.__file__).read_text()
    assert "scipy" not in text and "import oracle" not in text and "from oracle" not in text
    doc = " ".join(X.__doc__.split())
    assert "from memory" in doc and "Not decoded: the voice" in doc and "UDCH" in doc  # where the constants come from, and what is left out
    for name in ("slice_frames", "lich_fields", "decoder_classes", "decode_frames", "check_sacch", "check_facch1", "check_cac", "join_superframes",
                 "layer3_fields", "parse_frames", "track_calls", "decode_stream", "channel_of", "finish_nxdn", "nxdn_result", "stage_keys"):
        assert callable(getattr(X, name))
    assert issubclass(X.NxdnDecoder, A.protocol_layer.StoredTheta) and X.NxdnDecoder(FS).rate == 4800 and X.NxdnDecoder(FS, rate=2400).plan.rate == 2400
    assert callable(DS.ChannelDescriber.finish_nxdn) and callable(DS.ChannelDescriber.nxdn_result) and DS._MODULES["nxdn"] is X
    assert "nxdn.hip" in (Path(X.__file__).parent / "csrc" / "Makefile").read_text()


def test_c_abi_refuses_bad_arguments():
    """The library has the two entry points, and the argument checks come before the launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some = c_void_p(0), c_void_p(8)  # (never dereferenced: every call below is refused, or has nothing to do)
    for name in ("iqa_nxdn_slice", "iqa_nxdn_decode"):
        assert hasattr(N.lib(), name) and name in N.EXPORTS
    assert N.lib().iqa_abi_version() == 1
    plan = P.plan_nxdn(FS)

    def slice_(plane=some, n=100_000, hits=some, k=2, offsets=plan.offsets, bits=some, levels=some):
        off = None if offsets is None else (c_int32 * 192)(*offsets)
        N.call("iqa_nxdn_slice", plane, c_int64(n), hits, c_int64(k), off, bits, levels, null)

    def offs(at, value):
        o = list(plan.offsets)
        o[at] = value
        return tuple(o)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(k=-1), "negative"), (dict(n=(1 << 30) + 1), "2\\^30"), (dict(k=(1 << 20) + 1), "2\\^20"),
                         (dict(offsets=None), "NULL offsets"), (dict(offsets=offs(0, 1)), "o\\[0\\]"), (dict(offsets=offs(40, -9000)), "ascend"),
                         (dict(offsets=offs(191, plan.offsets[190] + 226)), "step"), (dict(plane=null), "NULL"), (dict(hits=null), "NULL"),
                         (dict(bits=null), "NULL"), (dict(levels=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            slice_(**kwargs)
    slice_(plane=null, hits=null, bits=null, levels=null, n=0)  # nothing to do: no pointer is touched
    slice_(plane=null, hits=null, bits=null, levels=null, k=0)

    def decode(bits=some, classes=some, k=2, info=some, rec=some):
        N.call("iqa_nxdn_decode", bits, classes, c_int64(k), info, rec, null)

    for kwargs, what in ((dict(k=-1), "negative"), (dict(k=(1 << 20) + 1), "2\\^20"), (dict(bits=null), "NULL"), (dict(classes=null), "NULL"),
                         (dict(info=null), "NULL"), (dict(rec=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            decode(**kwargs)
    decode(bits=null, classes=null, info=null, rec=null, k=0)

    # the sign of a hit and the class mask lie in device memory for the kernels: the package checks them before anything is launched
    class Plane:
        def numel(self):
            raise AssertionError("checked before the plane is looked at")

    for rows in ([(100, 0)], [(100, 2)], [(100, -3)]):
        with pytest.raises(ValueError, match="sign must be \\+-1"):
            X.slice_frames(Plane(), rows, plan)
    for bad in ([9], [15], [16], [-1], [255]):
        with pytest.raises(ValueError, match="a class mask must be 0 .. 7 or 8"):
            X.decode_frames(np.zeros((1, 12), dtype=np.uint32), bad)
    with pytest.raises(ValueError, match="one class mask to a frame"):
        X.decode_frames(np.zeros((2, 12), dtype=np.uint32), [1])


# ---- the model end to end ----------------------------------------------------------------------------------------------------------


def _strip(frames):
    return [{k: v for k, v in f.items() if k not in ("corrected", "time_s")} for f in frames]


@pytest.fixture(scope="module")
def clean():
    return NM.decode_theta(NM.test_stream(FS), FS)


def _decodes_every_frame(out) -> bool:
    """Whether the model found the eleven frames of the test stream and nothing else, read every block of them and followed the call."""
    failed = {k: v for k, v in out["counts"].items() if v and k not in ("fixed", "lich_inner")}
    return len(out["rows"]) == 11 and out["classes"].tolist() == NM.CLASSES and not failed and [NM.call_line(c) for c in out["calls"]] == [NM.LINE]


@pytest.mark.parametrize("case", ["clean", "noise", "negated", "rate2400"])
def test_model_end_to_end(clean, case):
    args = dict(noise=dict(noise=NOISE), negated=dict(negate=True), rate2400=dict(rate=2400)).get(case, {})
    rate = 2400 if case == "rate2400" else 4800
    out = clean if case == "clean" else NM.decode_theta(NM.test_stream(FS, **args), FS, 0, rate)
    assert len(out["rows"]) == 11 and set(out["rows"][:, 1].tolist()) == ({-1} if case == "negated" else {1})
    assert _strip(out["frames"]) == _strip(clean["frames"]) and out["classes"].tolist() == NM.CLASSES and out["kinds"] == NM.KINDS
    (call,) = out["calls"]
    assert NM.call_line(call) == (NM.LINE.replace("0.40", "0.80") if rate == 2400 else NM.LINE)
    assert (call["late"], call["released"], call["conflicts"], call["ran"], call["mode"], call["emergency"]) == (False, True, 0, 5, 2, 0)
    changed = int(out["rec"][:, 1:].sum())
    print(case, "channel bits changed", changed, "fixed", out["counts"]["fixed"], "lich_inner", out["counts"]["lich_inner"])
    if case == "noise":
        assert changed > 0 and out["counts"]["fixed"] > 0 and out["counts"] == dict(CLEAN, fixed=out["counts"]["fixed"], lich_inner=out["counts"]["lich_inner"])
        assert np.abs(out["rows"][:, 0] - clean["rows"][:, 0]).max() <= 1
    else:
        assert changed == 0 and out["counts"] == CLEAN
    if case == "negated":
        np.testing.assert_array_equal(out["v"], -clean["v"])  # (no shift at this rate: the plane is the clean one negated)
        np.testing.assert_array_equal(out["bits"], clean["bits"])
        np.testing.assert_array_equal(out["levels"] * np.array([1, -1, 1]), clean["levels"])
        assert out["frames"] == clean["frames"] and out["calls"] == clean["calls"]
    if case == "rate2400":
        for name in ("bits", "classes", "info", "rec"):
            np.testing.assert_array_equal(out[name], clean[name], err_msg=name)
    # the slicing at the stream's ends
    pl = out["plan"]
    n = len(out["v"])
    rows = [(5, 1), (n - 3, -1), (n - pl["o"][17] - 1, 1), (n - pl["o"][17], -1), (-1, 1), (n + 5, 1)]
    _, levels = NM.slice_all(out["v"], rows, pl)
    assert levels[:, 2].tolist() == [192, 1, 18, 17, 0, 0]


def test_the_control_stream():
    out = NM.decode_theta(NM.test_stream(FS, script=NM.CONTROL_SCRIPT), FS)
    assert out["classes"].tolist() == [8] * 6 and out["counts"] == CLEAN and out["calls"] == [] and out["kinds"] == {"RCCH outbound": 6}
    assert [NM.control_line(c) for c in out["control"]] == NM.CONTROL_LINES
    assert len(NM.station(NM.SCRIPT)) / 4800.0 < 1.0 and len(NM.station(NM.CONTROL_SCRIPT)) / 4800.0 < 1.0  # both streams stay under a second


def test_the_noise_level_is_the_largest_that_decodes():
    """The search that NOISE comes from: sigma upward in steps of 0.01 rad until the model alone no longer decodes every frame."""
    sigma = 0.0
    while _decodes_every_frame(NM.decode_theta(NM.test_stream(FS, noise=round(sigma + 0.01, 2)), FS)):
        sigma = round(sigma + 0.01, 2)
        assert sigma < 0.5
    assert sigma == NOISE
    out = NM.decode_theta(NM.test_stream(FS, noise=round(NOISE + 0.01, 2)), FS)
    print("one step above:", len(out["rows"]), "rows", out["counts"])
    assert len(out["rows"]) == 12 and out["counts"]["lich_failed"] == 1  # a false frame sync in the voice bits


def test_model_capture_reads_fsk_4800_and_nxdn():
    """The model capture of the GPU test's CLI run, through the numpy finder, the float64 channelizer, section 23's keying and
    section 25's identification: it reads ``fsk 4800`` and ``nxdn``, and the model finds both calls."""
    nxdn, voice = NM.model_run()
    assert nxdn["keyed"]["label"] == "fsk 4800" and voice["keyed"]["label"] == "unkeyed" and voice["nxdn"] is None
    assert (nxdn["named"]["protocol"], nxdn["named"]["confirmed"], nxdn["named"]["rate"]) == ("nxdn", True, 4800)
    assert 4.0 <= nxdn["described"]["plan"]["fs_ch"] / 4800.0 <= 224.0
    out = nxdn["nxdn"]
    # (192 random symbols lead the capture; the second call runs until the capture ends.  A sync word of ten symbols is also
    # found in random and voice bits: of those false frames most fail the LICH's parity, and one reads as an inbound frame)
    assert [NM.call_line(c) for c in out["calls"]] == [NM.LINE, "NXDN RAN 5 4321 -> 8765 individual cipher 1 1.48 s (38 frames)"]
    assert [(c["late"], c["released"], c["conflicts"], c["key"]) for c in out["calls"]] == [(False, True, 0, 0), (False, False, 0, 9)]
    c = out["counts"]
    assert (c["sacch_failed"], c["facch_failed"], c["cac_failed"], c["no_level"], c["udch"]) == (0, 0, 0, 0, 0) and c["lich_failed"] > 0
    assert out["kinds"]["RTCH non-superframe"] == 4 and out["kinds"]["RTCH superframe"] >= 44
