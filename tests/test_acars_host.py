"""ACARS beside AM (--demod am --acars), the host side: the protocol constants pinned, the numpy oracle
(tests/acars_model.py) round trip over channel rates, clock errors and noise, no decode on voice and on noise, the walker on
hand-made symbol streams, ``plan_acars`` against the oracle's plan, the promised integer widths on the largest input, the
parser on fixed byte strings and the command line's usage errors.  No GPU needed."""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load("acars_model")

RATES, TEXT, stream, check_two_messages = M.RATES, M.TEXT, M.two_message_stream, M.check_two_messages


# ---- the oracle alone ---------------------------------------------------------------------------------------------------


def test_constants_are_pinned():
    assert M.crc16(b"123456789") == 0x2189
    assert len(M.PARITY) == 128 and all(bin(c).count("1") % 2 == 1 and c & 0x7F == k for k, c in enumerate(M.PARITY))
    assert [M.PARITY[c] for c in (0x2B, 0x2A, 0x16, 0x01, 0x03, 0x17, 0x7F, 0x02, 0x41)] == [0xAB, 0x2A, 0x16, 0x01, 0x83, 0x97, 0x7F, 0x02, 0xC1]
    assert M.OPENER == bytes(M.PARITY[c] for c in (0x2A, M.SYN, M.SYN, M.SOH)) and M.OPENER[-1] >> 7 == 0
    assert M.opener_symbols().size == 31


def test_a_hand_built_frame_byte_for_byte():
    body = M.body_bytes("2", ".N12345", "A", "H1", "2", "Hi")
    assert body == bytes([0x32, 0xAE, 0xCE, 0x31, 0x32, 0xB3, 0x34, 0xB5, 0xC1, 0xC8, 0x31, 0x32, 0x02, 0xC8, 0xE9, 0x83])
    reg = M.crc16(body)
    full = M.message_bytes(body, prekey=2)
    assert full == bytes([0xFF, 0xFF, 0xAB, 0x2A, 0x16, 0x16, 0x01]) + body + bytes([reg & 0xFF, reg >> 8, 0x7F])
    assert M.bits_of(bytes([0x2A])).tolist() == [0, 1, 0, 1, 0, 1, 0, 0]
    g = M.transitions(M.bits_of(full))
    (s,) = M.openers(g).tolist()
    assert s == 8 * 7 and M.walk(g, s) == (body + bytes([reg & 0xFF, reg >> 8]), True)


@pytest.mark.parametrize("ppm", [-50.0, 50.0])
@pytest.mark.parametrize("sigma", [0.0, 0.1, 0.2])
@pytest.mark.parametrize("fs", RATES)
def test_oracle_round_trip(fs, sigma, ppm):
    out = M.oracle(M.envelope(stream(fs, sigma, ppm)), fs)
    check_two_messages(out["messages"])
    assert out["reached"] >= len(out["records"]) == sum(m["hits"] for m in out["messages"])
    assert M.line(out["messages"][0]) == "ACARS .N12345 H1 2 M01A XX0123 " + TEXT[10:] and M.line(out["messages"][1]) == "ACARS .D-ABCD Q0 S"


def test_voice_and_noise_decode_to_nothing():
    fs = 96_000.0
    n = int(4 * fs)
    for z in (M.voice_am(n, fs, seed=3), M.noise_only(n, 1.0, seed=4)):
        out = M.oracle(M.envelope(z), fs)
        assert out["records"] == [] and out["messages"] == []
    assert M.oracle(np.zeros(1000, dtype=np.float32), fs)["q"] is None


def test_quantiser_range():
    """emax 2^sh lies in [2^14, 2^15); rounding takes the last 2^-9 below 2^15 up to 2^15 itself, and nothing goes beyond."""
    top = np.nextafter(np.float32(0.25), np.float32(0.0))
    for emax, qmax in ((np.float32(0.25), 2 ** 14), (top, 2 ** 15), (np.float32(0.25 - 2.0 ** -17), 2 ** 15 - 1), (np.float32(1e-30), None)):
        e = np.array([0.0, emax, emax / 2, emax / 3], dtype=np.float32)
        q, sh, got = M.quantise(e)
        assert got == emax and 2 ** 14 <= q.max() <= 2 ** 15 and (qmax is None or q.max() == qmax)
    assert M.quantise(np.array([0.5, 1.5, 2.5, 16384.0], dtype=np.float32))[0].tolist() == [0, 2, 2, 16384]  # sh = 0: half-even


def test_the_largest_input_keeps_the_promised_widths():
    """A full-scale 0 / emax square wave at 1800 Hz at every phase step: sums inside int32 (asserted by ``correlate``),
    |I|, |Q| < 2^23 (the 24-bit multiply is not needed for them, but the header promises it), |y| < 2^57."""
    for fs in (19_200.0, 21_600.0, 96_000.0, 957_600.0, 960_000.0):
        pl = M.plan(fs)
        worst = 0
        for phase in np.linspace(0.0, 2.0 * np.pi, 16, endpoint=False):
            q, sh, emax = M.quantise(M.square_wave(4 * pl["W"] + 2 * pl["L"], fs, 0.75, phase))
            assert q.max() == 3 << 13 and sh == 15
            q = np.where(q > 0, 2 ** 15, 0)  # the largest q any scale gives (emax within 2^-9 of the next power of two rounds up to it)
            I, Q = M.correlate(q, pl)
            y, _ = M.detect(I, Q, pl)
            worst = max(worst, int(np.abs(I).max()), int(np.abs(Q).max()))
            assert max(np.abs(I).max(), np.abs(Q).max()) < 2 ** 23 and np.abs(y).max() < 2 ** 57
        pos = max(np.maximum(pl["c"], 0).sum(), np.maximum(pl["s"], 0).sum(), -np.minimum(pl["c"], 0).sum(), -np.minimum(pl["s"], 0).sum())
        assert 2 ** 15 * int(pos) < 2 ** 31 and worst > 0.9 * (2 ** 15 * int(pos) >> 8)  # the square wave is the worst case


# ---- the walker and the parser --------------------------------------------------------------------------------------------


def test_walker_on_hand_made_symbol_streams():
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.decoders import acars as AC

    plan = P.plan_acars(96_000.0)
    seen = {}
    for name, g, count, expect in M.hand_made_streams():
        kept, reached = M.frames_of(g[:count])
        assert len(kept) == expect, name
        seen[name] = (kept, reached)
        rec = dict(phase=[0] * len(kept), s=[s for s, _ in kept], start=[int(plan.instant(s, 0)) for s, _ in kept],
                   nbytes=[len(raw) for _, raw in kept], data=np.array([list(raw.ljust(AC.SLOT_BYTES, b"\0")) for _, raw in kept], dtype=np.uint8))
        res = AC.parse_messages(plan, rec, reached)
        assert (res is None) == (expect == 0), name
        if res is not None:
            assert [m.raw for m in res.messages] == [raw.hex() for _, raw in kept] and res.candidates == reached and res.crc_ok == 1
    assert seen["plain"][0] == seen["inverted"][0]  # the polarity comes from SOH's last bit, not from the stream
    assert seen["12 bytes"][1] == seen["wrong BCS"][1] == seen["ends inside the BCS"][1] == 1  # reached ETX / ETB, not kept
    assert seen["241 bytes"][1] == seen["ends inside the body"][1] == 0
    assert len(seen["240 bytes"][0][0][1]) == 242 and len(seen["13 bytes"][0][0][1]) == 15
    raw = seen["ETX inside the BCS"][0][0][1]
    assert M.ETX in (raw[-1] & 0x7F, raw[-2] & 0x7F) and AC.crc16_kermit(raw[:-2]) == raw[-2] | (raw[-1] << 8)


def test_parser_on_fixed_byte_strings():
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.decoders import acars as AC

    assert AC.crc16_kermit(b"123456789") == 0x2189 and (AC.MIN_BODY, AC.MAX_BODY, AC.SLOT_BYTES) == (M.MIN_BODY, M.MAX_BODY, 244)
    plan = P.plan_acars(96_000.0)
    down = M.with_bcs(M.body_bytes("2", ".N12345", "\x15", "H1", "2", "M01AXX0123pos\x07report"))
    up = M.with_bcs(M.body_bytes("2", "..G-ABC", "3", "10", "A", "short"))
    bare = M.with_bcs(M.body_bytes("X", ".D-ABCD", "A", "_\x7f", "S", None, etb=True))
    odd = bytearray(down)
    odd[3] ^= 0x80  # a parity error (the CRC is not the parser's business)
    for raw in (down, up, bare, bytes(odd)):
        want = M.parse(raw)
        assert AC.parse_message(raw) == want
    got = AC.parse_message(down)
    assert (got["msgno"], got["flight"], got["text"], got["ack"], got["more"], got["parity_errors"]) == ("M01A", "XX0123", "pos�report", "�", False, 0)
    got = AC.parse_message(up)
    assert (got["registration"], got["msgno"], got["flight"], got["text"]) == ("G-ABC", None, None, "short")
    got = AC.parse_message(bare)
    assert (got["text"], got["more"], got["label"]) == (None, True, "_�") and AC.parse_message(bytes(odd))["parity_errors"] == 1
    # merging: the same bytes within L of a group's first start are one message; further away, or other bytes, another
    L = plan.L
    rows = [(0, 100, 5000, down), (3, 100, 5000 + L, down), (5, 101, 5000 + L + 1, down), (1, 300, 9000, up), (2, 300, 9010, up), (4, 99, 4990, bare)]
    rec = dict(phase=[r[0] for r in rows], s=[r[1] for r in rows], start=[r[2] for r in rows], nbytes=[len(r[3]) for r in rows],
               data=np.array([list(r[3].ljust(AC.SLOT_BYTES, b"\xAA")) for r in rows], dtype=np.uint8))
    res = AC.parse_messages(plan, rec, 9)
    assert [(m.raw, m.hits, m.time_s) for m in res.messages] == [(bare.hex(), 1, 4990 / 96_000.0), (down.hex(), 2, 5000 / 96_000.0),
                                                                 (down.hex(), 1, (5000 + L + 1) / 96_000.0), (up.hex(), 2, 9000 / 96_000.0)]
    assert (res.candidates, res.crc_ok) == (9, 6) and res.to_json()["messages"][1]["flight"] == "XX0123"
    assert res.messages[1].line() == "ACARS .N12345 H1 2 M01A XX0123 pos�report" and res.messages[0].line() == "ACARS .D-ABCD _� S"
    assert [M.line(M.parse(r)) for r in (down, up, bare)] == [AC.AcarsMessage(time_s=0.0, hits=1, **AC.parse_message(r)).line() for r in (down, up, bare)]
    assert AC.parse_messages(plan, dict(phase=[], s=[], start=[], nbytes=[], data=[]), 3) is None


# ---- the plan -----------------------------------------------------------------------------------------------------------


def test_plan_is_the_oracles():
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.decoders import acars as AC

    for fs in (19_200.0, 21_600.0, 28_800.0, 48_000.0, 96_000.0, 10e6 / 104, 957_600.0, 960_000.0):
        plan, want = P.plan_acars(fs), M.plan(fs)
        assert (plan.fs, plan.sps, plan.L, plan.W, plan.step, plan.cr, plan.sr) == (want["fs"], want["sps"], want["L"], want["W"], want["step"], want["cr"], want["sr"])
        assert plan.taps.dtype == np.int16 and plan.taps.shape == (2, plan.W) and np.abs(plan.taps).max() <= 256
        np.testing.assert_array_equal(plan.taps[0], want["c"])
        np.testing.assert_array_equal(plan.taps[1], want["s"])
        for n in (0, 1, plan.W - 1, plan.W, plan.W + plan.L, 5000, 5001):
            for p in range(8):
                at = M.instants(want, p, n)
                assert plan.bit_count(p, n) == at.size
                np.testing.assert_array_equal(plan.instant(np.arange(at.size), p), at)
        if float(plan.sps).is_integer():
            assert (plan.cr, plan.sr) == (0, -256)
    assert [(P.plan_acars(fs).L, P.plan_acars(fs).W) for fs in (19_200.0, 21_600.0, 96_000.0, 957_600.0, 960_000.0)] == [(8, 11), (9, 12), (40, 53), (399, 532), (400, 533)]
    # exact .5 ties in rint((8 i + p) step): step = 1.5 at 28 800 Hz; half-even
    tie = P.plan_acars(28_800.0)
    assert (tie.step, tie.W) == (1.5, 16)
    assert [int(tie.instant(i, p)) - 15 for i, p in ((0, 1), (1, 1), (2, 1), (0, 3), (0, 5), (1, 7))] == [2, 14, 26, 4, 8, 22]
    for fs in (19_199.0, 960_001.0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            P.plan_acars(fs)
    assert (P.ACARS_MAX_SPS, P.ACARS_PHASES) == (M.MAX_SPS, M.PHASES) and AC.PHASES == 8
    for e, sh in ((1.0, 14), (0.999, 15), (0.013, 21), (2.0 ** -149, 163), (3.0e38, -113), (16384.0, 0)):
        assert AC.shift_of(np.float32(e)) == M.shift_of(np.float32(e)) == sh and 2 ** 14 <= float(np.float32(e)) * 2.0 ** sh < 2 ** 15


# ---- the surface ----------------------------------------------------------------------------------------------------------


def test_cli_usage_errors(tmp_path, capsys):
    from iq_to_audio_amd import cli

    for mode in ("nfm", "usb", "wfm", "none"):
        with pytest.raises(SystemExit) as exc:
            cli.main(["--in", str(tmp_path / "x.wav"), "--ft", "1e6", "--acars", "--demod", mode])
        assert exc.value.code == 2 and "--acars needs --demod am" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        cli.main(["--in", str(tmp_path / "x.wav"), "--ft", "1e6", "--acars"])  # (the default --demod is nfm)
    assert exc.value.code == 2 and "--acars needs --demod am" in capsys.readouterr().err
    args = cli.build_parser().parse_args(["--in", "x.wav", "--demod", "am", "--acars"])
    assert args.acars and not cli.build_parser().parse_args(["--in", "x.wav"]).acars


def test_pipelines_take_the_flag_and_check_the_mode(tmp_path):
    import iq_to_audio_amd as A
    from iq_to_audio_amd import batch

    am = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="am")
    nfm = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="nfm")
    assert A.ProcessingPipeline(am, acars=True).acars_enabled and not A.ProcessingPipeline(am).acars_enabled
    assert all(o.acars_enabled for o in A.MultiChannelPipeline([am, am], acars=True).owners)
    for make in (lambda: A.ProcessingPipeline(nfm, acars=True), lambda: A.MultiChannelPipeline([am, nfm], acars=True)):
        with pytest.raises(ValueError, match="--demod am"):
            make()
    with pytest.raises(ValueError, match="acars"):
        batch.reject_side_decoders(acars=True)
    batch.reject_side_decoders(acars=False)
    assert len(A.ProcessingConfig.__dataclass_fields__) == 23
