"""AX.25 over Bell-202 AFSK beside narrowband FM (--demod nfm --ax25), the host side: the protocol constants pinned three
ways, the numpy oracle (tests/ax25_model.py) round trip over channel rates, space gains, clock errors and noise, no decode
from noise, the frame walker on hand-made bit streams, the address validator and the TNC2 line on fixed byte strings, the
plan, CLI and pipeline validation.  No GPU compute."""
from __future__ import annotations

import importlib.util
import itertools
import sys
from ctypes import c_double, c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest

import iq_to_audio_amd as A
from iq_to_audio_amd import dsp_plan as P
from iq_to_audio_amd.decoders import ax25 as AX


def _load_model():
    name = "ax25_model"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name("ax25_model.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load_model()

SIGMA = 0.2  # complex noise per component against a carrier of 1: the tested limit the feature request states
INFO = "!4903.50N/07201.75W-Test 001234 of the AFSK decoder, padded out to its length.."
SOURCE, DEST, PATH = "N0CALL-7", "APRS", ["WIDE1-1*", "WIDE2-1"]


def _frame(info=INFO):
    return M.ui_frame(SOURCE, DEST, PATH, info)


def _records(out: dict) -> dict:
    recs = out["records"]
    width = max([len(r[3]) for r in recs], default=0)
    data = np.zeros((len(recs), width), dtype=np.uint8)
    for k, r in enumerate(recs):
        data[k, : len(r[3])] = np.frombuffer(r[3], dtype=np.uint8)
    return dict(variant=[r[0] for r in recs], s=[r[1] for r in recs], start=[r[2] for r in recs], nbytes=[len(r[3]) for r in recs], data=data)


# ---- constants -----------------------------------------------------------------------------------------------------------


def test_constants_are_pinned_three_ways():
    """The check value of CRC-16/X.25, its residue, and a hand-built frame through stuffing, flags and the walker."""
    assert M.crc16(b"123456789") == AX.crc16_x25(b"123456789") == 0x906E
    assert (AX.CRC_POLY, AX.FLAG, AX.MIN_FRAME, AX.MAX_FRAME) == (M.CRC_POLY, M.FLAG, M.MIN_FRAME, M.MAX_FRAME) == (0x8408, 0x7E, 17, 330)
    assert (P.AFSK_GAINS, P.AFSK_PHASES, float(P.AFSK_MAX_SPS)) == (M.GAINS, M.PHASES, M.MAX_SPS)
    frame = _frame()
    assert len(frame) == 28 + 2 + len(INFO) + 2  # (four addresses, control, PID, the text, FCS)
    reg = 0xFFFF
    for byte in frame:  # the register before the final xor, run over a frame and its own FCS
        reg ^= byte
        for _ in range(8):
            reg = (reg >> 1) ^ 0x8408 if reg & 1 else reg >> 1
    assert reg == M.CRC_RESIDUE == 0xF0B8
    # by hand: destination "APRS  " command, source "N0CALL" SSID 7 last, UI, no layer 3, "hi"
    hand = bytes([0x82, 0xA0, 0xA4, 0xA6, 0x40, 0x40, 0xE0, 0x9C, 0x60, 0x86, 0x82, 0x98, 0x98, 0x6F, 0x03, 0xF0, 0x68, 0x69])
    assert M.ui_frame("N0CALL-7", "APRS", [], "hi")[:-2] == hand
    full = hand + bytes([M.crc16(hand) & 0xFF, M.crc16(hand) >> 8])
    bits = M.hdlc_bits([full], preamble=2, postamble=1)
    assert M.frames_of(bits) == ([(16, full)], 1)
    got = AX.parse_frame(full)
    assert got == dict(dest="APRS", source="N0CALL-7", path=[], control=3, pid=0xF0, info="hi")
    assert M.nrzi([1, 0, 0, 1, 0]).tolist() == [1, 0, 1, 1, 0]


# ---- the oracle ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("sigma", [0.0, SIGMA])
@pytest.mark.parametrize("ppm", [0.0, 50.0, -50.0])
@pytest.mark.parametrize("gain", [1.0, 2.0, 0.5])
@pytest.mark.parametrize("fs", [96_000.0, 96_153.846])
def test_oracle_round_trip(fs, gain, ppm, sigma):
    """The transmitted frame comes back (source, destination, path, info) through the oracle AND through the package's
    parser on the oracle's kept frames; at least one grid point decodes it; no CRC-passing frame differs from it."""
    frame = _frame()
    z = M.modulate(M.hdlc_bits([frame]), fs, space_gain=gain, offset_hz=500.0, ppm=ppm, sigma=sigma, seed=7)
    out = M.oracle(M.theta_of(z), fs)
    print(f"fs {fs} gain {gain} ppm {ppm} sigma {sigma}: {len(out['records'])} of 24 grid points, {out['closed']} closed candidates")
    assert len(out["records"]) >= 1
    assert all(r[3] == frame for r in out["records"])
    assert len(out["frames"]) == 1 and out["rejected"] == 0
    f = out["frames"][0]
    assert (f["source"], f["dest"], f["path"], f["info"]) == (SOURCE, DEST, PATH, INFO)
    assert M.tnc2(f) == f"N0CALL-7>APRS,WIDE1-1*,WIDE2-1:{INFO}"
    res = AX.parse_frames(P.plan_afsk(fs), _records(out), out["closed"])
    assert len(res.frames) == 1 and res.crc_ok == len(out["records"]) and res.candidates == out["closed"] and res.rejected == 0
    g = res.frames[0]
    assert (g.source, g.dest, g.path, g.info, g.control, g.pid, g.raw, g.hits) == (SOURCE, DEST, PATH, INFO, 3, 0xF0, frame.hex(), f["hits"])
    assert g.time_s == f["time_s"] and g.line() == M.tnc2(f)
    assert g.hits == len(out["records"])
    assert res.to_json()["frames"][0]["info"] == INFO


def test_noise_decodes_nothing():
    """Twenty seconds of carrier-less noise at 96 kHz: not one CRC-passing frame over all 24 grid points."""
    fs = 96_000.0
    out = M.oracle(M.theta_of(M.noise_only(int(20 * fs), SIGMA, 1)), fs)
    print("noise: closed candidates", out["closed"])
    assert out["records"] == [] and out["frames"] == []
    assert AX.parse_frames(P.plan_afsk(fs), _records(out), out["closed"]) is None


def test_sums_stay_in_range():
    """The largest |t| against full-scale taps stays inside int32 up to L = 512, and the slicer inside int64."""
    t_max = int(np.rint(np.float64(np.float32(np.pi)) * 4096.0))
    assert t_max == 12_868
    assert t_max * 256 * 512 < 2 ** 31
    e_max = (2 * (t_max * 256 * 512) ** 2) >> 4
    assert 4 * e_max + e_max < 2 ** 63
    pl = M.plan(480_000.0)  # L = 400: the longest window
    E = M.energies(np.full(1000, t_max, dtype=np.int32), pl)  # (asserts the int32 bound itself)
    assert max(int(e.max()) for e in E.values()) <= e_max


# ---- the walker ----------------------------------------------------------------------------------------------------------


def _with_fcs(body: bytes) -> bytes:
    fcs = M.crc16(body)
    return body + bytes([fcs & 0xFF, fcs >> 8])


def test_walker_on_hand_made_bit_streams():
    body = M.ui_frame("AB1CDE", "BEACON", [], b"\x7e\x7e\xff\xff\x7e and \x3e\x7c")[:-2]  # 0x7E and runs of ones inside the payload
    frame = _with_fcs(body)
    stuffed = M.stuffed_bits(frame)
    assert len(stuffed) > 8 * len(frame)
    assert all("".join(map(str, stuffed[i : i + 6])) != "111111" for i in range(len(stuffed)))
    bits = M.hdlc_bits([frame], preamble=3, postamble=2)
    assert M.frames_of(bits) == ([(24, frame)], 1)
    # an abort: seven ones inside the frame
    broken = M.FLAG_BITS + stuffed[:40] + [1] * 7 + stuffed[40:] + M.FLAG_BITS
    assert M.frames_of(np.array(broken, dtype=np.uint8)) == ([], 0)
    # a flag that is not on a byte boundary ends the walk as an abort
    off = M.FLAG_BITS + stuffed[:43] + M.FLAG_BITS
    assert M.walk(off, 8) is None
    # back-to-back frames sharing one flag
    other = M.ui_frame("N0CALL-7", "APRS", ["WIDE1-1*"], ">status")
    shared = M.hdlc_bits([frame, other], preamble=1, between=1, postamble=1)
    kept, closed = M.frames_of(shared)
    assert [raw for _, raw in kept] == [frame, other] and closed == 2
    assert kept[1][0] == 8 + len(stuffed) + 8
    # repeated flags open nothing: only the last flag in front of the frame does, and the last one of the stream (into nothing)
    idle = M.hdlc_bits([frame], preamble=30, postamble=5)
    assert M.openers(idle).tolist() == [240, idle.size] and M.walk(idle, idle.size) is None
    # 16 bytes: too short; 17: kept; 330: kept; 331: too long
    for size, want in ((16, 0), (17, 1), (330, 1), (331, 0)):
        f = _with_fcs(bytes(range(7, 7 + size - 2)) if size < 200 else bytes((3 * k + 1) & 0xFF for k in range(size - 2)))
        assert len(f) == size
        kept, closed = M.frames_of(M.hdlc_bits([f], preamble=2, postamble=1))
        assert (len(kept), closed) == (want, want), size
    # cut by the end of the stream: inside the frame, and inside the closing flag (the bit behind the sixth one is missing)
    assert M.frames_of(bits[: 24 + len(stuffed) - 5]) == ([], 0)
    assert M.frames_of(bits[: 24 + len(stuffed) + 7]) == ([], 0)
    assert M.frames_of(bits[: 24 + len(stuffed) + 8]) == ([(24, frame)], 1)
    # a damaged frame closes and is counted, but is not kept
    bad = bits.copy()
    bad[24 + 50] ^= 1
    kept, closed = M.frames_of(bad)
    assert kept == [] and closed <= 1


# ---- the parser ----------------------------------------------------------------------------------------------------------


def test_address_validator_and_tnc2_line():
    ok = M.ui_frame("DL1ABC-15", "APDR16", ["DB0XYZ-2*", "WIDE2-1"], "=4903.50N/07201.75W$ caf\xe9\x01!")
    got = AX.parse_frame(ok)
    model = M.parse(ok)
    assert model.pop("raw") == ok.hex() and got == model
    assert (got["source"], got["dest"], got["path"], got["control"], got["pid"]) == ("DL1ABC-15", "APDR16", ["DB0XYZ-2*", "WIDE2-1"], 3, 0xF0)
    assert got["info"] == "=4903.50N/07201.75W$ caf��!"
    fr = AX.Ax25Frame(time_s=0.5, raw=ok.hex(), hits=3, **got)
    assert fr.line() == "DL1ABC-15>APDR16,DB0XYZ-2*,WIDE2-1:=4903.50N/07201.75W$ caf��!"

    def refused(frame: bytes) -> bool:
        return AX.parse_frame(frame) is None and M.parse(frame) is None

    body = bytearray(ok[:-2])
    for at, value in ((2, body[2] | 1), (3, ord("a") << 1), (4, ord("-") << 1)):  # a low bit, a lower-case letter, punctuation
        bad = bytearray(body)
        bad[at] = value
        assert refused(_with_fcs(bytes(bad)))
    early = bytearray(body)
    early[6] |= 1  # the extension bit on the destination: one address only
    assert refused(_with_fcs(bytes(early)))
    never = bytearray(body)
    never[27] &= 0xFE  # no extension bit on the last address: the field runs into the payload
    assert refused(_with_fcs(bytes(never)))
    eleven = M.address("A", high=True) + b"".join(M.address(f"B{k}") for k in range(9)) + M.address("C", last=True) + b"\x03\xf0x"
    assert refused(_with_fcs(eleven))
    ten = M.address("A", high=True) + b"".join(M.address(f"B{k}") for k in range(8)) + M.address("C", last=True) + b"\x03\xf0x"
    assert len(AX.parse_frame(_with_fcs(ten))["path"]) == 8
    assert refused(_with_fcs(M.address("A", high=True) + M.address("B", last=True)))  # no control field
    # not a UI frame: the info is hex; a supervisory frame has no PID
    rr = AX.parse_frame(_with_fcs(M.address("A", high=True) + M.address("B", last=True) + b"\x11"))
    assert (rr["control"], rr["pid"], rr["info"]) == (0x11, None, "")
    iframe = AX.parse_frame(_with_fcs(M.address("A", high=True) + M.address("B", last=True) + b"\x00\xcfAB"))
    assert (iframe["control"], iframe["pid"], iframe["info"]) == (0, 0xCF, "4142")


def test_merge_counts_hits_and_keeps_repeats_apart():
    plan = P.plan_afsk(96_000.0)
    a, b = _frame("one"), _frame("two")
    junk = _with_fcs(bytes(range(1, 30)))  # passes the CRC, but is no address field
    rows = [(3, 40, 5000, a), (4, 40, 5010, a), (11, 40, 5000 + plan.L, a), (3, 400, 5000 + plan.L + 1, a), (5, 90, 9000, b), (0, 10, 100, junk)]
    width = max(len(r[3]) for r in rows)
    data = np.zeros((len(rows), width + 5), dtype=np.uint8)
    for k, r in enumerate(rows):
        data[k, : len(r[3])] = np.frombuffer(r[3], dtype=np.uint8)
    order = [4, 2, 0, 5, 1, 3]  # any order
    recs = dict(variant=[rows[k][0] for k in order], s=[rows[k][1] for k in order], start=[rows[k][2] for k in order],
                nbytes=[len(rows[k][3]) for k in order], data=data[order])
    res = AX.parse_frames(plan, recs, candidates=9)
    assert [(f.info, f.hits, f.time_s) for f in res.frames] == [("one", 3, 5000 / 96_000.0), ("one", 1, (5000 + plan.L + 1) / 96_000.0), ("two", 1, 9000 / 96_000.0)]
    assert (res.candidates, res.crc_ok, res.rejected) == (9, 6, 1)
    assert [(at, raw, hits) for at, raw, hits in M.merge(rows, plan.L)] == [(100, junk, 1), (5000, a, 3), (5000 + plan.L + 1, a, 1), (9000, b, 1)]
    only_junk = dict(variant=[0], s=[10], start=[100], nbytes=[len(junk)], data=data[5:6])
    assert AX.parse_frames(plan, only_junk) is None
    assert AX.parse_frames(plan, dict(variant=[], s=[], start=[], nbytes=[], data=np.zeros((0, 0), dtype=np.uint8))) is None


# ---- the host surface ----------------------------------------------------------------------------------------------------


def test_plan():
    for fs in (96_000.0, 10e6 / 104, 48_000.0, 480_000.0, 9_600.0):
        plan, want = P.plan_afsk(fs), M.plan(fs)
        assert (plan.sps, plan.L, plan.step) == (want["sps"], want["L"], want["step"])
        assert plan.taps.dtype == np.int16 and plan.taps.shape == (4, plan.L) and np.abs(plan.taps).max() <= 256
        for row, arr in zip(plan.taps, [want["taps"][1200][0], want["taps"][1200][1], want["taps"][2200][0], want["taps"][2200][1]]):
            np.testing.assert_array_equal(row, arr)
        for p in (0, 3, 7):
            for n in (0, 1, plan.L - 1, plan.L, plan.L + 1, 12_345, 1_000_003):
                assert plan.bit_count(p, n) == M.instants(want, p, n).size, (fs, p, n)
            np.testing.assert_array_equal(plan.instant(np.arange(50), p), M.instants(want, p, 10 ** 9)[:50])
    assert P.plan_afsk(96_000.0).L == 80 and P.plan_afsk(10e6 / 104).L == 80
    for fs in (9_000.0, 481_000.0, 0.0, float("nan")):
        with pytest.raises(ValueError):
            P.plan_afsk(fs)
    assert P.AFSK_MAX_SPS == 400


def test_cli_and_pipeline_validation(tmp_path, capsys):
    from iq_to_audio_amd import cli
    from iq_to_audio_amd.batch import ResidentBankRunner, ResidentCaptureRunner, demodulate_sharded

    with pytest.raises(SystemExit) as exc:
        cli.main(["--in", str(tmp_path / "x.wav"), "--ft", "1e6", "--ax25", "--demod", "am"])
    assert exc.value.code == 2 and "--ax25 needs --demod nfm" in capsys.readouterr().err
    assert cli.build_parser().parse_args(["--in", "x.wav"]).ax25 is False
    both = cli.build_parser().parse_args(["--in", "x.wav", "--ax25", "--pocsag"])
    assert both.ax25 and both.pocsag
    wfm = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="wfm")
    nfm = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="nfm")
    with pytest.raises(ValueError, match="ax25"):
        A.ProcessingPipeline(wfm, ax25=True)
    with pytest.raises(ValueError, match="ax25"):
        A.MultiChannelPipeline([nfm, wfm], ax25=True)
    assert A.ProcessingPipeline(nfm, ax25=True).ax25_enabled and not A.ProcessingPipeline(nfm).ax25_enabled
    assert all(o.ax25_enabled and o.pocsag_enabled for o in A.MultiChannelPipeline([nfm, nfm], ax25=True, pocsag=True).owners)
    assert len(A.ProcessingConfig.__dataclass_fields__) == 23
    with pytest.raises(ValueError, match="ax25"):
        ResidentBankRunner([dict(freq_offset=25e3)], sample_rate=2.5e6, n_frames=1 << 20, ax25=True)
    with pytest.raises(ValueError, match="ax25"):
        ResidentCaptureRunner(np.ones(8), sample_rate=2.5e6, freq_offset=25e3, decimation=26, fs_channel=2.5e6 / 26, chunk=1 << 20,
                              n_frames=1 << 20, ax25=True)
    with pytest.raises(ValueError, match="ax25"):
        demodulate_sharded([dict(freq_offset=25e3)], sample_rate=2.5e6, n_frames=1 << 20, axis="channels", ax25=True)


def test_c_abi_refuses_bad_arguments():
    """The library has the three entry points, and their argument checks come before any launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some = c_void_p(0), c_void_p(8)  # (never dereferenced: every call below is refused, or has nothing to do)
    for name in ("iqa_afsk_correlate", "iqa_afsk_bits", "iqa_afsk_frames"):
        assert hasattr(N.lib(), name)
    for window in (7, 401):
        with pytest.raises(ValueError, match="window"):
            N.call("iqa_afsk_correlate", some, c_int64(16), null, c_int32(window), some, some, some, null, null, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_afsk_correlate", some, c_int64(16), null, c_int32(80), null, some, some, null, null, null)
    with pytest.raises(ValueError, match="negative"):
        N.call("iqa_afsk_correlate", some, c_int64(-1), null, c_int32(80), some, some, some, null, null, null)
    N.call("iqa_afsk_correlate", null, c_int64(0), null, c_int32(80), null, null, null, null, null, null)  # nothing to do
    with pytest.raises(ValueError, match="step"):
        N.call("iqa_afsk_bits", some, c_int64(16), c_int32(80), c_double(0.5), c_int64(4), some, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_afsk_bits", null, c_int64(16), c_int32(80), c_double(10.0), c_int64(4), some, null)
    N.call("iqa_afsk_bits", null, c_int64(16), c_int32(80), c_double(10.0), c_int64(0), null, null)
    counts = (c_int64 * 8)(*[4] * 8)
    with pytest.raises(ValueError, match="count_of"):
        N.call("iqa_afsk_frames", some, c_int64(3), counts, c_int32(80), c_double(10.0), some, some, c_int64(1), some, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_afsk_frames", some, c_int64(4), counts, c_int32(80), c_double(10.0), some, some, c_int64(1), null, null)
    with pytest.raises(ValueError, match="window"):
        N.call("iqa_afsk_frames", some, c_int64(4), counts, c_int32(0), c_double(10.0), some, some, c_int64(1), some, null)
