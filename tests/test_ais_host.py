"""AIS beside narrowband FM (--demod nfm --ais), the host side: the protocol constants pinned three ways, the numpy oracle
(tests/ais_model.py) over channel rates, training alignments, clock errors, tuning errors and noise, no decode from noise or
from a voice carrier, the frame walker on hand-made symbol planes, the bit fields and sentences on fixed bit strings, the
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
from iq_to_audio_amd.decoders import ais as AI


def _load_model():
    name = "ais_model"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name("ais_model.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load_model()

REFERENCE = M.frame_bytes(M.dearmour(M.REFERENCE_PAYLOAD))
RATES = (96_000.0, 10e6 / 104, 48_000.0)


def _records(recs: list) -> dict:
    width = max([len(r[3]) for r in recs], default=0)
    data = np.zeros((len(recs), width), dtype=np.uint8)
    for k, r in enumerate(recs):
        data[k, : len(r[3])] = np.frombuffer(r[3], dtype=np.uint8)
    return dict(phase=[r[0] for r in recs], s=[r[1] for r in recs], start=[r[2] for r in recs], nbytes=[len(r[3]) for r in recs], data=data)


def _one(raw: bytes, frequency=None):
    """The package's message of one frame, as its JSON form."""
    res = AI.parse_frames(P.plan_ais(96_000.0), _records([(0, 40, 9600, raw)]), 1, frequency=frequency)
    assert len(res.messages) == 1
    return res.messages[0].to_json()


# ---- constants -----------------------------------------------------------------------------------------------------------


def test_constants_are_pinned_three_ways():
    M.self_check()
    assert (AI.MIN_FRAME, AI.MAX_FRAME, AI.SLOT_BYTES, AI.PHASES) == (M.MIN_FRAME, M.MAX_FRAME, 128, M.PHASES) == (11, 128, 128, 8)
    assert (P.AIS_BAUD, P.AIS_BT, float(P.AIS_MAX_SPS), P.AIS_MIN_SPS, P.AIS_T_MAX) == (M.BAUD, M.BT, M.MAX_SPS, M.MIN_SPS, M.T_PI)
    assert int(np.rint(np.float64(np.float32(np.pi)) * 4096.0)) == M.T_PI
    # the package on the same three pins
    got = _one(REFERENCE, frequency=162_025_000.0)
    assert (got["type"], got["repeat"], got["mmsi"], got["status"], got["speed"], got["course"], got["heading"], got["second"]) == (
        1, 0, 477553000, 5, 0.0, 51.0, 181, 15)
    assert abs(got["lat"] - 47.58283333) < 1e-8 and abs(got["lon"] + 122.34583333) < 1e-8
    assert got["nmea"] == [M.REFERENCE_SENTENCE] and got["channel"] == "B" and got["raw"] == REFERENCE.hex()


# ---- the oracle alone ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("fs", RATES)
def test_oracle_decodes_the_grid(fs):
    """Two training alignments x three clock offsets x three carrier offsets (the last with an inverted spectrum) x three
    noise levels: the transmitted frame passes at >= 3 phases in every case, and no CRC-passing frame differs from it."""
    worst = 8
    for first, ppm, (off, inv), sigma in itertools.product((0, 1), (0.0, 50.0, -50.0), ((0.0, False), (500.0, False), (-1500.0, True)),
                                                           (0.0, 0.1, 0.2)):
        z = M.modulate(M.burst_bits(REFERENCE, first=first), fs, offset_hz=off, ppm=ppm, invert=inv, sigma=sigma, seed=int(sigma * 10) + 7)
        out = M.oracle(M.theta_of(z), fs, frequency=161_975_000.0)
        assert all(r[3] == REFERENCE for r in out["records"]), (fs, first, ppm, off, sigma)
        assert len(out["records"]) >= 3, (fs, first, ppm, off, sigma, len(out["records"]))
        worst = min(worst, len(out["records"]))
        assert len(out["messages"]) == 1 and out["messages"][0]["hits"] == len(out["records"])
        assert out["messages"][0]["nmea"] == [M.REFERENCE_SENTENCE.replace(",B,", ",A,")[:-2] + M.checksum(M.REFERENCE_SENTENCE[1:-3].replace(",B,", ",A,"))]
    print(f"fs {fs}: fewest phases passing {worst}")


def test_type_5_gives_two_sentences():
    bits = M.static_data(235_087_654, imo=9_321_483, callsign="2ABC5", name="EVER GIVEN TWO", ship_type=70, dims=(200, 100, 20, 12),
                         eta=(10, 17, 6, 30), draught=123, destination="ROTTERDAM")
    assert len(bits) == 424
    raw = M.frame_bytes(bits)
    z = M.modulate(M.burst_bits(raw), 96_000.0, sigma=0.1, seed=2)
    out = M.oracle(M.theta_of(z), 96_000.0, frequency=162_025_000.0)
    assert len(out["messages"]) == 1
    msg = out["messages"][0]
    assert (msg["type"], msg["mmsi"], msg["imo"], msg["callsign"], msg["name"], msg["destination"], msg["draught"]) == (
        5, 235_087_654, 9_321_483, "2ABC5", "EVER GIVEN TWO", "ROTTERDAM", 12.3)
    assert len(msg["nmea"]) == 2 and msg["nmea"][0].startswith("!AIVDM,2,1,0,B,") and msg["nmea"][1].startswith("!AIVDM,2,2,0,B,")
    first, second = (s.split(",") for s in msg["nmea"])
    assert len(first[5]) == 60 and len(second[5]) == 11 and first[6][0] == "0" and second[6][0] == "2"
    assert M.dearmour(first[5] + second[5], 2) == bits
    assert _one(raw, frequency=162_025_000.0) == dict(msg, time_s=0.1, hits=1)


@pytest.mark.parametrize("kind,seed", [("noise", 1), ("voice", 2)])
def test_nothing_from_noise_or_voice(kind, seed):
    """Ten seconds without a carrier and ten seconds of a voice-modulated carrier: no message (a 16-bit check passes one
    closed candidate in 65 536; the seeds are ones for which the oracle gives none)."""
    fs = 96_000.0
    n = int(10 * fs)
    z = M.noise_only(n, 0.2, seed) if kind == "noise" else M.voice_carrier(n, fs, 0.05, seed)
    out = M.oracle(M.theta_of(z), fs)
    print(kind, "closed candidates", out["closed"])
    assert out["records"] == [] and out["messages"] == []
    assert AI.parse_frames(P.plan_ais(fs), _records([]), out["closed"]) is None


# ---- the walker ----------------------------------------------------------------------------------------------------------


def test_walker_on_hand_made_planes():
    names = []
    for name, v, count, kept in M.hand_made_planes():
        got, closed = M.frames_of(v[:count])
        assert len(got) == kept and closed >= kept, name
        for s, raw in got:
            assert s == M.TRAINING + 8 and M.opens(v[:count], s) and M.MIN_FRAME <= len(raw) <= M.MAX_FRAME, name
        names.append(name)
        assert sorted(M.openers(v[:count]).tolist()) == [s for s in range(24, count + 1) if M.opens(v[:count], s)], name
    assert {"flag in the payload", "10 bytes", "11 bytes", "128 bytes", "129 bytes", "abort", "flag off the byte boundary", "cut inside the frame",
            "cut inside the closing flag", "level tie", "damaged"} <= set(names)
    planes = {name: (v, count) for name, v, count, _ in M.hand_made_planes()}
    v, count = planes["flag in the payload"]
    assert M.frames_of(v)[0][0][1][:5] == bytes([0x7E, 0x7E, 0xFF, 0xFF, 0x7E])
    assert M.frames_of(planes["damaged"][0]) == ([], 1)
    tie, _ = planes["level tie"]
    s = M.TRAINING + 8
    assert M.level_sum(tie, s) == 32 and (16 * tie.astype(np.int64) == 32).sum() == 1
    assert M.frames_of(tie)[0] == M.frames_of(np.where(tie == 2, 1, tie))[0]  # the tie is read as the low level
    assert M.frames_of(np.where(tie == 2, 3, tie))[0] == []  # and not as the high one


# ---- fields --------------------------------------------------------------------------------------------------------------


def _same(bits, **want):
    raw = M.frame_bytes(bits)
    got, ref = _one(raw), M.decode_fields(M.message_bits(raw))
    for key in ("time_s", "raw", "nmea", "channel", "hits"):
        got.pop(key)
    assert got == ref, (got, ref)
    for key, value in want.items():
        assert got[key] == value, (key, got[key], value)
    return got


def test_fields_of_every_decoded_type():
    for mtype in (1, 2, 3):
        _same(M.position_report(mtype, 366_123_456, status=3, turn=-127, speed=1022, accuracy=1, lon=-179.999999, lat=-89.5, course=3599,
                                heading=359, second=59, repeat=3),
              type=mtype, repeat=3, mmsi=366_123_456, status=3, turn=-127, speed=102.2, accuracy=1, lon=-107_999_999 / 600_000, lat=-89.5,
              course=359.9, heading=359, second=59)
    _same(M.position_report(1, 1), lon=None, lat=None, course=None, heading=None, speed=0.0, turn=0)
    _same(M.position_report(1, 1, turn=-128, speed=1023), turn=None, speed=None)
    _same(M.base_station(2_275_200, (2026, 10, 17, 23, 59, 58), lon=2.5, lat=-48.25), type=4, year=2026, month=10, day=17, hour=23, minute=59,
          second=58, accuracy=1, lon=2.5, lat=-48.25)
    _same(M.base_station(2_275_200), lon=None, lat=None)
    _same(M.static_data(1_073_741_823, imo=1_073_741_823, callsign="ABCDEFG", name="A NAME OF TWENTY CHR", ship_type=255, dims=(511, 1, 63, 2),
                        eta=(12, 31, 23, 59), draught=255, destination="@@"),
          type=5, mmsi=1_073_741_823, imo=1_073_741_823, callsign="ABCDEFG", name="A NAME OF TWENTY CHR", ship_type=255, to_bow=511, to_stern=1,
          to_port=63, to_starboard=2, eta_month=12, eta_day=31, eta_hour=23, eta_minute=59, draught=25.5, destination="")
    _same(M.static_data(7, name="TRAILING  ", destination="X @"), name="TRAILING", destination="X")
    _same(M.class_b_report(338_000_001, speed=61, accuracy=1, lon=-0.000005, lat=0.000005, course=1, heading=0, second=0),
          type=18, speed=6.1, accuracy=1, lon=-3 / 600_000, lat=3 / 600_000, course=0.1, heading=0, second=0)
    _same(M.class_b_report(338_000_001), lon=None, lat=None, course=None, heading=None)
    _same(M.aid_to_navigation(993_672_001, aid_type=14, name="N CARDINAL 7", accuracy=1, lon=-70.25, lat=43.5), type=21, aid_type=14,
          name="N CARDINAL 7", lon=-70.25, lat=43.5)
    _same(M.aid_to_navigation(993_672_001), name="", lon=None, lat=None)
    _same(M.static_part_a(338_000_001, "LITTLE BOAT"), type=24, part="A", name="LITTLE BOAT")
    _same(M.static_part_b(338_000_001, ship_type=37, vendor="GRMN123", callsign="WDA1234", dims=(5, 6, 2, 1)), type=24, part="B", ship_type=37,
          vendor="GRMN123", callsign="WDA1234", to_bow=5, to_stern=6, to_port=2, to_starboard=1)
    other = _same(M.field(8, 6) + M.field(1, 2) + M.field(123_456_789, 30) + M.field(0xABCDEF, 24) + M.field(0, 18))
    assert other == dict(type=8, repeat=1, mmsi=123_456_789)
    short = _same(M.field(5, 6) + M.field(0, 2) + M.field(42, 30) + M.field(0, 50))  # a type 5 cut to 11 bytes: no fields
    assert short == dict(type=5, repeat=0, mmsi=42)


def test_sentences_channels_and_merging():
    plan = P.plan_ais(96_000.0)
    assert [AI.channel_of(f) for f in (161_975_000.0, 161_970_000.0, 161_969_999.0, 162_025_000.0, 162_030_000.0, 162_030_001.0, 156.8e6, None)] == [
        "A", "A", "", "B", "B", "", "", ""]
    assert [M.channel_of(f) for f in (161_970_000.0, 161_969_999.0, 162_030_000.0, 162_030_001.0, None)] == ["A", "", "B", "", ""]
    a = REFERENCE
    long_one = M.frame_bytes(M.static_data(11, name="ONE"))
    rows = [(3, 40, 5000, a), (4, 40, 5004, a), (7, 40, 5000 + plan.L, a), (3, 400, 5000 + plan.L + 1, a)]
    rows += [(p, 90 + 500 * k, 9000 + 50_000 * k, long_one) for k in range(12) for p in (1, 2)]
    order = np.random.default_rng(0).permutation(len(rows)).tolist()
    res = AI.parse_frames(plan, _records([rows[k] for k in order]), candidates=99, frequency=161_975_000.0)
    want = M.messages_of(rows, M.plan(96_000.0), 161_975_000.0)
    assert [m.to_json() for m in res.messages] == want
    assert (res.candidates, res.crc_ok, len(res.messages)) == (99, len(rows), 14)
    assert [(m.hits, m.time_s) for m in res.messages[:2]] == [(3, 5000 / 96_000.0), (1, (5000 + plan.L + 1) / 96_000.0)]
    ids = [m.nmea[0].split(",")[3] for m in res.messages[2:]]
    assert ids == ["0", "1", "2", "3", "4", "5", "6", "7", "8", "9", "0", "1"] and res.messages[0].nmea[0].split(",")[3] == ""
    for m in res.messages:
        for s in m.nmea:
            assert s[-2:] == M.checksum(s[1:-3]) and len(s.split(",")[5]) <= 60
    line = res.messages[0].line()
    assert line.startswith("AIS 1 mmsi=477553000 47.58283N 122.34583W 0.0kn 51.0°")
    assert res.to_json()["messages"][0]["nmea"] == [M.REFERENCE_SENTENCE.replace(",B,", ",A,")[:-2] + res.messages[0].nmea[0][-2:]]


# ---- the host surface ----------------------------------------------------------------------------------------------------


def test_plan():
    for fs in (48_000.0, 96_000.0, 10e6 / 104, 960_000.0):
        plan, want = P.plan_ais(fs), M.plan(fs)
        assert (plan.sps, plan.L, plan.W, plan.step) == (want["sps"], want["L"], want["W"], want["step"])
        assert plan.taps.dtype == np.int16 and plan.taps.shape == (plan.W,) and plan.taps.max() == 256 and plan.taps.min() >= 0
        np.testing.assert_array_equal(plan.taps, want["taps"])
        np.testing.assert_array_equal(plan.taps, plan.taps[::-1])
        assert M.T_PI * int(plan.taps.astype(np.int64).sum()) < 2 ** 31
        for p in (0, 3, 7):
            for n in (0, 1, plan.W - 1, plan.W, plan.W + 1, 12_345, 1_000_003):
                assert plan.symbol_count(p, n) == M.instants(want, p, n).size, (fs, p, n)
            np.testing.assert_array_equal(plan.instant(np.arange(50), p), M.instants(want, p, 10 ** 9)[:50])
    assert (P.plan_ais(96_000.0).L, P.plan_ais(10e6 / 104).L, P.plan_ais(48_000.0).W, P.plan_ais(960_000.0).W) == (10, 10, 14, 299)
    for fs in (47_999.0, 960_001.0, 0.0, float("nan")):
        with pytest.raises(ValueError):
            P.plan_ais(fs)
        if fs > 0:
            with pytest.raises(ValueError):
                M.plan(fs)
    assert P.AIS_MAX_SPS == 100


def test_cli_and_pipeline_validation(tmp_path, capsys):
    from iq_to_audio_amd import cli
    from iq_to_audio_amd.batch import ResidentBankRunner, ResidentCaptureRunner, demodulate_sharded

    with pytest.raises(SystemExit) as exc:
        cli.main(["--in", str(tmp_path / "x.wav"), "--ft", "1e6", "--ais", "--demod", "am"])
    assert exc.value.code == 2 and "--ais needs --demod nfm" in capsys.readouterr().err
    parse = lambda *argv: cli.resolve_mode_defaults(cli.build_parser().parse_args(["--in", "x.wav", *argv]))  # noqa: E731
    assert parse().ais is False and parse().bandwidth == 12_500.0 and parse("--ais").bandwidth == 25_000.0
    assert parse("--ais", "--bw", "12500").bandwidth == 12_500.0 and parse("--ais", "--bw", "30000").bandwidth == 30_000.0
    assert parse("--pocsag", "--ax25", "--tones").bandwidth == 12_500.0 and parse("--demod", "wfm").bandwidth == 250_000.0
    assert (parse("--ais").fs_ch, parse("--ais").deemph_us) == (parse().fs_ch, parse().deemph_us)
    four = parse("--ais", "--ax25", "--pocsag", "--tones")
    assert four.ais and four.ax25 and four.pocsag and four.tones
    wfm = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="wfm")
    am = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="am")
    nfm = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="nfm")
    for bad in (wfm, am):
        with pytest.raises(ValueError, match="--demod nfm"):
            A.ProcessingPipeline(bad, ais=True)
        with pytest.raises(ValueError, match="--demod nfm"):
            A.MultiChannelPipeline([nfm, bad], ais=True)
    assert A.ProcessingPipeline(nfm, ais=True).ais_enabled and not A.ProcessingPipeline(nfm).ais_enabled
    assert all(o.ais_enabled and o.pocsag_enabled and o.ax25_enabled and o.tones_enabled
               for o in A.MultiChannelPipeline([nfm, nfm], ais=True, pocsag=True, ax25=True, tones=True).owners)
    assert len(A.ProcessingConfig.__dataclass_fields__) == 23
    with pytest.raises(ValueError, match="ais"):
        ResidentBankRunner([dict(freq_offset=25e3)], sample_rate=2.5e6, n_frames=1 << 20, ais=True)
    with pytest.raises(ValueError, match="ais"):
        ResidentCaptureRunner(np.ones(8), sample_rate=2.5e6, freq_offset=25e3, decimation=26, fs_channel=2.5e6 / 26, chunk=1 << 20,
                              n_frames=1 << 20, ais=True)
    with pytest.raises(ValueError, match="ais"):
        demodulate_sharded([dict(freq_offset=25e3)], sample_rate=2.5e6, n_frames=1 << 20, axis="channels", ais=True)


def test_c_abi_refuses_bad_arguments():
    """The library has the three entry points, and their argument checks come before any launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some = c_void_p(0), c_void_p(8)  # (never dereferenced: every call below is refused, or has nothing to do)
    for name in ("iqa_ais_filter", "iqa_ais_symbols", "iqa_ais_frames"):
        assert hasattr(N.lib(), name)
    assert N.lib().iqa_abi_version() == 1
    for window in (0, 300):
        with pytest.raises(ValueError, match="window"):
            N.call("iqa_ais_filter", some, c_int64(16), null, c_int32(window), some, some, some, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_ais_filter", some, c_int64(16), null, c_int32(29), null, some, some, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_ais_filter", some, c_int64(16), null, c_int32(29), some, some, null, null)
    with pytest.raises(ValueError, match="negative"):
        N.call("iqa_ais_filter", some, c_int64(-1), null, c_int32(29), some, some, some, null)
    N.call("iqa_ais_filter", null, c_int64(0), null, c_int32(29), null, null, null, null)  # nothing to do
    for step in (0.5, 12.6):
        with pytest.raises(ValueError, match="step"):
            N.call("iqa_ais_symbols", some, c_int64(16), c_int32(29), c_double(step), c_int64(4), some, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_ais_symbols", null, c_int64(16), c_int32(29), c_double(1.25), c_int64(4), some, null)
    N.call("iqa_ais_symbols", null, c_int64(16), c_int32(29), c_double(1.25), c_int64(0), null, null)
    counts = (c_int64 * 8)(*[4] * 8)
    with pytest.raises(ValueError, match="count_of"):
        N.call("iqa_ais_frames", some, c_int64(3), counts, c_int32(29), c_double(1.25), some, some, c_int64(1), some, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_ais_frames", some, c_int64(4), counts, c_int32(29), c_double(1.25), some, some, c_int64(1), null, null)
    with pytest.raises(ValueError, match="window"):
        N.call("iqa_ais_frames", some, c_int64(4), counts, c_int32(0), c_double(1.25), some, some, c_int64(1), some, null)
