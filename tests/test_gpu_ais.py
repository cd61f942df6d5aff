"""AIS beside narrowband FM (--demod nfm --ais) on the MI355X: every integer stage identical to the numpy oracle of
tests/ais_model.py, the pulse filter at its edge shapes against np.convolve, block invariance bit for bit, the device walker
on hand-made symbol planes, the bounded frame list, the CLI end to end on a capture with an AIS channel, a pager channel and
a voice carrier, and the proof that a run without --ais calls no AIS entry point."""
from __future__ import annotations

import importlib.util
import json
import math
import sys
from ctypes import c_double, c_int32, c_int64
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


M = _load("ais_model")
PM = _load("pocsag_model")

SIGMA = 0.1
POSITION = M.frame_bytes(M.dearmour(M.REFERENCE_PAYLOAD))
STATIC = M.frame_bytes(M.static_data(235_087_654, imo=9_321_483, callsign="2ABC5", name="EVER GIVEN TWO", ship_type=70, dims=(200, 100, 20, 12),
                                     eta=(10, 17, 6, 30), draught=123, destination="ROTTERDAM"))
CLASS_B = M.frame_bytes(M.class_b_report(338_000_001, speed=61, accuracy=1, lon=-70.25, lat=43.5, course=1805, heading=180, second=7))
PAGES = [(1234567, 3, "Pump 4 low")]  # 1664 bits: 0.7 s at 2400 baud
CHANNEL_B = 162_025_000.0


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _stream(fs: float, seed: int) -> np.ndarray:
    """About 60 k samples, three bursts behind one another at SIGMA: plain; 1500 Hz low with an inverted spectrum, 50 ppm
    fast; 500 Hz high, 50 ppm slow, the other training alignment."""
    parts = [M.modulate(M.burst_bits(POSITION), fs, sigma=SIGMA, seed=seed, lead=8000, tail=8000),
             M.modulate(M.burst_bits(STATIC), fs, offset_hz=-1500.0, invert=True, ppm=50.0, sigma=SIGMA, seed=seed + 1, lead=8000, tail=8000),
             M.modulate(M.burst_bits(CLASS_B, first=1), fs, offset_hz=500.0, ppm=-50.0, sigma=SIGMA, seed=seed + 2, lead=8000, tail=8000)]
    return np.concatenate(parts)


@pytest.fixture(scope="module")
def streams():
    return {fs: _stream(fs, seed=21) for fs in (96_000.0, 10e6 / 104)}


def _same_stages(st: dict, want: dict) -> None:
    assert st["S"].dtype == np.int32
    np.testing.assert_array_equal(st["S"], want["S"])
    assert len(st["v"]) == len(want["v"]) == 8
    for p in range(8):
        assert st["v"][p].dtype == np.int32
        np.testing.assert_array_equal(st["v"][p], want["v"][p], err_msg=f"v of phase {p}")
    assert st["records"] == want["records"]
    assert st["candidates"] == want["closed"]


@pytest.mark.parametrize("fs", [96_000.0, 10e6 / 104])
def test_stages_are_the_oracles(A, streams, fs):
    """t is the oracle's quantiser of the GPU's own theta, exactly; against numpy's float32 theta it differs by at most 1
    (the share is printed); from the GPU's t, the filter output, all 8 symbol planes, the sorted kept-frame list, both
    counters and the parsed messages are the oracle's.  Integers: no tolerance."""
    from iq_to_audio_amd.decoders.ais import AisDecoder

    z = streams[fs]
    assert 55_000 < z.size < 65_000
    dec = AisDecoder(fs, frequency=CHANNEL_B)
    dec.process(z)
    st = dec.stages()
    assert st["t"].dtype == np.int32 and st["t"].size == z.size
    np.testing.assert_array_equal(st["t"], M.quantise(st["theta"]))
    dt = np.abs(st["t"].astype(np.int64) - M.quantise(M.theta_of(z)).astype(np.int64))
    print(f"fs {fs}: t against numpy's theta: {np.mean(dt != 0):.4%} of {dt.size} samples differ, max |dt| {dt.max()}")
    assert dt.max() <= 1
    want = M.oracle(fs=fs, t=st["t"], frequency=CHANNEL_B)
    _same_stages(st, want)
    res = dec.finish()
    assert [m.to_json() for m in res.messages] == want["messages"]
    assert (res.candidates, res.crc_ok) == (want["closed"], len(want["records"]))
    assert [m.raw for m in res.messages] == [POSITION.hex(), STATIC.hex(), CLASS_B.hex()]
    assert [(m.type, m.mmsi, m.channel, len(m.nmea)) for m in res.messages] == [(1, 477553000, "B", 1), (5, 235_087_654, "B", 2), (18, 338_000_001, "B", 1)]
    assert res.messages[0].nmea == [M.REFERENCE_SENTENCE]
    print("hits", [m.hits for m in res.messages], "candidates", res.candidates, "crc_ok", res.crc_ok)
    assert all(m.hits >= 3 for m in res.messages) and res.crc_ok == sum(m.hits for m in res.messages)


def _crafted_theta(n: int, L: int, seed: int) -> np.ndarray:
    """float32[n] over [-pi, pi]: random values, a stretch of full-scale +-pi (3 L of +pi, then a square wave of period 2 L),
    and half-even ties of 4096 theta ((k + 1/2) / 4096 is exact in float32)."""
    rng = np.random.default_rng(seed)
    pi32 = np.float32(np.pi)
    th = np.clip(rng.uniform(-np.pi, np.pi, n).astype(np.float32), -pi32, pi32)
    run = np.concatenate([np.full(3 * L, pi32), np.where((np.arange(6 * L) // L) % 2 == 0, pi32, -pi32), np.full(3 * L, -pi32)]).astype(np.float32)
    at = min(40, n)
    th[at : at + run.size] = run[: max(0, n - at)]
    ties = ((np.arange(-6, 6, dtype=np.float64) + 0.5) / 4096.0).astype(np.float32)
    th[: min(n, ties.size)] = ties[: min(n, ties.size)]
    if n > 2050:
        th[2040:2052] = ties
    return th


@pytest.mark.parametrize("L", [5, 6, 7, 8, 9, 10, 99, 100])
def test_filter_at_its_edge_shapes(A, L):
    """``iqa_ais_filter`` directly: W - 1 = 13, 16, 19, 22, 25, 28, 295, 298 covers every remainder modulo 8; n around the
    2048-sample tile and equal to the history; with and without a history (shorter than, as long as and longer than the
    block); with and without the t output.  S equals np.convolve in int64, t the quantiser; nothing is written behind n."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    W = 3 * L - 1
    pl = dict(W=W, taps=M.taps_for(L, float(L)))
    taps = D.from_numpy(pl["taps"].astype(np.int16))
    assert {(3 * k - 2) % 8 for k in (5, 6, 7, 8, 9, 10, 99, 100)} == set(range(8))
    for k, n in enumerate((1, W - 1, 2047, 2048, 2049, 2 * 2048 + 1)):
        theta = _crafted_theta(n, L, seed=100 * L + k)
        want_t = M.quantise(theta)
        if n >= 12:
            assert list(want_t[:12]) == [-6, -4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6]  # half-even
        assert np.abs(want_t).max() <= M.T_PI and (n < 40 + 3 * L or np.abs(want_t).max() == M.T_PI)
        for with_hist in (False, True):
            hist = None
            if with_hist:
                hist = np.random.default_rng(L + n).integers(-M.T_PI, M.T_PI + 1, size=W - 1).astype(np.int32)
                hist[0], hist[-1] = M.T_PI, -M.T_PI
            want_s = M.pulse_filter(want_t, pl, hist)
            for with_t in (True, False):
                th_dev = D.from_numpy(theta)
                h_dev = None if hist is None else D.from_numpy(hist)
                t_dev = D.from_numpy(np.full(n + 16, -7, dtype=np.int32)) if with_t else None
                s_dev = D.from_numpy(np.full(n + 16, -7, dtype=np.int32))
                N.call("iqa_ais_filter", N.ptr(th_dev), c_int64(n), N.ptr(h_dev), c_int32(W), N.ptr(taps), N.ptr(t_dev), N.ptr(s_dev), N.stream_ptr())
                got = s_dev.cpu().numpy()
                np.testing.assert_array_equal(got[:n], want_s, err_msg=f"S: L {L} n {n} hist {with_hist} t {with_t}")
                assert (got[n:] == -7).all()
                if with_t:
                    got_t = t_dev.cpu().numpy()
                    np.testing.assert_array_equal(got_t[:n], want_t, err_msg=f"t: L {L} n {n}")
                    assert (got_t[n:] == -7).all()


@pytest.mark.parametrize("fs", [96_000.0, 10e6 / 104])
def test_block_invariance(A, streams, fs):
    """One stream as a single block and in uneven cuts (shorter than the carried history, a single sample, exactly 2048):
    bit-identical theta, t, S, symbol planes and kept frames."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.decoders.ais import AisDecoder

    z = D.to_device(streams[fs], "complex64")
    n = int(z.numel())
    runs = []
    for cuts in ([0, n], [0, 10_003, 10_004, 10_020, 12_068, 30_001, n], [0, 7, 2047, 2049, 4097, 4097 + 2048, 4097 + 2048 + 17, n - 9_000, n - 1, n]):
        dec = AisDecoder(fs)
        sizes = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
        assert len(cuts) == 2 or (min(sizes) < dec.core.hist_len and 1 in sizes and 2048 in sizes)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            dec.process(z[lo:hi])
        assert dec.core.pos == n
        runs.append(dec.stages())
    assert len(runs[0]["records"]) >= 9
    for st in runs[1:]:
        for key in ("theta", "t", "S"):
            np.testing.assert_array_equal(st[key], runs[0][key], err_msg=key)
        for p in range(8):
            np.testing.assert_array_equal(st["v"][p], runs[0]["v"][p], err_msg=f"v of phase {p}")
        assert st["records"] == runs[0]["records"] and st["candidates"] == runs[0]["candidates"]


def test_symbols_at_another_rate(A):
    """``iqa_ais_symbols`` on a random plane at sps 5 (step 0.625) and sps 99.4: the planes are the oracle's, with zeros where
    an instant lies beyond the stream."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    for fs, n in ((48_000.0, 3_001), (954_240.0, 70_003)):
        pl = M.plan(fs)
        S = np.random.default_rng(int(fs)).integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32)
        planes = M.symbol_planes(S, pl)
        nsym = max(v.size for v, _ in planes) + 3
        out = D.from_numpy(np.full(8 * nsym + 8, -7, dtype=np.int32))
        N.call("iqa_ais_symbols", N.ptr(D.from_numpy(S)), c_int64(n), c_int32(pl["W"]), c_double(pl["step"]), c_int64(nsym), N.ptr(out), N.stream_ptr())
        got = out.cpu().numpy()
        assert (got[8 * nsym :] == -7).all()
        for p, (v, _) in enumerate(planes):
            row = got[p * nsym : (p + 1) * nsym]
            np.testing.assert_array_equal(row[: v.size], v.astype(np.int32), err_msg=f"fs {fs} phase {p}")
            assert (row[v.size :] == 0).all()


def test_walker_on_hand_made_planes(A):
    """The host module's symbol planes through ``iqa_ais_symbols`` (every symbol held for one bit of ten samples, so that all
    8 phases read it) and ``iqa_ais_frames``: kept frames, positions, start instants, bytes and both counters are the
    oracle walker's, at the exact 10 / 11 and 128 / 129 byte limits, for an abort, a flag off the byte boundary, a level
    tie, and streams that end inside a frame, inside the closing flag and right behind it."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.decoders import ais as AI

    plan = P.plan_ais(96_000.0)
    assert plan.sps == 10.0 and sorted({int(plan.instant(0, p)) - plan.W + 1 for p in range(8)})[-1] < 10
    capacity = 16
    for name, v, count, expect in M.hand_made_planes():
        kept, closed = M.frames_of(v[:count])
        assert len(kept) == expect, name  # the oracle first, so that the equality below is not one of empty lists
        S = np.concatenate([np.full(plan.W - 1, 123_456, dtype=np.int32), np.repeat(v, 10)])
        n = plan.W - 1 + 10 * count  # exactly ``count`` symbols of every phase exist
        counts_of = [plan.symbol_count(p, n) for p in range(8)]
        assert counts_of == [count] * 8, name
        nsym = int(v.size)
        plane = D.empty(8 * nsym, "int32")
        N.call("iqa_ais_symbols", N.ptr(D.from_numpy(S)), c_int64(n), c_int32(plan.W), c_double(plan.step), c_int64(nsym), N.ptr(plane), N.stream_ptr())
        got_v = plane.cpu().numpy().reshape(8, nsym)
        for p in range(8):
            np.testing.assert_array_equal(got_v[p, :count], v[:count], err_msg=name)
        plane = D.from_numpy(np.ascontiguousarray(np.tile(v, (8, 1))))  # (what lies behind ``count`` must not be read)
        lst = D.from_numpy(np.full(4 * capacity, -7, dtype=np.int64))
        slots = D.from_numpy(np.full(capacity * AI.SLOT_BYTES, 0xAA, dtype=np.uint8))
        counts = D.from_numpy(np.array([99, 99], dtype=np.int64))
        N.call("iqa_ais_frames", N.ptr(plane), c_int64(nsym), (c_int64 * 8)(*counts_of), c_int32(plan.W), c_double(plan.step), N.ptr(lst),
               N.ptr(slots), c_int64(capacity), N.ptr(counts), N.stream_ptr())
        assert [int(x) for x in counts.cpu().numpy()] == [8 * len(kept), 8 * closed], name
        k = 8 * len(kept)
        entries, data = lst.cpu().numpy().reshape(-1, 4), slots.cpu().numpy().reshape(capacity, -1)
        assert (entries[k:] == -7).all() and (data[k:] == 0xAA).all(), name
        got = sorted((int(p), int(s), int(at), data[i, : int(nb)].tobytes(), bool((data[i, int(nb) :] == 0).all()))
                     for i, (p, s, at, nb) in enumerate(entries[:k]))
        want = sorted((p, s, int(plan.instant(s, p)), raw, True) for p in range(8) for s, raw in kept)
        assert got == want, name


def test_frame_list_overflow_is_repeated_not_truncated(A, streams):
    """A list of capacity 1 reports the full count and writes nothing past its one entry; ``finish`` then repeats the call
    with room for all and gives the same messages as a run whose list was long enough from the start."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N
    from iq_to_audio_amd.decoders import ais as AI

    fs = 96_000.0
    z = streams[fs]
    roomy, tight = AI.AisDecoder(fs), AI.AisDecoder(fs)
    roomy.process(z)
    tight.process(z)
    a, b = roomy.core.finish(), tight.core.finish(capacity=1)
    assert len(a["start"]) > 1
    for key in ("phase", "s", "start", "nbytes", "data"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["candidates"] == b["candidates"]
    assert [m.to_json() for m in AI.parse_frames(tight.plan, b, b["candidates"]).messages] == [m.to_json() for m in roomy.finish().messages]
    # the call itself
    lst = D.from_numpy(np.full(8, -7, dtype=np.int64))
    slots = D.from_numpy(np.full(2 * AI.SLOT_BYTES, 0xAA, dtype=np.uint8))
    counts = D.from_numpy(np.array([99, 99], dtype=np.int64))
    N.call("iqa_ais_frames", N.ptr(a["v"]), c_int64(a["nsym"]), (c_int64 * 8)(*a["count_of"]), c_int32(roomy.plan.W), c_double(roomy.plan.step),
           N.ptr(lst), N.ptr(slots), c_int64(1), N.ptr(counts), N.stream_ptr())
    assert [int(x) for x in counts.cpu().numpy()] == [len(a["start"]), a["candidates"]]
    got, data = lst.cpu().numpy(), slots.cpu().numpy().reshape(2, -1)
    assert (got[4:] == -7).all() and (data[1] == 0xAA).all()
    rows = [tuple(int(x) for x in r) for r in zip(a["phase"], a["s"], a["start"], a["nbytes"])]
    assert tuple(int(x) for x in got[:4]) in rows
    k = rows.index(tuple(int(x) for x in got[:4]))
    np.testing.assert_array_equal(data[0], a["data"][k])
    assert (data[0][int(got[3]) :] == 0).all()


def test_reset_starts_a_new_run(A, streams):
    """``ChannelDemod.reset`` also clears the AIS history, position, stored plane and discriminator state; a non-nfm mode
    is refused with the flag's name."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.processing import ChannelDemod

    fs = 96_000.0
    first = D.to_device(streams[fs][:30_000], "complex64")
    second = D.to_device(M.modulate(M.burst_bits(CLASS_B), fs, sigma=0.05, seed=4), "complex64")

    def run(dem, z):
        dem.process(z, np.array([0], dtype=np.int64), D.empty(int(z.numel()), "float32"))

    used = ChannelDemod("nfm", fs, deemph_us=300.0, agc_enabled=True, ais=True, pocsag=True, ax25=True, tones=True)
    run(used, first)
    used.reset()
    run(used, second)
    fresh = ChannelDemod("nfm", fs, deemph_us=300.0, agc_enabled=True, ais=True)
    run(fresh, second)
    assert used.side["ais"].pos == fresh.side["ais"].pos == int(second.numel())
    a, b = used.side["ais"].finish(), fresh.side["ais"].finish()
    assert len(b["start"]) >= 3
    for key in ("phase", "s", "start", "nbytes", "data"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert [m.raw for m in used.side_result("ais").messages] == [m.raw for m in fresh.side_result("ais", frequency=CHANNEL_B).messages] == [CLASS_B.hex()]
    for mode in ("am", "usb"):
        with pytest.raises(ValueError, match="--demod nfm"):
            ChannelDemod(mode, fs, deemph_us=300.0, agc_enabled=True, ais=True)


def _capture(fs=2.4e6, secs=1.0, seed=17):
    """int16 I/Q: an AIS channel at +525 kHz (a position report, then a two-sentence static report, the carrier 300 Hz off
    tune), a 2400-baud POCSAG channel at -500 kHz, an NFM voice carrier (1 kHz tone, 3 kHz deviation) at +800 kHz; every
    transmitter is keyed from the first sample, so that the mixer-sign probe sees it; complex noise 40 dB below a carrier."""
    n = int(round(fs * secs))
    t = np.arange(n, dtype=np.float64) / fs
    amp = 0.28
    x = np.zeros(n, dtype=np.complex128)
    keyed = np.ones(n, dtype=np.complex128)
    at = int(0.2 * fs)
    for frame, first in ((POSITION, 0), (STATIC, 1)):
        b = M.modulate(M.burst_bits(frame, first=first), fs, offset_hz=300.0, lead=0, tail=0).astype(np.complex128)
        keyed[at : at + b.size] = b
        at += b.size + int(0.1 * fs)
    assert at < n
    x += amp * keyed * np.exp(2j * np.pi * 525e3 * t)
    pager = np.ones(n, dtype=np.complex128)
    b = PM.modulate(PM.transmission_bits(PAGES), fs, 2400, lead=0, tail=0).astype(np.complex128)
    start = int(0.1 * fs)
    assert start + b.size < n
    pager[start : start + b.size] = b
    x += amp * pager * np.exp(2j * np.pi * -500e3 * t)
    x += amp * np.exp(1j * (2 * np.pi * 800e3 * t + 2 * np.pi * 3000.0 / fs * np.cumsum(np.sin(2 * np.pi * 1000.0 * t))))
    rng = np.random.default_rng(seed)
    std = amp * math.sqrt(1e-4 / 2.0)
    x += std * (rng.normal(size=n) + 1j * rng.normal(size=n))
    iq = np.column_stack((x.real, x.imag))
    return np.rint(np.clip(iq, -0.999, 0.999) * 32767.0).astype(np.int16)


def _count_calls(monkeypatch, prefix="iqa_ais_"):
    from iq_to_audio_amd import _native

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith(prefix):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    return calls


def test_end_to_end_three_targets(A, tmp_path, monkeypatch, capsys):
    """One second at 2.4 MS/s through ``cli.main``.  The runs without --ais name --bw 25000, which is what the flag resolves
    an unset --bw to; so the WAVs and the other decoders' files can be compared byte for byte."""
    from iq_to_audio_amd import cli, iqio

    fs, fc = 2.4e6, 161.5e6
    raw = _capture(fs)
    freqs = [fc + 525e3, fc - 500e3, fc + 800e3]
    assert freqs[0] == CHANNEL_B
    outs = {}
    calls = _count_calls(monkeypatch)
    for tag, extra in (("plain", ["--bw", "25000"]), ("ais", ["--ais"]), ("others", ["--pocsag", "--ax25", "--bw", "25000"]),
                       ("all", ["--ais", "--pocsag", "--ax25"])):
        d = tmp_path / tag
        d.mkdir()
        wav = d / "marine_161500000Hz.wav"
        iqio.write_wav_iq(wav, raw, int(fs), "s16")
        argv = ["--in", str(wav), "--demod", "nfm", *extra]
        for f in freqs:
            argv += ["--ft", str(f)]
        before = len(calls)
        assert cli.main(argv) == 0
        outs[tag] = [d / f"audio_{int(f)}_48k.wav" for f in freqs]
        if "--ais" not in extra:
            assert len(calls) == before  # a run without --ais calls no AIS entry point
            assert not list(d.glob("*.ais.json"))
        else:
            assert {"iqa_ais_filter", "iqa_ais_symbols", "iqa_ais_frames"} <= set(calls[before:])
        if tag == "ais":
            printed = capsys.readouterr().out
        else:
            capsys.readouterr()
    for tag in ("ais", "others", "all"):
        for a, b in zip(outs["plain"], outs[tag]):
            assert a.read_bytes() == b.read_bytes()  # the audio does not change
    for tag in ("ais", "all"):
        js = [json.loads(p.with_name(p.stem + ".ais.json").read_text()) for p in outs[tag]]
        print(tag, "targets:", js)
        assert js[1] is None and js[2] is None  # the pager and the voice carrier
        assert [m["raw"] for m in js[0]["messages"]] == [POSITION.hex(), STATIC.hex()]
        assert [(m["type"], m["mmsi"], m["channel"]) for m in js[0]["messages"]] == [(1, 477553000, "B"), (5, 235_087_654, "B")]
        assert js[0]["messages"][0]["nmea"] == [M.REFERENCE_SENTENCE] and js[0]["messages"][1]["name"] == "EVER GIVEN TWO"
        assert [len(m["nmea"]) for m in js[0]["messages"]] == [1, 2] and js[0]["messages"][1]["nmea"][0].startswith("!AIVDM,2,1,0,B,")
        assert all(m["hits"] >= 3 for m in js[0]["messages"])
        assert js[0]["crc_ok"] == sum(m["hits"] for m in js[0]["messages"]) <= js[0]["candidates"]
        times = [m["time_s"] for m in js[0]["messages"]]
        assert times == sorted(times) and 0.2 < times[0] < 0.25
    lines = printed.splitlines()
    assert any(l.startswith(f"{freqs[0]:.0f} Hz: AIS 1 mmsi=477553000 47.58283N 122.34583W 0.0kn 51.0°") for l in lines)
    assert any(l.startswith(f"{freqs[0]:.0f} Hz: AIS 5 mmsi=235087654") and "EVER GIVEN TWO" in l for l in lines)
    assert M.REFERENCE_SENTENCE in lines and sum(l.startswith("!AIVDM") for l in lines) == 3
    assert not any("AIS" in l for l in lines if l.startswith(f"{freqs[1]:.0f} Hz") or l.startswith(f"{freqs[2]:.0f} Hz"))
    # --ais beside --pocsag --ax25 leaves their results as they are
    for a, b in zip(outs["others"], outs["all"]):
        for kind in ("pocsag", "ax25"):
            one, two = (p.with_name(p.stem + f".{kind}.json").read_text() for p in (a, b))
            assert one == two
    pager = json.loads(outs["all"][1].with_name(outs["all"][1].stem + ".pocsag.json").read_text())
    assert [(m["address"], m["function"]) for m in pager["messages"]] == [(a, f) for a, f, _ in PAGES]
