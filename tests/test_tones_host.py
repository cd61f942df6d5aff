"""CTCSS tones and DTMF digits beside narrowband FM (--demod nfm --tones), the host side: the plan, the numpy oracle
(tests/tones_model.py) against plain loops, the decision rules on hand-made energy rows, the bridge / run / sequence rules
on hand-made planes, the oracle alone on model signals (tones and digits under voice and noise come back exactly; voice,
noise, a packet channel and a bare carrier give nothing), CLI and pipeline validation, the C ABI.  No GPU compute."""
from __future__ import annotations

import importlib.util
import sys
from ctypes import c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest

import iq_to_audio_amd as A
from iq_to_audio_amd import dsp_plan as P
from iq_to_audio_amd.decoders import tones as T


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load("tones_model")
AM = _load("ax25_model")

SIGMA = 0.2  # complex noise per component against a carrier of 1
VOICE = 667.0  # Hz rms of the band-limited gaussian "voice"
RATES = [96_000.0, 10e6 / 104]


# ---- plan ----------------------------------------------------------------------------------------------------------------


def test_plan_values():
    want = {8000.0: (1, 8000.0, 80, 1600), 15_999.0: (1, 15_999.0, 160, 3200), 48_000.0: (6, 8000.0, 80, 1600),
            96_000.0: (12, 8000.0, 80, 1600), 10e6 / 104: (12, 10e6 / 104 / 12, 80, 1603), 512_000.0: (64, 8000.0, 80, 1600)}
    for fs, (R, fd, Hd, Hc) in want.items():
        plan, model = P.plan_tones(fs), M.plan(fs)
        assert (plan.R, plan.fd, plan.Hd, plan.Nd, plan.Hc, plan.Nc) == (R, fd, Hd, 2 * Hd, Hc, 2 * Hc), fs
        assert (plan.R, plan.fd, plan.Hd, plan.Nd, plan.Hc, plan.Nc) == tuple(model[k] for k in ("R", "fd", "Hd", "Nd", "Hc", "Nc"))
        assert 8000.0 <= plan.fd < 16_000.0 and plan.Nc <= 6400
        assert plan.ctcss_taps.dtype == np.int16 and plan.ctcss_taps.shape == (50, 2, plan.Nc)
        assert plan.dtmf_taps.dtype == np.int16 and plan.dtmf_taps.shape == (8, 2, plan.Nd)
        np.testing.assert_array_equal(plan.ctcss_taps, model["ctcss_taps"])
        np.testing.assert_array_equal(plan.dtmf_taps, model["dtmf_taps"])
        assert np.abs(plan.ctcss_taps).max() <= 256 and plan.ctcss_taps[:, 0, 0].tolist() == [256] * 50
        for m in (0, plan.Nd - 1, plan.Nd, plan.Nd + plan.Hd - 1, plan.Nd + plan.Hd, 12_345):
            assert plan.frames(plan.Nd, plan.Hd, m) == M.frames_of(plan.Nd, plan.Hd, m)
    assert P.plan_tones(15_999.0).Nc == 6400
    # one tap by hand: tone 1 (69.3 Hz), k = 1000, fd = 8000
    assert P.plan_tones(96_000.0).ctcss_taps[1, 1, 1000] == round(256 * np.sin(2 * np.pi * 69.3 * 1000 / 8000.0))
    for fs in (7999.0, 520_000.0, 0.0, float("nan")):
        with pytest.raises(ValueError):
            P.plan_tones(fs)
    assert (P.CTCSS_TONES, P.DTMF_TONES, P.DTMF_KEYS, P.TONES_MAX_R, P.TONES_NONE) == (M.CTCSS, M.DTMF, M.KEYS, M.MAX_R, M.NONE)
    assert len(P.CTCSS_TONES) == 50 and P.CTCSS_TONES[0] == 67.0 and P.CTCSS_TONES[-1] == 254.1
    assert [P.DTMF_KEYS[4 * r + c] for r, c in ((0, 0), (1, 1), (2, 2), (3, 3), (3, 2), (3, 1))] == list("159D#0")


# ---- decimator and banks ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("R", [1, 2, 3, 12, 64])
def test_decimator_against_a_double_loop(R):
    rng = np.random.default_rng(R)
    n = 5 * R + R // 2 + 37
    t = rng.integers(-12_868, 12_869, size=n).astype(np.int32)
    t[: n // 3] = -np.abs(t[: n // 3])  # long negative sums, so that floor (not truncation) is checked
    got = M.decimate(t, R)
    want, differs = [], 0
    for m in range(n // R):
        acc = 0
        for j in range(2 * R - 1):
            at = (m + 1) * R - 1 - j
            if at >= 0:
                acc += min(j + 1, 2 * R - 1 - j) * int(t[at])
        want.append(acc // R)  # python's // floors
        differs += int(acc / R) != acc // R
    assert got.dtype == np.int32 and got.tolist() == want
    assert R == 1 or differs > 0  # the case distinguishes floor from truncation
    assert M.decimate(t[: R - 1], R).size == 0 and M.decimate(t[:R], R).size == 1
    assert R * 12_868 < 2 ** 20


def test_bank_against_a_plain_loop():
    pl = M.plan(96_000.0)
    rng = np.random.default_rng(1)
    u = rng.integers(-(2 ** 20) + 1, 2 ** 20, size=pl["Nd"] + 3 * pl["Hd"] + 5).astype(np.int32)
    E, Pw = M.bank(u, pl["dtmf_taps"], pl["Nd"], pl["Hd"])
    assert E.shape == (4, 8) and E.dtype == np.int64 and Pw.shape == (4,)
    for i in range(4):
        fr = [int(v) for v in u[i * pl["Hd"] : i * pl["Hd"] + pl["Nd"]]]
        assert int(Pw[i]) == sum(v * v for v in fr)
        for f in range(8):
            I = sum(int(c) * v for c, v in zip(pl["dtmf_taps"][f, 0], fr))
            Q = sum(int(s) * v for s, v in zip(pl["dtmf_taps"][f, 1], fr))
            assert int(E[i, f]) == (I >> 12) ** 2 + (Q >> 12) ** 2
    assert M.bank(u[: pl["Nd"] - 1], pl["dtmf_taps"], pl["Nd"], pl["Hd"])[0].shape == (0, 8)
    # the bounds the specification states: |I| < 2^41 at the longest frame, E < 2^59
    worst = 64 * 12_868 * 256 * 6400
    assert worst < 2 ** 41 and 2 * (worst >> 12) ** 2 < 2 ** 59 and worst >= 2 ** 31


# ---- decisions -------------------------------------------------------------------------------------------------------------


def test_ctcss_decision_rules():
    base = [2000] * 50

    def code(row):
        return int(M.decide_ctcss(np.array([row], dtype=np.int64))[0])

    hit = list(base)
    hit[7] = 64 * 2000 + 63
    assert code(hit) == 7  # (E >> 6) == med: the boundary is a hit
    hit[7] = 64 * 2000 - 1
    assert code(hit) == 255 and hit[7] >= 1 << 16  # one below it: the ratio alone fails
    tie = list(base)
    tie[30] = tie[12] = 1 << 20
    assert code(tie) == 12  # the lowest index of the maximum
    assert code([0] * 50) == 255  # all zero: 0 >= 0 holds, the floor of 2^16 does not
    low = [0] * 50
    low[3] = (1 << 16) - 1
    assert code(low) == 255
    low[3] = 1 << 16
    assert code(low) == 3
    # the median is sorted[24], not sorted[25]: 25 small values and 25 large ones
    half = [10] * 25 + [1 << 30] * 24 + [1 << 35]
    assert code(half) == 49  # med = 10
    half = [10] * 24 + [1 << 30] * 25 + [1 << 35]
    assert code(half) == 255  # med = 2^30 > 2^35 >> 6
    big = [(1 << 59) - 1] * 50
    assert code(big) == 255  # 64 x the median is never formed: no overflow at the largest energies


def test_dtmf_decision_rules():
    Nd = 160
    big = 1 << 30

    def code(row, p=0):
        return int(M.decide_dtmf(np.array([row], dtype=np.int64), np.array([p], dtype=np.int64), Nd)[0])

    good = [big >> 4, big, big >> 4, 0, 0, big >> 4, big, big >> 4]
    assert code(good) == 4 * 1 + 2 and M.KEYS[code(good)] == "6"
    assert code([0] * 8) == 255
    fail = list(good)
    fail[0] = (big >> 3) + 1  # E_r < 8 r2
    assert code(fail) == 255
    fail[0] = big >> 3  # E_r == 8 r2: a hit
    assert code(fail) == 6
    fail = list(good)
    fail[7] = (big >> 3) + 1  # E_c < 8 c2
    assert code(fail) == 255
    twist = [0, big, 0, 0, 0, 0, 16 * big, 0]
    assert code(twist) == 6
    twist[6] = 16 * big + 1  # E_c > 16 E_r
    assert code(twist) == 255
    twist = [0, 16 * big + 1, 0, 0, 0, 0, big, 0]  # E_r > 16 E_c
    assert code(twist) == 255
    floor = [0, 1 << 16, 0, 0, 0, 0, 1 << 16, 0]
    assert code(floor) == 6
    assert code([0, (1 << 16) - 1, 0, 0, 0, 0, 1 << 16, 0]) == 255  # E_r below the floor
    assert code([0, 1 << 16, 0, 0, 0, 0, (1 << 16) - 1, 0]) == 255  # E_c below the floor
    # the talk-off guard: 1024 (E_r + E_c) >= Nd P
    p_edge = 1024 * 2 * big // Nd
    assert 1024 * 2 * big >= Nd * p_edge and code([0, big, 0, 0, 0, 0, big, 0], p_edge) == 6
    assert code([0, big, 0, 0, 0, 0, big, 0], p_edge + 7) == 255
    # ties: two equal row maxima count as maximum and second, so 8 r2 > E_r; the lowest index is the row
    assert code([big, big, 0, 0, 0, 0, big, 0]) == 255
    assert code([0, 0, 0, big, 0, 0, 0, big]) == 15


# ---- bridge, runs, sequences -----------------------------------------------------------------------------------------------


def _both(plan, cc, dc):
    got, want = T.parse_tones(plan, np.array(cc, dtype=np.uint8), np.array(dc, dtype=np.uint8)), M.parse(M.plan(plan.fs), cc, dc)
    assert (got is None) == (want is None)
    if got is not None:
        assert got.to_json() == want
    return got


def test_bridge_and_run_rules():
    plan = P.plan_tones(96_000.0)
    n = 255
    assert T.bridge([5, n, 5, n, n, 5, 9, n, 5, n]).tolist() == [5, 5, 5, n, n, 5, 9, n, 5, n] == M.bridge([5, n, 5, n, n, 5, 9, n, 5, n])
    assert T.bridge([5, n, 5, n, 5]).tolist() == [5, 5, 5, 5, 5]  # one pass over the original plane fills both
    assert T.bridge([n, 5, n]).tolist() == [n, 5, n] and T.bridge([5, n]).tolist() == [5, n] and T.bridge([]).tolist() == []
    assert T.bridge([5, 7, 5]).tolist() == [5, 7, 5]  # a foreign code in the gap stays
    assert T.runs([5, 5, n, 7, 7, 7, n, n, 7, 7, 7, 7]) == [(7, 3, 5), (7, 8, 11)] == M.runs([5, 5, n, 7, 7, 7, n, n, 7, 7, 7, 7])
    # runs of 2 and 3; a gap of 1 is bridged, a gap of 2 is not; a foreign code splits
    assert _both(plan, [], [3, 3, n, n]) is None
    res = _both(plan, [], [3, 3, 3, n, n])
    assert [(e.key, e.frames, e.start_s, e.end_s) for e in res.dtmf] == [("A", 3, 0.0, (2 * 80 + 160) * 12 / 96_000.0)]
    res = _both(plan, [], [n, 3, n, 3, n])
    assert [(e.key, e.frames, e.start_s) for e in res.dtmf] == [("A", 3, 80 * 12 / 96_000.0)]
    assert _both(plan, [], [3, n, n, 3, 3]) is None
    assert _both(plan, [], [3, 3, 4, 3, 3]) is None
    res = _both(plan, [0, 0, n, 0, 49, 49, 49], [])
    assert [(e.tone_hz, e.frames, e.start_s, e.end_s) for e in res.ctcss] == [(67.0, 4, 0.0, (3 * 1600 + 3200) / 8000.0), (254.1, 3, 0.8, 1.6)]
    assert res.dtmf == [] and res.sequences == [] and res.lines() == ["CTCSS 67.0 Hz 0.00-1.00 s", "CTCSS 254.1 Hz 0.80-1.60 s"]
    # sequences: a digit that starts within 2.0 s of the end of the one before continues the sequence
    # (the first digit, frames 0 .. 2, ends at 0.04 s; a second one from frame 203 starts 1.99 s later, from frame 205 2.01 s)
    for at, want in ((203, ["25"]), (205, ["2", "5"])):
        res = _both(plan, [], [1] * 3 + [n] * (at - 3) + [5] * 3)
        assert [s.digits for s in res.sequences] == want, at
        assert res.sequences[-1].time_s == (0.0 if len(want) == 1 else at * 80 * 12 / 96_000.0)
    res = _both(plan, [12] * 11, [n] * 50 + [0] * 4 + [n] * 6 + [5] * 4 + [n] * 6 + [10] * 4 + [n] * 300 + [15] * 3)
    assert [(s.time_s, s.digits) for s in res.sequences] == [(0.5, "159"), (3.74, "D")]
    assert res.lines() == ["CTCSS 100.0 Hz 0.00-2.40 s", "DTMF 159 at 0.50 s", "DTMF D at 3.74 s"]
    assert res.to_json()["sequences"][0] == dict(time_s=0.5, digits="159")


# ---- the oracle alone on model signals -------------------------------------------------------------------------------------


def _report(name, fs, out):
    r = M.median_ratios(out["E_ctcss"])
    hits = {}
    for c in out["dtmf"].tolist():
        if c != 255:
            hits[M.KEYS[c]] = hits.get(M.KEYS[c], 0) + 1
    print(f"fs {fs:.1f} {name}: winner / median {r.min():.0f} .. {r.max():.0f} over {r.size} frames; DTMF hit frames {hits}")
    return r


@pytest.mark.parametrize("fs", RATES)
def test_oracle_recovers_tones_and_digits(fs):
    """Every case under voice of 667 Hz rms and noise of 0.2 per component: exactly the transmitted tone, exactly the
    transmitted digits, nothing else."""
    secs = 2.4
    for name, kw, tone in (("67.0 Hz at 500 Hz", dict(ctcss_hz=67.0, ctcss_dev=500.0), 67.0),
                           ("69.3 Hz at 300 Hz, 500 Hz off tune", dict(ctcss_hz=69.3, ctcss_dev=300.0, offset_hz=500.0), 69.3),
                           ("254.1 Hz", dict(ctcss_hz=254.1, ctcss_dev=500.0), 254.1)):
        out = M.oracle(M.theta_of(M.synth(fs, secs, voice_rms=VOICE, sigma=SIGMA, seed=3, **kw)), fs)
        r = _report(name, fs, out)
        assert r.min() >= 64
        res = out["result"]
        assert [e["tone_hz"] for e in res["ctcss"]] == [tone] and res["dtmf"] == [] and res["sequences"] == []
        ev = res["ctcss"][0]
        assert ev["start_s"] == 0.0 and ev["frames"] == out["ctcss"].size >= 10 and secs - 0.2 <= ev["end_s"] <= secs
        assert (out["ctcss"] == M.CTCSS.index(tone)).all()
        got = T.parse_tones(P.plan_tones(fs), out["ctcss"], out["dtmf"])
        assert got.to_json() == res and got.lines()[0].startswith(f"CTCSS {tone:.1f} Hz 0.00-")
    for digits, gain in (("159D#0", 1.0), ("A7*", 2.0)):
        out = M.oracle(M.theta_of(M.synth(fs, secs, voice_rms=VOICE, sigma=SIGMA, seed=3, digits=digits, col_gain=gain)), fs)
        _report(f"digits {digits} columns x{gain:.0f}", fs, out)
        res = out["result"]
        assert res["ctcss"] == [] and [e["key"] for e in res["dtmf"]] == list(digits)
        assert all(3 <= e["frames"] <= 5 for e in res["dtmf"])
        assert [s["digits"] for s in res["sequences"]] == [digits] and abs(res["sequences"][0]["time_s"] - 0.5) <= 0.011
        got = T.parse_tones(P.plan_tones(fs), out["ctcss"], out["dtmf"])
        assert got.to_json() == res and got.lines() == [f"DTMF {digits} at 0.50 s"]


@pytest.mark.parametrize("fs", RATES)
def test_oracle_finds_nothing_in_voice_noise_packets_and_a_carrier(fs):
    """Voice alone, 4 s of carrier-less noise, and the two other channels of the GPU test's capture (an AX.25 transmission
    and a bare carrier) carry no event."""
    frame = AM.ui_frame("N0CALL-7", "APRS", ["WIDE1-1*"], "!4903.50N/07201.75W-Test 001234 of the tone detector, which must not hear this")
    cases = (("voice alone", M.synth(fs, 2.4, voice_rms=VOICE, sigma=SIGMA, seed=4), 39),
             ("noise", M.synth(fs, 4.0, carrier=0.0, sigma=SIGMA, seed=5), 18),
             ("AX.25", AM.modulate(AM.hdlc_bits([frame, frame, frame]), fs, sigma=0.01, seed=6, lead=0, tail=0), None),
             ("bare carrier", M.synth(fs, 2.4, sigma=0.01, seed=7), None))
    for name, z, seen in cases:
        out = M.oracle(M.theta_of(z), fs)
        r = _report(name, fs, out)
        assert out["result"] is None, name
        assert T.parse_tones(P.plan_tones(fs), out["ctcss"], out["dtmf"]) is None
        if seen is not None:
            assert r.max() < 64  # (the feature request's own run saw at most 39 for voice and 18 for noise)


# ---- the host surface ------------------------------------------------------------------------------------------------------


def test_cli_and_pipeline_validation(tmp_path, capsys):
    from iq_to_audio_amd import cli
    from iq_to_audio_amd.batch import ResidentBankRunner, ResidentCaptureRunner, demodulate_sharded

    with pytest.raises(SystemExit) as exc:
        cli.main(["--in", str(tmp_path / "x.wav"), "--ft", "1e6", "--tones", "--demod", "am"])
    assert exc.value.code == 2 and "--tones needs --demod nfm" in capsys.readouterr().err
    assert cli.build_parser().parse_args(["--in", "x.wav"]).tones is False
    allthree = cli.build_parser().parse_args(["--in", "x.wav", "--tones", "--ax25", "--pocsag"])
    assert allthree.tones and allthree.ax25 and allthree.pocsag
    wfm = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="wfm")
    nfm = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="nfm")
    with pytest.raises(ValueError, match="tones"):
        A.ProcessingPipeline(wfm, tones=True)
    with pytest.raises(ValueError, match="tones"):
        A.MultiChannelPipeline([nfm, wfm], tones=True)
    assert A.ProcessingPipeline(nfm, tones=True).tones_enabled and not A.ProcessingPipeline(nfm).tones_enabled
    assert all(o.tones_enabled and o.ax25_enabled for o in A.MultiChannelPipeline([nfm, nfm], tones=True, ax25=True).owners)
    assert len(A.ProcessingConfig.__dataclass_fields__) == 23
    with pytest.raises(ValueError, match="tones"):
        ResidentBankRunner([dict(freq_offset=25e3)], sample_rate=2.5e6, n_frames=1 << 20, tones=True)
    with pytest.raises(ValueError, match="tones"):
        ResidentCaptureRunner(np.ones(8), sample_rate=2.5e6, freq_offset=25e3, decimation=26, fs_channel=2.5e6 / 26, chunk=1 << 20,
                              n_frames=1 << 20, tones=True)
    with pytest.raises(ValueError, match="tones"):
        demodulate_sharded([dict(freq_offset=25e3)], sample_rate=2.5e6, n_frames=1 << 20, axis="channels", tones=True)


def test_c_abi_refuses_bad_arguments():
    """The library has the three entry points, and their argument checks come before any launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some = c_void_p(0), c_void_p(8)  # (never dereferenced: every call below is refused, or has nothing to do)
    for name in ("iqa_tones_decimate", "iqa_tones_bank", "iqa_tones_decide"):
        assert hasattr(N.lib(), name) and name in N.EXPORTS
    assert N.lib().iqa_abi_version() == 1
    for R in (0, 65, -1):
        with pytest.raises(ValueError, match="R must be"):
            N.call("iqa_tones_decimate", some, c_int64(16), c_int64(0), null, c_int32(R), some, some, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_tones_decimate", null, c_int64(16), c_int64(0), null, c_int32(12), some, some, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_tones_decimate", some, c_int64(16), c_int64(0), null, c_int32(12), null, some, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_tones_decimate", some, c_int64(16), c_int64(0), null, c_int32(12), some, null, null)  # (completes u[0])
    with pytest.raises(ValueError, match="negative"):
        N.call("iqa_tones_decimate", some, c_int64(-1), c_int64(0), null, c_int32(12), some, some, null)
    with pytest.raises(ValueError, match="negative"):
        N.call("iqa_tones_decimate", some, c_int64(16), c_int64(-5), null, c_int32(12), some, some, null)
    N.call("iqa_tones_decimate", null, c_int64(0), c_int64(7), null, c_int32(12), null, null, null)  # nothing to do
    for frame, hop, ntones, what in ((0, 1, 8, "frame"), (6401, 80, 8, "frame"), (160, 0, 8, "hop"), (160, 161, 8, "hop"), (160, 80, 0, "ntones"),
                                     (160, 80, 65, "ntones")):
        with pytest.raises(ValueError, match=what):
            N.call("iqa_tones_bank", some, c_int64(1000), c_int32(frame), c_int32(hop), c_int32(ntones), some, some, null, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_tones_bank", null, c_int64(1000), c_int32(160), c_int32(80), c_int32(8), some, some, null, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_tones_bank", some, c_int64(1000), c_int32(160), c_int32(80), c_int32(8), some, null, null, null)
    with pytest.raises(ValueError, match="negative"):
        N.call("iqa_tones_bank", some, c_int64(-1), c_int32(160), c_int32(80), c_int32(8), some, some, null, null)
    N.call("iqa_tones_bank", null, c_int64(159), c_int32(160), c_int32(80), c_int32(8), null, null, null, null)  # no frame: nothing to do
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_tones_decide", null, c_int64(4), some, some, c_int64(4), c_int32(160), some, some, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_tones_decide", some, c_int64(4), some, null, c_int64(4), c_int32(160), some, some, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_tones_decide", some, c_int64(4), some, some, c_int64(4), c_int32(160), some, null, null)
    with pytest.raises(ValueError, match="frame"):
        N.call("iqa_tones_decide", some, c_int64(4), some, some, c_int64(4), c_int32(0), some, some, null)
    with pytest.raises(ValueError, match="negative"):
        N.call("iqa_tones_decide", some, c_int64(-1), some, some, c_int64(4), c_int32(160), some, some, null)
    N.call("iqa_tones_decide", null, c_int64(0), null, null, c_int64(0), c_int32(160), null, null, null)  # nothing to do
