"""CTCSS tones and DTMF digits beside narrowband FM (--demod nfm --tones) on the MI355X: every integer stage identical to
the numpy oracle of tests/tones_model.py, the edge geometries (R = 1, the longest frame, R = 64, streams of exactly one
frame and one sample short of it), sums beyond int32, block invariance bit for bit, the decision kernel on hand-made energy
rows, the CLI end to end on a capture with a voice channel, a packet channel and a bare carrier, and the proof that a run
without --tones calls no tone entry point."""
from __future__ import annotations

import importlib.util
import json
import math
import sys
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


M = _load("tones_model")
AM = _load("ax25_model")

SIGMA, VOICE, SECS = 0.2, 667.0, 2.4
RATES = [96_000.0, 10e6 / 104]
DIGITS = "159D#0"
STAGES = ("u", "E_ctcss", "E_dtmf", "P", "ctcss", "dtmf")


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _stream(fs: float, seed: int = 3, secs: float = SECS, tone: float = 67.0) -> np.ndarray:
    return M.synth(fs, secs, ctcss_hz=tone, ctcss_dev=500.0, voice_rms=VOICE, digits=DIGITS, sigma=SIGMA, seed=seed)


def _same_stages(st: dict, want: dict) -> None:
    for key in STAGES:
        assert st[key].dtype == want[key].dtype and st[key].shape == want[key].shape, (key, st[key].dtype, st[key].shape, want[key].shape)
        np.testing.assert_array_equal(st[key], want[key], err_msg=key)


def _same_result(res, want) -> None:
    assert (res is None) == (want is None)
    if res is not None:
        assert res.to_json() == want


def _run(fs: float, block, cuts=None):
    from iq_to_audio_amd.decoders.tones import ToneDecoder

    dec = ToneDecoder(fs)
    n = len(block)
    cuts = [0, n] if cuts is None else cuts
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        dec.process(block[lo:hi])
    assert dec.core.pos == n
    return dec


@pytest.mark.parametrize("fs", RATES)
def test_stages_are_the_oracles(A, fs):
    """t is the oracle's quantiser of the GPU's own theta, exactly; against numpy's float32 theta it differs by at most 1;
    from the GPU's t, the decimated stream, both energy arrays, the power sums, both code planes and the parsed result are
    the oracle's.  Integers: no tolerance."""
    z = _stream(fs)
    dec = _run(fs, z)
    st = dec.stages()
    assert st["t"].dtype == np.int32 and st["t"].size == z.size
    np.testing.assert_array_equal(st["t"], M.quantise(st["theta"]))
    dt = np.abs(st["t"].astype(np.int64) - M.quantise(M.theta_of(z)).astype(np.int64))
    print(f"fs {fs}: t against numpy's theta: {np.mean(dt != 0):.4%} of {dt.size} samples differ, max |dt| {dt.max()}")
    assert dt.max() <= 1
    want = M.oracle(fs=fs, t=st["t"])
    assert want["u"].size == z.size // dec.plan.R and want["E_ctcss"].shape[0] >= 10 and want["E_dtmf"].shape[0] >= 200
    _same_stages(st, want)
    res = dec.finish()
    _same_result(res, want["result"])
    assert [e.tone_hz for e in res.ctcss] == [67.0] and [s.digits for s in res.sequences] == [DIGITS]
    assert res.lines()[0].startswith("CTCSS 67.0 Hz 0.00-2.") and res.lines()[1] == f"DTMF {DIGITS} at 0.50 s"


@pytest.mark.parametrize("fs", [8000.0, 15_999.0, 512_000.0])
def test_edge_rates(A, fs):
    """R = 1 (the window degenerates to [1]; no history), R = 1 with the longest frame (Nc = 6400), and R = 64; each fed in
    two blocks."""
    z = _stream(fs, seed=8)
    dec = _run(fs, z, [0, z.size // 3 + 1, z.size])
    assert (dec.plan.R, dec.plan.Nc) == {8000.0: (1, 3200), 15_999.0: (1, 6400), 512_000.0: (64, 3200)}[fs]
    assert dec.core.hist_len == 2 * dec.plan.R - 2
    st = dec.stages()
    np.testing.assert_array_equal(st["t"], M.quantise(st["theta"]))
    want = M.oracle(fs=fs, t=st["t"])
    if dec.plan.R == 1:
        np.testing.assert_array_equal(st["u"], st["t"])
    assert want["E_ctcss"].shape[0] >= 5
    _same_stages(st, want)
    _same_result(dec.finish(), want["result"])


@pytest.mark.parametrize("extra", ["Nc-1", "Nc", "Nc+Hc"])
@pytest.mark.parametrize("fs", RATES)
def test_edge_stream_lengths(A, fs, extra):
    """Streams whose decimated length is one short of a CTCSS frame (F = 0: nothing is written), exactly one frame, and one
    frame and one hop; the channel-rate length is not a multiple of R."""
    from ctypes import c_int32, c_int64

    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    pl = M.plan(fs)
    m = {"Nc-1": pl["Nc"] - 1, "Nc": pl["Nc"], "Nc+Hc": pl["Nc"] + pl["Hc"]}[extra]
    z = _stream(fs, seed=9, secs=1.0)[: m * pl["R"] + pl["R"] - 1]
    dec = _run(fs, z)
    st = dec.stages()
    want = M.oracle(fs=fs, t=st["t"])
    assert want["u"].size == m and want["E_ctcss"].shape[0] == {"Nc-1": 0, "Nc": 1, "Nc+Hc": 2}[extra]
    _same_stages(st, want)
    _same_result(dec.finish(), want["result"])
    if extra == "Nc-1":  # the call itself: no frame, so the output stays as it was
        sentinel = D.from_numpy(np.full(100, -7, dtype=np.int64))
        N.call("iqa_tones_bank", N.ptr(dec.core.joined()["u"]), c_int64(m), c_int32(pl["Nc"]), c_int32(pl["Hc"]), c_int32(50),
               N.ptr(dec.core._ctcss_taps), N.ptr(sentinel), N.ptr(None), N.stream_ptr())
        assert (sentinel.cpu().numpy() == -7).all()


@pytest.mark.parametrize("fs", [15_999.0, 512_000.0])
def test_sums_beyond_int32(A, fs):
    """theta a +-pi square wave at 67.0 Hz: |t| = 12 868 throughout and the 67.0 Hz correlator's sums lie far beyond int32
    (near their bound at R = 64 and at Nc = 6400).  The energies are the oracle's."""
    n = int(round(fs * SECS))
    k = np.arange(n, dtype=np.float64)
    theta = np.where(np.sin(2.0 * np.pi * 67.0 * k / fs) >= 0.0, np.float32(np.pi), np.float32(-np.pi)).astype(np.float32)
    dec = _run(fs, theta)
    st = dec.stages()
    assert np.abs(st["t"]).min() == np.abs(st["t"]).max() == 12_868
    want = M.oracle(fs=fs, t=st["t"])
    top = int(want["E_ctcss"].max())
    print(f"fs {fs}: max E {top} = 2^{math.log2(top):.1f}; max |u| {np.abs(want['u']).max()}")
    assert top > 2 * ((1 << 32) >> 12) ** 2  # so |I| or |Q| is beyond 2^32: an int32 sum is wrong here
    assert top < 1 << 59
    _same_stages(st, want)
    assert st["ctcss"].size >= 10


@pytest.mark.parametrize("fs", RATES)
def test_block_invariance(A, fs):
    """One stream as a single block and in uneven cuts (shorter than R, a single sample, cuts inside the 2R - 2 carried
    history, a block that completes no output): every stage bit-identical."""
    from iq_to_audio_amd import _dev as D

    z = D.to_device(_stream(fs, seed=5), "complex64")
    n = int(z.numel())
    runs = []
    for cuts in (None, [0, 100_003, 100_004, 101_000, 200_001, n], [0, 5, 6, 13, 14, 30, 41, 8192 + 17, 8192 + 20, n - 30_000, n - 7, n - 1, n]):
        dec = _run(fs, z, cuts)
        if cuts is not None:
            assert min(b - a for a, b in zip(cuts[:-1], cuts[1:])) == 1 < dec.plan.R and dec.core.hist_len == 22
        runs.append(dec.stages())
    assert (runs[0]["ctcss"] != 255).any() and (runs[0]["dtmf"] != 255).any()
    for st in runs[1:]:
        for key in ("theta", "t") + STAGES:
            np.testing.assert_array_equal(st[key], runs[0][key], err_msg=key)


def _hand_made_rows():
    rng = np.random.default_rng(2)
    rows = []
    for at, top in ((7, 64 * 2000 + 63), (7, 64 * 2000 - 1), (12, 1 << 20)):
        row = [2000] * 50
        row[at] = top
        rows.append(row)
    rows[2][30] = 1 << 20
    rows += [[0] * 50, [0] * 3 + [(1 << 16) - 1] + [0] * 46, [0] * 3 + [1 << 16] + [0] * 46, [10] * 25 + [1 << 30] * 24 + [1 << 35],
             [10] * 24 + [1 << 30] * 25 + [1 << 35], [(1 << 59) - 1] * 50]
    rows += [[int(v) for v in r] for r in (rng.integers(0, 1 << 40, size=(40, 50)) >> rng.integers(0, 40, size=(40, 50)))]
    Ec = np.array(rows, dtype=np.int64)
    big, Nd = 1 << 30, 160
    p_edge = 1024 * 2 * big // Nd
    drows = [([big >> 4, big, big >> 4, 0, 0, big >> 4, big, big >> 4], 0), ([0] * 8, 0), ([(big >> 3) + 1, big, 0, 0, 0, 0, big, 0], 0),
             ([big >> 3, big, 0, 0, 0, 0, big, 0], 0), ([0, big, 0, 0, 0, 0, big, (big >> 3) + 1], 0), ([0, big, 0, 0, 0, 0, 16 * big, 0], 0),
             ([0, big, 0, 0, 0, 0, 16 * big + 1, 0], 0), ([0, 16 * big + 1, 0, 0, 0, 0, big, 0], 0), ([0, 1 << 16, 0, 0, 0, 0, 1 << 16, 0], 0),
             ([0, (1 << 16) - 1, 0, 0, 0, 0, 1 << 16, 0], 0), ([0, 1 << 16, 0, 0, 0, 0, (1 << 16) - 1, 0], 0), ([0, big, 0, 0, 0, 0, big, 0], p_edge),
             ([0, big, 0, 0, 0, 0, big, 0], p_edge + 7), ([big, big, 0, 0, 0, 0, big, 0], 0), ([0, 0, 0, big, 0, 0, 0, big], 0),
             ([0, 0, (1 << 51) - 1, 0, (1 << 51) - 1, 0, 0, 0], (1 << 62) // Nd - 100)]
    Ed = np.array([r for r, _ in drows], dtype=np.int64)
    Pd = np.array([p for _, p in drows], dtype=np.int64)
    return Ec, Ed, Pd, Nd


def test_decisions_on_hand_made_rows(A):
    """``iqa_tones_decide`` on hand-made energies: ties, zeros, the >> 6 boundary, the floors, every DTMF condition at its
    edge, the largest energies.  The codes are the oracle's, and planes of different lengths are handled in one call."""
    from ctypes import c_int32, c_int64

    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    Ec, Ed, Pd, Nd = _hand_made_rows()
    want_c, want_d = M.decide_ctcss(Ec), M.decide_dtmf(Ed, Pd, Nd)
    assert want_c[:9].tolist() == [7, 255, 12, 255, 255, 3, 49, 255, 255]
    assert want_d.tolist() == [6, 255, 255, 6, 255, 6, 255, 255, 6, 255, 255, 6, 255, 255, 15, 8]
    got_c = D.from_numpy(np.full(Ec.shape[0] + 3, 0xAA, dtype=np.uint8))
    got_d = D.from_numpy(np.full(Ed.shape[0] + 3, 0xAA, dtype=np.uint8))
    dev = [D.from_numpy(x) for x in (Ec, Ed, Pd)]  # (held: a temporary's memory would be handed to the next upload)
    N.call("iqa_tones_decide", N.ptr(dev[0]), c_int64(Ec.shape[0]), N.ptr(dev[1]), N.ptr(dev[2]), c_int64(Ed.shape[0]), c_int32(Nd),
           N.ptr(got_c), N.ptr(got_d), N.stream_ptr())
    got_c, got_d = got_c.cpu().numpy(), got_d.cpu().numpy()
    np.testing.assert_array_equal(got_c[:-3], want_c)
    np.testing.assert_array_equal(got_d[:-3], want_d)
    assert (got_c[-3:] == 0xAA).all() and (got_d[-3:] == 0xAA).all()


def test_reset_starts_a_new_run(A):
    """``ChannelDemod.reset`` also clears the tone history, position, stored u and discriminator state; a non-nfm target
    refuses tones."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.processing import ChannelDemod

    fs = 96_000.0
    first = D.to_device(_stream(fs, seed=5)[:150_001], "complex64")
    second = D.to_device(_stream(fs, seed=6, tone=254.1), "complex64")

    def run(dem, z):
        dem.process(z, np.array([0], dtype=np.int64), D.empty(int(z.numel()), "float32"))

    used = ChannelDemod("nfm", fs, deemph_us=300.0, agc_enabled=True, tones=True)
    run(used, first)
    used.reset()
    run(used, second)
    fresh = ChannelDemod("nfm", fs, deemph_us=300.0, agc_enabled=True, tones=True)
    run(fresh, second)
    assert used.side["tones"].pos == fresh.side["tones"].pos == int(second.numel())
    a, b = used.side["tones"].finish(), fresh.side["tones"].finish()
    for key in ("E_ctcss", "E_dtmf", "P", "ctcss", "dtmf"):
        np.testing.assert_array_equal(a[key].cpu().numpy(), b[key].cpu().numpy(), err_msg=key)
    res = used.side_result("tones")
    assert res.to_json() == fresh.side_result("tones").to_json()
    assert [e.tone_hz for e in res.ctcss] == [254.1] and [s.digits for s in res.sequences] == [DIGITS]
    with pytest.raises(ValueError, match="tones"):
        ChannelDemod("am", fs, deemph_us=300.0, agc_enabled=True, tones=True)


FRAME = ("N0CALL-7", "APRS", ["WIDE1-1*"], "!4903.50N/07201.75W-Test 001234 of the tone detector, which must not hear this")
TONE = 100.0


def _capture(fs=2.4e6, secs=3.0, seed=17):
    """int16 I/Q: a voice channel at +300 kHz (100.0 Hz CTCSS at 500 Hz, voice of 667 Hz rms, the digits 159D#0 from 0.5 s),
    an AX.25 channel at -500 kHz (three frames from 0.2 s, a carrier around them), a bare carrier at +800 kHz; complex noise
    40 dB below a carrier."""
    n = int(round(fs * secs))
    t = np.arange(n, dtype=np.float64) / fs
    amp = 0.28
    x = amp * M.synth(fs, secs, ctcss_hz=TONE, ctcss_dev=500.0, voice_rms=VOICE, digits=DIGITS, seed=seed).astype(np.complex128) * np.exp(
        2j * np.pi * 300e3 * t)
    keyed = np.ones(n, dtype=np.complex128)
    b = AM.modulate(AM.hdlc_bits([AM.ui_frame(*FRAME)] * 3), fs, lead=0, tail=0).astype(np.complex128)
    at = int(0.2 * fs)
    assert at + b.size < n
    keyed[at : at + b.size] = b
    x += amp * keyed * np.exp(2j * np.pi * -500e3 * t)
    x += amp * np.exp(2j * np.pi * 800e3 * t)
    rng = np.random.default_rng(seed)
    std = amp * math.sqrt(1e-4 / 2.0)
    x += std * (rng.normal(size=n) + 1j * rng.normal(size=n))
    iq = np.column_stack((x.real, x.imag))
    return np.rint(np.clip(iq, -0.999, 0.999) * 32767.0).astype(np.int16)


def _count_calls(monkeypatch, prefix="iqa_tones_"):
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
    from iq_to_audio_amd import cli, iqio

    fs, fc = 2.4e6, 455.5e6
    raw = _capture(fs)
    freqs = [fc + 300e3, fc - 500e3, fc + 800e3]
    outs = {}
    calls = _count_calls(monkeypatch)
    for tag, extra in (("plain", []), ("tones", ["--tones"]), ("others", ["--ax25", "--pocsag"]), ("all", ["--tones", "--ax25", "--pocsag"])):
        d = tmp_path / tag
        d.mkdir()
        wav = d / "voice_455500000Hz.wav"
        iqio.write_wav_iq(wav, raw, int(fs), "s16")
        argv = ["--in", str(wav), "--demod", "nfm", *extra]
        for f in freqs:
            argv += ["--ft", str(f)]
        before = len(calls)
        assert cli.main(argv) == 0
        outs[tag] = [d / f"audio_{int(f)}_48k.wav" for f in freqs]
        if "--tones" not in extra:
            assert len(calls) == before  # a run without --tones calls no tone entry point
            assert not list(d.glob("*.tones.json"))
        else:
            assert {"iqa_tones_decimate", "iqa_tones_bank", "iqa_tones_decide"} <= set(calls[before:])
        if tag == "tones":
            printed = capsys.readouterr().out
        else:
            capsys.readouterr()
    for tag in ("tones", "others", "all"):
        for a, b in zip(outs["plain"], outs[tag]):
            assert a.read_bytes() == b.read_bytes()  # the audio does not change
    for tag in ("tones", "all"):
        js = [json.loads(p.with_name(p.stem + ".tones.json").read_text()) for p in outs[tag]]
        print(tag, "targets:", js)
        assert js[1] is None and js[2] is None  # the packet channel and the bare carrier
        assert [e["tone_hz"] for e in js[0]["ctcss"]] == [TONE]
        ev = js[0]["ctcss"][0]
        assert ev["start_s"] <= 0.2 and ev["end_s"] >= 2.8 and ev["frames"] >= 13
        assert [e["key"] for e in js[0]["dtmf"]] == list(DIGITS)
        assert [s["digits"] for s in js[0]["sequences"]] == [DIGITS] and abs(js[0]["sequences"][0]["time_s"] - 0.5) <= 0.02
    lines = [l for l in printed.splitlines() if " Hz: CTCSS " in l or " Hz: DTMF " in l]
    assert len(lines) == 2 and all(l.startswith(f"{freqs[0]:.0f} Hz: ") for l in lines)
    assert lines[0].startswith(f"{freqs[0]:.0f} Hz: CTCSS {TONE:.1f} Hz 0.") and lines[1].startswith(f"{freqs[0]:.0f} Hz: DTMF {DIGITS} at 0.")
    # --tones beside --ax25 --pocsag leaves those decoders' results as they are
    for a, b in zip(outs["others"], outs["all"]):
        for kind in (".ax25.json", ".pocsag.json"):
            assert a.with_name(a.stem + kind).read_bytes() == b.with_name(b.stem + kind).read_bytes()
    packets = json.loads(outs["all"][1].with_name(outs["all"][1].stem + ".ax25.json").read_text())
    assert [f["source"] for f in packets["frames"]] == ["N0CALL-7"] * 3


def test_pipeline_surface(A, tmp_path, monkeypatch):
    from iq_to_audio_amd import iqio
    from iq_to_audio_amd.batch import ResidentBankRunner

    fs, fc = 2.4e6, 455.5e6
    wav = tmp_path / "voice_455500000Hz.wav"
    iqio.write_wav_iq(wav, _capture(fs, 2.6), int(fs), "s16")

    def cfgs(tag):
        return [A.ProcessingConfig(in_path=wav, target_freq=f, demod_mode="nfm", chunk_size=65_536, output_path=tmp_path / f"{tag}{i}.wav")
                for i, f in enumerate((fc + 300e3, fc + 800e3))]

    calls = _count_calls(monkeypatch)

    def several_blocks(pipe):
        for o in getattr(pipe, "owners", [pipe]):
            o.block_frames_target = 1_048_576  # several device blocks: the carried history is exercised
        return pipe

    plain = several_blocks(A.MultiChannelPipeline(cfgs("p")))
    plain.run()
    assert calls == [] and plain.tones == [None, None]
    multi = several_blocks(A.MultiChannelPipeline(cfgs("m"), tones=True))
    multi.run()
    assert multi.tones[1] is None and multi.tones[0] is multi.owners[0].tones
    assert [e.tone_hz for e in multi.tones[0].ctcss] == [TONE] and [s.digits for s in multi.tones[0].sequences] == [DIGITS]
    assert calls.count("iqa_tones_decimate") >= 2 * 5 and calls.count("iqa_tones_bank") == 4 and calls.count("iqa_tones_decide") == 2
    one = A.ProcessingPipeline(cfgs("o")[0], tones=True)
    one.run()
    assert [e.tone_hz for e in one.tones.ctcss] == [TONE] and [s.digits for s in one.tones.sequences] == [DIGITS]
    for i in range(2):
        assert (tmp_path / f"p{i}.wav").read_bytes() == (tmp_path / f"m{i}.wav").read_bytes()
    with pytest.raises(ValueError, match="tones"):
        ResidentBankRunner([dict(freq_offset=300e3)], sample_rate=fs, n_frames=1 << 20, tones=True)
