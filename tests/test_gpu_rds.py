"""RDS beside wideband FM (--demod wfm --rds) on the MI355X: every stage against the float64 oracle of tests/rds_model.py,
block invariance, the CLI end to end on a capture with an RDS station, a pilot-less station and an NFM carrier, and the
proof that a run without --rds calls no RDS entry point."""
from __future__ import annotations

import importlib.util
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _load_model():
    name = "rds_model"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name("rds_model.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load_model()


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def rms(a):
    return float(np.sqrt(np.mean(np.abs(np.asarray(a).astype(np.complex128)) ** 2)))


def test_stages_against_the_oracle(A):
    """Measured on an MI355X: y 2.1e-7 RMS / 9.5e-7 max of rms(y); q within 2.0e-7 rad of the
    oracle's dev.  The bounds are the issue's (1e-5 / 1e-4 of rms(y), 1e-4 rad), not these."""
    from iq_to_audio_amd.decoders.rds import RdsDecoder, parse_groups

    fs = 480_000.0
    m, sent = M.multiplex(fs, 2.0, ppm=30.0, sigma=0.01, seed=5)
    theta = M.theta_of(m, fs)
    want = M.oracle_baseband(theta, fs)
    plan = want["plan"]
    dec = RdsDecoder(fs)
    dec.process(theta)
    st = dec.stages()
    j0 = plan.j0
    assert st["y"].shape == want["y"].shape and st["y"].dtype == np.complex64
    scale = rms(want["y"][j0:])
    err = st["y"][j0:].astype(np.complex128) - want["y"][j0:]
    print(f"y: rms(y) {scale:.4e}, error rms {rms(err) / scale:.3e} max {np.abs(err).max() / scale:.3e} (of rms(y))")
    dq = st["q"][j0:].astype(np.float64) * (2.0 * np.pi * 2.0 ** -44) - want["dev"][j0:]
    print(f"q: max |q 2 pi 2^-44 - dev| {np.abs(dq).max():.3e} rad, rms {rms(dq):.3e}")
    assert rms(err) <= 1e-5 * scale and np.abs(err).max() <= 1e-4 * scale, (rms(err) / scale, np.abs(err).max() / scale)
    assert st["q"].dtype == np.int64 and st["q"][0] == 0
    assert np.abs(dq).max() <= 1e-4, np.abs(dq).max()
    # the clock: exact on the GPU's own q
    phi, psi = M.oracle_clock(st["q"], plan)
    np.testing.assert_array_equal(st["phi"], phi)
    np.testing.assert_allclose(st["psi"], psi, rtol=0, atol=1e-10)
    # timing, symbols, bits, words, syndromes, groups: the oracle on its own y and clock
    full = M.oracle_chain(theta, fs)
    print(f"tau {st['tau']:+.6f} (oracle {full['tau']:+.6f}), strength {st['strength']:.4f} (oracle {full['strength']:.4f})")
    assert abs(st["tau"] - full["tau"]) < 1e-4 and abs(st["strength"] - full["strength"]) < 1e-4
    assert st["k_first"] == full["k_first"] and st["symbols"].size == full["symbols"].size
    serr = st["symbols"].astype(np.complex128) - full["symbols"]
    assert rms(serr) < 1e-3 * rms(full["symbols"])
    np.testing.assert_array_equal(st["bits"], full["bits"])
    np.testing.assert_array_equal(st["words"], full["words"])
    np.testing.assert_array_equal(st["syndromes"], full["syndromes"])
    got, ref = dec.finish(), parse_groups(full["words"], full["syndromes"])
    assert got is not None and got.group_offsets == ref.group_offsets and got.groups >= len(sent) - 3
    assert (got.pi, got.ps, got.radiotext) == (ref.pi, ref.ps, ref.radiotext) == (M.PI, M.PS, M.RT_SHOWN)
    assert got.groups_by_type == ref.groups_by_type and got.bits == full["bits"].size
    off, errors = M.align(st["bits"], M.bits_of(M.schedule(len(sent) + 2)))
    assert errors == 0


@pytest.mark.parametrize("fs", [480_000.0, 240_000.0])
def test_block_invariance(A, fs):
    """One stream cut into uneven blocks (not multiples of R, one shorter than the carried history, one of a single
    sample) gives bit-identical y, q, Phi, psi, symbols and bits."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.decoders.rds import RdsDecoder

    m, _ = M.multiplex(fs, 1.0, ppm=-40.0, sigma=0.01, seed=9)
    theta = D.to_device(M.theta_of(m, fs), "float32")
    n = int(theta.numel())
    runs = []
    for cuts in ([0, n], [0, 100_003, 100_004, 101_000, 200_001, n], [0, 7, 2047, 2049, 4096 + 17, n - 30_000, n - 1, n]):
        dec = RdsDecoder(fs)
        assert len(cuts) == 2 or min(b - a for a, b in zip(cuts[:-1], cuts[1:])) < dec.plan.hist_len
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            dec.process(theta[lo:hi])
        runs.append(dec.stages())
    assert runs[0]["bits"].size > 1000
    for st in runs[1:]:
        for key in ("y", "q", "phi", "psi", "symbols", "bits", "words", "syndromes"):
            np.testing.assert_array_equal(st[key], runs[0][key], err_msg=key)
        assert st["tau"] == runs[0]["tau"] and st["k_first"] == runs[0]["k_first"]


def _capture(fs=2.4e6, secs=2.0, seed=11):
    """int16 I/Q: a stereo station with RDS at +300 kHz (10 % pilot 30 ppm high, L = 1 kHz, R = 2.5 kHz, 4 % RDS), a
    pilot-less mono station at -500 kHz (400 Hz), an NFM carrier at +800 kHz, complex noise 40 dB below a station."""
    n = int(round(fs * secs))
    t = np.arange(n, dtype=np.float64) / fs
    amp = 0.28
    m1, sent = M.multiplex(fs, secs, ppm=30.0)
    m2 = 0.5 * np.sin(2 * np.pi * 400.0 * t)
    k = 2 * np.pi * 75_000.0 / fs
    x = amp * np.exp(1j * (2 * np.pi * 300e3 * t + k * np.cumsum(m1)))
    x += amp * np.exp(1j * (-2 * np.pi * 500e3 * t + k * np.cumsum(m2)))
    x += amp * np.exp(1j * (2 * np.pi * 800e3 * t + 2 * np.pi * 5000.0 / fs * np.cumsum(np.sin(2 * np.pi * 1000.0 * t))))
    rng = np.random.default_rng(seed)
    std = amp * math.sqrt(1e-4 / 2.0)
    x += std * (rng.normal(size=n) + 1j * rng.normal(size=n))
    iq = np.column_stack((x.real, x.imag))
    return np.rint(np.clip(iq, -0.999, 0.999) * 32767.0).astype(np.int16), sent


def _count_rds_calls(monkeypatch):
    from iq_to_audio_amd import _native

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith("iqa_rds_"):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    return calls


def test_end_to_end_two_stations(A, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import cli, iqio

    fs, fc = 2.4e6, 100e6
    raw, sent = _capture(fs)
    outs = {}
    calls = _count_rds_calls(monkeypatch)
    for tag, extra in (("plain", []), ("rds", ["--rds"])):
        d = tmp_path / tag
        d.mkdir()
        wav = d / "fm_100000000Hz.wav"
        iqio.write_wav_iq(wav, raw, int(fs), "s16")
        assert cli.main(["--in", str(wav), "--ft", str(fc + 300e3), "--ft", str(fc - 500e3), "--demod", "wfm", *extra]) == 0
        outs[tag] = [d / f"audio_{int(fc + 300e3)}_48k.wav", d / f"audio_{int(fc - 500e3)}_48k.wav"]
        if tag == "plain":
            assert calls == []  # a run without --rds calls no RDS entry point
            assert not list(d.glob("*.rds.json"))
    assert {"iqa_rds_baseband", "iqa_rds_clock", "iqa_rds_timing", "iqa_rds_symbols", "iqa_rds_syndromes"} <= set(calls)
    for a, b in zip(outs["plain"], outs["rds"]):
        assert a.read_bytes() == b.read_bytes()  # the audio does not change
    printed = capsys.readouterr().out
    assert f'PI=54A8 PS="{M.PS}" RT="{M.RT_SHOWN}"' in printed and "no RDS" in printed
    js = json.loads(outs["rds"][0].with_name(outs["rds"][0].stem + ".rds.json").read_text())
    print("station:", js)
    assert (js["pi"], js["ps"], js["radiotext"]) == (M.PI, M.PS, M.RT_SHOWN)
    assert js["groups"] >= len(sent) - 3 and len(sent) >= 20, (js["groups"], len(sent))
    assert js["tp"] is True and js["pty"] == 10 and set(js["groups_by_type"]) == {"0A", "2A", "4A", "14A"}
    assert js["timing"]["strength"] > 0.1
    assert json.loads(outs["rds"][1].with_name(outs["rds"][1].stem + ".rds.json").read_text()) is None


def test_pipeline_surface_and_no_rds_calls_without_rds(A, tmp_path, monkeypatch):
    from iq_to_audio_amd import iqio

    fs, fc = 2.4e6, 100e6
    raw, sent = _capture(fs, 1.2, seed=3)
    wav = tmp_path / "fm_100000000Hz.wav"
    iqio.write_wav_iq(wav, raw, int(fs), "s16")

    def cfgs(tag):
        return [A.ProcessingConfig(in_path=wav, target_freq=f, demod_mode="wfm", bandwidth=250_000.0, fs_ch_target=480_000.0,
                                   deemph_us=50.0, chunk_size=65_536, output_path=tmp_path / f"{tag}{i}.wav")
                for i, f in enumerate((fc + 300e3, fc - 500e3))]

    calls = _count_rds_calls(monkeypatch)
    plain = A.MultiChannelPipeline(cfgs("p"))
    plain.run()
    assert calls == [] and plain.rds == [None, None] and plain.wfm_stereo == [True, False]
    single = A.ProcessingPipeline(cfgs("s")[0])
    single.run()
    assert calls == [] and single.rds is None
    multi = A.MultiChannelPipeline(cfgs("m"), rds=True)
    multi.run()
    assert multi.wfm_stereo == [True, False] and multi.rds[1] is None and multi.owners[1].rds is None
    res = multi.rds[0]
    assert res is multi.owners[0].rds and (res.pi, res.ps, res.radiotext) == (M.PI, M.PS, M.RT_SHOWN)
    assert res.groups >= len(sent) - 3
    assert calls.count("iqa_rds_timing") == 1  # the pilot-less target decodes nothing at the end
    for i in range(2):
        assert (tmp_path / f"p{i}.wav").read_bytes() == (tmp_path / f"m{i}.wav").read_bytes()
    one = A.ProcessingPipeline(cfgs("o")[0], rds=True)
    one.run()
    assert one.rds.group_offsets == res.group_offsets and one.rds.ps == M.PS
