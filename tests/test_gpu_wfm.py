"""Wideband FM stereo (--demod wfm) on the MI355X: the stage API against the float64 oracle of tests/test_wfm_host.py,
block invariance of the stereo matrix kernel, the CLI end to end on a capture with a stereo station, a mono station and an
NFM carrier, the channelizer at the mode's shapes, and the long-row 48 kHz resampler."""
from __future__ import annotations

import importlib.util
import math
import wave
from pathlib import Path

import numpy as np
import pytest
import resampler_model as RM

from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("wfm_host_oracle", Path(__file__).with_name("test_wfm_host.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)) ** 2)))


def _stereo_z(fs, secs, seed=5, snr_db=40.0):
    m = H.multiplex(fs, secs, lambda t: 0.5 * np.sin(2 * np.pi * 1000.0 * t), lambda t: 0.5 * np.sin(2 * np.pi * 2500.0 * t))
    z = H.fm_modulate(m, fs).astype(np.complex128)
    rng = np.random.default_rng(seed)
    std = math.sqrt(10.0 ** (-snr_db / 10.0) / 2.0)
    return (z + std * (rng.normal(size=z.size) + 1j * rng.normal(size=z.size))).astype(np.complex64)


def test_stages_against_the_oracle(A):
    fs = 480_000.0
    z = _stereo_z(fs, 1.0)
    want = H.wfm_oracle(z, fs, 50.0)
    dec = A.create_decoder("wfm", deemph_us=50.0, agc_enabled=False, extensions=True)
    dec.setup(fs)
    audio, stats = dec.process(z)
    st = dec.intermediates()
    assert [k for k in st] == ["demod", "mono", "stereo_diff", "left", "right", "audio"]
    skip = 2 * (want["plan"].ntaps - 1)
    for name, key in (("demod", "m"), ("mono", "a"), ("stereo_diff", "b"), ("left", "left"), ("right", "right")):
        got, ref = st[name][0].astype(np.float64), want[key]
        assert got.shape == ref.shape, name
        err = got[skip:] - ref[skip:]
        assert rms(err) <= 1e-5 and np.abs(err).max() <= 1e-4, (name, rms(err), np.abs(err).max())
        assert st[name][1] == fs
    assert dec.stereo and want["stereo"] and abs(dec.pilot_level - want["level"]) < 1e-4 * want["level"] + 1e-6
    assert audio.shape == (z.size, 2) and audio.dtype == np.float32
    for ch in range(2):
        err = audio[skip:, ch].astype(np.float64) - want["deemph"][ch][skip:]
        assert rms(err) <= 1e-5, (ch, rms(err))
    assert np.isfinite(stats.rms_dbfs)
    # a call without a pilot is mono: (n,) audio
    mono = A.create_decoder("wfm", deemph_us=50.0, agc_enabled=False, extensions=True)
    mono.setup(fs)
    zm = H.fm_modulate(0.5 * np.sin(2 * np.pi * 400.0 * np.arange(48_000) / fs), fs)
    out, _ = mono.process(zm)
    assert out.shape == (zm.size,) and not mono.stereo


def test_block_invariance(A):
    """The stereo matrix kernel's outputs do not depend on where a stream is cut into blocks: bit-identical planes."""
    import torch

    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.processing import WfmDemod

    fs = 480_000.0
    z = D.to_device(_stereo_z(fs, 1.0, seed=9), "complex64")
    n = int(z.numel())
    runs = []
    for cuts in ([0, n], [0, 100_003, 100_004, 300_001, n], [0, 2047, 2049, 4096 + 17, 470_000, n]):
        dem = WfmDemod(fs, deemph_us=50.0)
        planes = torch.empty((2, n), dtype=torch.float32, device=D.device())
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            dem.process(z[lo:hi], np.array([0], dtype=np.int64), planes[:, lo:hi])
        pcm, ch = dem.finish(planes)
        runs.append((planes.cpu().numpy(), pcm, ch, dem.stereo, torch.stack(dem.channel_audio).cpu().numpy()))
    for planes, pcm, ch, stereo, chan in runs[1:]:
        np.testing.assert_array_equal(planes, runs[0][0])
        assert ch == 2 and stereo and runs[0][3]
        np.testing.assert_array_equal(pcm, runs[0][1])
        np.testing.assert_allclose(chan, runs[0][4], rtol=0, atol=1e-6)


def _capture(fs=2.4e6, secs=1.5, seed=11):
    """int16 I/Q: a stereo station at +300 kHz (10 % pilot, L = 1 kHz, R = 2.5 kHz), a pilot-less mono station at -500 kHz
    (400 Hz), an NFM carrier at +800 kHz, complex noise 40 dB below a station."""
    n = int(round(fs * secs))
    t = np.arange(n, dtype=np.float64) / fs
    amp = 0.28
    m1 = H.multiplex(fs, secs, lambda t: 0.5 * np.sin(2 * np.pi * 1000.0 * t), lambda t: 0.5 * np.sin(2 * np.pi * 2500.0 * t))
    m2 = 0.5 * np.sin(2 * np.pi * 400.0 * t)
    k = 2 * np.pi * 75_000.0 / fs
    x = amp * np.exp(1j * (2 * np.pi * 300e3 * t + k * np.cumsum(m1)))
    x += amp * np.exp(1j * (-2 * np.pi * 500e3 * t + k * np.cumsum(m2)))
    x += amp * np.exp(1j * (2 * np.pi * 800e3 * t + 2 * np.pi * 5000.0 / fs * np.cumsum(np.sin(2 * np.pi * 1000.0 * t))))
    rng = np.random.default_rng(seed)
    std = amp * math.sqrt(1e-4 / 2.0)
    x += std * (rng.normal(size=n) + 1j * rng.normal(size=n))
    iq = np.column_stack((x.real, x.imag))
    return np.rint(np.clip(iq, -0.999, 0.999) * 32767.0).astype(np.int16)


def _read_wav(path):
    with wave.open(str(path), "rb") as w:
        ch, rate, frames = w.getnchannels(), w.getframerate(), w.readframes(w.getnframes())
    return np.frombuffer(frames, dtype="<i2").reshape(-1, ch), rate


def _tone_amp(y, f, rate=48_000):
    t = np.arange(y.size) / rate
    return 2.0 * abs(np.sum(y * np.exp(-2j * np.pi * f * t))) / y.size


def test_end_to_end_two_stations(A, tmp_path):
    from iq_to_audio_amd import cli, iqio

    fs, fc = 2.4e6, 100e6
    raw = _capture(fs)
    wav = tmp_path / "fm_100000000Hz.wav"
    iqio.write_wav_iq(wav, raw, int(fs), "s16")
    assert cli.main(["--in", str(wav), "--ft", str(fc + 300e3), "--ft", str(fc - 500e3), "--demod", "wfm"]) == 0
    out1, out2 = tmp_path / f"audio_{int(fc + 300e3)}_48k.wav", tmp_path / f"audio_{int(fc - 500e3)}_48k.wav"
    pcm1, r1 = _read_wav(out1)
    pcm2, r2 = _read_wav(out2)
    assert (r1, r2) == (48_000, 48_000) and pcm1.shape[1] == 2 and pcm2.shape[1] == 1
    y1 = pcm1.astype(np.float64) / 32768.0
    win = slice(24_000, 24_000 + 43_200)  # 0.5 .. 1.4 s: whole cycles of both tones
    left, right = y1[win, 0], y1[win, 1]
    sep_l = 20 * math.log10(_tone_amp(left, 1000.0) / _tone_amp(left, 2500.0))
    sep_r = 20 * math.log10(_tone_amp(right, 2500.0) / _tone_amp(right, 1000.0))
    assert sep_l >= 35.0 and sep_r >= 35.0, (sep_l, sep_r)
    y2 = pcm2[:, 0].astype(np.float64) / 32768.0
    assert _tone_amp(y2[win], 400.0) > 0.2 and _tone_amp(y2[win], 400.0) > 100 * _tone_amp(y2[win], 1000.0)

    # the same capture through MultiChannelPipeline: the stereo decisions, and z for the oracle
    cfgs = [A.ProcessingConfig(in_path=wav, target_freq=f, demod_mode="wfm", bandwidth=250_000.0, fs_ch_target=480_000.0,
                               deemph_us=50.0, output_path=tmp_path / f"mc{i}.wav", dump_iq_path=tmp_path / f"z{i}.c64")
            for i, f in enumerate((fc + 300e3, fc - 500e3))]
    multi = A.MultiChannelPipeline(cfgs)
    res = multi.run()
    assert multi.wfm_stereo == [True, False]
    assert [o.wfm_stereo for o in multi.owners] == [True, False]
    for i, (r, pcm) in enumerate(zip(res, (pcm1, pcm2))):
        z = np.fromfile(tmp_path / f"z{i}.c64", dtype=np.complex64)
        want = H.wfm_oracle(z, r.fs_channel, 50.0)
        assert want["stereo"] == (i == 0)
        got = pcm.astype(np.float64) / 32768.0
        skip = 480  # 10 ms
        for ch in range(got.shape[1]):
            ref = want["audio48"][ch]
            assert ref.size == got.shape[0]
            assert rms(got[skip:, ch] - ref[skip:]) < 1e-4, (i, ch, rms(got[skip:, ch] - ref[skip:]))
        assert abs(r.audio_peak - want["peak"]) < 1e-4
        np.testing.assert_array_equal(_read_wav(tmp_path / f"mc{i}.wav")[0], pcm)


def test_pipeline_outputs_do_not_depend_on_the_chunk(A, tmp_path):
    from iq_to_audio_amd import iqio

    fs, fc = 2.4e6, 100e6
    wav = tmp_path / "fm_100000000Hz.wav"
    iqio.write_wav_iq(wav, _capture(fs, 0.8, seed=3), int(fs), "s16")
    outs = []
    for chunk in (65_536, 1_048_576):
        cfg = A.ProcessingConfig(in_path=wav, target_freq=fc + 300e3, demod_mode="wfm", bandwidth=250_000.0,
                                 fs_ch_target=480_000.0, deemph_us=50.0, chunk_size=chunk, output_path=tmp_path / f"o{chunk}.wav")
        pipe = A.ProcessingPipeline(cfg)
        pipe.keep_channel_audio = True
        pipe.run()
        assert pipe.wfm_stereo is True and pipe.audio_fs_channel.shape[0] == 2
        outs.append((pipe.wfm_planes.cpu().numpy(), pipe.audio_fs_channel.cpu().numpy()))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_allclose(outs[0][1], outs[1][1], rtol=0, atol=1e-6)


@pytest.mark.parametrize("fs,d", [(2.4e6, 5), (10e6, 21)])
def test_channelizer_at_the_mode_shapes(A, fs, d):
    from iq_to_audio_amd import dsp_plan as P

    assert P.choose_decimation(fs, 480_000.0)[0] == d
    rng = np.random.default_rng(4)
    n = 400_000
    raw = rng.integers(-12000, 12000, size=2 * n).astype(np.int16)
    f_off = 300e3
    tone = 8000 * np.exp(2j * np.pi * (f_off + 15_000.0) / fs * np.arange(n))
    raw[0::2] += np.rint(tone.real).astype(np.int16)
    raw[1::2] += np.rint(tone.imag).astype(np.int16)
    taps = A.design_channel_filter(fs, 250_000.0, d)
    assert taps.size == 1025
    x = O.ingest_to_complex64(raw, "s16")
    want = O.decimate(O.overlap_save(O.nco_mix(x, O.NcoState(f_off, fs), 1), O.OverlapSaveState(taps, 65536)), O.DecimState(d))
    assert rms(want) > 0.05
    wideband = rms(x)
    for precision in ("full", "fast"):
        ch = A.Channelizer(taps, sample_rate=fs, freq_offset=f_off, mix_sign=1, decimation=d, precision=precision)
        got = np.concatenate([ch.process(raw[: 2 * 150_001]), ch.process(raw[2 * 150_001 :])])
        assert got.shape == want.shape
        if precision == "full":  # the existing parity bar: z error below float32 rounding
            assert rms(got - want) < 2e-6, (precision, rms(got - want))
        else:  # the fixed-point error this shape's int8 taps are planned for (x5: tonal captures)
            bound = ch._kernel.fixed_point_error_rms(wideband)
            assert rms(got - want) < max(2e-6, 5.0 * bound), (precision, rms(got - want), bound)


@pytest.mark.parametrize("fs_ch", [480_000.0, 10e6 / 21, 300_000.0])
def test_long_row_resampler_matches_spec(A, fs_ch):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.processing import Resampler48k

    rs = Resampler48k(fs_ch)
    assert 2 * rs.plan.half_taps + 1 > 192  # the direct kernel
    x = (0.5 * np.sin(2 * np.pi * 1234.5 * np.arange(200_003) / fs_ch)
         + np.random.default_rng(1).normal(scale=0.05, size=200_003)).astype(np.float32)
    y, pcm = rs.process(D.to_device(x, "float32"), want="both")
    assert y.numel() == O.resample_48k(x, fs_ch).size
    RM.check(y.cpu().numpy(), *RM.y64(x, fs_ch))
    np.testing.assert_array_equal(pcm.cpu().numpy(), O.float_to_pcm16(y.cpu().numpy()))
