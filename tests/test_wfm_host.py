"""Wideband FM stereo (--demod wfm), the host side: the filter plan against its specification, the decoder factory, CLI
default resolution, validation, the batch runners' refusal, the C ABI's argument checks -- and the float64 numpy oracle of
the whole chain that tests/test_gpu_wfm.py compares the GPU with.  No GPU compute here."""
from __future__ import annotations

import ctypes
import math
from ctypes import c_float, c_int32, c_int64, c_void_p

import numpy as np
import pytest

import iq_to_audio_amd as A
from iq_to_audio_amd import dsp_plan as P
from iq_to_audio_amd import iqio
from oracle import cpu_ref as O


# ---- the float64 oracle of the chain (steps 1-6 of the specification) --------------------------------------------------


def wfm_oracle(z: np.ndarray, fs: float, deemph_us: float = 50.0) -> dict:
    """float64 numpy statement of the wfm chain on the channelizer output ``z`` (complex64) at channel rate ``fs``:
    composite, pilot, stereo matrix, the per-run stereo decision, de-emphasis, clip, 48 kHz resampler."""
    plan = P.plan_wfm(fs)
    n, d = z.size, plan.delay
    m = O.quadrature(np.asarray(z, dtype=np.complex64), O.QuadState()).astype(np.float64) * fs / (2.0 * math.pi * P.WFM_DEVIATION)
    p = np.convolve(m, plan.h_pilot)[:n]
    mag2 = np.abs(p) ** 2
    u2 = np.where(mag2 > 0, p * p / np.where(mag2 > 0, mag2, 1.0), 0.0)
    c = np.where(np.abs(p) < 1e-12, 0.0, -np.imag(u2))
    md = np.concatenate([np.zeros(d), m[: n - d]]) if n > d else np.zeros(n)
    a = np.convolve(md, plan.h_audio)[:n]
    b = np.convolve(2.0 * md * c, plan.h_audio)[:n]
    level = math.sqrt(float(np.mean(mag2))) if n else 0.0
    stereo = level >= P.WFM_STEREO_LEVEL
    chans = [a + b, a - b] if stereo else [a]
    alpha = O.deemph_alpha(deemph_us, fs)
    deemph, clipped, audio48, peak = [], [], [], 0.0
    for x in chans:
        y = O.deemphasis(x.astype(np.float32), O.DeemphState(alpha))
        deemph.append(y)
        yc, peak = O.writer_clip(y, peak)
        clipped.append(yc)
        audio48.append(O.resample_48k(yc, fs))
    return dict(m=m, p=p, c=c, a=a, b=b, left=a + b, right=a - b, level=level, stereo=stereo, deemph=deemph, clipped=clipped,
                audio48=audio48, peak=peak, plan=plan)


def multiplex(fs: float, seconds: float, left, right, pilot: float = 0.1, g: float = 0.9) -> np.ndarray:
    """Composite of a standard stereo multiplex: g/2 (L+R) + g/2 (L-R) sin 2 theta + pilot sin theta, theta = 2 pi 19 kHz t
    (``left`` / ``right``: functions of t in seconds)."""
    t = np.arange(int(round(fs * seconds)), dtype=np.float64) / fs
    th = 2.0 * math.pi * P.WFM_PILOT_HZ * t
    lv, rv = left(t), right(t)
    return 0.5 * g * (lv + rv) + 0.5 * g * (lv - rv) * np.sin(2.0 * th) + pilot * np.sin(th)


def fm_modulate(m: np.ndarray, fs: float) -> np.ndarray:
    """Baseband FM of the composite at 75 kHz deviation per unit (phase accumulated in float64), complex64."""
    return np.exp(1j * 2.0 * math.pi * P.WFM_DEVIATION / fs * np.cumsum(m)).astype(np.complex64)


def test_oracle_against_a_hand_computed_case():
    """Constant L = 0.5, R = 0.1 with a 10 % pilot: the matrix gives a = g/2 (L+R) = 0.27, b = g/2 (L-R) = 0.18, the pilot
    level reads a_p / 2 = 0.05 (stereo), and after the filters' start-up L, R come out as g L, g R -- also through the
    de-emphasis (unit gain at DC), the clip and the 48 kHz resampler."""
    fs = 480_000.0
    m = multiplex(fs, 0.1, lambda t: 0.5 + 0 * t, lambda t: 0.1 + 0 * t)
    w = wfm_oracle(fs_modulate := fm_modulate(m, fs), fs)
    assert fs_modulate.dtype == np.complex64
    np.testing.assert_allclose(w["m"], m, atol=2e-6)  # the discriminator recovers the composite (float32 angle)
    tail = slice(2 * (w["plan"].ntaps - 1), None)
    np.testing.assert_allclose(w["a"][tail], 0.27, atol=2e-3)
    np.testing.assert_allclose(w["b"][tail], 0.18, atol=2e-3)
    np.testing.assert_allclose(w["left"][tail], 0.45, atol=3e-3)
    np.testing.assert_allclose(w["right"][tail], 0.09, atol=3e-3)
    assert w["stereo"] and abs(w["level"] - 0.05) < 0.005
    np.testing.assert_allclose(np.abs(w["p"][tail]), 0.05, atol=1e-3)
    settled = slice(int(0.05 * 48_000), int(0.09 * 48_000))
    np.testing.assert_allclose(w["audio48"][0][settled], 0.45, atol=3e-3)
    np.testing.assert_allclose(w["audio48"][1][settled], 0.09, atol=3e-3)
    # the same programme without its pilot is mono: one channel, a = g/2 (L+R)
    w0 = wfm_oracle(fm_modulate(multiplex(fs, 0.1, lambda t: 0.5 + 0 * t, lambda t: 0.1 + 0 * t, pilot=0.0), fs), fs)
    assert not w0["stereo"] and len(w0["audio48"]) == 1 and w0["level"] < 1e-3
    np.testing.assert_allclose(w0["audio48"][0][settled], 0.27, atol=3e-3)


# ---- the filter plan -------------------------------------------------------------------------------------------------


def _response_db(h: np.ndarray, fs: float, nfft: int = 1 << 20):
    """(frequencies in Hz, -fs/2 .. fs/2, and |H| in dB) of a (complex) FIR."""
    H = np.fft.fftshift(np.fft.fft(h, nfft))
    f = np.fft.fftshift(np.fft.fftfreq(nfft, 1.0 / fs))
    return f, 20.0 * np.log10(np.maximum(np.abs(H), 1e-300))


@pytest.mark.parametrize("fs,ntaps", [(240_000.0, 347), (480_000.0, 693), (10e6 / 21, 687), (128_000.0, 185)])
def test_filter_plan_meets_its_specification(fs, ntaps):
    plan = P.plan_wfm(fs)
    assert plan.ntaps == ntaps == P.wfm_num_taps(fs) and ntaps % 2 == 1 and plan.delay == (ntaps - 1) // 2
    h_a, h_p = plan.h_audio, plan.h_pilot
    np.testing.assert_allclose(h_a, h_a[::-1], rtol=0, atol=1e-18)
    np.testing.assert_allclose(h_p, np.conj(h_p[::-1]), rtol=0, atol=1e-16)
    assert abs(h_a.sum() - 1.0) < 1e-12
    lp = h_p * np.exp(-2j * np.pi * P.WFM_PILOT_HZ * (np.arange(ntaps) - plan.delay) / fs)
    assert abs(lp.real.sum() - 1.0) < 1e-12 and np.abs(lp.imag).max() < 1e-12
    f, ha_db = _response_db(h_a, fs)
    assert ha_db[np.abs(f) >= 19_000.0].max() <= -70.0
    assert np.abs(ha_db[np.abs(f) < 15_000.0]).max() <= 0.1
    f, hp_db = _response_db(h_p, fs)
    k19 = int(np.argmin(np.abs(f - 19_000.0)))
    assert abs(10.0 ** (hp_db[k19] / 20.0) - 1.0) <= 1e-3
    assert hp_db[(f <= 15_000.0) | (f >= 23_000.0)].max() <= -70.0
    assert abs(plan.m_scale - fs / (2 * math.pi * 75_000.0)) < 1e-6 * plan.m_scale
    d = plan.delay
    np.testing.assert_array_equal(plan.taps_packed, np.concatenate([h_a[: d + 1], h_p.real[: d + 1], h_p.imag[: d + 1]]).astype(np.float32))


def test_filter_plan_rejects_rates_outside_the_mode():
    for fs in (96_000.0, 127_999.0):
        with pytest.raises(ValueError):
            P.plan_wfm(fs)
    P.plan_wfm(128_000.0)
    with pytest.raises(ValueError):
        P.plan_wfm(2_000_000.0)  # more taps than the kernel holds


# ---- factory, CLI, validation ------------------------------------------------------------------------------------------


def test_create_decoder_wfm():
    from iq_to_audio_amd.decoders import GpuDecoder, WidebandFMDecoder

    dec = A.create_decoder("wfm", deemph_us=50.0, agc_enabled=True, extensions=True)
    assert isinstance(dec, WidebandFMDecoder) and isinstance(dec, GpuDecoder)
    assert isinstance(A.create_decoder("WFM", deemph_us=75.0, agc_enabled=False, extensions=True), WidebandFMDecoder)
    assert dec.name == "wideband_fm" and dec.deemph_us == 50.0
    with pytest.raises(NotImplementedError):
        dec.fused_params()  # no form on the fused iqa_demodulate engine
    with pytest.raises(RuntimeError):
        dec.process(np.ones(4, dtype=np.complex64))  # setup() not called
    with pytest.raises(ValueError):
        dec.setup(96_000.0)  # below the mode's minimum channel rate (plan_wfm, before any device work)
    # the reference-parity factory keeps the reference's mode set: wfm is an extension the caller asks for
    with pytest.raises(ValueError, match="extensions=True"):
        A.create_decoder("wfm", deemph_us=50.0, agc_enabled=True)
    with pytest.raises(ValueError):
        A.create_decoder("dsb", deemph_us=50.0, agc_enabled=True, extensions=True)
    from iq_to_audio_amd.decoders import NarrowbandFMDecoder

    assert isinstance(A.create_decoder("fm", deemph_us=300.0, agc_enabled=True, extensions=True), NarrowbandFMDecoder)


def test_cli_defaults_resolve_by_mode():
    from iq_to_audio_amd import cli

    p = cli.build_parser()

    def resolved(*extra):
        a = cli.resolve_mode_defaults(p.parse_args(["--in", "x.wav", "--ft", "100e6", *extra]))
        return a.bandwidth, a.fs_ch, a.deemph_us

    assert resolved("--demod", "wfm") == (250_000.0, 480_000.0, 50.0)
    assert resolved("--demod", "wfm", "--deemph", "75") == (250_000.0, 480_000.0, 75.0)
    assert resolved("--demod", "wfm", "--bw", "200000", "--fs-ch", "240000") == (200_000.0, 240_000.0, 50.0)
    for mode in ("nfm", "am", "usb", "lsb", "ssb", "none"):
        assert resolved("--demod", mode) == (12_500.0, 96_000.0, 300.0)
    assert resolved() == (12_500.0, 96_000.0, 300.0)
    assert resolved("--demod", "am", "--bw", "250000", "--deemph", "50") == (250_000.0, 96_000.0, 50.0)
    for v in resolved("--demod", "nfm"):
        assert type(v) is float


def _tiny_capture(tmp_path, fs=2.4e6, secs=0.01):
    wav = tmp_path / "cap_100000000Hz.wav"
    n = int(fs * secs)
    iqio.write_wav_iq(wav, np.zeros(2 * n, dtype=np.int16), int(fs), "s16")
    return wav


def test_wfm_channel_rate_below_the_minimum_is_rejected_before_any_launch(tmp_path):
    wav = _tiny_capture(tmp_path)
    cfg = A.ProcessingConfig(in_path=wav, target_freq=100.3e6, demod_mode="wfm", bandwidth=250_000.0, fs_ch_target=96_000.0,
                             deemph_us=50.0, output_path=tmp_path / "o.wav")
    with pytest.raises(ValueError, match="wfm"):
        A.ProcessingPipeline(cfg).run()
    with pytest.raises(ValueError, match="wfm"):
        A.MultiChannelPipeline([cfg]).run()
    assert not (tmp_path / "o.wav").exists()


def test_processing_config_keeps_its_fields():
    import dataclasses

    assert len(dataclasses.fields(A.ProcessingConfig)) == 23


def test_batch_runners_reject_wfm():
    from iq_to_audio_amd import batch

    taps = P.design_channel_filter(2.4e6, 250_000.0, 5)
    with pytest.raises(ValueError, match="wfm"):
        batch.ResidentCaptureRunner(taps, sample_rate=2.4e6, freq_offset=3e5, decimation=5, fs_channel=480e3, chunk=1 << 20,
                                    n_frames=1 << 20, demod_mode="wfm")
    with pytest.raises(ValueError, match="wfm"):
        batch.ResidentBankRunner([dict(freq_offset=3e5), dict(freq_offset=-5e5, demod_mode="wfm")], sample_rate=2.4e6,
                                 n_frames=1 << 20)
    with pytest.raises(ValueError, match="wfm"):
        batch.demodulate_sharded([dict(freq_offset=3e5, demod_mode="wfm")], sample_rate=2.4e6, n_frames=1 << 20, axis="channels")


def test_abi_entries_reject_bad_arguments_without_a_gpu():
    lib = A.native.lib()
    assert lib.iqa_wfm_partials(0) == 0 and lib.iqa_wfm_partials(2048) == 1 and lib.iqa_wfm_partials(2049) == 2
    buf = (ctypes.c_float * 16)()
    ok = ctypes.cast(buf, c_void_p)
    null = c_void_p(0)

    def stereo(ntaps, n, taps=ok, theta=ok, a=ok, b=ok, scale=1.0):
        A.native.call("iqa_wfm_stereo", c_int32(ntaps), taps, c_float(scale), theta, c_int64(n), null, null, a, b, null, null)

    for bad in (0, 1, 2, 692, P.WFM_MAX_TAPS + 2, -5):
        with pytest.raises(ValueError):
            stereo(bad, 8)
        assert "ntaps" in lib.iqa_last_error().decode()
    with pytest.raises(ValueError):
        stereo(693, -1)
    assert "negative" in lib.iqa_last_error().decode()
    for kw in ("taps", "theta", "a", "b"):
        with pytest.raises(ValueError):
            stereo(693, 8, **{kw: null})
        assert "NULL" in lib.iqa_last_error().decode()
    with pytest.raises(ValueError):
        stereo(693, 8, scale=float("nan"))
    with pytest.raises(ValueError):
        A.native.call("iqa_wfm_matrix", null, ok, c_int64(4), ok, ok, null)
    with pytest.raises(ValueError):
        A.native.call("iqa_wfm_matrix", ok, ok, c_int64(-1), ok, ok, null)
    # the 48 kHz resampler takes the long rows of wfm channel rates; the limit moved, the checks stay
    with pytest.raises(ValueError):
        A.native.call("iqa_resample", ok, c_int64(8), null, c_int32(1), c_int32(10), c_int32(160), c_int64(0), c_int64(1), ok, null, null)
    with pytest.raises(ValueError):
        A.native.call("iqa_resample", ok, c_int64(8), ok, c_int32(1), c_int32(10), c_int32(2049), c_int64(0), c_int64(1), ok, null, null)
    assert "4097" in lib.iqa_last_error().decode()
