"""The fixed-point channelizers' error model and the precision guard on quiet data, by exact integer emulation (no GPU).

``MfmaPlan.z_error_rms`` predicts the z error of the int8 matrix-core kernels, ``precision.pick_precision`` relies on it
to keep NFM audio within 1e-4 RMS of the float64 chain.  The level-independent part of that error is the (low tap byte)
x (low data byte) products the int16 kernels drop; its RMS was modelled for uniform low bytes only.  Here the exact model
(oracle/mfma_model.py, through ``test_host_logic._emulate_mfma_outputs``) runs on the captures that are NOT of that class
-- silence, a DC offset, noise of one LSB, a clean NFM signal a few dozen LSB tall alone in the capture, the quiet half of
a gated full-scale tone -- and on the ones that are, per plan: 10 MS/s D = 104 with the 12.5 kHz filter at offset 0,
+1.0 MHz and +1.3 MHz, and 20 MS/s D = 208 with the 2.8 kHz filter (three tap-row groups) at offset 0; "fast" and "fine";
2000 consecutive outputs against a float64 FFT convolution with the unquantised taps.  A fifth plan, 50 MS/s D = 521 at
+2.2 MHz (three chained k-step ranges), runs a few of the captures: its zero-input response (8.4e-7) lies below its uniform
floor (1.86e-6), so there the coherent bound alone stands between a 64 LSB signal and "fast" (1.3e-4 off).

Figures of the exact model, D = 104 at offset 0, "fast" (plan: err_norm 1.94e-6, floor_rms 1.40e-6, zero_rms 2.49e-5,
coherent_rms 2.24e-5): z error 2.49e-5 on zeros (a constant), 9.8e-6 on 1 LSB of noise, 2.4e-5 on DC +-3 LSB, 2.0e-6 /
1.4e-6 / 1.4e-6 on 30 / 300 / 3000 LSB of noise; NFM audio at "fast" 2.2e-4, 1.9e-4, 1.3e-4, 9.3e-5, 6.2e-5, 2.7e-5, 5.4e-6
RMS off the float64 chain at 46, 50, 64, 80, 100, 200, 1000 LSB, ~1e-6 at "fine".  D = 208 at offset 0 (the signal's phase
stands still against a filter of 32769 taps twice per modulation cycle): "fast" is 3.5e-4 off at 200 LSB, 5.9e-5 at 1000.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import pytest

from iq_to_audio_amd import dsp_plan as P
from iq_to_audio_amd import precision as PR
from oracle import cpu_ref as O
from oracle import mfma_model as M
from test_host_logic import _emulate_mfma_outputs

N_OUT = 2000
SETTLE = 200  # outputs the discriminator and the de-emphasis take to forget their initial state
AUDIO_BAR = 1e-4  # the project's audio bar: what ``pick_precision`` promises to keep

PLANS = {  # name -> (fs, bandwidth, D, offset)
    "d104-0Hz": (10e6, 12_500.0, 104, 0.0),
    "d208-2k8-0Hz": (20e6, 2_800.0, 208, 0.0),
    "d104+1.0MHz": (10e6, 12_500.0, 104, 1.0e6),
    "d104+1.3MHz": (10e6, 12_500.0, 104, 1.3e6),
    "d521+2.2MHz": (50e6, 12_500.0, 521, 2.2e6),
}
PLAN_KW = {"fast": dict(acc32=True), "fine": dict(acc32=True, residual=True), "full": dict(acc32=False, residual=True)}
FLAT = ["zeros", "dc3", "noise1", "noise30", "noise300", "noise3000", "gated-tone"]  # held to 2x the prediction
NFM = [f"nfm{a}-noise{n}" for a in (46, 50, 64, 80, 100, 200, 1000) for n in (1, 10)]  # clean constant envelope: 6x
FEW = ["zeros", "noise1", "noise300", "nfm64-noise1", "nfm64-noise10", "nfm80-noise1", "nfm100-noise1", "nfm200-noise1"]
CASES = [(name, c) for name in PLANS for c in (FEW if name.startswith("d521") else FLAT + NFM)]


@functools.lru_cache(maxsize=None)
def _setup(name: str):
    fs, bw, d, off = PLANS[name]
    taps = P.design_channel_filter(fs, bw, d)
    plan = P.plan_channel(taps, sample_rate=fs, freq_offset=off, mix_sign=1, decimation=d, fmt="s16", iq_order="iq")
    groups_q = max(1, -(-(-(-len(taps) // d)) // P.MFMA_Q))
    assert groups_q == (3 if d == 208 else 1)
    max_ks = 11 if d == 521 else None  # (the row-staged ring slots' k-step ranges)
    return SimpleNamespace(fs=fs, d=d, off=off, plan=plan, fs_ch=fs / d, rows=64 * groups_q,
                           mps={k: P.plan_mfma(plan, max_ksteps=max_ks, **kw) for k, kw in PLAN_KW.items()})


@functools.lru_cache(maxsize=None)
def _case(name: str, capture: str):
    """(raw int16, wideband RMS, m0, float64 z of outputs m0 .. m0 + N_OUT - 1 before the output rotation, its mean
    power).  Seeded generators; the reference is computed once per case and shared, read-only."""
    s = _setup(name)
    m0 = s.rows + 1
    gated = capture == "gated-tone"
    if gated:  # the tone fills the first half; the outputs' whole windows (rows * D frames back) lie in the quiet half
        m0 += N_OUT + s.rows
    n = (m0 + N_OUT + 64) * s.d
    t = np.arange(n) / s.fs
    seed = sorted(FLAT + NFM).index(capture)
    noise = lambda lsb: np.random.default_rng(seed).normal(scale=lsb, size=(n, 2))  # noqa: E731
    if capture == "zeros":
        iq = np.zeros((n, 2))
    elif capture == "dc3":
        iq = np.array([3.0, -3.0]) + noise(1.0)
    elif gated:
        tone = 0.95 * 32767.0 * np.exp(2j * np.pi * (s.off + 3_000.0) * t)
        tone[(m0 - s.rows - 1) * s.d:] = 0.0
        iq = np.column_stack((tone.real, tone.imag)) + noise(1.0)
    elif capture.startswith("noise"):
        iq = noise(float(capture[5:]))
    else:
        amp, lsb = (float(v) for v in capture[3:].split("-noise"))
        z = amp * np.exp(1j * (2 * np.pi * s.off * t + 3.0 * (1.0 - np.cos(2 * np.pi * 1000.0 * t))))
        iq = np.column_stack((z.real, z.imag)) + noise(lsb)
    raw = np.rint(iq).astype(np.int16).reshape(-1)
    xc = raw[0::2].astype(np.float64) + 1j * raw[1::2].astype(np.float64)
    wide = float(np.sqrt(np.mean(np.abs(xc / 32768.0) ** 2)))
    g = s.plan.taps_natural  # ingest scale folded in
    nfft = 1 << int(np.ceil(np.log2(xc.size + g.size)))
    want = np.fft.ifft(np.fft.fft(xc, nfft) * np.fft.fft(g, nfft))[np.arange(m0, m0 + N_OUT) * s.d]
    for a in (raw, want):
        a.setflags(write=False)
    return raw, wide, m0, want, float(np.mean(np.abs(want) ** 2))


@functools.lru_cache(maxsize=None)
def _emulated(name: str, capture: str, precision: str):
    s = _setup(name)
    raw, _, m0, want, _ = _case(name, capture)
    if precision == "float32":  # the VALU kernel: float32 products, error at the rounding of z itself
        return want.astype(np.complex64).astype(np.complex128)
    return _emulate_mfma_outputs(s.mps[precision], raw, s.d, m0, N_OUT, acc32=PLAN_KW[precision]["acc32"])


def _rms(a) -> float:
    return float(np.sqrt(np.mean(np.abs(a) ** 2)))


def _audio(name: str, z: np.ndarray, m0: int) -> np.ndarray:
    """The NFM chain behind the channelizer: output rotation, float32 z, discriminator + de-emphasis, the writer's clip."""
    s = _setup(name)
    cw, sw = M.rotation(np.arange(m0, m0 + N_OUT, dtype=np.uint64), s.plan.rot_step, s.plan.rot_base)
    y, _ = O.demodulate((z * (cw + 1j * sw)).astype(np.complex64), O.DemodState("nfm", s.fs_ch))
    return np.clip(y, -0.99, 0.99)[SETTLE:].astype(np.float64)


def _picked(name: str, capture: str) -> str:
    """What the guard chooses for this capture, given its true wideband RMS and the float64 channel power."""
    s = _setup(name)
    _, wide, _, _, power = _case(name, capture)
    kernel_for = lambda p: SimpleNamespace(precision=p, _mfma_ok=True, _ensure_mfma=lambda: s.mps[p])  # noqa: E731
    return PR.pick_precision(kernel_for, "fast", "nfm", power, wide)


@pytest.mark.parametrize("precision", ["fast", "fine"])
@pytest.mark.parametrize("name,capture", CASES)
def test_plan_predicts_the_emulated_error_on_every_data_class(name, capture, precision):
    """Prediction: the exact model's RMS z error stays below 2x ``z_error_rms`` on the noise-only and constant classes (the
    bar of the long-run check in test_host_logic) and below the tonal allowance, 6x, on clean constant-envelope signals."""
    _, wide, _, want, _ = _case(name, capture)
    err = _rms(_emulated(name, capture, precision) - want)
    pred = _setup(name).mps[precision].z_error_rms(wide)
    factor = 6.0 if capture in NFM else 2.0
    print(f"{name} {capture} {precision}: wideband {wide:.2e}, z rms err {err:.2e}, predicted {pred:.2e} (x{err / pred:.2f})")
    assert err < factor * pred + 1e-12, (name, capture, precision, err, pred)


@pytest.mark.parametrize("name,capture", [c for c in CASES if c[1] in NFM])
def test_guard_keeps_the_audio_bar_on_quiet_nfm_captures(name, capture):
    """Promise: at the precision ``pick_precision`` returns, the emulated audio is within 1e-4 RMS of the audio of the
    float64 z."""
    _, wide, m0, want, power = _case(name, capture)
    picked = _picked(name, capture)
    err = _rms(_audio(name, _emulated(name, capture, picked), m0) - _audio(name, want, m0))
    at_fast = _rms(_audio(name, _emulated(name, capture, "fast"), m0) - _audio(name, want, m0))
    print(f"{name} {capture}: wideband {wide:.2e}, |z| {np.sqrt(power):.2e}: guard picks {picked}, audio rms err {err:.2e} "
          f"(at fast {at_fast:.2e})")
    assert err < AUDIO_BAR, (name, capture, picked, err)


@pytest.mark.parametrize("name", ["d104+1.0MHz", "d104+1.3MHz", "d521+2.2MHz"])
def test_guard_does_not_escalate_a_signal_above_the_quiet_level(name):
    """Away from offset 0 (where the zero-input response is of the order of the uniform floor) an NFM signal of 200 or
    1000 LSB alone in the capture stays at "fast" -- and keeps the bar there; one of 64 LSB does not stay."""
    for capture in [c for n_, c in CASES if n_ == name and c.startswith(("nfm200", "nfm1000"))]:
        assert _picked(name, capture) == "fast", (name, capture)
    assert _picked(name, "nfm64-noise1") != "fast"


def test_zero_input_response_is_the_kernels_output_on_an_all_zero_capture():
    """``zero_rms`` is exact: on an all-zero capture the model emits one constant of that magnitude, per plan and
    precision (the float64 filter gives 0); uint8 captures drop no product and have no floor at all."""
    for name in PLANS:
        s = _setup(name)
        for precision in ("fast", "fine", "full"):
            z = _emulated(name, "zeros", precision)
            assert np.all(z == z[0])
            assert abs(abs(z[0]) - s.mps[precision].zero_rms) <= 1e-9 * s.mps[precision].zero_rms + 1e-18, (name, precision)
        fs, bw, d, off = PLANS[name]
        u8 = P.plan_channel(P.design_channel_filter(fs, bw, d), sample_rate=fs, freq_offset=off, mix_sign=1, decimation=d, fmt="u8")
        assert P.plan_mfma(u8, acc32=True).floors() == (0.0, 0.0, 0.0)


def test_guard_applies_the_coherent_bound_below_the_quiet_level_of_the_planes():
    """``dropped_floor``: the zero-input response holds at every level, the coherent bound below QUIET_WIDEBAND of the
    KERNEL's full scale -- for float32 planes with ``shift`` bits of headroom at 2^shift times that level of the capture,
    and worth 2^shift times as much there."""
    floors = (1e-6, 3e-6, 2e-5)
    q = P.QUIET_WIDEBAND
    assert q == 128.0 / 32768.0
    assert P.dropped_floor(floors, 0.5) == 3e-6 and P.dropped_floor(floors, q) == 3e-6
    assert P.dropped_floor(floors, q * (1 - 1e-9)) == 2e-5 and P.dropped_floor(floors, 0.0) == 2e-5
    assert P.dropped_floor((4e-6, 3e-6, 1e-6), 0.0) == 4e-6
    mp = SimpleNamespace(err_norm=0.0, floor_rms=floors[0], zero_rms=floors[1], coherent_rms=floors[2])
    kernels = {p: SimpleNamespace(precision=p, _mfma_ok=True, _ensure_mfma=lambda: mp) for p in ("fast", "fine", "full")}
    level = PR.PRECISION_GUARD * 1e-5  # between the two floors' bars
    for scale in (1.0, 4.0):
        memo = {}
        pick = lambda wide: PR.pick_precision(kernels.__getitem__, "fast", "nfm", (scale * level) ** 2, wide,  # noqa: E731
                                              memo=memo, floor_scale=scale)
        assert pick(scale * q * 1.01) == "fast" and pick(scale * q * 0.99) == "float32"
        assert memo["fast"] == (0.0, floors)  # what a batch remembers per precision: the norm and all three floors
        assert pick(scale * q * 1.01) == "fast" and pick(scale * q * 0.99) == "float32"  # ... and judges by again
