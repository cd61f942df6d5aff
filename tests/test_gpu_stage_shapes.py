"""The stand-alone stage kernels through the C ABI: k_oscillator_mix (csrc/stages.hip) against the bound of
tests/stage_model.py, k_decimate (csrc/demod.hip) and k_trickle_copy (csrc/stages.hip) as exact copies.

Every output is a view GUARD elements into a buffer of a fill pattern: the fill in front of and behind the output must
survive.  Inputs are followed, inside their allocation, by NaN / 32767 / 255.

The mixer: at step = 0, phase0 = 0 the output is the ingest conversion itself (times cos 0 = 1, plus or minus the other
component times sin 0 = 0: exact with or without fma; the sign of a zero aside), for all 12 format / order pairs with
the formats' extreme values planted.  Otherwise per component |got - exact| <= (|xr| + |xi|)(3 * 2^-24 + ulp64(|ph|))
(derivation: the model's docstring), at a small step from phase 0 and at phase0 = 1e6 with step
+-2.0, where a float32 or otherwise lossy ramp fails by orders of magnitude.
"""
from __future__ import annotations

import importlib.util
import sys
from ctypes import c_double, c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest

from iq_to_audio_amd import _dev as D
from iq_to_audio_amd import _native as N
from oracle import cpu_ref as O


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load("spectrum_model")
SG = _load("stage_model")

pytestmark = pytest.mark.gpu

GUARD = 64
FILL32 = 0x7FC5A5A5
FILL8 = 0xA5
MARGIN = 256
RATIOS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    N.lib()
    N.require_gpu()
    yield
    for name, ratio in sorted(RATIOS.items()):
        print(f"\nmixer [{name}]: largest |err| / bound = {ratio:.4f}")


def _with_margin(raw, fmt):
    raw = np.ascontiguousarray(raw).reshape(-1)
    host = np.full(raw.size + 2 * MARGIN, M.HOSTILE[fmt], dtype=raw.dtype)
    host[:raw.size] = raw
    return D.from_numpy(host)


def oscillator_mix(raw, fmt, order, phase0, step, n=None):
    """iqa_oscillator_mix into a guarded complex64 output.  ``raw``: interleaved values (or complex64 for f32)."""
    torch = D.torch_mod()
    raw = np.ascontiguousarray(raw)
    if raw.dtype == np.complex64:
        raw = raw.view(np.float32)
    n = raw.size // 2 if n is None else n
    src = _with_margin(raw, fmt)
    buf = torch.full((2 * (GUARD + max(n, 0) + GUARD),), FILL32, dtype=torch.int32, device=D.device())
    try:
        N.call("iqa_oscillator_mix", c_int32(M.FMT_CODE[fmt]), c_int32(M.ORDER_CODE[order]), N.ptr(src), c_int64(n), c_double(phase0),
               c_double(step), N.ptr(buf[2 * GUARD:]), N.stream_ptr())
    finally:
        h = buf.cpu().numpy()
        assert np.all(h[:2 * GUARD] == FILL32) and np.all(h[2 * (GUARD + max(n, 0)):] == FILL32), "a store landed outside the output"
    return h[2 * GUARD:2 * (GUARD + n)].copy().view(np.complex64)


def decimate(words, n, first, d, n_out):
    """iqa_decimate on complex64 given as uint32 words, into a guarded output.  Returns uint32 words."""
    torch = D.torch_mod()
    host = np.concatenate([np.asarray(words, dtype=np.uint32), np.full(2 * MARGIN, FILL32 ^ 0xFFFF, dtype=np.uint32)])
    src = D.from_numpy(host)
    room = n_out if 0 <= n_out <= len(words) else 0  # (the refusals ask for absurd counts: they get no room at all)
    buf = torch.full((2 * (GUARD + room + GUARD),), FILL32, dtype=torch.int32, device=D.device())
    try:
        N.call("iqa_decimate", N.ptr(src), c_int64(n), c_int64(first), c_int32(d), N.ptr(buf[2 * GUARD:]), c_int64(n_out), N.stream_ptr())
    finally:
        h = buf.cpu().numpy().view(np.uint32)
        assert np.all(h[:2 * GUARD] == FILL32) and np.all(h[2 * (GUARD + room):] == FILL32), "a store landed outside the output"
    return h[2 * GUARD:2 * (GUARD + room)].copy()


def trickle_copy(data, workgroups, src_offset=0, dst_offset=0):
    """iqa_trickle_copy from a device buffer into pinned host memory (as batch.py's PCM egress uses it) with a 64-byte
    guard behind the destination; returns the destination bytes after a stream synchronise."""
    torch = D.torch_mod()
    data = np.ascontiguousarray(data, dtype=np.uint8)
    nbytes = data.size
    src = D.from_numpy(np.concatenate([data, np.full(64, 0x3C, dtype=np.uint8)]))
    host = torch.full((nbytes + 64 + 16,), FILL8, dtype=torch.uint8).pin_memory()
    assert src.data_ptr() % 16 == 0 and host.data_ptr() % 16 == 0
    try:
        N.call("iqa_trickle_copy", c_void_p(src.data_ptr() + src_offset), c_void_p(host.data_ptr() + dst_offset), c_int64(nbytes),
               c_int32(workgroups), N.stream_ptr())
    finally:
        torch.cuda.current_stream().synchronize()
        h = host.numpy().copy()
    assert np.all(h[nbytes:] == FILL8), "a store landed behind the destination"
    return h[:nbytes]


# ---------------------------------------------------------------------------------------------------------------
# iqa_oscillator_mix


@pytest.mark.parametrize("order", M.ORDERS)
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_mixer_at_step_zero_is_the_ingest_conversion(fmt, order):
    for n in SG.MIX_LENGTHS:
        raw = SG.mix_raw(fmt, n)
        got = oscillator_mix(raw, fmt, order, 0.0, 0.0)
        want = O.ingest_to_complex64(raw, fmt, order)
        assert SG.same_values(got, want), (n, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:4])


@pytest.mark.parametrize("phase0,step", SG.MIX_SETTINGS, ids=lambda v: f"{v:g}")
@pytest.mark.parametrize("fmt", M.FORMATS)
def test_mixer_within_its_bound_and_back(fmt, phase0, step):
    """Every sample of every length within the bound, all four orders; then the output mixed with (-phase0, -step)
    returns the ingest conversion within twice the bound (each pass contributes at most one)."""
    for n in SG.MIX_LENGTHS:
        for order in M.ORDERS:
            raw = SG.mix_raw(fmt, n, plant=fmt != "f32")
            x = SG.ingest_c64(raw, fmt, order)
            got = oscillator_mix(raw, fmt, order, phase0, step)
            ratio = SG.mix_ratio(got, x, phase0, step)
            key = f"{fmt} phase0 {phase0:g} step {step:g}"
            RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
            if order == "iq":
                back = oscillator_mix(got, "f32", "iq", -phase0, -step)
                bound = 2.0 * SG.mix_bound(x, phase0, step)
                err = np.maximum(np.abs(back.real.astype(np.float64) - x.real), np.abs(back.imag.astype(np.float64) - x.imag))
                assert np.all(err <= bound), (n, float(np.max(err[bound > 0] / bound[bound > 0])))


def test_mixer_continuity_across_calls():
    """Two calls split at 3000 with the phase ComplexOscillator carries (wrapped mod 2 pi on the host) against one call:
    within the bound of each; the wrapper's phase agrees with the oracle's."""
    from iq_to_audio_amd.processing import ComplexOscillator

    n, cut = 5000, 3000
    raw = SG.mix_raw("f32", n, plant=False)
    x = raw.view(np.complex64)
    osc, st = ComplexOscillator(12345.678, 1e6), O.NcoState(12345.678, 1e6)
    step = 1 * osc.increment
    whole = oscillator_mix(raw, "f32", "iq", 0.0, step)
    SG.mix_ratio(whole, x, 0.0, step)
    first = osc.mix(x[:cut], 1)
    carried = osc.phase
    O.nco_mix(x[:cut], st, 1)
    assert abs(carried - st.phase) < 1e-12 and carried == (step * cut) % (2.0 * np.pi)
    second = oscillator_mix(raw[2 * cut:], "f32", "iq", carried, step)
    SG.mix_ratio(second, x[cut:], carried, step)
    np.testing.assert_array_equal(first.view(np.uint32), whole[:cut].view(np.uint32))
    # the carried phase is step * cut less a multiple of the float64 2 pi (37 turns, each 2.4e-16 off) and rounded once: off by
    # less than ulp64(step * n); both calls lie within their bounds of products that differ by that rotation
    slack = (np.abs(x[cut:].real.astype(np.float64)) + np.abs(x[cut:].imag)) * np.spacing(abs(step) * n)
    gap = np.maximum(np.abs(second.real.astype(np.float64) - whole[cut:].real), np.abs(second.imag.astype(np.float64) - whole[cut:].imag))
    assert np.all(gap <= SG.mix_bound(x[cut:], carried, step) + SG.mix_bound(x, 0.0, step)[cut:] + slack)
    osc.mix(x[cut:], 1)
    O.nco_mix(x[cut:], st, 1)
    assert abs(osc.phase - st.phase) < 1e-12


def test_mixer_edges():
    raw = SG.mix_raw("s16", 8)
    assert oscillator_mix(raw, "s16", "iq", 1.0, 1.0, n=0).size == 0  # writes nothing
    with pytest.raises(ValueError):
        oscillator_mix(raw, "s16", "iq", 0.0, 0.0, n=-1)


# ---------------------------------------------------------------------------------------------------------------
# iqa_decimate


def test_decimate_is_the_strided_slice():
    """Byte-equal to x[first::D] for D in {1, 2, 3, 26, n, n + 5}, first in {0, D - 1}, n in {1, 255, 256, 257}, with every
    output the input has (the last read is the input's last reachable sample) and with n_out = 0; NaN payloads,
    infinities, -0.0 and denormals survive as bits."""
    for n, d, first, n_out in SG.decimate_cases():
        words = SG.decimate_input(n)
        got = decimate(words, n, first, d, n_out)
        want = words.reshape(n, 2)[first::d][:n_out].reshape(-1)
        np.testing.assert_array_equal(got, want, err_msg=str((n, d, first, n_out)))


def test_decimate_refuses_a_read_past_the_input():
    words = SG.decimate_input(257)
    for n, first, d, n_out in ((257, 0, 2, 130), (257, 1, 2, 129), (257, 256, 1, 2), (257, 257, 1, 1), (257, 0, 0, 1), (257, 0, -1, 1),
                               (-1, 0, 1, 1), (257, 0, 1, -1), (257, -1, 1, 1), (257, 0, 4, 1 << 62)):
        with pytest.raises(ValueError):
            decimate(words, n, first, d, n_out)


# ---------------------------------------------------------------------------------------------------------------
# iqa_trickle_copy


@pytest.mark.parametrize("nbytes", SG.TRICKLE_BYTES)
def test_trickle_copy_is_byte_exact(nbytes):
    """0, 1, 15, 16, 17, 4096, 4096 + 15 and 1 MiB + 3 bytes (no words, a tail alone, words alone, words and every tail
    length class) with 0 (= 8), 1, 8, 64 workgroups and more workgroups than 16-byte words."""
    data = np.random.default_rng(nbytes).integers(0, 256, size=nbytes).astype(np.uint8)
    for wg in SG.trickle_workgroups(nbytes):
        np.testing.assert_array_equal(trickle_copy(data, wg), data, err_msg=f"{wg} workgroups")


def test_trickle_copy_refuses_misaligned_pointers():
    data = np.arange(64, dtype=np.uint8)
    for off in ((8, 0), (0, 8)):
        with pytest.raises(ValueError):
            trickle_copy(data[:32], 1, *off)
