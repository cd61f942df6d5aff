"""The spectrum and stage models (tests/spectrum_model.py, tests/stage_model.py) before they judge a kernel
(tests/test_gpu_spectrum_shapes.py, tests/test_gpu_stage_shapes.py): the model against the oracle's PSD, shift_index
against numpy's fftshift, the constant of the power bound measured against a long-double DFT, the condition that lets
the GPU test compare every bin with no mask, the pair average against the oracle's reduction, the mixer's bound against
the oracle's mixer and against a float32 ramp, and the host-side argument checks of the five entry points (made before
any launch).  No GPU needed."""
from __future__ import annotations

import ctypes
import importlib.util
import sys
from ctypes import c_double, c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest

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


def test_power_and_db_agree_with_the_oracle_for_a_hann_window():
    """O.psd_frame_db / O.compute_psd (Hann window of the frame's length, zero-padded to nfft) against db(power(...)) with
    that window and scale handed in: the same pocketfft transform, so a few ulp of the dB value."""
    fs = 2.0e6
    for nfft, n in ((256, 256), (257, 257), (1024, 700), (999, 998), (64, 1)):
        raw = M.noisy("f32", n, 3)
        x = raw.view(np.complex64)
        w = np.hanning(n).astype(np.float64)
        got = M.db(M.power(raw, "f32", "iq", 0, 1, 1, nfft, n, w, M.scale_of(w, fs)))[0]
        np.testing.assert_allclose(got, O.psd_frame_db(x, nfft, fs), rtol=0, atol=1e-10)
        np.testing.assert_allclose(got, O.compute_psd(x, fs, nfft)[1], rtol=0, atol=1e-10)
    # frames after the first, through first / hop
    raw = M.noisy("f32", 300, 4)
    w = np.hanning(64).astype(np.float64)
    got = M.db(M.power(raw, "f32", "iq", 5, 17, 4, 64, 64, w, M.scale_of(w, fs)))
    for f in range(4):
        np.testing.assert_allclose(got[f], O.psd_frame_db(raw.view(np.complex64)[5 + 17 * f:5 + 17 * f + 64], 64, fs), rtol=0, atol=1e-10)


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("order", M.ORDERS)
def test_ingest_is_the_oracles(fmt, order):
    raw = SG.mix_raw(fmt, 300)
    want = O.ingest_to_complex64(raw, fmt, order)
    got = SG.ingest_c64(raw, fmt, order)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_shift_index_is_fftshift():
    for nfft in sorted({c.nfft for c in M.ALL_CASES} | {nfft for _, nfft, *_ in M.WATERFALL_CASES}):
        k = np.arange(nfft)
        np.testing.assert_array_equal(M.shift_index(k, nfft), np.fft.fftshift(k))
    assert {c.nfft % 2 for c in M.ALL_CASES} == {0, 1}


def test_the_tables_hold_what_the_issue_lists():
    sizes = {(c.nfft, c.use, c.n_frames) for c in M.SIZE_CASES}
    for nfft in (2, 3, 255, 256, 257, 999, 1024):
        for use in (1, nfft - 1, nfft):
            assert (nfft, use, 1) in sizes and (nfft, use, 3) in sizes
    assert {(c.fmt, c.order, c.nfft) for c in M.FORMAT_CASES} == {(f, o, n) for f in M.FORMATS for o in M.ORDERS for n in (256, 257)}
    g = M.GEOMETRY_NFFT
    assert {(c.n_frames, c.hop, c.first) for c in M.GEOMETRY_CASES} == {(nf, h, f0) for nf in (1, 2, 65) for h in (1, g // 4, g, g + 7)
                                                                       for f0 in (0, 5)}
    assert len({(c.nfft, c.n_frames) for c in M.PLAN_CASES}) == 10
    for c in M.FORMAT_CASES:  # the extremes are inside the frames
        raw = c.raw()
        lo, hi = 2 * c.first, 2 * c.n_samples
        for v in M.EXTREMES[c.fmt][:2]:
            assert np.any(raw[lo:hi].view(np.uint8 if c.fmt == "u8" else raw.dtype) == np.array(v, dtype=raw.dtype))
    assert {c.n_samples for c in M.ALL_CASES if c.n_frames > 1}  # (n_samples is exactly the last frame's end, by construction)


@pytest.fixture(scope="module")
def measured():
    """Per case: (largest |p_fft - p_exact| / form, smallest p_exact / power_bound over the bins)."""
    out = {}
    for c in M.ALL_CASES:
        a = c.args()
        p, pe, form = M.power(*a), M.exact_power(*a), M.fft_form(*a)
        ratio = float(np.max(np.abs(p - pe) / form)) if form.min() > 0 else 0.0
        bound = M.power_bound(*a, p=pe)
        out[c.name] = (c, ratio, float(np.min(pe / bound)))
    return out


def test_the_constant_of_the_power_bound(measured):
    """c: the float64 CPU FFT's error against the long-double DFT, as a multiple of eps log2(n) ||x w||^2 / scale, largest
    over every bin of every case; C = 8 times that."""
    per_nfft: dict = {}
    for c, ratio, _ in measured.values():
        per_nfft[c.nfft] = max(per_nfft.get(c.nfft, 0.0), ratio)
    worst = max(per_nfft.values())
    print("\nlargest CPU-FFT ratio per nfft: " + ", ".join(f"{n}: {r:.2f}" for n, r in sorted(per_nfft.items())))
    print(f"measured ratio {worst:.3f}; C_MEASURED = {M.C_MEASURED}; c = 8 C_MEASURED = {M.C}")
    assert worst <= M.C_MEASURED <= 1.01 * worst and M.C == 8.0 * M.C_MEASURED
    assert max(per_nfft, key=per_nfft.get) in (3, 255, 257, 999)  # a Bluestein length dominates


def test_no_bin_of_a_noisy_case_needs_a_mask(measured):
    """Every bin of every case compared in dB terms carries at least 10^6 times its bound: a deviation the bound lets
    through is below 4.4e-6 dB everywhere, and the GPU test compares every bin."""
    assert {c.name for c in M.NOISY_CASES} <= set(measured)
    for c, _, margin in measured.values():
        if c.kind == "noisy":
            assert margin >= 1e6, (c.name, margin)
    worst = min((m, c.name) for c, _, m in measured.values() if c.kind == "noisy")
    print(f"\nsmallest bin power / bound over the noisy cases: {worst[0]:.3e} ({worst[1]})")


def test_the_waterfall_cases_need_no_mask_either():
    fs = M.SAMPLE_RATE
    for name, nfft, hop, max_slices, sizes in M.WATERFALL_CASES:
        chunks = M.waterfall_chunks(sizes)
        blocks = [b for b in chunks if b is not None and b.size]
        stream = np.concatenate(blocks)
        starts = O.sliding_window_starts([b.size for b in blocks], nfft, hop)
        assert len(starts) >= 10, name
        w = np.hanning(nfft).astype(np.float64)
        scale = M.scale_of(w, fs)
        raw = stream.view(np.float32)
        for _, s0 in starts:
            p = M.power(raw, "f32", "iq", s0, 1, 1, nfft, nfft, w, scale)
            assert np.min(p / M.power_bound(raw, "f32", "iq", s0, 1, 1, nfft, nfft, w, scale, p=p)) >= 1e6, (name, s0)
    # the shapes the cases are named for
    name, nfft, hop, max_slices, sizes = M.WATERFALL_CASES[2]
    n_win = (sizes[0] - nfft) // hop + 1
    assert n_win > 64 and max_slices + 1 < 64  # more than BATCH_FRAMES windows in one block, room() below a batch
    assert M.WATERFALL_CASES[0][3] == 1 and M.WATERFALL_CASES[1][2] > M.WATERFALL_CASES[1][1]
    assert M.reductions(3, 1) == 2 and M.reductions(41, 40) == 1 and M.reductions(40, 40) == 0


def test_the_tones_sit_where_shift_index_says():
    for c in M.TONE_CASES:
        p = M.exact_power(*c.args())[0]
        k = int(np.argmax(p))
        assert M.shift_index(k, c.nfft) == c.bin and p[k] == pytest.approx(c.nfft / 4.0, rel=1e-6)
        assert np.max(np.delete(p, k)) < 1e-12 * p[k]  # the float32 rounding of the exponential, nothing else
    for c in M.ZERO_CASES:
        assert not M.power(*c.args()).any()


def test_pair_average_is_the_oracles_reduction_and_rounds_ties_to_even():
    for n_rows in M.PAIR_ROWS:
        for n_cols in M.PAIR_COLS:
            rows = M.pair_rows(n_rows, n_cols)
            want, _ = O.waterfall_reduce(list(rows), list(range(n_rows)), (n_rows + 1) // 2 if n_rows > 1 else 1)
            got = M.pair_average(rows)
            if n_rows > 1:
                np.testing.assert_array_equal(got.view(np.uint32), np.stack(want).view(np.uint32))
            else:
                np.testing.assert_array_equal(got.view(np.uint32), rows.view(np.uint32))
    rows = M.pair_rows(2, 257)
    got = M.pair_average(rows)[0]
    a, b = rows[0, :2].view(np.uint32).astype(np.int64), rows[1, :2].view(np.uint32).astype(np.int64)
    assert np.all(np.abs(a - b) == 1)  # float32 neighbours: the float64 mean is a tie
    assert np.all(got[:2].view(np.uint32) % 2 == 0) and {int(a[0]) % 2, int(a[1]) % 2} == {0, 1}
    assert got[2] == 0 and got[3] > 0 and got[4] == np.float32(2e-45) and got[5] == 0 and got[6] == 0
    assert np.isfinite(rows).all() and (np.abs(rows[:, 4:7]) < np.finfo(np.float32).tiny).all()


def test_the_mixers_bound_holds_the_oracle_and_refuses_a_float32_ramp():
    """The oracle's mixer (float64 ramp, complex64 oscillator and product) lies inside the bound at every setting; the
    same with the ramp rounded to float32, with phase0 dropped, or with the wrong sign of step does not."""
    n = 70_001
    x = SG.ingest_c64(SG.mix_raw("f32", n, plant=False), "f32", "iq")
    for phase0, step in SG.MIX_SETTINGS:
        k = np.arange(n, dtype=np.float64)
        good = (x * np.exp(1j * (phase0 + step * k)).astype(np.complex64)).astype(np.complex64)
        assert SG.mix_ratio(good, x, phase0, step) <= 1.0
        ramp32 = (np.float32(phase0) + np.float32(step) * k.astype(np.float32)).astype(np.float64)
        for bad_ramp in (ramp32, step * k, phase0 - step * k):
            if np.array_equal(bad_ramp, phase0 + step * k):
                continue
            bad = (x * np.exp(1j * bad_ramp).astype(np.complex64)).astype(np.complex64)
            with pytest.raises(AssertionError):
                SG.mix_ratio(bad, x, phase0, step)
    # at 1e6 rad a float32 ramp of a NON-integer step is off by up to ulp32(1e6) / 2 = 0.03 rad: 1e5 bounds
    assert 0.03 / (3 * SG.U32 + np.spacing(1e6)) > 1e5


def test_decimate_and_trickle_tables():
    cases = SG.decimate_cases()
    for n in SG.DECIM_LENGTHS:
        for d in (1, 2, 3, 26, n, n + 5):
            for first in (0, d - 1):
                assert any(c[:3] == (n, d, first) and c[3] == 0 for c in cases)
                full = [c[3] for c in cases if c[:3] == (n, d, first)][-1]
                assert full == np.arange(n)[first::d].size
    assert set(SG.TRICKLE_BYTES) == {0, 1, 15, 16, 17, 4096, 4111, (1 << 20) + 3}
    words = SG.decimate_input(257).view(np.float32)
    assert np.isnan(words).sum() >= 3 and np.signbit(words[3]) and words[3] == 0


# ---------------------------------------------------------------------------------------------------------------
# argument checks: made on the host before any launch


def _refused(name, *args):
    from iq_to_audio_amd import _native as N

    with pytest.raises(ValueError):
        N.call(name, *args)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from iq_to_audio_amd import _native as N

    N.build()
    p, null = c_void_p(4096), c_void_p(0)  # (never dereferenced: every call below is refused, or returns, on the host)

    def psd(fmt=2, order=0, samples=p, n_samples=100, first=0, hop=8, n_frames=3, nfft=16, use=16, window=p, scale=1.0, work=p):
        return ("iqa_psd_frames", c_int32(fmt), c_int32(order), samples, c_int64(n_samples), c_int64(first), c_int64(hop),
                c_int32(n_frames), c_int32(nfft), c_int32(use), window, c_double(scale), work, null, null, null, null)

    for bad in (dict(use=17), dict(nfft=1, use=1), dict(hop=0), dict(first=-1), dict(fmt=3), dict(fmt=-1), dict(order=4), dict(order=-1),
                dict(scale=0.0), dict(scale=float("nan")), dict(samples=null), dict(window=null), dict(work=null), dict(use=0),
                dict(n_frames=-1), dict(n_samples=31), dict(first=69), dict(n_samples=-5)):
        _refused(*psd(**bad))
    # sums that do not fit 64 bits: first + (n_frames - 1) hop + use wrapped to a small value and the call was accepted.  With NULL
    # pointers (checked after the geometry) nothing is launched either way; the message says which check refused.
    for bad in (dict(hop=1 << 62), dict(hop=(1 << 63) - 1), dict(first=(1 << 63) - 1, n_frames=1), dict(hop=(1 << 63) - 1, n_frames=2),
                dict(hop=1 << 62, n_frames=5)):
        _refused(*psd(samples=null, window=null, work=null, **bad))
        assert "reach past" in N.lib().iqa_last_error().decode(), bad
    N.call(*psd(n_frames=0, samples=null, window=null, work=null))
    N.call(*psd(n_frames=0, samples=null, window=null, work=null, hop=1 << 62))

    def decim(n=10, first=0, d=2, n_out=5, src=p, dst=p):
        return ("iqa_decimate", src, c_int64(n), c_int64(first), c_int32(d), dst, c_int64(n_out), null)

    for bad in (dict(d=0), dict(d=-3), dict(n=-1), dict(n_out=-1), dict(first=-1), dict(n_out=6), dict(first=2), dict(first=10, n_out=1),
                dict(n=0, n_out=1), dict(src=null), dict(dst=null)):
        _refused(*decim(**bad))
    for bad in (dict(n_out=1 << 62, d=4), dict(n_out=(1 << 63) - 1, d=2), dict(first=(1 << 63) - 1, n_out=2), dict(n_out=(1 << 62) + 1, d=4)):
        _refused(*decim(src=null, dst=null, **bad))  # (n_out - 1) D wrapped: as above
        assert "reads past" in N.lib().iqa_last_error().decode(), bad
    N.call(*decim(n_out=0, src=null, dst=null))
    N.call(*decim(n=0, n_out=0, first=7))

    _refused("iqa_pair_average_rows", p, c_int32(2), c_int32(0), p, null)
    _refused("iqa_pair_average_rows", p, c_int32(-1), c_int32(4), p, null)
    _refused("iqa_pair_average_rows", null, c_int32(2), c_int32(4), p, null)
    N.call("iqa_pair_average_rows", null, c_int32(0), c_int32(4), null, null)

    _refused("iqa_trickle_copy", c_void_p(4096 + 8), p, c_int64(64), c_int32(1), null)
    _refused("iqa_trickle_copy", p, c_void_p(4096 + 8), c_int64(64), c_int32(1), null)
    _refused("iqa_trickle_copy", p, p, c_int64(-1), c_int32(1), null)
    _refused("iqa_trickle_copy", null, p, c_int64(16), c_int32(1), null)
    N.call("iqa_trickle_copy", null, null, c_int64(0), c_int32(1), null)

    for bad in (dict(fmt=3), dict(order=4), dict(n=-1), dict(src=null)):
        a = dict(fmt=2, order=0, n=4, src=p)
        a.update(bad)
        _refused("iqa_oscillator_mix", c_int32(a["fmt"]), c_int32(a["order"]), a["src"], c_int64(a["n"]), c_double(0.0), c_double(0.0), p, null)
    N.call("iqa_oscillator_mix", c_int32(2), c_int32(0), null, c_int64(0), c_double(0.0), c_double(0.0), null, null)
    assert ctypes.sizeof(c_int64) == 8
