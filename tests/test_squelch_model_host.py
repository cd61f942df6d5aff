"""The squelch oracle (tests/squelch_model.py) against the reference's recorded results and against numpy's own
int8 / float32 convolutions, before it judges a kernel (tests/test_gpu_squelch_shapes.py).  No GPU needed."""
from __future__ import annotations

import numpy as np
import pytest
import squelch_model as M

import iq_to_audio_amd.squelch as S

N = 700
HOLDS = [0, 1, 126, 127, 128, 255, 256, 300, N - 1, N, 5 * N]
FADES = [1, 2, 7, N - 1, N, N + 1, 3 * N + 2]
DENSITIES = [0.02, 0.5, 0.98]


def _mask(density, seed=0):
    return np.random.default_rng(seed).random(N) < density


@pytest.mark.parametrize("fixture", ["squelch.npz", "squelch_edges.npz"])
def test_the_oracle_reproduces_the_reference_fixtures(golden, fixture):
    seen = 0
    for name, x, rate, params, scalars, mask_bits, gain in M.fixture_cases(golden(fixture)):
        cfg = S.SquelchConfig(**params)
        got = M.chain(x, float(rate), cfg)
        want_floor, want_thr, start, stop = scalars
        assert abs(got["noise_floor_db"] - want_floor) <= 1e-4, (name, got["noise_floor_db"], want_floor)
        assert abs(got["threshold_db"] - want_thr) <= 1e-4, (name, got["threshold_db"], want_thr)
        assert (got["start"], got["stop"]) == (int(start), int(stop)), name
        assert got["gain"].dtype == np.float32 and float(np.max(np.abs(got["gain"] - gain))) <= 1e-6, name
        want_mask = np.unpackbits(mask_bits)[:x.shape[0]].astype(bool)
        differ = got["mask"] != want_mask
        near = np.abs(got["level"] - got["threshold"]) <= 1e-3
        print(f"{fixture} {name}: {int(differ.sum())} mask samples differ, {int(near.sum())} lie within 1e-3 dB")
        assert not np.any(differ & ~near), (name, int(np.sum(differ & ~near)))
        # the oracle's windows are the package's
        w = S._windows(x.shape[0], float(rate), cfg)
        assert {k: got[k] for k in w} == w, name
        seen += 1
    assert seen == len(golden(fixture)["cases"]) and seen >= 9


def _numpy_int8_dilate(mask, h):
    """numpy's own int8 convolution of the mask with h + 1 ones, forwards and backwards: the accumulator wraps."""
    out = mask.copy()
    if h > 0:
        ones = np.ones(h + 1, dtype=np.int8)
        m8 = mask.astype(np.int8)
        back = np.convolve(m8, ones, mode="full")
        assert back.dtype == np.int8
        out |= back[:mask.size] > 0
        out |= np.convolve(m8[::-1], ones, mode="full")[:mask.size][::-1] > 0
    return out


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("hold", HOLDS)
def test_dilate_is_numpy_int8_convolution(density, hold):
    mask = _mask(density, seed=hold)
    got = M.dilate(mask, hold)
    assert got.dtype == bool and np.array_equal(got, _numpy_int8_dilate(mask, hold))


@pytest.mark.parametrize("hold", HOLDS)
def test_dilate_of_bursts_is_numpy_int8_convolution_and_wraps_from_hold_128(hold):
    mask = M.burst_mask()
    hold = {N - 1: mask.size - 1, N: mask.size, 5 * N: 5 * mask.size}.get(hold, hold)
    got = M.dilate(mask, hold)
    assert np.array_equal(got, _numpy_int8_dilate(mask, hold))
    # a clear sample's window holds at most `hold` set samples, so 128 -- the first count that is not positive as
    # int8 -- is reached from hold 128 on, not at 127
    assert np.array_equal(got, M.dilate(mask, hold, wrap=False)) == (hold < 128)


def test_window_counts_are_direct_counts():
    mask = _mask(0.5, seed=3)
    for h in (1, 5, N - 1, N + 9):
        tail, head = M.window_counts(mask, h)
        for i in (0, 1, 4, 5, 6, N // 2, N - 6, N - 2, N - 1):
            assert tail[i] == mask[max(0, i - h):i + 1].sum() and head[i] == mask[i:i + h + 1].sum()


def _numpy_f32_gain(mask, f):
    """The fade as a float32 convolution of the edge-padded mask with [0, 1/f, .., 1, 1, .., 1/f], clipped."""
    up = np.linspace(0.0, 1.0, f + 1, dtype=np.float32)
    taps = np.concatenate((up[:-1], np.ones(1, np.float32), up[:0:-1]))
    padded = np.pad(mask.astype(np.float32), f, mode="edge")
    return np.clip(np.convolve(padded, taps, mode="same")[f:f + mask.size], 0.0, 1.0)


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("fade", FADES)
def test_gain_is_the_float32_pad_and_convolve_formulation(density, fade):
    for seed, first, last in ((fade, None, None), (fade + 1, True, False), (fade + 2, False, True)):
        mask = _mask(density, seed=seed)
        if first is not None:
            mask[0], mask[-1] = first, last
        got = M.gain(mask, fade)
        assert got.dtype == np.float32 and got.shape == mask.shape
        assert float(np.max(np.abs(got - _numpy_f32_gain(mask, fade)))) <= 1e-6, (density, fade, seed)
    assert np.array_equal(M.gain(mask, 0), mask.astype(np.float32))


@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, N])
def test_box_is_float32_convolve_same(w):
    rng = np.random.default_rng(w)
    mag = (np.abs(rng.standard_normal(N)) * np.where(rng.random(N) < 0.3, 0.5, 0.003)).astype(np.float32)
    got = M.box(mag, w)
    want = mag if w == 1 else np.convolve(mag, np.ones(w, dtype=np.float32) / float(w), mode="same")
    assert got.dtype == np.float32 and want.dtype == np.float32
    rel = np.max(np.abs(got.astype(np.float64) - want) / want)
    print(f"w={w}: max relative difference {rel:.3g}")
    assert rel <= 2.3e-7
    # the taps, spelled out at a few samples
    for i in (0, 1, w // 2, N // 2, N - 2, N - 1):
        lo = i - w // 2
        taps = mag[max(lo, 0):max(min(lo + w, N), 0)].astype(np.float64)
        assert got[i] == np.float32(taps.sum() / w) or abs(float(got[i]) - taps.sum() / w) <= np.spacing(got[i])


def test_dbfs_bounds_and_stage_helpers():
    v = np.array([0.0, 1e-12, 1e-10, 1e-8, 1.0, 4.0], dtype=np.float32)
    db = M.dbfs(v)
    assert db.dtype == np.float32 and db[:3].tolist() == [-160.0, -160.0, -160.0] and db[3] == -160.0
    assert db[4] == 0.0 and db[5] == np.float32(20 * np.log10(4.0))
    b = M.envelope_bound(np.array([-160.0, -6.0, 12.0], dtype=np.float32))
    assert np.all(b > 1.03e-6) and b[0] == pytest.approx(1.0355e-6 + 2.0 ** -16, rel=1e-3)
    g = np.array([0, 0.001, 0.0011, 1, 0.5, 0.001], dtype=np.float32)
    assert M.bounds(g, 6, 0, 0, True) == (2, 5) and M.bounds(g, 6, 1, 9, True) == (1, 6)
    assert M.bounds(g, 6, 3, 0, False) == (0, 6) and M.bounds(np.zeros(4, np.float32), 4, 1, 1, True) == (0, 0)
    x = np.array([[0.5, -0.5], [1.5, -1.5], [1.0, -1.0]], dtype=np.float32)
    pcm = M.output_pcm16(x, np.ones(3, np.float32), 0, 3)
    assert pcm.tolist() == [[16384, -16384], [32767, -32768], [32767, -32767]]  # ties to even, saturation
