"""iqa_describe_accumulate on the MI355X at its edge shapes: hand-made streams, every row held bit for
bit to the numpy oracle of tests/describe_model.py, with what the oracle itself must give asserted first.  Lengths around the
2048-sample tile with and without the carried sample; the quantiser's special inputs and its extreme shifts; gates that are all
off, all on, single slices, edges inside a thread's eight samples, a decimation that does not divide the slice, a delay longer
than the stream's position, raw frames past 2^32, the clamp to the last frame; sums at their largest and the integer root at
perfect squares and beside them."""
from __future__ import annotations

import importlib.util
import math
import sys
from ctypes import c_int32, c_int64
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


M = _load("describe_model")
SMALL = dict(D=7, delay=11, hop=16, T=3, F=10)  # slices of 48 raw frames: an edge every 6.9 samples, 7 does not divide 48
GUARD = -7


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def gpu_rows(z, pos, prev, sh, g, *, D, delay, hop, T, F) -> np.ndarray:
    """The entry point's rows for one call, read back; a guard row behind them must stay as it was."""
    from iq_to_audio_amd import _dev as Dv
    from iq_to_audio_amd import _native as N

    z = np.ascontiguousarray(z, dtype=np.complex64)
    tiles = int(N.lib().iqa_describe_tiles(z.size))
    assert tiles == -(-z.size // 2048)
    out = Dv.from_numpy(np.full((tiles + 1) * 8, GUARD, dtype=np.int64))
    z_dev, g_dev = Dv.from_numpy(z.view(np.float32)), Dv.from_numpy(np.ascontiguousarray(g, dtype=np.uint8))
    prev_dev = None if prev is None else Dv.from_numpy(np.asarray([prev], dtype=np.complex64).view(np.float32))
    S = -(-F // T)
    assert len(g) == S
    N.call("iqa_describe_accumulate", N.ptr(z_dev), c_int64(z.size), c_int64(pos), N.ptr(prev_dev), c_int32(sh), c_int32(D), c_int32(delay),
           c_int32(hop), c_int32(T), c_int64(F), c_int32(S), N.ptr(g_dev), N.ptr(out), N.stream_ptr())
    got = out.cpu().numpy().reshape(tiles + 1, 8)
    assert (got[tiles] == GUARD).all()
    return got[:tiles]


def check(z, pos, prev, sh, g, **find) -> np.ndarray:
    want = M.rows(z, pos, prev, sh, g, **find)
    got = gpu_rows(z, pos, prev, sh, g, **find)
    np.testing.assert_array_equal(got, want)
    return want


def noise(n, seed=2, scale=0.01):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * scale).astype(np.complex64)


@pytest.mark.parametrize("n", [1, 2, 2047, 2048, 2049, 3 * 2048 + 5])
def test_lengths_with_and_without_the_sample_in_front(A, n):
    z = noise(n + 1)
    g = np.array([1, 1, 0, 1], dtype=np.uint8)
    big = dict(D=7, delay=11, hop=1024, T=5, F=20)  # slices of 5120 raw frames = 731.4 samples: several to a tile

    def expect(pos, carried):
        """(N, NP): slice 2 is off, samples 1465 .. 2195 of the stream (raw frames 7 m - 11 in 10240 .. 15359)."""
        on = [m for m in range(pos, pos + n) if not 1465 <= m <= 2195]
        starts = sum(1 for m in on if m == pos or m == 2196)  # the first sample of a gated stretch pairs with nothing ...
        return len(on), len(on) - starts + (1 if carried and on and on[0] == pos else 0)  # ... but with a carried one

    alone = check(z[1:], 0, None, 12, g, **big)
    assert alone.shape == (-(-n // 2048), 8) and (alone[:, 0].sum(), alone[:, 1].sum()) == expect(0, False)
    carried = check(z[1:], 1, z[0], 12, g, **big)
    assert (carried[:, 0].sum(), carried[:, 1].sum()) == expect(1, True)
    nowhere = check(z[1:], 5, None, 12, g, **big)  # a call in mid-stream that carries nothing: sample 0 forms no pair
    assert (nowhere[:, 0].sum(), nowhere[:, 1].sum()) == expect(5, False)


@pytest.mark.parametrize("sh", [-30, 0, 12, 30])
def test_quantiser_inputs(A, sh):
    z = noise(600, 3, 1.0 if sh <= 0 else 0.01)
    z[10] = complex(np.nan, 1.0)
    z[11] = complex(np.inf, -np.inf)
    z[12] = complex(-np.inf, np.nan)
    z[13] = complex(math.ldexp(40000.0, -sh), -math.ldexp(32767.5, -sh)) if abs(sh) < 30 else complex(3e38, -3e38)
    z[14] = complex(math.ldexp(2.5, -sh), math.ldexp(3.5, -sh))  # exact ties: to even
    z[15] = complex(math.ldexp(-0.5, -sh), math.ldexp(-1.5, -sh))
    z[16] = complex(1e-42, -1e-45)  # denormals
    q = M.quantise(np.float32([z[14].real, z[14].imag, z[15].real, z[15].imag, z[11].real, z[11].imag, z[10].real, z[13].real]), sh)
    if sh in (0, 12):
        assert q.tolist() == [2, 4, 0, -2, 32767, -32767, 0, 32767]
    if sh == 30:
        assert (np.abs(M.quantise(z.real[:10], sh)) == 32767).all()  # everything of size is clamped
    if sh == -30:
        assert not M.quantise(z.real[:10], sh).any()
    g = np.ones(4, dtype=np.uint8)
    check(z, 0, None, sh, g, **SMALL)
    check(z[1:], 1, z[0], sh, g, **SMALL)
    check(z[12:], 12, z[11], sh, g, **SMALL)  # the carried sample is infinite
    check(z[11:], 11, z[10], sh, g, **SMALL)  # ... or not a number


def test_gate_patterns(A):
    z = noise(2500, 4)
    for g in ([0, 0, 0, 0], [1, 1, 1, 1], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 1, 0], [0, 1, 1, 0]):
        g = np.array(g, dtype=np.uint8)
        # slices of 48 raw frames at D = 7 and a delay of 11: samples 0 .. 8, 9 .. 15, 16 .. 22, and from 23 on the last slice,
        # first by its own frames and then by the clamp to F - 1: the first edges fall inside threads 1 and 2's eight samples
        want = check(z, 0, None, 12, g, **SMALL)
        first = M.gate_of(np.arange(30), g, **SMALL).tolist()
        assert first == [int(g[0])] * 9 + [int(g[1])] * 7 + [int(g[2])] * 7 + [int(g[3])] * 7
        assert want[:, 0].sum() == sum(first[:23]) + (2500 - 23) * int(g[3])
        if not g.any():
            assert not want.any()
        check(z[100:], 100, z[99], 12, g, **SMALL)
    # a delay longer than the stream's position: the first samples all lie at raw frame 0
    late = dict(D=7, delay=1000, hop=16, T=3, F=100)
    g = (np.arange(34) % 2).astype(np.uint8)
    assert M.gate_of(np.arange(150), g, **late).tolist()[:143] == [0] * 143 and M.gate_of([150], g, **late)[0] == 1
    check(z, 0, None, 12, g, **late)
    check(z[1:], 1, z[0], 12, g, **late)
    # a decimation larger than a whole slice: a slice or more is stepped over between two samples
    coarse = dict(D=100, delay=3, hop=16, T=3, F=4000)
    g = (np.arange(1334) % 3 == 0).astype(np.uint8)
    want = check(z[:600], 0, None, 12, g, **coarse)
    assert want[:, 0].sum() == sum(1 for m in range(600) if (max(100 * m - 3, 0) // 48) % 3 == 0) and 150 < want[:, 0].sum() < 250
    # one frame, one slice
    check(z, 0, None, 12, np.array([1], dtype=np.uint8), D=3, delay=0, hop=1, T=1, F=1)


def test_raw_frames_past_two_to_the_32(A):
    find = dict(D=5, delay=77, hop=65536, T=65536, F=12 * 65536)  # slices of 2^32 raw frames
    g = np.array([0, 1] * 6, dtype=np.uint8)
    pos = -(-(10 << 32) // 5) - 2000  # the stream enters slice 10 a little after sample 2000
    z = noise(5000, 5)
    gate = M.gate_of(pos + np.arange(5000), g, **find)
    edge = int(np.argmin(gate))
    assert pos * 5 > 1 << 35 and gate[:edge].all() and not gate[edge:].any() and 2000 < edge < 2048
    want = check(z, pos, z[0], 12, g, **find)
    assert want[:, 0].tolist() == [edge, 0, 0]
    # behind the last frame the last slice goes on
    pos = (12 << 32) // 5 - 100
    assert M.gate_of(pos + np.arange(300), g, **find).all()
    check(z[:300], pos, None, 12, g, **find)


def test_extreme_sums_and_the_integer_root(A):
    g = np.ones(4, dtype=np.uint8)
    for value in (complex(1.0, 1.0), complex(-1.0, -1.0), complex(1.0, -1.0)):
        z = np.full(2 * 2048 + 3, value, dtype=np.complex64)  # 32768 at sh = 15: clamped to +-32767
        want = check(z, 0, None, 15, g, **SMALL)
        p = 2 * 32767 ** 2
        assert want[0].tolist() == [2048, 2047, 2048 * p, 2048 * (p >> 8) ** 2, 2048 * math.isqrt(p), 2047 * p, 0, 2047 * p]
        assert want[1, 7] == 2048 * p and 0.999 * 2 ** 62 < p * p < 2 ** 62 and 0.999 * 2 ** 57 < want[0, 3] < 2 ** 57
    z = np.full(4096, complex(1.0, 1.0), dtype=np.complex64)
    z[1::2] = complex(-1.0, 1.0)  # a quarter turn a sample: cr = 0, ci = +-p
    want = check(z, 0, None, 15, g, **SMALL)
    p = 2 * 32767 ** 2  # (the odd samples turn by +p, the even ones by -p: 1024 against 1023 in the first tile)
    assert want[0, 5:].tolist() == [0, p, 2047 * p] and want[1, 5:].tolist() == [0, 0, 2048 * p]
    # perfect squares and their neighbours: p = a^2 and a^2 + 1, p p' = (a a')^2 and beside it
    a = np.array([1, 2, 3, 181, 182, 255, 256, 257, 5792, 5793, 23170, 23171, 32766, 32767], dtype=np.float32)
    re = np.repeat(a, 6)
    im = np.tile(np.float32([0, 1, 0, 0, 1, 1]), a.size)
    z = (re + 1j * im).astype(np.complex64)
    z = np.concatenate((z, z[::-1], -z, np.conj(z))).astype(np.complex64)
    want = check(z, 0, None, 0, g, **SMALL)
    t = M.terms(z, 0, None, 0, g, **SMALL)
    assert t[0, 4] == 1 and t[1, 4] == 1 and t[6, 4] == 2 and t[7, 4] == 2 and (t[::6, 4][: a.size] == a.astype(np.int64)).all()
    pw = [int(v.real) ** 2 + int(v.imag) ** 2 for v in z.tolist()]
    prods = [pw[k] * pw[k - 1] for k in range(1, len(pw))]
    assert t[1:, 7].tolist() == [math.isqrt(v) for v in prods] and t[:, 4].tolist() == [math.isqrt(v) for v in pw]
    squares = sum(1 for v in prods if math.isqrt(v) ** 2 == v)
    beside = sum(1 for v in prods if math.isqrt(v - 1) ** 2 == v - 1 or math.isqrt(v + 1) ** 2 == v + 1)
    assert squares >= 50 and beside >= 20 and max(prods) > 2 ** 59
    assert want[:, 0].sum() == z.size
    check(z[5:], 5, z[4], 0, g, **SMALL)
