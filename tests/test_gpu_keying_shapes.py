"""iqa_keying_accumulate on the MI355X at its edge shapes, on hand-made theta streams: every row equals
the numpy oracle's (tests/keying_model.py), and what the oracle must give for the stream is asserted first.  Call lengths and
fronts, calls that begin and end in mid-window, crossings at a window's first sample and between two threads, gate edges
inside a pair, the quantiser's ties and non-finite values, t == c, the extreme centres, a window of 2048 crossings, positions
past 2^35 with the largest clock step, a zero step, and a guard row behind the rows."""
from __future__ import annotations

import importlib.util
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


K = _load("keying_model")
GUARD = 0x5A5A5A5A
FIND = dict(D=40, delay=1600, hop=4096, T=5, F=1170)  # 234 slices of 5 frames: 512 channel samples to a slice
S = 234
INCS = K.plan(48000.0)["incs"]
ALL_ON = np.ones(S, dtype=np.uint8)


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


@pytest.fixture(scope="module")
def table(A):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import dsp_plan as P

    return D.from_numpy(np.ascontiguousarray(P.keying_table()))


def gpu_rows(table, theta, pos, front, c, incs, g, find=FIND):
    """The entry point's rows (int64[windows][16]); a guard row behind them must come back untouched."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    theta = np.ascontiguousarray(theta, dtype=np.float32)
    n = theta.size
    w = int(N.lib().iqa_keying_windows(pos, n))
    assert w == K.windows(pos, n)
    out = D.from_numpy(np.full((w + 1) * 16, GUARD, dtype=np.int32))
    S_ = -(-find["F"] // find["T"])
    # (the device copies are held in names until the rows are read back: a temporary's memory would be handed out again)
    theta_dev = D.from_numpy(theta)
    front_dev = None if front is None else D.from_numpy(np.array([front], dtype=np.float32))
    gate_dev = D.from_numpy(np.ascontiguousarray(g, dtype=np.uint8))
    N.call("iqa_keying_accumulate", N.ptr(theta_dev), c_int64(n), c_int64(pos), N.ptr(front_dev), c_int32(c), (c_int32 * 7)(*incs), N.ptr(table),
           c_int32(find["D"]), c_int32(find["delay"]), c_int32(find["hop"]), c_int32(find["T"]), c_int64(find["F"]), c_int32(S_),
           N.ptr(gate_dev), N.ptr(out), N.stream_ptr())
    got = out.cpu().numpy().astype(np.int64).reshape(w + 1, 16)
    assert (got[w] == GUARD).all(), "the guard row was written"
    return got[:w]


def check(table, theta, pos, front, c, incs=INCS, g=ALL_ON, find=FIND):
    want = K.rows(theta, pos, front, c, incs, g, **find)
    got = gpu_rows(table, theta, pos, front, c, incs, g, find)
    np.testing.assert_array_equal(got, want)
    return want


def _wave(seed: int, n: int, flips: float = 0.25) -> np.ndarray:
    rng = np.random.default_rng(seed)
    sign = np.where(np.cumsum(rng.random(n) < flips) % 2 == 0, 1.0, -1.0)
    return (sign * 0.5 + 0.05 * rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 2047, 2048, 2049, 3 * 2048 + 5])
def test_call_lengths_and_fronts(A, table, n):
    g = (np.random.default_rng(n).random(S) < 0.8).astype(np.uint8)
    theta = _wave(n, n)
    # from the stream's start (the front must be NULL there), and from mid-window with and without the front
    want = check(table, theta, 0, None, 30, g=g)
    assert want.shape[0] == -(-n // 2048) and want[:, 0].sum() <= n - 1
    for pos in (1, 1000, 2047, 2048, 3 * 2048 + 5):
        a = check(table, theta, pos, None, 30, g=g)
        b = check(table, theta, pos, np.float32(-0.5), 30, g=g)
        assert a.shape[0] == (pos + n - 1) // 2048 - pos // 2048 + 1
        assert 0 <= b[0, 0] - a[0, 0] <= 1 and (a[1:] == b[1:]).all()  # the front adds the call's first pair at the most


def test_calls_that_begin_and_end_in_mid_window(A, table):
    g = (np.random.default_rng(7).random(S) < 0.8).astype(np.uint8)
    kp = K.plan(48000.0)
    theta = _wave(8, 9000)
    whole = K.stream_rows(theta, [9000], -12, 0, kp["incs"], g, **FIND)
    parts, pos = [], 0
    for n in (700, 1348, 1, 2047, 4100, 804):  # ends at 700, 2048, 2049, 4096, 8196, 9000
        front = None if pos == 0 else theta[pos - 1]
        parts.append((pos // 2048, gpu_rows(table, theta[pos : pos + n], pos, front, -12, kp["incs"], g)))
        np.testing.assert_array_equal(parts[-1][1], K.rows(theta[pos : pos + n], pos, front, -12, kp["incs"], g, **FIND))
        pos += n
    assert pos == 9000
    np.testing.assert_array_equal(K.add_by_window(parts, 5), whole)
    np.testing.assert_array_equal(gpu_rows(table, theta, 0, None, -12, kp["incs"], g), whole)


def test_crossing_positions(A, table):
    # a single crossing at m = 2048 k belongs to window k, not to the one its partner lies in
    for k in (1, 2):
        theta = np.full(3 * 2048, 0.5, dtype=np.float32)
        theta[2048 * k :] = -0.5
        want = check(table, theta, 0, None, 0)
        assert want[:, 1].tolist() == [1 if w == k else 0 for w in range(3)] and want[:, 0].tolist() == [2047, 2048, 2048]
    # ... also where the call starts there: the crossing needs the front value
    theta = np.full(100, -0.5, dtype=np.float32)
    assert check(table, theta, 4096, np.float32(0.5), 0)[0, :2].tolist() == [100, 1]
    assert check(table, theta, 4096, None, 0)[0, :2].tolist() == [99, 0]
    # crossings at multiples of 8: the partner is another thread's last sample
    theta = np.full(2048, 0.5, dtype=np.float32)
    for m in range(8, 2048, 8):
        theta[m:] *= -1.0
    want = check(table, theta, 0, None, 0)
    assert want[0, :2].tolist() == [2047, 255]
    # ... and at every other place in a thread's run
    for r in range(1, 8):
        theta = np.full(2048, 0.5, dtype=np.float32)
        theta[r::8] = -0.5
        assert check(table, theta, 2048, np.float32(0.5), 0)[0, :2].tolist() == [2048, 512 if r < 7 else 511]  # (r = 7: the last way back lies in the next window)


def test_gate_positions(A, table):
    theta = _wave(3, 3 * 2048, 0.5)
    # delay 0: slice s covers the samples 512 s .. 512 s + 511.  Alternating slices: the pair across an edge is none
    find = dict(FIND, delay=0)
    g = (np.arange(S) % 2 == 0).astype(np.uint8)
    want = check(table, theta, 0, None, 0, g=g, find=find)
    assert want[:, 0].tolist() == [2 * 511] * 3
    # an edge between a call's front and its first sample, from both sides
    assert check(table, theta[:10], 512, np.float32(0.5), 0, g=g, find=find)[0, 0] == 0  # slice 1 is off
    assert check(table, theta[:10], 1024, np.float32(0.5), 0, g=g, find=find)[0, 0] == 9  # the front lies in slice 1: off
    assert check(table, theta[:10], 1025, np.float32(0.5), 0, g=g, find=find)[0, 0] == 10
    # with the filter's delay the edges move by delay / D = 40 samples
    assert check(table, theta, 0, None, 0, g=g)[0, 0] == (552 - 1) + 511
    # all off, all on, a single slice
    assert check(table, theta, 0, None, 0, g=np.zeros(S, dtype=np.uint8), find=find)[:, :2].sum() == 0
    assert check(table, theta, 0, None, 0, find=find)[:, 0].tolist() == [2047, 2048, 2048]
    one = np.zeros(S, dtype=np.uint8)
    one[5] = 1
    assert check(table, theta, 0, None, 0, g=one, find=find)[:, 0].tolist() == [0, 511, 0]
    # the last slice holds every sample behind the capture's end
    last = np.zeros(S, dtype=np.uint8)
    last[S - 1] = 1
    assert check(table, theta[:100], 1 << 20, np.float32(0.1), 0, g=last, find=find)[0, 0] == 100
    # D larger than a slice: every sample in a slice of its own
    wide = dict(D=50000, delay=0, hop=4096, T=5, F=1170)
    g3 = (np.arange(S) % 3 != 0).astype(np.uint8)
    want = check(table, theta[:300], 0, None, 0, g=g3, find=wide)
    assert 0 < want[0, 0] < 299
    check(table, theta[:300], 77, np.float32(0.5), 0, g=g3, find=wide)


def test_values_and_centres(A, table):
    u = np.float32(1.0 / 4096.0)
    # t == c is the >= side
    for c in (300, -300, 0, 12868, -12868):
        theta = np.array([c - 1, c, c - 1, c + 1, c, c - 1], dtype=np.float32) * u
        assert K.quantise(theta).tolist() == [c - 1, c, c - 1, c + 1, c, c - 1]
        assert check(table, theta, 0, None, c)[0, :2].tolist() == [5, 4]
    # the extreme centres against a full-scale discriminator
    theta = np.tile(np.array([np.pi, -np.pi, 3.0, -3.0], dtype=np.float32), 64)
    assert K.quantise(theta[:4]).tolist() == [12868, -12868, 12288, -12288]
    for c, crossings in ((0, 255), (12868, 127), (-12868, 0), (-12867, 128), (32767, 0), (-32767, 0)):  # s = 1010, 1000, 1111, 1011, 0000, 1111
        assert check(table, theta, 0, None, c)[0, :2].tolist() == [255, crossings], c
    # exact ties of the quantiser go to the even side: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> 0, -1.5 -> -2
    ties = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3.5], dtype=np.float32) * u
    assert K.quantise(ties).tolist() == [0, 2, 2, 0, -2, 4]
    assert check(table, ties, 0, None, 1)[0, :2].tolist() == [5, 3]  # s = 0 1 1 0 0 1; rounding halves up would give 1 1 1 0 0 1
    assert check(table, ties, 0, None, 3)[0, :2].tolist() == [5, 1]  # s = 0 0 0 0 0 1; rounding halves up would give 0 0 1 0 0 1
    assert check(table, ties, 0, None, -1)[0, :2].tolist() == [5, 2]  # s = 1 1 1 1 0 1
    # NaN reads as 0, +-inf as +-32767, and values past the clamp stay on their side
    odd = np.array([np.nan, 1.0, np.nan, -1.0, np.inf, -np.inf, 100.0, -100.0, 1e30, -1e30, np.nan], dtype=np.float32)
    assert K.quantise(odd).tolist() == [0, 4096, 0, -4096, 32767, -32767, 32767, -32767, 32767, -32767, 0]
    assert check(table, odd, 0, None, 0)[0, :2].tolist() == [10, 8]  # s = 1 1 1 0 1 0 1 0 1 0 1
    assert check(table, odd, 0, None, 1)[0, :2].tolist() == [10, 8]  # s = 0 1 0 0 1 0 1 0 1 0 0: every NaN lies below 1
    assert check(table, odd, 0, None, 32767)[0, :2].tolist() == [10, 6]  # only +inf and what clamps to 32767 reach it
    assert check(table, odd, 5, np.float32(np.nan), -32767)[0, :2].tolist() == [11, 0]  # nothing lies below -32767
    assert check(table, odd, 5, np.float32(np.inf), 1)[0, :2].tolist() == [11, 9]


def test_extremes(A, table):
    alt = np.where(np.arange(3 * 2048) % 2 == 0, 0.5, -0.5).astype(np.float32)
    # 2048 crossings in a window, all at phase 0 (inc = 0): the largest sums, 2048 * 1024 = 2^21
    want = check(table, alt, 2048, np.float32(-0.5), 0, incs=(0,) * 7)
    assert want[:, :2].tolist() == [[2048, 2048]] * 3 and (want[:, 2::2] == 1 << 21).all() and (want[:, 3::2] == 0).all()
    # a clock of half the rate puts alternate crossings on opposite phases; one of a quarter on four
    half, quarter = 1 << 31, 1 << 30
    assert half >= 1 << 30  # (not a step the entry point takes: the largest is 2^30 - 1)
    big = (1 << 30) - 1
    want = check(table, alt, 2048, np.float32(-0.5), 0, incs=(big, 0, 1, big, 1 << 22, 1 << 29, (1 << 29) + 1))
    assert want[0, 1] == 2048 and want[0, 2 + 2 * 4] == sum(int(K.table()[(m % 1024), 0]) for m in range(2048, 4096))
    assert abs(want[0, 2 + 2 * 5]) <= 8 and abs(want[0, 3 + 2 * 5]) <= 8  # eighth turns: the vectors cancel
    # positions past 2^35, where m inc wraps 2^32 many times over
    g = ALL_ON
    for pos in ((1 << 35) + 5, (1 << 35) + 2047, (1 << 36) - 2048 - 3):
        theta = _wave(pos % 1000, 2048 + 7, 0.5)
        want = check(table, theta, pos, np.float32(0.5), 0, incs=(big, big - 1, 1, 0, INCS[1], INCS[6], 123456789), g=g)
        assert want.shape[0] == K.windows(pos, 2048 + 7) and want[:, 1].sum() > 500
        ref = K.rows_by_loops(theta[:300], pos, np.float32(0.5), 0, (big, big - 1, 1, 0, INCS[1], INCS[6], 123456789), g, **FIND)
        first = K.rows(theta[:300], pos, np.float32(0.5), 0, (big, big - 1, 1, 0, INCS[1], INCS[6], 123456789), g, **FIND)
        assert [first[j].tolist() for j in range(first.shape[0])] == [ref[w] for w in sorted(ref)]
    # inc = 0 beside live candidates: the skipped candidate's sums are 1024 K and 0
    theta = _wave(5, 5000)
    want = check(table, theta, 100, np.float32(0.5), 0, incs=P_INCS_LOW)
    assert (want[:, 2 + 2 * 4] == 1024 * want[:, 1]).all() and (want[:, 3 + 2 * 4] == 0).all() and want[:, 1].sum() > 100


P_INCS_LOW = K.plan(12000.0)["incs"]  # 3200, 4800 and 9600 skipped


def test_the_plan_the_package_passes(A, table):
    """The package's own wrapper on a describer's plans: the same rows."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import keying as KY
    from iq_to_audio_amd import dsp_plan as P

    assert P_INCS_LOW == P.plan_keying(12000.0).incs and P_INCS_LOW[4:] == (0, 0, 0)
    fp = P.plan_find(2.4e6, 4_800_000)
    dp = P.plan_describe(2.4e6, 300e3, 11000.0)
    kp = P.plan_keying(dp.fs_ch)
    g = (np.random.default_rng(9).random(fp.slices) < 0.8).astype(np.uint8)
    theta = _wave(11, 5000)
    theta_dev, front_dev, gate_dev = D.from_numpy(theta), D.from_numpy(np.array([0.25], dtype=np.float32)), D.from_numpy(g)
    first, rows = KY.accumulate_keying(theta_dev, 3000, front_dev, 17, kp, table, dp, fp, gate_dev)
    want = K.rows(theta, 3000, np.float32(0.25), 17, K.plan(dp.fs_ch)["incs"], g, D=dp.decimation, delay=dp.delay, hop=fp.hop, T=fp.slice_frames, F=fp.frames)
    assert first == 1
    np.testing.assert_array_equal(rows.cpu().numpy().reshape(-1, 16), want)
