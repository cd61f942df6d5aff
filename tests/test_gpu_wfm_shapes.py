"""The stereo matrix kernel (csrc/wfm.hip) against the float64 statement of DESIGN.md section 10 at every class of
channel rate: the shortest filter (128 kHz, N = 185), the longest (1.42 MHz, N = 2047 = IQA_WFM_MAX_TAPS) and four between
them; from the first sample of a stream (the ``hist == NULL`` path), over a partial last tile, cut into uneven blocks
(against the oracle, not only against itself), on silence and on a composite without a pilot; ``iqa_wfm_matrix`` on
synthetic planes.  Streams are a few tiles long: the oracle shares the kernel's zero initial state, so nothing settles.

Bounds (section 10, float32 FIRs of this length; not widened): planes within 1e-5 RMS and 1e-4 max of the oracle, the
pilot level within 1e-4 level + 1e-6.  Each test prints what it measured."""
from __future__ import annotations

import importlib.util
import math
from ctypes import c_int64
from pathlib import Path

import numpy as np
import pytest

from iq_to_audio_amd import dsp_plan as P

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("wfm_host_oracle", Path(__file__).with_name("test_wfm_host.py"))
H = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(H)

RMS_BOUND, MAX_BOUND = 1e-5, 1e-4
TILE = 2048  # WFM_TILE of csrc/wfm.hip: iqa_wfm_partials(n) = ceil(n / 2048) pins it below

# rate -> (N, R, M) of the plans
RATES = {128_000.0: (185, 7, 216), 171_000.0: (247, 9, 288), 240_000.0: (347, 13, 405), 10e6 / 21: (687, 25, 803),
         960_000.0: (1385, 51, 1617), 1_420_000.0: (2047, 75, 2392)}
EDGE_RATES = [128_000.0, 960_000.0, 1_420_000.0]
EXTREME_RATES = [128_000.0, 1_420_000.0]


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, dtype=np.float64) ** 2))) if np.size(a) else 0.0


def length(fs) -> int:
    """Three full tiles past the carried history, a partial last tile, not a multiple of the tile."""
    return 2 * (RATES[fs][0] - 1) + 3 * TILE + 777


def multiplex(fs, n):
    """n samples of the host tests' stereo multiplex: L = 0.5 sin 1 kHz, R = 0.5 sin 2.5 kHz, a 10 % pilot."""
    m = H.multiplex(fs, n / fs, lambda t: 0.5 * np.sin(2 * np.pi * 1000.0 * t), lambda t: 0.5 * np.sin(2 * np.pi * 2500.0 * t))
    assert m.size == n
    return m


def theta_of(m, fs):
    """The discriminator output that reads as composite ``m``: float32 radians per sample."""
    return (m * (2.0 * math.pi * P.WFM_DEVIATION / fs)).astype(np.float32)


def matrix_oracle(theta, fs) -> dict:
    """Steps 1-5 of section 10 on the float32 discriminator values, in float64 (the statement of
    tests/test_wfm_host.py ``wfm_oracle`` from the composite on)."""
    plan = P.plan_wfm(fs)
    n, d = theta.size, plan.delay
    m = theta.astype(np.float64) * fs / (2.0 * math.pi * P.WFM_DEVIATION)
    p = np.convolve(m, plan.h_pilot)[:n]
    mag2 = np.abs(p) ** 2
    u2 = np.where(mag2 > 0, p * p / np.where(mag2 > 0, mag2, 1.0), 0.0)
    c = np.where(np.abs(p) < 1e-12, 0.0, -np.imag(u2))
    md = np.concatenate([np.zeros(d), m[: n - d]]) if n > d else np.zeros(n)
    a = np.convolve(md, plan.h_audio)[:n]
    b = np.convolve(2.0 * md * c, plan.h_audio)[:n]
    out = dict(m=m, a=a, b=b, left=a + b, right=a - b, mag2=mag2, level=math.sqrt(float(np.mean(mag2))))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


_cases: dict = {}


def case(fs, kind="stereo"):
    """(theta, oracle) of one rate, computed once and shared read-only."""
    key = (fs, kind)
    if key not in _cases:
        n = length(fs)
        if kind == "stereo":
            m = multiplex(fs, n)
        else:  # a programme without a pilot: a 400 Hz tone
            m = 0.5 * np.sin(2 * np.pi * 400.0 * np.arange(n) / fs)
        theta = theta_of(m, fs)
        theta.setflags(write=False)
        _cases[key] = (theta, matrix_oracle(theta, fs))
    return _cases[key]


def run(fs, theta, cuts=None, *, extras=True):
    """The planes of ``theta`` through one WfmStereoCore, cut at ``cuts``: host copies of m, a, b, the sum of the per-tile
    |p|^2 sums; every output starts as NaN, so a sample the kernel does not write shows."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.decoders.wfm import WfmStereoCore

    core = WfmStereoCore(P.plan_wfm(fs))
    assert core.hist_len == 2 * (RATES[fs][0] - 1)
    n = theta.size
    th = D.to_device(np.array(theta), "float32")
    nan = float("nan")
    m, a, b = (D.empty(n, "float32").fill_(nan) for _ in range(3))
    powers = []
    cuts = [0, n] if cuts is None else cuts
    assert cuts[0] == 0 and cuts[-1] == n and all(hi > lo for lo, hi in zip(cuts[:-1], cuts[1:])), cuts
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if extras:
            tiles = core.partials_for(hi - lo)
            assert tiles == -(-(hi - lo) // TILE)
            part = D.empty(tiles, "float64").fill_(nan)
            core.process(th[lo:hi], a[lo:hi], b[lo:hi], m_out=m[lo:hi], partials=part)
            powers.append(float(part.sum().item()))
        else:
            core.process(th[lo:hi], a[lo:hi], b[lo:hi])
    out = dict(a=a.cpu().numpy(), b=b.cpu().numpy(), a_dev=a, b_dev=b)
    if extras:
        out.update(m=m.cpu().numpy(), power=sum(powers), level=math.sqrt(max(sum(powers), 0.0) / n), block_powers=powers)
    return out


def check_planes(tag, fs, got, want, names, skip):
    for name in names:
        g, w = got[name].astype(np.float64), want[name]
        assert g.shape == w.shape and np.all(np.isfinite(g)), (tag, name)
        err = g[skip:] - w[skip:]
        at = int(np.argmax(np.abs(err)))
        print(f"{tag} fs {fs:.0f} N {RATES[fs][0]} {name:>5} from {skip}: error rms {rms(err):.3e} max {np.abs(err).max():.3e} "
              f"(at {at + skip})")
    for name in names:
        err = got[name].astype(np.float64)[skip:] - want[name][skip:]
        assert rms(err) <= RMS_BOUND and np.abs(err).max() <= MAX_BOUND, (tag, fs, name, rms(err), np.abs(err).max())


def check_level(tag, fs, got, want):
    print(f"{tag} fs {fs:.0f} pilot level {got['level']:.9e} oracle {want['level']:.9e} diff {abs(got['level'] - want['level']):.3e}")
    assert abs(got["level"] - want["level"]) <= 1e-4 * want["level"] + 1e-6, (tag, fs, got["level"], want["level"])


def cuts_for(n, h):
    """A first block shorter than the history, a block of one sample, a block longer than the history that spans tiles, a
    block of half the history behind it (the ``cat([prev[n:], theta])`` path each time: the block behind a short one needs
    what was carried in front of it), the rest."""
    cuts = [0, h // 3, h // 3 + 1, h // 3 + 1 + h + 300, h // 3 + 1 + h + 300 + h // 2, n]
    sizes = [hi - lo for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert sizes[0] < h and sizes[1] == 1 and sizes[2] > h and sizes[3] < h and sizes[4] > h // 2, (cuts, h)
    return cuts


@pytest.mark.parametrize("fs", list(RATES))
def test_rate_classes_against_the_oracle(A, fs):
    """m and a from sample 0 (linear: the start of a stream is as good a target as any), b, L, R from 2(N-1) on (in front
    of it the pilot filter fills, |p| is tiny and c = -Im u^2 is ill-conditioned in any precision), the pilot level over
    all n; without m_out and partials the same a, b bit for bit."""
    from iq_to_audio_amd.decoders.wfm import stereo_matrix

    N, R, M = RATES[fs]
    rplan = P.plan_rds(fs)
    assert (rplan.wfm.ntaps, rplan.decim, rplan.half) == (N, R, M) and P.plan_wfm(fs).ntaps == N
    theta, want = case(fs)
    n, H2 = theta.size, 2 * (N - 1)
    assert n == H2 + 3 * TILE + 777 and n % TILE != 0
    got = run(fs, theta)
    left, right = stereo_matrix(got["a_dev"], got["b_dev"])
    got.update(left=left.cpu().numpy(), right=right.cpu().numpy())
    check_planes("one block", fs, got, want, ("m", "a"), 0)
    check_planes("one block", fs, got, want, ("b", "left", "right"), H2)
    assert np.all(np.isfinite(got["b"]))
    check_level("one block", fs, got, want)
    bare = run(fs, theta, extras=False)
    np.testing.assert_array_equal(bare["a"], got["a"])
    np.testing.assert_array_equal(bare["b"], got["b"])


@pytest.mark.parametrize("fs", EDGE_RATES)
def test_uneven_blocks_against_the_oracle(A, fs):
    N = RATES[fs][0]
    theta, want = case(fs)
    n, H2 = theta.size, 2 * (N - 1)
    cuts = cuts_for(n, H2)
    got = run(fs, theta, cuts)
    check_planes("blocks", fs, got, want, ("m", "a"), 0)
    check_planes("blocks", fs, got, want, ("b",), H2)
    check_level("blocks", fs, got, want)
    for (lo, hi), power in zip(zip(cuts[:-1], cuts[1:]), got["block_powers"]):  # each block's own sums: its samples, no other
        lvl, ref = math.sqrt(power / (hi - lo)), math.sqrt(float(np.mean(want["mag2"][lo:hi])))
        print(f"blocks fs {fs:.0f} [{lo}, {hi}) pilot level {lvl:.6e} oracle {ref:.6e}")
        assert abs(lvl - ref) <= 1e-4 * ref + 1e-6, (fs, lo, hi, lvl, ref)
    one = run(fs, theta)
    for name in ("m", "a", "b"):
        np.testing.assert_array_equal(got[name], one[name], err_msg=name)


@pytest.mark.parametrize("fs", EXTREME_RATES)
def test_silence(A, fs):
    """theta = 0: every plane and the power sum are exactly 0 (c is 0 where |p| < 1e-12, not 0 / 0)."""
    n = length(fs)
    got = run(fs, np.zeros(n, np.float32))
    for name in ("m", "a", "b"):
        assert np.all(got[name] == 0.0), name
    assert got["power"] == 0.0


@pytest.mark.parametrize("fs", EXTREME_RATES)
def test_composite_without_a_pilot(A, fs):
    """A 400 Hz tone and nothing at 19 kHz: m and a as ever; the level is the filter's leakage, below the stereo
    threshold; b is the tone times the phase of that leakage -- finite and, because |c| <= 1, within 2 sum|h_a| max|m| --
    and not compared with the oracle.  Cut into blocks, bit for bit the same."""
    N = RATES[fs][0]
    theta, want = case(fs, "mono")
    n, H2 = theta.size, 2 * (N - 1)
    got = run(fs, theta)
    check_planes("no pilot", fs, got, want, ("m", "a"), 0)
    check_level("no pilot", fs, got, want)
    assert got["level"] < P.WFM_STEREO_LEVEL and want["level"] < P.WFM_STEREO_LEVEL
    assert np.all(np.isfinite(got["b"]))
    bound = 2.0 * float(np.sum(np.abs(P.plan_wfm(fs).h_audio))) * float(np.abs(got["m"]).max())
    print(f"no pilot fs {fs:.0f}: max |b| {np.abs(got['b']).max():.4f}, bound {bound:.4f}")
    assert float(np.abs(got["b"]).max()) <= bound
    cut = run(fs, theta, cuts_for(n, H2))
    for name in ("m", "a", "b"):
        np.testing.assert_array_equal(cut[name], got[name], err_msg=name)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_matrix_kernel(A, n):
    """iqa_wfm_matrix: exactly a + b and a - b in float32, out of place and in place, nothing written past n."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as Nat

    rng = np.random.default_rng(n)
    a = (rng.standard_normal(n + 64) * 10.0 ** rng.uniform(-6, 2, n + 64)).astype(np.float32)
    b = (rng.standard_normal(n + 64) * 10.0 ** rng.uniform(-6, 2, n + 64)).astype(np.float32)
    for in_place in (False, True):
        ad, bd = D.to_device(a, "float32").clone(), D.to_device(b, "float32").clone()
        if in_place:
            left, right, fill_l, fill_r = ad, bd, a, b
        else:
            left, right = D.empty(n + 64, "float32").fill_(7.0), D.empty(n + 64, "float32").fill_(7.0)
            fill_l = fill_r = np.full(n + 64, 7.0, np.float32)
        Nat.call("iqa_wfm_matrix", Nat.ptr(ad), Nat.ptr(bd), c_int64(n), Nat.ptr(left), Nat.ptr(right), Nat.stream_ptr())
        lh, rh = left.cpu().numpy(), right.cpu().numpy()
        np.testing.assert_array_equal(lh[:n], a[:n] + b[:n])
        np.testing.assert_array_equal(rh[:n], a[:n] - b[:n])
        np.testing.assert_array_equal(lh[n:], fill_l[n:])
        np.testing.assert_array_equal(rh[n:], fill_r[n:])
        if not in_place:
            np.testing.assert_array_equal(ad.cpu().numpy(), a)
            np.testing.assert_array_equal(bd.cpu().numpy(), b)
