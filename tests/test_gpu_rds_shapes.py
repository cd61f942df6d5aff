"""The RDS kernels (csrc/rds.hip) against the float64 oracle of tests/rds_model.py at every class of channel rate -- the
three LDS tiles the plans reach (64, 32, 16 outputs per workgroup), the shortest and the longest filters, R = 9 exactly --
from the first sample of a stream, over a partial last tile, cut into uneven blocks (against the oracle, not only against
itself), hours into a stream (``pos`` = 3 * 2^32 + 5), on silence and without a pilot; the whole chain at the two extreme
rates; and every finish-stage entry point on synthetic data at the lengths where its loops take another pass.  Streams
are a few tiles long: the oracle shares the kernels' zero initial state, so nothing settles.

Bounds (not widened): y within 1e-5 RMS and 1e-4 max of rms(y), q 2 pi 2^-44 within 1e-4 rad of the
oracle's dev, Phi exact and psi bit for bit on the GPU's own q.  Each test prints what it measured."""
from __future__ import annotations

import importlib.util
import math
import sys
from ctypes import c_double, c_int64
from pathlib import Path

import numpy as np
import pytest

from iq_to_audio_amd import dsp_plan as P

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

RMS_BOUND, MAX_BOUND, Q_BOUND = 1e-5, 1e-4, 1e-4
TWO44 = 2.0 ** 44

# rate -> (N, R, M, outputs per workgroup, ppm of the pilot)
RATES = {128_000.0: (185, 7, 216, 64, 40.0), 171_000.0: (247, 9, 288, 64, -40.0), 240_000.0: (347, 13, 405, 64, 40.0),
         10e6 / 21: (687, 25, 803, 64, -40.0), 960_000.0: (1385, 51, 1617, 32, 40.0), 1_420_000.0: (2047, 75, 2392, 16, -40.0)}
EDGE_RATES = [128_000.0, 960_000.0, 1_420_000.0]
EXTREME_RATES = [128_000.0, 1_420_000.0]
POS = 3 * 2 ** 32 + 5  # about 7.5 h into a 480 kHz stream


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def rms(a):
    return float(np.sqrt(np.mean(np.abs(np.asarray(a).astype(np.complex128)) ** 2)))


def lds_floats(N, Mh, R, tile):
    """The kernel header's statement: pilot window (tile R + N, + 1 of alignment), mixed window, pilot values."""
    return tile * R + N + 1 + 2 * ((tile - 1) * R + 1 + 2 * Mh) + 2 * (tile + 1)


def tile_of(fs):
    """The tile iqa_rds_lds_bytes reports for the plan of ``fs``, by the header's formula (None if it matches no tile)."""
    import iq_to_audio_amd as pkg

    plan = P.plan_rds(fs)
    N, R, Mh = plan.wfm.ntaps, plan.decim, plan.half
    lds = int(pkg.native.lib().iqa_rds_lds_bytes(N, Mh, R))
    hits = [t for t in (64, 32, 16, 8) if lds_floats(N, Mh, R, t) * 4 == lds]
    return hits[0] if len(hits) == 1 else None


def length(fs, pos=0, tile=None):
    """n such that the block holds nj = j0 + 3 tile + tile / 2 + 1 outputs (three full tiles past the start-up, half a
    tile, one more) and ends between two decimated instants."""
    plan = P.plan_rds(fs)
    R = plan.decim
    tile = RATES[fs][3] if tile is None else tile
    nj = plan.j0 + 3 * tile + tile // 2 + 1
    first = -(-pos // R) * R - pos
    return first + (nj - 1) * R + 1 + R // 2, nj


_cases: dict = {}


def case(fs, kind="rds", pos=0, tile=None):
    """(theta, oracle) of one rate and position, computed once and shared read-only."""
    key = (fs, kind, pos)
    if key not in _cases:
        n, nj = length(fs, pos, tile)
        if kind == "rds":
            m, _ = M.multiplex(fs, n / fs, ppm=RATES.get(fs, (0, 0, 0, 0, 40.0))[4], sigma=0.01, seed=5)
            assert m.size == n
        else:  # a programme without a pilot: a 400 Hz tone
            m = 0.5 * np.sin(2 * np.pi * 400.0 * np.arange(n) / fs)
        theta = M.theta_of(m, fs)
        theta.setflags(write=False)
        want = M.oracle_baseband(theta, fs, pos=pos)
        assert want["y"].size == nj
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cases[key] = (theta, want)
    return _cases[key]


def run(fs, theta, cuts=None, pos=0):
    """``theta`` through one fresh RdsCore that starts at absolute index ``pos``, cut at ``cuts``: host copies of the
    stored y, q, Phi, psi, and the number of blocks that launched nothing."""
    import iq_to_audio_amd as pkg
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.decoders.rds import RdsCore

    plan = P.plan_rds(fs)
    core = RdsCore(plan)
    core.pos = pos
    th = D.to_device(np.array(theta), "float32")
    n = int(theta.size)
    cuts = [0, n] if cuts is None else cuts
    assert cuts[0] == 0 and cuts[-1] == n and all(hi > lo for lo, hi in zip(cuts[:-1], cuts[1:])), cuts
    counts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        counts.append(int(pkg.native.lib().iqa_rds_outputs(pos + lo, hi - lo, plan.decim)))
        core.process(th[lo:hi])
        assert len(core._store) == sum(1 for c in counts if c)
    assert core.pos == pos + n
    out = {k: v.cpu().numpy() for k, v in core.joined().items()}
    out["counts"] = counts
    out["total"] = int(core.total.cpu().numpy()[0])
    return out


def check_baseband(tag, fs, got, want, j0):
    """y and q from the j0-th output on against the oracle; in front of it (the pilot phasor is ill-conditioned while its
    filter fills) only the shape, finiteness and q[0] = 0."""
    y, q = got["y"], got["q"]
    assert y.shape == want["y"].shape and y.dtype == np.complex64 and q.shape == want["q"].shape and q.dtype == np.int64
    assert np.all(np.isfinite(y.view(np.float32))) and q[0] == 0
    assert np.abs(q).max() <= 2 ** 43  # |dev| <= pi
    scale = rms(want["y"][j0:])
    err = y[j0:].astype(np.complex128) - want["y"][j0:]
    dq = q[j0:].astype(np.float64) * (2.0 * np.pi / TWO44) - want["dev"][j0:]
    e_rms, e_max = rms(err) / scale, float(np.abs(err).max()) / scale
    print(f"{tag} fs {fs:.0f} outputs {y.size} (from {j0}): rms(y) {scale:.4e}; y error rms {e_rms:.3e} max {e_max:.3e} of rms(y) "
          f"(at {int(np.argmax(np.abs(err))) + j0}); q 2 pi 2^-44 - dev rms {rms(dq):.3e} max {np.abs(dq).max():.3e} rad "
          f"(at {int(np.argmax(np.abs(dq))) + j0})")
    assert scale > 1e-4
    assert e_rms <= RMS_BOUND and e_max <= MAX_BOUND, (tag, fs, e_rms, e_max)
    assert np.abs(dq).max() <= Q_BOUND, (tag, fs, float(np.abs(dq).max()))


def check_clock(got, plan, j_first=0):
    """Phi is the integer sum of the GPU's own q and psi the float64 statement on it, bit for bit (the kernel and numpy
    round the same three float64 operations)."""
    phi, psi = M.oracle_clock(got["q"], plan, j_first=j_first)
    np.testing.assert_array_equal(got["phi"], phi)
    assert got["psi"].dtype == np.float64
    np.testing.assert_array_equal(got["psi"], psi)
    assert got["total"] == (int(phi[-1]) if phi.size else 0)


def cuts_for(n, h, R):
    """Cuts with: a first block shorter than the history; a block of one sample; a block between two multiples of R (no
    output, no launch); a block of one sample that holds exactly one decimated instant; a block of R samples that holds
    exactly one; a block longer than the history where the stream has room for it (the longest filter's has not); a block of
    half the history (the ``cat([prev[n:], theta])`` path: the block behind it needs what was carried in front of it);
    a last block of R + 2 samples, which holds an output."""
    c1 = h // 8 + 3
    c2 = c1 + 1
    c3 = -(-c2 // R) * R + 1  # = 1 mod R
    c4 = c3 + R - 1  # [c3, c4) holds no multiple of R; c4 is one
    c5 = c4 + 1
    c6 = c5 + R
    c7 = c6 + h + R + 7
    last = n - R - 2
    c8 = last - h // 2
    cuts = [0, c1, c2, c3, c4, c5, c6] + ([c7] if c7 < c8 else []) + [c8, last, n]
    assert all(hi > lo for lo, hi in zip(cuts[:-1], cuts[1:])), (cuts, h, R)
    assert c1 < h and c3 % R == 1 and c4 % R == 0 and last - c8 < h, (cuts, h, R)
    return cuts


@pytest.mark.parametrize("fs", list(RATES))
def test_rate_classes_against_the_oracle(A, fs):
    N, R, Mh, tile, _ = RATES[fs]
    plan = P.plan_rds(fs)
    assert (plan.wfm.ntaps, plan.decim, plan.half) == (N, R, Mh)
    assert tile_of(fs) == tile, "the picker moved: this rate no longer covers the tile it is here for"
    assert lds_floats(N, Mh, R, tile) * 4 <= 64 * 1024 - 64 < lds_floats(N, Mh, R, 2 * tile) * 4 or tile == 64
    theta, want = case(fs)
    got = run(fs, theta)
    nj = plan.j0 + 3 * tile + tile // 2 + 1
    assert got["y"].size == nj == got["counts"][0] and theta.size % R != 0
    print(f"fs {fs:.0f}: N {N} R {R} M {Mh} tile {tile}, n {theta.size}, outputs {nj}, j0 {plan.j0}")
    check_baseband("one block", fs, got, want, plan.j0)
    check_clock(got, plan)


@pytest.mark.parametrize("fs", EDGE_RATES)
def test_uneven_blocks_against_the_oracle(A, fs):
    plan = P.plan_rds(fs)
    theta, want = case(fs)
    cuts = cuts_for(theta.size, plan.hist_len, plan.decim)
    got = run(fs, theta, cuts)
    counts = got["counts"]
    print(f"fs {fs:.0f}: cuts {cuts}, outputs per block {counts}")
    assert counts[3] == 0 and counts[4] == 1 and counts[5] == 1 and cuts[5] - cuts[4] == 1 and cuts[6] - cuts[5] == plan.decim
    assert sum(counts) == want["y"].size and counts[-1] >= 1
    assert fs == 1_420_000.0 or max(hi - lo for lo, hi in zip(cuts[:-1], cuts[1:])) > plan.hist_len
    check_baseband("blocks", fs, got, want, plan.j0)
    check_clock(got, plan)
    one = run(fs, theta)
    for key in ("y", "q", "phi", "psi"):
        np.testing.assert_array_equal(got[key], one[key], err_msg=key)


@pytest.mark.parametrize("fs", [480_000.0, 1_420_000.0])
def test_absolute_position(A, fs):
    """A stream that starts at absolute index 3 * 2^32 + 5 (not a multiple of R): the mixer phase and the clock come from
    the absolute index in float64, the outputs are j >= ceil(pos / R), dev of the first is 0."""
    plan = P.plan_rds(fs)
    tile = tile_of(fs)
    assert tile == (64 if fs == 480_000.0 else 16) and POS % plan.decim != 0
    theta, want = case(fs, pos=POS, tile=tile)
    j_first = -(-POS // plan.decim)
    assert want["j_first"] == j_first and j_first > 2 ** 27
    got = run(fs, theta, pos=POS)
    check_baseband(f"pos {POS}", fs, got, want, plan.j0)
    check_clock(got, plan, j_first=j_first)


@pytest.mark.parametrize("fs", EXTREME_RATES)
def test_whole_chain_at_the_extreme_rates(A, fs):
    from iq_to_audio_amd.decoders.rds import RdsDecoder, parse_groups

    m, sent = M.multiplex(fs, 0.5, ppm=RATES[fs][4], sigma=0.01, seed=7)
    theta = M.theta_of(m, fs)
    full = M.oracle_chain(theta, fs)
    dec = RdsDecoder(fs)
    dec.process(theta)
    st = dec.stages()
    print(f"fs {fs:.0f}: tau {st['tau']:+.6f} (oracle {full['tau']:+.6f}), strength {st['strength']:.4f} (oracle "
          f"{full['strength']:.4f}), bits {st['bits'].size}, k_first {st['k_first']}")
    assert abs(st["tau"] - full["tau"]) < 1e-4 and abs(st["strength"] - full["strength"]) < 1e-4
    assert st["k_first"] == full["k_first"] and st["symbols"].size == full["symbols"].size
    assert full["bits"].size > 500
    np.testing.assert_array_equal(st["bits"], full["bits"])
    np.testing.assert_array_equal(st["words"], full["words"])
    np.testing.assert_array_equal(st["syndromes"], full["syndromes"])
    got, ref = dec.finish(), parse_groups(full["words"], full["syndromes"])
    assert ref.groups >= 3 and got is not None and got.group_offsets == ref.group_offsets
    assert got.pi == ref.pi == M.PI


@pytest.mark.parametrize("fs", EXTREME_RATES)
def test_silence(A, fs):
    """theta = 0: y, q and Phi are exactly 0 (u is 0 where |p| < 1e-12, dev is 0 where the phasor product is 0: no 0 / 0)."""
    n, nj = length(fs)
    got = run(fs, np.zeros(n, np.float32))
    assert got["y"].size == nj
    assert np.all(got["y"] == 0) and np.all(got["q"] == 0) and np.all(got["phi"] == 0) and got["total"] == 0
    check_clock(got, P.plan_rds(fs))


@pytest.mark.parametrize("fs", EXTREME_RATES)
def test_composite_without_a_pilot(A, fs):
    """A 400 Hz tone: u is the phase of filter leakage, so y and q are only finite and in range -- and the same bit for
    bit when the stream is cut into blocks."""
    plan = P.plan_rds(fs)
    theta, _ = case(fs, "mono")
    got = run(fs, theta)
    assert np.all(np.isfinite(got["y"].view(np.float32))) and np.abs(got["q"]).max() <= 2 ** 43 and got["q"][0] == 0
    assert np.all(np.isfinite(got["psi"]))
    check_clock(got, plan)
    cut = run(fs, theta, cuts_for(theta.size, plan.hist_len, plan.decim))
    for key in ("y", "q", "phi", "psi"):
        np.testing.assert_array_equal(cut[key], got[key], err_msg=key)


# ---- the finish-stage entry points on synthetic data -------------------------------------------------------------------

STEP = 0.9895833333333334  # 19 000 * 25 / 480 000


def _clock(q_dev, n, j_first, step, total_dev):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as Nat

    chunks = int(Nat.lib().iqa_rds_clock_chunks(n))
    assert chunks == -(-n // 4096)
    work = D.empty(chunks, "int64")
    phi, psi = D.empty(n + 8, "int64").fill_(-7), D.empty(n + 8, "float64").fill_(-7.0)
    Nat.call("iqa_rds_clock", Nat.ptr(q_dev), c_int64(n), c_int64(j_first), c_double(step), Nat.ptr(total_dev), Nat.ptr(work),
             Nat.ptr(phi), Nat.ptr(psi), Nat.stream_ptr())
    phi, psi = phi.cpu().numpy(), psi.cpu().numpy()
    assert np.all(phi[n:] == -7) and np.all(psi[n:] == -7.0)  # nothing written past n
    return phi[:n], psi[:n]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096, 4097, 256 * 4096 + 4097])
def test_clock_scan(A, n):
    """Two calls in a row on one carried total, preset to -2^50, q uniform in [-2^43, 2^43], first output 3 * 2^28: Phi is
    total + cumsum(q) exactly across both calls and psi = ((j step) + (Phi 2^-44)) 0.0625 in that order, bit for bit.  The
    last length has more than 256 chunks: the sums in front of a chunk and the carry take a second pass."""
    from iq_to_audio_amd import _dev as D

    rng = np.random.default_rng(n)
    j_first, total0 = 3 * 2 ** 28, -(2 ** 50)
    total = D.to_device(np.array([total0], np.int64), "int64").clone()
    start = total0
    for call in range(2):
        q = rng.integers(-(2 ** 43), 2 ** 43, size=n, endpoint=True, dtype=np.int64)
        phi, psi = _clock(D.to_device(q, "int64"), n, j_first, STEP, total)
        want_phi = start + np.cumsum(q)
        j = np.arange(n, dtype=np.float64) + float(j_first)
        want_psi = ((j * STEP) + (want_phi.astype(np.float64) * 2.0 ** -44)) * 0.0625
        bad = np.nonzero(phi != want_phi)[0]
        assert bad.size == 0, (call, n, int(bad[0]), int(bad.size))
        np.testing.assert_array_equal(psi, want_psi)
        start = int(want_phi[-1])
        assert int(total.cpu().numpy()[0]) == start
        j_first += n


def _timing(y, psi, n, j0):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as Nat

    tiles = int(Nat.lib().iqa_rds_timing_partials(n))
    assert tiles == -(-n // 1024)
    partials = D.empty(3 * tiles, "float64").fill_(float("nan"))
    z = D.empty(3, "float64").fill_(float("nan"))
    Nat.call("iqa_rds_timing", Nat.ptr(y), Nat.ptr(psi), c_int64(n), c_int64(j0), Nat.ptr(partials), Nat.ptr(z), Nat.stream_ptr())
    return z.cpu().numpy()


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 256 * 1024 + 1025])
def test_timing_sums(A, n):
    """Z and sum |y|^2 against math.fsum of the float64 terms.  Bound 1e-13 sum|y|^2 per component: a term has a few ulps
    of relative error, a thread adds at most 4 terms per tile and at most 2 tile partials, two four-way adds follow:
    under about 20 * 2^-53 sum|y|^2; the bound is roughly 50 times that.  The last length has more than 256 tiles."""
    from iq_to_audio_amd import _dev as D

    rng = np.random.default_rng(n)
    yh = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    psih = np.cumsum(rng.uniform(0.1, 1.0, size=n))
    psih *= 999_999.3 / psih[-1]
    assert np.all(np.diff(psih) > 0) and 9.0e5 < psih[-1] <= 1.0e6
    y, psi = D.to_device(yh, "complex64"), D.to_device(psih, "float64")
    e = yh.real.astype(np.float64) ** 2 + yh.imag.astype(np.float64) ** 2
    fr = psih - np.floor(psih)
    zr, zi = e * np.cos(2.0 * np.pi * fr), -e * np.sin(2.0 * np.pi * fr)
    for j0 in sorted({0, min(119, n - 1), n - 1, n}):
        got = _timing(y, psi, n, j0)
        want = [math.fsum(zr[j0:].tolist()), math.fsum(zi[j0:].tolist()), math.fsum(e[j0:].tolist())]
        bound = 1e-13 * want[2]
        print(f"timing n {n} j0 {j0}: error {[f'{abs(g - w):.2e}' for g, w in zip(got, want)]}, bound {bound:.2e}")
        if j0 == n:
            assert np.all(got == 0.0)
        for g, w in zip(got, want):
            assert abs(float(g) - w) <= bound, (n, j0, float(g), w, bound)


def _symbols(y_dev, psi_dev, psih, n, j0, tau, k_first=None, nsym=None):
    """iqa_rds_symbols with k_first and nsym as RdsCore.finish computes them (unless given): host symbols, bits."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as Nat

    if k_first is None:
        k_first = int(math.floor(float(psih[j0]) - tau)) + 1
        nsym = int(math.floor(float(psih[n - 1]) - tau)) - k_first + 1
    sym, bits = D.zeros(nsym + 8, "complex64"), D.empty(nsym + 8, "uint8").fill_(9)
    Nat.call("iqa_rds_symbols", Nat.ptr(y_dev), Nat.ptr(psi_dev), c_int64(n), c_int64(j0), c_double(tau), c_int64(k_first),
             c_int64(nsym), Nat.ptr(sym), Nat.ptr(bits), Nat.stream_ptr())
    sym, bits = sym.cpu().numpy(), bits.cpu().numpy()
    assert np.all(sym[nsym:] == 0) and np.all(bits[nsym - 1 :] == 9)  # nothing written past nsym, nsym - 1
    return sym[:nsym], bits[: nsym - 1], k_first, nsym


def test_symbols_and_bits(A):
    """psi from the GPU clock at n = 4097 + 300 and step 0.99 (each step of psi in (0.03, 0.1)), random y, three timing
    offsets, j0 = 0 and 119: every symbol is the float64 statement of the kernel header within one float32 ulp of
    max(|y[j-1]|, |y[j]|) per component, every slot is filled, none comes from j <= j0, and the bits are the sign of
    Re(s[i+1] conj(s[i])) of the GPU's own symbols."""
    from iq_to_audio_amd import _dev as D

    n = 4097 + 300
    rng = np.random.default_rng(44)
    q = rng.integers(-(2 ** 43), 2 ** 43, size=n, endpoint=True, dtype=np.int64)
    total = D.zeros(1, "int64")
    _, psih = _clock(D.to_device(q, "int64"), n, 0, STEP, total)
    steps = np.diff(psih)
    assert 0.03 < steps.min() and steps.max() < 0.1
    yh = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    # y and psi sit behind a NaN each: a read of index j0 - 1 = -1 shows as NaN, not as a fault
    yg = D.to_device(np.concatenate([np.array([np.nan + 0j], np.complex64), yh]), "complex64")
    pg = D.to_device(np.concatenate([np.array([np.nan]), psih]), "float64")
    y_dev, psi_dev = yg[1:], pg[1:]
    y64 = yh.astype(np.complex128)

    def expected(tau, j0):
        r = psih - tau
        fl = np.floor(r)
        j = np.nonzero(fl[1:] > fl[:-1])[0] + 1
        j = j[j > j0]
        k = fl[j]
        s = y64[j - 1] + (y64[j] - y64[j - 1]) * ((k - r[j - 1]) / (r[j] - r[j - 1]))
        tol = np.spacing(np.maximum(np.abs(yh[j - 1]), np.abs(yh[j])).astype(np.float32))
        return j, k.astype(np.int64), s, tol.astype(np.float64)

    def check(sym, bits, k_first, j, k, s, tol, slots):
        assert np.all(np.diff(k) == 1) and k.size == slots.size and np.all(k - k_first == slots)
        assert np.all((sym[slots].real != 0) | (sym[slots].imag != 0))  # no slot stays at its zero fill
        want = s.astype(np.complex64)
        assert np.all(np.abs(sym[slots].real.astype(np.float64) - want.real) <= tol)
        assert np.all(np.abs(sym[slots].imag.astype(np.float64) - want.imag) <= tol)
        s64 = sym.astype(np.complex128)
        np.testing.assert_array_equal(bits, (np.real(s64[1:] * np.conj(s64[:-1])) < 0).astype(np.uint8))

    for j0 in (0, 119):
        for tau in (0.0, 0.37, -0.49):
            sym, bits, k_first, nsym = _symbols(y_dev, psi_dev, psih, n, j0, tau)
            j, k, s, tol = expected(tau, j0)
            assert nsym == k.size > 250 and j.min() > j0
            check(sym, bits, k_first, j, k, s, tol, np.arange(nsym))
    # a symbol boundary exactly at j0 (floor(r[j0]) > floor(r[j0 - 1])) with room for it in the output (k_first one lower
    # than finish() passes): that slot stays empty, the symbol would come from j = j0
    j0 = 119
    mid = 0.5 * (psih[j0 - 1] + psih[j0])
    tau = mid - math.floor(mid)
    assert math.floor(psih[j0] - tau) > math.floor(psih[j0 - 1] - tau)
    k_first = int(math.floor(psih[j0] - tau))
    nsym = int(math.floor(psih[n - 1] - tau)) - k_first + 1
    sym, bits, _, _ = _symbols(y_dev, psi_dev, psih, n, j0, tau, k_first, nsym)
    j, k, s, tol = expected(tau, j0)
    assert k[0] == k_first + 1 and k.size == nsym - 1
    assert sym[0] == 0, "a symbol from j = j0"
    check(sym, bits, k_first, j, k, s, tol, np.arange(1, nsym))


@pytest.mark.parametrize("nbits", [25, 26, 27, 281, 282, 10_007])
def test_syndromes(A, nbits):
    """Random bits with valid blocks spliced in at odd offsets: W and S equal the model's; a spliced block's syndrome is
    its offset word; fewer than 26 bits write nothing, and nothing is written past nbits - 25."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as Nat

    rng = np.random.default_rng(nbits)
    bits = rng.integers(0, 2, size=nbits).astype(np.uint8)
    spliced = []
    for i, (at, name) in enumerate([(1, "A"), (33, "B"), (255, "C"), (1001, "C'"), (5555, "D"), (nbits - 26, "A")]):
        if at >= 0 and at + 26 <= nbits and all(abs(at - o) >= 26 for o, _ in spliced):
            w = M.block(int(rng.integers(0, 1 << 16)), name)
            bits[at : at + 26] = [(w >> (25 - b)) & 1 for b in range(26)]
            spliced.append((at, name))
    assert len(spliced) >= (1 if nbits >= 26 else 0) and (nbits < 10_000 or len(spliced) == 6)
    nw = max(nbits - 25, 0)
    words, synd = D.empty(nw + 8, "int32").fill_(-3), D.empty(nw + 8, "int16").fill_(-3)
    Nat.call("iqa_rds_syndromes", Nat.ptr(D.to_device(bits, "uint8")), c_int64(nbits), Nat.ptr(words), Nat.ptr(synd), Nat.stream_ptr())
    words, synd = words.cpu().numpy(), synd.cpu().numpy()
    assert np.all(words[nw:] == -3) and np.all(synd[nw:] == -3)
    want_w, want_s = M.words_and_syndromes(bits)
    assert want_w.size == nw
    np.testing.assert_array_equal(words[:nw].view(np.uint32).astype(np.int64), want_w)
    np.testing.assert_array_equal(synd[:nw].view(np.uint16).astype(np.int64), want_s)
    for at, name in spliced:
        assert int(synd[at]) == M.OFFSETS[name], (at, name)
