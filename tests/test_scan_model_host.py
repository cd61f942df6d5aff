"""CPU checks of tests/scan_model.py, the per-sample oracle of the demodulator's scan engine: each float64 recurrence
against the same recurrence run sequentially in np.longdouble (the oracle's own error stays inside a quarter of the
floor term the GPU tests allow), against the reference's float32 loops (oracle/cpu_ref.py) at the bounds
tests/test_gpu_parity.py uses, and the structure of the segmented AGC.  No GPU, nothing from the product."""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import cpu_ref as O


def _load_model():
    name = "scan_model"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name("scan_model.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load_model()

LD = np.longdouble
N_LOOP = 12_000  # the longdouble loops are Python loops: the classes at a reduced size (their zero stretches included)


def _ld_deemphasis(x, alpha, y_prev=0.0):
    a, b, y = LD(alpha), LD(1.0 - alpha), LD(y_prev)
    out = np.empty(x.size, dtype=LD)
    for i, s in enumerate(x.astype(LD)):
        y = b * s + a * y
        out[i] = y
    return out


def _ld_dc(x, radius, x_prev=0.0, y_prev=0.0):
    r, y = LD(np.float32(radius)), LD(y_prev)
    d = x - np.concatenate(([np.float32(x_prev)], x[:-1])).astype(np.float32)  # the float32 difference
    assert d.dtype == np.float32
    out = np.empty(x.size, dtype=LD)
    for i, s in enumerate(d.astype(LD)):
        y = s + r * y
        out[i] = y
    return out


def _ld_agc_gain(x, restarts, target=M.AGC_TARGET, decay=M.AGC_DECAY):
    tf, df = np.float32(target), LD(np.float32(decay))
    rs = set(int(r) for r in restarts)
    g = LD(1.0)
    out = np.empty(x.size, dtype=LD)
    for i, s in enumerate(x):
        if i in rs:
            g = LD(1.0)
        mag = np.abs(s)
        if mag > M.AGC_THRESHOLD:
            g = g + df * (LD(tf / mag) - g)
        out[i] = g
    return out


def _classes(op):
    return {"deemph": ("a", "b", "c", "f"), "dc": ("a", "b", "c", "e", "f"), "agc": ("a", "b", "c", "d", "f")}[op]


@pytest.mark.parametrize("cls", _classes("deemph"))
def test_deemphasis_f64_within_quarter_floor_of_longdouble(cls):
    x = M.make_x("deemph", cls, N_LOOP)
    blk = M.stage_deemphasis(x, M.ALPHA, 0.37)
    err = np.abs(blk.y64.astype(LD) - _ld_deemphasis(x, M.ALPHA, 0.37)).max()
    assert float(err) <= blk.F / 4, (cls, float(err), blk.F)


@pytest.mark.parametrize("cls", _classes("dc"))
def test_dc_block_f64_within_quarter_floor_of_longdouble(cls):
    x = M.make_x("dc", cls, N_LOOP)
    blk = M.stage_dc(x, M.DC_RADIUS, 0.125, -0.4)
    err = np.abs(blk.y64.astype(LD) - _ld_dc(x, M.DC_RADIUS, 0.125, -0.4)).max()
    assert float(err) <= blk.F / 4, (cls, float(err), blk.F)


@pytest.mark.parametrize("cls", _classes("agc"))
@pytest.mark.parametrize("lay", ["single", "stair", "tile"])
def test_agc_gain_f64_within_quarter_floor_of_longdouble(cls, lay):
    x = M.make_x("agc", cls, N_LOOP)
    restarts = M.layout(lay, N_LOOP)
    blk = M.stage_agc(x, restarts)
    err = np.abs(blk.extra["gain"].astype(LD) - _ld_agc_gain(x, restarts)).max()
    assert float(err) <= blk.F / 4, (cls, lay, float(err), blk.F)


def test_floor_term_is_far_below_a_float32_ulp():
    """F is what a correct scan may differ by; a wrong carry, restart or neighbour sample leaves at least a float32 ulp."""
    for pole in (M.ALPHA, float(np.float32(M.DC_RADIUS)), 1.0 - float(np.float32(M.AGC_DECAY))):
        assert M.floor_term(1.0, pole) < 1e-11 and M.floor_term(1.0, pole) < 2.0 ** -23 * 1e-4  # four orders under an ulp of S


def test_deemphasis_agrees_with_the_reference_filter_and_streams():
    x = M.make_x("deemph", "a", 50_000)
    st = O.DeemphState(M.ALPHA)
    want = np.concatenate([O.deemphasis(x[:1234], st), O.deemphasis(x[1234:], st)])
    y = M.deemphasis(x, M.ALPHA)
    np.testing.assert_array_equal(y.astype(np.float32), want)
    head = M.deemphasis(x[:1234], M.ALPHA)
    tail = M.deemphasis(x[1234:], M.ALPHA, head[-1])
    np.testing.assert_array_equal(np.concatenate([head, tail]), y)  # the carried state is y[last], bit for bit


def test_dc_block_agrees_with_the_float32_reference_loop():
    rng = np.random.default_rng(20)
    x = rng.normal(size=5000).astype(np.float32)
    st = O.DcState()
    want = np.concatenate([O.dc_block(x[:1234], st), O.dc_block(x[1234:], st)])
    y = M.dc_block(x)
    # float64 recurrence vs the reference's float32 sequential loop: the bound of test_dc_blocker_and_agc
    np.testing.assert_allclose(y.astype(np.float32), want, rtol=0, atol=2e-5)
    head = M.dc_block(x[:1234])
    tail = M.dc_block(x[1234:], M.DC_RADIUS, x[1233], head[-1])
    np.testing.assert_array_equal(np.concatenate([head, tail]), y)
    # and the existing float64 statement (float32 out) is this one rounded
    st64 = O.DcState()
    np.testing.assert_array_equal(O.ssb_demod_f64(x.astype(np.complex64), st64, agc_enabled=False), y.astype(np.float32))
    assert st64.y_prev == y[-1] and st64.x_prev == float(x[-1])


def test_agc_agrees_with_the_float32_reference_loop():
    rng = np.random.default_rng(20)
    x = (rng.normal(size=2000) * 0.01).astype(np.float32)
    blk = M.stage_agc(x)
    np.testing.assert_allclose(blk.v, O.agc(x), rtol=2e-5, atol=1e-6)  # the bound of test_dc_blocker_and_agc
    assert np.abs(blk.y64 - blk.v).max() <= (3 * M.EPS32 * np.abs(blk.y64)).max()


@pytest.mark.parametrize("cls", ["c", "d"])
@pytest.mark.parametrize("lay", ["stair", "tile", "tile-1", "tile+1", "c5", "last"])
def test_segmented_agc_has_the_structure_of_the_reference_per_call(cls, lay):
    """The same samples hold and the same samples restart as O.agc applied segment by segment: a held sample leaves the
    reference's output at x * (the gain before it), the first sample of every segment sees a gain that started at 1.0."""
    n = 30_000
    x = M.make_x("agc", cls, n)
    restarts = M.layout(lay, n)
    g, held = M.agc_gain(x, restarts)
    b = M.restart_bounds(n, restarts)
    ref = np.concatenate([O.agc(x[lo:hi]) for lo, hi in zip(b[:-1], b[1:])])
    # holds: |x| <= float32(1e-6) exactly, and there the gain does not move (in the reference: output == x * previous gain)
    np.testing.assert_array_equal(held, np.abs(x) <= M.AGC_THRESHOLD)
    starts = np.zeros(n, dtype=bool)
    starts[b[:-1]] = True
    prev_g = np.concatenate(([1.0], g[:-1]))
    prev_g[starts] = 1.0
    assert np.array_equal(g[held], prev_g[held])
    assert held.sum() > 0 and (held & starts).sum() > 0, "a restart must land on a held sample in this case"
    # restarts: the first sample of a segment moves from 1.0 exactly as one step of the recurrence
    first = b[:-1][~held[b[:-1]]]
    tf, df = np.float32(M.AGC_TARGET), float(np.float32(M.AGC_DECAY))
    np.testing.assert_array_equal(g[first], 1.0 + df * ((tf / np.abs(x[first])).astype(np.float64) - 1.0))
    # and the values follow the float32 loop (its own rounding: 1 / decay steps of float32 error)
    live = ~held
    np.testing.assert_allclose((x * g.astype(np.float32))[live], ref[live], rtol=2e-4, atol=1e-9)
    np.testing.assert_array_equal((x * g.astype(np.float32))[held & starts], ref[held & starts])  # gain 1.0: x itself


def test_threshold_neighbours_straddle_the_hold():
    v = M.threshold_values()
    _, held = M.agc_gain(v)
    assert held.tolist() == [True, True, False, True, True, False]  # at and below float32(1e-6) hold, its upper neighbour moves


def test_sink_counts_every_sample_once_and_empty_segments_are_zero():
    v = M.make_x("clip", "f", 10_000)
    for lay in M.LAYOUTS:
        s = M.layout(lay, v.size)
        k = M.sink(v, s)
        assert k.sums.size == s.size
        assert np.isclose(k.sums.sum(), np.sum(v.astype(np.float64) ** 2), rtol=1e-13, atol=0)
        if lay == "dup":
            assert k.sums[1] == 0.0 and k.sums[2] > 0.0
    k = M.sink(v, [0])
    assert k.peak > 0.99 and np.abs(k.audio).max() == M.CLIP and k.peak == np.abs(v).max()
    assert np.array_equal(k.audio, np.clip(v, -0.99, 0.99).astype(np.float32))
    assert np.array_equal(k.audio, O.writer_clip(v, 0.0)[0]) and float(k.peak) == O.writer_clip(v, 0.0)[1]


def test_source_stages_are_the_reference_statements():
    z = M.make_z("b", 5000)
    st = O.QuadState()
    np.testing.assert_array_equal(M.quadrature(z), O.quadrature(z, st))
    np.testing.assert_array_equal(M.quadrature(z[100:], z[99]), O.quadrature(z, O.QuadState())[100:])
    assert M.envelope(z).dtype == np.float32 and M.real_part(z).dtype == np.float32
    # zeros reach atan2(0, 0) = 0 (class c keeps the products at +0 +0j)
    zc = M.make_z("c", 30_000)
    q = M.quadrature(zc)
    assert (zc == 0).sum() >= 8 + 2048 + 1 + 5000 and zc[0] == 0 and zc[-1] == 0
    assert np.all(q[zc == 0] == 0.0) and not np.signbit(q[zc == 0]).any()


# every (class, n) the GPU matrix runs through the discriminator: the modulo-2-pi rule is the ONLY exclusion from a
# per-sample comparison and must apply to fewer than 1 in 10 000 samples of a run
SIZES = (1, 2, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4097, 131_071, 131_073, 300_001, 2_097_152, 2_097_153, 2_099_205, 5_769_231)


@pytest.mark.parametrize("cls", M.CLASSES_Z)
def test_modulo_two_pi_rule_stays_under_the_exclusion_cap(cls):
    for n in SIZES:
        if n > 2_200_000 and cls != "a":
            continue  # the config-2 block runs class (a) only
        hits = int(M.near_pi(M.quadrature(M.make_z(cls, n))).sum())
        assert hits * 10_000 < n, (cls, n, hits)


def test_layouts_and_shape_classes():
    assert [M.per_thread_tiles(n) for n in (2_097_152, 2_097_153, 2_099_205, 5_769_231)] == [1, 2, 2, 3]
    c5 = M.layout("c5", 5_769_231)
    assert set(np.diff(c5)) == {2012, 2013} and c5[1] == 2013
    per_tile = np.bincount(c5[1:] // M.TILE)
    assert set(per_tile) == {1, 2}  # `simple` and `general` tiles
    assert M.layout("s100", 131_071).size == 1000 and M.layout("stair", 4097).size > 20
    assert M.layout("last", 2049).tolist() == [0, 2048]
    assert M.layout("prod", 300_001).tolist() == [0, 40_330, 80_660, 120_990, 161_320, 201_650, 241_980, 282_310]
    assert [hi - lo for lo, hi in M.stream_blocks(300_001)][:6] == list(M.STREAM_CUTS)
    for lay in M.LAYOUTS:
        for n in SIZES[:14]:
            s = M.layout(lay, n)
            assert s[0] == 0 and s[-1] < n and np.all(np.diff(s) >= 0)
