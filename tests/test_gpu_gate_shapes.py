"""iqa_gate_power, iqa_gate_decide and iqa_gate_apply on the MI355X at their edge shapes, on hand-made
inputs: every value equals the numpy oracle's (tests/gate_model.py), and what the oracle must give is asserted first.  Call
lengths and positions around the cell and the tile, positions past 2^35, calls that cut cells, the extreme shifts, the
quantiser's clamp, ties and non-finite values, a guard entry behind the cells; frame counts around the floor's rank and the
state kernel's chunk of 1024, short and long last frames, every rule at equality, hold chains across a chunk edge, runs at both
ends, the largest and smallest frame; ramps of zero length and longer than half a run, unaligned buffers and odd lengths."""
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


G = _load("gate_model")
GUARD = 0x5A5A5A5A5A5A5A5A
STAGES = ("v", "s", "s2", "g", "lo", "hi")


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def stream(seed: int, n: int, scale: float = 300.0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def gpu_cells(z, pos: int, sh: int) -> np.ndarray:
    """The entry point's cells; a guard entry behind them must come back untouched."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    z = np.ascontiguousarray(z, dtype=np.complex64)
    k = int(N.lib().iqa_gate_cells(pos, z.size))
    assert k == G.n_cells(pos, z.size)
    out = D.from_numpy(np.full(k + 1, GUARD, dtype=np.int64))
    z_dev = D.from_numpy(z)  # (held in a name until the cells are read back)
    N.call("iqa_gate_power", N.ptr(z_dev), c_int64(z.size), c_int64(pos), c_int32(sh), N.ptr(out), N.stream_ptr())
    got = out.cpu().numpy()
    assert got[k] == GUARD, "the guard entry was written"
    return got[:k]


def check_cells(z, pos: int, sh: int) -> np.ndarray:
    want = G.cells(z, pos, sh)
    np.testing.assert_array_equal(gpu_cells(z, pos, sh), want)
    return want


# ---- iqa_gate_power -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("pos", (0, 1, 255, 256, 1000, 2047, 2048, (1 << 35) + 1000))
def test_power_lengths_and_positions(A, pos):
    z = stream(pos % 97, 3 * 2048 + 5)
    for n in (1, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 5):
        want = check_cells(z[:n], pos, 0)
        assert int(want.sum()) == int(G.power(z[:n], 0).sum()) and want.size == (pos + n - 1) // 256 - pos // 256 + 1


def test_power_cut_cells_add_up(A):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    z = stream(5, 6000)
    whole = G.cells(z, 0, 0)
    for cuts in ((6000,), (1, 5999), (255, 1, 1, 5743), (100,) * 60, (2047, 2, 2047, 1904), (256, 256, 5488)):
        parts, pos = [], 0
        total = D.zeros(whole.size, "int64")
        for k in cuts:
            part = gpu_cells(z[pos : pos + k], pos, 0)
            parts.append((pos // 256, part))
            part_dev = D.from_numpy(part)
            N.call("iqa_gate_add_cells", N.ptr(part_dev), c_int64(part.size), N.ptr(total[pos // 256 :]), N.stream_ptr())
            pos += k
        np.testing.assert_array_equal(G.add_cells(parts, 6000), whole)
        np.testing.assert_array_equal(total.cpu().numpy(), whole)


def test_power_shifts(A):
    base = stream(7, 700, 1.0)
    for sh, scale in ((-30, 2.0 ** 38), (0, 300.0), (30, 2.0 ** -22)):
        z = (base * np.float32(scale)).astype(np.complex64)
        want = check_cells(z, 300, sh)
        assert want.min() > 0 and G.quantise(z.real, sh).max() < 32767  # (neither silent nor clamped)


def test_power_clamp_ties_and_non_finite(A):
    re = np.array([32767.0, 32768.0, 1e9, -32767.0, -32768.0, -1e9, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, np.nan, np.inf, -np.inf, 32766.5, 32767.49], dtype=np.float32)
    assert G.quantise(re, 0).tolist() == [32767, 32767, 32767, -32767, -32767, -32767, 0, 2, 2, 0, -2, -2, 0, 32767, -32767, 32766, 32767]
    zr, zi = np.zeros(600, dtype=np.float32), np.zeros(600, dtype=np.float32)
    zr[: re.size] = zi[300 : 300 + re.size] = zr[400 : 400 + re.size] = zi[400 : 400 + re.size] = re
    z = np.empty(600, dtype=np.complex64)
    z.real, z.imag = zr, zi
    want = check_cells(z, 0, 0)
    assert want[0] == int((G.quantise(re, 0) ** 2).sum()) and want[1] == 3 * want[0]
    full = np.full(2048 + 256, 1e9 * (1 + 1j), dtype=np.complex64)  # every sample clamped: the largest cell there is
    want = check_cells(full, 0, 0)
    assert (want == 256 * 2 * 32767 ** 2).all() and 2 * 32767 ** 2 < 2 ** 31
    half = np.full(512, 0.25 + 0.75j, dtype=np.complex64)  # ties made by the shift: 0.5 -> 0, 1.5 -> 2
    assert check_cells(half, 0, 1).tolist() == [256 * 4, 256 * 4]
    assert check_cells(np.full(300, np.nan + 1j * np.nan, dtype=np.complex64), 100, 5).tolist() == [0, 0]


# ---- iqa_gate_decide ----------------------------------------------------------------------------------------------------------


def make_plan(Lf=256, M=5, H=38, A_=3, num_open=4077, num_close=2572, R=0):
    from iq_to_audio_amd import dsp_plan as P

    ramp = np.array([np.float32((k + 1) / (R + 1)) for k in range(R)], dtype=np.float32)
    return (P.GatePlan(fs=96000.0, frame=Lf, hang=H, min_frames=M, lead=A_, ramp_len=R, num_open=num_open, num_close=num_close, ramp=ramp),
            dict(fs=96000.0, Lf=Lf, M=M, H=H, A=A_, R=R, num_open=num_open, num_close=num_close, ramp=ramp))


def gpu_decide(cells, n: int, plan) -> dict:
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.gate import CarrierGate

    cells_dev = D.from_numpy(np.ascontiguousarray(cells, dtype=np.int64))
    out = CarrierGate.decide(cells_dev, n, plan)
    got = {k: t.cpu().numpy() for k, t in out.items()}
    got["floor"] = int(got["floor"][0])
    return got


def check_decide(cells, n: int, **opts) -> dict:
    plan, p = make_plan(**opts)
    want = G.decide(np.asarray(cells, dtype=np.int64), n, p)
    got = gpu_decide(cells, n, plan)
    assert got["floor"] == want["floor"]
    for k in STAGES:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    return want


def from_v(v) -> tuple:
    """(cells, n) at Lf = 256 whose frames come out as ``v`` exactly: v = 16 P / 256."""
    v = np.asarray(v, dtype=np.int64)
    return 16 * v, 256 * v.size


def busy_v(seed: int, F: int) -> np.ndarray:
    """A floor of about 1000 with bursts of every length, levels on either side of both thresholds."""
    rng = np.random.default_rng(seed)
    v = rng.integers(900, 1100, F)
    f = 0
    while f < F:
        f += int(rng.integers(1, 60))
        k = int(rng.choice([1, 2, 4, 9, 30, 49]))
        v[f : f + k] = rng.choice([2600, 3000, 3900, 4100, 6000, 20000], size=len(v[f : f + k]))
        v[f : f + 1] = 20000  # (the burst opens at once)
        f += k
    return v


@pytest.mark.parametrize("F", (1, 2, 10, 11, 255, 256, 257, 1023, 1024, 1025, 2049, 5000))
def test_decide_frame_counts(A, F):
    v = busy_v(F, F)
    want = check_decide(*from_v(v), M=3, H=7, A_=2)
    assert want["v"].tolist() == v.tolist() and want["floor"] == max(1, int(np.sort(v)[(F - 1) // 10]))
    if F >= 255:
        assert want["s"].any() and want["g"].any() and not want["g"].all()
    if F >= 256:
        assert (want["s"] != want["s2"]).any()  # a run shorter than M
    check_decide(*from_v(v))  # the defaults' M, H, A


def test_decide_short_and_long_last_frames(A):
    c = np.arange(1, 10, dtype=np.int64) * 1000
    assert check_decide(c[:1], 100, Lf=768)["v"].tolist() == [160]  # n < Lf
    assert check_decide(c[:6], 2 * 768 - 1, Lf=768)["v"].tolist() == [16 * 21000 // 1535]  # one long frame
    assert check_decide(c, 2 * 768 + 700, Lf=768)["v"].tolist() == [125, 16 * 39000 // 1468]
    assert check_decide(c[:1], 1, Lf=256)["v"].tolist() == [16000]


def test_decide_constant_descending_and_zero(A):
    for F in (1, 10, 300):
        flat = check_decide(*from_v(np.full(F, 5000)))
        assert flat["floor"] == 5000 and not flat["s"].any() and (flat["lo"] == -1).all()
        zero = check_decide(*from_v(np.zeros(F, dtype=np.int64)))
        assert zero["floor"] == 1 and not zero["g"].any()
    down = check_decide(*from_v(np.arange(3000, 0, -10)), M=1, H=0, A_=0)
    assert down["floor"] == int(np.sort(np.arange(3000, 0, -10))[29]) and down["s"][0] == 1 and down["s"][-1] == 0
    assert G.runs(down["s"]) == [(0, int(np.flatnonzero(1024 * np.arange(3000, 0, -10) >= 2572 * down["floor"])[-1]))]


def test_decide_thresholds_at_equality(A):
    for k in (1, 3, 1000):
        # twelve frames: rank 1 of the sorted values is the floor, 1024 k
        quiet = [1024 * k] * 8
        for pair, want_s in (([4077 * k, 2572 * k], [1, 1]), ([4077 * k - 1, 2572 * k], [0, 0]), ([4077 * k, 2572 * k - 1], [1, 0]),
                             ([4077 * k + 1, 4077 * k], [1, 1])):
            d = check_decide(*from_v([0] + quiet + pair + [1024 * k]), M=1, H=0, A_=0)
            assert d["floor"] == 1024 * k and d["s"][9:11].tolist() == want_s, (k, pair)
    d = check_decide(*from_v([0] * 10 + [4, 3, 2, 0]), M=1, H=0, A_=0)  # the floor clamped at 1
    assert d["floor"] == 1 and d["s"][9:].tolist() == [0, 1, 1, 0, 0]


def test_decide_minimum_duration_hang_and_lead_at_equality(A):
    M, H, A_ = 5, 38, 3
    for gap, merged in ((H + A_, True), (H + A_ + 1, False)):
        v = np.full(200, 1000)
        v[20 : 20 + M] = 9000
        second = 20 + M + gap
        v[second : second + M] = 9000
        v[150 : 150 + M - 1] = 9000  # one frame short: dropped
        d = check_decide(*from_v(v), M=M, H=H, A_=A_)
        assert G.runs(d["s"]) == [(20, 24), (second, second + M - 1), (150, 153)] and G.runs(d["s2"]) == [(20, 24), (second, second + M - 1)]
        assert G.runs(d["g"]) == ([(17, second + M - 1 + H)] if merged else [(17, 24 + H), (second - A_, second + M - 1 + H)])
    for M_, H_, A2 in ((1, 0, 0), (300, 0, 0), (1, 300, 0), (1, 0, 300), (1 << 20, 1 << 30, 1 << 30), (1, (1 << 31) - 1, (1 << 31) - 1)):
        v = np.full(200, 1000)
        v[[0, 199]] = 9000
        v[90:100] = 9000
        d = check_decide(*from_v(v), M=M_, H=H_, A_=A2)  # runs at both ends; M, H and A larger than F
        assert d["g"].all() == (M_ == 1 and (H_ >= 300 or A2 >= 300))


@pytest.mark.parametrize("edge", (1024, 2048))
def test_decide_hold_chains_across_a_chunk_edge(A, edge):
    for start, stop in ((edge - 1, edge), (edge - 40, edge + 40), (edge, edge + 1), (5, edge + 7), (edge - 1, edge - 1)):
        v = np.full(2 * edge + 100, 1000)
        v[start] = 9000  # opens
        v[start + 1 : stop + 1] = 3000  # neither opens nor closes: holds
        d = check_decide(*from_v(v), M=1, H=0, A_=0)
        assert G.runs(d["s"]) == [(start, stop)]
        d = check_decide(*from_v(v), M=stop - start + 1, H=edge, A_=edge)
        assert G.runs(d["s2"]) == [(start, stop)] and G.runs(d["g"]) == [(max(0, start - edge), min(v.size - 1, stop + edge))]
        assert not check_decide(*from_v(v), M=stop - start + 2, H=edge, A_=edge)["g"].any()
        v[start] = 3000  # nothing opens: the chain holds "closed"
        assert not check_decide(*from_v(v), M=1, H=0, A_=0)["s"].any()


def test_decide_smallest_and_largest_frame(A):
    Lf = 1 << 20
    n = 3 * Lf + 5
    cells = np.full(-(-n // 256), 256 * 1000, dtype=np.int64)
    cells[4096 : 2 * 4096] *= 8
    d = check_decide(cells, n, Lf=Lf, M=1, H=0, A_=0)
    assert d["v"].tolist() == [16000, 128000, (16 * (4097 * 256000)) // (Lf + 5)] and d["floor"] == 16000 and d["s"].tolist() == [0, 1, 0]
    d = check_decide(cells[:40], 40 * 256, Lf=256, M=1, H=0, A_=0)
    assert d["v"].size == 40 and not d["s"].any()


# ---- iqa_gate_apply -----------------------------------------------------------------------------------------------------------


def gpu_apply(a, g, lo, hi, n: int, p: dict, offset: int = 0) -> np.ndarray:
    """``offset``: floats by which both buffers are moved off their 16-byte alignment."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    a_dev = D.from_numpy(np.concatenate((np.zeros(offset, dtype=np.float32), np.asarray(a, dtype=np.float32))))
    out = D.from_numpy(np.full(offset + n + 8, 77.0, dtype=np.float32))
    g_dev, lo_dev, hi_dev = (D.from_numpy(np.ascontiguousarray(x)) for x in (g.astype(np.uint8), lo.astype(np.int32), hi.astype(np.int32)))
    ramp_dev = D.from_numpy(p["ramp"]) if p["R"] else None
    N.call("iqa_gate_apply", N.ptr(a_dev[offset:]), c_int64(n), c_int32(p["Lf"]), c_int32(g.size), N.ptr(g_dev), N.ptr(lo_dev), N.ptr(hi_dev),
           N.ptr(ramp_dev), c_int32(p["R"]), N.ptr(out[offset:]), N.stream_ptr())
    got = out.cpu().numpy()
    assert (got[:offset] == 77.0).all() and (got[offset + n :] == 77.0).all(), "written outside the output"
    return got[offset : offset + n]


@pytest.mark.parametrize("R", (0, 1, 100, 480, 700, 5000))
def test_apply_ramps_ends_and_odd_lengths(A, R):
    rng = np.random.default_rng(R)
    for n, Lf in ((256 * 12 + 5, 256), (256 * 12, 256), (768 * 4 + 767, 768), (3000, 768), (100, 768), (7, 256)):
        _, p = make_plan(Lf=Lf, R=R)
        F = max(1, n // Lf)
        for runs in ([(0, 1), (F - 1, F - 1)], [(0, F - 1)], [(1, 2)] if F > 3 else [], [(F - 1, F - 1)]):
            g = np.zeros(F, dtype=np.uint8)
            for a, b in runs:
                g[a : min(b, F - 1) + 1] = 1
            lo, hi = G.bounds(g)
            a = rng.standard_normal(n).astype(np.float32)
            a[::37] = np.nan
            gn = G.gain_loops(g, lo, hi, n, p)
            want = G.apply(a, g, lo, hi, p)
            # the oracle first: zero outside, the float32 product inside, the ramps inside the transmission
            open_ = g[np.minimum(np.arange(n) // Lf, F - 1)] != 0
            assert (want[~open_] == 0).all() and want.dtype == np.float32
            np.testing.assert_array_equal(want[open_], (a * gn)[open_])
            for s0, s1 in G.transmissions(g, n, Lf):
                assert gn[s0] == gn[s1 - 1] == (p["ramp"][0] if R else 1.0) and (gn[s0:s1] > 0).all()
                if s1 - s0 < 2 * R:  # a ramp longer than half the run: the two meet in the middle, below 1
                    assert gn[s0:s1].max() == p["ramp"][(s1 - s0 - 1) // 2] < 1.0
            for offset in (0, 1):
                got = gpu_apply(a, g, lo, hi, n, p, offset)
                finite = ~np.isnan(want)  # (bit for bit, -0.0 included; a NaN stays a NaN)
                np.testing.assert_array_equal(got.view(np.uint32)[finite], want.view(np.uint32)[finite])
                np.testing.assert_array_equal(np.isnan(got), ~finite)
