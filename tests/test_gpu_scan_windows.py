"""The one-launch form of the de-emphasis scan (csrc/demod_fused.hip: k_fused_windowed, k_fused_clear, scan_window) at
EVERY window the product reaches -- W = 512 ... 4096, and the three launches just past the largest -- against the float64
oracle of tests/scan_model.py, PER SAMPLE and PER CHUNK.  Run with ``-m gpu`` on an MI355X.

tests/test_gpu_scan_windowed.py pins the form at W = 1536 and 4096; each W splits a workgroup's four rounds differently into
warm-up-only threads, emitting threads and whole warm-up rounds, and gives block 0's state hand-off another round count.
Here the sizes of that file run at all eight windows, chunk starts are put ON the edges of a workgroup's own range
(scan_model.windowed_layout; tests/test_scan_windows_host.py proves the case matrix complete), the hand-off runs at one, two
and three warm-up rounds, and DeemphasisFilter runs at the rates the product runs it.

No bound is new: per sample |got - y64| <= 2^-24 |y64| + F with F = scan_model.floor_term for the pole in use (the state a
block ignores is at most 2^-64 S, and F >= 64 * 2^-53 S for every pole in (0, 1)), y_last within F, prev bit for bit, fused
== stages bit for bit, peak and sums as check_sink (check_sink_with_floor for inputs with stretches of exact zeros).  The
helpers are those of test_gpu_scan_exact.py and test_gpu_scan_windowed.py.  The window under test is reached with the pole
alpha = exp(-64 ln 2 / (W - 100)).  Every test prints, per window, the worst err / bound over samples (the outgoing state's
err / F among them) and over chunk sums: measurements, asserted no further than the bounds above.
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _load(name: str, file: str):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(file))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load("scan_model", "scan_model.py")
X = _load("_scan_exact_helpers", "test_gpu_scan_exact.py")        # device buffers, entry points, comparisons
WIN = _load("_scan_windowed_helpers", "test_gpu_scan_windowed.py")  # SIZES, check_sink_with_floor, window()
HOST = _load("_scan_windows_host", "test_scan_windows_host.py")    # the alphas of the host test
G = X.G

WORST = {}  # window -> [worst sample err / bound, worst chunk-sum err / bound] over what has run


def _note(W, label, sample=0.0, chunk=0.0):
    w = WORST.setdefault(W, [0.0, 0.0])
    w[0], w[1] = max(w[0], sample), max(w[1], chunk)
    print(f"[scan-windows] W={W} {label}: sample err/bound {sample:.3f}, chunk-sum err/bound {chunk:.3e}; "
          f"worst so far at this W: {w[0]:.3f}, {w[1]:.3e}; share of F needed beyond one rounding {max(FLOOR_USED.get(W, 0.0), 0.0):.3e}")


FLOOR_USED = {}  # window -> the largest share of F that a sample needed beyond its one float32 rounding


def sample_ratio(got, blk, clipped=False, W=None) -> float:
    """max |got - y64| / (2^-24 |y64| + F): the share of check_block's bound that is used.  The rounding of the result to
    float32 alone takes up to 2^-24 |y64|, so this figure comes close to 1 for a correct kernel; what tells kernels apart is
    the share of F that is left to need, max (|got - y64| - 2^-24 |y64|) / F, kept per window in FLOOR_USED."""
    want = np.clip(blk.y64, -float(M.CLIP), float(M.CLIP)) if clipped else blk.y64
    if not want.size:
        return 0.0
    err = np.abs(got.astype(np.float64) - want)
    if W is not None:
        FLOOR_USED[W] = max(FLOOR_USED.get(W, 0.0), float(np.max((err - M.EPS32 * np.abs(want)) / blk.F)))
    return float(np.max(err / (M.EPS32 * np.abs(want) + blk.F)))


def chunk_ratio(got_slots, blk, segs, floor: bool) -> float:
    """max over chunks of |sum - oracle's| / bound, the bound check_sink's (2^-21 relative) or check_sink_with_floor's."""
    want = M.sink(blk.v, segs).sums
    r = 2.0 ** -21
    tol = r * want
    if floor:
        counts = np.diff(np.append(np.asarray(segs, dtype=np.int64), blk.v.size))
        tol = tol + counts * (2.0 ** -64 * blk.S) ** 2 * (1.0 + 1.0 / r)
    live = tol > 0
    return float(np.max(np.abs(got_slots.sum(axis=1) - want)[live] / tol[live])) if live.any() else 0.0


def alpha_of(G, W):
    """The pole that reaches window W, checked against the library."""
    alpha = M.alpha_for_need(W - 100.0)
    assert alpha == float(np.exp(-64.0 * np.log(2.0) / (W - 100)))
    assert WIN.window(G, alpha) == (0, W, M.SPAN), (W, WIN.window(G, alpha))
    return alpha


def fused_case(G, W, alpha, label, z, segs, *, st=None, fresh=False, z_off=0, y_off=0, floor=False, img=None):
    """One fused NFM call and every assertion of the project on it; returns (what the GPU gave, the oracle's block)."""
    st = M.State() if fresh else (X.USED_STATE if st is None else st)
    img = st.image() if img is None else img
    z_dev = X.dev_in(G, z, z_off)
    got = X.gpu_demod(G, "nfm", False, z_dev, segs, state_img=img, fresh=fresh, y_off=y_off, alpha=alpha)
    u, blk, v_gpu, after, lin_F = X._fused_oracle(G, "nfm", False, z, z_dev, st, segs, got, alpha=alpha)
    X.check_source(label, "nfm", u, z, st.prev)
    X.check_block(label, got.audio, blk, clipped=True)
    assert np.array_equal(got.audio.view(np.uint32), np.clip(v_gpu, -M.CLIP, M.CLIP).view(np.uint32)), (label, "fused != stages")
    X.check_state(label, "nfm", got.state, after, lin_F, np.full(32, X.POISON, np.uint8) if fresh else img)
    (WIN.check_sink_with_floor if floor else X.check_sink)(label, got.peak, got.sums, v_gpu, blk, segs)
    counts = np.diff(np.append(np.asarray(segs, dtype=np.int64), z.size))
    assert np.all(got.sums[counts == 0] == 0.0), (label, "a chunk without samples received something")
    return got, blk, sample_ratio(got.audio, blk, clipped=True, W=W), chunk_ratio(got.sums, blk, segs, floor)


@pytest.mark.parametrize("form", ["deemph", "state", "fresh"])
@pytest.mark.parametrize("W", M.WINDOWS)
def test_every_window_sizes_per_sample(G, W, form):
    """test_windowed_sizes_per_sample at window W: every size of SIZES at every z / x offset and every output offset, through
    iqa_deemphasis with a state, iqa_demodulate from a used state block and iqa_demodulate_from_reset over poison."""
    alpha = alpha_of(G, W)
    worst_s = worst_c = 0.0
    for k, size in enumerate(WIN.SIZES):
        n = WIN.SIZES[size](W, M.SPAN)
        cls, lay = WIN._class_and_layout(k)
        if form == "deemph":
            x = M.make_x("deemph", cls, n)
            blk = M.stage_deemphasis(x, alpha, 0.37)
            for x_off in WIN.Z_OFFS:
                for y_off in WIN.Y_OFFS:
                    y, st = X.gpu_stage(G, "deemph", x, state=[0.37], x_off=x_off, y_off=y_off, alpha=alpha)
                    X.check_block(X._id("wins", W, form, size, n, cls, x_off, y_off), y, blk)
                    assert abs(st[0] - blk.y64[-1]) <= blk.F, (W, size, n, st, blk.y64[-1], blk.F)
                    worst_s = max(worst_s, sample_ratio(y, blk, W=W), abs(st[0] - blk.y64[-1]) / blk.F)
            continue
        z, segs = M.make_z(cls, n), M.layout(lay, n)
        for z_off in WIN.Z_OFFS:
            for y_off in WIN.Y_OFFS:
                label = X._id("wins", W, form, size, n, cls, lay, z_off, y_off)
                _, _, rs, rc = fused_case(G, W, alpha, label, z, segs, fresh=form == "fresh", z_off=z_off, y_off=y_off, floor=cls == "c")
                worst_s, worst_c = max(worst_s, rs), max(worst_c, rc)
    _note(W, f"sizes-{form}", worst_s, worst_c)


@pytest.mark.parametrize("layout", M.WINDOWED_LAYOUTS)
@pytest.mark.parametrize("W", M.WINDOWS)
def test_chunk_boundaries_on_own_edges(G, W, layout):
    """Chunk starts on own0, own0 +- 1 and own1 - 1 of every block, two in a block, one every 50 samples (more than 512
    starts), duplicated on an edge, and in a warm-up only: every chunk's sum against the oracle's, the total, the peak.  A
    block that credits its first or last sample to the neighbouring chunk fails `own`, `own-1`, `own+1` or `own-last`."""
    alpha = alpha_of(G, W)
    worst_s = worst_c = 0.0
    cases = [c for c in M.windowed_chunk_cases(W) if c[0] == layout]
    assert cases
    for lay, n, cls in cases:
        z, segs = M.make_z(cls, n), M.windowed_layout(lay, n, W, M.SPAN)
        for form in ("state", "fresh"):
            label = X._id("wins", W, "chunks", lay, n, cls, form, len(segs))
            _, _, rs, rc = fused_case(G, W, alpha, label, z, segs, fresh=form == "fresh", floor=cls == "c")
            worst_s, worst_c = max(worst_s, rs), max(worst_c, rc)
    _note(W, f"chunks-{layout}", worst_s, worst_c)


@pytest.mark.parametrize("W", M.WINDOWS)
def test_state_hand_off_lengths(G, W):
    """More than one block, so block 0 hands the state on from a warm-up of its own from t0 = (n - W) & ~7: lengths that put
    t0 at 0 and next to a multiple of 8, and give the warm-up one, two and three rounds.  y_last within F, prev bit for bit;
    a second call of 1000 samples from the GPU's own state block meets the per-sample bound."""
    alpha = alpha_of(G, W)
    own = M.SPAN - W
    worst_s = worst_c = 0.0
    for n in (own + 1, own + 7, own + 8, own + 9, own + W, own + W + 2048 + 3, 2 * own):
        assert n > own and -(-(n - ((n - W) & ~7)) // 2048) in (1, 2, 3)
        z = M.make_z("a", n + 1000)
        label = X._id("wins", W, "hand-off", n)
        got, blk, rs, rc = fused_case(G, W, alpha, label, z[:n], M.layout("prod", n))  # (checks y_last and prev)
        de_y = float(got.state[8:16].view(np.float64)[0])
        worst_s = max(worst_s, rs, abs(de_y - blk.y64[-1]) / blk.F)
        st2 = M.State(got.state[:8].view(np.complex64)[0], de_y, X.USED_STATE.dc_x, X.USED_STATE.dc_y)
        assert np.array_equal(st2.image(), got.state), label
        _, _, rs2, rc2 = fused_case(G, W, alpha, label + "-next", z[n:], M.layout("prod", 1000), st=st2)
        worst_s, worst_c = max(worst_s, rs2), max(worst_c, rc, rc2)
    _note(W, "hand-off", worst_s, worst_c)


@pytest.mark.parametrize("W", M.WINDOWS)
def test_full_scale_past_is_forgotten(G, W):
    """test_a_block_forgets_a_full_scale_past (tail `quiet`) at window W: 3 SPAN of |u| near pi, then 3 SPAN of u = 0; the first
    own sample of every block is within 2^-24 |y| + F."""
    alpha = alpha_of(G, W)
    own, n = M.SPAN - W, 6 * M.SPAN
    z = np.empty(n, dtype=np.complex64)
    z[:3 * M.SPAN] = np.exp(1j * (np.pi - 0.01) * np.arange(3 * M.SPAN, dtype=np.float64)).astype(np.complex64)
    z[3 * M.SPAN:] = M.QUIET
    got, blk, rs, rc = fused_case(G, W, alpha, f"wins-{W}-forget", z, M.layout("prod", n))
    assert blk.S > 3.0, blk.S
    want = np.clip(blk.y64, -float(M.CLIP), float(M.CLIP))
    first_own = np.arange(own, n, own)
    err = np.abs(got.audio[first_own].astype(np.float64) - want[first_own])
    tol = M.EPS32 * np.abs(want[first_own]) + blk.F
    bad = first_own[err > tol]
    assert bad.size == 0, ("the first own sample of a block", bad.tolist(), "block", (bad // own).tolist(), err[err > tol].tolist(), tol[err > tol].tolist())
    _note(W, "forget", max(rs, float(np.max(err / tol))), rc)


def test_window_boundaries_match_the_model(G):
    """iqa_scan_window equals scan_model.window at every alpha of the host test; rc 1 leaves the outputs as they were."""
    for alpha, _ in HOST.window_alphas():
        rc, w, span = WIN.window(G, alpha)  # (passes -1 into both outputs)
        want = M.window(alpha)
        assert (rc, w, span) == ((1, -1, -1) if want is None else (0, want, M.SPAN)), (alpha, rc, w, span, want)


def test_product_filters_at_the_rates_the_product_runs(G):
    """DeemphasisFilter(tau, fs) at every row of the table of settings (the two fallback rows too): its pole, the window
    the library takes for it, and a stream in ragged cuts and whole, each block per sample against the oracle run from the
    filter's own carried state."""
    from iq_to_audio_amd.decoders.nfm import DeemphasisFilter

    for tau, fs, W in M.PRODUCT_WINDOWS:
        probe = DeemphasisFilter(tau, fs)
        alpha = probe.alpha
        assert alpha == float(np.exp(-1.0 / (fs * max(tau * 1e-6, 1e-6)))), (tau, fs, alpha)
        assert WIN.window(G, alpha) == ((1, -1, -1) if W is None else (0, W, M.SPAN)), (tau, fs, WIN.window(G, alpha))
        n = 20_000 if W is None else 3 * (M.SPAN - W) + W + 5
        x = M.make_x("deemph", "a", n)
        worst = 0.0
        for cuts in ((1, 1, 2047, 2049, 8), ()):
            f = DeemphasisFilter(tau, fs)
            assert f.state == 0.0
            edges = np.concatenate(([0], np.cumsum(cuts), [n])).astype(np.int64)
            assert edges[-2] < n
            for lo, hi in zip(edges[:-1], edges[1:]):
                y_prev = f.state / alpha  # the filter carries alpha * y_last, as the reference does
                y = f.process(x[lo:hi])
                blk = M.stage_deemphasis(x[lo:hi], alpha, y_prev)
                label = f"wins-product-{tau:g}us-{fs:g}Hz-{lo}-{hi}"
                assert isinstance(y, np.ndarray)
                X.check_block(label, y, blk)
                assert abs(f.state - alpha * blk.y64[-1]) <= alpha * blk.F, (label, f.state, alpha * blk.y64[-1], alpha * blk.F)
                worst = max(worst, sample_ratio(y, blk, W="three launches" if W is None else W), abs(f.state - alpha * blk.y64[-1]) / (alpha * blk.F))
        _note("three launches" if W is None else W, f"product-{tau:g}us-{fs:g}Hz", worst)


def test_fallback_just_past_the_largest_window(G):
    """need = 4096.5 keeps the three launches, need = 4095.5 takes the one-launch form at W = 4096: both sides of the switch
    on the same input, iqa_deemphasis and iqa_demodulate, the same bounds."""
    n = 20_000
    z, segs = M.make_z("a", n), M.layout("tile+1", n)
    x = M.make_x("deemph", "a", n)
    for need, want in ((4096.5, (1, -1, -1)), (4095.5, (0, 4096, M.SPAN))):
        alpha = M.alpha_for_need(need)
        assert WIN.window(G, alpha) == want, (need, WIN.window(G, alpha))
        y, st = X.gpu_stage(G, "deemph", x, state=[0.37], alpha=alpha)
        blk = M.stage_deemphasis(x, alpha, 0.37)
        X.check_block(f"wins-switch-{need}-deemph", y, blk)
        assert abs(st[0] - blk.y64[-1]) <= blk.F, (need, st, blk.y64[-1], blk.F)
        key = "three launches" if want[0] else 4096
        _, _, rs, rc = fused_case(G, key, alpha, f"wins-switch-{need}-demod", z, segs)
        _note(key, f"switch-need-{need}", max(rs, sample_ratio(y, blk, W=key)), rc)
