"""CPU checks of the one-launch de-emphasis scan's geometry as tests/scan_model.py states it: ``window`` against a
brute-force search in np.longdouble, the layouts that put chunk starts on a workgroup's own-range edges, and the
completeness of the case matrix tests/test_gpu_scan_windows.py runs -- a condition on its INPUTS, computed from
``windowed_plan_classes``, for every one of the eight windows.  No GPU, nothing from the product."""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest


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
PLACED = [(512 * k + d, 512 * k if d < 0 else 512 * (k + 1) if k < 8 else None) for k in range(1, 9) for d in (-0.5, 0.5)]
BEYOND = [(4096.5, None), (8191.5, None)]
ODD_ALPHAS = (0.5, 1e-300, 5e-324, 1.0 - 2.0 ** -53)
NO_POLE = (0.0, 1.0, -0.5, float("nan"))


def window_alphas():
    """Every alpha of this file, with the W it must give where the issue's table or the placement says so (else ...):
    the GPU test runs iqa_scan_window over the same list."""
    out = [(M.product_alpha(tau, fs), w) for tau, fs, w in M.PRODUCT_WINDOWS]
    out += [(M.alpha_for_need(need), w) for need, w in PLACED + BEYOND]
    out += [(a, ...) for a in ODD_ALPHAS]
    out += [(a, None) for a in NO_POLE]
    return out


def brute_force_window(alpha: float, span: int = 8192):
    """The smallest multiple of 512 in [512, span / 2] with alpha^w <= 2^-64, the power in np.longdouble."""
    if not (alpha > 0.0 and alpha < 1.0):
        return None
    for w in range(512, span // 2 + 1, 512):
        if LD(alpha) ** LD(w) <= LD(2.0) ** -64:
            return w
    return None


def test_the_table_of_product_settings():
    """The W column, and the `need` column to the digit it is printed with."""
    needs = (213.3, 21.3, 831.8, 1279.7, 1597.0, 2555.2, 2994.4, 3327.1, 3832.8, 5110.4, 4360.9)
    for (tau, fs, w), need in zip(M.PRODUCT_WINDOWS, needs):
        alpha = M.product_alpha(tau, fs)
        assert alpha == float(np.exp(-1.0 / (fs * max(tau * 1e-6, 1e-6))))
        assert abs(64.0 * np.log(2.0) * fs * max(tau, 1.0) * 1e-6 - need) < 0.06, (tau, fs)
        assert M.window(alpha) == w == brute_force_window(alpha), (tau, fs, M.window(alpha), w)
    assert {w for _, _, w in M.PRODUCT_WINDOWS} >= set(M.WINDOWS)  # the product reaches all eight
    assert M.window(M.ALPHA) == 1536


@pytest.mark.parametrize("alpha,want", window_alphas(), ids=lambda v: repr(v))
def test_window_against_a_brute_force_search(alpha, want):
    got = M.window(alpha)
    assert got == brute_force_window(alpha), (alpha, got)
    if want is not ...:
        assert got == want, (alpha, got, want)
    if got is not None:  # what the specification promises of a W
        assert got % 512 == 0 and got >= 512 and 2 * got <= M.SPAN
        assert alpha ** got <= 2.0 ** -64
        assert got == 512 or alpha ** (got - 512) > 2.0 ** -64


def test_odd_alphas():
    assert [M.window(a) for a in ODD_ALPHAS] == [512, 512, 512, None]
    assert [M.window(a) for a in NO_POLE] == [None] * 4
    assert M.window(0.5, span=512) is None and M.window(0.5, span=1024) == 512  # 2 W <= span


def test_placed_alphas_keep_their_distance_from_the_threshold():
    """need = 512 k +- 0.5 puts alpha^(512 k) a factor alpha^(+-1/2) from 2^-64: far beyond the rounding of any pow, so the
    kernel's pow, Python's and longdouble's cannot legitimately disagree about these alphas."""
    for need, _ in PLACED + BEYOND:
        alpha = M.alpha_for_need(need)
        factor = alpha ** 0.5
        assert factor < 1.0 - 1e-3, (need, factor)
        edge = 512 * round(need / 512.0)
        ratio = float(LD(alpha) ** LD(edge) / LD(2.0) ** -64)
        assert (ratio < 1.0 - 1e-3) if need < edge else (ratio > 1.0 + 1e-3), (need, ratio)
    for W in M.WINDOWS:  # and the alpha the GPU tests run window W with, need = W - 100
        assert M.window(M.alpha_for_need(W - 100.0)) == W


@pytest.mark.parametrize("W", M.WINDOWS)
def test_layouts_sit_where_they_say(W):
    own = M.SPAN - W
    n = 3 * own + W + 5
    for lay in M.WINDOWED_LAYOUTS:
        for m in (n, 4 * own + 3, own, own + 1, 1):
            s = M.windowed_layout(lay, m, W, M.SPAN)
            assert s.dtype == np.int64 and s[0] == 0 and np.all(np.diff(s) >= 0), (lay, m)
            if not lay.startswith("dup") and lay != "warmup-only":
                assert s[-1] < m and np.all(np.diff(s) > 0), (lay, m)
    nb = -(-n // own)  # 4 blocks, 5 at W = 4096 (the last one of W + 5 - own = 5 samples)
    edges = [k * own for k in range(1, nb)]
    assert M.windowed_layout("own", n, W).tolist() == [0] + edges
    assert M.windowed_layout("own-1", n, W).tolist() == [0] + [e - 1 for e in edges]
    assert M.windowed_layout("own+1", n, W).tolist() == [0] + [e + 1 for e in edges]
    assert M.windowed_layout("own-last", n, W).tolist() == [0] + [e - 1 for e in edges] + [n - 1]
    two = {0} | {k * own + 1 for k in range(nb)} | {k * own + own // 2 for k in range(nb)}
    assert M.windowed_layout("two-in-one", n, W).tolist() == sorted(v for v in two if v < n)
    assert M.windowed_layout("dup-own", n, W).tolist() == [0, own, own]
    assert M.windowed_layout("dup-own-1", n, W).tolist() == [0, own - 1, own - 1]
    assert M.windowed_layout("warmup-only", n, W).tolist() == [0, own - W // 2]
    assert M.windowed_layout("fifty", n, W).size == -(-n // 50)


def _plans(W, lay, n):
    segs = M.windowed_layout(lay, n, W, M.SPAN)
    return segs, M.windowed_plan_classes(n, W, M.SPAN, segs)


@pytest.mark.parametrize("W", M.WINDOWS)
def test_plan_of_every_layout_is_the_one_it_was_built_for(W):
    """What each layout is FOR, block by block: were the restatement of sink_count_segments / sink_plan off by one at an
    own-range edge, these fail (the same restatement then carries the completeness check below)."""
    own = M.SPAN - W
    n = 3 * own + W + 5
    nb = -(-n // own)
    segs, p = _plans(W, "own", n)
    assert len(p) == nb and [(b.own0, b.own1) for b in p] == [(k * own, min((k + 1) * own, n)) for k in range(nb)]
    assert [(b.kind, b.seg0, b.seg1) for b in p] == [("uniform", k, k) for k in range(nb)]  # a start ON own0 belongs to its block
    assert all(b.at_own0 for b in p[1:]) and not any(b.at_last or b.after_own0 for b in p)
    segs, p = _plans(W, "own+1", n)
    assert [(b.kind, b.seg0, b.seg1, b.bnd) for b in p[1:]] == [("simple", k - 1, k, k * own + 1) for k in range(1, nb)]
    assert p[0].kind == "uniform" and all(b.after_own0 for b in p[1:])
    segs, p = _plans(W, "own-1", n)
    assert [(b.kind, b.seg0, b.seg1, b.bnd) for b in p[:-1]] == [("simple", k, k + 1, (k + 1) * own - 1) for k in range(nb - 1)]
    assert p[-1].kind == "uniform" and all(b.at_last for b in p[:-1]) and all(b.before_own0 for b in p[1:])
    segs, p = _plans(W, "own-last", n)
    assert [(b.kind, b.bnd) for b in p] == [("simple", b.own1 - 1) for b in p] and p[-1].bnd == n - 1
    segs, p = _plans(W, "two-in-one", n)
    assert [b.kind for b in p[:3]] == ["general"] * 3 and [b.seg1 - b.seg0 for b in p[:3]] == [2, 2, 2]
    segs, p = _plans(W, "fifty", n)
    assert all(b.kind == "general" for b in p[:-1]) and p[0].seg1 - p[0].seg0 > 80
    segs, p = _plans(W, "dup-own", n)
    assert [(b.kind, b.seg0, b.seg1) for b in p] == [("uniform", 0, 0)] + [("uniform", 2, 2)] * (nb - 1)
    segs, p = _plans(W, "dup-own-1", n)
    assert (p[0].kind, p[0].seg0, p[0].seg1) == ("general", 0, 2) and [(b.kind, b.seg0) for b in p[1:]] == [("uniform", 2)] * (nb - 1)
    segs, p = _plans(W, "warmup-only", n)
    assert (p[0].kind, p[0].bnd) == ("simple", own - W // 2) and (p[1].kind, p[1].seg0, p[1].warmup_only) == ("uniform", 1, True)
    assert not p[0].warmup_only and not p[2].warmup_only


@pytest.mark.parametrize("W", M.WINDOWS)
def test_case_matrix_of_the_gpu_file_is_complete(W):
    """For this window the chunk-boundary cases reach every decision of the sink's plan, every own-range edge, more than
    512 starts, an empty chunk and a block that sees a boundary in its warm-up only; and in every case the chunk the plan
    credits each sample to is the chunk the oracle's sink (``segment_of``) credits it to."""
    own = M.SPAN - W
    reach = dict.fromkeys(("uniform", "simple", "general", "own0", "own0+1", "own0-1", "own1-1", "more than 512 starts",
                           "an empty chunk", "warm-up only", "class c"), False)
    per_layout = {}
    for lay, n, cls in M.windowed_chunk_cases(W):
        assert n <= 40_000, (lay, n)
        segs = M.windowed_layout(lay, n, W, M.SPAN)
        plans = M.windowed_plan_classes(n, W, M.SPAN, segs)
        assert len(plans) == -(-n // own) >= 4
        assert np.array_equal(M.windowed_chunk_of(n, W, M.SPAN, segs), M.segment_of(n, segs)), (W, lay, n)
        for b in plans:
            reach[b.kind] = True
            # an edge counts as reached where the plan also puts the start's chunk on the right side of it
            reach["own0"] |= b.at_own0 and segs[b.seg0] == b.own0           # the first own sample opens its chunk
            reach["own0+1"] |= b.after_own0 and b.kind == "simple" and b.bnd == b.own0 + 1
            reach["own0-1"] |= b.before_own0 and segs[b.seg0] == b.own0 - 1  # ... opened by the block in front
            reach["own1-1"] |= b.at_last and segs[b.seg1] == b.own1 - 1     # the last own sample opens one
            reach["warm-up only"] |= b.warmup_only
        reach["more than 512 starts"] |= segs.size > M.FIFTY_STARTS
        reach["an empty chunk"] |= bool(np.any(np.diff(segs) == 0))
        reach["class c"] |= cls == "c"
        per_layout.setdefault(lay, set()).add(cls)
    assert [k for k, ok in reach.items() if not ok] == []
    assert set(per_layout) == set(M.WINDOWED_LAYOUTS)
    assert per_layout["own"] == per_layout["own-last"] == {"a", "c"}
    ns = [n for lay, n, _ in M.windowed_chunk_cases(W) if lay == "fifty"]
    assert ns[:2] == [3 * own + W + 5, 4 * own + 3] and max(ns) > 25_600
    # class (c): live samples on both sides of block 1's first own sample, and a later edge inside a stretch of exact zeros
    z = M.make_z("c", 3 * own + W + 5)
    assert np.any(z[own - 8:own] != 0) and np.any(z[own:own + 8] != 0)
    assert any(np.all(z[k * own - 8:k * own + 8] == 0) for k in range(2, 5))


def test_the_plan_restatement_notices_a_start_credited_to_the_neighbour():
    """The check of the check: a sink that gives the sample ON a start to the chunk in front (`<` for `<=`) differs from the
    oracle's at exactly the starts, so the equality asserted above is not vacuous."""
    W, own = 1536, M.SPAN - 1536
    n = 3 * own + W + 5
    segs = M.windowed_layout("own", n, W, M.SPAN)
    wrong = np.searchsorted(segs, np.arange(n), side="left") - 1
    wrong[0] = 0
    assert np.flatnonzero(wrong != M.windowed_chunk_of(n, W, M.SPAN, segs)).tolist() == segs[1:].tolist()
