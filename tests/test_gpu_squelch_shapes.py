"""The squelch kernels (csrc/squelch.hip) per sample against tests/squelch_model.py, at the shapes where the kernels'
own structure changes: tile edges and scan carries, window / hold / fade edges, the int8 wrap, both envelope signs in
the radix select, percentile edges, channel counts, trim edges, PCM16 rounding, and segment tables (more than 64
segments, mixed rates, gaps between bases).

Every check applies the oracle to the GPU's own previous stage and demands equality per sample -- level, threshold
array, mask, dilated mask, gain, floor, threshold, bounds, float32 and PCM16 output -- except two places where the
previous stage is the input and float64 sums and log10 stand between:

* envelope dB: |got - want| <= 20 log10(1 + 2^-23) + ulp32(want) (M.envelope_bound: the float32 averages may differ
  by one ulp, the final cast adds one), exactly -160 where the oracle clamps, no sample excused.  With window 1 there
  is no sum and the average is the magnitude itself, so only ulp32(want) is allowed.
* the transient level, dbfs(short) - dbfs(long + 1e-10): each term within the envelope bound, plus one ulp of the
  float32 difference.  The transient mask is then exact on the GPU's own level.

Seconds are multiples of 1 ms at 1000 Hz, so a configuration's sample counts are the intended integers (asserted).
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import squelch_model as M

import iq_to_audio_amd.squelch as S
from iq_to_audio_amd import _native as N

pytestmark = pytest.mark.gpu

RATE = 1000.0
METHODS = ["adaptive", "static", "transient"]
TILE = N.SQ_TILE
STATS: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _envelope_report():
    yield
    for cls, (total, differ, worst) in sorted(STATS.items()):
        print(f"\nenvelope [{cls}]: {differ} of {total} samples not bit-identical, largest |got - want| / bound {worst:.3f}")


def ms(k: int) -> float:
    return k / 1000.0


def config(method="adaptive", window=40, short=3, hold=30, fade=5, lead=150, trail=350, **kw):
    return S.SquelchConfig(method=method, window_seconds=ms(window), transient_window_seconds=ms(short),
                           hold_seconds=ms(hold), fade_seconds=ms(fade), trim_lead_seconds=ms(lead),
                           trim_trail_seconds=ms(trail), **kw)


def signal(n, channels=1, seed=0, noise=0.003, amp=0.3):
    """Noise with tone bursts (for the level methods) and 3-sample clicks (for "transient"); one burst ends at n."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, channels)) * noise
    t = np.arange(n)
    for a, b in ((0.2, 0.3), (0.55, 0.6), (0.93, 1.0)):
        lo, hi = int(a * n), max(int(b * n), int(a * n) + 1)
        x[lo:hi] += amp * np.sin(0.9 * t[lo:hi] + 0.3)[:, None]
    for a in (0.1, 0.45, 0.8):
        x[int(a * n):int(a * n) + 3] += 0.8
    return x.astype(np.float32)


def from_mask(mask):
    """With window 1 and a manual floor, "static" turns this input into exactly `mask` (-6 dB against -160 dB)."""
    return np.where(mask, np.float32(0.5), np.float32(0.0)).astype(np.float32)[:, None]


def mask_config(**kw):
    kw.setdefault("hold", 0)
    kw.setdefault("fade", 0)
    return config("static", window=1, auto_noise_floor=False, manual_noise_floor_db=-50.0, **kw)


def check(res, x, rate, cfg, *, pcm16=False, cls="general"):
    """Every stage of one segment against the oracle applied to the GPU's previous stage.  Returns the GPU's stages
    and the oracle's envelope (numpy)."""
    x = x.reshape(x.shape[0], -1)
    n = x.shape[0]
    st = res.stages
    w = M.windows(rate, cfg)
    assert (st["window"], st["hold"], st["fade"]) == (w["window"], w["hold"], w["fade"])
    g = {k: st[k].cpu().numpy() for k in ("envelope_db", "level", "threshold", "mask", "dilated", "gain")}
    assert all(v.shape == (n,) for v in g.values())
    mag = M.magnitude(x)

    # envelope: the derived bound, no sample excused
    env, want_env = g["envelope_db"], M.envelope_db(mag, w["window"])
    assert env.dtype == np.float32
    bound = M.envelope_bound(want_env)
    if w["window"] == 1:
        bound = np.spacing(np.abs(want_env)).astype(np.float64)
    err = np.abs(env.astype(np.float64) - want_env.astype(np.float64))
    differ = int(np.count_nonzero(env != want_env))
    tot = STATS.setdefault(cls, [0, 0, 0.0])
    tot[0], tot[1], tot[2] = tot[0] + n, tot[1] + differ, max(tot[2], float(np.max(err / bound)))
    assert np.all(err <= bound), (cls, int(np.argmax(err / bound)), float(np.max(err / bound)))
    clamp = want_env == np.float32(M.MIN_DBFS)
    assert np.all(env[clamp] == np.float32(M.MIN_DBFS))

    # floor and threshold: np.percentile of the GPU's envelope
    if cfg.auto_noise_floor:
        assert st["noise_floor_db"] == M.noise_floor(env, cfg.noise_floor_percentile)
    else:
        assert st["noise_floor_db"] == float(cfg.manual_noise_floor_db)
    thr_db = st["noise_floor_db"] + cfg.threshold_margin_db
    assert st["threshold_db"] == thr_db
    assert (res.noise_floor_db, res.threshold_db) == (st["noise_floor_db"], st["threshold_db"])

    if cfg.method == "adaptive":
        assert np.array_equal(g["level"], M.relative(env))
        assert np.array_equal(g["threshold"], M.adaptive_threshold(env, g["level"], thr_db))
        assert np.array_equal(g["mask"], M.adaptive_mask(env, g["threshold"], thr_db))
    elif cfg.method == "static":
        assert np.array_equal(g["threshold"], np.full(n, np.float32(thr_db)))
        assert np.array_equal(g["mask"], M.static_mask(env, thr_db))
    else:
        assert (w["short_window"], w["long_window"]) == tuple(S._windows(n, rate, cfg)[k] for k in ("short_window", "long_window"))
        want = M.transient_level(mag, w["short_window"], w["long_window"])
        lim = (M.envelope_bound(M.dbfs(M.box(mag, w["short_window"])))
               + M.envelope_bound(M.dbfs(M.box(mag, w["long_window"]) + np.float32(M.EPS)))
               + np.spacing(np.maximum(np.abs(want), np.abs(g["level"]))).astype(np.float64))
        lerr = np.abs(g["level"].astype(np.float64) - want.astype(np.float64))
        assert np.all(lerr <= lim), (cls, int(np.argmax(lerr / lim)), float(np.max(lerr / lim)))
        assert np.array_equal(g["threshold"], np.full(n, np.float32(cfg.transient_margin_db)))
        assert np.array_equal(g["mask"], M.transient_mask(g["level"], cfg.transient_margin_db))

    assert np.array_equal(g["dilated"], M.dilate(g["mask"], w["hold"]))
    want_gain = M.gain(g["dilated"], w["fade"])
    assert g["gain"].dtype == np.float32 and np.array_equal(g["gain"], want_gain)
    start, stop = M.bounds(g["gain"], n, w["lead"], w["trail"], cfg.trim_silence)
    assert (st["start"], st["stop"]) == (start, stop) == (res.start, res.stop)
    y = res.samples.cpu().numpy()
    want_y = (M.output_pcm16 if pcm16 else M.output_f32)(x, g["gain"], start, stop)
    assert y.dtype == want_y.dtype and y.shape == want_y.shape and np.array_equal(y, want_y)
    g["want_envelope_db"] = want_env
    g["output"] = y
    return g


def run(x, cfg, *, rate=RATE, pcm16=False, cls="general"):
    (res,) = S.squelch_device([(x, rate)], cfg, pcm16=pcm16, return_stages=True)
    return check(res, x, rate, cfg, pcm16=pcm16, cls=cls), res


# ---------------------------------------------------------------------------------------------------------------
# lengths: tile edges and scan carries


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [40, 2047, 2048, 2049, 4097])
def test_lengths_at_tile_edges(n, method):
    """n == window; one sample short of a tile, a whole tile, one sample into the second and the third tile."""
    cfg = config(method, window=40, short=3, hold=130, fade=7, lead=2, trail=3)
    assert S._windows(n, RATE, cfg)["long_window"] == 40
    g, _ = run(signal(n, 2, seed=n), cfg, cls=f"n={n}")
    if n > 40 and method != "transient":
        assert g["mask"].any() and not g["mask"].all()


@pytest.mark.parametrize("method", METHODS)
def test_a_second_pass_of_the_tile_scan_carries(method):
    """n = 256 * 2048 + 1: 257 tiles, so the per-segment scan of tile partials takes a second 256-wide pass, and
    the last tile holds one sample.  A burst ends at n, so that sample's prefix-dependent stages are not trivial."""
    n = 256 * TILE + 1
    assert -(-n // TILE) == 257 > 256
    cfg = config(method, window=64, short=4, hold=130, fade=7, lead=5, trail=5)
    assert S._windows(n, RATE, cfg)["long_window"] == 64
    x = signal(n, 1, seed=5)
    g, res = run(x, cfg, cls="n=524289")
    last = n - 1
    assert abs(float(g["envelope_db"][last]) - float(g["want_envelope_db"][last])) <= float(M.envelope_bound(g["want_envelope_db"][last:])[0])
    assert g["envelope_db"][last] > -40.0  # the closing burst
    if method == "adaptive":
        assert g["level"][last] == g["envelope_db"][last] - g["envelope_db"].min() and g["level"][last] > 20.0
    if method != "transient":
        assert g["mask"][last] and g["dilated"][last] and g["gain"][last] == 1.0 and res.stop == n
    # window counts of the last tile reach back over the tile carry
    assert g["dilated"][last] == M.dilate(g["mask"][last - 400:], 130)[-1]
    assert g["gain"][last] == M.gain(g["dilated"][last - 30:], 7)[-1]


def test_a_third_pass_of_the_tile_scan_accumulates_its_carry():
    """n = 512 * 2048 + 1: 513 tiles, three passes.  After two passes a carry that is only the previous pass's total
    equals the accumulated one; the third pass tells them apart -- in the float64 and int64 sums and, with the
    quietest stretch in the first quarter, in the running minimum."""
    n = 512 * TILE + 1
    assert -(-n // TILE) == 513 > 2 * 256
    x = signal(n, 1, seed=6)
    x[:n // 4] *= np.float32(0.5)
    cfg = config("adaptive", window=16, hold=20, fade=7, lead=5, trail=5)
    g, res = run(x, cfg, cls="n=1048577")
    assert int(np.argmin(g["envelope_db"])) < n // 4
    assert g["level"][n - 1] == g["envelope_db"][n - 1] - g["envelope_db"].min()
    assert g["mask"][n - 1] and g["gain"][n - 1] == 1.0 and res.stop == n


# ---------------------------------------------------------------------------------------------------------------
# windows


@pytest.mark.parametrize("window", [1, 2, 3, 4, 5, 2047, 2048, 2049, 4097])
def test_window_edges(window):
    """box's early return (1), even against odd centring at small w, windows around a tile, window == n."""
    n = 4097
    for method in ("adaptive", "static"):
        g, _ = run(signal(n, 1, seed=window), config(method, window=window), cls=f"window={window}")
        assert g["envelope_db"].min() > -160.0


@pytest.mark.parametrize("window,short,want", [(5, 1, (1, 5)), (3, 1, (1, 4)), (5, 3, (3, 12)), (40, 3, (3, 40)),
                                               (12, 3, (3, 12)), (1, 1, (1, 4))])
def test_transient_window_branches(window, short, want):
    """short_window == 1 (box returns the magnitude); long_window = 4 * short against long_window = window."""
    n = 2049
    cfg = config("transient", window=window, short=short, transient_margin_db=3.0)
    ws = S._windows(n, RATE, cfg)
    assert (ws["window"], ws["short_window"], ws["long_window"]) == (window, *want)
    g, _ = run(signal(n, 1, seed=window + short), cfg, cls="transient windows")
    assert g["mask"].any() and not g["mask"].all()


# ---------------------------------------------------------------------------------------------------------------
# hold: the int8 wrap


def _hold_of(tag, n):
    return {"n-1": n - 1, "n": n, "5n": 5 * n}.get(tag, tag)


@pytest.mark.parametrize("hold", [0, 1, 126, 127, 128, 255, 256, 300, "n-1", "n", "5n"])
def test_hold_edges_on_bursts(hold):
    """Bursts of 100, 128, 129, 256 and 400 samples.  A clear sample's window of hold + 1 samples holds at most
    `hold` set ones, so the first count that is not positive as int8, 128, is reached from hold 128 on: there the
    oracle's dilated mask must differ from the unwrapped one (at 127 it cannot -- see M.burst_mask)."""
    mask = M.burst_mask()
    n = mask.size
    hold = _hold_of(hold, n)
    g, _ = run(from_mask(mask), mask_config(hold=hold, fade=3), cls="masks")
    assert np.array_equal(g["mask"], mask)
    assert np.array_equal(g["dilated"], M.dilate(mask, hold, wrap=False)) == (hold < 128)


@pytest.mark.parametrize("hold", [0, 1, 126, 127, 128, 255, 256, 300, "n-1", "n", "5n"])
def test_hold_edges_on_a_dense_mask(hold):
    n = 2500
    mask = np.random.default_rng(98).random(n) < 0.98
    mask[[0, 1, 2, n - 1]] = [False, True, False, False]
    g, _ = run(from_mask(mask), mask_config(hold=_hold_of(hold, n)), cls="masks")
    assert np.array_equal(g["mask"], mask)


# ---------------------------------------------------------------------------------------------------------------
# fade: edge padding and the 1e-3 activity edge


@pytest.mark.parametrize("ends", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("fade", [0, 1, 2, 999, 1000, 1001, "n-1", "n", "3n+2"])
def test_fade_edges(fade, ends):
    """fade 1; fade >= n, where both edge-padding terms apply to one sample; masks with and without the first and
    the last sample set; and, with no trim padding, the gain > 1e-3 edge: at fade 1000 the first ramp value is
    float32(1e-3) itself and is not active, at 999 it is, at 1001 the second one is."""
    n = 2049
    fade = {"n-1": n - 1, "n": n, "3n+2": 3 * n + 2}.get(fade, fade)
    mask = np.zeros(n, dtype=bool)
    for a, ln in ((1100, 1), (1500, 90), (1900, 3)):  # more than 1001 clear samples before the first
        mask[a:a + ln] = True
    mask[0], mask[n - 1] = ends
    g, res = run(from_mask(mask), mask_config(fade=fade, lead=0, trail=0), cls="masks")
    assert np.array_equal(g["dilated"], mask)
    if fade == 1000 and not ends[0]:
        first = int(np.flatnonzero(g["gain"] > 0)[0])
        assert g["gain"][first] == np.float32(1e-3) and res.start == first + 1
    if fade in (999, 1001) and not ends[0]:
        first = int(np.flatnonzero(g["gain"] > 0)[0])
        assert res.start == first + (fade == 1001)


# ---------------------------------------------------------------------------------------------------------------
# channels


@pytest.mark.parametrize("channels", [1, 2, 3, 5])
def test_channel_counts(channels):
    for method in METHODS:
        run(signal(2049, channels, seed=channels), config(method), cls="channels")


@pytest.mark.parametrize("channels", [3, 5])
def test_the_channel_mean_is_rounded_once_from_float64(channels):
    """Magnitudes near 1.0 with window 1: the envelope is dbfs(mean) with no sum in between, and near 0 dB one ulp
    of the float32 mean moves the dB value by many of its ulps -- a mean divided in float32 shows."""
    rng = np.random.default_rng(channels)
    x = (rng.uniform(0.8, 1.25, (2049, channels)) * rng.choice([-1.0, 1.0], (2049, channels))).astype(np.float32)
    mag = M.magnitude(x)
    lossy = (np.sum(np.abs(x), axis=1, dtype=np.float64).astype(np.float32) / np.float32(channels))
    assert np.count_nonzero(lossy != mag) > 100  # the input tells the two apart
    g, _ = run(x, config("static", window=1), cls="window=1")
    assert np.count_nonzero(M.dbfs(lossy) != g["want_envelope_db"]) > 100


# ---------------------------------------------------------------------------------------------------------------
# radix select: both signs, percentile edges, ties


@pytest.mark.parametrize("method", METHODS)
def test_an_envelope_of_both_signs(method):
    """Float input from 1e-4 up to 4.0: the envelope crosses 0 dB, so the select's key transform takes both branches."""
    n = 3000
    rng = np.random.default_rng(4)
    amp = np.exp(np.interp(np.arange(n), [0, 900, 1000, 1800, 2000, n], np.log([1e-4, 1e-3, 4.0, 2.0, 1e-2, 4.0])))
    x = (amp[:, None] * rng.uniform(0.5, 1.0, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))).astype(np.float32)
    x[1000], x[1001] = 4.0, -3.95
    assert 3.9 < np.abs(x).max() <= 4.0
    g, _ = run(x, config(method, window=8, short=2, hold=20), cls="both signs")
    assert (g["want_envelope_db"] > 1.0).sum() > 200 and (g["want_envelope_db"] < -1.0).sum() > 200
    assert g["envelope_db"].max() > 0 > g["envelope_db"].min()
    if method == "static":
        for pct in (0.0, 0.5, 0.62, 1.0):  # floors on both sides of 0 dB
            run(x, config("static", window=8, noise_floor_percentile=pct), cls="both signs")


def _gamma_class(n, pct):
    lo, hi, g = S.percentile_plan(n, pct * 100.0)
    return "0" if g == 0 else "0.5" if g == 0.5 else "<0.5" if g < 0.5 else ">0.5"


@pytest.mark.parametrize("pct", [0.0, 0.2, 0.5, 0.999, 1.0])
def test_percentile_edges(pct):
    """Percentile 0 (weight 0 on the minimum) and 1 (prev = next = n - 1), and lengths at which numpy's interpolation weight is 0, 0.5 and on
    either side of 0.5 (both forms of its lerp).  Window 1: the envelope is the input's, with its minimum on the
    last sample of the first tile and its maximum on the first sample of the second."""
    seen = set()
    for n in (2049, 2050, 2052, 2054, 4097, 4100):
        rng = np.random.default_rng(n)
        x = (rng.uniform(0.01, 0.5, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        x[TILE - 1], x[TILE] = 0.001, 0.9
        for method in ("static", "adaptive"):
            g, _ = run(x, config(method, window=1, noise_floor_percentile=pct, threshold_margin_db=1.0), cls="window=1")
        assert int(np.argmin(g["envelope_db"])) == TILE - 1 and int(np.argmax(g["envelope_db"])) == TILE
        seen |= {_gamma_class(n, pct), _gamma_class(n, 0.05), _gamma_class(n, 0.95)}
        lo, hi, gam = S.percentile_plan(n, pct * 100.0)
        if pct == 1.0:
            assert lo == hi == n - 1
        if pct == 0.0:
            assert (lo, float(gam)) == (0, 0.0)
    assert {"<0.5", ">0.5"} <= seen, seen
    if pct == 0.5:
        assert {"0", "0.5"} <= seen, seen


@pytest.mark.parametrize("method", METHODS)
def test_ties(method):
    """A constant input (every order statistic tied, the adaptive span at its 1e-6 floor), an input of four levels,
    and silence (-160 dB everywhere)."""
    n = 2049
    const = np.full((n, 1), 0.25, dtype=np.float32)
    g, _ = run(const, config(method, window=1), cls="window=1")
    assert np.all(g["envelope_db"] == g["envelope_db"][0])
    if method == "adaptive":
        assert M.span(g["level"])[1] == 1e-6 and np.all(g["level"] == 0)
    levels = np.random.default_rng(1).choice(np.array([0.001, 0.01, 0.1, 1.5], dtype=np.float32), (n, 1))
    run(levels, config(method, window=1), cls="window=1")
    run(levels, config(method, window=4), cls="general")
    g, res = run(np.zeros((n, 2), dtype=np.float32), config(method), cls="general")
    assert np.all(g["envelope_db"] == -160.0) and res.noise_floor_db == -160.0
    assert not g["mask"].any() and g["output"].shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------------
# trim


@pytest.mark.parametrize("lead", [0, 1, "n+7"])
@pytest.mark.parametrize("trail", [0, 1, "n+7"])
def test_trim_edges(lead, trail):
    n, k = 2100, 37
    lead, trail = (n + 7 if v == "n+7" else v for v in (lead, trail))
    for spans in ([(0, k)], [(n - k, n)], [(0, k), (n - k, n)], [(900, 950)]):
        mask = np.zeros(n, dtype=bool)
        for a, b in spans:
            mask[a:b] = True
        g, res = run(from_mask(mask), mask_config(hold=4, fade=3, lead=lead, trail=trail), cls="masks")
        active = np.flatnonzero(g["gain"] > np.float32(1e-3))
        assert (res.start, res.stop) == (max(0, active[0] - lead), min(n, active[-1] + trail + 1))
        if spans[0][0] == 0:
            assert res.start == 0 and g["gain"][0] == 1.0
        if spans[-1][1] == n:
            assert res.stop == n and g["gain"][n - 1] == 1.0


@pytest.mark.parametrize("trim", [False, True])
def test_nothing_active(trim):
    n = 2100
    x = signal(n, 2, seed=3)
    for method in ("static", "adaptive"):
        cfg = config(method, auto_noise_floor=False, manual_noise_floor_db=10.0, trim_silence=trim)
        g, res = run(x, cfg, cls="general")
        assert not g["mask"].any() and (res.start, res.stop) == ((0, 0) if trim else (0, n))
        assert g["output"].shape == ((0, 2) if trim else (n, 2)) and not g["output"].any()


# ---------------------------------------------------------------------------------------------------------------
# PCM16


def test_pcm16_rounding_and_saturation():
    """rint ties to even, +-full scale, saturation beyond +-1, at gain 1 and at fractional gains.  32767 y is a
    half-integer only for y = +-0.5 (and +-1.5, saturated): 32767 = 7 * 31 * 151 is odd, so y = m / 2.  Ties are
    reached with x = +-0.5 at gain 1 and x = +-1.0 at gain 0.5; inputs next to (k + 0.5) / 32767 sit beside a tie.
    A loud stretch starts below the threshold (window 64 at -4.5 dB needs 39 samples of 1.0), so its first samples
    are not active and carry the fade's fractional gains: with fade 6, 2/12 and 6/12 before a run."""
    n, a = 2049, 500
    rng = np.random.default_rng(16)
    k = rng.integers(16384, 32766, n - a)
    pool = np.concatenate(([0.5, -0.5, 1.0, -1.0, 1.5, -1.5], (k + 0.5) / 32767.0 * rng.choice([-1.0, 1.0], n - a)))
    x = np.zeros((n, 2), dtype=np.float32)
    x[a:, 0] = rng.permutation(pool.astype(np.float32))[:n - a]
    x[a:, 1] = rng.permutation(pool.astype(np.float32))[:n - a]
    x[a:a + 40] = np.where(np.arange(40) % 2 == 0, 1.0, -1.0)[:, None]
    x[1200:1206, 0] = [0.5, -0.5, 1.0, -1.0, 1.5, -1.5]
    x[1200:1206, 1] = [-0.5, 0.5, -1.0, 1.0, -1.5, 1.5]
    cfg = config("static", window=64, hold=0, fade=6, auto_noise_floor=False, manual_noise_floor_db=-10.5,
                 trim_silence=False)
    g, _ = run(x, cfg, pcm16=True, cls="general")
    scaled = (x * g["gain"][:, None]).astype(np.float64) * 32767.0
    frac = np.abs(scaled) - np.floor(np.abs(scaled))
    ties = (frac == 0.5) & (np.abs(scaled) < 32767)
    fractional = (g["gain"] > 0) & (g["gain"] < 1)
    assert (ties & (scaled > 0)).any() and (ties & (scaled < 0)).any()
    assert (ties & fractional[:, None]).any() and (ties & (g["gain"] == 1)[:, None]).any()
    assert (g["gain"] == 0.5).any() and fractional.sum() >= 2
    assert (scaled > 40000).any() and (scaled < -40000).any()
    y = g["output"]
    assert y.max() == 32767 and y.min() == -32768
    assert np.array_equal(y[1200], [16384, -16384]) and np.array_equal(y[1202], [32767, -32767])
    assert np.array_equal(y[1204], [32767, -32768])
    # the same input as float32 output
    run(x, cfg, cls="general")


# ---------------------------------------------------------------------------------------------------------------
# segment tables


def _items(specs, seed=0):
    return [(signal(n, c, seed=seed + k), float(rate)) for k, (n, c, rate) in enumerate(specs)]


@pytest.mark.parametrize("method", METHODS)
def test_a_batch_of_seven_unlike_items(method):
    """Rates, windows, channel counts and lengths differ per segment; lengths of exactly one tile and one tile + 1."""
    specs = [(2048, 1, 1000), (2049, 2, 2000), (700, 3, 1000), (5000, 1, 4000), (4096, 2, 500), (90, 5, 1000), (4097, 1, 8000)]
    items = _items(specs)
    cfg = config(method, window=20, short=4, hold=130, fade=6, lead=10, trail=20)
    results = S.squelch_device(items, cfg, return_stages=True)
    assert len({r.stages["window"] for r in results}) == 5
    for (x, rate), r in zip(items, results):
        check(r, x, rate, cfg, cls="segments")
    pcm = S.squelch_device(items, cfg, pcm16=True, return_stages=True)
    for (x, rate), r in zip(items, pcm):
        check(r, x, rate, cfg, pcm16=True, cls="segments")


_MANY = [(50 + (37 * k) % 260, 1 + k % 3, 1000 * (1 + k % 2)) for k in range(130)]


@pytest.mark.parametrize("n_segs,method", [(64, "adaptive"), (65, "adaptive"), (130, "adaptive"), (65, "static"),
                                           (130, "static"), (130, "transient")])
def test_more_segments_than_one_finishing_block(n_segs, method):
    """The per-segment finishing kernels run 64 threads per block: 64 segments fill one block, 65 start a second,
    130 a third."""
    items = _items(_MANY[:n_segs], seed=100)
    cfg = config(method, window=10, short=2, hold=15, fade=4, lead=3, trail=5)
    results = S.squelch_device(items, cfg, return_stages=True)
    assert len(results) == n_segs
    for (x, rate), r in zip(items, results):
        check(r, x, rate, cfg, cls="segments")


def _run_raw(items, cfg, gaps, pcm16=False):
    """iqa_squelch on a hand-built segment table: `gaps[k]` empty tiles before segment k, the workspace zeroed."""
    torch = N.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    segs, in_off, base = [], 0, 0
    for (x, rate), gap in zip(items, gaps):
        base += gap * TILE
        n, c = x.shape
        segs.append(S._segment(n, c, rate, cfg, in_off, base))
        in_off += -(-(n * c) // 64) * 64
        base += -(-n // TILE) * TILE
    nseg = len(segs)
    host = np.zeros(in_off, dtype=np.float32)
    for (x, _), s in zip(items, segs):
        host[s.in_off:s.in_off + x.size] = x.reshape(-1)
    inp = torch.from_numpy(host).to(dev)
    table = (N.SquelchSeg * nseg)(*segs)
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    handle = N.lib()
    ws_bytes = int(handle.iqa_squelch_workspace_bytes(base, nseg))
    assert ws_bytes > 0
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.zeros(in_off, dtype=torch.int16 if pcm16 else torch.float32, device=dev)
    res_dev = torch.zeros(nseg * ctypes.sizeof(N.SquelchResult), dtype=torch.uint8, device=dev)
    params = N.SquelchParams(method=N.SQ_METHOD[cfg.method], auto_floor=int(cfg.auto_noise_floor), trim=int(cfg.trim_silence),
                             out_pcm16=int(pcm16), margin_db=float(cfg.threshold_margin_db),
                             transient_margin_db=float(cfg.transient_margin_db))
    N.call("iqa_squelch", ctypes.byref(params), table, nseg, N.ptr(table_dev), N.ptr(inp), N.ptr(out), N.ptr(res_dev),
           N.ptr(ws), ctypes.c_int64(ws_bytes), N.stream_ptr())
    results = (N.SquelchResult * nseg).from_buffer_copy(res_dev.cpu().numpy().tobytes())
    offs = {k: int(handle.iqa_squelch_stage_offset(base, nseg, v)) for k, v in N.SQ_STAGE.items()}
    outs = []
    for s, r in zip(segs, results):
        def arr(name, dtype, s=s):
            width = torch.empty(0, dtype=dtype).element_size()
            o = offs[name] + s.base * width
            return ws[o:o + s.n * width].view(dtype)

        stages = dict(envelope_db=arr("envelope_db", torch.float32), level=arr("level", torch.float32),
                      threshold=arr("threshold", torch.float32), mask=arr("mask", torch.uint8).bool(),
                      dilated=arr("dilated", torch.uint8).bool(), gain=arr("gain", torch.float32),
                      noise_floor_db=float(r.noise_floor_db), threshold_db=float(r.threshold_db), start=int(r.start),
                      stop=int(r.stop), window=int(s.window), hold=int(s.hold), fade=int(s.fade))
        n_out = int(r.stop - r.start)
        y = out[s.in_off:s.in_off + n_out * s.channels].reshape(n_out, s.channels)
        outs.append(S._DeviceResult(y, float(r.noise_floor_db), float(r.threshold_db), int(r.start), int(r.stop), stages))
    return outs


@pytest.mark.parametrize("method", METHODS)
def test_gaps_between_segment_bases(method):
    """The ABI allows bases with empty tiles between segments (the Python packer never leaves any): one tile before
    the second segment, three before the third.  Every result and every stage equals the gap-free run's, and the
    oracle's."""
    items = _items([(2049, 2, 1000), (700, 1, 2000), (4100, 3, 1000)], seed=40)
    cfg = config(method, window=20, short=4, hold=130, fade=6, lead=10, trail=20)
    dense = _run_raw(items, cfg, (0, 0, 0))
    sparse = _run_raw(items, cfg, (0, 1, 3))
    for (x, rate), a, b in zip(items, dense, sparse):
        check(b, x, rate, cfg, cls="segments")
        assert (a.noise_floor_db, a.threshold_db, a.start, a.stop) == (b.noise_floor_db, b.threshold_db, b.start, b.stop)
        for key in ("envelope_db", "threshold", "mask", "dilated", "gain") + (("level",) if method != "static" else ()):
            assert np.array_equal(a.stages[key].cpu().numpy(), b.stages[key].cpu().numpy()), key
        assert np.array_equal(a.samples.cpu().numpy(), b.samples.cpu().numpy())
    packed = S.squelch_device(items, cfg, return_stages=True)
    for a, p in zip(dense, packed):
        assert (a.start, a.stop, a.noise_floor_db) == (p.start, p.stop, p.noise_floor_db)
        assert np.array_equal(a.samples.cpu().numpy(), p.samples.cpu().numpy())
