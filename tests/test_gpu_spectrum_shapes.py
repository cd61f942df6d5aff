"""The spectrum kernels (csrc/spectrum.hip: k_psd_window in its three ingest builds, rocFFT behind the plan cache,
k_psd_finish, k_pair_average) against the float64 model of tests/spectrum_model.py, through the C ABI at small sizes:
one thread block and its guard, the 256-wide block edge, odd and non-power-of-two lengths, use < nfft in frames after the
first, every format and iq_order (which the Python wrapper never reaches: it converts to complex64 first), first > 0 with
every hop, the NULL / non-NULL combinations of the three outputs, sum_db across calls, more plans than the cache keeps.
tests/test_spectrum_model_host.py asserts the tables, measures the constant of the bound and proves that no bin of a noisy
case needs a mask.

Every call writes into buffers with 64 elements of a fill pattern behind them (the work buffer included), which must
survive; the samples are followed, inside their allocation, by NaN / 32767 / 255.  Values: every bin of every frame
satisfies |10^(dB / 10) - 1e-18 - p| <= M.power_bound (derivation: the model's docstring).
"""
from __future__ import annotations

import importlib.util
import sys
from ctypes import c_double, c_int32, c_int64
from pathlib import Path

import numpy as np
import pytest

from iq_to_audio_amd import _dev as D
from iq_to_audio_amd import _native as N
from oracle import cpu_ref as O


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load("spectrum_model")

pytestmark = pytest.mark.gpu

GUARD = 64
FILL64 = 0x7FF8A5A5A5A5A5A5  # NaN patterns no result produces
FILL32 = 0x7FC5A5A5
MARGIN = 1024  # hostile samples behind the call's samples
RATIOS: dict = {}
_CACHE: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    N.lib()
    N.require_gpu()
    yield
    for nfft, ratio in sorted(RATIOS.items()):
        print(f"\nspectrum [nfft {nfft}]: largest |p_gpu - p| / bound = {ratio:.4f}")


def _guarded(n: int, kind: str):
    torch = D.torch_mod()
    if kind == "f64":
        return torch.full((n + GUARD,), FILL64, dtype=torch.int64, device=D.device())
    return torch.full((n + GUARD,), FILL32, dtype=torch.int32, device=D.device())


def _read(t, n: int, kind: str, what: str):
    h = t.cpu().numpy()
    fill = FILL64 if kind == "f64" else FILL32
    assert np.all(h[n:] == fill), f"a store landed behind {what}"
    return h[:n].copy()


def psd_frames(raw, fmt, order, first, hop, n_frames, nfft, use, window, scale, *, want64=True, want32=True, sum_start=None,
               n_samples=None, calls=1, fmt_code=None, order_code=None):
    """iqa_psd_frames (``calls`` times into the same buffers) with guarded outputs and work buffer.  Returns a dict of
    numpy arrays: "f64" / "f32" [n_frames][nfft] (as raw bits where nothing was written), "sum" [nfft], and "untouched":
    whether every output still holds its fill (the refusals)."""
    torch = D.torch_mod()
    raw = np.ascontiguousarray(raw).reshape(-1)
    host = np.full(raw.size + 2 * MARGIN, M.HOSTILE[fmt], dtype=raw.dtype)
    host[:raw.size] = raw
    samples = D.from_numpy(host)
    win = D.from_numpy(np.asarray(window, dtype=np.float64))
    rows = max(n_frames, 0) * nfft
    work = _guarded(2 * rows, "f64")
    o64 = _guarded(rows, "f64") if want64 else None
    o32 = _guarded(rows, "f32") if want32 else None
    acc = None
    if sum_start is not None:
        acc = _guarded(nfft, "f64")
        acc[:nfft] = D.from_numpy(np.asarray(sum_start, dtype=np.float64)).view(torch.int64)
    n_samples = raw.size // 2 if n_samples is None else n_samples
    try:
        for _ in range(calls):
            N.call("iqa_psd_frames", c_int32(M.FMT_CODE[fmt] if fmt_code is None else fmt_code),
                   c_int32(M.ORDER_CODE[order] if order_code is None else order_code), N.ptr(samples), c_int64(n_samples), c_int64(first),
                   c_int64(hop), c_int32(n_frames), c_int32(nfft), c_int32(use), N.ptr(win), c_double(scale), N.ptr(work), N.ptr(o64),
                   N.ptr(o32), N.ptr(acc), N.stream_ptr())
    finally:
        out = {"work": _read(work, 2 * rows, "f64", "the work buffer")}
        out["f64"] = None if o64 is None else _read(o64, rows, "f64", "psd_db").reshape(max(n_frames, 0), nfft)
        out["f32"] = None if o32 is None else _read(o32, rows, "f32", "psd_db_f32").reshape(max(n_frames, 0), nfft)
        out["sum"] = None if acc is None else _read(acc, nfft, "f64", "sum_db")
        out["untouched"] = (np.all(out["work"] == FILL64) and (o64 is None or np.all(out["f64"] == FILL64))
                            and (o32 is None or np.all(out["f32"] == FILL32)))
        _CACHE["last"] = out
    for key in ("f64", "sum"):
        if out[key] is not None:
            out[key] = out[key].view(np.float64)
    if out["f32"] is not None:
        out["f32"] = out["f32"].view(np.float32)
    return out


def pair_average_rows(rows, n_rows=None, n_cols=None):
    """iqa_pair_average_rows into a guarded output at an offset view (fill in front and behind)."""
    torch = D.torch_mod()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n_rows = rows.shape[0] if n_rows is None else n_rows
    n_cols = rows.shape[1] if n_cols is None else n_cols
    n_out = ((max(n_rows, 0) + 1) // 2) * max(n_cols, 0)
    src = D.from_numpy(np.concatenate([rows.reshape(-1), np.full(GUARD, np.nan, dtype=np.float32)]))
    buf = torch.full((GUARD + n_out + GUARD,), FILL32, dtype=torch.int32, device=D.device())
    try:
        N.call("iqa_pair_average_rows", N.ptr(src), c_int32(n_rows), c_int32(n_cols), N.ptr(buf[GUARD:]), N.stream_ptr())
    finally:
        h = buf.cpu().numpy()
        assert np.all(h[:GUARD] == FILL32) and np.all(h[GUARD + n_out:] == FILL32), "a store landed outside the output rows"
    return h[GUARD:GUARD + n_out].copy()


def check_values(case, got_db, *, name=None):
    """Every bin of every frame inside the bound, in linear power; no mask.  Records |err| / bound per nfft."""
    a = case.args()
    p = M.power(*a)
    bound = M.power_bound(*a, p=p)
    got = np.asarray(got_db, dtype=np.float64)
    assert got.shape == p.shape and np.isfinite(got).all(), name or case.name
    err = np.abs(M.from_db(got) - p)
    ratio = float(np.max(err / bound))
    if case.kind == "noisy":
        RATIOS[case.nfft] = max(RATIOS.get(case.nfft, 0.0), ratio)
    bad = np.argwhere(~(err <= bound))
    assert bad.size == 0, (f"{name or case.name}: {bad.shape[0]} of {p.size} bins outside the bound; first at frame {bad[0][0]} bin "
                           f"{bad[0][1]}: |p_gpu - p| = {err[tuple(bad[0])]:.3e}, bound {bound[tuple(bad[0])]:.3e}, p = {p[tuple(bad[0])]:.3e}")
    return ratio


def run_case(case, **kw):
    return psd_frames(*case.args(), **kw)


# ---------------------------------------------------------------------------------------------------------------
# iqa_psd_frames


@pytest.mark.parametrize("case", M.SIZE_CASES, ids=lambda c: c.name)
def test_nfft_and_use(case):
    """nfft in {2, 3, 255, 256, 257, 999, 1024} x use in {1, nfft - 1, nfft} x 1 and 3 frames: the zero padding behind
    `use` in every frame, Bluestein and power-of-two plans, one and several thread blocks per frame."""
    out = run_case(case, want32=False)
    check_values(case, out["f64"])


@pytest.mark.parametrize("case", M.FORMAT_CASES, ids=lambda c: c.name)
def test_formats_and_orders(case):
    """s16 / u8 / f32 x the four iq_order values at nfft 256 and 257, the formats' extreme values inside the frames, Q at
    half the gain of I and tones of unequal strength either side of 0: a swap or a lost negation moves every bin."""
    out = run_case(case, want32=False)
    check_values(case, out["f64"])
    # what agreeing with this order's model excludes: a lost swap or a lost negation (the mirrored spectrum, far outside the
    # bound on this input).  Losing both turns the frame by -j, which no power spectrum shows: "iq" | "qi_inv" and "qi" | "iq_inv"
    # are the same to this entry point (the mixer's identity test tells all four apart).
    p = M.power(*case.args())
    for other in M.ORDERS:
        a = list(case.args())
        a[2] = other
        gap = np.max(np.abs(M.power(*a) - p) / M.power_bound(*case.args(), p=p))
        assert gap == 0 if M.ORDER_CODE[other] ^ M.ORDER_CODE[case.order] in (0, 3) else gap > 1e6


@pytest.mark.parametrize("case", M.GEOMETRY_CASES, ids=lambda c: c.name)
def test_frame_geometry(case):
    """1, 2 and 65 frames x hop in {1, nfft / 4, nfft, nfft + 7} x first in {0, 5}; the last frame ends exactly at
    n_samples (NaN / 32767 / 255 behind it), and one sample fewer is refused with nothing written."""
    out = run_case(case)
    check_values(case, out["f64"])
    np.testing.assert_array_equal(out["f32"].view(np.uint32), out["f64"].astype(np.float32).view(np.uint32))
    with pytest.raises(ValueError):
        run_case(case, n_samples=case.n_samples - 1)
    assert _CACHE["last"]["untouched"]


@pytest.mark.parametrize("case", M.TONE_CASES + M.ZERO_CASES, ids=lambda c: c.name)
def test_bin_placement(case):
    """A window of ones over one complex exponential on bin b: output bin shift_index^-1(b) carries nfft / 4, every
    other bin only the float32 rounding of the exponential -- position asserted, values in linear power under the bound.
    All-zero frames (128 for u8): every bin at the floor."""
    out = run_case(case, want32=False)
    check_values(case, out["f64"])
    if case.kind == "tone":
        lin = M.from_db(out["f64"][0])
        k = int(np.argmax(lin))
        assert M.shift_index(k, case.nfft) == case.bin and abs(lin[k] - case.nfft / 4.0) < 1e-6 * case.nfft
        assert np.max(np.delete(lin, k)) < 1e-9 * lin[k]
    else:
        assert np.max(np.abs(out["f64"] + 180.0)) < 1e-9


def test_outputs_in_every_combination_and_sum_db_across_calls():
    """float64 only, float32 only, both, neither (sum_db alone): the same values whichever are asked for; float32 is
    float32(float64) bit for bit; sum_db, started from a random vector and called twice, is the start plus, per call,
    the in-order float64 sum over the frames of the float64 rows the GPU itself returned -- exactly."""
    case = M.OUTPUT_CASE
    start = np.random.default_rng(2).normal(scale=50.0, size=case.nfft)
    both = run_case(case, sum_start=start, calls=2)
    check_values(case, both["f64"])
    rows = both["f64"]
    np.testing.assert_array_equal(both["f32"].view(np.uint32), rows.astype(np.float32).view(np.uint32))
    acc = np.zeros(case.nfft)
    for f in range(case.n_frames):
        acc = acc + rows[f]
    want_sum = (start + acc) + acc
    np.testing.assert_array_equal(both["sum"].view(np.uint64), want_sum.view(np.uint64))
    assert np.all(start != 0) and not np.array_equal((start + acc) + acc, acc)
    only64 = run_case(case, want32=False)
    np.testing.assert_array_equal(only64["f64"].view(np.uint64), rows.view(np.uint64))
    only32 = run_case(case, want64=False)
    np.testing.assert_array_equal(only32["f32"].view(np.uint32), both["f32"].view(np.uint32))
    neither = run_case(case, want64=False, want32=False, sum_start=start, calls=2)
    np.testing.assert_array_equal(neither["sum"].view(np.uint64), want_sum.view(np.uint64))
    once = run_case(case, want64=False, want32=False, sum_start=start)
    np.testing.assert_array_equal(once["sum"].view(np.uint64), (start + acc).view(np.uint64))


def test_more_plans_than_the_cache_keeps():
    """Ten distinct (nfft, n_frames) plans in sequence on the current stream (the cache keeps 8: the first two are
    evicted behind a stream wait and destroyed), the first shape again (made anew), then a third time on a second
    stream (the cached plan moves streams): every result inside its bound."""
    torch = D.torch_mod()
    for case in M.PLAN_CASES:
        check_values(case, run_case(case, want32=False)["f64"])
    first = M.PLAN_CASES[0]
    again = run_case(first, want32=False)["f64"]
    check_values(first, again, name=first.name + " (again)")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run_case(first, want32=False)["f64"]
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    check_values(first, third, name=first.name + " (second stream)")
    np.testing.assert_array_equal(third.view(np.uint64), again.view(np.uint64))


def test_refusals_write_nothing():
    case = M.OUTPUT_CASE
    a = dict(zip(("raw", "fmt", "order", "first", "hop", "n_frames", "nfft", "use", "window", "scale"), case.args()))
    for bad in (dict(use=case.nfft + 1), dict(nfft=1, use=1), dict(hop=0), dict(first=-1), dict(fmt_code=3), dict(order_code=4),
                dict(scale=0.0), dict(hop=1 << 62), dict(n_frames=-1), dict(use=0)):
        kw = dict(a)
        extra = {k: bad[k] for k in ("fmt_code", "order_code") if k in bad}
        kw.update({k: v for k, v in bad.items() if k not in extra})
        if kw["use"] > len(kw["window"]):
            kw["window"] = np.ones(kw["use"])
        with pytest.raises(ValueError):
            psd_frames(kw["raw"], kw["fmt"], kw["order"], kw["first"], kw["hop"], kw["n_frames"], kw["nfft"], kw["use"], kw["window"],
                       kw["scale"], **extra)
        assert _CACHE["last"]["untouched"], bad


def test_null_pointers():
    """A NULL sample pointer with frames to do is refused; no frames is fine with every pointer NULL."""
    null = N.ptr(None)
    with pytest.raises(ValueError):
        N.call("iqa_psd_frames", c_int32(2), c_int32(0), null, c_int64(1000), c_int64(0), c_int64(8), c_int32(2), c_int32(16), c_int32(16),
               N.ptr(D.from_numpy(np.ones(16))), c_double(1.0), N.ptr(D.empty(64, "float64")), null, null, null, N.stream_ptr())
    N.call("iqa_psd_frames", c_int32(2), c_int32(0), null, c_int64(0), c_int64(0), c_int64(8), c_int32(0), c_int32(16), c_int32(16),
           null, c_double(1.0), null, null, null, null, N.stream_ptr())


# ---------------------------------------------------------------------------------------------------------------
# iqa_pair_average_rows


@pytest.mark.parametrize("n_cols", M.PAIR_COLS)
@pytest.mark.parametrize("n_rows", M.PAIR_ROWS)
def test_pair_average_rows(n_rows, n_cols):
    """Bit-equal to the float64 mean rounded to float32, an odd last row copied; ties (to even), opposite signs and
    denormals planted in rows 0 | 1."""
    rows = M.pair_rows(n_rows, n_cols)
    got = pair_average_rows(rows)
    np.testing.assert_array_equal(got.view(np.uint32), M.pair_average(rows).reshape(-1).view(np.uint32))


def test_pair_average_rows_edges():
    rows = M.pair_rows(2, 4)
    assert pair_average_rows(rows, n_rows=0).size == 0  # writes nothing (the guards are checked inside)
    with pytest.raises(ValueError):
        pair_average_rows(rows, n_cols=0)


# ---------------------------------------------------------------------------------------------------------------
# the Python layer


@pytest.mark.parametrize("name,nfft,hop,max_slices,sizes", M.WATERFALL_CASES, ids=[c[0] for c in M.WATERFALL_CASES])
def test_streaming_waterfall_against_the_oracle(name, nfft, hop, max_slices, sizes):
    """frames and times exact; avg on every bin within the dB distance the power bound allows (plus the rounding of the
    float64 sum over the frames); matrix on every bin within that plus one float32 ulp for the conversion and one per
    reduction level."""
    from iq_to_audio_amd import spectrum as S

    fs = M.SAMPLE_RATE
    chunks = M.waterfall_chunks(sizes)
    freqs, avg, wf, frames = S.streaming_waterfall(chunks, fs, nfft=nfft, hop=hop, max_slices=max_slices)
    freqs_o, avg_o, times_o, matrix_o, frames_o = O.streaming_waterfall(chunks, fs, nfft=nfft, hop=hop, max_slices=max_slices)
    assert frames == frames_o and wf.matrix.shape == matrix_o.shape and wf.matrix.dtype == np.float32
    np.testing.assert_array_equal(freqs, freqs_o)
    np.testing.assert_array_equal(wf.times, times_o)
    blocks = [b for b in chunks if b is not None and b.size]
    raw = np.concatenate(blocks).view(np.float32)
    w = np.hanning(nfft).astype(np.float64)
    scale = M.scale_of(w, fs)
    tol = np.zeros(nfft)
    for _, s0 in O.sliding_window_starts([b.size for b in blocks], nfft, hop):
        p = M.power(raw, "f32", "iq", s0, 1, 1, nfft, nfft, w, scale)
        tol = np.maximum(tol, M.db_tolerance(p, M.power_bound(raw, "f32", "iq", s0, 1, 1, nfft, nfft, w, scale, p=p))[0])
    assert tol.max() < 5e-6
    biggest = float(np.max(np.abs(matrix_o)))
    tol_avg = tol + frames * M.EPS64 * biggest  # each of the `frames` additions rounds the running sum, below frames * biggest
    assert np.all(np.abs(avg - avg_o) <= tol_avg), float(np.max(np.abs(avg - avg_o) / tol_avg))
    ulp32 = float(np.spacing(np.float32(biggest)))
    tol_m = tol[None, :] + (1 + M.reductions(frames, max_slices)) * ulp32
    err = np.abs(wf.matrix.astype(np.float64) - matrix_o.astype(np.float64))
    assert np.all(err <= tol_m), float(np.max(err / tol_m))
