"""The 48 kHz resampler (csrc/demod.hip: k_resample in its four taps-per-lane builds and three output forms, the
unstaged path, k_resample_long) against the float64 model of tests/resampler_model.py, at the shapes where the kernel's
own structure changes: waves that run more steps than the LDS ring has windows (ring wrap, slot refill, a counted wait
with real younger DMAs behind it), the row lengths at the limits of the builds, j0 > 0, stream lengths that are no
multiple of a DMA lane or shorter than one, and the PCM16 quantiser at its ties, its limits and non-finite values.
tests/test_resampler_model_host.py asserts that every shape here reaches the path its test names.

Every call goes through the C ABI into outputs with 64 guard elements on each side; the guards must survive (the
dropped stores at RS_NOWHERE, the descriptors cut at n_out).  The input is uniform noise in (-0.9, 0.9): no tone and no
period, so a stale or shifted window is an O(1) error.  The float32 output must be float32(y64) bit for bit
(M.check: only outputs whose float64 value lies within the evaluation error of a rounding midpoint may take the
neighbouring float, and their share is capped before the GPU's value is looked at).

Each case runs once.  A stale window can depend on timing: a pass is evidence, not proof.
"""
from __future__ import annotations

from ctypes import c_int32, c_int64

import numpy as np
import pytest
import resampler_model as M

from iq_to_audio_amd import _dev as D
from iq_to_audio_amd import _native as N
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

FORMS = ("f32", "pcm16", "both")
GUARD = 64
Y_GUARD = 0x7FC5A5A5  # a NaN pattern no sum produces
P_GUARD = 0x5A5B
STATS: dict = {}
_FULL: dict = {}
RATE_C2 = M.RATE_C2
reference = M.reference


@pytest.fixture(scope="module", autouse=True)
def _midpoint_report():
    N.lib()
    N.require_gpu()
    yield
    for name, (excepted, n_out, other_side) in sorted(STATS.items()):
        print(f"\nresampler [{name}]: {excepted} of {n_out} outputs within the bound of a rounding midpoint, "
              f"{other_side} of them on the other side of it")


def resampler(fs: float):
    from iq_to_audio_amd.processing import Resampler48k

    return Resampler48k(fs)


def run(x, fs: float, form: str, *, j0: int = 0, n_out: int | None = None):
    """iqa_resample into guarded outputs.  Returns (y, pcm) as numpy (None where the form has none)."""
    torch = D.torch_mod()
    rs = resampler(fs)
    n_in = 0 if x is None else int(x.size)
    if n_out is None:
        n_out = rs.plan.n_out(n_in) - j0
    xd = D.to_device(x, "float32") if n_in else None
    yg = torch.full((n_out + 2 * GUARD,), Y_GUARD, dtype=torch.int32, device=D.device()) if form != "pcm16" else None
    pg = torch.full((n_out + 2 * GUARD,), P_GUARD, dtype=torch.int16, device=D.device()) if form != "f32" else None
    N.call("iqa_resample", N.ptr(xd), c_int64(n_in), N.ptr(rs.table_dev), c_int32(rs.plan.up), c_int32(rs.plan.down),
           c_int32(rs.plan.half_taps), c_int64(j0), c_int64(n_out), N.ptr(None if yg is None else yg[GUARD:]),
           N.ptr(None if pg is None else pg[GUARD:]), N.stream_ptr())
    out = []
    for g, pattern in ((yg, Y_GUARD), (pg, P_GUARD)):
        if g is None:
            out.append(None)
            continue
        h = g.cpu().numpy()
        assert np.all(h[:GUARD] == pattern) and np.all(h[GUARD + n_out:] == pattern), "a store landed outside [0, n_out)"
        out.append(h[GUARD:GUARD + n_out].copy())
    y, pcm = out
    return (None if y is None else y.view(np.float32)), pcm


def pin(name: str, y_gpu, y, a, row):
    """M.check, and the near-midpoint share of the case for the report."""
    excepted = M.check(y_gpu, y, a, row)
    other = int(np.count_nonzero(y_gpu.view(np.uint32) != M._rounded(y).view(np.uint32)))
    STATS[name] = (excepted, y.size, other)


def run_both(name: str, x, fs: float, y, a, row):
    """Form "both": float32 pinned to the model, PCM16 the quantiser of the GPU's own float32."""
    y_gpu, pcm = run(x, fs, "both")
    assert y_gpu.size == y.size == pcm.size
    pin(name, y_gpu, y, a, row)
    np.testing.assert_array_equal(pcm, O.float_to_pcm16(y_gpu))
    return y_gpu, pcm


def full(fs: float, n: int):
    """The whole stream's (y, pcm) in form "both", pinned to the model; computed once per stream."""
    key = (fs, n)
    if key not in _FULL:
        x, y, a, row = reference(fs, n)
        _FULL[key] = run_both(f"{fs:.0f} Hz x {n}", x, fs, y, a, row)
    return _FULL[key]


# ---------------------------------------------------------------------------------------------------------------
# long waves: ring wrap, slot refill, the counted wait


@pytest.mark.parametrize("fs,n", M.LONG_WAVES, ids=lambda v: f"{v:.0f}")
def test_waves_longer_than_the_ring(fs, n):
    """A wave runs 11 to 14 steps: windows land in every ring slot, slots are refilled after they were read, and the
    counted wait has the DMAs of RS_AHEAD younger windows and the stores of two groups behind it -- with one output
    plane (float32 alone, PCM16 alone) and with two."""
    p = M.paths(fs, n)
    assert p["kernel"] == "staged" and p["g_per"] > M.RS_RING and p["g_per"] % M.RS_GROUP and p["unstaged_groups"] == 0
    x = reference(fs, n)[0]
    y_both, pcm_both = full(fs, n)
    y_only, _ = run(x, fs, "f32")
    _, pcm_only = run(x, fs, "pcm16")
    np.testing.assert_array_equal(y_only.view(np.uint32), y_both.view(np.uint32))
    np.testing.assert_array_equal(pcm_only, pcm_both)


# ---------------------------------------------------------------------------------------------------------------
# the row lengths at which the build changes


@pytest.mark.parametrize("fs", M.CLASS_LIMITS, ids=lambda v: f"{v:.0f}")
def test_row_lengths_at_the_limits_of_the_builds(fs):
    """Rows of 67 | 69, 95, 127, 191 | 193 taps: the last row of each taps-per-lane build (one lane's last tap is
    masked to zero), the first of the next, and the first row of k_resample_long.  The 191-tap row's one wave is
    unstaged (15 down / up > SPREAD)."""
    full(fs, 30_011)


# ---------------------------------------------------------------------------------------------------------------
# j0 > 0


@pytest.mark.parametrize("fs,n,j0,cnt", M.LATER_STRETCHES, ids=lambda v: f"{v:.0f}")
def test_a_later_stretch_equals_the_slice_of_the_whole_stream(fs, n, j0, cnt):
    """Outputs [j0, j0 + cnt) through the C ABI against the same outputs of the whole stream's run, bit for bit, beside
    the float32 plane and PCM16 alone: the residues of (j0 + jj) mod up start elsewhere, one wave's wrap around `up`
    (unstaged), g_all and the split follow cnt."""
    y_all, pcm_all = full(fs, n)
    assert j0 + cnt <= y_all.size
    x = reference(fs, n)[0]
    y, pcm = run(x, fs, "both", j0=j0, n_out=cnt)
    np.testing.assert_array_equal(y.view(np.uint32), y_all[j0:j0 + cnt].view(np.uint32))
    np.testing.assert_array_equal(pcm, pcm_all[j0:j0 + cnt])
    _, pcm = run(x, fs, "pcm16", j0=j0, n_out=cnt)
    np.testing.assert_array_equal(pcm, pcm_all[j0:j0 + cnt])


# ---------------------------------------------------------------------------------------------------------------
# stream ends


@pytest.mark.parametrize("fs", M.END_RATES, ids=lambda v: f"{v:.0f}")
def test_stream_lengths_at_the_edges_of_a_dma_lane(fs):
    """n_in % 4 = 1, 2, 3 (the last 16-byte DMA lane straddles the end of x), a stream shorter than a row (every window
    hangs over both ends) and streams shorter than one DMA lane, in the 24 / 32 / 48 taps-per-lane builds and the long
    kernel."""
    x_all = reference(fs, 30_011)[0]
    for n in M.END_LENGTHS:
        x = x_all[:n].copy()
        y, a, row = M.y64(x, fs)
        assert n >= 30_009 or n < row
        y_gpu, _ = run_both(f"{fs:.0f} Hz x {n}", x, fs, y, a, row)
        assert y_gpu.size == M.n_out_of(fs, n) and np.any(y_gpu != 0)


@pytest.mark.parametrize("fs,j0", [(RATE_C2, 0), (RATE_C2, 23_999), (285_000.0, 0), (288_000.0, 0)], ids=lambda v: f"{v:.0f}")
def test_an_empty_stream_gives_zeros(fs, j0):
    """n_in = 0 with x NULL and n_out = 7: a sum over nothing, whatever the waves of a stream at this rate and j0 would
    do -- staged, wrapped around `up` (unstaged: loads of x[clamped index], which an empty stream does not have),
    unstaged by its ratio, the long kernel."""
    for form in FORMS:
        y, pcm = run(None, fs, form, j0=j0, n_out=7)
        assert y is None or (y.size == 7 and not y.view(np.uint32).any())
        assert pcm is None or (pcm.size == 7 and not pcm.any())


def test_no_outputs_writes_nothing():
    x = M.stream(4096)
    for form in FORMS:
        run(x, RATE_C2, form, n_out=0)
        run(x, RATE_C2, form, j0=1_000, n_out=0)


# ---------------------------------------------------------------------------------------------------------------
# PCM16 values


def to_pcm16(y: np.ndarray) -> np.ndarray:
    torch = D.torch_mod()
    pg = torch.full((y.size + 2 * GUARD,), P_GUARD, dtype=torch.int16, device=D.device())
    N.call("iqa_float_to_pcm16", N.ptr(D.to_device(y, "float32")), c_int64(y.size), N.ptr(pg[GUARD:]), N.stream_ptr())
    h = pg.cpu().numpy()
    assert np.all(h[:GUARD] == P_GUARD) and np.all(h[GUARD + y.size:] == P_GUARD)
    return h[GUARD:GUARD + y.size].copy()


def crafted() -> np.ndarray:
    ties = [(k + 0.5) / 32768.0 for k in (0, 1, 2, 3, 4, 5, 254, 255, 16_382, 16_383, 32_765, 32_766)]
    v = ties + [32_767.5 / 32768.0, 1.0, 1.5, 0.0, float(np.finfo(np.float32).smallest_subnormal), float("inf")]
    v = np.array(v + [-e for e in v], dtype=np.float32)
    assert np.array_equal(v.astype(np.float64)[:12] * 32768.0 % 1.0, np.full(12, 0.5))  # the ties are exact in float32
    return v


def test_quantiser_at_ties_limits_and_non_finite_values():
    v = crafted()
    want = O.float_to_pcm16(v)
    assert want[0] == 0 and want[1] == 2 and want[12] == 32767 and want[18 + 12] == -32768  # half to even; saturated
    np.testing.assert_array_equal(to_pcm16(v), want)
    # NaN: where pcm16_of's fmax / fmin send it (the numpy oracle is undefined there)
    np.testing.assert_array_equal(to_pcm16(np.array([np.nan, -np.nan, 0.25], dtype=np.float32)), np.array([-32768, -32768, 8192], dtype=np.int16))


@pytest.mark.parametrize("head", ["finite", "inf"])
def test_fused_quantiser_saturates_like_the_stand_alone_one(head):
    """The PCM16 written beside (and instead of) the float32 plane is the quantiser of that float32 value: saturated at
    both limits, through zero, and -- behind one +inf sample, whose row products are +-inf and, at the taps that are
    zero, NaN -- where iqa_float_to_pcm16 sends the non-finite values."""
    fs, x = 96_000.0, M.saturating_stream(M.SATURATING_N)
    if head == "inf":
        x = np.concatenate([np.array([np.inf], dtype=np.float32), x])
    y, pcm = run(x, fs, "both")
    finite = np.isfinite(y)
    if head == "finite":
        assert finite.all()
        pin("96000 Hz saturating", y, *M.y64(x, fs))
    else:
        assert 0 < np.count_nonzero(~finite) < 40 and np.isinf(y).any()
    assert y[finite].max() > 1.0 and y[finite].min() < -1.0
    assert (pcm == 32767).any() and (pcm == -32768).any() and (np.abs(pcm.astype(np.int32)) <= 1).any()
    np.testing.assert_array_equal(pcm[finite], O.float_to_pcm16(y[finite]))
    np.testing.assert_array_equal(pcm[~finite], to_pcm16(y)[~finite])
    np.testing.assert_array_equal(run(x, fs, "pcm16")[1], pcm)
    np.testing.assert_array_equal(run(x, fs, "f32")[0].view(np.uint32), y.view(np.uint32))
