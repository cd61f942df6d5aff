"""The one-launch form of the de-emphasis scan (csrc/demod_fused.hip: k_fused_windowed, k_fused_clear) against the float64
oracle of tests/scan_model.py, PER SAMPLE, at the sizes where its geometry changes.  Run with ``-m gpu`` on an MI355X.

Geometry (``iqa_scan_window(alpha)`` -> W, SPAN): a workgroup covers SPAN positions, the first W of them a warm-up from
state 0, the other SPAN - W its own; block 0 starts at index 0 from the carried state and writes the outgoing one.  The
sizes below are placed on the edges of that geometry; the assertions and their bounds are those of
tests/test_gpu_scan_exact.py (its helpers are used as they are): the per-sample bound with the model's floor term F, fused ==
stages bit for bit, prev bit for bit, y_last within F, peak and sums as ``check_sink``.  The floor term F is not widened
for the warm-up: the state a block ignores is a y of the same call (|y| <= S), decayed by alpha^W <= 2^-64, which is 2^-17 F.
"""
from __future__ import annotations

import importlib.util
import sys
from ctypes import byref, c_double, c_int64, c_void_p
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
X = _load("_scan_exact_helpers", "test_gpu_scan_exact.py")  # the device buffers, entry points and comparisons, read-only
G = X.G

# the sizes of the issue, from (W, SPAN); "own" = SPAN - W
SIZES = {
    "1": lambda W, S: 1,
    "W-1": lambda W, S: W - 1, "W": lambda W, S: W, "W+1": lambda W, S: W + 1,
    "own-1": lambda W, S: S - W - 1, "own": lambda W, S: S - W, "own+1": lambda W, S: S - W + 1,
    "SPAN-1": lambda W, S: S - 1, "SPAN": lambda W, S: S, "SPAN+1": lambda W, S: S + 1,
    "2own+1": lambda W, S: 2 * (S - W) + 1,
    "3own+W+5": lambda W, S: 3 * (S - W) + W + 5,
}
Z_OFFS, Y_OFFS = (0, 1), (0, 1, 2, 3)


def window(G, alpha=None):
    w, s = c_int64(-1), c_int64(-1)
    rc = G.lib.iqa_scan_window(c_double(M.ALPHA if alpha is None else alpha), byref(w), byref(s))
    return rc, int(w.value), int(s.value)


def test_window_is_the_smallest_multiple_of_512_that_forgets(G):
    rc, W, SPAN = window(G)
    assert rc == 0 and W % 512 == 0 and 0 < 2 * W <= SPAN, (rc, W, SPAN)
    assert M.ALPHA ** W <= 2.0 ** -64 < M.ALPHA ** (W - 512), (W, M.ALPHA ** W)
    assert W == 1536  # config 2: alpha^1280 is just above 2^-64


def _class_and_layout(k: int):
    """Input classes (a) FM tone, (b) noise, (c) stretches of exact zeros, (f) past the clip, and every segment layout,
    rotating over the sizes."""
    return ("a", "b", "c", "f")[k % 4], M.LAYOUTS[k % len(M.LAYOUTS)]


def check_sink_with_floor(label, got_peak, got_slots, v_gpu, blk, segs):
    """``check_sink`` for inputs with stretches of exact zeros.  The one-launch form's error per sample is ABSOLUTE,
    e <= 2^-64 S (the state a block ignores, decayed over its warm-up): a block whose whole warm-up is exact zeros puts out
    0 where the exact chain still holds alpha^k of an old state.  A square then moves by at most 2 |v| e + e^2, and
    2 |v| e - r v^2 <= e^2 / r for every v, so with check_sink's relative bound r = 2^-21 a segment of c samples is held to
    |got - want| <= r want + c e^2 (1 + 1 / r), and the total likewise.  (Measured without the floor, own+1 = 6657, layout
    s100: segment [6600, 6657) got 2.3833e-52, oracle 2.3866e-52; the floor there is 57 * 2^-107 S^2 = 3.5e-31 S^2.)
    The peak is checked as check_sink checks it."""
    want = M.sink(blk.v, segs)
    own = np.float32(np.max(np.abs(v_gpu)))
    assert got_peak == own, (label, got_peak, own)
    assert abs(float(got_peak) - float(want.peak)) <= 2.0 ** -23 * float(want.peak), (label, got_peak, want.peak)
    got = got_slots.sum(axis=1)
    assert np.isfinite(got_slots).all() and got.shape == want.sums.shape, label
    r, e2 = 2.0 ** -21, (2.0 ** -64 * blk.S) ** 2
    counts = np.diff(np.append(np.asarray(segs, dtype=np.int64), blk.v.size))
    tol = r * want.sums + counts * e2 * (1.0 + 1.0 / r)
    err = np.abs(got - want.sums)
    print(f"[scan-windowed] {label}: {len(segs)} segments, max sum err / tol {float(np.max(err / np.maximum(tol, 1e-300))):.3e}")
    bad = np.flatnonzero(err > tol)
    assert bad.size == 0, (label, "segment", bad[:5], "got", got[bad[:5]], "want", want.sums[bad[:5]], "tol", tol[bad[:5]])
    assert np.all(got_slots[counts == 0] == 0.0), (label, "a segment without samples received something")
    assert abs(got.sum() - want.sums.sum()) <= r * want.sums.sum() + blk.v.size * e2 * (1.0 + 1.0 / r), (label, "total")


@pytest.mark.parametrize("form", ["deemph", "state", "fresh"])
@pytest.mark.parametrize("size", list(SIZES))
def test_windowed_sizes_per_sample(G, size, form):
    """Every size at every z offset and every output offset, through iqa_deemphasis with a state, iqa_demodulate from a
    used state block, and iqa_demodulate_from_reset over poisoned state, peak and sums."""
    rc, W, SPAN = window(G)
    assert rc == 0
    n = SIZES[size](W, SPAN)
    cls, lay = _class_and_layout(list(SIZES).index(size))
    if form == "deemph":
        x = M.make_x("deemph", cls, n)
        blk = M.stage_deemphasis(x, M.ALPHA, 0.37)
        for x_off in Z_OFFS:
            for y_off in Y_OFFS:
                y, st = X.gpu_stage(G, "deemph", x, state=[0.37], x_off=x_off, y_off=y_off)
                X.check_block(X._id("win", form, size, n, cls, x_off, y_off), y, blk)
                assert abs(st[0] - blk.y64[-1]) <= blk.F, (size, n, st, blk.y64[-1], blk.F)
        return
    z = M.make_z(cls, n)
    segs = M.layout(lay, n)
    fresh = form == "fresh"
    st = M.State() if fresh else X.USED_STATE
    for z_off in Z_OFFS:
        z_dev = X.dev_in(G, z, z_off)
        for y_off in Y_OFFS:
            label = X._id("win", form, size, n, cls, lay, z_off, y_off)
            got = X.gpu_demod(G, "nfm", False, z_dev, segs, state_img=st.image(), fresh=fresh, y_off=y_off)
            u, blk, v_gpu, after, lin_F = X._fused_oracle(G, "nfm", False, z, z_dev, st, segs, got)
            X.check_source(label, "nfm", u, z, st.prev)
            X.check_block(label, got.audio, blk, clipped=True)
            assert np.array_equal(got.audio.view(np.uint32), np.clip(v_gpu, -M.CLIP, M.CLIP).view(np.uint32)), (label, "fused != stages")
            X.check_state(label, "nfm", got.state, after, lin_F, np.full(32, X.POISON, np.uint8) if fresh else st.image())
            (check_sink_with_floor if cls == "c" else X.check_sink)(label, got.peak, got.sums, v_gpu, blk, segs)


@pytest.mark.parametrize("tail", ["quiet", "zeros"])
def test_a_block_forgets_a_full_scale_past(G, tail):
    """3 SPAN samples of full-scale z whose phase alternates (|u| near pi, the largest state the filter can hold), then
    3 SPAN of a constant (u = 0: the output is the decaying state alone) or of exact zeros: every block that starts in
    the tail warms up over a past it must have forgotten by its first own sample."""
    rc, W, SPAN = window(G)
    assert rc == 0
    own, n = SPAN - W, 6 * SPAN
    k = np.arange(3 * SPAN, dtype=np.float64)
    z = np.empty(n, dtype=np.complex64)
    z[:3 * SPAN] = np.exp(1j * (np.pi - 0.01) * k).astype(np.complex64)  # u = pi - 0.01 per sample
    z[3 * SPAN:] = M.QUIET if tail == "quiet" else 0
    segs = M.layout("prod", n)
    st = X.USED_STATE
    z_dev = X.dev_in(G, z, 0)
    got = X.gpu_demod(G, "nfm", False, z_dev, segs, state_img=st.image())
    u, blk, v_gpu, after, lin_F = X._fused_oracle(G, "nfm", False, z, z_dev, st, segs, got)
    assert blk.S > 3.0, blk.S
    want = np.clip(blk.y64, -float(M.CLIP), float(M.CLIP))
    first_own = np.arange(own, n, own)
    err = np.abs(got.audio[first_own].astype(np.float64) - want[first_own])
    tol = M.EPS32 * np.abs(want[first_own]) + blk.F
    print(f"[scan-windowed] {tail}: first own samples {first_own.tolist()} err {err.tolist()} tol {tol.tolist()}")
    bad = first_own[err > tol]
    assert bad.size == 0, ("the first own sample of a block", bad.tolist(), "block", (bad // own).tolist(), err[err > tol].tolist(), tol[err > tol].tolist())
    X.check_block(f"win-forget-{tail}", got.audio, blk, clipped=True)
    assert np.array_equal(got.audio.view(np.uint32), np.clip(v_gpu, -M.CLIP, M.CLIP).view(np.uint32)), "fused != stages"
    X.check_state(f"win-forget-{tail}", "nfm", got.state, after, lin_F, st.image())
    X.check_sink(f"win-forget-{tail}", got.peak, got.sums, v_gpu, blk, segs)


def _deemph_alpha(G, x, alpha, y0):
    N, n = G.N, int(x.size)
    x_dev, out, work = X.dev_in(G, x.astype(np.float32), 0), X.Out(G, n, 0), X.workspace(G, n)
    st = X.dev_bytes(G, np.array([y0], dtype=np.float64))
    N.call("iqa_deemphasis", N.ptr(x_dev), c_int64(n), c_double(alpha), N.ptr(st), N.ptr(out.view), N.ptr(work), N.stream_ptr())
    return out.numpy(), st.cpu().numpy().view(np.float64)


def _demod_alpha(G, z, alpha, st, segs):
    N, t, n = G.N, G.torch, int(z.size)
    p = N.DemodParams(mode=N.DEMOD_MODE["nfm"], agc_enabled=0, deemph_alpha=alpha, dc_radius=M.DC_RADIUS,
                      agc_target=M.AGC_TARGET, agc_decay=M.AGC_DECAY)
    z_dev, state = X.dev_in(G, z, 0), X.dev_bytes(G, st.image())
    peak = t.zeros(1, dtype=t.float32, device=G.dev)
    sums = t.zeros(len(segs) * M.SLOTS, dtype=t.float64, device=G.dev)
    out, work, segs_dev = X.Out(G, n, 0), X.workspace(G, n), X.dev_bytes(G, np.asarray(segs, dtype=np.int64))
    N.call("iqa_demodulate", byref(p), N.ptr(z_dev), c_int64(n), N.ptr(state), N.ptr(segs_dev), c_int64(len(segs)), N.ptr(peak),
           N.ptr(sums), N.ptr(out.view), c_void_p(0), N.ptr(work), N.stream_ptr())
    return out.numpy(), state.cpu().numpy(), np.float32(peak.cpu().numpy()[0]), sums.cpu().numpy().reshape(len(segs), M.SLOTS)


def test_a_long_time_constant_keeps_the_three_launches(G):
    """alpha = exp(-1/3000): alpha^W <= 2^-64 needs 133 085 samples, far above half a span -- iqa_scan_window reports 1 and
    the reduce / carry / apply form still meets the bound, at 65 tiles."""
    alpha = float(np.exp(-1.0 / 3000.0))
    rc, _, _ = window(G, alpha)
    assert rc == 1
    n = 131_073
    x = M.make_x("deemph", "a", n)
    y, st = _deemph_alpha(G, x, alpha, 0.37)
    blk = M.stage_deemphasis(x, alpha, 0.37)
    X.check_block("win-guard", y, blk)
    assert abs(st[0] - blk.y64[-1]) <= blk.F, (st, blk.y64[-1], blk.F)
    for bad in (0.0, 1.0, -0.5, float("nan")):
        assert window(G, bad)[0] == 1, bad


def test_a_window_of_exactly_half_a_span(G):
    """The longest window the one-launch form takes: W = SPAN / 2, where block 1's warm-up begins at index 0.  Block 1
    does not read the state block (block 0 may already have written the outgoing state into it): it starts from state 0
    with the sample at index 0 taken as 0, which costs alpha^W |y[0]| <= 2^-64 S.  Stage and fused forms, a used state."""
    _, _, SPAN = window(G)
    alpha = float(np.exp(-64.0 * np.log(2.0) / (SPAN // 2 - 100)))
    rc, W, span = window(G, alpha)
    assert rc == 0 and span == SPAN and W == SPAN // 2, (rc, W, span)
    st = X.USED_STATE
    for n in (W, W + 1, 2 * W + 3, 5 * W + 77):
        z = M.make_z("f" if n == 2 * W + 3 else "a", n)
        segs = M.layout("prod", n)
        audio, state, peak, sums = _demod_alpha(G, z, alpha, st, segs)
        u = X.gpu_source(G, "nfm", X.dev_in(G, z, 0), st.prev)
        blk = M.stage_deemphasis(u, alpha, st.de_y)
        v_gpu, st_after = _deemph_alpha(G, u, alpha, st.de_y)
        label = f"win-half-span-{n}"
        X.check_block(label, v_gpu, blk)
        X.check_block(label, audio, blk, clipped=True)
        assert np.array_equal(audio.view(np.uint32), np.clip(v_gpu, -M.CLIP, M.CLIP).view(np.uint32)), (label, "fused != stages")
        X.check_state(label, "nfm", state, M.advance("nfm", st, z, u, blk), blk.F, st.image())
        assert abs(st_after[0] - blk.y64[-1]) <= blk.F
        X.check_sink(label, peak, sums, v_gpu, blk, segs)


def test_resident_runner_reuses_a_slot_from_a_clean_state():
    """ResidentCaptureRunner.submit(..., resident=True), two slots, three submits (config 1's shape cut to 0.2 s): the
    third runs on the first's slot, whose decoder has seen a LOUDER capture -- its state block, peak and per-chunk sums are
    put back on the aux stream -- and must return the PCM16, peak and chunk levels that the quieter capture gives on a
    runner of its own.  A peak that was not cleared would stay the louder one; sums that were not cleared would add up."""
    import torch

    import iq_to_audio_amd as A
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.batch import ResidentCaptureRunner
    from oracle import cpu_ref as O

    A.native.lib()
    A.native.require_gpu()
    fs, secs, f_off = 2.5e6, 0.2, 25e3
    n = int(round(fs * secs))
    d, fs_ch = P.choose_decimation(fs, 96_000.0)
    taps = A.design_channel_filter(fs, 12_500.0, d)
    _, slack = ResidentCaptureRunner.padded_capture_frames(d, len(taps))

    def resident(seed):
        buf = torch.zeros(2 * (n + slack), dtype=torch.int16, device=D.device())
        buf[: 2 * n] = torch.from_numpy(O.synth_capture_s16(fs, secs, f_off, seed=seed).reshape(-1)).to(D.device())
        return buf

    def make_runner():
        return ResidentCaptureRunner(taps, sample_rate=fs, freq_offset=f_off, decimation=d, fs_channel=fs_ch,
                                     chunk=P.tune_chunk_size(fs, 1_048_576), n_frames=n, slots=2)

    def run(runner, buf):
        t = runner.submit(buf[: 2 * n], enclosing=buf, lead_frames=0, resident=True)
        r = runner.collect(t)
        return t["slot"], r["pcm_host"].numpy().copy(), r["demod"].peak, list(r["demod"].chunk_rms_dbfs())

    bufs = [resident(42), resident(43)]
    torch.cuda.synchronize()
    alone = [run(make_runner(), b) for b in bufs]
    assert alone[0][2] != alone[1][2] and alone[0][2] > 0.0 and alone[1][2] > 0.0, (alone[0][2], alone[1][2])
    loud, quiet = (0, 1) if alone[0][2] > alone[1][2] else (1, 0)
    runner = make_runner()
    seen = [run(runner, bufs[loud]), run(runner, bufs[loud]), run(runner, bufs[quiet])]
    assert seen[2][0] is seen[0][0] and seen[1][0] is not seen[0][0]
    assert len(seen[2][3]) == len(runner.starts) and np.abs(seen[2][1]).max() > 0
    for got, want in ((seen[0], alone[loud]), (seen[1], alone[loud]), (seen[2], alone[quiet])):
        assert np.array_equal(got[1], want[1])
        # (the sums are float64 atomics of several blocks in an order that may differ from run to run: 2^-52 relative per
        # addition, far below 1e-9 dB)
        assert got[2] == want[2] and np.allclose(got[3], want[3], rtol=0, atol=1e-9), (got[2], want[2])
    assert seen[2][2] < seen[0][2]
