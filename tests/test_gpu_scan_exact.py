"""The demodulator's scan engine (csrc/demod_fused.hip: k_fused_reduce / k_fused_carry / k_fused_apply), the stand-alone
sink (k_writer_clip), iqa_mean_power and iqa_raw_level against the float64 oracle of tests/scan_model.py, PER SAMPLE.
Run with ``-m gpu`` on an MI355X.

What is asserted ("The scan engine per sample"):

  stage entry points, fused modes without AGC   |got - y64| <= 2^-24 |y64| + F      (one float32 rounding)
  AGC                                           |got - x g64| <= 3 * 2^-24 |x g64| + |x| F
  floor term                                    F = 64 * 2^-53 * S / (1 - A)        (scan_model.floor_term: derived)
  source stages                                 real exact, envelope 1 ulp, discriminator atol 1e-6 (modulo 2 pi where
                                                |want| > pi - 1e-5: the only exclusion, < 1 in 10 000 samples -- checked on
                                                the CPU in test_scan_model_host.py)
  peak                                          == max |v| of the stage entry point's unclipped output, bit for bit, and
                                                within 2^-23 of the oracle's
  per-segment sums                              the eight slots add up to the oracle's float64 sum within 2^-21 relative,
                                                exactly 0 where the oracle's is 0; the total likewise
  carried state                                 prev and x_last bit for bit, the two y_last within F

The fused modes are compared with the oracle run on the GPU's OWN source values (each source stage is checked on its own
against numpy; test_stage_api_equals_fused_demodulator in test_gpu_parity.py is the proof that the fused passes see the
same values).  Every output buffer lies between guard words that must come back untouched.

The matrix is not a full product.  Left out, by name: the segment layouts for iqa_deemphasis / iqa_dc_block (they take
none); input class (d) outside the AGC and (e) outside the DC blocker (the classes are defined for those); the sizes above
2 M run once per operation (class (a), the config-5 layout -- the config-2 block of 5 769 231 with it too); alignment offsets
and layouts rotate over the sizes instead of multiplying them (every value appears at least once per operation, asserted by
test_case_matrix_reaches_every_shape_class, which also names the shape classes of the engine and the cells that reach them).
"""
from __future__ import annotations

import importlib.util
import itertools
import sys
from ctypes import byref, c_double, c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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

SMALL = (1, 2, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 4097, 131_071, 131_073)
LARGE = (2_097_152, 2_097_153, 2_099_205, 5_769_231)  # per = 1 (every carry thread busy), 2 (half idle), 2, 3 (config 2)
MODES = (("nfm", False), ("am", False), ("usb", False), ("lsb", False), ("usb", True))
GUARD, SENTINEL = 64, 12345.0
POISON = 0x7F


@pytest.fixture(scope="module")
def G():
    import torch

    import iq_to_audio_amd as pkg

    pkg.native.lib()  # fail loudly if the HIP library is missing
    pkg.native.require_gpu()

    class Ns:
        pass

    g = Ns()
    g.torch, g.N, g.lib, g.dev = torch, pkg.native, pkg.native.lib(), torch.device("cuda", torch.cuda.current_device())
    return g


# ---- device buffers at chosen offsets ------------------------------------------------------------------------


def dev_in(G, arr: np.ndarray, off: int = 0):
    """``arr`` on the device, starting ``off`` elements into an allocation of its own (a tensor slice)."""
    t = G.torch
    arr = np.ascontiguousarray(arr)
    base = t.zeros(arr.size + off + 4, dtype=getattr(t, arr.dtype.name), device=G.dev)
    assert base.data_ptr() % 16 == 0
    view = base[off:off + arr.size]
    if arr.size:
        view.copy_(t.from_numpy(arr))
    assert (view.data_ptr() % 16 == 0) == ((off * arr.dtype.itemsize) % 16 == 0)
    return view


class Out:
    """A float32 output of n elements at float offset ``off`` between guard words."""

    def __init__(self, G, n: int, off: int = 0):
        self.G, self.n = G, n
        self.full = G.torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=G.torch.float32, device=G.dev)
        assert self.full.data_ptr() % 16 == 0
        self.lo = GUARD + off
        self.view = self.full[self.lo:self.lo + n]

    def numpy(self) -> np.ndarray:
        full = self.full.cpu().numpy()
        assert np.all(full[:self.lo] == SENTINEL) and np.all(full[self.lo + self.n:] == SENTINEL), "write outside the output"
        return full[self.lo:self.lo + self.n].copy()


def workspace(G, n: int):
    return G.torch.empty(int(G.lib.iqa_scan_workspace_bytes(n)) + 16, dtype=G.torch.uint8, device=G.dev)


def dev_bytes(G, img: np.ndarray):
    return G.torch.from_numpy(np.ascontiguousarray(img).view(np.uint8).copy()).to(G.dev)


# ---- the entry points ------------------------------------------------------------------------------------------


def gpu_source(G, mode: str, z_dev, prev: np.complex64 = np.complex64(1 + 0j)) -> np.ndarray:
    N, n = G.N, int(z_dev.numel())
    out = Out(G, n)
    if M.SOURCE[mode] == "quad":
        prev_dev = dev_bytes(G, np.array([prev], dtype=np.complex64))
        N.call("iqa_quadrature", N.ptr(z_dev), c_int64(n), N.ptr(prev_dev), N.ptr(out.view), N.stream_ptr())
    elif M.SOURCE[mode] == "env":
        N.call("iqa_envelope", N.ptr(z_dev), c_int64(n), N.ptr(out.view), N.stream_ptr())
    else:
        N.call("iqa_real_part", N.ptr(z_dev), c_int64(n), N.ptr(out.view), N.stream_ptr())
    return out.numpy()


def gpu_stage(G, op: str, x: np.ndarray, *, state=(), resets=None, x_off=0, y_off=0, alpha=None):
    """iqa_deemphasis / iqa_dc_block / iqa_agc on float input ``x``: (unclipped output, state after as float64[]).
    ``alpha``: the de-emphasis pole, M.ALPHA where none is given."""
    alpha = M.ALPHA if alpha is None else alpha
    N, n = G.N, int(x.size)
    x_dev, out, work = dev_in(G, x.astype(np.float32), x_off), Out(G, n, y_off), workspace(G, n)
    st = dev_bytes(G, np.array(state, dtype=np.float64)) if len(state) else None
    if op == "deemph":
        N.call("iqa_deemphasis", N.ptr(x_dev), c_int64(n), c_double(alpha), N.ptr(st), N.ptr(out.view), N.ptr(work), N.stream_ptr())
    elif op == "dc":
        N.call("iqa_dc_block", N.ptr(x_dev), c_int64(n), c_double(M.DC_RADIUS), N.ptr(st), N.ptr(out.view), N.ptr(work), N.stream_ptr())
    else:
        r_dev = dev_bytes(G, np.asarray(resets, dtype=np.int64)) if resets is not None else None  # None: NULL, n_resets = 0
        N.call("iqa_agc", N.ptr(x_dev), c_int64(n), c_double(M.AGC_TARGET), c_double(M.AGC_DECAY), N.ptr(r_dev),
               c_int64(0 if resets is None else len(resets)), N.ptr(out.view), N.ptr(work), N.stream_ptr())
    y = out.numpy()
    return y, (st.cpu().numpy().view(np.float64) if st is not None else None)


class Fused:
    pass


def gpu_demod(G, mode, agc, z_dev, segs, *, state_img=None, fresh=False, y_off=0, s_off=0, peak0=0.0, alpha=None):
    """iqa_demodulate (``state_img``: the 32-byte state block going in) or iqa_demodulate_from_reset (``fresh``: state,
    peak and sums go in filled with 0x7F bytes).  Returns audio, state image, peak, sums[n_segs, 8], scratch.
    ``alpha``: the de-emphasis pole, M.ALPHA where none is given."""
    N, t, n = G.N, G.torch, int(z_dev.numel())
    segs = np.asarray(segs, dtype=np.int64)
    p = N.DemodParams(mode=N.DEMOD_MODE[mode], agc_enabled=int(agc), deemph_alpha=M.ALPHA if alpha is None else alpha,
                      dc_radius=M.DC_RADIUS, agc_target=M.AGC_TARGET, agc_decay=M.AGC_DECAY)
    if fresh:
        state = t.full((32,), POISON, dtype=t.uint8, device=G.dev)
        peak = t.full((4,), POISON, dtype=t.uint8, device=G.dev).view(t.float32)
        sums = t.full((segs.size * M.SLOTS * 8,), POISON, dtype=t.uint8, device=G.dev).view(t.float64)
    else:
        state = dev_bytes(G, state_img)
        peak = t.full((1,), float(peak0), dtype=t.float32, device=G.dev)
        sums = t.zeros(segs.size * M.SLOTS, dtype=t.float64, device=G.dev)
    out, work, segs_dev = Out(G, n, y_off), workspace(G, n), dev_bytes(G, segs)
    scratch = Out(G, n, s_off) if (agc and mode in ("usb", "lsb")) else None
    N.call("iqa_demodulate_from_reset" if fresh else "iqa_demodulate", byref(p), N.ptr(z_dev), c_int64(n), N.ptr(state),
           N.ptr(segs_dev), c_int64(segs.size), N.ptr(peak), N.ptr(sums), N.ptr(out.view),
           N.ptr(scratch.view) if scratch is not None else c_void_p(0), N.ptr(work), N.stream_ptr())
    r = Fused()
    r.audio, r.state = out.numpy(), state.cpu().numpy()
    r.peak, r.sums = np.float32(peak.cpu().numpy()[0]), sums.cpu().numpy().reshape(segs.size, M.SLOTS)
    r.scratch = scratch.numpy() if scratch is not None else None
    return r


def gpu_writer_clip(G, a_dev, segs, *, out="new", peak0=0.0, with_peak=True, out_off=0, peak_word=None):
    """iqa_writer_clip; ``out``: "new" (a buffer of its own), "inplace" (out == in) or None (statistics only).
    ``peak_word``: a peak word that an earlier call has written (the running peak), instead of a new one holding ``peak0``."""
    N, t, n = G.N, G.torch, int(a_dev.numel())
    segs = np.asarray(segs, dtype=np.int64)
    peak = peak_word if peak_word is not None else t.full((1,), float(peak0), dtype=t.float32, device=G.dev) if with_peak else None
    sums = t.zeros(segs.size * M.SLOTS, dtype=t.float64, device=G.dev)
    segs_dev = dev_bytes(G, segs)
    o = Out(G, n, out_off) if out == "new" else None
    out_ptr = N.ptr(o.view) if out == "new" else N.ptr(a_dev) if out == "inplace" else c_void_p(0)
    N.call("iqa_writer_clip", N.ptr(a_dev), c_int64(n), N.ptr(peak), N.ptr(segs_dev), c_int64(segs.size), N.ptr(sums), out_ptr,
           N.stream_ptr())
    audio = o.numpy() if out == "new" else a_dev.cpu().numpy() if out == "inplace" else None
    return audio, (np.float32(peak.cpu().numpy()[0]) if with_peak else None), sums.cpu().numpy().reshape(segs.size, M.SLOTS)


# ---- the comparisons (each prints its figure before it asserts) ------------------------------------------------------


def check_samples(label, got, want64, rel, floor):
    """|got - want| <= rel * 2^-24 * |want| + floor for EVERY sample."""
    got64 = got.astype(np.float64)
    assert got.dtype == np.float32 and got.shape == want64.shape and np.isfinite(got64).all(), label
    err = np.abs(got64 - want64)
    tol = rel * M.EPS32 * np.abs(want64) + floor
    k = int(np.argmax(err - tol)) if err.size else 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    print(f"[scan-exact] {label}: n={got.size} max err/tol={ratio.max() if err.size else 0:.3f} max err={err.max() if err.size else 0:.3e}")
    assert np.all(err <= tol), (label, "sample", k, "got", float(got64[k]), "want", float(want64[k]), "err", float(err[k]), "tol", float(tol[k]),
                                "tile", k // M.TILE, "in tile", k % M.TILE, "bad", int((err > tol).sum()))


def check_block(label, got, blk, clipped=False):
    want = np.clip(blk.y64, -float(M.CLIP), float(M.CLIP)) if clipped else blk.y64
    check_samples(label, got, want, blk.extra.get("rel", 1.0), blk.extra.get("floor", blk.F))


def check_sink(label, got_peak, got_slots, v_gpu, blk, segs):
    """peak: == max |v| of the GPU's own unclipped output, within 2^-23 of the oracle's; sums: slot by slot of a segment
    against the oracle's float64 sum (2^-21 relative, 0 exactly where the oracle's is 0), and the total."""
    want = M.sink(blk.v, segs)
    if got_peak is not None:
        own = np.float32(np.max(np.abs(v_gpu)))
        print(f"[scan-exact] {label}: peak {got_peak!r} own {own!r} oracle {want.peak!r}")
        assert got_peak == own, (label, got_peak, own)
        assert abs(float(got_peak) - float(want.peak)) <= 2.0 ** -23 * float(want.peak), (label, got_peak, want.peak)
    got = got_slots.sum(axis=1)
    assert np.isfinite(got_slots).all() and got.shape == want.sums.shape, label
    zero = want.sums == 0.0
    rel = np.abs(got - want.sums)[~zero] / want.sums[~zero]
    tot = abs(got.sum() - want.sums.sum()) / want.sums.sum() if want.sums.sum() > 0 else abs(got.sum())
    print(f"[scan-exact] {label}: {len(segs)} segments ({int(zero.sum())} zero) max rel sum err {rel.max() if rel.size else 0:.3e} total {tot:.3e}")
    assert np.all(got_slots[zero] == 0.0), (label, "a segment whose sum is 0 received something", np.flatnonzero(zero & (got != 0))[:5])
    bad = np.flatnonzero(~zero)[rel > 2.0 ** -21]
    assert bad.size == 0, (label, "segment", bad[:5], "got", got[bad[:5]], "want", want.sums[bad[:5]], "starts", np.asarray(segs)[bad[:5]])
    assert tot <= 2.0 ** -21, (label, "total", got.sum(), want.sums.sum())


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def check_source(label, mode, got, z, prev=np.complex64(1 + 0j)):
    want = M.source(mode, z, prev)
    kind = M.SOURCE[mode]
    if kind == "real":
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), label  # exact, the sign of zero included
    elif kind == "env":
        d = ulp_distance(got, want)
        print(f"[scan-exact] {label}: envelope max ulp {int(d.max())}, {int((d > 0).sum())} of {d.size} differ")
        assert d.max() <= 1, (label, int(d.max()))
    else:
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        wrap = M.near_pi(want)
        err[wrap] = np.minimum(err[wrap], np.abs(err[wrap] - 2 * np.pi))
        print(f"[scan-exact] {label}: discriminator max err {err.max():.3e}, {int(wrap.sum())} of {want.size} compared modulo 2 pi")
        assert wrap.sum() * 10_000 < want.size, (label, int(wrap.sum()))
        assert err.max() <= 1e-6, (label, int(np.argmax(err)), float(err.max()))


# ---- the case matrix ------------------------------------------------------------------------------------------------

STAGE_CLASSES = {"deemph": ("a", "b", "c", "f"), "dc": ("a", "b", "c", "e", "f"), "agc": ("a", "b", "c", "d", "f")}
MODE_CLASSES = {"nfm": ("a", "b", "c", "f"), "am": ("a", "b", "c", "e", "f"), "usb": ("a", "b", "c", "f"), "lsb": ("a", "b", "c", "f")}


def _rotating(n_list, classes, layouts, offsets, large=True):
    """One cell per size, the other axes rotating; then every class, every layout and every offset once more at sizes
    that reach several tiles (131 073: 65 tiles, the last one a single sample; 4097)."""
    cells, seen = [], set()

    def add(n, cls, lay, off):
        lay = lay if (n > 1 or lay != "last") else "single"
        if (n, cls, lay, off) not in seen:
            seen.add((n, cls, lay, off))
            cells.append((n, cls, lay, off))

    cyc_c, cyc_l, cyc_o = itertools.cycle(classes), itertools.cycle(layouts), itertools.cycle(offsets)
    for n in n_list:
        add(n, next(cyc_c), next(cyc_l), next(cyc_o))
    for cls in classes:
        add(131_073, cls, "c5", offsets[0])
        add(4097, cls, "stair", offsets[-1])
    for lay in layouts:
        add(131_073, "a", lay, offsets[1 % len(offsets)])
    for off in offsets:
        add(131_071, "b", "tile-1", off)
        add(2049, "a", "tile+1", off)
    for n in LARGE if large else ():
        add(n, "a", "c5", offsets[0])
    return cells


def _id(*parts):
    return "-".join("".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in parts)


# (x offset, y offset): float input at 0 / 1, output at 0 .. 3
STAGE_OFFSETS = ((0, 0), (1, 1), (0, 2), (1, 3), (0, 1), (1, 0))
STAGE_CELLS = [(op,) + c for op in ("deemph", "dc", "agc")
               for c in _rotating(SMALL, STAGE_CLASSES[op], M.LAYOUTS if op == "agc" else ("single",), STAGE_OFFSETS)]
# (z offset, y offset, scratch offset): z at complex-sample offsets 0 / 1, output at 0 .. 3, the SSB-with-AGC scratch at 0 / 1
FUSED_OFFSETS = ((0, 0, 0), (1, 1, 1), (0, 2, 1), (1, 3, 0), (0, 1, 0), (1, 0, 1), (0, 3, 0), (1, 2, 0))
# iqa_demodulate ("state": from a used state block) in every mode over the whole matrix; iqa_demodulate_from_reset ("fresh")
# likewise for nfm and for usb with AGC, and for the other modes without the sizes above 2 M and with three of the small sizes
FRESH_FULL = (("nfm", False), ("usb", True))
FUSED_CELLS = [(mode, agc, "state") + c for (mode, agc) in MODES for c in _rotating(SMALL, MODE_CLASSES[mode], M.LAYOUTS, FUSED_OFFSETS)]
FUSED_CELLS += [(mode, agc, "fresh") + c for (mode, agc) in MODES
                for c in (_rotating(SMALL, MODE_CLASSES[mode], M.LAYOUTS, FUSED_OFFSETS) if (mode, agc) in FRESH_FULL
                          else _rotating((1, 9, 2049), MODE_CLASSES[mode], M.LAYOUTS, FUSED_OFFSETS, large=False))]
CLIP_CELLS = [c for c in _rotating(SMALL, ("a", "b", "c", "f"), M.LAYOUTS, ((0, 0), (1, 1), (0, 2), (1, 3)))]

USED_STATE = M.State(np.complex64(-0.3 + 0.2j), 0.37, 0.125, -0.4)  # a decoder that has seen something


# (the 2 M size runs classes (a) and (c) only)
SOURCE_CELLS = [(mode, cls, n, z_off) for mode in ("nfm", "am", "usb") for cls in M.CLASSES_Z
                for n, z_off in ((1, 0), (2, 1), (9, 0), (513, 1), (2049, 0), (131_073, 1), (2_099_205, 0)) if n < 2_000_000 or cls in "ac"]


@pytest.mark.parametrize("mode,cls,n,z_off", SOURCE_CELLS, ids=[_id(*c) for c in SOURCE_CELLS])
def test_source_stage_against_numpy(G, mode, cls, n, z_off):
    z = M.make_z(cls, n)
    prev = np.complex64(0.5 - 0.25j)
    check_source(_id(mode, cls, n, z_off), mode, gpu_source(G, mode, dev_in(G, z, z_off), prev), z, prev)


@pytest.mark.parametrize("op,n,cls,lay,offs", STAGE_CELLS, ids=[_id(*c) for c in STAGE_CELLS])
def test_stage_entry_point_per_sample(G, op, n, cls, lay, offs):
    """iqa_deemphasis, iqa_dc_block and iqa_agc from a float input with an incoming state: every sample, the state after."""
    x = M.make_x(op, cls, n)
    x_off, y_off = offs
    if op == "deemph":
        y, st = gpu_stage(G, op, x, state=[0.37], x_off=x_off, y_off=y_off)
        blk = M.stage_deemphasis(x, M.ALPHA, 0.37)
        assert abs(st[0] - blk.y64[-1]) <= blk.F, (st, blk.y64[-1])
    elif op == "dc":
        y, st = gpu_stage(G, op, x, state=[0.125, -0.4], x_off=x_off, y_off=y_off)
        blk = M.stage_dc(x, M.DC_RADIUS, 0.125, -0.4)
        assert st[0] == float(x[-1]) and abs(st[1] - blk.y64[-1]) <= blk.F, (st, x[-1], blk.y64[-1])
    else:
        resets = M.layout(lay, n)
        y, _ = gpu_stage(G, op, x, resets=resets, x_off=x_off, y_off=y_off)
        blk = M.stage_agc(x, resets)
        held = blk.extra["held"]
        print(f"[scan-exact] agc {n} {lay} {cls}: {int(held.sum())} held, {int(held[M.restart_bounds(n, resets)[:-1]].sum())} restarts on a held sample, S={blk.S:.4g}")
    check_block(_id(op, n, cls, lay, offs), y, blk)


@pytest.mark.parametrize("n", [1, 9, 2049, 131_073])
def test_agc_without_restart_list(G, n):
    """n_resets = 0 with a NULL pointer: only element 0 restarts."""
    x = M.make_x("agc", "d", n)
    y, _ = gpu_stage(G, "agc", x, resets=None)
    check_block(f"agc-null-{n}", y, M.stage_agc(x, None))


def _fused_oracle(G, mode, agc, z, z_dev, st, segs, got, img_in=None, alpha=None):
    """The oracle of one fused call from the GPU's own source values; checks the audio (and the scratch of SSB with AGC).
    Returns (the source values, the block whose values reach the sink, the stage entry points' unclipped output, the state
    after, the linear filter's floor term).  The stage entry points start from the state block the fused call read
    (``img_in``; the oracle's own where none is given): in a stream the GPU's y_last may differ from the oracle's by up to F,
    and the bit-for-bit comparisons with the stages' output (the peak, the scratch) must not hang on that.
    ``alpha``: the de-emphasis pole the fused call ran with, M.ALPHA where none is given."""
    alpha = M.ALPHA if alpha is None else alpha
    u = gpu_source(G, mode, z_dev, st.prev)
    lin = M.demod_block(mode, u, st, alpha)
    after = M.advance(mode, st, z, u, lin)
    de_y, dc_x, dc_y = (st.de_y, st.dc_x, st.dc_y) if img_in is None else img_in[8:].view(np.float64)
    if mode == "nfm":
        v_gpu, _ = gpu_stage(G, "deemph", u, state=[de_y], alpha=alpha)
    else:
        v_gpu, _ = gpu_stage(G, "dc", u, state=[dc_x, dc_y])
    if not (agc and mode in ("usb", "lsb")):
        return u, lin, v_gpu, after, lin.F
    check_block("scratch (DC blocker in front of the AGC)", got.scratch, lin)
    assert np.array_equal(got.scratch.view(np.uint32), v_gpu.view(np.uint32))
    blk = M.stage_agc(got.scratch, segs)  # the AGC's oracle on the values the AGC read
    v_gpu, _ = gpu_stage(G, "agc", got.scratch, resets=segs)
    return u, blk, v_gpu, after, lin.F


def check_state(label, mode, got_img, after, F, before_img):
    """``before_img``: the 32 bytes that went in -- the used state, or 0x7F bytes for iqa_demodulate_from_reset.  Either entry
    point writes the 16 bytes its mode owns (prev and the de-emphasis state for nfm, the DC blocker's for the others: "receives
    the outgoing state as usual", iqa_hotpath.h) and nothing else: under the fresh form the owned half is fully overwritten and
    the other half is still poison, byte for byte."""
    prev = got_img[:8].view(np.complex64)[0]
    de_y, dc_x, dc_y = got_img[8:].view(np.float64)
    if mode == "nfm":
        assert np.array_equal(got_img[:8], np.array([after.prev], dtype=np.complex64).view(np.uint8)), (label, prev, after.prev)
        print(f"[scan-exact] {label}: y_last err {abs(de_y - after.de_y):.3e} (F {F:.3e})")
        assert abs(de_y - after.de_y) <= F, (label, de_y, after.de_y)
        owned = slice(0, 16)
    else:
        assert np.float64(dc_x).tobytes() == np.float64(after.dc_x).tobytes(), (label, dc_x, after.dc_x)
        print(f"[scan-exact] {label}: y_last err {abs(dc_y - after.dc_y):.3e} (F {F:.3e})")
        assert abs(dc_y - after.dc_y) <= F, (label, dc_y, after.dc_y)
        owned = slice(16, 32)
    keep = np.ones(32, dtype=bool)
    keep[owned] = False
    assert np.array_equal(got_img[keep], before_img[keep]), (label, "a field the mode does not own was written")


@pytest.mark.parametrize("mode,agc,entry,n,cls,lay,offs", FUSED_CELLS, ids=[_id(*c) for c in FUSED_CELLS])
def test_fused_mode_per_sample(G, mode, agc, entry, n, cls, lay, offs):
    """iqa_demodulate from a used state and iqa_demodulate_from_reset over poisoned state, peak and sums: every audio sample,
    the state after, the peak and the per-segment sums slot by slot."""
    z = M.make_z(cls, n)
    segs = M.layout(lay, n)
    z_off, y_off, s_off = offs
    z_dev = dev_in(G, z, z_off)
    fresh = entry == "fresh"
    st = M.State() if fresh else USED_STATE
    got = gpu_demod(G, mode, agc, z_dev, segs, state_img=st.image(), fresh=fresh, y_off=y_off, s_off=s_off)
    label = _id(mode, "agc" if agc else "plain", entry, n, cls, lay, offs)
    u, blk, v_gpu, after, lin_F = _fused_oracle(G, mode, agc, z, z_dev, st, segs, got)
    check_source(label, mode, u, z, st.prev)
    check_block(label, got.audio, blk, clipped=True)
    assert np.array_equal(got.audio.view(np.uint32), np.clip(v_gpu, -M.CLIP, M.CLIP).view(np.uint32)), (label, "fused != stages")
    check_state(label, mode, got.state, after, lin_F, np.full(32, POISON, np.uint8) if fresh else st.image())
    check_sink(label, got.peak, got.sums, v_gpu, blk, segs)
    if cls == "f" and n >= 2047:  # class (f) drives every mode past the clip within a tile: the peak is pre-clip, the audio is not
        assert np.max(np.abs(blk.v)) > M.CLIP, label
        assert got.peak > M.CLIP and np.abs(got.audio).max() == M.CLIP, label


@pytest.mark.parametrize("n,cls,lay,offs", CLIP_CELLS, ids=[_id(*c) for c in CLIP_CELLS])
def test_writer_clip_per_sample(G, n, cls, lay, offs):
    """iqa_writer_clip on its own: out of place, in place, statistics only (out = NULL) and peak = NULL."""
    a = M.make_x("clip", cls, n)
    segs = M.layout(lay, n)
    in_off, out_off = offs
    want = M.sink(a, segs)
    blk = M.Block(a.astype(np.float64), a, 0.0, 0.0)
    label = _id("clip", n, cls, lay, offs)
    for form in ("new", "inplace", None):
        for with_peak in (True, False):
            if form == "inplace":  # the buffer that is read and written lies between guard words too
                both = Out(G, n, in_off)
                both.view.copy_(G.torch.from_numpy(a))
                a_dev = both.view
            else:
                a_dev = dev_in(G, a, in_off)
            audio, peak, slots = gpu_writer_clip(G, a_dev, segs, out=form, with_peak=with_peak, out_off=out_off)
            if form == "inplace":
                audio = both.numpy()
            if audio is not None:
                assert np.array_equal(audio.view(np.uint32), want.audio.view(np.uint32)), (label, form)
            else:
                assert np.array_equal(a_dev.cpu().numpy().view(np.uint32), a.view(np.uint32))
            check_sink(f"{label}-{form}-{with_peak}", peak, slots, a, blk, segs)
    # a running peak: a word that starts below, between or above holds the larger value, whichever side brought it
    for peak0 in (0.0, 0.5 * float(want.peak), 2.0 * float(want.peak) + 1.0):
        _, peak, _ = gpu_writer_clip(G, dev_in(G, a, in_off), segs, out=None, peak0=peak0)
        assert peak == max(np.float32(peak0), want.peak), (label, peak0, peak, want.peak)
    # ... and carried over two calls on ONE peak word: a block and its half-scale and double-scale copies, in both orders
    for first, second in ((1.0, 0.5), (0.5, 1.0), (1.0, 2.0)):
        word = G.torch.zeros(1, dtype=G.torch.float32, device=G.dev)
        for scale in (first, second):
            _, peak, _ = gpu_writer_clip(G, dev_in(G, a * np.float32(scale), in_off), segs, out=None, peak_word=word)
        assert peak == np.float32(max(first, second)) * want.peak, (label, first, second, peak, want.peak)


@pytest.mark.parametrize("mode,agc", MODES)
@pytest.mark.parametrize("first", ["state", "fresh"])
def test_streaming_blocks_meet_the_oracle(G, mode, agc, first):
    """One stream of 300 001 samples cut into blocks of 1, 1, 2047, 2049, 8, 100 003 and the rest through ONE state block
    (the first block as iqa_demodulate on the pristine image or as iqa_demodulate_from_reset over poison): every block
    meets the oracle run over the same cuts, and the state block after every call is the oracle's."""
    n = 300_001
    z = M.make_z("a", n)
    st = M.State()
    img = st.image()
    for k, (lo, hi) in enumerate(M.stream_blocks(n)):
        zb = z[lo:hi]
        segs = M.layout("prod", hi - lo)  # the AGC restarts at every block start and at the chunk starts inside it
        z_dev = dev_in(G, zb, k & 1)
        fresh = (k == 0 and first == "fresh")
        got = gpu_demod(G, mode, agc, z_dev, segs, state_img=img, fresh=fresh, y_off=k % 4, s_off=k & 1)
        label = _id("stream", mode, "agc" if agc else "plain", first, "block", k, hi - lo)
        u, blk, v_gpu, after, lin_F = _fused_oracle(G, mode, agc, zb, z_dev, st, segs, got, None if fresh else img)
        check_source(label, mode, u, zb, st.prev)
        check_block(label, got.audio, blk, clipped=True)
        assert np.array_equal(got.audio.view(np.uint32), np.clip(v_gpu, -M.CLIP, M.CLIP).view(np.uint32)), (label, "fused != stages")
        check_state(label, mode, got.state, after, lin_F, np.full(32, POISON, np.uint8) if fresh else img)
        check_sink(label, got.peak, got.sums, v_gpu, blk, segs)
        if k == 0 and fresh:  # and the two forms of the first block agree bit for bit
            ref = gpu_demod(G, mode, agc, z_dev, segs, state_img=M.State().image())
            assert np.array_equal(ref.audio.view(np.uint32), got.audio.view(np.uint32)) and ref.peak == got.peak
            owned = slice(0, 16) if mode == "nfm" else slice(16, 32)
            assert np.array_equal(ref.state[owned], got.state[owned])
        # the GPU goes on from ITS state block; the oracle from its own (they agree within F, asserted above)
        img, st = got.state.copy(), after
        if fresh:  # the fields this mode does not own are still poison: give the next call the oracle's image of them
            fixed = after.image()
            owned = slice(0, 16) if mode == "nfm" else slice(16, 32)
            fixed[owned] = got.state[owned]
            img = fixed


# ---- iqa_mean_power, iqa_raw_level ----------------------------------------------------------------------------------

def power_z(n: int, seed: int) -> np.ndarray:
    """Seeded complex64 white noise whose level changes along the array (a stretch read at the wrong place shows).  The
    kernels form |z| as numpy does, statement for statement (csrc/common.h: np_abs_c64), so the bound below is about the
    summation, the range and the count -- and a magnitude formed any other way (hypotf: up to 2 ulps away) misses it."""
    rng = np.random.default_rng(seed)
    z = rng.normal(size=n) + 1j * rng.normal(size=n)
    return (z * (0.05 + 0.2 * np.arange(n) / max(n, 1))).astype(np.complex64)


def _mean_power_want(mag32: np.ndarray) -> float:
    return float(np.mean((mag32 * mag32).astype(np.float64))) if mag32.size else 0.0


@pytest.mark.parametrize("count,skip", [(65_536, 0), (65_536, 1000), (65_537, 0), (65_537, 3), (3_000_001, 0), (3_000_001, 12_345),
                                        (1, 0), (0, 77_000)])
def test_mean_power_against_float64_mean(G, count, skip):
    """mean of float32(|z|)^2 over z[skip:n] within 1e-12 relative: the one-block path (count <= 65 536), the atomic path
    above it, skip > 0, and skip == n, which writes 0 over whatever was there."""
    N, t, n = G.N, G.torch, count + skip
    z = power_z(n, 4001 + count)
    z_dev = dev_in(G, z, 1)
    out = t.full((1,), 777.0, dtype=t.float64, device=G.dev)
    N.call("iqa_mean_power", N.ptr(z_dev), c_int64(n), c_int64(skip), N.ptr(out), N.stream_ptr())
    got = float(out.cpu().numpy()[0])
    mag = np.abs(z)
    assert mag.dtype == np.float32
    want = _mean_power_want(mag[skip:])
    print(f"[scan-exact] mean_power count={count} skip={skip}: got {got!r} want {want!r}")
    assert (got == 0.0) if count == 0 else abs(got - want) <= 1e-12 * want, (got, want)


@pytest.mark.parametrize("n_each,skip", [(70_000, 0), (70_000, 5), (1_000_003, 11), (4096, 96)])
def test_mean_power_batch_long_and_short_stretches(G, n_each, skip):
    N, t, parts = G.N, G.torch, 3
    z = power_z(n_each * parts, 4100 + n_each)
    z[n_each:2 * n_each] *= np.float32(0.5)  # a stretch read at the wrong offset shows
    z_dev = dev_in(G, z, 1)
    out = t.full((parts,), 777.0, dtype=t.float64, device=G.dev)
    N.call("iqa_mean_power_batch", N.ptr(z_dev), c_int64(n_each), c_int32(parts), c_int64(skip), N.ptr(out), N.stream_ptr())
    got = out.cpu().numpy()
    want = np.array([_mean_power_want(np.abs(z[p * n_each + skip:(p + 1) * n_each])) for p in range(parts)])
    print(f"[scan-exact] mean_power_batch {n_each} {skip}: {got} {want}")
    assert np.all(np.abs(got - want) <= 1e-12 * want), (got, want)


RAW, _raw_level_want = M.RAW_LEVEL_FORMATS, M.raw_level_want  # (shared with tests/test_gpu_runner_buffers.py)


def _raw_values(fmt: str, n_values: int, seed: int) -> np.ndarray:
    """The level rises along the array, so a stretch taken from the wrong place shows.  int16 values reach full scale, both
    ends of the range planted: the mean square of integers is exact in float64 far below the bound, and the kernel's has to
    be too (float32 squares would round by 2^-24 each up there)."""
    rng = np.random.default_rng(seed)
    ramp = 0.25 + 0.75 * np.arange(n_values) / max(n_values, 1)
    if fmt == "s16":
        v = np.rint(ramp * rng.integers(-32768, 32768, size=n_values)).astype(np.int16)
        v[1::97] = -32768
        v[2::89] = 32767
        return v
    if fmt == "u8":
        return (128 + np.rint(ramp * rng.integers(-128, 128, size=n_values))).astype(np.uint8)
    return (ramp * rng.normal(size=n_values)).astype(np.float32)


@pytest.mark.parametrize("fmt", ["s16", "u8", "f32"])
@pytest.mark.parametrize("n_vec,extra", [(0, 0), (0, 3), (1, 0), (1023, 1), (1024, 0), (8191, 3), (8192, 0), (8193, 2), (1_000_003, 1)])
def test_raw_level_against_the_documented_stretches(G, fmt, n_vec, extra):
    """iqa_raw_level feeds the precision guard of the fixed-point channelizers: the mean square over exactly the eight
    documented stretches, for value counts that are not a multiple of the vector width too (the tail is not read)."""
    N, t = G.N, G.torch
    code, per_vec, _ = RAW[fmt]
    raw = _raw_values(fmt, n_vec * per_vec + extra, 5000 + n_vec)
    raw_dev = dev_in(G, raw, 0) if raw.size else None
    out = t.full((1,), 777.0, dtype=t.float64, device=G.dev)
    N.call("iqa_raw_level", c_int32(code), N.ptr(raw_dev), c_int64(raw.size), N.ptr(out), N.stream_ptr())
    got, want = float(out.cpu().numpy()[0]), _raw_level_want(fmt, raw)
    print(f"[scan-exact] raw_level {fmt} n_vec={n_vec}+{extra}: got {got!r} want {want!r}")
    assert (got == 0.0) if want == 0.0 else abs(got - want) <= 1e-12 * want, (got, want)


@pytest.mark.parametrize("fmt", ["s16", "u8", "f32"])
def test_raw_level_refuses_an_unaligned_pointer(G, fmt):
    N, t = G.N, G.torch
    code, per_vec, _ = RAW[fmt]
    raw_dev = dev_in(G, _raw_values(fmt, 4096 * per_vec, 1), 1)
    out = t.full((1,), 777.0, dtype=t.float64, device=G.dev)
    with pytest.raises(ValueError, match="16-byte aligned"):
        N.call("iqa_raw_level", c_int32(code), N.ptr(raw_dev), c_int64(raw_dev.numel()), N.ptr(out), N.stream_ptr())
    G.torch.cuda.synchronize()
    assert float(out.cpu().numpy()[0]) == 777.0  # nothing was launched


# ---- the shape classes of the engine and the cells that reach them ---------------------------------------------------


def _boundaries_per_tile(n, segs):
    """Chunk starts in (first, last] of each tile: the sink compares the chunk of a tile's first sample with that of its last,
    so a start exactly on a tile's first sample is no boundary of that tile (the tile is `uniform`)."""
    tiles = (n + M.TILE - 1) // M.TILE
    inner = np.asarray(segs)[1:]
    inner = inner[inner % M.TILE != 0]
    return np.bincount(inner // M.TILE, minlength=tiles) if inner.size else np.zeros(max(tiles, 1), int)


def test_case_matrix_reaches_every_shape_class():
    """Names each shape class of the scan engine and asserts that the matrices above hold a cell that reaches it (the
    predicates restate the kernels' own conditions), and that every value of the issue's axes appears per operation."""
    fused = [c for c in FUSED_CELLS]
    z_cells = [(n, offs[0], offs[1], M.layout(lay, n), cls, mode, agc, entry) for (mode, agc, entry, n, cls, lay, offs) in fused]
    reach = {
        # load_u: `z_aligned && wave_base + 512 <= n` -- whole-wave vector loads
        "vector load path": any(zo == 0 and n >= 512 for n, zo, *_ in z_cells),
        # ... else the scalar loads: an unaligned z, or the last, partly filled wave of an aligned one
        "scalar load path (unaligned z)": any(zo == 1 and n >= 512 for n, zo, *_ in z_cells),
        "scalar load path (last wave of an aligned z)": any(zo == 0 and n % 512 for n, zo, *_ in z_cells),
        # lane 0 of a vector-path wave fetches z[base-2 .. base-1] by hand; the discriminator and the DC blocker read them
        "lane-0 hand fetch": any(zo == 0 and n >= 1024 and mode in ("nfm", "am") for n, zo, _, _, _, mode, *_ in z_cells),
        # k_fused_apply: `y_aligned && base + 8 <= n`
        "vector store": any(yo == 0 and n >= 8 for n, _, yo, *_ in z_cells),
        "scalar store (unaligned y)": all(any(yo == k and n >= 8 for n, _, yo, *_ in z_cells) for k in (1, 2, 3)),
        "scalar store (last thread of an aligned y)": any(yo == 0 and n % 8 for n, _, yo, *_ in z_cells),
        # k_fused_carry: per = ceil(tiles / 1024)
        "per = 1, every carry thread busy": any(n == 2_097_152 for n, *_ in z_cells),
        "per = 2, half the carry threads idle": any(n == 2_097_153 for n, *_ in z_cells),
        "per = 2, a partly filled last run": any(n == 2_099_205 for n, *_ in z_cells),
        "per = 3": any(M.per_thread_tiles(n) == 3 for n, *_ in z_cells),
        # the sink's statistics paths
        "uniform": any((_boundaries_per_tile(n, s) == 0).any() for n, _, _, s, *_ in z_cells),
        "simple": any((_boundaries_per_tile(n, s) == 1).any() for n, _, _, s, *_ in z_cells),
        "general": any((_boundaries_per_tile(n, s) >= 2).any() for n, _, _, s, *_ in z_cells),
        "n_segs > 256": any(len(s) > 256 for _, _, _, s, *_ in z_cells),
        # AGC restarts next to a tile edge, and on held samples
        "restart at a tile's first sample": any(agc and (s[1:] % M.TILE == 0).any() for _, _, _, s, _, _, agc, _ in z_cells),
        "restart at a tile's last sample": any(agc and (s[1:] % M.TILE == M.TILE - 1).any() for _, _, _, s, _, _, agc, _ in z_cells),
        "AGC hold": any(agc and cls == "c" for _, _, _, _, cls, _, agc, _ in z_cells) and any(c[0] == "agc" and c[2] == "d" for c in STAGE_CELLS),
        "fresh": all(any(e == "fresh" and (m, a) == ma for *_, m, a, e in z_cells) for ma in MODES),
    }
    missing = [k for k, ok in reach.items() if not ok]
    assert not missing, missing
    # every value of every axis, per operation
    for op in ("deemph", "dc", "agc"):
        cells = [c for c in STAGE_CELLS if c[0] == op]
        assert {c[1] for c in cells} >= set(SMALL) | set(LARGE), op
        assert {c[2] for c in cells} == set(STAGE_CLASSES[op]), op
        assert {c[4][0] for c in cells} == {0, 1} and {c[4][1] for c in cells} == {0, 1, 2, 3}, op
    assert {c[3] for c in STAGE_CELLS if c[0] == "agc"} == set(M.LAYOUTS)
    for (mode, agc) in MODES:
        cells = [c for c in FUSED_CELLS if (c[0], c[1]) == (mode, agc)]
        assert {c[3] for c in cells if c[2] == "state"} >= set(SMALL) | set(LARGE), mode
        assert {c[3] for c in cells if c[2] == "fresh"} >= {1, 9, 2049, 131_073}, mode
        assert {c[4] for c in cells} == set(MODE_CLASSES[mode]) and {c[5] for c in cells} == set(M.LAYOUTS), mode
        assert {c[6][0] for c in cells} == {0, 1} and {c[6][1] for c in cells} == {0, 1, 2, 3} and {c[6][2] for c in cells} == {0, 1}, mode
    assert {c[3] for c in FUSED_CELLS if c[2] == "fresh" and c[0] == "nfm"} >= set(LARGE)  # iqa_demodulate_from_reset above 2 M
    assert {c[0] for c in CLIP_CELLS} >= set(SMALL) | set(LARGE) and {c[2] for c in CLIP_CELLS} == set(M.LAYOUTS)
    assert {c[3][0] for c in CLIP_CELLS} == {0, 1} and {c[3][1] for c in CLIP_CELLS} == {0, 1, 2, 3}
