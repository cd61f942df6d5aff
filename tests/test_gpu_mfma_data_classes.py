"""The int8 matrix-core channelizer kernels on the data classes their other exact tests never feed them.

tests/test_gpu_mfma_exact.py and the modules built on it vary shape, phase and dispatch; their captures are uniform
full-range values throughout.  The kernels split an int16 value into a high byte and a biased low byte
(v = 256 hi + lo' + 128), so the values at which those bytes sit on an edge or never move are a class of their own: all
0 (hi 0, lo' -128), all -1 (hi -1, lo' +127), the two ends of the range, the values around every byte edge -- and the
worst-case coherent capture, in which every product of one output has the sign of its tap, so that the folded
accumulations (the 7-instruction half step, the LDS scatter adds, the 64-bit lanes) carry their largest sums of one sign.

Every case is ONE launch, held bit for bit to the exact integer model (oracle/mfma_model.py) with ``torch.equal``; the
rotated lane within the rotation's own bar, as everywhere.  Shapes are the smallest that reach each kernel form (the
stream-phase module's, N_OUT = 2 * 256 + 37), plus one launch of the per-lane kernel, one of a lane with 64-bit sums, one
of a "fine" plan (a high-byte-only lane and its residue lane) and the uint8 ring kernel.  Before the launch each case
asserts on the host that the input is legal, that the model's int32 form equals its 64-bit form for every lane with
int32 sums (nothing wraps), and the launch's documented read bounds.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import mfma_dispatch as X
from oracle import mfma_model as M
from test_gpu_mfma_exact import (Lane, _check_abi_selects, _N, _perlane_run, _rot, capture, check_lane, check_z, launch,
                                 make_plan, perlane_frames_needed, setup_capture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


OPB, N_OUT, M_FIRST = 256, 2 * 256 + 37, 64 + 1000
TARGETS = {0: M_FIRST + 150, 1: M_FIRST + 400}  # component -> the output the coherent captures are built for (windows apart)

SHAPES = {  # name -> (entry, format, D, the kernel the launch reaches; "plain": the per-lane kernel, no ring dispatch)
    "d8-half1": ("multi", "s16", 8, "k_channelize_mfma_s16_ring_multi_half<1>"),
    "d104-half7": ("multi", "s16", 104, "k_channelize_mfma_s16_ring_multi_half<7>"),
    "d100-half7": ("multi", "s16", 100, "k_channelize_mfma_s16_ring_multi_half<7>"),
    "d208-multi13": ("multi", "s16", 208, "k_channelize_mfma_s16_ring_multi<13>"),
    "d208-pairs13": ("pairs", "s16", 208, "k_channelize_mfma_s16_ring_pairs<13>"),
    "d104-plain": ("plain", "s16", 104, "k_channelize_mfma_s16"),
    "d104-full64": ("multi", "s16", 104, "k_channelize_mfma_s16_ring_multi64<7>"),
    "d104-fine": ("multi", "s16", 104, "k_channelize_mfma_s16_ring_multi<7, SKIPK>"),
    "d104-u8-rows": ("multi", "u8", 104, "k_channelize_mfma_u8_ring_rows_multi<7>"),
}
EDGE_CYCLE = [-257, -256, -255, -129, -128, -127, -1, 0, 1, 127, 128, 129, 255, 256]
S16_CLASSES = ["zeros", "minus-one", "min", "max", "byte-edges", "coherent", "coherent-negated", "coherent-64"]
U8_CLASSES = ["u8-0", "u8-127", "u8-128", "u8-255", "u8-coherent"]
CASES = [(s, c) for s, v in SHAPES.items() for c in (U8_CLASSES if v[1] == "u8" else S16_CLASSES)]


def _ks(d):
    return -(-2 * d // 32)


def _lanes(shape):
    """One plain lane; one rotated, conjugated and scaled by j.  "full64", "plain": 16-bit taps.  "fine": the two
    lanes of a residual plan (high-byte-only taps, the launch's skip variant, and their residue)."""
    _, fmt, d, _ = SHAPES[shape]
    step, base = _rot(np.random.default_rng(9000 + d))
    turn = dict(rotate=1, conj=1, scale=1j, rot_step=step, rot_base=base, fmt=fmt)
    if shape.endswith("fine"):
        mp = make_plan(64 * d - d // 3 - 1, d, fmt, True, residual=True, seed=d + 1)
        assert mp.groups[0].high_only and not mp.groups[1].high_only
        return [Lane(mp, 0, fmt=fmt), Lane(mp, 1, **turn)]
    acc32 = not shape.endswith(("full64", "plain"))
    return [Lane(make_plan(64 * d - d // 3 - 1, d, fmt, acc32, seed=d + 2), 0, fmt=fmt),
            Lane(make_plan(64 * d - d // 3 - 6, d, fmt, acc32, seed=d + 102), 0, **turn)]


def _coherent(tq, d, consumed, n_frames, pos, neg, rest):
    """Every value a tap of ``TARGETS``' outputs meets is ``pos`` or ``neg`` by the sign of that tap (tap row qq of the
    output m meets data row m - qq: frames (m - qq) D + 1 ..), ``rest`` where the tap is 0 and everywhere else."""
    v = np.full(2 * n_frames, rest, dtype=np.int64)
    for comp, m in TARGETS.items():
        for qq in range(1, 65):
            first = 2 * ((m - qq) * d + 1 - consumed)
            row = np.asarray(tq[comp * 64 + qq - 1, : 2 * d])
            v[first : first + 2 * d] = np.where(row > 0, pos, np.where(row < 0, neg, rest))
    return v


def _data(cls, tq, d, consumed):
    """The ``data=`` callable of a class (see ``test_gpu_mfma_exact.capture``)."""
    const = {"zeros": 0, "minus-one": -1, "min": -32768, "max": 32767, "u8-0": 0, "u8-127": 127, "u8-128": 128, "u8-255": 255}
    if cls in const:
        return lambda fmt, n: np.full(2 * n, const[cls], dtype=np.int64)
    if cls == "byte-edges":
        return lambda fmt, n: np.resize(np.array(EDGE_CYCLE, dtype=np.int64), 2 * n)
    pos, neg, rest = {"coherent": (32767, -32768, 0), "coherent-negated": (-32768, 32767, 0), "coherent-64": (64, -64, 0),
                      "u8-coherent": (255, 0, 128)}[cls]
    return lambda fmt, n: _coherent(tq, d, consumed, n, pos, neg, rest)


def _assert_no_wrap(lanes, raw, fmt, d, consumed, cls):
    """The model's int32 form of every lane with int32 sums equals its 64-bit form; on the full-scale coherent captures the
    chosen output of lane 0 carries the launch's largest sum of its component."""
    for i, ln in enumerate(lanes):
        grp = ln.mp.groups[ln.gi]
        s1, s2 = M.pass_sums(grp.tq, raw, fmt, d, grp.q, 0, _ks(d), consumed, M_FIRST, N_OUT)
        v64 = M.ring_value(s1, s2, False)
        if fmt == "u8" or ln.mp._acc32:
            assert np.array_equal(M.ring_value(s1, s2, True), v64), (cls, i)
        if i == 0 and cls in ("coherent", "coherent-negated", "u8-coherent"):
            for comp, m in TARGETS.items():
                assert int(np.argmax(np.abs(v64[:, comp]))) == m - M_FIRST, (cls, comp)


@pytest.mark.parametrize("shape,cls", CASES, ids=[f"{s}-{c}" for s, c in CASES])
def test_kernel_equals_model_on_the_data_class(A, shape, cls):
    """One launch of the shape's kernel on the class's capture (a mid-capture block that holds exactly what the launch may
    read, random values behind it): every lane equals the exact model -- bit for bit, the rotated lane within the
    rotation bar."""
    from iq_to_audio_amd import _dev as D

    entry, fmt, d, kernel = SHAPES[shape]
    ks = _ks(d)
    lanes = _lanes(shape)
    tq = lanes[0].mp.groups[lanes[0].gi].tq
    consumed = (M_FIRST - 64) * d + 1 - 3  # a mid-capture block: 3 frames in front of the first row
    if entry == "plain":
        N = _N()
        mp = lanes[0].mp  # (one group, one pass, 16-bit taps: the per-lane kernel's separate S1 / S2 sums)
        assert len(mp.passes) == 1 and mp.groups[0].q == 0
        n_frames = perlane_frames_needed(d, 0, ks, 0, M_FIRST, N_OUT, OPB, consumed)
        raw = capture(fmt, n_frames + 4096, seed=d)
        raw[: 2 * n_frames] = capture(fmt, n_frames, 0, data=_data(cls, tq, d, consumed))
        x = D.to_device(raw, "int16")
        raw = raw[: 2 * n_frames]
        _assert_no_wrap(lanes[:1], raw, fmt, d, consumed, cls)
        prm = N.ChanParams(fmt=0, ntaps=64 * d - d // 3 - 1, decimation=d, conj_sum=0, rotate=0, reserved=0, rot_step=0, rot_base=0,
                           out_scale_re=1.0, out_scale_im=0.0)
        z = _perlane_run(mp, x, n_frames, consumed, M_FIRST, N_OUT, OPB, prm)  # (asserts its read bounds before the call)
        want = M.finish(M.plan_sums(mp, raw, fmt, d, consumed, M_FIRST, N_OUT, False), M_FIRST, 0, 0)
        check_z(z, want, 0, f"{shape} {cls}")
        return
    acc64 = shape.endswith("full64")
    assert X.expected_kernel(entry, fmt, d, 0, ks, acc64, shape.endswith("fine")) == kernel
    _check_abi_selects(A, entry, fmt, d, 0, ks, acc64, kernel)
    mode = X.ring_mode(fmt, d, 0, ks, acc64)
    assert mode == (2 if fmt == "u8" else 1)
    raw, x, n_frames, consumed = setup_capture(fmt, d, mode, 0, ks, 0, 0, M_FIRST, N_OUT, OPB, seed=d, consumed=consumed,
                                               data=_data(cls, tq, d, consumed))  # (asserts the read bounds)
    _assert_no_wrap(lanes, raw, fmt, d, consumed, cls)
    launch(entry, fmt, d, 0, ks, OPB, lanes, x, n_frames, consumed, M_FIRST, N_OUT)
    for i, ln in enumerate(lanes):
        check_lane(ln, 0, raw, d, consumed, M_FIRST, N_OUT, f"{shape} {cls} lane {i}")
