"""The ACARS kernels (csrc/acars.hip) against the numpy oracle of tests/acars_model.py at their edge shapes, on the MI355X:
``iqa_acars_detect`` at (W, L) = (1, 8), (2, 8), (8, 9), (9, 15), (16, 16), (17, 400), (255, 8), (536, 8), (536, 400) (no
plan's pair; W = 1 has no tap group at all) with arbitrary taps in -256 .. 256, n = 7, 8, 9 and one workgroup's outputs - 1,
+ 0, + 1 and two of them + 3, five (cr, sr), every pointer a view at its own element offset (``same`` at every byte offset
0 .. 7, so the 8-byte store and the byte stores of whole runs are both taken on purpose), the optional outputs present and
NULL; with all 2 . 255 taps +256 and -256 on q = 2^15 everywhere (every settled sum +-2 139 095 040, the int32 bound, and the
largest |y| of the path); the quantiser on exact ties and at sh = 163, 140 and -113; ``iqa_acars_max`` on both sides of the
grid cap, on denormals and on the largest float; ``iqa_acars_bits`` at six (step, W) and 0, 1, 255, 256, 257 symbols on planes
that end on, before and behind the last instant; ``iqa_acars_frames`` with a different row and count per phase, a candidate
at s = 31 and at s = nb, capacity 0 with NULL list and slots; and every refusal of the four entry points.  Integers
throughout: no tolerance.  The case tables, the oracle's own branch facts and the comparisons are in tests/acars_model.py;
tests/test_acars_shapes_host.py runs the same comparisons without a GPU."""
from __future__ import annotations

import importlib.util
import sys
from ctypes import c_double, c_int32, c_int64
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


M = _load("acars_model")


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _up(arr):
    from iq_to_audio_amd import _dev as D

    if arr is None:
        return None
    dev = D.from_numpy(arr)
    assert dev.data_ptr() % 16 == 0  # the view offsets below are offsets from a 16-byte boundary
    return dev


def _detect(e_alloc, e_at, n, sh, W, L, taps_alloc, cr, sr, bufs, ats):
    from iq_to_audio_amd import _native as N

    e, taps = _up(e_alloc), _up(taps_alloc)
    dev = {k: _up(v) for k, v in bufs.items()}
    assert dev["same"][ats["same"] :].data_ptr() % 8 == ats["same"] % 8
    view = {k: dev[k][ats[k] :] if k in dev else None for k in ("q", "I", "Q", "y", "same")}
    N.call("iqa_acars_detect", N.ptr(e[e_at:]), c_int64(n), c_int32(sh), c_int32(W), c_int32(L), N.ptr(taps), c_int32(cr), c_int32(sr), N.ptr(view["q"]),
           N.ptr(view["I"]), N.ptr(view["Q"]), N.ptr(view["y"]), N.ptr(view["same"]), N.stream_ptr())
    return {k: v.cpu().numpy() for k, v in dev.items()}


def _max(e_alloc, e_at, n, out_alloc, out_at):
    from iq_to_audio_amd import _native as N

    e, out = _up(e_alloc), _up(out_alloc.view(np.int32))
    N.call("iqa_acars_max", N.ptr(e[e_at:]), c_int64(n), N.ptr(out[out_at:]), N.stream_ptr())
    return out.cpu().numpy().view(np.uint32)


def _bits(same, n, W, step, nbits, buf):
    from iq_to_audio_amd import _native as N

    s, out = _up(same), _up(buf)
    N.call("iqa_acars_bits", N.ptr(s), c_int64(n), c_int32(W), c_double(step), c_int64(nbits), N.ptr(out), N.stream_ptr())
    return out.cpu().numpy()


def _frames(planes, nbits, count_of, W, step, capacity, lst, slots, counts):
    from iq_to_audio_amd import _native as N

    dev = [_up(x) for x in (planes, lst, slots, counts)]
    N.call("iqa_acars_frames", N.ptr(dev[0]), c_int64(nbits), (c_int64 * 8)(*count_of), c_int32(W), c_double(step), N.ptr(dev[1]), N.ptr(dev[2]),
           c_int64(capacity), N.ptr(dev[3]), N.stream_ptr())
    return tuple(None if x is None else x.cpu().numpy() for x in dev[1:])


# ---- a. iqa_acars_detect --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("W,L", list(M.DETECT_SHAPES))
def test_detect_at_any_window_delay_and_alignment(A, W, L):
    """q, I, Q, y and same are the model's in every case of the table, and the sentinels in front of and behind every view
    stay; at W = 255 also the two full-scale sets."""
    cases = M.detect_cases(W, L)
    assert {c["offsets"]["same"] for c in cases} == set(range(8)) and sum(1 for c in cases if c["full"]) == 6 * (W == 255)
    assert any(c["outputs"] == "" and c["offsets"]["same"] == 3 for c in cases)
    for case in cases:
        M.check_detect(case, _detect)


def test_quantiser_on_ties_and_at_the_ends_of_the_shift_range(A):
    """e 2^sh on k + 1/2 for even and odd k, on 2^15 - 1/2 and either side; emax = 2^-149 (sh = 163), 2^-126 (sh = 140) and
    3.4028235e38 (sh = -113): q and everything behind it are the float64 oracle's."""
    for case in M.quantiser_cases():
        M.check_detect(case, _detect)


# ---- b. iqa_acars_max -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n", list(M.MAX_LENGTHS))
def test_max_on_both_sides_of_the_grid_cap(A, n):
    """The maximum alone at index 0 and at n - 1 (at n = 4 194 305 that element is the only one read in a 17th round), among
    denormals and as the largest float; the words around max_out stay."""
    cases = [c for c in M.max_cases() if c["n"] == n]
    assert len(cases) >= 2
    for case in cases:
        M.check_max(case, _max)


# ---- c. iqa_acars_bits ----------------------------------------------------------------------------------------------------


def test_bits_at_the_block_edge_and_on_ties(A):
    """The streams are the model's at 0, 1, 255, 256 and 257 symbols per phase; an instant beyond the plane reads zero; the
    steps 1.5 and 1.25 put instants on exact .5 ties, half of which round down."""
    stats: dict = {}
    for case in M.bit_cases():
        M.check_bits(case, _bits, stats)
    print(stats)
    assert all(stats[s]["ties"] > 1000 and stats[s]["down"] > 1000 for s in (1.5, 1.25))


# ---- d. iqa_acars_frames --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("capacity", [16, 1, 0])
def test_frames_with_a_row_and_a_count_per_phase(A, capacity):
    """Counters, list rows, slots and slot padding are the oracle walker's; capacity 0 passes NULL for the list and the
    slots and still counts."""
    for sc in M.frame_scenarios():
        M.check_frames(sc, _frames, capacity=capacity)


# ---- e. refusals ----------------------------------------------------------------------------------------------------------


def _sentinels(k, size=4096):
    return [_up(np.full(size, M.SENT, dtype=np.int64)) for _ in range(k)]


def _untouched(bufs) -> bool:
    from iq_to_audio_amd import _dev as D

    D.torch_mod().cuda.synchronize()
    return all((b.cpu().numpy() == M.SENT).all() for b in bufs)


def test_detect_refuses_before_it_launches(A):
    from iq_to_audio_amd import _native as N

    for what, n, sh, W, L, cr, sr, has_e, has_taps, has_same, message in M.detect_refusals():
        bufs = _sentinels(7)
        e, taps, q, i, qq, y, same = bufs
        with pytest.raises(ValueError, match=message):
            N.call("iqa_acars_detect", N.ptr(e if has_e else None), c_int64(n), c_int32(sh), c_int32(W), c_int32(L), N.ptr(taps if has_taps else None),
                   c_int32(cr), c_int32(sr), N.ptr(q), N.ptr(i), N.ptr(qq), N.ptr(y), N.ptr(same if has_same else None), N.stream_ptr())
        assert _untouched(bufs), what


def test_max_refuses_before_it_launches(A):
    """Also max_out: a refused call clears nothing."""
    from iq_to_audio_amd import _native as N

    for what, n, has_e, has_out, message in M.max_refusals():
        bufs = _sentinels(2)
        e, out = bufs
        with pytest.raises(ValueError, match=message):
            N.call("iqa_acars_max", N.ptr(e if has_e else None), c_int64(n), N.ptr(out if has_out else None), N.stream_ptr())
        assert _untouched(bufs), what


def test_bits_refuse_before_they_launch(A):
    from iq_to_audio_amd import _native as N

    for what, n, W, step, nbits, has_same, has_out, message in M.bit_refusals():
        bufs = _sentinels(2)
        same, out = bufs
        with pytest.raises(ValueError, match=message):
            N.call("iqa_acars_bits", N.ptr(same if has_same else None), c_int64(n), c_int32(W), c_double(step), c_int64(nbits),
                   N.ptr(out if has_out else None), N.stream_ptr())
        assert _untouched(bufs), what


def test_frames_refuse_before_they_launch(A):
    """Also the counters: a refused call clears nothing."""
    from iq_to_audio_amd import _native as N

    for what, nbits, count_of, W, step, capacity, has_bits, has_list, has_slots, has_counts, message in M.frame_refusals():
        bufs = _sentinels(4)
        bits, lst, slots, counts = bufs
        table = None if count_of is None else (c_int64 * 8)(*count_of)
        with pytest.raises(ValueError, match=message):
            N.call("iqa_acars_frames", N.ptr(bits if has_bits else None), c_int64(nbits), table, c_int32(W), c_double(step), N.ptr(lst if has_list else None),
                   N.ptr(slots if has_slots else None), c_int64(capacity), N.ptr(counts if has_counts else None), N.stream_ptr())
        assert _untouched(bufs), what
