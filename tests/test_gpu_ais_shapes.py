"""The AIS kernels (csrc/ais.hip) against the numpy oracle of tests/ais_model.py at their edge shapes, on the MI355X:
``iqa_ais_filter`` at windows 1, 2, 8, 9, 16, 17, 298, 299 (outside the plan's 3L - 1; W = 1 has no tap group at all) with
arbitrary taps in 0 .. 256 and with all taps 256 on theta held at +-pi (every sum +-12 868 . 256 . W, the int32 bound the
kernel promises), n = 7, 8, 9, 2056, 4101, every pointer a view at its own element offset 0 .. 3 (so the 16-byte store and
the element-wise store of full runs are both taken on purpose), with and without history; ``iqa_ais_symbols`` at 0, 1, 255,
256, 257 symbols, on steps whose instants tie at .5, and on a plane shorter than W - 1; ``iqa_ais_frames`` with a different
plane and count per phase (0, 23, 24, 25, nsym), a candidate at s = 24, a closing flag that ends on count - 1 and on count,
and the same planes under v -> a v + b with every symbol positive and the largest next to 2^31 - 1; and every refusal of the
three entry points.  Integers throughout: no tolerance.  The case tables, the oracle's own branch facts and the comparisons
are in tests/ais_model.py; tests/test_ais_shapes_host.py runs the same comparisons without a GPU."""
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


M = _load("ais_model")


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


def _filter(theta, th_at, n, hist, h_at, W, taps, t_alloc, t_at, s_alloc, s_at):
    from iq_to_audio_amd import _native as N

    th, h, tp, t, s = (_up(x) for x in (theta, hist, taps, t_alloc, s_alloc))
    assert s[s_at:].data_ptr() % 16 == 4 * (s_at % 4)
    N.call("iqa_ais_filter", N.ptr(th[th_at:]), c_int64(n), N.ptr(None if h is None else h[h_at:]), c_int32(W), N.ptr(tp), N.ptr(t[t_at:]),
           N.ptr(s[s_at:]), N.stream_ptr())
    return t.cpu().numpy(), s.cpu().numpy()


def _symbols(S, n, W, step, nsym, v_buf):
    from iq_to_audio_amd import _native as N

    s, v = _up(S), _up(v_buf)
    N.call("iqa_ais_symbols", N.ptr(s), c_int64(n), c_int32(W), c_double(step), c_int64(nsym), N.ptr(v), N.stream_ptr())
    return v.cpu().numpy()


def _frames(planes, nsym, count_of, W, step, capacity, lst, slots, counts):
    from iq_to_audio_amd import _native as N

    dev = [_up(x) for x in (planes, lst, slots, counts)]
    N.call("iqa_ais_frames", N.ptr(dev[0]), c_int64(nsym), (c_int64 * 8)(*count_of), c_int32(W), c_double(step), N.ptr(dev[1]), N.ptr(dev[2]),
           c_int64(capacity), N.ptr(dev[3]), N.stream_ptr())
    return tuple(x.cpu().numpy() for x in dev[1:])


# ---- a. iqa_ais_filter ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("W", list(M.FILTER_WINDOWS))
def test_filter_at_any_window_and_alignment(A, W):
    """S and t are the model's in every case of the table, and the sentinels in front of and behind both views stay."""
    cases = M.filter_cases(W)
    assert {c["offsets"][3] for c in cases} == {0, 1, 2, 3} and sum(1 for c in cases if c["full"]) == 6
    for case in cases:
        M.check_filter(case, _filter)


def test_filter_without_the_t_output(A):
    """t_out NULL at an unaligned s_out: S alone, as the model gives it."""
    from iq_to_audio_amd import _native as N

    case = next(c for c in M.filter_cases(17) if c["n"] == M.TILE + 8 and c["hist"] is not None and c["offsets"][3] == 3)
    want = M.pulse_filter(M.quantise(case["theta"]), dict(W=17, taps=case["taps"].astype(np.int64)), case["hist"])
    th, h, tp = _up(case["theta"]), _up(case["hist"]), _up(case["taps"])
    s = _up(np.full(M.FRONT + 3 + case["n"] + M.GUARD, M.SENT, dtype=np.int32))
    N.call("iqa_ais_filter", N.ptr(th), c_int64(case["n"]), N.ptr(h), c_int32(17), N.ptr(tp), N.ptr(None), N.ptr(s[M.FRONT + 3 :]), N.stream_ptr())
    got = s.cpu().numpy()
    np.testing.assert_array_equal(got[M.FRONT + 3 : M.FRONT + 3 + case["n"]], want)
    assert (got[: M.FRONT + 3] == M.SENT).all() and (got[M.FRONT + 3 + case["n"] :] == M.SENT).all()


# ---- b. iqa_ais_symbols ---------------------------------------------------------------------------------------------------


def test_symbols_at_the_block_edge_and_on_ties(A):
    """The planes are the model's at 0, 1, 255, 256 and 257 symbols per phase; an instant beyond the plane reads zero; the
    steps 1.25 and 0.75 put instants on exact .5 ties, half of which round down."""
    stats: dict = {}
    for case in M.symbol_cases():
        M.check_symbols(case, _symbols, stats)
    print(stats)
    assert stats["ties"] > 1000 and 0 < stats["ties rounded down"] < stats["ties"]


# ---- c. iqa_ais_frames ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mapped", [False, True], ids=["as made", "a v + b"])
@pytest.mark.parametrize("nsym", list(M.FRAME_NSYM))
def test_frames_with_a_plane_and_a_count_per_phase(A, nsym, mapped):
    """Counters, list rows, slots and slot padding are the oracle walker's; under the affine map they are the unmapped
    planes'."""
    for sc in M.frame_scenarios(nsym):
        M.check_frames(sc, _frames, mapped=mapped)


# ---- d. refusals ----------------------------------------------------------------------------------------------------------


def _sentinels(k, size=4096):
    return [_up(np.full(size, M.SENT, dtype=np.int64)) for _ in range(k)]


def _untouched(bufs) -> bool:
    from iq_to_audio_amd import _dev as D

    D.torch_mod().cuda.synchronize()
    return all((b.cpu().numpy() == M.SENT).all() for b in bufs)


def test_filter_refuses_before_it_launches(A):
    from iq_to_audio_amd import _native as N

    for what, n, W, has_theta, has_taps, has_s, message in M.filter_refusals():
        bufs = _sentinels(5)
        theta, hist, taps, t, s = bufs
        with pytest.raises(ValueError, match=message):
            N.call("iqa_ais_filter", N.ptr(theta if has_theta else None), c_int64(n), N.ptr(hist), c_int32(W), N.ptr(taps if has_taps else None),
                   N.ptr(t), N.ptr(s if has_s else None), N.stream_ptr())
        assert _untouched(bufs), what


def test_symbols_refuse_before_they_launch(A):
    from iq_to_audio_amd import _native as N

    for what, n, W, step, nsym, has_s, has_v, message in M.symbol_refusals():
        bufs = _sentinels(2)
        s, v = bufs
        with pytest.raises(ValueError, match=message):
            N.call("iqa_ais_symbols", N.ptr(s if has_s else None), c_int64(n), c_int32(W), c_double(step), c_int64(nsym), N.ptr(v if has_v else None),
                   N.stream_ptr())
        assert _untouched(bufs), what


def test_frames_refuse_before_they_launch(A):
    """Also the counters: a refused call clears nothing."""
    from iq_to_audio_amd import _native as N

    for what, nsym, count_of, W, step, capacity, has_v, has_list, has_slots, has_counts, message in M.frame_refusals():
        bufs = _sentinels(4)
        v, lst, slots, counts = bufs
        table = None if count_of is None else (c_int64 * 8)(*count_of)
        with pytest.raises(ValueError, match=message):
            N.call("iqa_ais_frames", N.ptr(v if has_v else None), c_int64(nsym), table, c_int32(W), c_double(step), N.ptr(lst if has_list else None),
                   N.ptr(slots if has_slots else None), c_int64(capacity), N.ptr(counts if has_counts else None), N.stream_ptr())
        assert _untouched(bufs), what
