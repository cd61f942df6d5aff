"""The ADS-B kernels (csrc/adsb.hip) against the numpy oracle of tests/adsb_model.py at their edge shapes, on the MI355X:
``iqa_adsb_search`` with offset tables that are no plan's (h = 1 with o[k] = 10 k and span = 2400, the LDS size the
static_assert is written for; slack behind o[239] + h; h = 3; equal neighbouring offsets at a data pair and at the preamble
pair), the strictness of the seven inequalities and of the six 6 C_j < P rules at h = 2 and 10 on chip sums that tie where no
sample does, and at full scale (P = 2 621 400); more than 256 passing positions in one tile, so that pass 2 goes round twice;
``is_long ? reg : reg56`` from both sides and every dropped format; flags_out NULL and capacity 0 with NULL list and slots;
``q`` and ``flags`` as views at their own offsets; ``iqa_adsb_quantise`` at n = 0, 1, 255, 256, 257, 2049 on views at odd
element offsets; and every refusal of the two entry points.  Integers throughout: no tolerance.  The case tables, the
oracle's own branch facts and the comparisons are in tests/adsb_model.py; tests/test_adsb_shapes_host.py runs the same
comparisons without a GPU."""
from __future__ import annotations

import importlib.util
import sys
from ctypes import POINTER, c_int32, c_int64
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


M = _load("adsb_model")


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
    dev = D.from_numpy(arr.view(np.int16) if arr.dtype == np.uint16 else arr)
    assert dev.data_ptr() % 16 == 0  # the view offsets below are offsets from a 16-byte boundary
    return dev


def _search(q_alloc, q_at, n, o_alloc, o_host, h, span, flags, f_at, lst, slots, capacity, counts):
    from iq_to_audio_amd import _native as N

    q, o, f, l, s, c = (_up(x) for x in (q_alloc, o_alloc, flags, lst, slots, counts))
    beside = [_up(np.full(M.GUARD, M.SENT, dtype=np.int64)) for _ in range(2)]  # allocated next to the counters
    N.call("iqa_adsb_search", N.ptr(q[q_at:]), c_int64(n), N.ptr(o), o_host.ctypes.data_as(POINTER(c_int32)), c_int32(h), c_int32(span),
           N.ptr(None if f is None else f[f_at:]), N.ptr(l), N.ptr(s), c_int64(capacity), N.ptr(c), N.stream_ptr())
    out = tuple(None if x is None else x.cpu().numpy() for x in (f, l, s, c))
    assert all((b.cpu().numpy() == M.SENT).all() for b in beside)
    return out


def _quantise(e_alloc, e_at, n, q_alloc, q_at):
    from iq_to_audio_amd import _native as N

    e, q = _up(e_alloc), _up(q_alloc)
    N.call("iqa_adsb_quantise", N.ptr(e[e_at:]), c_int64(n), N.ptr(q[q_at:]), N.stream_ptr())
    return q.cpu().numpy().view(np.uint16)


def _run(cases):
    assert cases
    for case in cases:
        M.check_search(case, _search)


CASES = M.search_cases()


# ---- a. iqa_adsb_search ---------------------------------------------------------------------------------------------------


def test_search_with_tables_that_are_no_plans(A):
    """o[k] = 10 k with span 2400; slack behind o[239] + h (position count and flags length follow span); h = 3; equal
    offsets at a data pair (the bit reads 0) and at the preamble pair (no position passes)."""
    _run([c for c in CASES if "table" in c["name"] or "equal offsets" in c["name"]])


@pytest.mark.parametrize("h", [2, 10])
def test_strictness_on_sums_that_tie_where_no_sample_does(A, h):
    """Each of the seven strict inequalities and of the six 6 C_j < P rules: a tie of sums fails, one less passes; at h = 10
    also at full scale, where the kept record's P is 2 621 400."""
    _run([c for c in CASES if c["name"].startswith(f"h {h}")])


def test_more_than_256_passing_positions_in_a_tile(A):
    """The period-7 plane over three tiles, alone and with frames laid over it in the last positions of tile 0 and across
    the tile edge: pass 2 goes round twice.  The list's order is arrival order; which round a frame lands in is not asserted."""
    _run([c for c in CASES if c["tile0"]])


def test_the_register_choice_and_the_format_filter(A):
    """A DF17 whose first 56 bits are a codeword while the 112 are not, a DF11 whose 56 bits fail while the 112 would pass,
    valid frames of DF 0, 4, 5, 16, 20, 21 and 24: dropped.  DF 11, 17 and 18: kept."""
    _run([c for c in CASES if "DF" in c["name"] and not c["tile0"]])


def test_optional_outputs(A):
    """flags_out NULL and capacity 0 with NULL list and slots on a plane with three frames: the counters are the oracle's and
    the buffers allocated beside them stay."""
    _run([c for c in CASES if "three frames" in c["name"]])


def test_every_case_is_run(A):
    names = [c["name"] for c in CASES]
    picked = [n for n in names if "table" in n or "equal offsets" in n or n.startswith(("h 2", "h 10")) or "period 7" in n or "DF" in n or "three frames" in n]
    assert sorted(picked) == sorted(names) and len(set(names)) == len(names)


# ---- b. iqa_adsb_quantise -------------------------------------------------------------------------------------------------


def test_quantise_at_the_block_edge_on_odd_views(A):
    """n = 0, 1, 255, 256, 257, 2049 with e and q_out at odd element offsets and sentinels on both sides; NaN, inf, -0, -1,
    -inf and k + 1/2 over even and odd k."""
    for case in M.quantise_cases():
        M.check_quantise(case, _quantise)


# ---- c. refusals ----------------------------------------------------------------------------------------------------------


def _sentinels(k, size=4096):
    return [_up(np.full(size, M.SENT, dtype=np.int64)) for _ in range(k)]


def _untouched(bufs) -> bool:
    from iq_to_audio_amd import _dev as D

    D.torch_mod().cuda.synchronize()
    return all((b.cpu().numpy() == M.SENT).all() for b in bufs)


def test_search_refuses_before_it_launches(A):
    """Also the counters: a refused call clears nothing."""
    from iq_to_audio_amd import _native as N

    for what, n, o_host, h, span, capacity, has_q, has_o, has_list, has_slots, has_counts, message in M.search_refusals():
        bufs = _sentinels(5)
        q, flags, lst, slots, counts = bufs
        o = _up(np.arange(M.CHIPS + 16, dtype=np.int32))
        table = None if o_host is None else o_host.ctypes.data_as(POINTER(c_int32))
        with pytest.raises(ValueError, match=message):
            N.call("iqa_adsb_search", N.ptr(q if has_q else None), c_int64(n), N.ptr(o if has_o else None), table, c_int32(h), c_int32(span), N.ptr(flags),
                   N.ptr(lst if has_list else None), N.ptr(slots if has_slots else None), c_int64(capacity), N.ptr(counts if has_counts else None), N.stream_ptr())
        assert _untouched(bufs) and (o.cpu().numpy() == np.arange(M.CHIPS + 16)).all(), what


def test_quantise_refuses_before_it_launches(A):
    from iq_to_audio_amd import _native as N

    for what, n, has_e, has_q, message in M.quantise_refusals():
        bufs = _sentinels(2)
        e, q = bufs
        with pytest.raises(ValueError, match=message):
            N.call("iqa_adsb_quantise", N.ptr(e if has_e else None), c_int64(n), N.ptr(q if has_q else None), N.stream_ptr())
        assert _untouched(bufs), what
