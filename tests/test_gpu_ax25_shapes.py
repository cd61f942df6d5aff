"""The AFSK kernels (csrc/afsk.hip) against the numpy oracle of tests/ax25_model.py at their edge shapes, on the MI355X: the
channel rates at the short end (L = 8, one tap group) and with sampling instants on half-even ties, ``iqa_afsk_correlate``
called directly at every tap-group remainder and tile-edge length on random and full-scale theta, with and without a
history, with either energy output absent and with the slicer plane off its 8-byte alignment, and ``iqa_afsk_bits`` on
random planes that end on and one before a sampling instant.  Integers throughout: no tolerance.  The oracle's own branch
facts are asserted before every comparison; tests/test_ax25_shapes_host.py holds them without a GPU."""
from __future__ import annotations

import importlib.util
import sys
from ctypes import c_double, c_int32, c_int64, c_void_p
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


M = _load("ax25_model")

SENT32, SENT64, SENT8 = -7_777_777, -7_777_777_777, 0xAA  # what untouched output words hold
GUARD = 16  # sentinel words behind (and, for the slicer plane, in front of) every output


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


# ---- a. rates through Ax25Decoder ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("fs", M.EDGE_RATES)
def test_rate_classes(A, fs):
    """One UI frame in two blocks at L = 8, at sps 10.5 (L = 10, step 21/16), at L = 81 and L = 84 (step 10.5): t is the
    oracle's quantiser of the GPU's own theta; from that t every stage and the parsed frame are the oracle's."""
    from iq_to_audio_amd.decoders.ax25 import Ax25Decoder

    pl = M.plan(fs)
    z = M.edge_stream(fs)
    ties = M.tie_instants(pl, z.size)
    assert bool(ties) == (fs in M.TIE_RATES)
    dec = Ax25Decoder(fs)
    assert (dec.plan.L, dec.plan.step, dec.core.hist_len) == (pl["L"], pl["step"], pl["L"] - 1)
    dec.process(z[:5001])
    dec.process(z[5001:])
    st = dec.stages()
    assert st["t"].dtype == np.int32 and st["t"].size == z.size
    np.testing.assert_array_equal(st["t"], M.quantise(st["theta"]))
    want = M.oracle(fs=fs, t=st["t"])
    assert len(want["records"]) >= 8 and len(want["frames"]) == 1 and want["rejected"] == 0
    for f in (1200, 2200):
        assert st["E"][f].dtype == np.int64
        np.testing.assert_array_equal(st["E"][f], want["E"][f], err_msg=f"E {f}")
    np.testing.assert_array_equal(st["sign"], want["sign"])
    assert len(st["bits"]) == len(want["bits"]) == 24
    for v in range(24):
        np.testing.assert_array_equal(st["bits"][v], want["bits"][v], err_msg=f"bits of variant {v}")
    assert st["records"] == want["records"] and st["candidates"] == want["closed"]
    res = dec.finish()
    assert [(f.source, f.dest, f.path, f.control, f.pid, f.info, f.raw, f.hits, f.time_s) for f in res.frames] == [
        (f["source"], f["dest"], f["path"], f["control"], f["pid"], f["info"], f["raw"], f["hits"], f["time_s"]) for f in want["frames"]]
    assert [f.raw for f in res.frames] == [M.ui_frame(*M.EDGE_FRAME).hex()]
    assert (res.candidates, res.crc_ok, res.rejected) == (want["closed"], len(want["records"]), 0)


# ---- b. iqa_afsk_correlate on crafted theta -----------------------------------------------------------------------------


def _correlate(theta_dev, n, hist_dev, L, taps_dev, energy_out, sign_offset):
    """-> (t[n + GUARD], E_1200 or None, E_2200 or None, the whole slicer allocation uint8[GUARD + n + GUARD]); the slicer
    plane handed to the kernel starts ``sign_offset`` bytes behind an 8-byte aligned address."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    t = D.from_numpy(np.full(n + GUARD, SENT32, dtype=np.int32))
    e = [D.from_numpy(np.full(n + GUARD, SENT64, dtype=np.int64)) if want else None for want in energy_out]
    sign = D.from_numpy(np.full(GUARD + n + GUARD, SENT8, dtype=np.uint8))
    assert sign.data_ptr() % 8 == 0 and GUARD % 8 == 0
    N.call("iqa_afsk_correlate", N.ptr(theta_dev), c_int64(n), N.ptr(hist_dev), c_int32(L), N.ptr(taps_dev), N.ptr(t),
           c_void_p(sign.data_ptr() + GUARD + sign_offset), N.ptr(e[0]), N.ptr(e[1]), N.stream_ptr())
    return t.cpu().numpy(), *[None if x is None else x.cpu().numpy() for x in e], sign.cpu().numpy()


@pytest.mark.parametrize("L", M.EDGE_WINDOWS)
def test_correlate_on_crafted_theta(A, L):
    """One tap group (L = 8), every remainder of the tap padding (9, 15, 16, 17, 393, 399, 400), lengths below one group and
    around the tile edges, random theta with two stretches of a full-scale square wave at the mark and the space tone, a NULL
    and a full-scale history, energy outputs both given, both NULL and one of each, and the slicer plane at byte offsets
    0 (packed 8-byte stores), 1 and 4 (byte stores): t, E and the slicer byte are the oracle's, nothing else is written."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import dsp_plan as P

    fs = 1200.0 * L
    pl = M.plan(fs)
    assert pl["L"] == L
    taps = D.from_numpy(np.ascontiguousarray(P.plan_afsk(fs).taps))
    hist = M.crafted_history(L, seed=L)
    hist_dev = D.from_numpy(hist)
    full = M.crafted_theta(L, max(M.EDGE_LENGTHS), seed=L)
    full_dev = D.from_numpy(full)
    launches = 0
    for n in M.EDGE_LENGTHS:
        theta = full[:n]
        for h, h_dev in ((None, None), (hist, hist_dev)):
            want_t, want_e, want_sign, sums = M.correlate_block(theta, h, pl)
            peak = max(int(np.abs(x).max()) for iq in sums.values() for x in iq)
            if L == 400 and n >= 2047:
                assert peak > M.T_PI * 256 * L // 2  # more than half of the bound the int32 sums are promised
            if n >= 2047:
                assert set(np.unique(want_sign).tolist()) == {0, 4, 5, 7}  # all four slicer decisions occur
            for energy_out in ((True, True), (False, False), (True, False), (False, True)):
                for offset in (0, 1, 4):
                    t, e1, e2, sign = _correlate(full_dev, n, h_dev, L, taps, energy_out, offset)
                    launches += 1
                    tag = f"n {n}, hist {'NULL' if h is None else 'given'}, energies {energy_out}, slicer offset {offset}"
                    np.testing.assert_array_equal(t[:n], want_t, err_msg=tag)
                    assert (t[n:] == SENT32).all(), tag
                    for got, f in ((e1, 1200), (e2, 2200)):
                        if got is not None:
                            np.testing.assert_array_equal(got[:n], want_e[f], err_msg=f"E {f}, {tag}")
                            assert (got[n:] == SENT64).all(), tag
                    lo = GUARD + offset
                    np.testing.assert_array_equal(sign[lo : lo + n], want_sign, err_msg=tag)
                    assert (sign[:lo] == SENT8).all() and (sign[lo + n :] == SENT8).all(), tag
    assert launches == len(M.EDGE_LENGTHS) * 2 * 4 * 3


def test_correlate_rejects_windows_outside_its_range(A):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import dsp_plan as P

    taps = D.from_numpy(np.ascontiguousarray(P.plan_afsk(9_600.0).taps))
    theta = D.from_numpy(M.crafted_theta(8, 64, seed=0))
    for L in (7, 401):
        with pytest.raises(ValueError, match="window"):
            _correlate(theta, 64, None, L, taps, (True, True), 0)


# ---- c. iqa_afsk_bits on a random slicer plane ---------------------------------------------------------------------------


@pytest.mark.parametrize("fs", M.EDGE_RATES + (480_000.0,))
def test_bits_on_a_plane_that_ends_on_an_instant(A, fs):
    """A random plane of bytes 0 .. 7 whose last sample is the instant of bit 37 at phase 3, and the same plane one sample
    shorter: all 24 rows are the oracle's bit streams, a bit whose instant is >= n is 0, with ``nbits`` the largest per-phase
    count and that count + 3."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    pl = M.plan(fs)
    plane, n_full = M.bits_case(pl)
    for n in (n_full, n_full - 1):
        counts = [M.instants(pl, p, n).size for p in range(M.PHASES)]
        assert counts[3] == (38 if n == n_full else 37) and max(counts) == 38
        if n == n_full:
            assert int(M.instants(pl, 3, n)[-1]) == n - 1
        sign = D.from_numpy(plane[:n].copy())
        for nbits in (max(counts), max(counts) + 3):
            want = M.bits_plane(plane[:n], pl, nbits)
            for v in range(24):
                assert (want[v, counts[v % 8] :] == 0).all()
            assert 0 < int(want.sum()) < want.size
            out = D.from_numpy(np.full(24 * nbits + GUARD, SENT8, dtype=np.uint8))
            N.call("iqa_afsk_bits", N.ptr(sign), c_int64(n), c_int32(pl["L"]), c_double(pl["step"]), c_int64(nbits), N.ptr(out),
                   N.stream_ptr())
            got = out.cpu().numpy()
            assert (got[24 * nbits :] == SENT8).all()
            np.testing.assert_array_equal(got[: 24 * nbits].reshape(24, nbits), want, err_msg=f"n {n}, nbits {nbits}")


# ---- d. iqa_afsk_frames refuses before it clears ------------------------------------------------------------------------


def test_frames_refuse_before_they_clear_the_counters(A):
    """A call refused for a NULL bit plane, list or slot pointer leaves the counters, and every other buffer, as they were."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    for missing in ("bits", "list", "slots"):
        bufs = dict(bits=D.from_numpy(np.full(4096, SENT8, dtype=np.uint8)), list=D.from_numpy(np.full(64, SENT64, dtype=np.int64)),
                    slots=D.from_numpy(np.full(4096, SENT8, dtype=np.uint8)), counts=D.from_numpy(np.array([SENT64, SENT64, SENT64], dtype=np.int64)))
        arg = {k: None if k == missing else v for k, v in bufs.items()}
        with pytest.raises(ValueError, match="NULL device pointer"):
            N.call("iqa_afsk_frames", N.ptr(arg["bits"]), c_int64(8), (c_int64 * 8)(*[8] * 8), c_int32(40), c_double(5.0), N.ptr(arg["list"]), N.ptr(arg["slots"]),
                   c_int64(4), N.ptr(arg["counts"]), N.stream_ptr())
        D.torch_mod().cuda.synchronize()
        assert all((v.cpu().numpy() == (SENT8 if v.dtype == D.torch_mod().uint8 else SENT64)).all() for v in bufs.values()), missing
