"""The tone kernels (csrc/tones.hip) against the numpy oracle of tests/tones_model.py at their edge shapes, on the MI355X:
``iqa_tones_decimate`` called directly at R = 1, 2, 31, 32, 33, 63, 64 (tiles of 256 outputs, and of 8192 // R with MB R
below 8192), blocks of three tiles and a ragged rest, of one sample, ending on a tile's last and first sample, at positions
0, k R, off it and 2^40 + 3, with and without history, on random, full-scale and tie-valued theta; block invariance through
``ToneDecoder`` at R = 33 and 64 with cuts around the tile edge and inside the history; ``iqa_tones_bank`` at the frames of the
lowest and highest rate, of the longest frame and of both stream rates, on u whose I and Q are negative, beyond int32 and not
multiples of 4096; and every refusal of the three entry points.  Integers throughout: no tolerance.  The case tables, the
oracle's own branch facts and the comparisons are in tests/tones_model.py; tests/test_tones_shapes_host.py runs the same
comparisons without a GPU."""
from __future__ import annotations

import importlib.util
import sys
from ctypes import c_int32, c_int64
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


M = _load("tones_model")
STAGES = ("t", "u", "E_ctcss", "E_dtmf", "P", "ctcss", "dtmf")


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _up(arr):
    from iq_to_audio_amd import _dev as D

    return None if arr is None else D.from_numpy(arr)


def _decimate(theta, n, pos, hist, R, t_buf, u_buf):
    from iq_to_audio_amd import _native as N

    th, h, t, u = _up(theta), _up(hist), _up(t_buf), _up(u_buf)
    N.call("iqa_tones_decimate", N.ptr(th), c_int64(n), c_int64(pos), N.ptr(h), c_int32(R), N.ptr(t), N.ptr(u), N.stream_ptr())
    return t.cpu().numpy(), u.cpu().numpy()


def _bank(u, m, frame, hop, ntones, taps, e_buf, p_buf):
    from iq_to_audio_amd import _native as N

    dev = [_up(x) for x in (u, taps, e_buf, p_buf)]
    N.call("iqa_tones_bank", N.ptr(dev[0]), c_int64(m), c_int32(frame), c_int32(hop), c_int32(ntones), N.ptr(dev[1]), N.ptr(dev[2]), N.ptr(dev[3]),
           N.stream_ptr())
    return dev[2].cpu().numpy(), None if p_buf is None else dev[3].cpu().numpy()


# ---- a. iqa_tones_decimate, called directly -------------------------------------------------------------------------------


@pytest.mark.parametrize("R", list(M.SHAPE_R))
def test_decimate_at_every_tile_shape(A, R):
    """t is the quantiser and u the oracle's floor of the window sum, in every case of the table; nothing is written behind
    n or behind the outputs the block completes."""
    assert M.tile_outputs(R) * R == {1: 256, 2: 512, 31: 7936, 32: 8192, 33: 8184, 63: 8190, 64: 8192}[R]
    stats: dict = {}
    cases = M.decimate_cases(R)
    for case in cases:
        M.check_decimate(case, _decimate, stats)
    print(f"R {R}: {len(cases)} cases, {stats}")
    assert R == 1 or (stats["no output"] >= 2 and stats["from the history alone"] >= 2 and stats["negative, not divisible"] > 100)


def test_a_block_without_an_output_takes_a_null_u(A):
    """One sample that completes no output, with u_out NULL, as ``TonesCore`` calls it: t is written, nothing else."""
    from iq_to_audio_amd import _native as N

    R = 33
    theta = np.concatenate([np.array([1.5], dtype=np.float32), M.HOSTILE_F32])
    th, t = _up(theta), _up(np.full(1 + M.GUARD, M.SENT, dtype=np.int32))
    N.call("iqa_tones_decimate", N.ptr(th), c_int64(1), c_int64(5 * R), N.ptr(None), c_int32(R), N.ptr(t), N.ptr(None), N.stream_ptr())
    got = t.cpu().numpy()
    assert got[0] == 6144 and (got[1:] == M.SENT).all()


# ---- b. block invariance through ToneDecoder ------------------------------------------------------------------------------


@pytest.mark.parametrize("R", [33, M.MAX_R])
def test_block_invariance_around_the_tile_edge(A, R):
    """fs = 8000 R, theta fed as float32 blocks: cuts one before, on and one behind the first tile edge, a 1-sample block,
    blocks inside the 2R - 2 history and one that ends on its own second tile edge.  Every stage of every schedule is the
    oracle's, and so the single block's."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.decoders.tones import ToneDecoder

    fs, n, schedules = M.invariance_case(R)
    theta = M.shape_stream(fs, n)
    want = M.oracle(fs=fs, t=M.quantise(theta))
    assert want["plan"]["R"] == R
    dev = D.from_numpy(theta)
    runs = []
    for cuts in schedules:
        dec = ToneDecoder(fs)
        assert dec.plan.R == R and dec.core.hist_len == 2 * R - 2
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            dec.process(dev[lo:hi])
        assert dec.core.pos == n
        runs.append(dec.stages())
    M.check_invariance(runs, want, STAGES)


# ---- c. iqa_tones_bank, called directly -----------------------------------------------------------------------------------


def test_bank_at_the_plans_frames(A):
    """E and P are the oracle's at (N, H) of 8000, 519 999, 15 999, 96 000 and 96 153.8 Hz, with 50 tones without P and 8
    with it, at M exactly (F - 1) H + N and one more; the guards stay."""
    cases = M.bank_cases()
    assert {(c["N"], c["H"]) for c in cases} >= {(160, 80), (3200, 1600), (6400, 3200), (162, 81), (3250, 1625)}
    for case in cases:
        M.check_bank(case, _bank)


# ---- d. refusals ----------------------------------------------------------------------------------------------------------


def _sentinels(size=64):
    return [_up(np.full(size, M.SENT, dtype=np.int64)) for _ in range(5)]


def _untouched(bufs) -> bool:
    from iq_to_audio_amd import _dev as D

    D.torch_mod().cuda.synchronize()
    return all((b.cpu().numpy() == M.SENT).all() for b in bufs)


def test_decimate_refuses_before_it_launches(A):
    from iq_to_audio_amd import _native as N

    for what, n, pos, R, has_theta, has_t, has_u, message in M.decimate_refusals():
        with pytest.raises(ValueError, match=message):  # the model's entry first: the table is its own
            M.entry_decimate(np.zeros(64, np.float32) if has_theta else None, n, pos, None, R, np.zeros(64, np.int32) if has_t else None,
                             np.zeros(64, np.int32) if has_u else None)
        bufs = _sentinels()
        theta, hist, t, u = bufs[:4]
        with pytest.raises(ValueError, match=message):
            N.call("iqa_tones_decimate", N.ptr(theta if has_theta else None), c_int64(n), c_int64(pos), N.ptr(hist), c_int32(R),
                   N.ptr(t if has_t else None), N.ptr(u if has_u else None), N.stream_ptr())
        assert _untouched(bufs), what
    # the largest position the entry point takes is 2^50, and 2^40 + 3 lies below it
    assert M.BIG_POS < M.MAX_POS
    t = _up(np.full(1 + M.GUARD, M.SENT, dtype=np.int32))
    th = _up(np.array([0.25], dtype=np.float32))
    N.call("iqa_tones_decimate", N.ptr(th), c_int64(1), c_int64(M.MAX_POS), N.ptr(None), c_int32(7), N.ptr(t), N.ptr(None), N.stream_ptr())
    got = t.cpu().numpy()
    assert got[0] == 1024 and (got[1:] == M.SENT).all() and M.MAX_POS % 7 != 6


def test_bank_refuses_before_it_launches(A):
    from iq_to_audio_amd import _native as N

    for what, m, frame, hop, ntones, has_u, has_taps, has_e, message in M.bank_refusals():
        with pytest.raises(ValueError, match=message):
            M.entry_bank(np.zeros(8, np.int32) if has_u else None, m, frame, hop, ntones, np.zeros(8, np.int16) if has_taps else None,
                         np.zeros(8, np.int64) if has_e else None, None)
        bufs = _sentinels()
        u, taps, e, p = bufs[:4]
        with pytest.raises(ValueError, match=message):
            N.call("iqa_tones_bank", N.ptr(u if has_u else None), c_int64(m), c_int32(frame), c_int32(hop), c_int32(ntones),
                   N.ptr(taps if has_taps else None), N.ptr(e if has_e else None), N.ptr(p), N.stream_ptr())
        assert _untouched(bufs), what


def test_decide_refuses_before_it_launches(A):
    from iq_to_audio_amd import _native as N

    for what, fc, fd, frame, has_ec, has_ed, has_p, has_c, has_d, message in M.decide_refusals():
        with pytest.raises(ValueError, match=message):
            M.entry_decide_checks(fc, fd, frame, *[0 if has else None for has in (has_ec, has_ed, has_p, has_c, has_d)])
        bufs = _sentinels(1024)
        ec, ed, p, out_c, out_d = bufs
        with pytest.raises(ValueError, match=message):
            N.call("iqa_tones_decide", N.ptr(ec if has_ec else None), c_int64(fc), N.ptr(ed if has_ed else None), N.ptr(p if has_p else None),
                   c_int64(fd), c_int32(frame), N.ptr(out_c if has_c else None), N.ptr(out_d if has_d else None), N.stream_ptr())
        assert _untouched(bufs), what
