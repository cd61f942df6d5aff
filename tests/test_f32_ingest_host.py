"""float32 ingest as int16 planes: the host-side parts, no GPU needed -- the C ABI's argument checks of
``iqa_f32_split_s16`` / ``iqa_f32_to_s16_exact`` and the precision guard's arithmetic for planes with headroom."""
from __future__ import annotations

import math
from ctypes import c_int32, c_int64, c_void_p
from types import SimpleNamespace

import pytest

import iq_to_audio_amd as A
from iq_to_audio_amd import processing as PR

OK, BAD = c_void_p(4096), c_void_p(4096 + 4)  # never dereferenced: the checks come first (BAD is 4 bytes off 16-byte alignment)


def _split(f32=OK, n=16, shift=0, hi=OK, lo=OK, flag=OK):
    A.native.call("iqa_f32_split_s16", f32, c_int64(n), c_int32(shift), hi, lo, flag, c_void_p(0))


def _exact(f32=OK, n=16, out=OK, flag=OK):
    A.native.call("iqa_f32_to_s16_exact", f32, c_int64(n), out, flag, c_void_p(0))


@pytest.mark.parametrize("bad", [dict(n=-1), dict(shift=-1), dict(shift=16), dict(f32=None), dict(hi=None), dict(lo=None),
                                 dict(flag=None), dict(f32=BAD)])
def test_f32_split_abi_rejects_bad_arguments_before_any_launch(bad):
    A.native.build()
    A.native.lib()
    with pytest.raises(ValueError):
        _split(**bad)


@pytest.mark.parametrize("bad", [dict(n=-1), dict(f32=None), dict(out=None), dict(flag=None), dict(f32=BAD)])
def test_f32_to_s16_exact_abi_rejects_bad_arguments_before_any_launch(bad):
    A.native.build()
    A.native.lib()
    with pytest.raises(ValueError):
        _exact(**bad)


def test_f32_ingest_zero_length_is_a_no_op():
    """n_values == 0 returns IQA_OK without touching a pointer (NULL ones included) or the device."""
    A.native.build()
    A.native.lib()
    for shift in (0, 15):
        _split(n=0, shift=shift)
        _split(None, 0, shift, None, None, None)
    _exact(n=0)
    _exact(None, 0, None, None)


class _Kernel(SimpleNamespace):
    """A planned kernel as ``pick_precision`` sees it: its precision, and (tap-rounding norm, floors) of its plan -- the
    uniform-low-byte floor alone (zero-input response and coherent bound 0: ``floor`` is the whole level-independent part)."""

    def _ensure_mfma(self):
        return SimpleNamespace(err_norm=self.norm, floor_rms=self.floor, zero_rms=0.0, coherent_rms=0.0)


def test_precision_guard_scales_the_floor_by_the_planes_headroom():
    """A float32 capture run as int16 planes with ``shift`` bits of headroom: hi = rint(2^(15 - shift) x), so the kernel's
    level-independent floor is worth 2^shift of the capture's full scale while the tap-rounding term follows the level.
    pick_precision(floor_scale=2^shift) judges err = hypot(norm * wideband, 2^shift * floor)."""
    plans = {"fast": (1e-4, 4e-6), "fine": (1e-5, 1e-7), "full": (1e-7, 1e-9)}
    kernels = {k: _Kernel(precision=k, _mfma_ok=True, norm=n, floor=f) for k, (n, f) in plans.items()}
    wide = 0.01

    def err(name, scale):
        n, f = plans[name]
        return math.hypot(n * wide, scale * f)

    assert err("fast", 2.0) > 1.1 * err("fast", 1.0)  # the floor matters at this level
    # a channel just above the "fast" bar at shift 0 ...
    power = (PR.PRECISION_GUARD * err("fast", 1.0) * 1.05) ** 2
    assert PR.pick_precision(kernels.__getitem__, "fast", "nfm", power, wide) == "fast"
    assert PR.pick_precision(kernels.__getitem__, "fast", "nfm", power, wide, floor_scale=1.0) == "fast"
    # ... is below it when the planes have one bit of headroom, and moves on to "fine"
    assert PR.pick_precision(kernels.__getitem__, "fast", "nfm", power, wide, floor_scale=2.0) == "fine"
    # the boundary itself, at shift 3: exactly guard x error passes, just below it does not
    at = PR.PRECISION_GUARD * err("fast", 8.0)
    assert PR.pick_precision(kernels.__getitem__, "fast", "nfm", (at * (1 + 1e-9)) ** 2, wide, floor_scale=8.0) == "fast"
    assert PR.pick_precision(kernels.__getitem__, "fast", "nfm", (at * (1 - 1e-6)) ** 2, wide, floor_scale=8.0) == "fine"
    # a floor that is all of the error: the scale moves the bar by exactly 2^shift
    flat = {k: _Kernel(precision=k, _mfma_ok=True, norm=0.0, floor=f) for k, (_, f) in plans.items()}
    bar = PR.PRECISION_GUARD * plans["fast"][1]
    assert PR.pick_precision(flat.__getitem__, "fast", "nfm", (bar * 1.5) ** 2, wide, floor_scale=1.0) == "fast"
    assert PR.pick_precision(flat.__getitem__, "fast", "nfm", (bar * 1.5) ** 2, wide, floor_scale=2.0) == "fine"
    # not NFM: never guarded, whatever the scale
    assert PR.pick_precision(kernels.__getitem__, "fast", "am", 1e-30, wide, floor_scale=256.0) == "fast"


def test_target_judges_float32_planes_with_their_headroom(monkeypatch):
    """_Target._pick_precision hands 2^f32_shift to the guard for a float32 capture on the int16 path, 1 otherwise."""
    seen = []
    monkeypatch.setattr(PR, "pick_precision", lambda *a, floor_scale=1.0, **k: seen.append(floor_scale) or "fast")
    for fmt, integer_path, shift, want in (("f32", True, 0, 1.0), ("f32", True, 3, 8.0), ("f32", False, 3, 1.0),
                                           ("s16", True, 3, 1.0)):
        t = PR._Target.__new__(PR._Target)
        t.cfg = SimpleNamespace(demod_mode="nfm", agc_enabled=True)
        t.demod = object()
        t.info = SimpleNamespace(fmt=fmt)
        t.owner = SimpleNamespace(f32_integer_path=integer_path)
        t.f32_shift = shift
        t.mix_sign = 1
        t._pick_precision(1e-6, 0.1)
        assert seen[-1] == want, (fmt, integer_path, shift)
