"""The reference's pluggable stage classes (``ComplexOscillator``, ``OverlapSaveFIR``, ``Decimator``) on the GPU.

Same names, arguments, state attributes and error behaviour as the reference classes (cited per class).  Stage methods
accept either NumPy arrays (NumPy comes back, like the reference) or device tensors (device tensors come back -- no host
round trip).  The pipelines do not run them: they run :class:`channelizer.Channelizer`, the three stages fused.
"""
from __future__ import annotations

import math
from ctypes import c_double, c_int32, c_int64

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P
from .channelizer import _ChannelKernel


def _size(x) -> int:
    return int(x.numel()) if D.is_tensor(x) else int(np.asarray(x).size)


class ComplexOscillator:
    """Continuous complex exponential for frequency translation (reference processing.py:282-297).

    ``phase`` (radians) and ``increment`` are host floats exactly as in the reference; the
    float64 ramp ``phase + sign*increment*n`` is evaluated per sample on the GPU.
    ``fmt``/``iq_order`` let the stage also do the ingest convert when fed raw frames.
    """

    def __init__(self, freq_offset_hz: float, sample_rate: float):
        self.phase = 0.0
        self.increment = -2.0 * np.pi * freq_offset_hz / sample_rate

    def mix(self, samples, sign: int, *, fmt: str = "f32", iq_order: str = "iq"):
        if _size(samples) == 0:
            return samples
        if iq_order not in N.ORDER:
            raise ValueError(f"Unsupported iq_order '{iq_order}'")
        if fmt == "f32":
            x = D.to_device(samples, "complex64")
            n = x.numel()
        else:
            x = D.to_device(samples, {"s16": "int16", "u8": "uint8"}[fmt]).reshape(-1)
            n = x.numel() // 2
        out = D.empty(n, "complex64")
        step = sign * self.increment
        N.call("iqa_oscillator_mix", c_int32(P.FMT_CODE[fmt]), c_int32(N.ORDER[iq_order]), N.ptr(x), c_int64(n),
               c_double(self.phase), c_double(step), N.ptr(out), N.stream_ptr())
        self.phase = (self.phase + step * n) % (2.0 * np.pi)
        return D.like_input(out, samples)


class OverlapSaveFIR:
    """Streaming channel filter stage (reference processing.py:300-346).

    Same constructor, attributes (``taps``, ``filter_len``, ``overlap``, ``block_size``,
    ``fft_size``, ``state``) and semantics -- causal linear convolution, zero initial state,
    output length == input length, history of the last L-1 input samples carried across
    calls -- but evaluated as a direct time-domain dot product on the GPU: ``block_size``
    and ``fft_size`` are kept for API compatibility and do not affect the result.
    """

    def __init__(self, taps: np.ndarray, block_size: int, *, workers: int | None = None):
        if block_size <= 0:
            raise ValueError("block_size must be positive")
        self.taps = np.asarray(taps).astype(np.complex128)
        self.filter_len = len(taps)
        self.overlap = self.filter_len - 1
        self.block_size = block_size
        self.fft_size = 1 << math.ceil(math.log2(self.block_size + self.filter_len - 1))
        self.workers = None
        self._kernel = None
        self._real_taps = np.asarray(taps, dtype=np.float64)
        self._hist = None  # device complex64[L-1]
        self._consumed = 0

    @property
    def state(self) -> np.ndarray:
        if self._hist is None:
            return np.zeros(self.overlap, dtype=np.complex64)
        return self._hist.cpu().numpy()

    @property
    def taps_fft(self) -> np.ndarray:
        """The reference's frequency response of the zero-padded taps (processing.py:317-321), computed on request:
        nothing here uses it (the filter runs in the time domain), it exists for callers that inspect the stage."""
        padded = np.zeros(self.fft_size, dtype=np.complex128)
        padded[: self.filter_len] = self.taps
        return np.fft.fft(padded)

    def process(self, samples):
        if _size(samples) == 0:
            return samples
        if self._kernel is None:
            self._kernel = _ChannelKernel(P.plan_plain_fir(self._real_taps))
        x = D.to_device(samples, "complex64")
        n = x.numel()
        y = self._kernel.run(x, n, self._consumed, self._hist, self._consumed, n)
        if self.overlap:
            nxt = D.empty(self.overlap, "complex64")
            N.call("iqa_history_update", c_int32(P.FMT_CODE["f32"]), c_int32(self.filter_len), N.ptr(self._hist),
                   N.ptr(x), c_int64(n), N.ptr(nxt), N.stream_ptr())
            self._hist = nxt
        self._consumed += n
        return D.like_input(y, samples)


class Decimator:
    """Keep global sample indices 0, D, 2D, ... across calls (reference processing.py:349-360)."""

    def __init__(self, factor: int):
        self.factor = max(1, factor)
        self.offset = 0

    def process(self, samples):
        n = _size(samples)
        if self.factor == 1 or n == 0:
            return samples
        start = (-self.offset) % self.factor
        self.offset = (self.offset + n) % self.factor
        n_out = 0 if start >= n else -(-(n - start) // self.factor)
        x = D.to_device(samples, "complex64")
        out = D.empty(n_out, "complex64")
        N.call("iqa_decimate", N.ptr(x), c_int64(n), c_int64(start), c_int32(self.factor), N.ptr(out), c_int64(n_out),
               N.stream_ptr())
        return D.like_input(out, samples)
