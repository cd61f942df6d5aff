"""GPU stand-in for the reference's ``src/iq_to_audio/processing.py`` DSP surface.

Same names, arguments, state attributes and error behaviour as the reference classes
(cited per class), with all arithmetic in the HIP library (``libiqa_hotpath.so``):

    ProcessingConfig / ProcessingPipeline / ProcessingResult / ProcessingCancelled
    ComplexOscillator, OverlapSaveFIR, Decimator, design_channel_filter,
    choose_mix_sign, tune_chunk_size

plus :class:`Channelizer` (``channelizer.py``), the fused ingest+mix+filter+decimate stage the pipeline
actually runs (one pass over the raw int16/u8/f32 capture in HBM).

Stage methods accept either NumPy arrays (NumPy comes back, like the reference) or
device tensors (device tensors come back -- no host round trip).  There is no CPU path:
without a GPU or without the built library every stage raises ``RuntimeError``.
"""
from __future__ import annotations

import contextlib
import logging
import math
import threading
from ctypes import byref, c_double, c_int32, c_int64
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P
from . import iqio
from .channelizer import (_KERNEL_CACHE, _KERNEL_CACHE_LOCK, _KERNEL_CACHE_MAX, _TAPS_MEMO, ChannelBank,  # noqa: F401  (re-exported)
                          Channelizer, _as_frames, _cached_kernel, _ChannelKernel, _taps_fingerprint, immutable_taps)
from .decoders import create_decoder
from .decoders.common import unit_prev
from .decoders.rds import RdsCore
from .decoders.side import SIDE_DECODERS, check_modes
from .decoders.wfm import WfmStereoCore, stereo_matrix
from .dsp_plan import design_channel_filter, tune_chunk_size  # noqa: F401  (re-exported API)
from .gate import CarrierGate, CarrierSquelch
from .progress import PhaseState, ProgressSink, ProgressTracker

LOG = logging.getLogger(__name__)


@dataclass
class ProcessingConfig:
    """Identical field set and defaults to the reference (processing.py:38-62).
    ``fft_workers`` is accepted and ignored (there is no FFT on this path)."""

    in_path: Path
    target_freq: float = 0.0
    bandwidth: float = 12_500.0
    center_freq: float | None = None
    center_freq_source: str | None = None
    demod_mode: str = "nfm"
    fs_ch_target: float = 96_000.0
    deemph_us: float = 300.0
    agc_enabled: bool = True
    output_path: Path | None = None
    dump_iq_path: Path | None = None
    chunk_size: int = 1_048_576
    filter_block: int = 65_536
    iq_order: str = "iq"
    probe_only: bool = False
    mix_sign_override: int | None = None
    plot_stages_path: Path | None = None
    fft_workers: int | None = None
    max_input_seconds: float | None = None
    input_container: str | None = None
    input_format: str | None = None
    input_format_source: str | None = None
    input_sample_rate: float | None = None


@dataclass
class SampleRateProbe:
    """Where the sample rate came from (reference probe.py SampleRateProbe; only the header
    parse exists here -- no ffprobe / libsndfile)."""

    ffprobe: float | None = None
    header: float | None = None
    wave: float | None = None

    @property
    def value(self) -> float:
        for v in (self.ffprobe, self.header, self.wave):
            if v:
                return float(v)
        raise RuntimeError("Unable to determine sample rate.")


def _size(x) -> int:
    return int(x.numel()) if D.is_tensor(x) else int(np.asarray(x).size)


# --------------------------------------------------------------------------------------------- #
# pluggable stages                                                                              #
# --------------------------------------------------------------------------------------------- #


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


def probe_targets(warmup, sample_rate: float, specs: list, decimation: int, *, fmt: str, iq_order: str, host) -> list | None:
    """The mixer-sign probes of SEVERAL targets of one capture (``specs``: ``(freq_offset, taps)`` each) in as few launches
    as one bank takes: both signs of every target are channels of one :class:`ChannelBank` over the snippet (lane pairs,
    tap-row groups and their combine launches as for the capture itself) and ONE reduction writes all mean powers into
    ``host`` (pinned float64, two per target, owned by the caller until the probes have been read).  Returns one
    :class:`MixSignProbe` per target, or None when the grouped path does not apply (the caller then probes target by
    target): float32 captures, targets whose snippet or discard lengths differ, kernels without a shared shape."""
    if fmt not in ("s16", "u8") or not specs:
        return None
    x_all, n_in = _as_frames(warmup, fmt)
    decim = max(decimation, 1)
    shapes = set()
    for _, taps in specs:  # the lengths MixSignProbe.__init__ / _probe_one derive (reference processing.py:636-656)
        ntaps = len(taps)
        snippet = min(n_in, max(int(sample_rate * 0.05), ntaps * 4, 131_072))
        if snippet < ntaps:
            snippet = min(n_in, ntaps * 2)
        n_z = -(-snippet // decim)
        discard = min(ntaps, n_z // 4)
        shapes.add((n_z, discard if n_z - discard else 0))
    if len(shapes) != 1:
        return None
    n_z, discard = shapes.pop()
    keep = n_z - discard
    if keep < 64 or keep > MixSignProbe.DIRECT_MAX or host.numel() < 2 * len(specs):
        return None
    chans = [Channelizer(taps, sample_rate=sample_rate, freq_offset=f_off, mix_sign=sign, decimation=decim, fmt=fmt, iq_order=iq_order)
             for f_off, taps in specs for sign in (1, -1)]
    z_keep = D.empty(len(chans) * keep, "complex64")
    if not ChannelBank(chans).run_interior_only(x_all, n_in, discard, keep, [z_keep[i * keep : (i + 1) * keep] for i in range(len(chans))]):
        return None
    N.call("iqa_mean_power_batch", N.ptr(z_keep), c_int64(keep), c_int32(len(chans)), c_int64(0), N.ptr(host), N.stream_ptr())
    level_slot = None
    if host.numel() > 2 * len(specs):  # room for the wideband level of the warm-up block behind the powers
        level_slot = host[2 * len(specs) : 2 * len(specs) + 1]
        queue_raw_level(warmup, fmt, level_slot)
    done = D.torch_mod().cuda.Event()
    done.record()
    return [MixSignProbe.from_powers(host[2 * i : 2 * i + 2], done, level_slot, fmt) for i in range(len(specs))]


def _mean_power_into(z_dev, skip: int, out_slot) -> None:
    N.call("iqa_mean_power", N.ptr(z_dev), c_int64(z_dev.numel()), c_int64(skip), N.ptr(out_slot), N.stream_ptr())


_PINNED_SCALARS: list = []  # [pinned double[4], owner] -- a buffer goes back to the pool when its probe has been read


def _pinned_scalars(owner):
    """A reusable pinned double[4] for probe read-backs (pin_memory() is slow: allocate once per slot).  The
    buffer stays with ``owner`` until ``_release_scalars``: several probes may be in flight at once."""
    torch = D.torch_mod()
    with _KERNEL_CACHE_LOCK:
        for t in _PINNED_SCALARS:
            if t[1] is None:
                t[1] = owner
                return t[0]
        t = [torch.zeros(4, dtype=torch.float64).pin_memory(), owner]  # [power(+1), power(-1), raw mean square, spare]
        _PINNED_SCALARS.append(t)
        return t[0]


def reserve_pinned_scalars(count: int) -> None:
    """Make sure ``count`` probe read-back buffers are free NOW (pinning memory is not allowed while a stream is being
    captured: a caller about to capture ``count`` probes into a graph reserves them first)."""
    torch = D.torch_mod()
    with _KERNEL_CACHE_LOCK:
        free = sum(1 for t in _PINNED_SCALARS if t[1] is None)
        for _ in range(max(0, count - free)):
            _PINNED_SCALARS.append([torch.zeros(4, dtype=torch.float64).pin_memory(), None])


def _release_scalars(buf) -> None:
    with _KERNEL_CACHE_LOCK:
        for t in _PINNED_SCALARS:
            if t[0] is buf:
                t[1] = None


def queue_raw_level(warmup, fmt: str, out_slot) -> None:
    """Queue the wideband-level estimate of raw frames (``iqa_raw_level``: mean square of up to 65536 values spread over
    ``warmup``) into ``out_slot`` (double[1], device or pinned host memory) on the current stream."""
    x, n = _as_frames(warmup, fmt)
    flat = x.view(D.torch_mod().float32) if x.is_complex() else x
    N.call("iqa_raw_level", c_int32(P.FMT_CODE[fmt]), N.ptr(flat), c_int64(flat.numel()), N.ptr(out_slot), N.stream_ptr())


def wideband_rms_from(mean_square: float, fmt: str) -> float:
    """RMS of the complex samples (fraction of full scale) from the mean square of the raw values."""
    return math.sqrt(max(2.0 * float(mean_square), 0.0)) * P.INGEST_SCALE[fmt]


#: Precision guard.  The fixed-point channelizers' error is a fraction of the WIDEBAND level whatever the channel holds
#: (tap rounding x wideband RMS, 1..5 x that on tonal captures, plus a level-independent floor: MfmaPlan.z_error_rms), and
#: the FM discriminator divides by the channel's own level: audio error ~ 0.024 x error / |z|.  An NFM channel whose
#: probed level is below guard x (expected z error) is therefore channelized at the next precision that clears it
#: (measured: a -70 dBFS NFM signal beside a full-scale tone comes out 2.8e-4 RMS off the reference at "fast").
PRECISION_GUARD = 1000.0
#: the demodulators that divide by |z| (the discriminator): what the guard protects
FM_MODES = ("nfm", "fm", "wfm")


def pick_precision(kernel_for, base: str, demod_mode: str | None, channel_power, wideband_rms, guard: float | None = None,
                   memo: dict | None = None, floor_scale: float = 1.0) -> str:
    """The cheapest precision, not below ``base``, at which a channel of mean power ``channel_power`` (|z|^2, from the
    mixer-sign probe) in a capture of wideband RMS ``wideband_rms`` keeps the 1e-4 audio bar.  Only NFM is guarded (AM
    and SSB do not divide by |z|).  ``kernel_for(precision)`` returns the planned ``_ChannelKernel``; ``memo`` (a dict the
    caller keeps per channel and sign) remembers each precision's (tap-rounding norm, floor), so that a batch asks the
    kernels once, not once per capture.  ``floor_scale``: what one unit of the kernel's full scale is worth in the capture's
    -- 2^shift for a float32 capture run as int16 planes with ``shift`` bits of headroom (hi = rint(2^(15 - shift) x)): the
    tap-rounding term follows the level and is unchanged, the level-independent floor grows by that factor."""
    levels = _ChannelKernel.PRECISIONS
    guard = PRECISION_GUARD if guard is None else guard
    if not guard or channel_power is None or wideband_rms is None or (demod_mode or "").lower() not in FM_MODES:
        return base
    level = math.sqrt(max(float(channel_power), 0.0))
    for name in levels[levels.index(base):]:
        if name == "float32":
            break
        known = None if memo is None else memo.get(name)
        if known is None:
            k = kernel_for(name)
            if k.precision != name:  # (this capture format has no such kernel: uint8 "full", float32 anything)
                known = False
            elif not k._mfma_ok:
                known = (0.0, 0.0)
            else:
                mp = k._ensure_mfma()
                known = (float(mp.err_norm), float(mp.floor_rms))
            if memo is not None:
                memo[name] = known
        if known is False:
            continue
        err = math.hypot(known[0] * wideband_rms, floor_scale * known[1])
        if err <= 0.0 or level >= guard * err:
            return name
    return "float32"


def base_precision(demod_mode: str | None, agc_enabled: bool) -> str:
    """SSB with the AGC on is ill-conditioned in the reference itself: ``_apply_agc`` adds 0.001*(target/|s| - gain) per
    sample for |s| down to 1e-6 (decoders/ssb.py:75-77), so a z difference of 1e-6 near a zero crossing moves the gain
    by hundreds.  Those targets take the "full" precision (z error below the float32 rounding of z itself); everything
    else starts at "fast"."""
    return SSB_AGC_PRECISION if ((demod_mode or "").lower() in ("usb", "lsb", "ssb") and agc_enabled) else "fast"


SSB_AGC_PRECISION = "full"


class MixSignProbe:
    """``choose_mix_sign`` split into an asynchronous launch and a blocking ``result()``, so the
    caller can plan the channelizer while the two probes run."""

    #: iqa_mean_power handles up to this many samples with its single-block, atomics-free kernel
    DIRECT_MAX = 65536

    def __init__(self, warmup, sample_rate: float, freq_offset: float, taps: np.ndarray, decimation: int, *,
                 fmt: str = "f32", iq_order: str = "iq", record_done: bool = True, matrix_cores: bool = True,
                 measure_level: bool = False):
        """``record_done=False``: the caller sets ``_done`` to event(s) of its own that lie behind both probes (an
        event record between two kernels of a stream costs ~7 us on this part).  ``matrix_cores=False``: the probes go
        through the float32 kernel (a few thousand outputs: tens of microseconds), which -- unlike a ring-kernel launch
        -- finds room on a CU beside a running channelizer pass.  ``measure_level``: also estimate the wideband level of
        ``warmup`` (``wideband_rms`` after ``result()`` / ``peek()``: what the precision guard compares ``power`` with)."""
        self._matrix_cores = bool(matrix_cores)
        self._powers = None
        self.power = None
        self.wideband_rms = None
        self._fmt = fmt
        self._level = bool(measure_level)
        self._valid = [False, False]
        x_all, n_in = _as_frames(warmup, fmt)
        if n_in == 0:
            return
        ntaps = len(taps)
        max_len = max(int(sample_rate * 0.05), ntaps * 4, 131_072)
        snippet_len = min(n_in, max_len)
        if snippet_len < ntaps:
            snippet_len = min(n_in, ntaps * 2)
        x = x_all[:snippet_len] if x_all.is_complex() else x_all[: 2 * snippet_len]
        decim = max(decimation, 1)
        self._powers = D.empty(2, "float64")  # iqa_mean_power overwrites its slot
        self._host = _pinned_scalars(id(self))
        self._sign = None
        if not (self._matrix_cores and self._probe_pair(x_all, n_in, snippet_len, taps, sample_rate, freq_offset, decim, fmt, iq_order)):
            for i, sign in enumerate((1, -1)):
                self._probe_one(i, sign, x_all, n_in, x, snippet_len, taps, sample_rate, freq_offset, decim, fmt, iq_order)
        if self._level:
            queue_raw_level(warmup, fmt, self._host[2:3])
        self._done = None
        if record_done:
            self._done = D.torch_mod().cuda.Event()
            self._done.record()

    @classmethod
    def from_powers(cls, host_pair, done_event, level_slot=None, fmt: str = "s16"):
        """A probe whose two mean powers (sign +1, sign -1) are being written into ``host_pair`` (a pinned float64[2] the
        caller owns) by launches already queued; ``done_event`` lies behind them.  See ``probe_targets``."""
        self = cls.__new__(cls)
        self._powers, self.power, self._valid, self._sign = host_pair, None, [True, True], None
        self._host, self._done, self._matrix_cores = host_pair, done_event, True
        self.wideband_rms, self._fmt, self._level, self._level_slot = None, fmt, level_slot is not None, level_slot
        return self

    def _probe_pair(self, x_all, n_in, snippet_len, taps, sample_rate, freq_offset, decim, fmt, iq_order) -> bool:
        """Both signs in two launches instead of four: the two channelizers as the two lanes of one matrix-core launch
        over the snippet (shared ingest) and one reduction with a workgroup per sign, written into the pinned slot.
        Only where ``_probe_one`` would take its interior-only path for both signs and a probe is short enough for the
        single-workgroup reduction; False (nothing queued) otherwise."""
        if fmt not in ("s16", "u8"):
            return False
        ntaps = len(taps)
        n_z = -(-snippet_len // decim)
        discard = min(ntaps, n_z // 4)
        keep = n_z - discard
        if keep <= 0 or keep > self.DIRECT_MAX:
            return False
        chans = [Channelizer(taps, sample_rate=sample_rate, freq_offset=freq_offset, mix_sign=sign, decimation=decim, fmt=fmt,
                             iq_order=iq_order) for sign in (1, -1)]
        z_keep = D.empty(2 * keep, "complex64")
        if not ChannelBank(chans).run_interior_only(x_all, n_in, discard, keep, [z_keep[:keep], z_keep[keep:]]):
            return False
        N.call("iqa_mean_power_batch", N.ptr(z_keep), c_int64(keep), c_int32(2), c_int64(0), N.ptr(self._host), N.stream_ptr())
        self._valid = [True, True]
        return True

    def _probe_one(self, i, sign, x_all, n_in, x, snippet_len, taps, sample_rate, freq_offset, decim, fmt, iq_order):
        """Queue the probe for one mixer sign on the current stream; its mean power ends up in ``_host[i]``."""
        ntaps = len(taps)
        ch = Channelizer(taps, sample_rate=sample_rate, freq_offset=freq_offset, mix_sign=sign, decimation=decim,
                         fmt=fmt, iq_order=iq_order)
        n_z = -(-snippet_len // decim)
        discard = min(ntaps, n_z // 4)
        if n_z - discard == 0:
            discard = 0
        # Only z[discard:] enters the power (processing.py:651-656), and those outputs see neither the zero
        # initial state nor anything past the snippet: when the warm-up buffer is longer than the snippet they are
        # all interior outputs of the matrix-core kernel -- one launch per sign instead of three.
        z_keep = D.empty(n_z - discard, "complex64")
        if self._matrix_cores and fmt in ("s16", "u8") and ch._kernel.run_interior_only(x_all, n_in, discard, n_z - discard, z_keep):
            # a short reduction is one block that WRITES its result: straight into the mapped pinned slot, no
            # device scalar and no copy behind it (a blit between kernels costs ~13 us of a 0.9 ms capture)
            direct = z_keep.numel() <= self.DIRECT_MAX
            _mean_power_into(z_keep, 0, (self._host if direct else self._powers)[i : i + 1])
            self._valid[i] = True
            if not direct:
                self._host[i : i + 1].copy_(self._powers[i : i + 1], non_blocking=True)
            return
        z = ch.process(x, last_block=True)
        if z.numel():
            discard = min(ntaps, z.numel() // 4)
            if z.numel() - discard == 0:
                discard = 0
            direct = z.numel() - discard <= self.DIRECT_MAX  # (one workgroup writes the mean: straight into the pinned slot)
            _mean_power_into(z, discard, (self._host if direct else self._powers)[i : i + 1])
            self._valid[i] = True
            if not direct:
                self._host[i : i + 1].copy_(self._powers[i : i + 1], non_blocking=True)

    def result(self) -> int:
        if self._powers is None:
            return 1
        if self._sign is None:
            self._wait()
            self._sign = self._decide()
            _release_scalars(self._host)
            self._host = None
        return self._sign

    def _decide(self) -> int:
        host = self._host.numpy()
        best_sign, best_power = 1, -np.inf
        for i, sign in enumerate((1, -1)):
            power = float(host[i]) if self._valid[i] else -np.inf
            if power > best_power:
                best_power, best_sign = power, sign
        self.power = best_power if np.isfinite(best_power) else None  # mean |z|^2 of the chosen sign's probe
        if self._level:
            slot = getattr(self, "_level_slot", None)
            self.wideband_rms = wideband_rms_from(float(slot[0]) if slot is not None else float(host[2]), self._fmt)
        return best_sign

    def peek(self) -> int:
        """The sign the two powers in the pinned slot say NOW, without giving the slot back: for probes that live inside
        a captured graph (every replay writes the same slot again; the caller has waited for the replay)."""
        return 1 if self._powers is None else self._decide()

    def _wait(self) -> None:
        done = self._done
        for ev in (done if isinstance(done, (list, tuple)) else [done]):
            ev.synchronize()

    def __del__(self):
        try:
            if getattr(self, "_host", None) is not None and self._sign is None:
                self._wait()  # the write into the pinned buffer must not land in someone else's read-back
                _release_scalars(self._host)
        except Exception:
            pass


def choose_mix_sign(warmup, sample_rate: float, freq_offset: float, taps: np.ndarray, decimation: int, *,
                    fmt: str = "f32", iq_order: str = "iq") -> int:
    """Pick the mixer sign that puts more power in the channel (reference processing.py:623-663).

    For each sign the first ``min(len, max(0.05*fs, 4L, 131072))`` samples are mixed, filtered
    from zero state, decimated (``[::D]``) and the mean power after dropping the first
    ``min(L, n/4)`` decimated samples is compared; strictly greater wins, ties give +1.
    ``warmup`` is complex64 (NumPy / tensor) or raw frames when ``fmt`` is 's16'/'u8'.
    Both probes are enqueued before the single host read-back of the two powers.
    """
    return MixSignProbe(warmup, sample_rate, freq_offset, taps, decimation, fmt=fmt, iq_order=iq_order).result()


# --------------------------------------------------------------------------------------------- #
# pipeline                                                                                      #
# --------------------------------------------------------------------------------------------- #


@dataclass
class ProcessingResult:
    """reference processing.py:666-675"""

    sample_rate_probe: SampleRateProbe
    center_freq: float
    target_freq: float
    freq_offset: float
    decimation: int
    fs_channel: float
    mix_sign: int
    audio_peak: float


class ProcessingCancelled(RuntimeError):  # noqa: N818
    """Raised when processing is aborted early by user request (reference processing.py:678)."""


class ChannelDemod:
    """Demodulate + AudioWriter.write for many reference chunks in one fused call.

    ``decoder.process`` (processing.py:1128) followed by ``audio_writer.write`` (:1147) for a whole
    block: the only per-chunk behaviour of the reference decoders is the SSB AGC restart
    (decoders/ssb.py:72), expressed as restart indices of the segmented scan; the writer's pre-clip
    peak, +-0.99 clip and the per-chunk sum of squares (rms_dbfs) are fused into the last scan pass
    (``iqa_demodulate``).  ``self.decoder`` is the matching pluggable decoder object (kept for its
    parameters and API parity; the fused path carries its own device state).

    The side decoders (``pocsag= ax25= tones= acars= ais= adsb=``; ``decoders/side.py`` lists their modes, plans and cores):
    after the fused call every block also runs, per active decoder in table order, ``iqa_quadrature`` with a ``prev`` of the
    decoder's own or ``iqa_envelope``, into a buffer that is never the audio buffer, and the core's per-block launch.
    ``side[name]`` is the core, ``side_result(name)`` the run's result.  Off, none of a decoder's entry points is called.
    """

    def __init__(self, mode: str, fs_channel: float, *, deemph_us: float, agc_enabled: bool, pocsag: bool = False, ax25: bool = False,
                 tones: bool = False, acars: bool = False, ais: bool = False, adsb: bool = False):
        self.decoder = create_decoder(mode, deemph_us=deemph_us, agc_enabled=agc_enabled)
        self.decoder.setup(fs_channel)
        self.params = self.decoder.fused_params()
        flags = dict(pocsag=pocsag, ax25=ax25, tones=tones, acars=acars, ais=ais, adsb=adsb)
        check_modes(flags, [mode], plural=False)
        # (entry, core, the discriminator's prev or None) per active decoder, in table order; a plan raises ValueError where the
        # channel rate does not fit it
        self._side = tuple((e, e.core(e.plan(fs_channel)), unit_prev() if e.source == "theta" else None)
                           for e in SIDE_DECODERS if flags.get(e.name))
        self.side = {e.name: core for e, core, _ in self._side}
        self._needs_scratch = self.params.mode in (N.DEMOD_MODE["usb"], N.DEMOD_MODE["lsb"]) and bool(self.params.agc_enabled)
        self.chunk_sumsq: list = []  # (device float64[n_chunks*8], counts)
        self._blk = None  # one device block: [state 32 B | peak 4 B (+pad to 64) | sumsq n_chunks*8 f64]
        self._starts_key = None
        self._fresh = False
        self._from_reset = False
        self._alloc_block(0)

    # {float2 prev = 1+0j; double y_last; double x_last, y_last} -- the states of a decoder that has seen nothing
    _STATE0 = np.array([1.0, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32)

    def _alloc_block(self, n_chunks: int) -> None:
        torch = D.torch_mod()
        img = np.zeros(64 + n_chunks * 64, dtype=np.uint8)
        img[:32] = self._STATE0.view(np.uint8)
        self._img, self._img_host = img, None
        self._blk = D.from_numpy(img)
        self._n_chunks = n_chunks
        self.state_dev = self._blk[:32].view(torch.float32)
        self.peak_dev = self._blk[32:36].view(torch.float32)
        self._sumsq = self._blk[64:].view(torch.float64)
        self._fresh = True

    def reset(self, force: bool = False, ahead: bool = False) -> None:
        """Back to a decoder that has seen nothing (states, peak, per-chunk sums).  Nothing is launched here: the next
        ``process`` starts from the initial state by itself (``iqa_demodulate_from_reset``).  ``ahead=True`` (nfm): the
        current stream is a side stream that the stream of ``process`` will wait for -- the state block, the peak and the
        sums are put back there now (``iqa_demod_reset``, one small launch), and ``process`` is the plain
        ``iqa_demodulate``: one launch on its stream instead of a clear and a scan."""
        self.chunk_sumsq = []
        if self._side:  # (before the early return: the side decoders' state is not part of ``_fresh``)
            for _, core, _ in self._side:
                core.reset()
            self._side = tuple((e, core, prev if prev is None else unit_prev()) for e, core, prev in self._side)
        if self._fresh and not force:  # (force: a step being captured into a graph must not depend on what ran before it)
            return
        if ahead and self.params.mode == N.DEMOD_MODE["nfm"]:
            N.call("iqa_demod_reset", N.ptr(self.state_dev), N.ptr(self.peak_dev), N.ptr(self._sumsq), c_int64(self._sumsq.numel()),
                   N.stream_ptr())
            self._from_reset = False
            self._fresh = True
            return
        # nothing is copied: the next ``process`` starts from the initial state by itself and clears the peak and the
        # per-chunk sums (iqa_demodulate_from_reset) -- one node less per capture in a captured step
        self._from_reset = True
        self._fresh = True

    def prepare(self, n: int, chunk_starts: np.ndarray):
        """Upload / allocate everything ``process`` needs for a block of ``n`` samples ahead of time, so the
        launches that follow a long kernel are not preceded by host-side copies.  The chunk starts and the scan
        workspace are kept while the block shape stays the same (a batch of equal captures uploads them once)."""
        starts64 = np.ascontiguousarray(chunk_starts, dtype=np.int64)
        key = (n, len(starts64), hash(starts64.tobytes()))
        if key != self._starts_key:
            self._starts_dev = D.from_numpy(starts64)
            self._work = D.empty(int(N.lib().iqa_scan_workspace_bytes(n)), "uint8")
            self._scratch = D.empty(n, "float32") if self._needs_scratch else None
            self._starts_key = key
        if self._fresh and not self.chunk_sumsq:
            if len(starts64) != self._n_chunks:
                self._alloc_block(len(starts64))  # nothing processed yet: the block is simply re-made at this size
            sumsq = self._sumsq
        else:  # later blocks of a streaming run: their own sums (all read back at the end)
            sumsq = D.zeros(len(starts64) * 8, "float64")  # IQA_SUMSQ_SLOTS sub-slots per chunk
        self._prepared = (n, len(starts64), self._starts_dev, sumsq, self._work, self._scratch)

    def process(self, z_dev, chunk_starts: np.ndarray, out_dev):
        """z_dev -> clipped float32 audio written into ``out_dev`` (len == len(z_dev))."""
        n = int(z_dev.numel())
        if n == 0:
            return
        prep = getattr(self, "_prepared", None)
        if prep is None or prep[0] != n or prep[1] != len(chunk_starts):
            self.prepare(n, chunk_starts)
        _, _, starts_dev, sumsq, work, scratch = self._prepared
        self._prepared = None
        self._fresh = False
        entry = "iqa_demodulate_from_reset" if self._from_reset else "iqa_demodulate"
        self._from_reset = False
        N.call(entry, byref(self.params), N.ptr(z_dev), c_int64(n), N.ptr(self.state_dev), N.ptr(starts_dev),
               c_int64(len(chunk_starts)), N.ptr(self.peak_dev), N.ptr(sumsq), N.ptr(out_dev), N.ptr(scratch), N.ptr(work),
               N.stream_ptr())
        counts = np.diff(np.append(chunk_starts, n))
        self.chunk_sumsq.append((sumsq, counts))
        for entry, core, prev in self._side:
            x = D.empty(n, "float32")
            if entry.source == "theta":
                N.call("iqa_quadrature", N.ptr(z_dev), c_int64(n), N.ptr(prev), N.ptr(x), N.stream_ptr())
            else:
                N.call("iqa_envelope", N.ptr(z_dev), c_int64(n), N.ptr(x), N.stream_ptr())
            core.process(x)

    def side_result(self, name: str, **context):
        """The run's result of side decoder ``name`` (``None`` where it found nothing, or is off); ``context``: what names
        the target in the result (``frequency`` for ais)."""
        core = self.side.get(name)
        return None if core is None else core.result(**context)

    @property
    def peak(self) -> float:
        return 0.0 if self._from_reset else float(self.peak_dev.item())  # (a reset not yet followed by a block)

    def chunk_rms_dbfs(self) -> list[float]:
        out = []
        for sumsq, counts in self.chunk_sumsq:
            for s, c in zip(sumsq.cpu().numpy().reshape(-1, 8).sum(axis=1), counts):
                if c > 0:
                    out.append(20.0 * math.log10(math.sqrt(float(s) / float(c) + 1e-18) + 1e-12))
        return out


class WfmDemod:
    """``ChannelDemod``'s block surface for ``--demod wfm``.

    Per block: the discriminator and ONE launch of the stereo matrix kernel (``iqa_wfm_stereo``) write the mono and
    stereo-difference planes (a, b) into the caller's ``(2, n)`` slice, and the block's per-tile sums of |p|^2 are added to a
    device running sum -- nothing is read back.  ``finish`` reads that sum once, takes the run's stereo decision
    (sqrt(mean |p|^2) >= ``dsp_plan.WFM_STEREO_LEVEL``) and runs the tail on the channels it writes (L, R or a): de-emphasis,
    the writer's pre-clip peak, +-0.99 clip and per-chunk sums of squares, 48 kHz PCM16.

    ``rds=True``: each block's discriminator output also runs through ``iqa_rds_baseband`` and
    ``iqa_rds_clock``; ``finish`` decodes the stored run after the stereo decision (``self.rds``: an ``RdsResult``, or
    ``None`` for a run without a pilot or without an accepted group).  Off, no RDS entry point is called."""

    def __init__(self, fs_channel: float, *, deemph_us: float, rds: bool = False):
        self.decoder = create_decoder("wfm", deemph_us=deemph_us, agc_enabled=False, extensions=True)
        self.decoder.setup(fs_channel)  # (plans the filters; ValueError below the mode's minimum rate)
        self.fs_channel = float(fs_channel)
        self.alpha = self.decoder.deemph["mono"].alpha  # the DeemphasisFilter rule
        self.core = self.decoder.core  # the pipeline's stream: the decoder's own stage API is not used beside it
        self.rds_core = RdsCore(P.plan_rds(fs_channel)) if rds else None
        self.side = {"rds": self.rds_core} if rds else {}
        self.rds = None
        self._prev = D.from_numpy(np.array([1 + 0j], dtype=np.complex64))
        self._pilot_sumsq = D.zeros(1, "float64")
        self._starts: list = []  # chunk starts of the run, channel-rate sample index
        self.n = 0
        self._prepared = None
        self.stereo = None
        self.pilot_level = None
        self.channel_audio = None  # de-emphasised, clipped channel-rate audio (list of device tensors) after finish
        self._peak = 0.0
        self._sumsq = None
        self._counts = None

    def prepare(self, n: int, chunk_starts: np.ndarray) -> None:
        self._prepared = (n, D.empty(n, "float32"), D.empty(max(1, WfmStereoCore.partials_for(n)), "float64"))

    def process(self, z_dev, chunk_starts: np.ndarray, out_dev) -> None:
        """z_dev -> a, b written into ``out_dev`` (shape (2, len(z_dev)))."""
        n = int(z_dev.numel())
        if n == 0:
            return
        if self._prepared is None or self._prepared[0] != n:
            self.prepare(n, chunk_starts)
        _, theta, partials = self._prepared
        self._prepared = None
        N.call("iqa_quadrature", N.ptr(z_dev), c_int64(n), N.ptr(self._prev), N.ptr(theta), N.stream_ptr())
        self.core.process(theta, out_dev[0], out_dev[1], partials=partials)
        if self.rds_core is not None:
            self.rds_core.process(theta)
        self._pilot_sumsq += partials[: WfmStereoCore.partials_for(n)].sum()
        self._starts.append(np.asarray(chunk_starts, dtype=np.int64) + self.n)
        self.n += n

    def finish(self, planes):
        """``planes``: device float32 (2, n), the run's (a, b).  Returns (host int16 PCM at 48 kHz, shape (n48, 2) when stereo
        else (n48,), channel count)."""
        torch = D.torch_mod()
        n = int(planes.shape[1])
        self.pilot_level = math.sqrt(max(float(self._pilot_sumsq.item()), 0.0) / n) if n else 0.0
        self.stereo = bool(self.pilot_level >= P.WFM_STEREO_LEVEL)
        chans = list(stereo_matrix(planes[0], planes[1])) if self.stereo else [planes[0]]
        starts = np.concatenate(self._starts) if self._starts else np.zeros(1, dtype=np.int64)
        starts_dev = D.from_numpy(starts)
        sumsq = D.zeros(len(starts) * 8, "float64")  # IQA_SUMSQ_SLOTS sub-slots per chunk, both channels together
        peak = D.zeros(1, "float32")
        work = D.empty(max(1, int(N.lib().iqa_scan_workspace_bytes(n))), "uint8")
        out = []
        for x in chans:
            y = D.empty(n, "float32")
            if n:
                state = D.zeros(1, "float64")
                N.call("iqa_deemphasis", N.ptr(x), c_int64(n), c_double(self.alpha), N.ptr(state), N.ptr(y), N.ptr(work), N.stream_ptr())
                N.call("iqa_writer_clip", N.ptr(y), c_int64(n), N.ptr(peak), N.ptr(starts_dev), c_int64(len(starts)), N.ptr(sumsq),
                       N.ptr(y), N.stream_ptr())
            out.append(y)
        self.channel_audio = out
        rs = Resampler48k(self.fs_channel)
        pcm = [rs.process(y, want="pcm16") for y in out]
        pcm = torch.stack(pcm, dim=1) if len(pcm) == 2 else pcm[0]  # interleaved L, R
        self._sumsq, self._counts = sumsq, np.diff(np.append(starts, n)) * len(chans)
        self._peak = float(peak.item())
        if self.rds_core is not None and self.stereo:  # (a pilot to lock to)
            self.rds = self.rds_core.result()
        return pcm.cpu().numpy(), len(chans)

    def side_result(self, name: str, **context):
        """``ChannelDemod.side_result`` for the one side decoder of wfm: the ``RdsResult`` that ``finish`` decoded."""
        return self.rds if name == "rds" else None

    @property
    def peak(self) -> float:
        return self._peak

    def chunk_rms_dbfs(self) -> list[float]:
        if self._sumsq is None:
            return []
        out = []
        for s, c in zip(self._sumsq.cpu().numpy().reshape(-1, 8).sum(axis=1), self._counts):
            if c > 0:
                out.append(20.0 * math.log10(math.sqrt(float(s) / float(c) + 1e-18) + 1e-12))
        return out


class Resampler48k:
    """The ``-ar 48000 -acodec pcm_s16le`` leg (reference processing.py:399-418) on the GPU.
    Build-defined specification (dsp_plan.plan_resampler); parity with libswresample is unpinned."""

    _TABLES: dict = {}  # (device, declared input rate) -> the polyphase table on that device (read-only, 12.9 MB at 96 154 Hz)

    def __init__(self, fs_channel: float):
        self.plan = P.plan_resampler(fs_channel)
        key = (D.torch_mod().cuda.current_device(), self.plan.in_rate)
        with _KERNEL_CACHE_LOCK:
            table = self._TABLES.get(key)
        if table is None:
            table = D.from_numpy(self.plan.table.reshape(-1))
            with _KERNEL_CACHE_LOCK:
                if len(self._TABLES) >= 16:
                    self._TABLES.clear()
                self._TABLES[key] = table
        self.table_dev = table

    def process(self, audio_dev, *, want: str = "f32"):
        """48 kHz audio of a whole stream: float32 (``want="f32"``), PCM16 (``"pcm16"``: what the WAV holds, rounded
        from the float32 value in the same pass) or the pair (``"both"``)."""
        if want not in ("f32", "pcm16", "both"):
            raise ValueError(f"want must be 'f32', 'pcm16' or 'both', not {want!r}")
        n_in = int(audio_dev.numel())
        n_out = self.plan.n_out(n_in)
        if self.plan.up == 1 and self.plan.down == 1:
            # a channel rate of exactly 48 kHz: `-ar 48000` on a 48 kHz stream resamples nothing (the build-defined
            # specification says so too: oracle resample_48k) -- the stream itself, and its PCM16
            y = audio_dev.clone() if want != "pcm16" else None
            pcm = self.to_pcm16(audio_dev) if want != "f32" else None
            return y if want == "f32" else pcm if want == "pcm16" else (y, pcm)
        y = D.empty(n_out, "float32") if want != "pcm16" else None
        pcm = D.empty(n_out, "int16") if want != "f32" else None
        if n_out:
            N.call("iqa_resample", N.ptr(audio_dev), c_int64(n_in), N.ptr(self.table_dev), c_int32(self.plan.up),
                   c_int32(self.plan.down), c_int32(self.plan.half_taps), c_int64(0), c_int64(n_out), N.ptr(y), N.ptr(pcm),
                   N.stream_ptr())
        return y if want == "f32" else pcm if want == "pcm16" else (y, pcm)

    @staticmethod
    def to_pcm16(y_dev):
        pcm = D.empty(y_dev.numel(), "int16")
        if y_dev.numel():
            N.call("iqa_float_to_pcm16", N.ptr(y_dev), c_int64(y_dev.numel()), N.ptr(pcm), N.stream_ptr())
        return pcm


class _BlockStager:
    """Capture blocks: memory-mapped file -> one of two pinned host buffers (filled by a helper thread,
    overlapping the previous block's GPU work) -> device tensor by asynchronous H2D copy.
    Replaces the reference's ffmpeg decode pipe + ``IQReader.read_block`` (processing.py:238-266): the
    capture's own sample format goes to the GPU untouched."""

    #: pinned staging buffers that finished runs gave back, by (dtype, elements): pinning 50 MB costs ~15 ms and a run
    #: on a small capture (the reference's --benchmark: 50 MB) spent a third of its wall time on it
    _POOL: dict = {}
    _POOL_MAX_BYTES = 2 << 30
    _POOL_LOCK = threading.Lock()

    def __init__(self, frames: np.ndarray, dtype: str, max_frames: int):
        torch = D.torch_mod()
        self.frames = frames
        self.dtype = getattr(torch, dtype)
        self.numel = 2 * max_frames
        self.bufs = [None, None]  # pinned lazily: a capture of one block needs one
        self.events = [None, None]
        self.pending = None  # (thread, slot, lo, hi)
        self.slot = 0

    def _buf(self, slot: int):
        if self.bufs[slot] is None:
            torch = D.torch_mod()
            key = (str(self.dtype), self.numel)
            with self._POOL_LOCK:
                stack = self._POOL.get(key)
                self.bufs[slot] = stack.pop() if stack else None
            if self.bufs[slot] is None:
                self.bufs[slot] = torch.empty(self.numel, dtype=self.dtype, pin_memory=True)
        return self.bufs[slot]

    def close(self) -> None:
        """Give the pinned buffers back (every H2D copy out of them has completed)."""
        if self.pending is not None:
            self.pending[0].join()
            self.pending = None
        for ev in self.events:
            if ev is not None:
                ev.synchronize()
        key = (str(self.dtype), self.numel)
        with self._POOL_LOCK:
            held = sum(t.numel() * t.element_size() for st in self._POOL.values() for t in st)
            for i, b in enumerate(self.bufs):
                if b is not None and held + b.numel() * b.element_size() <= self._POOL_MAX_BYTES:
                    self._POOL.setdefault(key, []).append(b)
                    held += b.numel() * b.element_size()
                self.bufs[i] = None

    #: helper threads of one block copy (file mapping -> pinned buffer): a single memcpy moves ~2.7 GB/s on the GPU boxes'
    #: hosts, which made the FILE the bottleneck of a file -> WAV run (10 s @ 10 MS/s: 0.148 s, of which ~0.1 s this copy)
    copy_threads = 8

    def _fill(self, slot: int, lo: int, hi: int) -> None:
        import threading

        dst = self._buf(slot).numpy()[: 2 * (hi - lo)]
        src = self.frames[2 * lo : 2 * hi]
        parts = min(int(self.copy_threads), max(1, dst.size // (1 << 22)))  # (NumPy copies release the GIL)
        if parts <= 1:
            np.copyto(dst, src)
            return
        cuts = [dst.size * i // parts for i in range(parts + 1)]
        workers = [threading.Thread(target=np.copyto, args=(dst[a:b], src[a:b]), name="iq-stager-copy", daemon=True)
                   for a, b in zip(cuts[1:-1], cuts[2:])]
        for w in workers:
            w.start()
        np.copyto(dst[: cuts[1]], src[: cuts[1]])
        for w in workers:
            w.join()

    def prefetch(self, lo: int, hi: int) -> None:
        import threading

        slot = self.slot ^ 1
        if self.events[slot] is not None:
            self.events[slot].synchronize()  # the previous H2D out of this buffer must be done
        th = threading.Thread(target=self._fill, args=(slot, lo, hi), name="iq-stager", daemon=True)
        th.start()
        self.pending = (th, slot, lo, hi)

    def fetch(self, lo: int, hi: int):
        torch = D.torch_mod()
        if self.pending is not None and self.pending[2:] == (lo, hi):
            th, slot = self.pending[0], self.pending[1]
            th.join()
        else:
            slot = self.slot ^ 1
            if self.events[slot] is not None:
                self.events[slot].synchronize()
            self._fill(slot, lo, hi)
        self.pending = None
        self.slot = slot
        dev = torch.empty(2 * (hi - lo), dtype=self.dtype, device=D.device())
        dev.copy_(self._buf(slot)[: 2 * (hi - lo)], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[slot] = ev
        return dev


def check_squelch(squelch, demod_mode):
    """``squelch`` (a ``CarrierSquelch`` or None) for a target of ``demod_mode``: ``ValueError`` for a mode that has no
    channel-rate mono audio to gate, or for options the plan refuses."""
    if squelch is None:
        return None
    if not isinstance(squelch, CarrierSquelch):
        raise ValueError("squelch must be a CarrierSquelch or None")
    mode = (demod_mode or "").lower()
    if mode == "wfm" or mode in {"none", "pass", "iq"}:
        raise ValueError(f"squelch cannot gate a '{mode}' target")
    P.plan_gate(96_000.0, squelch)  # (the options' own ranges, at the default channel rate)
    return squelch


class ProcessingPipeline:
    """``ProcessingPipeline(config).run(progress_sink) -> ProcessingResult``, ``.cancel()``
    (reference processing.py:682-1213).

    Differences that are deliberate and documented in DESIGN.md: the capture is memory-mapped
    and streamed to HBM in blocks of whole reference chunks (``block_chunks``); one kernel does
    ingest+mix+filter+decimate; the 48 kHz resample/PCM16 encode runs on the GPU at the end;
    no ffmpeg/ffprobe processes exist.  Per-chunk semantics (AGC restart points, mix-sign
    warm-up window, sample counts) are the reference's.
    """

    #: frames per device block (rounded down to whole chunks); 64 Mi frames = 256 MiB of int16 I/Q
    block_frames_target = 64 * 1024 * 1024

    def __init__(self, config: ProcessingConfig, *, rds: bool = False, pocsag: bool = False, ax25: bool = False, tones: bool = False,
                 acars: bool = False, ais: bool = False, adsb: bool = False, squelch: CarrierSquelch | None = None):
        self.config = config
        flags = dict(rds=rds, pocsag=pocsag, ax25=ax25, tones=tones, acars=acars, ais=ais, adsb=adsb)
        check_modes(flags, [config.demod_mode], plural=False)
        self.squelch = check_squelch(squelch, config.demod_mode)  # --squelch: gate the audio by the channel's power
        self.squelch_result = None  # after run(): the target's GateResult (None with the squelch off)
        self.squelch_paths: list = []  # after run(): the WAV of every transmission (CarrierSquelch.split)
        self.squelch_gate = None  # after run(): the target's CarrierGate (its stages(), for tests)
        self.squelch_audio = None  # after run() with keep_channel_audio: the gated channel-rate audio (device float32)
        self._cancelled = False
        self._resolved_chunk_size: int | None = None
        self.chunk_rms_dbfs: list[float] = []
        self.audio_fs_channel = None  # device float32 tensor of the clipped channel-rate audio (kept for tests)
        self.keep_channel_audio = False
        self.channelizer_kernel = None  # name of the channelizer kernel that produced the last block of the run
        self.f32_integer_path = True  # float32 captures whose values are all k / 32768 run as int16 on the matrix cores
        self.channelizer_precision = None  # "fast" / "fine" / "full" / "float32": what the run's channelizer was planned at
        self.wfm_stereo = None  # --demod wfm: whether the run's output is stereo (the pilot test, once per run)
        self.wfm_planes = None  # --demod wfm with keep_channel_audio: the stereo matrix's (a, b) planes, shape (2, n)
        for e in SIDE_DECODERS:  # --<name>: decode it beside the target (DESIGN.md section e.section)
            setattr(self, e.name + "_enabled", bool(flags[e.name]))
            setattr(self, e.name, None)  # after run(): the target's result (None where it found nothing, or with the decoder off)

    @property
    def side_enabled(self) -> dict:
        """name -> True for the side decoders that are switched on: the keywords of a run with the same ones."""
        return {e.name: True for e in SIDE_DECODERS if getattr(self, e.name + "_enabled")}

    def cancel(self) -> None:
        self._cancelled = True
        if getattr(self, "_multi", None) is not None:
            self._multi.cancel()

    def _is_pass_through_mode(self) -> bool:
        return (self.config.demod_mode or "").lower() in {"none", "pass", "iq"}

    def _effective_chunk_size(self, sample_rate: float) -> int:
        if self._resolved_chunk_size is None:
            self._resolved_chunk_size = tune_chunk_size(sample_rate, self.config.chunk_size)
        return self._resolved_chunk_size

    def _default_output_path(self, info: iqio.CaptureInfo) -> Path:
        ft = int(self.config.target_freq)
        if self._is_pass_through_mode():
            suffix = self.config.in_path.suffix
            if info.container == "wav":
                ext = suffix if suffix.lower() in {".wav", ".wave", ".wv", ".rf64"} else ".wav"
            else:
                ext = suffix or {"pcm_u8": ".cu8", "pcm_s16le": ".cs16", "pcm_f32le": ".cf32"}.get(info.codec, ".raw")
            return self.config.in_path.with_name(f"slice_{ft}{ext}")
        return self.config.in_path.with_name(f"audio_{ft}_48k.wav")

    def run(self, progress_sink: ProgressSink | None = None) -> ProcessingResult:
        """One target frequency: a :class:`MultiChannelPipeline` with a single channel."""
        multi = MultiChannelPipeline([self.config], _owner=self, **self.side_enabled, squelch=self.squelch)
        self._multi = multi
        if self._cancelled:
            multi.cancel()
        return multi.run(progress_sink)[0]


class _Target:
    """Per-target streaming state of a run: channelizer, demodulator, output buffers."""

    def __init__(self, cfg: ProcessingConfig, owner, *, info, sample_rate, center_freq, decimation, fs_channel, total):
        self.cfg, self.owner, self.info = cfg, owner, info
        self.sample_rate, self.decimation, self.fs_channel, self.total = sample_rate, decimation, fs_channel, total
        self.center_freq = center_freq
        self.target_freq = cfg.target_freq if cfg.target_freq > 0 else center_freq
        self.freq_offset = self.target_freq - center_freq
        self.pass_through = (cfg.demod_mode or "").lower() in {"none", "pass", "iq"}
        self.wfm = (cfg.demod_mode or "").lower() == "wfm"
        self.taps = design_channel_filter(sample_rate, cfg.bandwidth, decimation)
        LOG.info("Designed FIR channel filter with %d taps.", len(self.taps))
        if cfg.filter_block <= 0:
            raise ValueError("block_size must be positive")
        enabled = dict(getattr(owner, "side_enabled", {}))  # (read once; the constructors have checked it against the modes)
        rds = enabled.pop("rds", False)  # (WfmDemod's; the others are ChannelDemod's keywords)
        if self.pass_through:
            self.demod = None
        elif self.wfm:
            self.demod = WfmDemod(fs_channel, deemph_us=cfg.deemph_us, rds=rds)
        else:
            self.demod = ChannelDemod(cfg.demod_mode, fs_channel, deemph_us=cfg.deemph_us, agc_enabled=cfg.agc_enabled, **enabled)
        self.stereo = None  # wfm: the run's stereo decision (finish)
        self.side_results = {e.name: None for e in SIDE_DECODERS}  # the target's result per side decoder (finish)
        if cfg.iq_order not in N.ORDER:
            raise ValueError(f"Unsupported iq_order '{cfg.iq_order}'")
        self.chan = None
        self.sign_probe = None
        self.f32_shift = 0  # headroom bits of the int16 planes a float32 capture runs as (set by the run before settle())
        self.mix_sign = 1
        self.pos_dec = 0
        self.peak = 0.0
        self.output_path = cfg.output_path if cfg.output_path else owner._default_output_path(info)
        squelch = getattr(owner, "squelch", None)
        self.gate = None if squelch is None else CarrierGate(P.plan_gate(fs_channel, squelch))
        self.squelch_result = None

    def _channelizer(self, sign: int, exact: bool = False, fmt: str | None = None, precision: str | None = None) -> Channelizer:
        return Channelizer(self.taps, sample_rate=self.sample_rate, freq_offset=self.freq_offset, mix_sign=sign,
                           decimation=self.decimation, fmt=fmt or self.info.fmt, iq_order=self.cfg.iq_order, exact=exact,
                           precision=precision)

    #: Precision guard (see ``pick_precision``); 0 switches it off.
    precision_guard = PRECISION_GUARD

    def _pick_precision(self, probe_power, wideband_rms) -> str:
        """The precision this target's channelizer runs at: "full" for SSB with the AGC on, otherwise "fast" unless the
        precision guard asks for more.  A float32 capture that may run as int16 (``f32_integer_path``) is judged by its
        int16 twin -- that is the kernel its blocks take, on planes with ``f32_shift`` bits of headroom."""
        base = "fast" if self.demod is None else base_precision(self.cfg.demod_mode, self.cfg.agc_enabled)
        fmt, floor_scale = self.info.fmt, 1.0
        if fmt == "f32" and getattr(self.owner, "f32_integer_path", False):
            fmt, floor_scale = "s16", 2.0 ** self.f32_shift
        return pick_precision(lambda name: self._channelizer(self.mix_sign, fmt=fmt, precision=name)._kernel, base,
                              None if self.demod is None else self.cfg.demod_mode, probe_power, wideband_rms, self.precision_guard,
                              floor_scale=floor_scale)

    def begin(self, warm) -> None:
        """Launch the mixer-sign probes (asynchronously) and plan the channelizer for the likely sign meanwhile."""
        if self.cfg.mix_sign_override in (1, -1):
            self.mix_sign = self.cfg.mix_sign_override
            self.chan = self._channelizer(self.mix_sign)
        else:
            self.sign_probe = MixSignProbe(warm, self.sample_rate, self.freq_offset, self.taps, self.decimation,
                                           fmt=self.info.fmt, iq_order=self.cfg.iq_order)
            self.chan = self._channelizer(1)
        self.precision = "fast"

    def settle(self, wideband_rms=None) -> None:
        power = None
        if self.sign_probe is not None:
            self.mix_sign = self.sign_probe.result()
            power = self.sign_probe.power
            self.sign_probe = None
        self.precision = self._pick_precision(power, wideband_rms)
        if self.precision != "fast" and (self.cfg.demod_mode or "").lower() in FM_MODES:
            LOG.info("Channel level %.1f dBFS against a wideband level of %.1f dBFS: '%s' channelizer for this target.",
                     10.0 * math.log10(max(power or 0.0, 1e-30)), 20.0 * math.log10(max(wideband_rms or 0.0, 1e-15)), self.precision)
        self.chan = self._channelizer(self.mix_sign, precision=self.precision)
        self.chan.plan_ahead()
        self.owner.channelizer_precision = self.precision  # (the decision; a float32 capture's int16 twin runs at it)
        LOG.info("Selected mixer sign %d based on warm-up snippet.", self.mix_sign)
        n_dec_total = -(-self.total // self.decimation)
        self.z_all = D.empty(n_dec_total, "complex64") if (self.pass_through or self.cfg.dump_iq_path) else None
        self.audio_all = None
        if self.wfm:  # the (a, b) planes of the stereo matrix
            torch = D.torch_mod()
            self.audio_all = torch.empty((2, n_dec_total), dtype=torch.float32, device=D.device())
        elif not self.pass_through:
            self.audio_all = D.empty(n_dec_total, "float32")

    def before_block(self, done: int, n: int, chunk: int) -> None:
        """Upload what the demodulator needs for the block of ``n`` frames at frame ``done`` ahead of the channelizer."""
        _, n_out = self.chan.outputs_for(n)
        self._starts = None
        if self.demod is not None and n_out:
            self._starts = P.chunk_output_starts(chunk, self.decimation, done, n)
            self.demod.prepare(n_out, self._starts)

    def after_block(self, z, tracker) -> None:
        """The block's decimated stream ``z`` -> dump / slice buffers, demodulator, progress."""
        n_out = int(z.numel())
        tracker.advance("channel", float(n_out))
        if self.z_all is not None and n_out:
            self.z_all[self.pos_dec : self.pos_dec + n_out] = z
            if self.cfg.dump_iq_path:
                tracker.advance("dump_iq", float(n_out))
        if self.demod is not None and n_out:
            self.demod.process(z, self._starts, self.audio_all[..., self.pos_dec : self.pos_dec + n_out])
            if self.gate is not None:
                self.gate.process(z)
        tracker.advance("demod", float(n_out))
        tracker.advance("encode", n_out / max(self.fs_channel, 1e-9) * 48_000.0)
        self.pos_dec += n_out

    def finish(self) -> None:
        cfg, info = self.cfg, self.info
        self.owner.channelizer_kernel = getattr(self, "chan16_kernel", None) or self.chan._kernel.last_kernel
        self.output_path.parent.mkdir(parents=True, exist_ok=True)
        if cfg.dump_iq_path:
            Path(cfg.dump_iq_path).write_bytes(self.z_all[: self.pos_dec].cpu().numpy().astype(np.complex64).tobytes())
        if self.pass_through:
            zs = self.z_all[: self.pos_dec].cpu().numpy()
            self.peak = float(np.max(np.abs(zs))) if zs.size else 0.0
            values = iqio.encode_iq_slice(zs, info.codec, info.container)
            if info.container == "wav":
                iqio.write_wav_iq(self.output_path, values, max(1, int(round(self.fs_channel))), info.fmt)
            else:
                self.output_path.write_bytes(values.tobytes())
            return
        self.demod.decoder.finalize()
        if self.wfm:
            planes = self.audio_all[:, : self.pos_dec]
            pcm, channels = self.demod.finish(planes)
            iqio.write_wav_pcm16(self.output_path, pcm, 48_000, channels=channels)
            self.stereo = self.demod.stereo
            self.owner.wfm_stereo = self.stereo
            self._finish_side()
            if self.owner.keep_channel_audio:
                self.owner.wfm_planes = planes
                self.owner.audio_fs_channel = D.torch_mod().stack(self.demod.channel_audio)  # (channels, n), clipped
            self.peak = self.demod.peak
            self.owner.chunk_rms_dbfs = self.demod.chunk_rms_dbfs()
            LOG.info("Pilot level %.4f: %s output. Audio peak level %.2f dBFS.", self.demod.pilot_level,
                     "stereo" if self.stereo else "mono", 20.0 * math.log10(max(self.peak, 1e-6)))
            return
        audio = self.audio_all[: self.pos_dec]
        if self.owner.keep_channel_audio:
            self.owner.audio_fs_channel = audio
        if self.gate is not None:
            audio = self._squelch(audio)
        rs = Resampler48k(self.fs_channel)
        pcm = rs.process(audio, want="pcm16").cpu().numpy()
        iqio.write_wav_pcm16(self.output_path, pcm, 48_000)
        self.peak = self.demod.peak
        self.owner.chunk_rms_dbfs = self.demod.chunk_rms_dbfs()
        LOG.info("Audio peak level %.2f dBFS.", 20.0 * math.log10(max(self.peak, 1e-6)))
        self._finish_side()

    def _squelch(self, audio):
        """Decide the gate with the whole run in view; the gated audio (a buffer of its own: ``keep_channel_audio``, the side
        decoders, ``peak`` and ``chunk_rms_dbfs`` keep what they read).  With ``split`` every transmission's gated stretch
        goes through a fresh resampler into ``<output stem>.tx0001.wav``, ..."""
        self.gate.finish(self.pos_dec)
        gated = self.gate.apply(audio)
        res = self.squelch_result = self.owner.squelch_result = self.gate.result(frequency=self.target_freq)
        self.owner.squelch_gate = self.gate
        if self.owner.keep_channel_audio:
            self.owner.squelch_audio = gated
        self.owner.squelch_paths = []
        for line in res.lines(f"{self.target_freq:.0f} Hz: "):
            LOG.info("%s", line)
        if self.owner.squelch.split:
            for i, t in enumerate(res.transmissions, 1):
                path = self.output_path.with_name(f"{self.output_path.stem}.tx{i:04d}.wav")
                pcm = Resampler48k(self.fs_channel).process(gated[t.start : t.end], want="pcm16").cpu().numpy()
                iqio.write_wav_pcm16(path, pcm, 48_000)
                self.owner.squelch_paths.append(path)
        return gated

    def _finish_side(self) -> None:
        """The active side decoders' results, in table order: kept per target, handed to the owner, logged."""
        for e in SIDE_DECODERS:
            if e.name in self.demod.side:
                res = self.side_results[e.name] = self.demod.side_result(e.name, frequency=self.target_freq)
                setattr(self.owner, e.name, res)
                if res is not None:
                    LOG.info("%s", e.log(res))


class MultiChannelPipeline:
    """Several target frequencies of ONE capture in a single pass over the file.

    The reference CLI runs a whole pipeline per ``--ft`` target, re-decoding the input each time
    (cli.py:683-710).  Here every block of the capture is staged and uploaded once, and the channels that share a
    decimation are extracted by ONE launch of the channelizer over the HBM-resident block (:class:`ChannelBank`: every
    (channel, tap-row group) is a lane of the ring kernel; BASELINE configs 3/5); each channel keeps exactly the
    per-target semantics of :class:`ProcessingPipeline` (own mixer-sign probe, taps, decoder, output).
    ``configs`` must agree on the input file and its interpretation.
    """

    def __init__(self, configs: list, _owner=None, *, rds: bool = False, pocsag: bool = False, ax25: bool = False, tones: bool = False,
                 acars: bool = False, ais: bool = False, adsb: bool = False, squelch=None):
        if not configs:
            raise ValueError("at least one ProcessingConfig is required")
        if len(configs) > 5 and _owner is None:
            LOG.debug("more than the reference CLI's five targets in one pass (%d)", len(configs))
        first = configs[0]
        for c in configs[1:]:
            same = (c.in_path == first.in_path and c.input_format == first.input_format and c.input_container == first.input_container
                    and c.input_sample_rate == first.input_sample_rate and c.chunk_size == first.chunk_size
                    and c.max_input_seconds == first.max_input_seconds and c.center_freq == first.center_freq)
            if not same:
                raise ValueError("all targets of a multi-channel run must share the input file, format, rate and chunking")
        self.configs = configs
        flags = dict(rds=rds, pocsag=pocsag, ax25=ax25, tones=tones, acars=acars, ais=ais, adsb=adsb)
        check_modes(flags, [c.demod_mode for c in configs], plural=True)
        # squelch: one CarrierSquelch for every target, or a list with one entry (or None) per target
        each = list(squelch) if isinstance(squelch, (list, tuple)) else [squelch] * len(configs)
        if len(each) != len(configs):
            raise ValueError("squelch must name one entry per target")
        for c, sq in zip(configs, each):
            check_squelch(sq, c.demod_mode)
        self.owners = [_owner] if _owner is not None else [ProcessingPipeline(c, **flags, squelch=sq) for c, sq in zip(configs, each)]
        self.squelch_result = None  # after run(): per target, the GateResult (None where the squelch is off)
        self._cancelled = False
        self.wfm_stereo = None  # after run(): per target, the wfm stereo decision (None for the other modes)
        for e in SIDE_DECODERS:  # after run(): per target, the side decoder's result (None where it found nothing, or is off)
            setattr(self, e.name, None)

    def cancel(self) -> None:
        self._cancelled = True

    def run(self, progress_sink: ProgressSink | None = None) -> list:
        cfg = self.configs[0]
        tracker = ProgressTracker(progress_sink)
        targets: list[_Target] = []

        def _request_cancel() -> None:
            self._cancelled = True
            tracker.cancel()
            tracker.status("Cancelling…")

        def _check_cancel(stage: str = "") -> None:
            if self._cancelled or tracker.cancelled or any(o._cancelled for o in self.owners):
                self._cancelled = True
                LOG.info("Processing cancelled during %s.", stage or "run")
                raise ProcessingCancelled("Processing cancelled by user.")

        if progress_sink is not None:
            with contextlib.suppress(AttributeError):
                progress_sink.set_cancel_callback(_request_cancel)

        manual_rate = cfg.input_sample_rate
        if manual_rate is not None and manual_rate <= 0:
            raise ValueError("Input sample rate override must be positive.")
        try:
            info = iqio.probe_capture(cfg.in_path, input_format=cfg.input_format, input_container=cfg.input_container,
                                      input_sample_rate=manual_rate)
            for c in self.configs:
                c.input_container = c.input_container or info.container
                c.input_format = c.input_format or info.codec
            if info.container == "raw" and manual_rate is None:
                raise ValueError("Raw IQ inputs require --input-sample-rate (CLI) or a manual entry in the GUI.")
            if info.sample_rate is None or info.sample_rate <= 0:
                raise RuntimeError("Unable to determine input sample rate automatically. Provide --input-sample-rate.")
            sample_rate = float(info.sample_rate)
            rate_probe = SampleRateProbe(header=None if manual_rate else sample_rate, wave=sample_rate)

            preview_seconds = cfg.max_input_seconds
            if preview_seconds is not None and preview_seconds <= 0:
                preview_seconds = None
            total = info.n_frames
            if preview_seconds is not None:
                total = min(total, max(1, int(math.floor(preview_seconds * sample_rate))))

            for c in self.configs:
                if c.target_freq <= 0 and not c.probe_only:
                    raise ValueError("Target frequency must be positive. Provide --ft or use --interactive.")
                if c.bandwidth <= 0:
                    raise ValueError("Bandwidth must be positive.")
            center_freq = cfg.center_freq
            if center_freq is None:
                center_freq, source = iqio.center_frequency_from_filename(cfg.in_path)
                if center_freq is None:
                    raise ValueError(
                        "Center frequency not supplied and could not be determined from metadata or filename. "
                        "Use --fc to provide it explicitly.")
                for c in self.configs:
                    c.center_freq, c.center_freq_source = center_freq, source
            chunk = tune_chunk_size(sample_rate, cfg.chunk_size)
            for o in self.owners:
                o._resolved_chunk_size = chunk

            n_est = 0.0
            for c, o in zip(self.configs, self.owners):
                decimation, fs_channel = P.choose_decimation(sample_rate, c.fs_ch_target)
                if (c.demod_mode or "").lower() == "wfm" and fs_channel < P.WFM_MIN_RATE:
                    raise ValueError(f"wfm needs a channel rate of at least {P.WFM_MIN_RATE:.0f} Hz; --fs-ch {c.fs_ch_target:.0f} "
                                     f"gives {fs_channel:.0f} Hz")
                LOG.info("Input sample rate %.2f Hz; centre %.0f Hz, target %.0f Hz; decimation %d -> %.2f Hz",
                         sample_rate, center_freq, c.target_freq, decimation, fs_channel)
                n_est += total / max(decimation, 1)
            phases = [PhaseState("ingest", "Ingest IQ", float(total)), PhaseState("channel", "Channelize", n_est),
                      PhaseState("demod", "Demodulate", n_est),
                      PhaseState("encode", "Encode Audio", len(self.configs) * total / sample_rate * 48_000.0)]
            if any(c.dump_iq_path for c in self.configs):
                phases.insert(3, PhaseState("dump_iq", "Write IQ Dump", n_est))
            tracker.start(phases)
            tracker.status("design filter")
            _check_cancel("initialization")
            for c, o in zip(self.configs, self.owners):
                decimation, fs_channel = P.choose_decimation(sample_rate, c.fs_ch_target)
                targets.append(_Target(c, o, info=info, sample_rate=sample_rate, center_freq=center_freq,
                                       decimation=decimation, fs_channel=fs_channel, total=total))
            if total == 0:
                raise RuntimeError("Input stream produced no samples.")

            frames = iqio.map_frames(info)
            np_dt = {"s16": "int16", "u8": "uint8", "f32": "float32"}[info.fmt]
            block = max(1, self.owners[0].block_frames_target // chunk) * chunk
            stager = _BlockStager(frames, np_dt, min(block, total))
            warm = stager.fetch(0, min(chunk, total))
            _check_cancel("warm-up")
            for t in targets:  # all probes are enqueued before the first read-back
                t.begin(warm)
            # wideband level of the warm-up block as a fraction of full scale (for the precision guard): iqa_raw_level, the
            # same estimate the batch runners take (eight stretches spread over the block)
            level = D.zeros(1, "float64")
            queue_raw_level(warm, info.fmt, level)
            wideband_rms = wideband_rms_from(float(level.item()), info.fmt)
            # float32 captures as int16 planes: headroom from the warm-up block's largest value (a later block that exceeds
            # it falls back to the float32 kernel); decided before settle(), whose precision guard scales by it
            shift16 = 0
            if info.fmt == "f32" and self.owners[0].f32_integer_path:
                top = float(warm.view(D.torch_mod().float32).abs().max().item())
                while shift16 < 8 and top * 2.0 ** (15 - shift16) > 32767.0:
                    shift16 += 1
            self.f32_shift = shift16
            for t in targets:
                t.f32_shift = shift16
                t.settle(wideband_rms)
            if cfg.probe_only:
                tracker.advance("ingest", float(warm.numel() // 2))
                return [ProcessingResult(rate_probe, center_freq, t.target_freq, t.freq_offset, t.decimation, t.fs_channel,
                                         t.mix_sign, 0.0) for t in targets]

            # channels that share a decimation share their pass over every block (ChannelBank); built after settle(),
            # which may have replaced a channelizer by the one for the other mixer sign
            banks = []
            for key in sorted({t.decimation for t in targets}):
                members = [t for t in targets if t.decimation == key]  # (a bank runs its "full" / "float32" members one by one)
                banks.append((ChannelBank([t.chan for t in members]), members))
            self.banks = [b for b, _ in banks]
            # float32 captures run on the int16 matrix-core channelizers: each block is split on the device into TWO int16
            # planes, x = 2^shift (hi + lo / 32768) / 32768 exactly to 2^(shift - 31) (iqa_f32_split_s16), and the filter is
            # linear: z = 2^shift (z(hi) + 2^-15 z(lo)), two passes of the int16 channelizers (the second at "fast": its input
            # is 2^-15 of the first's).  A block whose low plane is all zeros (every value k / 32768 at shift 0: what SDR
            # software writes for int16 / 12-bit / int8 ADC samples) needs only the hi pass unless the low plane's history
            # reaches into it (below).  The first block with a value the planes cannot hold (rint(2^(15 - shift) x) outside
            # int16, or a NaN) switches the rest of the run to the float32 kernel, whose state has been carried along.
            banks16 = banks16_lo = None
            if info.fmt == "f32" and self.owners[0].f32_integer_path:
                banks16 = [(ChannelBank([t._channelizer(t.mix_sign, precision=t.precision, fmt="s16") for t in members]), members)
                           for _, members in banks]
                banks16_lo = [(ChannelBank([t._channelizer(t.mix_sign, precision="fast", fmt="s16") for t in members]), members)
                              for _, members in banks]
                flag16 = D.zeros(1, "int32")
                # the low plane's channelizers carry the last L-1 frames of the low plane into the next block: while those
                # may hold a non-zero value, a block whose own low plane is all zeros still has outputs at its head that
                # they reach (2^-15 z(lo) there), so the low plane is processed; frames of all-zero low plane seen since the
                # last block that had one (the history is zero from the start)
                lo_hist_frames = max(len(t.taps) for t in targets) - 1
                lo_quiet = lo_hist_frames
            self.integer_blocks = 0  # blocks of a float32 capture that ran as int16 planes with an all-zero low plane
            self.split_blocks = 0  # blocks of a float32 capture that ran as int16 planes with some lo != 0
            done = 0
            while done < total:
                _check_cancel(f"block at frame {done}")
                hi = min(done + block, total)
                raw = warm if (done == 0 and hi <= warm.numel() // 2) else stager.fetch(done, hi)
                if hi < total:
                    stager.prefetch(hi, min(hi + block, total))  # disk -> pinned memory while the GPU works
                n = hi - done
                tracker.advance("ingest", float(n))
                tracker.status(f"channel @ {done}")
                raw16 = raw16_lo = None
                lo_nonzero = lo_needed = False
                if banks16 is not None:
                    raw16, raw16_lo = D.empty(2 * n, "int16"), D.empty(2 * n, "int16")
                    flag16.zero_()
                    N.call("iqa_f32_split_s16", N.ptr(raw), c_int64(2 * n), c_int32(shift16), N.ptr(raw16), N.ptr(raw16_lo), N.ptr(flag16),
                           N.stream_ptr())
                    bits = int(flag16.item())  # (a host read per 64 Mi-frame block)
                    if bits & 1:
                        LOG.info("float32 capture leaves the range of the int16 planes (shift %d) at frame %d: float32 channelizer.",
                                 shift16, done)
                        banks16 = banks16_lo = raw16 = raw16_lo = None
                    else:
                        lo_nonzero = bool(bits & 2)
                        lo_needed = lo_nonzero or lo_quiet < lo_hist_frames
                for bi, (bank, members) in enumerate(banks):  # one pass over the block per decimation, all its channels at once
                    for t in members:
                        t.before_block(done, n, chunk)
                    if raw16 is not None:
                        zs = banks16[bi][0].process(raw16)
                        if lo_needed:
                            zs_lo = banks16_lo[bi][0].process(raw16_lo)
                            zs = [z.add_(zl, alpha=2.0 ** -15) for z, zl in zip(zs, zs_lo)]
                        else:  # (low plane and its history all zeros: z(lo) = 0, its channelizers' history and position move along)
                            for c in banks16_lo[bi][0].chans:
                                c._advance(raw16_lo, n)
                        if shift16:
                            zs = [z.mul_(2.0 ** shift16) for z in zs]
                        x32, _ = _as_frames(raw, "f32")
                        for c in bank.chans:  # the float32 channelizers' state moves along (history, position)
                            c._advance(x32, n)
                    else:
                        zs = bank.process(raw)
                    for t, z in zip(members, zs):
                        t.after_block(z, tracker)
                if raw16 is not None:
                    self.integer_blocks += 0 if lo_nonzero else 1
                    self.split_blocks += 1 if lo_nonzero else 0
                    lo_quiet = 0 if lo_nonzero else lo_quiet + n
                for bi, (_, members) in enumerate(banks):
                    for ti, t in enumerate(members):  # (for finish(): which kernel produced this target's last block)
                        t.chan16_kernel = banks16[bi][0].chans[ti]._kernel.last_kernel if raw16 is not None else None
                _check_cancel("encode")
                done = hi

            tracker.status("flush outputs")
            for t in targets:
                t.finish()
            self.wfm_stereo = [t.stereo for t in targets]  # per target: True / False for wfm, None for the other modes
            for e in SIDE_DECODERS:
                setattr(self, e.name, [t.side_results[e.name] for t in targets])
            self.squelch_result = [t.squelch_result for t in targets]
            self.output_paths = [t.output_path for t in targets]  # where each target's audio went
            for t in targets:
                t.owner.output_path = t.output_path
            tracker.status("Processing complete")
            return [ProcessingResult(rate_probe, center_freq, t.target_freq, t.freq_offset, t.decimation, t.fs_channel,
                                     t.mix_sign, t.peak) for t in targets]
        except ProcessingCancelled:
            if not cfg.probe_only:
                paths = [t.output_path for t in targets] or [c.output_path for c in self.configs if c.output_path]
                for pth in paths:
                    with contextlib.suppress(OSError):
                        pth.unlink(missing_ok=True)
            raise
        finally:
            if "stager" in locals():
                stager.close()
            tracker.close()
