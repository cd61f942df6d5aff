"""The mixer-sign probe (``choose_mix_sign``, reference processing.py:623-663) and what the precision guard reads with it.

``probe_window`` is the one place the probe's lengths are derived; ``_queue_sign_powers`` the one place a bank of probes is
launched (one target: ``MixSignProbe._probe_pair``; several: ``probe_targets``).
"""
from __future__ import annotations

import math
from ctypes import c_int32, c_int64

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P
from .channelizer import _KERNEL_CACHE_LOCK, ChannelBank, Channelizer, _as_frames

#: iqa_mean_power handles up to this many samples with its single-block, atomics-free kernel
DIRECT_MAX = 65536


def probe_window(n_in: int, ntaps: int, sample_rate: float, decimation: int) -> tuple[int, int, int, int]:
    """(snippet, n_z, discard, keep) of the probe over a warm-up of ``n_in`` >= 1 frames (reference processing.py:636-656,
    as the oracle's ``choose_mix_sign`` restates it): the first ``snippet`` frames are mixed, filtered from zero state and
    decimated to ``n_z`` outputs, of which the first ``discard`` (the filter's transient) stay out of the mean power of the other ``keep``.
    (``discard`` <= n_z // 4 never reaches ``n_z``; the rule for a probe it would empty is kept as the oracle states it.)"""
    snippet = min(n_in, max(int(sample_rate * 0.05), ntaps * 4, 131_072))
    if snippet < ntaps:
        snippet = min(n_in, ntaps * 2)
    n_z = -(-snippet // max(decimation, 1))
    discard = min(ntaps, n_z // 4)
    if n_z - discard == 0:
        discard = 0
    return snippet, n_z, discard, n_z - discard


def _queue_sign_powers(x_all, n_in: int, discard: int, keep: int, sample_rate: float, specs: list, decim: int, fmt: str,
                       iq_order: str, host) -> bool:
    """Queue the probes of ``specs`` (``(freq_offset, taps)`` each) on the current stream: both signs of every target as
    channels of ONE :class:`ChannelBank` over the snippet (shared ingest; lane pairs, tap-row groups and their combine
    launches as for the capture itself) and ONE reduction with a workgroup per channel, which writes the mean powers of
    outputs [discard, discard + keep) into ``host`` (pinned float64: sign +1, sign -1 per target).  False, with nothing
    queued, where that does not apply: float32 captures, a probe too long for the single-workgroup reduction, a ``host``
    too small, outputs that are not interior outputs of kernels with a shared shape (``ChannelBank.run_interior_only``,
    which also refuses fewer than 64 outputs)."""
    if fmt not in ("s16", "u8") or keep > DIRECT_MAX or host.numel() < 2 * len(specs):
        return False
    chans = [Channelizer(taps, sample_rate=sample_rate, freq_offset=f_off, mix_sign=sign, decimation=decim, fmt=fmt, iq_order=iq_order)
             for f_off, taps in specs for sign in (1, -1)]
    z_keep = D.empty(len(chans) * keep, "complex64")
    if not ChannelBank(chans).run_interior_only(x_all, n_in, discard, keep, [z_keep[i * keep : (i + 1) * keep] for i in range(len(chans))]):
        return False
    N.call("iqa_mean_power_batch", N.ptr(z_keep), c_int64(keep), c_int32(len(chans)), c_int64(0), N.ptr(host), N.stream_ptr())
    return True


def probe_targets(warmup, sample_rate: float, specs: list, decimation: int, *, fmt: str, iq_order: str, host) -> list | None:
    """The mixer-sign probes of SEVERAL targets of one capture (``specs``: ``(freq_offset, taps)`` each) in as few launches
    as one bank takes (``_queue_sign_powers``); ``host``: pinned float64, two per target, owned by the caller until the
    probes have been read.  Returns one :class:`MixSignProbe` per target, or None when the grouped path does not apply (the
    caller then probes target by target): float32 captures, targets whose output or discard counts differ, kernels without
    a shared shape."""
    if fmt not in ("s16", "u8") or not specs:
        return None
    x_all, n_in = _as_frames(warmup, fmt)
    if n_in == 0:
        return None
    shapes = {probe_window(n_in, len(taps), sample_rate, decimation)[1:] for _, taps in specs}
    if len(shapes) != 1:
        return None
    _, discard, keep = shapes.pop()
    if not _queue_sign_powers(x_all, n_in, discard, keep, sample_rate, specs, max(decimation, 1), fmt, iq_order, host):
        return None
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


LEVEL_VECTOR_BYTES = 16  # iqa_raw_level reads whole 16-byte vectors from a 16-byte aligned address


def level_window(address: int, n_values: int, value_bytes: int) -> tuple[int, int]:
    """(skip, count): the values of a run of ``n_values`` values of ``value_bytes`` bytes at byte ``address`` that
    ``iqa_raw_level`` is given -- the run from its first 16-byte boundary on (a run that ends before it: nothing).  Of fewer
    values than one vector the library reads nothing, whatever their address, and reports 0."""
    if value_bytes not in (1, 2, 4) or address % value_bytes:
        raise ValueError("raw values must be 1, 2 or 4 bytes wide and aligned to their own size")
    skip = min((-address % LEVEL_VECTOR_BYTES) // value_bytes, max(n_values, 0))
    return skip, max(n_values, 0) - skip


def queue_raw_level(warmup, fmt: str, out_slot) -> None:
    """Queue the wideband-level estimate of raw frames (``iqa_raw_level``: mean square of up to 65536 values spread over
    ``warmup``) into ``out_slot`` (double[1], device or pinned host memory) on the current stream.  ``warmup`` may start
    anywhere (a capture behind a lead-in of a few frames): the estimate is taken from its first 16-byte boundary on
    (``level_window``), at most 15 bytes of a block of a hundred thousand frames and more."""
    x, n = _as_frames(warmup, fmt)
    flat = x.view(D.torch_mod().float32) if x.is_complex() else x
    skip, count = level_window(int(flat.data_ptr()), int(flat.numel()), int(flat.element_size()))
    N.call("iqa_raw_level", c_int32(P.FMT_CODE[fmt]), N.ptr(flat[skip:] if skip else flat), c_int64(count), N.ptr(out_slot), N.stream_ptr())


def wideband_rms_from(mean_square: float, fmt: str) -> float:
    """RMS of the complex samples (fraction of full scale) from the mean square of the raw values."""
    return math.sqrt(max(2.0 * float(mean_square), 0.0)) * P.INGEST_SCALE[fmt]


class MixSignProbe:
    """``choose_mix_sign`` split into an asynchronous launch and a blocking ``result()``, so the
    caller can plan the channelizer while the two probes run."""

    DIRECT_MAX = DIRECT_MAX

    def __init__(self, warmup, sample_rate: float, freq_offset: float, taps: np.ndarray, decimation: int, *,
                 fmt: str = "f32", iq_order: str = "iq", record_done: bool = True, measure_level: bool = False, _queued=None):
        """``record_done=False``: the caller sets ``_done`` to event(s) of its own that lie behind both probes (an
        event record between two kernels of a stream costs ~7 us on this part).  ``measure_level``: also estimate the
        wideband level of ``warmup`` (``wideband_rms`` after ``result()`` / ``peek()``: what the precision guard compares
        ``power`` with).  ``_queued``: see ``from_powers``."""
        self.power = None  # mean |z|^2 of the chosen sign's probe
        self.wideband_rms = None
        self._fmt = fmt
        self._sign = None
        self._valid = [False, False]
        self._host = None  # pinned float64: [power(+1), power(-1), ...]; None before anything is queued and once it has been read
        self._level = None  # host view (float64[1]) of the pinned slot the raw level is written into (None: not measured)
        self._done = None  # event(s) behind the probes
        if _queued is not None:
            self._host, self._done, level_slot = _queued
            self._level = None if level_slot is None else level_slot.numpy()
            self._valid = [True, True]
            return
        x_all, n_in = _as_frames(warmup, fmt)
        if n_in == 0:
            return
        window = probe_window(n_in, len(taps), sample_rate, decimation)
        decim = max(decimation, 1)
        self._host = _pinned_scalars(id(self))
        if not self._probe_pair(x_all, n_in, window, taps, sample_rate, freq_offset, decim, fmt, iq_order):
            for i, sign in enumerate((1, -1)):
                self._probe_one(i, sign, x_all, n_in, window, taps, sample_rate, freq_offset, decim, fmt, iq_order)
        if measure_level:
            queue_raw_level(warmup, fmt, self._host[2:3])
            self._level = self._host.numpy()[2:3]
        if record_done:
            self._done = D.torch_mod().cuda.Event()
            self._done.record()

    @classmethod
    def from_powers(cls, host_pair, done_event, level_slot=None, fmt: str = "s16"):
        """A probe whose two mean powers (sign +1, sign -1) are being written into ``host_pair`` (a pinned float64[2] the
        caller owns) by launches already queued; ``done_event`` lies behind them, and behind the raw level's launch into
        ``level_slot`` where there is one.  See ``probe_targets``."""
        return cls(None, 0.0, 0.0, (), 1, fmt=fmt, _queued=(host_pair, done_event, level_slot))

    def _probe_pair(self, x_all, n_in, window, taps, sample_rate, freq_offset, decim, fmt, iq_order) -> bool:
        """Both signs in two launches instead of four: ``_queue_sign_powers`` for this one target, into the pinned slot.
        False (nothing queued) where it does not apply."""
        _, _, discard, keep = window
        if not _queue_sign_powers(x_all, n_in, discard, keep, sample_rate, [(freq_offset, taps)], decim, fmt, iq_order, self._host):
            return False
        self._valid = [True, True]
        return True

    def _probe_one(self, i, sign, x_all, n_in, window, taps, sample_rate, freq_offset, decim, fmt, iq_order):
        """Queue the probe for one mixer sign on the current stream; its mean power ends up in ``_host[i]``."""
        snippet, _, discard, keep = window
        ch = Channelizer(taps, sample_rate=sample_rate, freq_offset=freq_offset, mix_sign=sign, decimation=decim,
                         fmt=fmt, iq_order=iq_order)
        # Only z[discard:] enters the power (processing.py:651-656), and those outputs see neither the zero
        # initial state nor anything past the snippet: when the warm-up buffer is longer than the snippet they are
        # all interior outputs of the matrix-core kernel -- one launch per sign instead of three.
        z, skip = D.empty(keep, "complex64"), 0
        if not (fmt in ("s16", "u8") and ch._kernel.run_interior_only(x_all, n_in, discard, keep, z)):
            # the whole snippet from zero state: n_z outputs (Channelizer.outputs_for at position 0), the first ``discard`` skipped
            z, skip = ch.process(x_all[:snippet] if x_all.is_complex() else x_all[: 2 * snippet], last_block=True), discard
        slot = self._host[i : i + 1]
        if keep <= DIRECT_MAX:
            # a short reduction is one block that WRITES its result: straight into the mapped pinned slot, no
            # device scalar and no copy behind it (a blit between kernels costs ~13 us of a 0.9 ms capture)
            _mean_power_into(z, skip, slot)
        else:
            power = D.empty(1, "float64")  # iqa_mean_power overwrites its slot
            _mean_power_into(z, skip, power)
            slot.copy_(power, non_blocking=True)
        self._valid[i] = True

    def result(self) -> int:
        if self._sign is None:
            if self._host is None:  # (an empty warm-up: nothing was probed)
                return 1
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
        self.power = best_power if np.isfinite(best_power) else None
        if self._level is not None:
            self.wideband_rms = wideband_rms_from(float(self._level[0]), self._fmt)
        return best_sign

    def peek(self) -> int:
        """The sign the two powers in the pinned slot say NOW, without giving the slot back: for probes that live inside
        a captured graph (every replay writes the same slot again; the caller has waited for the replay)."""
        return 1 if self._host is None else self._decide()

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
