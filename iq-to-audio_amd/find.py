"""The occupied channels of a capture (``--find-channels``): from a wideband capture to the list of
frequencies worth an ``--ft``.

One pass over the capture: ``iqa_psd_frames`` turns the raw frames into float32 dB rows (Hann window, nfft / 2 hop) and
``iqa_find_accumulate`` quantises them to centi-dB and adds them into three integer planes -- the sum and the maximum of
every bin, and the sum of every bin over each of at most 256 time slices.  Once per run ``iqa_find_mean``,
``iqa_find_floor`` (the lower quartile of the +-500 kHz around each bin, of the mean and of the maximum), ``iqa_find_mask``
(bins over their floor, small gaps closed), ``iqa_find_runs`` (one record per stretch of closed bins) and
``iqa_find_activity`` (which slices each run is on in) turn the planes into the channel list.  Behind the quantiser
everything is integer; the floats of a ``FoundChannel`` are formed on the host from those integers.

The finder takes the spectrum as the stated I/Q order gives it: it does not probe the mixer sign, so a capture whose I/Q
order is stated wrongly comes back mirrored about the centre.  No CPU path: without a GPU or the built library the calls
raise ``RuntimeError``."""
from __future__ import annotations

import logging
import math
from ctypes import c_int32, c_int64
from dataclasses import asdict, dataclass, field
from pathlib import Path

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P
from . import iqio
from .decoders.common import search_with_room
from .find_layers import ALL_LAYERS, active_layers

LOG = logging.getLogger(__name__)

RECORD = 8  # int64 values of one run's record: lo, hi, hot, peak, e_peak, sum w, sum w (k - lo), max (max - fmax)
BLOCK_FRAMES = 1 << 22  # capture frames handed to ``process`` at a time by ``find_channels``
_RAW_DTYPE = {"s16": "int16", "u8": "uint8", "f32": "float32"}


@dataclass
class FoundChannel:
    offset_hz: float  # the centroid of the run, weighted by the dB over the floor, against the capture's centre
    freq_hz: float | None  # centre + offset; None without a centre frequency
    width_hz: float  # the run's bins
    snr_db: float  # the mean spectrum over its local floor at the run's peak
    peak_db: float  # the largest max-hold value over the floor of the max-hold spectrum
    level_db: float  # the mean spectrum at the peak (dB, as the PSD rows scale it)
    duty: float  # the share of the capture's frames that lie in slices where the run is on
    first_s: float | None  # the start of the first slice it is on in; None where it is on in none
    last_s: float | None  # the end of the last one
    bursts: int  # off -> on edges
    lo_bin: int
    hi_bin: int

    def line(self) -> str:
        head = f"{self.offset_hz:+.0f} Hz" if self.freq_hz is None else f"{self.freq_hz:.0f} Hz"
        when = "" if self.first_s is None else f" ({self.first_s:.2f} .. {self.last_s:.2f} s)"
        return f"{head}: {self.width_hz:.0f} Hz wide, {self.snr_db:.1f} dB over the floor, on {100.0 * self.duty:.0f} %{when}"

    def to_json(self) -> dict:
        return asdict(self)


@dataclass
class FindResult:
    channels: list = field(default_factory=list)  # FoundChannel, ascending in offset
    sample_rate: float = 0.0
    center_freq: float | None = None
    seconds: float = 0.0  # the capture's length
    nfft: int = 0
    bin_hz: float = 0.0
    frames: int = 0
    slice_frames: int = 0
    slices: int = 0
    threshold_db: float = 0.0
    peak_threshold_db: float = 0.0
    candidates: int = 0  # every run of closed bins, the dropped ones included

    def line(self) -> str:
        if not self.channels:
            return "no channel found"
        return f"{len(self.channels)} channel(s) in {self.seconds:.2f} s at {self.sample_rate:.0f} S/s, {self.bin_hz:.1f} Hz bins"

    def lines(self) -> list:
        return [ch.line() for ch in self.channels] or ["no channel found"]

    def to_json(self) -> dict:
        return asdict(self)

    @classmethod
    def from_json(cls, data: dict) -> "FindResult":
        data = dict(data)
        data["channels"] = [FoundChannel(**ch) for ch in data.get("channels", [])]
        return cls(**data)


def channels_from_records(plan: P.FindPlan, records, on, mean, center_freq: float | None = None) -> list:
    """The kept runs' records (int64[J][8]), their activity (uint8[J][S]) and the mean plane -> ``FoundChannel``s in ascending
    offset.  Plain numpy: float64 from the integers.  A run without any weight (kept by the max-hold term alone) takes its
    middle as the centroid."""
    records = np.asarray(records, dtype=np.int64).reshape(-1, RECORD)
    on = np.asarray(on, dtype=np.uint8).reshape(records.shape[0], plan.slices)
    lens = [plan.slice_len(s) for s in range(plan.slices)]
    out = []
    for (lo, hi, _hot, peak, e_peak, sw, swk, over), row in zip(records.tolist(), on):
        centroid = lo + (swk / sw if sw > 0 else (hi - lo) / 2.0)
        offset = (centroid - plan.dc_bin) * plan.bin_hz
        idx = np.flatnonzero(row)
        first = last = None
        if idx.size:
            first = int(idx[0]) * plan.slice_frames * plan.hop / plan.fs
            last = min((int(idx[-1]) + 1) * plan.slice_frames, plan.frames) * plan.hop / plan.fs
        edges = int(np.count_nonzero(np.diff(np.concatenate(([0], row.astype(np.int64)))) == 1))
        out.append(FoundChannel(offset_hz=offset, freq_hz=None if center_freq is None else center_freq + offset,
                                width_hz=(hi - lo + 1) * plan.bin_hz, snr_db=e_peak / 100.0, peak_db=over / 100.0,
                                level_db=int(mean[peak]) / 100.0, duty=sum(lens[s] for s in idx.tolist()) / plan.frames,
                                first_s=first, last_s=last, bursts=edges, lo_bin=lo, hi_bin=hi))
    out.sort(key=lambda ch: ch.offset_hz)
    return out


def select_targets(result: FindResult, top: int, grid_hz: float = 1.0) -> list:
    """The ``top`` channels of highest ``snr_db`` (ties to the lower frequency) as ``--ft`` targets: each rounded to the
    nearest multiple of ``grid_hz`` (halves upwards), duplicates dropped, ascending.  Needs a centre frequency."""
    if any(ch.freq_hz is None for ch in result.channels):
        raise ValueError("the targets need a centre frequency")
    best = sorted(result.channels, key=lambda ch: (-ch.snr_db, ch.freq_hz))[: max(int(top), 0)]
    grid = float(grid_hz)
    return sorted({math.floor(ch.freq_hz / grid + 0.5) * grid for ch in best})


class ChannelFinder:
    """The stage API: ``process(raw_block)`` per block of the capture (device tensor or numpy array of interleaved I/Q values in
    the capture's own format, any length: the tail that fills no frame yet is carried), ``finish()`` once (the stage arrays),
    ``result()`` (a ``FindResult``), ``stages()`` for the tests, ``reset()``."""

    def __init__(self, plan: P.FindPlan, fmt: str = "s16", iq_order: str = "iq", *, keep_stages: bool = False):
        if fmt not in _RAW_DTYPE:
            raise ValueError(f"Unsupported sample format '{fmt}'")
        if iq_order not in N.ORDER:
            raise ValueError(f"Unsupported iq_order '{iq_order}'")
        self.plan, self.fmt, self.iq_order, self._keep = plan, fmt, iq_order, keep_stages
        self._eng = None
        self.reset()

    def reset(self) -> None:
        """Back to a run that has seen nothing."""
        self._sum = self._max = self._slice = None
        self._pending = None  # device, raw values: the tail of the stream that has not filled a frame yet
        self.frames_done = 0
        self.samples_seen = 0
        self._c: list = []  # with keep_stages: the int16 c of every batch
        self._rows: list = []  # ... and its float32 rows
        self._fin = None

    def _start(self) -> None:
        from .spectrum import _PsdEngine

        p = self.plan
        if self._eng is None:
            self._eng = _PsdEngine(sample_rate=p.fs, nfft=p.nfft, fmt=self.fmt, iq_order=self.iq_order)
            assert self._eng.scale == p.scale
        self._sum = D.zeros(p.nfft, "int64")
        self._max = D.torch_mod().full((p.nfft,), P.FIND_C_MIN, dtype=D.torch_mod().int32, device=D.device())
        self._slice = D.zeros(p.slices * p.nfft, "int32")

    def process(self, raw_block) -> None:
        from .spectrum import BATCH_FRAMES

        p = self.plan
        x = D.to_device(raw_block, _RAW_DTYPE[self.fmt]).reshape(-1)
        if int(x.numel()) % 2:
            raise ValueError("a block holds whole I/Q frames: an even number of values")
        if int(x.numel()) == 0:
            return
        self.samples_seen += int(x.numel()) // 2
        if self.samples_seen > p.n_samples:
            raise ValueError(f"the plan was made for {p.n_samples} samples and the stream is longer")
        if self._sum is None:
            self._start()
        self._fin = None
        if self._pending is not None and int(self._pending.numel()):
            x = D.torch_mod().cat((self._pending, x))
        total = int(x.numel()) // 2
        if total < p.nfft:
            self._pending = x.clone()
            return
        n_win = (total - p.nfft) // p.hop + 1
        done = 0
        while done < n_win:
            k = min(BATCH_FRAMES, n_win - done)
            _, rows = self._eng.frames(x, total, done * p.hop, p.hop, k, want_f64=False, want_f32=True)
            c = D.empty(k * p.nfft, "int16") if self._keep else None
            N.call("iqa_find_accumulate", N.ptr(rows), c_int32(k), c_int32(p.nfft), c_int64(self.frames_done), c_int32(p.slice_frames),
                   c_int32(p.slices), N.ptr(self._sum), N.ptr(self._max), N.ptr(self._slice), N.ptr(c), N.stream_ptr())
            if self._keep:
                self._c.append(c)
                self._rows.append(rows)
            done += k
            self.frames_done += k
        self._pending = x[2 * n_win * p.hop :].clone()

    def _runs(self, capacity: int, counts, planes):
        lst = D.empty(RECORD * capacity, "int64")
        mean, fmean, fmax, mask = planes
        N.call("iqa_find_runs", N.ptr(mean), N.ptr(fmean), N.ptr(self._max), N.ptr(fmax), N.ptr(mask), c_int32(self.plan.nfft),
               c_int32(self.plan.min_hot), N.ptr(lst), c_int64(capacity), N.ptr(counts), N.stream_ptr())
        return lst

    def finish(self, capacity: int = 256) -> dict:
        """The stage arrays of the finished run as numpy arrays: sum, max, slice [S][nbins], mean, fmean, fmax, x, mask, runs (the
        kept records, int64[J][8], ascending in lo), candidates (every run) and on (uint8[J][S]).  A list too short for the
        kept runs is never used: the search is repeated with room for all of them."""
        p = self.plan
        if self.frames_done != p.frames:
            raise ValueError(f"the plan was made for {p.frames} frames and the stream held {self.frames_done}")
        if self._fin is not None:
            return self._fin
        capacity = max(int(capacity), 1)
        nb = c_int32(p.nfft)
        mean, fmean, fmax, x = (D.empty(p.nfft, "int32") for _ in range(4))
        mask = D.empty(p.nfft, "uint8")
        N.call("iqa_find_mean", N.ptr(self._sum), nb, c_int64(p.frames), N.ptr(mean), N.stream_ptr())
        for plane, out in ((mean, fmean), (self._max, fmax)):
            N.call("iqa_find_floor", N.ptr(plane), nb, c_int32(p.half), c_int32(p.num), c_int32(p.den), N.ptr(out), N.stream_ptr())
        N.call("iqa_find_mask", N.ptr(mean), N.ptr(fmean), N.ptr(self._max), N.ptr(fmax), nb, c_int32(p.thr), c_int32(p.thr_peak),
               c_int32(p.gap), c_int32(p.dc_bin), c_int32(p.dc_guard), N.ptr(x), N.ptr(mask), N.stream_ptr())
        counts = D.zeros(2, "int64")
        (lst,), (kept, total) = search_with_room([lambda room: self._runs(room, counts, (mean, fmean, fmax, mask))], counts, capacity)
        on = D.empty(kept * p.slices, "uint8")
        N.call("iqa_find_activity", N.ptr(self._slice), N.ptr(fmean), N.ptr(lst), c_int64(kept), nb, c_int64(p.frames),
               c_int32(p.slice_frames), c_int32(p.slices), c_int32(p.thr_act), N.ptr(on), N.stream_ptr())
        records = lst[: RECORD * kept].cpu().numpy().reshape(-1, RECORD)
        order = np.argsort(records[:, 0], kind="stable")
        host = lambda t: t.cpu().numpy()  # noqa: E731
        self._fin = dict(sum=host(self._sum), max=host(self._max), slice=host(self._slice).reshape(p.slices, p.nfft), mean=host(mean),
                         fmean=host(fmean), fmax=host(fmax), x=host(x), mask=host(mask), runs=records[order], candidates=total,
                         on=host(on).reshape(kept, p.slices)[order])
        return self._fin

    def result(self, center_freq: float | None = None, fin: dict | None = None) -> FindResult:
        fin = self.finish() if fin is None else fin
        p = self.plan
        return FindResult(channels=channels_from_records(p, fin["runs"], fin["on"], fin["mean"], center_freq), sample_rate=p.fs,
                          center_freq=center_freq, seconds=p.n_samples / p.fs, nfft=p.nfft, bin_hz=p.bin_hz, frames=p.frames,
                          slice_frames=p.slice_frames, slices=p.slices, threshold_db=p.threshold_db,
                          peak_threshold_db=p.peak_threshold_db, candidates=int(fin["candidates"]))

    def stages(self, capacity: int = 256) -> dict:
        """``finish()`` and, with ``keep_stages``, ``rows`` (float32[F][nbins]) and ``c`` (int16[F][nbins]) of every frame."""
        out = dict(self.finish(capacity))
        if self._keep:
            torch = D.torch_mod()
            out["rows"] = torch.cat(self._rows).cpu().numpy().reshape(-1, self.plan.nfft)
            out["c"] = torch.cat(self._c).cpu().numpy().reshape(-1, self.plan.nfft)
        return out


def find_channels(path, *, center_freq: float | None = None, input_format: str | None = None, input_container: str | None = None,
                  input_sample_rate: float | None = None, iq_order: str = "iq", max_seconds: float | None = None,
                  fs_ch: float | None = None, **options):
    """The occupied channels of the capture at ``path``.  The centre frequency is taken from the file name where it is not
    given; without one the channels carry offsets only.  ``options``: the keywords of ``dsp_plan.plan_find`` and the layers of a
    second pass over the mapped file (``find_layers.ALL_LAYERS``: the chain, each with the one in front of it, then the
    branches): ``describe=True`` measures
    every channel (``describe.ChannelDescriber``), ``keying=True`` also its keying and its side decoders
    (section 23; ``fs_ch``: an explicit channel rate of the targets that follow), ``identify=True`` searches the keyed channels of
    the usual digital rates for their frame synchronisation words (section 25), ``flex=True`` decodes the pages of the FLEX
    channels among them (section 26); ``dmr=True`` (``find_layers.FIND_BRANCHES``: with ``identify=True``, and without ``flex``
    if so wished) decodes the data bursts of the channels that carry DMR sync words (section 29), ``p25=True`` likewise the
    NIDs, link control and TSBKs of those that carry P25 frame sync words (section 31), ``ysf=True`` the FICH and the callsigns
    of those that carry YSF frame sync words (section 32), ``nxdn=True`` the LICH, the calls and the control messages of those
    that carry NXDN frame sync words at either symbol rate (section 34).  Returns the ``FindResult``
    alone without a layer, else a tuple of it and every layer's result in that order: ``DescribeResult``, ``KeyingResult``,
    ``ProtocolResult``, ``FlexResult``, ``DmrResult``, ``P25Result``, ``YsfResult``, ``NxdnResult``."""
    layers = active_layers({layer.name: options.pop(layer.name, False) for layer in ALL_LAYERS})
    path = Path(path)
    info = iqio.probe_capture(path, input_format=input_format, input_container=input_container, input_sample_rate=input_sample_rate)
    if not info.sample_rate:
        raise ValueError(f"{path}: the sample rate is unknown; pass input_sample_rate")
    n = info.n_frames
    if max_seconds is not None:
        n = min(n, int(float(max_seconds) * info.sample_rate))
    if center_freq is None:
        center_freq, _ = iqio.center_frequency_from_filename(path)
    plan = P.plan_find(info.sample_rate, n, **options)
    LOG.info("Finding channels: %d frames of %d bins (%.1f Hz), %d slices of %d frames.", plan.frames, plan.nfft, plan.bin_hz,
             plan.slices, plan.slice_frames)
    values = iqio.map_frames(info)

    def blocks():
        for a in range(0, n, BLOCK_FRAMES):
            yield np.ascontiguousarray(values[2 * a : 2 * min(n, a + BLOCK_FRAMES)])

    finder = ChannelFinder(plan, info.fmt, iq_order)
    for block in blocks():
        finder.process(block)
    result = finder.result(center_freq)
    if not layers:
        return result
    from .describe import ChannelDescriber

    describer = ChannelDescriber(plan, finder.finish(), result.channels, info.fmt, iq_order, **{layer.name: True for layer in layers[1:]})
    for block in blocks():
        describer.process(block)
    return (result, *(layer.result(describer, center_freq, fs_ch) for layer in layers))
