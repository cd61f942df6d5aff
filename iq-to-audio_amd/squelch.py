"""Audio post-processing (automatic squelch) on the GPU -- the reference's ``squelch.py`` and ``--audio-post``.

Same public surface as the reference (``SquelchConfig``, ``AudioPostOptions``, ``SquelchFileResult``,
``SquelchSummary``, ``apply_squelch``, ``gather_audio_targets``, ``process_audio_file``, ``process_audio_batch``);
every per-sample operation runs in ``csrc/squelch.hip`` (``iqa_squelch``).  A batch of files is one segmented launch
sequence; the only read-back is the per-file result (floor, threshold, trim bounds).  The reference's dilation
accumulates window counts in int8 and wraps; that is reproduced.

WAV only: ``.flac`` / ``.ogg`` / ``.mp3`` are gathered like the reference gathers them, then fail per file with a
"needs libsndfile" error in ``summary.errors``.
"""
from __future__ import annotations

import ctypes
import logging
from collections.abc import Callable, Iterable, Sequence
from dataclasses import dataclass
from pathlib import Path
from typing import Literal

import numpy as np

from . import _native as N
from . import iqio

SquelchMethod = Literal["adaptive", "static", "transient"]

LOG = logging.getLogger(__name__)

# device bytes a batch may take (input + output + workspace); one 60-s 48 kHz stereo file needs ~180 MB
BATCH_BYTES = 2 << 30
_WS_BYTES_PER_SAMPLE = 46


@dataclass(slots=True)
class SquelchConfig:
    method: SquelchMethod = "adaptive"
    auto_noise_floor: bool = True
    manual_noise_floor_db: float | None = None
    noise_floor_percentile: float = 0.2
    threshold_margin_db: float = 6.0
    window_seconds: float = 0.04
    transient_window_seconds: float = 0.012
    transient_margin_db: float = 8.0
    hold_seconds: float = 0.12
    fade_seconds: float = 0.01
    trim_silence: bool = True
    trim_lead_seconds: float = 0.15
    trim_trail_seconds: float = 0.35

    def validate(self) -> None:
        """The reference's configuration errors (raised from resolve_noise_floor / apply_squelch there)."""
        if not self.auto_noise_floor and self.manual_noise_floor_db is None:
            raise ValueError("manual_noise_floor_db must be provided when auto_noise_floor=False.")
        if self.method not in N.SQ_METHOD:
            raise ValueError(f"Unsupported squelch method: {self.method}")


@dataclass(slots=True)
class AudioPostOptions:
    config: SquelchConfig
    overwrite: bool = False
    cleaned_suffix: str = "-cleaned"
    allowed_suffixes: Sequence[str] = (".wav", ".flac", ".ogg", ".mp3")


@dataclass(slots=True)
class SquelchFileResult:
    input_path: Path
    output_path: Path
    samples_in: int
    samples_out: int
    duration_in: float
    duration_out: float
    bytes_in: int
    bytes_out: int
    noise_floor_db: float
    threshold_db: float
    method: SquelchMethod
    retained_ratio: float


@dataclass(slots=True)
class SquelchSummary:
    results: list[SquelchFileResult]
    errors: list[tuple[Path, Exception]]

    @property
    def processed(self) -> int:
        return len(self.results)

    @property
    def failed(self) -> int:
        return len(self.errors)

    @property
    def total(self) -> int:
        return self.processed + self.failed

    def aggregate_duration_delta(self) -> float:
        return float(sum(item.duration_out - item.duration_in for item in self.results))

    def aggregate_size_delta(self) -> int:
        return int(sum(item.bytes_out - item.bytes_in for item in self.results))


# ---------------------------------------------------------------------------------------------------------------
# host-side planning (sizes and percentile ranks: integers and numpy's own float32 index arithmetic)


def percentile_plan(n: int, pct: float) -> tuple[int, int, np.float32]:
    """np.percentile(float32[n], pct) (method "linear", numpy 2.2) as (previous index, next index, gamma): the
    result is numpy's float32 ``_lerp(sorted[prev], sorted[next], gamma)``."""
    q = np.asanyarray(np.true_divide(pct, np.float32(100)))
    virtual = np.asanyarray((n - 1) * q)
    prev = np.floor(virtual)
    if virtual >= n - 1:
        prev_i = next_i = n - 1
        prev_ref = -1
    elif virtual < 0:
        prev_i = next_i = prev_ref = 0
    else:
        prev_i = prev_ref = int(prev)
        next_i = prev_i + 1
    gamma = np.asanyarray(virtual - np.intp(prev_ref), dtype=virtual.dtype)
    return prev_i, next_i, np.float32(gamma)


def _windows(n: int, sample_rate: float, config: SquelchConfig) -> dict:
    """Sample counts, as the reference rounds them (apply_squelch, _transient_mask, _apply_trim)."""
    window = max(1, int(round(config.window_seconds * sample_rate)))
    short = max(1, int(round(config.transient_window_seconds * sample_rate)))
    long_ = max(short * 4, window)
    need = max(window, long_) if config.method == "transient" else window
    if n < need:
        # the reference fails here too (np.convolve swaps its operands and the shapes no longer broadcast)
        raise ValueError(f"audio of {n} samples is shorter than the {need}-sample squelch window")
    return dict(window=window, short_window=short, long_window=long_,
                hold=int(round(sample_rate * config.hold_seconds)), fade=max(0, int(round(sample_rate * config.fade_seconds))),
                lead=int(max(0, round(sample_rate * config.trim_lead_seconds))),
                trail=int(max(0, round(sample_rate * config.trim_trail_seconds))))


def _segment(n: int, channels: int, sample_rate: float, config: SquelchConfig, in_off: int, base: int) -> N.SquelchSeg:
    w = _windows(n, sample_rate, config)
    seg = N.SquelchSeg(n=n, in_off=in_off, base=base, channels=channels, **w)
    seg.manual_floor_db = float(config.manual_noise_floor_db) if not config.auto_noise_floor else 0.0
    pct = float(np.clip(config.noise_floor_percentile, 0.0, 1.0)) * 100.0
    for k, p in enumerate((pct, 0.05 * 100.0, 0.95 * 100.0)):
        lo, hi, g = percentile_plan(n, p)
        seg.q_index[2 * k], seg.q_index[2 * k + 1], seg.q_gamma[k] = lo, hi, float(g)
    return seg


def _pcm16_bytes(n_frames: int, channels: int) -> int:
    return n_frames * channels * 2


def batch_bytes(n_frames: int, channels: int) -> int:
    """Device bytes one file takes in a batch (input, output, workspace)."""
    padded = -(-n_frames // N.SQ_TILE) * N.SQ_TILE
    return 8 * n_frames * channels + _WS_BYTES_PER_SAMPLE * padded + 4096


def _ensure_2d(samples):
    if samples.ndim == 1:
        return samples.reshape(-1, 1)
    if samples.ndim != 2:
        raise ValueError(f"Expected mono/stereo audio, received shape {tuple(samples.shape)!r}.")
    return samples


# ---------------------------------------------------------------------------------------------------------------
# the device chain


@dataclass
class _DeviceResult:
    samples: object  # device tensor [n_out, C] (float32 or int16)
    noise_floor_db: float
    threshold_db: float
    start: int
    stop: int
    stages: dict | None


def squelch_device(items: Sequence[tuple[object, float]], config: SquelchConfig, *, pcm16: bool = False,
                   return_stages: bool = False) -> list[_DeviceResult]:
    """Squelch a batch in one segmented launch sequence.  ``items``: (frames [n, C] float32 as numpy or a device tensor,
    sample rate).  Returns device tensors (views of one output buffer)."""
    config.validate()
    torch = N.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    frames = [_ensure_2d(x) for x, _ in items]
    segs, in_off, base = [], 0, 0
    for x, (_, rate) in zip(frames, items):
        n, c = int(x.shape[0]), int(x.shape[1])
        segs.append(_segment(n, c, float(rate), config, in_off, base))
        in_off += -(-(n * c) // 64) * 64  # 256-byte aligned slots
        base += -(-n // N.SQ_TILE) * N.SQ_TILE
    nseg = len(segs)
    # input: one device buffer (a lone contiguous device tensor is used in place)
    if nseg == 1 and hasattr(frames[0], "is_cuda") and frames[0].is_cuda:
        inp = frames[0].to(torch.float32).contiguous().reshape(-1)
    else:
        host = np.zeros(in_off, dtype=np.float32)
        dev_parts = []
        for x, s in zip(frames, segs):
            if hasattr(x, "is_cuda"):
                dev_parts.append((x, s))
            else:
                host[s.in_off:s.in_off + x.size] = np.asarray(x, dtype=np.float32).reshape(-1)
        inp = torch.from_numpy(host).to(dev)
        for x, s in dev_parts:
            inp[s.in_off:s.in_off + x.numel()] = x.to(dev, torch.float32).reshape(-1)
    table = (N.SquelchSeg * nseg)(*segs)
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    handle = N.lib()
    ws_bytes = int(handle.iqa_squelch_workspace_bytes(base, nseg))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(max(in_off, 1), dtype=torch.int16 if pcm16 else torch.float32, device=dev)
    res_dev = torch.empty(nseg * ctypes.sizeof(N.SquelchResult), dtype=torch.uint8, device=dev)
    params = N.SquelchParams(method=N.SQ_METHOD[config.method], auto_floor=int(bool(config.auto_noise_floor)),
                             trim=int(bool(config.trim_silence)), out_pcm16=int(pcm16),
                             margin_db=float(config.threshold_margin_db),
                             transient_margin_db=float(config.transient_margin_db))
    N.call("iqa_squelch", ctypes.byref(params), table, nseg, N.ptr(table_dev), N.ptr(inp), N.ptr(out), N.ptr(res_dev),
           N.ptr(ws), ctypes.c_int64(ws_bytes), N.stream_ptr())
    res_host = res_dev.cpu().numpy().tobytes()  # the one read-back
    results = (N.SquelchResult * nseg).from_buffer_copy(res_host)
    offs = {k: int(handle.iqa_squelch_stage_offset(base, nseg, v)) for k, v in N.SQ_STAGE.items()} if return_stages else {}
    outs = []
    for s, r in zip(segs, results):
        c, n_out = s.channels, int(r.stop - r.start)
        y = out[s.in_off:s.in_off + n_out * c].reshape(n_out, c)
        stages = None
        if return_stages:
            def arr(name, dtype, s=s):
                width = torch.empty(0, dtype=dtype).element_size()
                o = offs[name] + s.base * width
                return ws[o:o + s.n * width].view(dtype)

            stages = dict(envelope_db=arr("envelope_db", torch.float32), level=arr("level", torch.float32),
                          threshold=arr("threshold", torch.float32), mask=arr("mask", torch.uint8).bool(),
                          dilated=arr("dilated", torch.uint8).bool(), gain=arr("gain", torch.float32),
                          noise_floor_db=float(r.noise_floor_db), threshold_db=float(r.threshold_db),
                          start=int(r.start), stop=int(r.stop), window=int(s.window), hold=int(s.hold), fade=int(s.fade))
        outs.append(_DeviceResult(y, float(r.noise_floor_db), float(r.threshold_db), int(r.start), int(r.stop), stages))
    return outs


def apply_squelch(audio, sample_rate: float, config: SquelchConfig, *, return_stages: bool = False):
    """ref: squelch.py apply_squelch.  numpy in -> (float32 [n_out, C] numpy, noise_floor_db, threshold_db);
    a CUDA tensor in -> the samples as a device tensor (nothing copied to the host).  ``return_stages=True`` appends
    a dict of the per-stage device arrays (envelope_db, level, threshold, mask, dilated, gain, trim bounds)."""
    on_device = hasattr(audio, "is_cuda") and audio.is_cuda
    samples = audio if on_device else np.asarray(audio, dtype=np.float32)
    samples = _ensure_2d(samples)
    (r,) = squelch_device([(samples, sample_rate)], config, return_stages=return_stages)
    y = r.samples if on_device else r.samples.cpu().numpy()
    if return_stages:
        return y, r.noise_floor_db, r.threshold_db, r.stages
    return y, r.noise_floor_db, r.threshold_db


# ---------------------------------------------------------------------------------------------------------------
# files


def _derive_output_path(path: Path, options: AudioPostOptions) -> Path:
    if options.overwrite:
        return path
    suffix = options.cleaned_suffix
    if not suffix:
        suffix = "-cleaned"
    return path.with_name(f"{path.stem}{suffix}{path.suffix}")


def _load_audio(path: Path) -> tuple[np.ndarray, int, str]:
    if path.suffix.lower() != ".wav":
        raise RuntimeError(f"{path.name}: {path.suffix} audio needs libsndfile, which this build does not use "
                           "(WAV only)")
    return iqio.read_wav_audio(path)


def _eligible_inputs(paths: Iterable[Path], allowed: Sequence[str]) -> list[Path]:
    choices: list[Path] = []
    suffixes = tuple(s.lower() for s in allowed)
    for path in paths:
        if not path.is_file():
            continue
        if suffixes and path.suffix.lower() not in suffixes:
            continue
        choices.append(path)
    return choices


def gather_audio_targets(path: Path, options: AudioPostOptions) -> list[Path]:
    if path.is_file():
        return _eligible_inputs([path], options.allowed_suffixes)
    if path.is_dir():
        return _eligible_inputs(sorted(path.iterdir()), options.allowed_suffixes)
    raise FileNotFoundError(f"No such file or directory: {path}")


def _finish(path: Path, data: np.ndarray, rate: int, subtype: str, r: _DeviceResult,
            options: AudioPostOptions, bytes_in: int) -> SquelchFileResult:
    output_path = _derive_output_path(path, options)
    y = r.samples.cpu().numpy()
    if y.dtype == np.int16:
        iqio.write_wav_audio(output_path, None, rate, subtype, encoded=y)
    else:
        iqio.write_wav_audio(output_path, y, rate, subtype)
    samples_in, samples_out = int(data.shape[0]), int(y.shape[0])
    return SquelchFileResult(
        input_path=path, output_path=output_path, samples_in=samples_in, samples_out=samples_out,
        duration_in=samples_in / float(rate), duration_out=samples_out / float(rate), bytes_in=bytes_in,
        bytes_out=output_path.stat().st_size, noise_floor_db=r.noise_floor_db, threshold_db=r.threshold_db,
        method=options.config.method, retained_ratio=samples_out / samples_in if samples_in else 0.0)


def process_audio_file(path: Path, options: AudioPostOptions) -> SquelchFileResult:
    path = Path(path)
    bytes_in = path.stat().st_size
    data, rate, subtype = _load_audio(path)
    (r,) = squelch_device([(data, float(rate))], options.config, pcm16=subtype == "PCM_16")
    return _finish(path, data, rate, subtype, r, options, bytes_in)


def process_audio_batch(
    targets: Sequence[Path],
    options: AudioPostOptions,
    *,
    progress_cb: Callable[[int, int, Path], None] | None = None,
    batch_bytes_limit: int = BATCH_BYTES,
) -> SquelchSummary:
    """ref: squelch.py process_audio_batch.  Files are read, packed into device batches of at most
    ``batch_bytes_limit`` bytes, squelched by one segmented launch sequence per batch and written in order;
    ``progress_cb`` sees the reference's calls ((i-1, total, path) before file i, (i, total, path) after it succeeded),
    each file's pair when the file is written."""
    results: list[SquelchFileResult] = []
    errors: list[tuple[Path, Exception]] = []
    total = len(targets)
    group: list[list] = []  # [index, path, loaded (data, rate, subtype, bytes_in) or None, exception or None]

    def flush() -> None:
        live = [g for g in group if g[3] is None]
        outs: list = []
        if live:
            pcm16 = all(g[2][2] == "PCM_16" for g in live)
            try:
                outs = squelch_device([(g[2][0], float(g[2][1])) for g in live], options.config, pcm16=pcm16)
            except Exception as exc:  # noqa: BLE001 - a failed launch fails each file of the batch
                for g in live:
                    g[3] = exc
        by_index = {g[0]: o for g, o in zip(live, outs)}
        for index, path, loaded, exc in group:
            if progress_cb:
                with np.errstate(all="ignore"):
                    progress_cb(index - 1, total, path)
            if exc is None:
                try:
                    result = _finish(path, loaded[0], loaded[1], loaded[2], by_index[index], options, loaded[3])
                except Exception as write_exc:  # noqa: BLE001
                    exc = write_exc
            if exc is not None:
                LOG.error("Audio post-processing failed for %s: %s", path, exc)
                errors.append((path, exc))
                continue
            results.append(result)
            if progress_cb:
                progress_cb(index, total, path)
        group.clear()

    used = 0
    for index, path in enumerate(targets, start=1):
        path = Path(path)
        try:
            bytes_in = path.stat().st_size
            data, rate, subtype = _load_audio(path)
            options.config.validate()
            _windows(int(data.shape[0]), float(rate), options.config)  # a file the chain rejects fails alone
        except Exception as exc:  # noqa: BLE001 - surfaced per file, as the reference does
            group.append([index, path, None, exc])
            continue
        cost = batch_bytes(int(data.shape[0]), int(data.shape[1]))
        if used and used + cost > batch_bytes_limit:
            flush()
            used = 0
        group.append([index, path, (data, rate, subtype, bytes_in), None])
        used += cost
    flush()
    return SquelchSummary(results=results, errors=errors)
