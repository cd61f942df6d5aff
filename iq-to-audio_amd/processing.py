"""GPU stand-in for the reference's ``src/iq_to_audio/processing.py`` DSP surface.

Same names, arguments, state attributes and error behaviour as the reference classes
(cited per class), with all arithmetic in the HIP library (``libiqa_hotpath.so``):

    ProcessingConfig / ProcessingPipeline / ProcessingResult / ProcessingCancelled
    ComplexOscillator, OverlapSaveFIR, Decimator, design_channel_filter,
    choose_mix_sign, tune_chunk_size

plus :class:`Channelizer` (``channelizer.py``), the fused ingest+mix+filter+decimate stage the pipeline
actually runs (one pass over the raw int16/u8/f32 capture in HBM).

This module holds the configuration and result records and the two file pipelines; the rest of the surface lives in
modules of its own and is re-exported here: the stage classes (``stages.py``), the mixer-sign probe (``mixsign.py``), the
precision rules (``precision.py``), the demodulator drivers and the resampler (``channel_demod.py``), the file stager
(``staging.py``).  There is no CPU path: without a GPU or without the built library every stage raises ``RuntimeError``.
"""
from __future__ import annotations

import contextlib
import logging
import math
from ctypes import c_int32, c_int64
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P
from . import iqio
from .channel_demod import ChannelDemod, Resampler48k, WfmDemod  # noqa: F401  (re-exported)
from .channelizer import (_KERNEL_CACHE, _KERNEL_CACHE_LOCK, _KERNEL_CACHE_MAX, _TAPS_MEMO, ChannelBank,  # noqa: F401  (re-exported)
                          Channelizer, _as_frames, _cached_kernel, _ChannelKernel, _taps_fingerprint, immutable_taps)
from .decoders.side import SIDE_DECODERS, check_modes
from .dsp_plan import design_channel_filter, tune_chunk_size  # noqa: F401  (re-exported API)
from .gate import CarrierGate, CarrierSquelch
from .mixsign import (MixSignProbe, choose_mix_sign, probe_targets, probe_window, queue_raw_level,  # noqa: F401  (re-exported)
                      reserve_pinned_scalars, wideband_rms_from)
from .precision import FM_MODES, PRECISION_GUARD, SSB_AGC_PRECISION, base_precision, is_guarded, pick_precision  # noqa: F401  (re-exported)
from .progress import PhaseState, ProgressSink, ProgressTracker
from .stages import ComplexOscillator, Decimator, OverlapSaveFIR  # noqa: F401  (re-exported)
from .staging import _BlockStager

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


def is_pass_through(demod_mode) -> bool:
    """A target that is written as a slice of the channel's I/Q, not demodulated."""
    return (demod_mode or "").lower() in {"none", "pass", "iq"}


def check_squelch(squelch, demod_mode):
    """``squelch`` (a ``CarrierSquelch`` or None) for a target of ``demod_mode``: ``ValueError`` for a mode that has no
    channel-rate mono audio to gate, or for options the plan refuses."""
    if squelch is None:
        return None
    if not isinstance(squelch, CarrierSquelch):
        raise ValueError("squelch must be a CarrierSquelch or None")
    mode = (demod_mode or "").lower()
    if mode == "wfm" or is_pass_through(mode):
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
        return is_pass_through(self.config.demod_mode)

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
        self.pass_through = is_pass_through(cfg.demod_mode)
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
        if self.precision != "fast" and is_guarded(self.cfg.demod_mode):
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


@dataclass
class _OpenCapture:
    """What ``MultiChannelPipeline._open`` found out about the capture, for the steps behind it."""

    info: iqio.CaptureInfo
    sample_rate: float
    rate_probe: SampleRateProbe
    total: int  # frames of the run
    center_freq: float
    chunk: int


class _Int16Planes:
    """A float32 capture on the int16 matrix-core channelizers, block by block.

    Each block is split on the device into TWO int16 planes, x = 2^shift (hi + lo / 32768) / 32768 exactly to
    2^(shift - 31) (iqa_f32_split_s16), and the filter is linear: z = 2^shift (z(hi) + 2^-15 z(lo)), two passes of the int16
    channelizers (the second at "fast": its input is 2^-15 of the first's).  A block whose low plane is all zeros (every
    value k / 32768 at shift 0: what SDR software writes for int16 / 12-bit / int8 ADC samples) needs only the hi pass
    unless the low plane's history reaches into it.  The first block with a value the planes cannot hold (rint(2^(15 -
    shift) x) outside int16, or a NaN) switches the rest of the run to the float32 kernel, whose state has been carried
    along.  ``banks``: the run's ``(ChannelBank, members)`` per decimation, settled."""

    def __init__(self, targets: list, banks: list, shift: int):
        self.shift = shift
        self.hi = [ChannelBank([t._channelizer(t.mix_sign, precision=t.precision, fmt="s16") for t in members]) for _, members in banks]
        self.lo = [ChannelBank([t._channelizer(t.mix_sign, precision="fast", fmt="s16") for t in members]) for _, members in banks]
        self._flag = D.zeros(1, "int32")
        # the low plane's channelizers carry the last L-1 frames of the low plane into the next block: while those
        # may hold a non-zero value, a block whose own low plane is all zeros still has outputs at its head that
        # they reach (2^-15 z(lo) there), so the low plane is processed; ``_lo_quiet``: frames of all-zero low plane seen
        # since the last block that had one (the history is zero from the start)
        self._lo_hist_frames = max(len(t.taps) for t in targets) - 1
        self._lo_quiet = self._lo_hist_frames
        self._planes = None  # (hi, lo) of the block in hand
        self._lo_nonzero = self._lo_needed = False
        self.integer_blocks = 0  # blocks that ran as int16 planes with an all-zero low plane
        self.split_blocks = 0  # blocks that ran as int16 planes with some lo != 0

    def split(self, raw, n: int, done: int):
        """The (hi, lo) int16 planes of the block of ``n`` frames at frame ``done``, or None once the capture has left
        their range (from then on the blocks go through the run's float32 banks)."""
        if self.hi is None:
            return None
        hi, lo = D.empty(2 * n, "int16"), D.empty(2 * n, "int16")
        self._flag.zero_()
        N.call("iqa_f32_split_s16", N.ptr(raw), c_int64(2 * n), c_int32(self.shift), N.ptr(hi), N.ptr(lo), N.ptr(self._flag),
               N.stream_ptr())
        bits = int(self._flag.item())  # (a host read per 64 Mi-frame block)
        if bits & 1:
            LOG.info("float32 capture leaves the range of the int16 planes (shift %d) at frame %d: float32 channelizer.",
                     self.shift, done)
            self.hi = self.lo = self._planes = None
            return None
        self._lo_nonzero = bool(bits & 2)
        self._lo_needed = self._lo_nonzero or self._lo_quiet < self._lo_hist_frames
        self._planes = (hi, lo)
        return self._planes

    def channelize(self, bank_index: int, bank, raw, n: int) -> list:
        """The block's decimated streams for the channels of ``bank`` (the float32 bank of that decimation, whose state
        moves along) from the planes ``split`` made of ``raw``."""
        hi, lo = self._planes
        zs = self.hi[bank_index].process(hi)
        if self._lo_needed:
            zs_lo = self.lo[bank_index].process(lo)
            zs = [z.add_(zl, alpha=2.0 ** -15) for z, zl in zip(zs, zs_lo)]
        else:  # (low plane and its history all zeros: z(lo) = 0, its channelizers' history and position move along)
            for c in self.lo[bank_index].chans:
                c._advance(lo, n)
        if self.shift:
            zs = [z.mul_(2.0 ** self.shift) for z in zs]
        x32, _ = _as_frames(raw, "f32")
        for c in bank.chans:  # the float32 channelizers' state moves along (history, position)
            c._advance(x32, n)
        return zs

    def end_block(self, n: int) -> None:
        """Count the block of ``n`` frames that every bank has channelized from the planes."""
        self.integer_blocks += 0 if self._lo_nonzero else 1
        self.split_blocks += 1 if self._lo_nonzero else 0
        self._lo_quiet = 0 if self._lo_nonzero else self._lo_quiet + n
        self._planes = None


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
        self._planes = None  # the run's _Int16Planes (float32 captures that run on the int16 channelizers)
        self.wfm_stereo = None  # after run(): per target, the wfm stereo decision (None for the other modes)
        for e in SIDE_DECODERS:  # after run(): per target, the side decoder's result (None where it found nothing, or is off)
            setattr(self, e.name, None)

    def cancel(self) -> None:
        self._cancelled = True

    @property
    def integer_blocks(self) -> int:
        """Blocks of a float32 capture that ran as int16 planes with an all-zero low plane."""
        return 0 if self._planes is None else self._planes.integer_blocks

    @property
    def split_blocks(self) -> int:
        """Blocks of a float32 capture that ran as int16 planes with some lo != 0."""
        return 0 if self._planes is None else self._planes.split_blocks

    def run(self, progress_sink: ProgressSink | None = None) -> list:
        cfg = self.configs[0]
        tracker = ProgressTracker(progress_sink)
        targets: list[_Target] = []
        stager = None

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

        if cfg.input_sample_rate is not None and cfg.input_sample_rate <= 0:
            raise ValueError("Input sample rate override must be positive.")
        try:
            cap = self._open(tracker, _check_cancel, targets)
            np_dt = {"s16": "int16", "u8": "uint8", "f32": "float32"}[cap.info.fmt]
            block = max(1, self.owners[0].block_frames_target // cap.chunk) * cap.chunk
            stager = _BlockStager(iqio.map_frames(cap.info), np_dt, min(block, cap.total))
            warm, banks = self._probe_and_settle(cap, stager, targets, _check_cancel)
            if cfg.probe_only:
                tracker.advance("ingest", float(warm.numel() // 2))
                return self._results(cap, targets)
            self._run_blocks(cap, stager, block, warm, banks, targets, tracker, _check_cancel)

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
            return self._results(cap, targets)
        except ProcessingCancelled:
            if not cfg.probe_only:
                paths = [t.output_path for t in targets] or [c.output_path for c in self.configs if c.output_path]
                for pth in paths:
                    with contextlib.suppress(OSError):
                        pth.unlink(missing_ok=True)
            raise
        finally:
            if stager is not None:
                stager.close()
            tracker.close()

    @staticmethod
    def _results(cap: _OpenCapture, targets: list) -> list:
        """One ``ProcessingResult`` per target (``peak`` is 0.0 until a target's ``finish``)."""
        return [ProcessingResult(cap.rate_probe, cap.center_freq, t.target_freq, t.freq_offset, t.decimation, t.fs_channel,
                                 t.mix_sign, t.peak) for t in targets]

    def _open(self, tracker, check_cancel, targets: list) -> _OpenCapture:
        """Open and validate: capture info, rates, centre frequency, chunk, progress phases; one ``_Target`` per config is
        appended to ``targets``."""
        cfg = self.configs[0]
        manual_rate = cfg.input_sample_rate  # (run() has refused a non-positive one)
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
        rates = []  # (decimation, channel rate) per target
        for c in self.configs:
            decimation, fs_channel = P.choose_decimation(sample_rate, c.fs_ch_target)
            if (c.demod_mode or "").lower() == "wfm" and fs_channel < P.WFM_MIN_RATE:
                raise ValueError(f"wfm needs a channel rate of at least {P.WFM_MIN_RATE:.0f} Hz; --fs-ch {c.fs_ch_target:.0f} "
                                 f"gives {fs_channel:.0f} Hz")
            LOG.info("Input sample rate %.2f Hz; centre %.0f Hz, target %.0f Hz; decimation %d -> %.2f Hz",
                     sample_rate, center_freq, c.target_freq, decimation, fs_channel)
            n_est += total / max(decimation, 1)
            rates.append((decimation, fs_channel))
        phases = [PhaseState("ingest", "Ingest IQ", float(total)), PhaseState("channel", "Channelize", n_est),
                  PhaseState("demod", "Demodulate", n_est),
                  PhaseState("encode", "Encode Audio", len(self.configs) * total / sample_rate * 48_000.0)]
        if any(c.dump_iq_path for c in self.configs):
            phases.insert(3, PhaseState("dump_iq", "Write IQ Dump", n_est))
        tracker.start(phases)
        tracker.status("design filter")
        check_cancel("initialization")
        for c, o, (decimation, fs_channel) in zip(self.configs, self.owners, rates):
            targets.append(_Target(c, o, info=info, sample_rate=sample_rate, center_freq=center_freq,
                                   decimation=decimation, fs_channel=fs_channel, total=total))
        if total == 0:
            raise RuntimeError("Input stream produced no samples.")
        return _OpenCapture(info, sample_rate, rate_probe, total, center_freq, chunk)

    def _probe_and_settle(self, cap: _OpenCapture, stager, targets: list, check_cancel):
        """Probe and settle on the warm-up block: mixer signs, wideband level, the float32 captures' headroom, every
        target's precision; then the banks (and a float32 capture's int16 planes).  Returns (warm-up block, banks as
        (ChannelBank, members)); banks is None for a ``probe_only`` run, which ends here."""
        info = cap.info
        warm = stager.fetch(0, min(cap.chunk, cap.total))
        check_cancel("warm-up")
        for t in targets:  # all probes are enqueued before the first read-back
            t.begin(warm)
        # wideband level of the warm-up block as a fraction of full scale (for the precision guard): iqa_raw_level, the
        # same estimate the batch runners take (eight stretches spread over the block)
        level = D.zeros(1, "float64")
        queue_raw_level(warm, info.fmt, level)
        wideband_rms = wideband_rms_from(float(level.item()), info.fmt)
        # float32 captures as int16 planes: headroom from the warm-up block's largest value (a later block that exceeds
        # it falls back to the float32 kernel); decided before settle(), whose precision guard scales by it
        as_planes = info.fmt == "f32" and self.owners[0].f32_integer_path
        shift16 = 0
        if as_planes:
            top = float(warm.view(D.torch_mod().float32).abs().max().item())
            while shift16 < 8 and top * 2.0 ** (15 - shift16) > 32767.0:
                shift16 += 1
        self.f32_shift = shift16
        for t in targets:
            t.f32_shift = shift16
            t.settle(wideband_rms)
        self._planes = None
        if self.configs[0].probe_only:
            return warm, None
        # channels that share a decimation share their pass over every block (ChannelBank); built after settle(),
        # which may have replaced a channelizer by the one for the other mixer sign
        banks = []
        for key in sorted({t.decimation for t in targets}):
            members = [t for t in targets if t.decimation == key]  # (a bank runs its "full" / "float32" members one by one)
            banks.append((ChannelBank([t.chan for t in members]), members))
        self.banks = [b for b, _ in banks]
        if as_planes:
            self._planes = _Int16Planes(targets, banks, shift16)
        return warm, banks

    def _run_blocks(self, cap: _OpenCapture, stager, block: int, warm, banks: list, targets: list, tracker, check_cancel) -> None:
        """The block loop: every block of the capture through every bank, its channels' outputs to their targets."""
        total, chunk, planes = cap.total, cap.chunk, self._planes
        done = 0
        while done < total:
            check_cancel(f"block at frame {done}")
            hi = min(done + block, total)
            raw = warm if (done == 0 and hi <= warm.numel() // 2) else stager.fetch(done, hi)
            if hi < total:
                stager.prefetch(hi, min(hi + block, total))  # disk -> pinned memory while the GPU works
            n = hi - done
            tracker.advance("ingest", float(n))
            tracker.status(f"channel @ {done}")
            as_int16 = planes is not None and planes.split(raw, n, done) is not None
            for bi, (bank, members) in enumerate(banks):  # one pass over the block per decimation, all its channels at once
                for t in members:
                    t.before_block(done, n, chunk)
                zs = planes.channelize(bi, bank, raw, n) if as_int16 else bank.process(raw)
                for t, z in zip(members, zs):
                    t.after_block(z, tracker)
            if as_int16:
                planes.end_block(n)
            for bi, (_, members) in enumerate(banks):
                for ti, t in enumerate(members):  # (for finish(): which kernel produced this target's last block)
                    t.chan16_kernel = planes.hi[bi].chans[ti]._kernel.last_kernel if as_int16 else None
            check_cancel("encode")
            done = hi
