"""The demodulator drivers of the pipelines and runners (``ChannelDemod``, ``WfmDemod``) and the 48 kHz leg (``Resampler48k``)."""
from __future__ import annotations

import math
from ctypes import byref, c_double, c_int32, c_int64

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P
from .channelizer import _KERNEL_CACHE_LOCK
from .decoders import create_decoder
from .decoders.common import unit_prev
from .decoders.rds import RdsCore
from .decoders.side import SIDE_DECODERS, check_modes
from .decoders.wfm import WfmStereoCore, stereo_matrix


def chunk_rms_dbfs(sumsq_dev, counts) -> list[float]:
    """The writer's per-chunk level (dBFS) from the device sums of squares (IQA_SUMSQ_SLOTS = 8 sub-slots per chunk) and
    the chunks' sample counts; empty chunks are left out."""
    return [20.0 * math.log10(math.sqrt(float(s) / float(c) + 1e-18) + 1e-12)
            for s, c in zip(sumsq_dev.cpu().numpy().reshape(-1, 8).sum(axis=1), counts) if c > 0]


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
        return [v for sumsq, counts in self.chunk_sumsq for v in chunk_rms_dbfs(sumsq, counts)]


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
        return [] if self._sumsq is None else chunk_rms_dbfs(self._sumsq, self._counts)


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
            D.uploads_complete()  # before another thread (on another stream) can take the table from _TABLES
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
