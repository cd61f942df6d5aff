"""The channelizer driver: host side of the fused ingest + mix + filter + decimate kernels.

:class:`_ChannelKernel` plans one channel (float32 VALU kernel, per-lane MFMA kernel, ring kernels) and is shared through
a small cache; :class:`Channelizer` carries one channel's streaming state across blocks; :class:`ChannelBank` runs several
channels of one capture as lanes of shared-ingest launches.  Every launch of the ring kernels goes through
``_launch_lanes``.  ``processing`` re-exports these names.
"""
from __future__ import annotations

import threading
from collections import OrderedDict
from ctypes import byref, c_double, c_int32, c_int64, c_void_p

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P
from . import iqio


def _as_frames(raw, fmt: str):
    """(device tensor, n_frames) for raw capture frames: int16/uint8 interleaved pairs, or
    float32 pairs / complex64 for 'f32' (both are the same bytes)."""
    if fmt == "f32":
        is_c = raw.is_complex() if D.is_tensor(raw) else np.iscomplexobj(raw)
        if is_c:
            x = D.to_device(raw, "complex64")
            return x, int(x.numel())
        x = D.to_device(raw, "float32").reshape(-1)
        return x, int(x.numel()) // 2
    x = D.to_device(raw, {"s16": "int16", "u8": "uint8"}[fmt]).reshape(-1)
    return x, int(x.numel()) // 2


def _block_size(n: int, ranges: int, floor: int, cap: int = 1 << 24) -> int:
    """Outputs per block of a launch of ``n`` outputs cut into ``ranges``: ceil(n / ranges) rounded up to whole 32-output
    tiles, at least ``floor`` and at most ``cap``."""
    return int(min(cap, max(floor, -(-(-(-n // ranges)) // 32) * 32)))


def _tap_unit(group, fmt: str) -> float:
    """``unit`` of a lane or a combine scale triple (include/iqa_hotpath.h: tap LSB / 256 for uint8 captures)."""
    return group.unit / (256.0 if fmt == "u8" else 1.0)


def _launch_lanes(lanes: list, pairs: bool, outputs_per_block: int, raw_dev, n_frames: int, consumed: int, m_first: int,
                  n_out: int) -> None:
    """ONE launch of the ring kernels (``pairs``: two lanes to a workgroup) for ``lanes``, each ``(kernel, pass, z_out,
    partial_in, partial_out, raw_partials)``: tap-row group ``pass.group`` of that channel kernel over the pass's k-step
    range (the same for every lane); buffers are device pointers or None, a lane without ``partial_out`` is final and
    writes z.  A lane that is ``None`` stays a zeroed entry: the empty half of an odd pair."""
    (k0, ps0), fmt = lanes[0][:2], lanes[0][0].plan.fmt
    table = (N.MfmaLane * len(lanes))()
    for lane, spec in zip(table, lanes):
        if spec is None:
            continue
        k, ps, z_out, partial_in, partial_out, raw_partials = spec
        group = k.mfma.groups[ps.group]
        lane.afrag_dev = k.afrag_dev[ps.group][ps.k_first * P.MFMA_KSTEP_BYTES :].data_ptr()
        lane.z_out_dev, lane.partial_in_dev, lane.partial_out_dev = z_out, partial_in, partial_out
        lane.unit = _tap_unit(group, fmt)
        lane.c_re, lane.c_im = ps.c_re, ps.c_im
        lane.rot_step, lane.rot_base = k.params.rot_step, k.params.rot_base
        lane.out_scale_re, lane.out_scale_im = k.params.out_scale_re, k.params.out_scale_im
        lane.conj_sum, lane.rotate = k.params.conj_sum, k.params.rotate
        lane.q_group, lane.finalize, lane.raw_partials = group.q, int(partial_out is None), int(raw_partials)
        lane.reserved = (0 if k.acc32 else 1) | (2 if group.high_only else 0)  # (bit 0: 64-bit sums; bit 1: q2 == 0)
        # a launch of one lane over all k steps: the rotated fragments, their rot in bits 8..13 (skips the zero high tap bytes)
        rot_dev = k.afrag_rot_dev[ps.group] if len(lanes) == 1 and not pairs and ps.k_first == 0 and ps.k_count == k.mfma.ksteps else None
        if rot_dev is not None:
            lane.afrag_dev = rot_dev.data_ptr()
            lane.reserved |= group.rot << 8
        k.last_kernel = f"k_channelize_mfma_{fmt}_ring"
    N.call("iqa_channelize_mfma_pairs" if pairs else "iqa_channelize_mfma_multi", c_int32(P.FMT_CODE[fmt]),
           c_int32(k0.plan.decimation), c_int32(ps0.k_first), c_int32(ps0.k_count), c_int32(outputs_per_block), table,
           c_int32(len(lanes)), N.ptr(raw_dev), c_int64(n_frames), c_int64(consumed), c_int64(m_first), c_int64(n_out),
           N.stream_ptr())


class _ChannelKernel:
    """Shared launcher for the fused channelizer kernels.

    ``iqa_channelize`` (float32 VALU form, every format, guarded edges) is always available;
    for int16 captures with ceil(L/D) <= 64 the interior of each block runs on the int8-MFMA
    form ``iqa_channelize_mfma`` and only the few outputs that touch the history (head) or the
    end of the block (tail) go through the VALU kernel.
    """

    #: set to False to force the float32 VALU kernel everywhere (tests compare the two)
    use_mfma = True
    #: set to False to launch single lanes on the unrotated fragments (tests compare the two; read when the plan is made)
    use_zero_rows = True
    #: data path of the MFMA kernel: "ring" (channelize_ring.hip: persistent blocks stream their contiguous run of the
    #: capture through an LDS-DMA ring, tap fragments in registers; falls back to "plain" where it does not apply:
    #: D % 4 != 0, D > 256, multi-range passes) or "plain" (channelize_mfma.hip: per-lane row loads into VGPRs)
    mfma_variant = "ring"
    #: sums of the ring kernel: True (default) = one int32 256*S1 + S2 per output component with the tap unit enlarged
    #: until that cannot overflow for any input (~14-bit taps, error ~1e-5 of full scale); False = one int64
    #: (S1 << 32) + S2 with 16-bit taps -- the same integers as the per-lane kernel (~1e-6) -- at +10 % kernel time
    #: (ds_add_u64 moves 3 dwords and takes two passes through the LDS banks).  Both are exact integer sums.
    ring_acc32 = True
    RING_ROWS_KSTEPS = 11  # k steps per pass of the row-staged ring kernel (its tap fragments live in registers)
    mfma_min_outputs = 32768

    #: Precisions of a channelizer, cheapest first:
    #:   "fast"    -- the ring kernels, ONE int32 sum per output component, ~14-bit taps: z error ~3e-6 of full scale
    #:   "fine"    -- the same kernels, every tap-row group as TWO lanes (high-byte-only taps + their residue, added by
    #:                iqa_mfma_combine): twice the matrix work, error 10..90x smaller; uint8 captures: exact products
    #:   "full"    -- 16-bit taps without the int32 bound, the same two groups: z error ~1e-9 of full scale -- below the float32
    #:                rounding of z itself -- at ~2.3x the time of "fast".  Contiguous ring slots (D % 4 == 0, <= 15 k steps):
    #:                lanes of the ring kernels with 64-bit sums (shared ingest, pairs at 9..14 k steps); every other
    #:                decimation: chained passes of the per-lane kernel (separate S1/S2 sums).  int16 captures; uint8 ->
    #:                "fine", float32 -> "float32"
    #:   "float32" -- the float32 VALU kernel for every output (~20x the time of "fast"; the only form for float32 captures)
    PRECISIONS = ("fast", "fine", "full", "float32")

    def __init__(self, plan: P.ChannelPlan, exact: bool = False, precision: str | None = None):
        self.plan = plan
        precision = precision or ("float32" if exact else "fast")
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {self.PRECISIONS}, not {precision!r}")
        if plan.fmt == "f32" and precision != "fast":
            precision = "float32"
        if plan.fmt == "u8" and precision == "full":
            precision = "fine"
        self.precision = precision
        self.exact = precision == "float32"  # float32 kernel everywhere
        self.variant = self.mfma_variant  # ("full" off the contiguous ring slots: no ring mode below -> the per-lane kernel)
        self.acc32 = bool(self.ring_acc32) and precision != "full"
        self.residual = precision in ("fine", "full")
        lpad = int(N.lib().iqa_taps_padded_len(plan.ntaps))
        if plan.taps_window.size != lpad:
            raise ValueError("tap window padding does not match the library")
        self.taps_dev = D.from_numpy(plan.taps_window)
        self.params = N.ChanParams(
            fmt=P.FMT_CODE[plan.fmt], ntaps=plan.ntaps, decimation=plan.decimation, conj_sum=plan.conj_sum,
            rotate=plan.rotate, reserved=0, rot_step=plan.rot_step, rot_base=plan.rot_base,
            out_scale_re=float(np.real(plan.out_scale)), out_scale_im=float(np.imag(plan.out_scale)),
        )
        self.mfma = None  # planned lazily, the first time a block is long enough to use it
        # kernels are shared through _KERNEL_CACHE: held while planning, and while a pass of the per-lane kernel sets and
        # launches its cached parameter struct (a ring pass builds its lane per launch)
        self._lock = threading.Lock()
        self.last_kernel = "k_channelize_v1"
        # which ring kernel covers this decimation: 1 = contiguous slots (all k steps in one pass), 2 = row-staged slots
        # (any D, k-step ranges of <= RING_ROWS_KSTEPS, int32 sums only; the only form for uint8 captures), 0 = none ->
        # the per-lane kernel (int16) or the VALU kernel (uint8)
        ks_all = -(-2 * plan.decimation // 32)
        self._ring_mode = 0
        if plan.fmt in ("s16", "u8") and self.variant == "ring":
            acc32, code = int(bool(self.acc32)), P.FMT_CODE[plan.fmt]
            self._ring_mode = int(N.lib().iqa_mfma_ring_mode(code, plan.decimation, 0, ks_all, acc32))
            if self._ring_mode == 0:
                self._ring_mode = int(N.lib().iqa_mfma_ring_mode(code, plan.decimation, 0, min(ks_all, self.RING_ROWS_KSTEPS), acc32))
        self._mfma_ok = bool(self.use_mfma and not self.exact and P.mfma_supported(plan) and (plan.fmt == "s16" or self._ring_mode == 2))

    def _ensure_mfma(self):
        with self._lock:
            if self.mfma is None:
                ring = self.variant == "ring" and self._ring_mode != 0
                mp = P.plan_mfma(self.plan, acc32=ring and self.acc32,
                                 max_ksteps=self.RING_ROWS_KSTEPS if self._ring_mode == 2 else None, residual=self.residual)
                self.afrag_dev = [D.from_numpy(g.afrag.reshape(-1).view(np.uint8)) for g in mp.groups]
                # rotated fragments (dsp_plan.zero_high_rotation) where a single-lane launch of this kernel takes them
                # (all k steps in one pass, a rot the kernel's lane groups can follow): None otherwise
                self.afrag_rot_dev = [
                    D.from_numpy(g.afrag_rot.reshape(-1).view(np.uint8))
                    if ring and self.use_zero_rows and g.rot and g.rot % 4 == 0 and g.rot <= 32 and N.lib().iqa_mfma_ring_zero_rows(
                        P.FMT_CODE[self.plan.fmt], self.plan.decimation, 0, mp.ksteps, int(bool(self.acc32))) else None
                    for g in mp.groups]
                # every pass with its variant: None = a lane of the ring kernels, else the per-lane ("plain") kernel's parameters
                self._passes = [(ps, None if ring else N.MfmaParams(
                    reserved=0, unit=mp.groups[ps.group].unit, c_re=ps.c_re, c_im=ps.c_im, q_group=mp.groups[ps.group].q,
                    k_first=ps.k_first, k_count=ps.k_count)) for ps in mp.passes]
                D.uploads_complete()  # the fragments' copies: this kernel is shared through _KERNEL_CACHE (see there)
                self.mfma = mp
            return self.mfma

    def fixed_point_error_norm(self) -> float:
        """z error (RMS) of the fixed-point kernels per unit RMS of a white wideband input at full scale = 1: the 2-norm
        of the tap quantisation error (0.0 when this channel never runs on the matrix cores)."""
        return float(self._ensure_mfma().err_norm) if self._mfma_ok else 0.0

    def fixed_point_error_rms(self, wideband_rms: float) -> float:
        """Expected z error (RMS, fraction of full scale) of this kernel for a capture of the given wideband RMS: tap
        rounding x wideband level plus the level-independent floor of the dropped (low tap byte) x (low data byte)
        products -- for uniform low bytes, never below the plan's zero-input response, and for a quiet capture the bound
        for low bytes coherent with an in-channel signal (``dsp_plan.dropped_floor``); 0.0 when this channel never runs on
        the matrix cores."""
        return float(self._ensure_mfma().z_error_rms(wideband_rms)) if self._mfma_ok else 0.0

    @staticmethod
    def _plain_range_max(k_count: int) -> int:
        """Per-lane kernel: one 8-wave block per CU owns all 160 KiB of LDS -- this pass's tap fragments + 16 B per output.
        (A block of the ring kernel is not bounded by LDS: tap fragments in registers, sums in a sliding window.)"""
        lds = 160 * 1024 - k_count * P.MFMA_KSTEP_BYTES
        return int(min(6144, (lds // 16 - 160) // 32 * 32))

    #: workgroups of a capture-long launch: one per CU of the MI355X
    launch_blocks = 256

    @classmethod
    def _block_outputs(cls, n_out: int, rmax: int, per_cu: int = 1) -> int:
        """Outputs per block for a launch of ``n_out`` outputs: as large as LDS allows, but chosen so that the
        number of blocks is a multiple of the 256 CUs (one block per CU, no ragged last round).  The ring kernel
        has no LDS bound (``rmax`` huge): every CU gets ONE contiguous range of the launch -- ``per_cu`` of them where
        that many of its workgroups fit into a CU's LDS (short rows: <= 3 k steps)."""
        blocks = cls.launch_blocks * per_cu
        rounds = max(1, -(-n_out // (blocks * rmax)))
        return _block_size(n_out, blocks * rounds, 512, rmax)

    def _workgroups_per_cu(self, ps) -> int:
        lds = int(N.lib().iqa_mfma_ring_lds_bytes(P.FMT_CODE[self.plan.fmt], self.plan.decimation, ps.k_first, ps.k_count,
                                                  1 if self.acc32 else 0))
        return 2 if 0 < lds <= 80 * 1024 else 1

    def _valu(self, raw_dev, n_frames, consumed, hist_dev, m_first, n_out, out_dev):
        if n_out > 0:
            N.call("iqa_channelize", byref(self.params), N.ptr(self.taps_dev), N.ptr(raw_dev), c_int64(n_frames),
                   c_int64(consumed), N.ptr(hist_dev), c_int64(m_first), c_int64(n_out), N.ptr(out_dev), N.stream_ptr())

    def _interior(self, consumed: int, n_frames: int, m_first: int, n_out: int) -> tuple[int, int]:
        """Outputs [m_a, m_b) the matrix-core kernels can produce from this block's frames alone."""
        d = self.plan.decimation
        ksteps = -(-2 * d // 32)
        n_groups = max(1, -(-(-(-self.plan.ntaps // d)) // P.MFMA_Q))
        m_a, m_b = P.mfma_interior(consumed, n_frames, m_first, n_out, d, ksteps, n_groups)
        if self.variant == "ring" and self._ring_mode == 1:
            # a contiguous ring tile is fetched as 2048*ksteps bytes from its first frame
            m_b = min(m_b, (n_frames + consumed - 512 * ksteps - 1) // d + 2)
        return (m_a, m_b) if m_b > m_a else (m_first, m_first)

    def _mfma_passes(self, raw_dev, n_frames: int, consumed: int, m_a: int, n_int: int, out_dev, min_block: int = 512):
        """The passes of the plan in order, chained through one float64 partial buffer; the last one writes z."""
        self._ensure_mfma()
        buf = D.empty(2 * n_int, "float64") if len(self._passes) > 1 else None
        partial = N.ptr(buf).value  # (None without a buffer)
        for i, (ps, prm) in enumerate(self._passes):
            last = i == len(self._passes) - 1
            partial_in, partial_out = (partial if i > 0 else None), (None if last else partial)
            if prm is None:
                rng = self._block_outputs(n_int, 1 << 24, self._workgroups_per_cu(ps))
                if min_block < 512:  # short launches: more, smaller blocks
                    rng = _block_size(n_int, 256, min_block, rng)
                _launch_lanes([(self, ps, out_dev.data_ptr() if last else None, partial_in, partial_out, False)], False, rng,
                              raw_dev, n_frames, consumed, m_a, n_int)
            else:
                self.last_kernel = "k_channelize_mfma_s16"
                afrag = self.afrag_dev[ps.group][ps.k_first * P.MFMA_KSTEP_BYTES :]
                with self._lock:
                    prm.outputs_per_block = self._block_outputs(n_int, self._plain_range_max(ps.k_count))
                    prm.finalize = int(last)
                    prm.partial_in_dev, prm.partial_out_dev = partial_in, partial_out
                    N.call("iqa_channelize_mfma", byref(self.params), byref(prm), N.ptr(afrag), N.ptr(raw_dev),
                           c_int64(n_frames), c_int64(consumed), c_int64(m_a), c_int64(n_int), N.ptr(out_dev), N.stream_ptr())

    def run_interior_only(self, raw_dev, n_frames: int, m_first: int, n_out: int, out_dev) -> bool:
        """Outputs [m_first, m_first + n_out) of a block that starts the capture (consumed = 0), matrix-core kernels
        only -- for callers that do not want the outputs near the block's edges (the mixer-sign probes discard the
        filter's transient and read a snippet of a longer buffer).  False (nothing launched) when the range is not
        wholly interior or the capture format has no matrix-core kernel."""
        if not (self._mfma_ok and self.variant == "ring" and self._ring_mode) or n_out < 64:
            return False
        m_a, m_b = self._interior(0, n_frames, m_first, n_out)
        if m_a != m_first or m_b != m_first + n_out:
            return False
        self._mfma_passes(raw_dev, n_frames, 0, m_first, n_out, out_dev, min_block=64)
        return True

    def _edges(self, edge_stream, *args):
        if edge_stream is None:
            return self._valu(*args)
        with D.torch_mod().cuda.stream(edge_stream):
            self._valu(*args)

    def run(self, raw_dev, n_frames: int, consumed: int, hist_dev, m_first: int, n_out: int, out_dev=None,
            events=None, halo=None, edge_stream=None):
        """``events``: optional (start, stop) torch.cuda.Event pair recorded around the dominant launch.
        ``halo``: optional (buffer, lead_frames) -- ``raw_dev`` is the slice ``buffer[lead : lead + n_frames]`` (in
        frames) of a larger device buffer whose ``lead`` frames in front hold the history of this block (zeros at the
        start of a capture) and whose frames behind may be read (their values are never used): the matrix-core
        kernels then cover the block's first and last outputs too and the two VALU edge launches disappear.
        ``edge_stream``: optional torch stream for the small VALU launches of the block's first and last outputs (they
        write their own part of ``out_dev``); the caller orders it against the producers of ``raw_dev`` and the
        consumers of ``out_dev``."""
        if out_dev is None:
            out_dev = D.empty(n_out, "complex64")
        self.last_kernel = "k_channelize_v1"
        if self._mfma_ok and n_out >= self.mfma_min_outputs:
            big, big_frames, big_consumed = raw_dev, n_frames, consumed
            if halo is not None:  # the matrix-core kernels address the enclosing buffer
                big, lead = halo
                big_frames, big_consumed = int(big.numel()) // 2, consumed - int(lead)  # 2 values per frame (I, Q)
            m_a, m_b = self._interior(big_consumed, big_frames, m_first, n_out)
            if m_b - m_a >= self.mfma_min_outputs:
                self._edges(edge_stream, raw_dev, n_frames, consumed, hist_dev, m_first, m_a - m_first, out_dev)
                if events:
                    events[0].record()
                self._mfma_passes(big, big_frames, big_consumed, m_a, m_b - m_a, out_dev[m_a - m_first :])
                if events:
                    events[1].record()
                self._edges(edge_stream, raw_dev, n_frames, consumed, hist_dev, m_b, m_first + n_out - m_b,
                            out_dev[m_b - m_first :])
                return out_dev
        if events:
            events[0].record()
        self._valu(raw_dev, n_frames, consumed, hist_dev, m_first, n_out, out_dev)
        if events:
            events[1].record()
        return out_dev


# Planned channelizer kernels (rotated taps, quantised MFMA fragments, their device copies) are immutable once
# built and cost ~0.5 ms of host NumPy per configuration: a batch of captures with the same settings, the two
# probes of choose_mix_sign and the channelizer that follows them all share them through this small LRU.
_KERNEL_CACHE: "OrderedDict[tuple, tuple]" = OrderedDict()
_KERNEL_CACHE_MAX = 192  # (BASELINE config 5 on one GPU: 40 channels x (two probe signs + the channel) = 120 kernels, ~0.5 MB of device taps each)
_KERNEL_CACHE_LOCK = threading.Lock()


_TAPS_MEMO: dict = {}  # id(array) -> (array, its bytes, their hash), for arrays that cannot change


def _taps_fingerprint(taps: np.ndarray):
    """(bytes, hash) of a tap vector.  Hashing 50-260 KB costs 25-130 us, and a batch asks three times per capture with
    the same array: an array that owns its data and is not writeable (``immutable_taps``) is fingerprinted once."""
    frozen = (not taps.flags.writeable) and taps.base is None
    if frozen:
        memo = _TAPS_MEMO.get(id(taps))
        if memo is not None and memo[0] is taps:
            return memo[1], memo[2]
    raw = taps.tobytes()
    h = hash(raw)
    if frozen:
        with _KERNEL_CACHE_LOCK:
            if len(_TAPS_MEMO) >= 64:
                _TAPS_MEMO.clear()
            _TAPS_MEMO[id(taps)] = (taps, raw, h)
    return raw, h


def immutable_taps(taps) -> np.ndarray:
    """A private, contiguous, read-only copy of a tap vector (what the kernel cache can recognise without hashing)."""
    out = np.array(taps, copy=True, order="C")
    out.setflags(write=False)
    return out


def _cached_kernel(taps: np.ndarray, *, sample_rate: float, freq_offset: float, mix_sign: int, decimation: int,
                   fmt: str, iq_order: str, exact: bool = False, precision: str | None = None):
    """(plan, kernel) for this configuration, planned once per process and device."""
    taps = np.ascontiguousarray(taps)
    raw, raw_hash = _taps_fingerprint(taps)
    key = (raw_hash, taps.dtype.str, taps.shape, float(sample_rate), float(freq_offset), int(mix_sign), int(decimation),
           fmt, iq_order, _ChannelKernel.use_mfma, _ChannelKernel.mfma_variant, _ChannelKernel.ring_acc32,
           precision or ("float32" if exact else "fast"), D.torch_mod().cuda.current_device())
    with _KERNEL_CACHE_LOCK:
        hit = _KERNEL_CACHE.get(key)
        if hit is not None and (hit[0] is raw or hit[0] == raw):
            _KERNEL_CACHE.move_to_end(key)
            return hit[1], hit[2]
    lpad = int(N.lib().iqa_taps_padded_len(len(taps)))
    plan = P.plan_channel(taps, sample_rate=sample_rate, freq_offset=freq_offset, mix_sign=mix_sign,
                          decimation=decimation, fmt=fmt, iq_order=iq_order, padded_len=lpad)
    kernel = _ChannelKernel(plan, exact, precision)
    D.uploads_complete()  # the tap window's copy, before another thread (on another stream) can take the kernel from the cache
    with _KERNEL_CACHE_LOCK:
        _KERNEL_CACHE[key] = (raw, plan, kernel)
        while len(_KERNEL_CACHE) > _KERNEL_CACHE_MAX:
            _KERNEL_CACHE.popitem(last=False)
    return plan, kernel


class Channelizer:
    """Fused ingest + NCO mix + channel FIR + decimate over raw capture frames.

    Equivalent to ``Decimator(D).process(OverlapSaveFIR(taps, B).process(
    ComplexOscillator(f_off, fs).mix(ingest(raw), sign)))`` of the reference
    (processing.py:1088-1096) with the streaming state of all three carried across calls,
    computed in one kernel that reads each raw frame (4 bytes for int16 I/Q) from HBM and
    writes only the decimated complex64 stream.
    """

    def __init__(self, taps: np.ndarray, *, sample_rate: float, freq_offset: float, mix_sign: int, decimation: int,
                 fmt: str = "s16", iq_order: str = "iq", exact: bool = False, precision: str | None = None):
        """``precision``: "fast" (default), "fine", "full" or "float32" -- see ``_ChannelKernel.PRECISIONS``; what the
        pipeline's precision guard and its SSB-with-AGC rule pick per target.  ``exact=True`` is "float32"."""
        self.plan, self._kernel = _cached_kernel(taps, sample_rate=sample_rate, freq_offset=freq_offset, mix_sign=mix_sign,
                                                 decimation=decimation, fmt=fmt, iq_order=iq_order, exact=exact, precision=precision)
        self.precision = self._kernel.precision
        self.fmt = fmt
        self.decimation = int(decimation)
        self.ntaps = len(taps)
        self.consumed = 0  # frames seen so far (global index of the next frame)
        self._hist = None  # device raw frames [L-1], same fmt

    def plan_ahead(self) -> None:
        """Do the host-side MFMA planning and tap upload now (otherwise done lazily by the first long block)."""
        if self._kernel._mfma_ok:
            self._kernel._ensure_mfma()

    def outputs_for(self, n_frames: int) -> tuple[int, int]:
        """(m_first, n_out) for a block of ``n_frames`` frames appended now."""
        d = self.decimation
        m_first = -(-self.consumed // d)
        m_end = -(-(self.consumed + n_frames) // d)
        return m_first, m_end - m_first

    def process(self, raw, out_dev=None, events=None, last_block: bool = False, halo=None, edge_stream=None):
        """``raw``: interleaved frames (NumPy or device tensor, dtype of ``fmt``; complex64 for f32).
        Returns the decimated complex64 samples for this block.  ``last_block``: nothing follows, so the
        L-1 frame history is not carried over (saves a launch for whole-capture calls).  ``halo``, ``edge_stream``:
        see ``_ChannelKernel.run`` (int16 / uint8 device captures only)."""
        x, n = _as_frames(raw, self.fmt)
        if n == 0:
            return D.like_input(D.empty(0, "complex64"), raw)
        m_first, n_out = self.outputs_for(n)
        if halo is not None and (self.fmt not in ("s16", "u8") or not D.is_tensor(raw)):
            halo = None
        z = None
        if n_out and D.is_tensor(raw) and self._several_lanes():
            # a filter with several tap-row groups: its groups as lanes of ONE shared-ingest launch (in pairs where the
            # kernel offers them) + the combine launch, instead of one pass over the capture per group
            if events:
                events[0].record()
            zs = ChannelBank([self])._run_shared(x, n, m_first, n_out, [out_dev], halo, edge_stream)
            if zs is not None:
                z = zs[0]
                if events:
                    events[1].record()
        if z is None:
            z = (self._kernel.run(x, n, self.consumed, self._hist, m_first, n_out, out_dev, events, halo, edge_stream)
                 if n_out else D.empty(0, "complex64"))
        self._advance(x, n, last_block)
        return D.like_input(z, raw)

    def _several_lanes(self) -> bool:
        k = self._kernel
        if not (self.lanes_for_groups and self.fmt in ("s16", "u8") and ChannelBank._lane_capable(k)):
            return False
        return len(k._ensure_mfma().groups) > 1

    lanes_for_groups = True  # (class switch: profiles compare against the chained passes)

    def _advance(self, x, n: int, last_block: bool = False) -> None:
        """Carry the last L-1 raw frames over to the next block and move on by ``n`` frames."""
        keep = 0 if last_block else self.ntaps - 1
        if keep:
            nxt = D.empty(keep * iqio.FRAME_BYTES[self.fmt], "uint8")
            N.call("iqa_history_update", c_int32(P.FMT_CODE[self.fmt]), c_int32(self.ntaps), N.ptr(self._hist),
                   N.ptr(x), c_int64(n), N.ptr(nxt), N.stream_ptr())
            self._hist = nxt
        self.consumed += n


class ChannelBank:
    """Several channels of ONE capture through a single pass over each block (BASELINE configs 3 and 5).

    The reference runs one whole pipeline per ``--ft`` target over the same file (cli.py:683-710).  Here the channelizers
    of a capture that share the decimation and the sample format put all their (channel, tap-row group) pairs into ONE
    launch of the ring kernel (``iqa_channelize_mfma_multi``): the lanes of a stretch of the capture run at the same time
    on the CUs of one XCD, so the stretch is fetched from HBM once and the other lanes read it from that XCD's L2.
    Filters with several tap-row groups (ceil(L/D) > 64) are several lanes whose partial sums ``iqa_mfma_combine`` adds
    up in group order -- the same additions, in the same order, as the chained single-channel passes, so a bank
    produces exactly what its channelizers would produce one by one.  The few outputs at a block's head and tail go
    through each channel's float32 kernel as usual.  Falls back to one channel at a time whenever a block is too short
    for the matrix-core kernels or the channels do not share a kernel shape.
    """

    MAX_LANES = 16  # per launch (the lane table travels as kernel arguments)
    pair_lanes = True  # two lanes of equal tap-row group per workgroup where the kernel offers it (see _run_shared)

    def __init__(self, channelizers: list):
        if not channelizers:
            raise ValueError("a bank needs at least one channelizer")
        self.chans = list(channelizers)
        first = self.chans[0]
        self.fmt, self.decimation = first.fmt, first.decimation
        for c in self.chans:
            if (c.fmt, c.decimation, c.consumed) != (self.fmt, self.decimation, first.consumed):
                raise ValueError("the channels of a bank share the capture: same sample format, decimation and position")
        self.last_launch = None  # {"lanes": n, "launches": n, "combines": n} of the most recent block (None: one by one)

    @staticmethod
    def _lane_capable(k) -> bool:
        """This channel's tap-row groups can be lanes of a shared-ingest launch: ring kernels with int32 sums (any slot
        form) or with 64-bit sums (contiguous slots only)."""
        return bool(k._mfma_ok and k.variant == "ring" and k._ring_mode and (k.acc32 or k._ring_mode == 1))

    def _shared_shape(self) -> bool:
        ks = [c._kernel for c in self.chans]
        if not ks or not all(self._lane_capable(k) for k in ks) or len({k.acc32 for k in ks}) != 1:
            return False
        if len(ks) == 1:  # one channel: worth a shared-ingest launch only when its filter is several lanes (tap-row groups)
            return len(ks[0]._ensure_mfma().groups) > 1
        return len({k._ring_mode for k in ks}) == 1

    def process(self, raw, outs=None, last_block: bool = False, halo=None, edge_stream=None) -> list:
        """One block of the capture for every channel; returns the decimated streams in channel order.
        ``edge_stream``: optional torch stream for the small float32 launches of every channel's first and last outputs
        (they write their own part of the outputs); the caller orders it against the producers of ``raw`` and the
        consumers of the outputs, as with ``Channelizer.process``."""
        x, n = _as_frames(raw, self.fmt)
        outs = list(outs) if outs is not None else [None] * len(self.chans)
        first = self.chans[0]
        m_first, n_out = first.outputs_for(n)
        zs = None
        if n and n_out and D.is_tensor(raw) and self._shared_shape():
            zs = self._run_shared(x, n, m_first, n_out, outs, halo, edge_stream)
        if zs is None:
            self.last_launch = None
            capable = [i for i, c in enumerate(self.chans) if self._lane_capable(c._kernel)]
            widths = sorted({self.chans[i]._kernel.acc32 for i in capable}, reverse=True)
            if D.is_tensor(raw) and capable and (len(capable) < len(self.chans) or len(widths) > 1):
                # channels of several precisions in the bank: the lanes with int32 sums share one pass, the lanes with
                # 64-bit sums ("full") another, whatever has no lanes ("full" off the contiguous slots, "float32") follows
                # one by one
                res = [None] * len(self.chans)
                self.last_launch, self.launches = None, []
                for acc32 in widths:
                    lanes = [i for i in capable if self.chans[i]._kernel.acc32 == acc32]
                    sub = ChannelBank([self.chans[i] for i in lanes])
                    got = sub.process(raw, outs=[outs[i] for i in lanes], last_block=last_block, halo=halo, edge_stream=edge_stream)
                    self.launches.append(sub.last_launch)
                    if self.last_launch is None:
                        self.last_launch = sub.last_launch
                    for i, z in zip(lanes, got):
                        res[i] = z
                for i, (c, o) in enumerate(zip(self.chans, outs)):
                    if res[i] is None:
                        res[i] = c.process(raw, out_dev=o, last_block=last_block, halo=halo)
                return res
            return [c.process(raw, out_dev=o, last_block=last_block, halo=halo) for c, o in zip(self.chans, outs)]
        for c in self.chans:
            c._advance(x, n, last_block)
        return zs

    def run_interior_only(self, x_all, n_frames: int, m_first: int, n_out: int, outs: list) -> bool:
        """Outputs [m_first, m_first + n_out) of a block that starts the capture, for every channel, matrix-core kernels
        only (no float32 edge launches): what ``_ChannelKernel.run_interior_only`` does for one channel, for callers that
        do not want the outputs near the block's edges (the mixer-sign probes).  False (nothing launched) when the range
        is not interior for every channel or the channels do not share a kernel shape."""
        if n_out < 64 or not self._shared_shape():
            return False
        kernels = [c._kernel for c in self.chans]
        plans = [k._ensure_mfma() for k in kernels]
        if len(kernels) > self.MAX_LANES or any(len(mp.groups) != 1 or len(mp.passes) != 1 for mp in plans):
            # filters with several tap-row groups / k-step passes: partial sums and combine launches as for a whole block
            return self._run_shared(x_all, n_frames, m_first, n_out, list(outs), None, None, interior_only=True) is not None
        # single-group, single-pass filters (the usual probe): one lane each, one launch, nothing else
        if any(k._interior(0, n_frames, m_first, n_out) != (m_first, m_first + n_out) for k in kernels):
            return False
        if len({(mp.passes[0].k_first, mp.passes[0].k_count) for mp in plans}) != 1:
            return False
        rng = _block_size(n_out, 8 * max(1, (_ChannelKernel.launch_blocks // 8) // len(kernels)), 64)
        _launch_lanes([(k, mp.passes[0], z.data_ptr(), None, None, False) for k, mp, z in zip(kernels, plans, outs)], False,
                      rng, x_all, n_frames, 0, m_first, n_out)
        self.last_launch = dict(lanes=len(kernels), launches=1, combines=0, pairs=0)
        return True

    def _run_shared(self, x, n: int, m_first: int, n_out: int, outs: list, halo, edge_stream=None, interior_only: bool = False):
        kernels = [c._kernel for c in self.chans]
        consumed = self.chans[0].consumed
        big, big_frames, big_consumed = x, n, consumed
        if halo is not None:
            big, lead = halo
            big_frames, big_consumed = int(big.numel()) // 2, consumed - int(lead)
        spans = [k._interior(big_consumed, big_frames, m_first, n_out) for k in kernels]
        m_a, m_b = max(s[0] for s in spans), min(s[1] for s in spans)
        if interior_only:
            if any(s != (m_first, m_first + n_out) for s in spans):
                return None
        elif any(s[1] <= s[0] for s in spans) or m_b - m_a < _ChannelKernel.mfma_min_outputs:
            return None
        n_int = m_b - m_a
        plans = [k._ensure_mfma() for k in kernels]
        if len({tuple((ps.k_first, ps.k_count) for ps in mp.passes if ps.group == 0) for mp in plans}) != 1:
            return None
        zs = [o if o is not None else D.empty(n_out, "complex64") for o in outs]
        if not interior_only:  # each channel's own edges (history in front, end of block behind)
            for c, k, z in zip(self.chans, kernels, zs):
                k._edges(edge_stream, x, n, consumed, c._hist, m_first, m_a - m_first, z)
                k._edges(edge_stream, x, n, consumed, c._hist, m_b, m_first + n_out - m_b, z[m_b - m_first :])
        kranges = [(ps.k_first, ps.k_count) for ps in plans[0].passes if ps.group == 0]
        ids = [(ci, gi) for ci, mp in enumerate(plans) for gi in range(len(mp.groups))]  # lane identities
        need_partial = {(ci, gi): (len(kranges) > 1 or len(plans[ci].groups) > 1) for ci, gi in ids}
        # single k-step range: a tap-row group's partial sums travel as the exact int32 pairs (8 B per output) and the
        # combine kernel scales them; chained k-step ranges -- and lanes with 64-bit sums -- hand on double2 sums (16 B)
        acc32 = bool(kernels[0].acc32)
        raw = len(kranges) == 1 and acc32
        partial = {key: D.empty(2 * n_int, "int32" if raw else "float64") for key, needed in need_partial.items() if needed}
        cpx = max(1, _ChannelKernel.launch_blocks // 8)  # CUs per XCD class the launch may fill
        launches = 0

        def launch(part, pairs: bool, units: int) -> None:
            """One launch per k-step range for the lanes ``part``; ``units`` workgroups share a stretch of the capture."""
            nonlocal launches
            rng = _block_size(n_int, 8 * max(1, cpx // units), 128)
            for ri, (k_first, _) in enumerate(kranges):
                lanes = []
                for ident in part:
                    if ident is None:  # the empty half of an odd pair
                        lanes.append(None)
                        continue
                    ci, gi = ident
                    mp = plans[ci]
                    ps = next(p_ for p_ in mp.passes if p_.group == gi and p_.k_first == k_first)
                    fin = ri == len(kranges) - 1 and len(mp.groups) == 1
                    buf = partial.get((ci, gi))
                    lanes.append((kernels[ci], ps, zs[ci][m_a - m_first :].data_ptr() if fin else None,
                                  buf.data_ptr() if (buf is not None and ri > 0) else None, None if fin else buf.data_ptr(),
                                  raw and not fin))
                _launch_lanes(lanes, pairs, rng, big, big_frames, big_consumed, m_a, n_int)
                launches += 1

        # Two lanes to a workgroup where the kernel offers it (contiguous ring slots without loader waves: 9..16 k steps):
        # both read every staged tile of the capture -- half the L2 -> LDS traffic per lane and a ring twice as deep in
        # rounds.  A pair's first lane has the larger (or the same) tap-row group: lanes in descending group order, two
        # by two; an odd lane out shares its workgroup with nobody (None).  ONE launch either way: the capture crosses
        # HBM once.
        if self.pair_lanes and len(kranges) == 1 and (N.lib().iqa_mfma_ring_lanes(P.FMT_CODE[self.fmt], self.decimation, *kranges[0], int(acc32)) & 2):
            paired = sorted(ids, key=lambda i: -plans[i[0]].groups[i[1]].q)
            if len(paired) & 1:
                paired.append(None)
            for lo in range(0, len(paired), self.MAX_LANES):
                part = paired[lo : lo + self.MAX_LANES]
                launch(part, True, len(part) // 2)
            n_pairs = len(paired) // 2
        else:
            n_pairs = 0
            for lo in range(0, len(ids), self.MAX_LANES):
                part = ids[lo : lo + self.MAX_LANES]
                launch(part, False, len(part))
        main = None
        if edge_stream is not None and any(len(mp.groups) > 1 for mp in plans):
            # the combine launches go where the consumers of the outputs are queued (behind the pass): the caller's stream
            # then holds the pass alone.  (No stream calls at all otherwise: this function also runs inside graph captures,
            # where a set_stream -- even to the current stream -- made the replays 2.5x slower.)
            torch = D.torch_mod()
            main = torch.cuda.current_stream()
            passed = torch.cuda.Event()
            passed.record(main)
            edge_stream.wait_event(passed)
            for t in partial.values():
                t.record_stream(edge_stream)
            torch.cuda.set_stream(edge_stream)
        try:
            combines = self._combine(plans, kernels, partial, raw, m_a, m_first, n_int, zs)
        finally:
            if main is not None:
                D.torch_mod().cuda.set_stream(main)
        self.last_launch = dict(lanes=len(ids), launches=launches, combines=combines, pairs=n_pairs)
        return zs

    def _combine(self, plans, kernels, partial, raw, m_a, m_first, n_int, zs) -> int:
        combines = 0
        for ci, mp in enumerate(plans):
            if len(mp.groups) > 1:
                ptrs = (c_void_p * len(mp.groups))(*[partial[(ci, gi)].data_ptr() for gi in range(len(mp.groups))])
                scale = None
                if raw:
                    vals = []
                    for gi in range(len(mp.groups)):
                        ps = next(p_ for p_ in mp.passes if p_.group == gi)
                        vals += [_tap_unit(mp.groups[gi], self.fmt), ps.c_re, ps.c_im]
                    scale = (c_double * len(vals))(*vals)
                N.call("iqa_mfma_combine", byref(kernels[ci].params), ptrs, c_int32(len(mp.groups)), scale, c_int64(m_a),
                       c_int64(n_int), N.ptr(zs[ci][m_a - m_first :]), N.stream_ptr())
                combines += 1
        return combines
