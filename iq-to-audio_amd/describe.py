"""What the found channels are (``--find-describe``): from the finder's channel list to a label and a
suggested ``--demod``, ``--bw`` and tuned frequency per channel.

A second pass over the capture: every channel the finder kept goes through a channelizer at its own offset (the channels
that share a decimation through one ``ChannelBank``), and ``iqa_describe_accumulate`` reduces the baseband to eight integer
sums, counting only the samples of the slices in which the finder saw the channel on.  The figures (envelope variation, AM
depth, carrier offset, RMS deviation, carrier line share, in-channel carrier-to-noise ratio) are formed on the host in
float64 from those integers and from the finder's planes; the label and the suggestion follow from fixed rules.  Behind the
quantiser everything is integer: the sums do not depend on how the stream is cut.  No CPU path: without a GPU or the built
library the calls raise ``RuntimeError``.

The layers above this one (``find_layers.ALL_LAYERS``, each in the module of its name) ride on the same pass: with ``keying=True``
it also takes every channel's discriminator and, once the channel holds 1024 gated pairs, its keying rows (``keying.py``); with
``identify=True`` it keeps that discriminator output for the sync-word search of ``identify.py``, whose hits the protocol layers
decode, each with its keyword (``flex=True``, ``dmr=True``, ...): a module with a ``LAYER`` (``protocol_layer.ProtocolLayer``), which
``finish_layer`` and ``layer_result`` run by name."""
from __future__ import annotations

import math
from ctypes import c_int32, c_int64
from dataclasses import asdict, dataclass, field
from importlib import import_module

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P
from . import identify as I
from . import keying as KY
from .find import _RAW_DTYPE
from .find_layers import ALL_LAYERS, active_layers

SUMS = ("N", "NP", "S1", "S2", "E", "CR", "CI", "A")
LABELS = ("nfm", "am", "ssb", "wfm", "carrier", "unknown")
MIX_SIGN = 1  # a tone at bin dc_bin + offset / bin_hz of the finder's spectrum comes to rest at 0 Hz

# the rules' constants (design constants, not measurements)
MIN_SAMPLES = 1024
MIN_CNR_DB = 26.0
WIDE_HZ = 100_000.0
WIDE_ENV = 0.05
FLAT_ENV = 0.02
CARRIER_DEV_HZ = 50.0
AM_LINE = 0.6
SSB_WIDTH_HZ = 6000.0
SSB_USB_FROM_HZ = 10e6
SSB_EDGE_HZ = 300.0


@dataclass
class ChannelDescription:
    offset_hz: float  # the finder's
    freq_hz: float | None
    width_hz: float
    label: str  # one of LABELS
    samples: int  # N: the gated samples of the channel stream
    fs_ch: float  # the rate of that stream
    cnr_db: float | None  # the run's power over the floor against the floor in the channel filter's bandwidth
    env: float | None  # var(|z|^2) / mean(|z|^2)^2: 0 for a constant envelope
    depth: float | None  # the AM depth a sine would need for this envelope
    carrier_hz: float | None  # the mean rotation against offset_hz
    dev_hz: float | None  # the RMS deviation about it
    line_share: float | None  # the share of the run's power in its strongest bin and its two neighbours
    demod: str | None  # the suggested --demod; None where the label is unknown
    bw: float | None  # the suggested --bw
    tuned_offset_hz: float | None  # the suggested tuning against the capture's centre
    tuned_hz: float | None  # centre + tuned_offset_hz; None without a centre frequency

    def line(self) -> str:
        if self.env is None:
            return f"    {self.label}: not measured ({self.samples} samples)"
        figures = (f"C/N {self.cnr_db:.1f} dB, env {self.env:.3f}, depth {self.depth:.2f}, carrier {self.carrier_hz:+.0f} Hz, "
                   f"dev {self.dev_hz:.0f} Hz, line {self.line_share:.2f}")
        if self.demod is None:
            return f"    {self.label}: {figures}"
        at = f"{self.tuned_offset_hz:+.0f} Hz" if self.tuned_hz is None else f"{self.tuned_hz:.0f} Hz"
        return f"    {self.label}: {figures} -> --demod {self.demod} --bw {self.bw:.0f} at {at}"

    def to_json(self) -> dict:
        return asdict(self)


@dataclass
class DescribeResult:
    channels: list = field(default_factory=list)  # ChannelDescription, in the order of the FindResult's channels
    sample_rate: float = 0.0
    center_freq: float | None = None

    def lines(self) -> list:
        return [ch.line() for ch in self.channels]

    def to_json(self) -> dict:
        return asdict(self)

    @classmethod
    def from_json(cls, data: dict) -> "DescribeResult":
        data = dict(data)
        data["channels"] = [ChannelDescription(**ch) for ch in data.get("channels", [])]
        return cls(**data)


# ---- the host arithmetic ----------------------------------------------------------------------------------------------------


def erode_gate(on) -> np.ndarray:
    """g[s] = on[s - 1] & on[s] & on[s + 1] with the ends taken as on: a slice counts only between two that are on."""
    on = (np.asarray(on).reshape(-1) != 0).astype(np.uint8)
    padded = np.concatenate(([1], on, [1])).astype(np.uint8)
    return padded[:-2] & padded[1:-1] & padded[2:]


def choose_shift(mean_power: float) -> int:
    """sh = clamp(10 - ceil(log2(rms)), -30, 30): the quantiser's scale, an RMS of about 2^10; 15 for a silent block."""
    if not (mean_power > 0.0):  # (zero, or not a number)
        return 15
    if math.isinf(mean_power):
        return -P.DESCRIBE_MAX_SHIFT
    rms = math.sqrt(mean_power)
    return int(min(max(10 - math.ceil(math.log2(rms)), -P.DESCRIBE_MAX_SHIFT), P.DESCRIBE_MAX_SHIFT))


def stream_figures(sums, fs_ch: float) -> dict | None:
    """env, depth, carrier_hz and dev_hz from the eight sums (Python integers); None where S1, E or A is zero."""
    n, _np, s1, s2, e, cr, ci, a = (int(v) for v in sums)
    if s1 == 0 or e == 0 or a == 0:
        return None
    env = n * s2 * 65536 / (s1 * s1) - 1.0  # (the quotient of two Python integers: rounded once)
    depth = math.sqrt(max(2.0 * (n * s1 / (e * e) - 1.0), 0.0))
    r = math.hypot(cr, ci) / a
    k = fs_ch / (2.0 * math.pi)
    return dict(env=env, depth=depth, carrier_hz=math.atan2(ci, cr) * k,
                dev_hz=math.sqrt(max(-2.0 * math.log(r), 0.0)) * k if r > 0.0 else math.inf)


def plane_figures(find_plan: P.FindPlan, fin: dict, lo: int, hi: int, gate, bw: float) -> dict | None:
    """line_share and cnr_db from the finder's slice and floor planes over the bins lo .. hi and the gated slices; None
    where no slice is gated."""
    gate = np.asarray(gate).reshape(-1) != 0
    if not gate.any():
        return None
    lens = np.array([find_plan.slice_len(s) for s in range(find_plan.slices)], dtype=np.int64)
    total = np.asarray(fin["slice"], dtype=np.int64)[gate, lo : hi + 1].sum(axis=0)
    m_on = total.astype(np.float64) / float(lens[gate].sum())
    lin = 10.0 ** (m_on / 1000.0)
    lin_f = 10.0 ** (np.asarray(fin["fmean"], dtype=np.float64)[lo : hi + 1] / 1000.0)
    at = int(np.argmax(lin))
    share = float(lin[max(at - 1, 0) : at + 2].sum() / lin.sum())
    over = max(float((lin - lin_f).sum()), 1e-30)
    return dict(line_share=share, cnr_db=10.0 * math.log10(over / (float(lin_f.mean()) * bw / find_plan.bin_hz)))


def label_of(samples: int, cnr_db, width_hz: float, env, dev_hz, line_share) -> str:
    """The first rule that holds."""
    if env is None or cnr_db is None or samples < MIN_SAMPLES or cnr_db < MIN_CNR_DB:
        return "unknown"
    if width_hz >= WIDE_HZ:
        return "wfm" if env < WIDE_ENV else "unknown"
    if env < FLAT_ENV:
        return "carrier" if dev_hz < CARRIER_DEV_HZ else "nfm"
    if line_share >= AM_LINE:
        return "am"
    if width_hz < SSB_WIDTH_HZ:
        return "ssb"
    return "unknown"


def suggestion(label: str, *, offset_hz: float, carrier_hz, width_hz: float, freq_hz, lo_bin: int, hi_bin: int, dc_bin: int,
               bin_hz: float):
    """(demod, bw, tuned offset) of a label; (None, None, None) for unknown."""
    if label in ("nfm", "carrier"):
        return "nfm", 25000.0 if width_hz > 16000.0 else 12500.0, offset_hz + carrier_hz
    if label == "am":
        return "am", 10000.0, offset_hz + carrier_hz
    if label == "wfm":
        return "wfm", 250000.0, offset_hz + carrier_hz
    if label == "ssb":
        if freq_hz is None or freq_hz >= SSB_USB_FROM_HZ:
            return "usb", 3000.0, (lo_bin - dc_bin) * bin_hz - SSB_EDGE_HZ
        return "lsb", 3000.0, (hi_bin + 1 - dc_bin) * bin_hz + SSB_EDGE_HZ
    return None, None, None


def describe_channel(find_plan: P.FindPlan, fin: dict, channel, gate, sums, plan: P.DescribePlan,
                     center_freq: float | None = None) -> ChannelDescription:
    """One channel's description from its sums, its gate and the finder's planes."""
    stream = stream_figures(sums, plan.fs_ch)
    planes = plane_figures(find_plan, fin, channel.lo_bin, channel.hi_bin, gate, plan.bw)
    figures = dict(env=None, depth=None, carrier_hz=None, dev_hz=None, line_share=None, cnr_db=None)
    if stream is not None and planes is not None:
        figures = {**stream, **planes}
    freq = None if center_freq is None else center_freq + channel.offset_hz
    label = label_of(int(sums[0]), figures["cnr_db"], channel.width_hz, figures["env"], figures["dev_hz"], figures["line_share"])
    demod, bw, tuned = suggestion(label, offset_hz=channel.offset_hz, carrier_hz=figures["carrier_hz"], width_hz=channel.width_hz,
                                  freq_hz=freq, lo_bin=channel.lo_bin, hi_bin=channel.hi_bin, dc_bin=find_plan.dc_bin,
                                  bin_hz=find_plan.bin_hz)
    return ChannelDescription(offset_hz=channel.offset_hz, freq_hz=freq, width_hz=channel.width_hz, label=label, samples=int(sums[0]),
                              fs_ch=plan.fs_ch, demod=demod, bw=bw, tuned_offset_hz=tuned,
                              tuned_hz=None if tuned is None or center_freq is None else center_freq + tuned, **figures)


def select_auto_targets(found, described: DescribeResult, top: int, grid_hz: float = 1.0, extras=None) -> tuple:
    """(targets, skipped) for ``--find-auto``: the ``top`` channels of highest ``snr_db`` (ties to the lower frequency) whose
    label is not unknown, each as (frequency rounded to ``grid_hz``, demod, bw), duplicates of a frequency dropped, ascending;
    ``skipped`` are the unknown channels that stood in front of the last one taken.  Needs a centre frequency.  ``extras``:
    one value per channel, carried as a fourth entry of its target (the side decoders of ``--find-decode``)."""
    if described.center_freq is None or any(ch.freq_hz is None for ch in found.channels):
        raise ValueError("the targets need a centre frequency")
    grid = float(grid_hz)
    order = sorted(range(len(found.channels)), key=lambda i: (-found.channels[i].snr_db, found.channels[i].freq_hz))
    targets, skipped = {}, []
    for i in order:
        if len(targets) >= max(int(top), 0):
            break
        d = described.channels[i]
        if d.label == "unknown":
            skipped.append(found.channels[i])
            continue
        freq = math.floor(d.tuned_hz / grid + 0.5) * grid
        targets.setdefault(freq, (freq, d.demod, d.bw) if extras is None else (freq, d.demod, d.bw, extras[i]))
    return sorted(targets.values()), skipped


# ---- the device pass --------------------------------------------------------------------------------------------------------


def accumulate(z, pos: int, prev, sh: int, plan: P.DescribePlan, find_plan: P.FindPlan, gate_dev):
    """``iqa_describe_accumulate`` for one stretch of a channel stream (device complex64): the device rows int64[tiles][8].
    The entry point checks its arguments before it launches (``ValueError``)."""
    n = int(z.numel())
    rows = D.empty(int(N.lib().iqa_describe_tiles(n)) * len(SUMS), "int64")
    N.call("iqa_describe_accumulate", N.ptr(z), c_int64(n), c_int64(pos), N.ptr(prev), c_int32(sh), c_int32(plan.decimation),
           c_int32(plan.delay), c_int32(find_plan.hop), c_int32(find_plan.slice_frames), c_int64(find_plan.frames),
           c_int32(find_plan.slices), N.ptr(gate_dev), N.ptr(rows), N.stream_ptr())
    return rows


def add_rows(rows: np.ndarray) -> tuple:
    """The column sums of int64[..][8] as Python integers (a whole run's S2 may pass 2^63)."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, len(SUMS))
    low = (rows & 0xFFFFFFFF).sum(axis=0, dtype=np.int64)  # (2^32 rows of 32 bits fit int64; so do the high halves)
    high = (rows >> 32).sum(axis=0, dtype=np.int64)
    return tuple((int(h) << 32) + int(l) for h, l in zip(high, low))


_MODULES = {layer.name: import_module(f"{__package__}.{layer.name}") for layer in ALL_LAYERS[1:]}  # a layer above the first lives in the module of its keyword


class _Lane:
    """One channel of the pass: its plan, gate and carried state."""

    def __init__(self, channel, plan: P.DescribePlan, gate: np.ndarray, chan):
        self.channel, self.plan, self.gate, self.chan = channel, plan, gate, chan
        self.gate_dev = D.from_numpy(gate)
        self.sh = None
        self.prev = None
        self.pos = 0
        self.rows: list = []
        self.z: list = []
        self.calls: list = []  # the samples of every feed
        # keying (section 23)
        self.kplan = None
        self.qprev = None  # iqa_quadrature's state
        self.front = None  # the theta in front of the next call
        self.centre = None
        self.run = [0, 0, 0]  # NP, CR, CI of the describe rows so far, until the centre is taken
        self.keyed_from = None  # the stream position of the first keyed sample
        self.krows: list = []  # (first window, device rows) per call
        self.theta: list = []
        self.stored: list = []  # identify (section 25): the theta of every block from the keyed-from one on


class ChannelDescriber:
    """The stage API: ``process(raw_block)`` per block of the capture (what ``ChannelFinder.process`` takes), ``finish()`` once
    (the eight sums of every channel), ``result()`` (a ``DescribeResult``), ``stages()`` for the tests, ``reset()``.
    ``fin`` is ``ChannelFinder.finish()`` of the same capture and ``channels`` the ``FoundChannel``s made from it.  ``layers``: the
    keywords of ``FIND_LAYERS`` above the first (``keying=True``, ``identify=True``, ``flex=True``), each with the one in front of
    it, and of ``FIND_BRANCHES`` (``dmr=True``, ``p25=True``, ``ysf=True``, ``nxdn=True``, with ``identify=True``).  Every protocol
    layer has its ``finish_<name>()`` and ``<name>_result(center_freq)``, installed below the class from the table."""

    def __init__(self, find_plan: P.FindPlan, fin: dict, channels, fmt: str = "s16", iq_order: str = "iq", *, keep_stages: bool = False,
                 **layers):
        if fmt not in _RAW_DTYPE:
            raise ValueError(f"Unsupported sample format '{fmt}'")
        if iq_order not in N.ORDER:
            raise ValueError(f"Unsupported iq_order '{iq_order}'")
        for name in layers:
            if name not in _MODULES:
                raise TypeError(f"ChannelDescriber() got an unexpected keyword argument '{name}'")
        self._names = tuple(layer.name for layer in active_layers({ALL_LAYERS[0].name: True, **layers}))  # this layer, then the others
        self.find_plan, self.fin, self.channels = find_plan, fin, list(channels)
        self.fmt, self.iq_order, self._keep, self._keying = fmt, iq_order, keep_stages, "keying" in self._names
        by_lo = {int(rec[0]): j for j, rec in enumerate(np.asarray(fin["runs"]).reshape(-1, 8))}
        self._run_of = []
        for ch in self.channels:
            if ch.lo_bin not in by_lo:
                raise ValueError(f"the channel at {ch.offset_hz:+.0f} Hz is no run of this finder")
            self._run_of.append(by_lo[ch.lo_bin])
        self.plans = [P.plan_describe(find_plan.fs, ch.offset_hz, ch.width_hz) for ch in self.channels]
        self.gates = [erode_gate(np.asarray(fin["on"])[j]) for j in self._run_of]
        self.kplans = [P.plan_keying(plan.fs_ch) for plan in self.plans] if self._keying else []
        self._table = None
        self.reset()

    def reset(self) -> None:
        """Back to a pass that has seen nothing."""
        self._lanes = None
        self._groups: list = []
        self.samples_seen = 0
        self._done: dict = {}  # what the finishes made of the blocks so far, by name

    def _start(self) -> None:
        from .channelizer import ChannelBank, Channelizer

        self._lanes = []
        for ch, plan, gate in zip(self.channels, self.plans, self.gates):
            chan = Channelizer(plan.taps, sample_rate=plan.fs, freq_offset=plan.offset_hz, mix_sign=MIX_SIGN, decimation=plan.decimation,
                               fmt=self.fmt, iq_order=self.iq_order, precision="fast")
            self._lanes.append(_Lane(ch, plan, gate, chan))
        if self._keying:
            if self._table is None:
                self._table = D.from_numpy(np.ascontiguousarray(self.kplans[0].table))
            for lane, kplan in zip(self._lanes, self.kplans):
                lane.kplan = kplan
                lane.qprev = D.from_numpy(np.array([1.0, 0.0], dtype=np.float32))
        by_d: dict = {}
        for lane in self._lanes:
            by_d.setdefault(lane.plan.decimation, []).append(lane)
        # the channels of one decimation share the pass over the block; a single one goes alone
        self._groups = [(ChannelBank([l.chan for l in lanes]) if len(lanes) > 1 else None, lanes) for lanes in by_d.values()]

    def process(self, raw_block) -> None:
        x = D.to_device(raw_block, _RAW_DTYPE[self.fmt]).reshape(-1)
        if int(x.numel()) % 2:
            raise ValueError("a block holds whole I/Q frames: an even number of values")
        if int(x.numel()) == 0:
            return
        self.samples_seen += int(x.numel()) // 2
        if self.samples_seen > self.find_plan.n_samples:
            raise ValueError(f"the plan was made for {self.find_plan.n_samples} samples and the stream is longer")
        if self._lanes is None:
            self._start()
        self._done = {}
        for bank, lanes in self._groups:
            zs = bank.process(x) if bank is not None else [lanes[0].chan.process(x)]
            for lane, z in zip(lanes, zs):
                self.feed(lane, z)

    def feed(self, lane: "_Lane", z) -> None:
        """The next stretch of a lane's channel stream into its sums."""
        n = int(z.numel())
        if n == 0:
            return
        if lane.sh is None:
            power = D.empty(1, "float64")
            N.call("iqa_mean_power", N.ptr(z), c_int64(n), c_int64(0), N.ptr(power), N.stream_ptr())
            lane.sh = choose_shift(float(power.cpu().numpy()[0]))
        lane.rows.append(accumulate(z, lane.pos, lane.prev, lane.sh, lane.plan, self.find_plan, lane.gate_dev))
        if self._keying:
            self._feed_keying(lane, z, n)
        lane.prev = z[n - 1 :].clone()
        lane.pos += n
        if self._keep:
            lane.z.append(z)
            lane.calls.append(n)

    def _feed_keying(self, lane: "_Lane", z, n: int) -> None:
        """The discriminator of the stretch (its own state, carried) and, from the block whose describe rows bring the lane's
        gated pairs to 1024 on, its keying rows."""
        theta = D.empty(n, "float32")
        N.call("iqa_quadrature", N.ptr(z), c_int64(n), N.ptr(lane.qprev), N.ptr(theta), N.stream_ptr())
        if lane.centre is None and self._gated(lane, lane.pos, n):  # (a stretch without a gated sample adds no pair: no read-back)
            new = add_rows(lane.rows[-1].cpu().numpy())
            lane.run = [lane.run[0] + new[1], lane.run[1] + new[5], lane.run[2] + new[6]]
            if lane.run[0] >= KY.KEYING_MIN_PAIRS:
                lane.centre = KY.keying_centre(lane.run[1], lane.run[2])
        if lane.centre is not None:
            if lane.keyed_from is None:
                lane.keyed_from = lane.pos
            lane.krows.append(KY.accumulate_keying(theta, lane.pos, lane.front if lane.pos >= 1 else None, lane.centre, lane.kplan,
                                                   self._table, lane.plan, self.find_plan, lane.gate_dev))
            if "identify" in self._names:
                lane.stored.append(theta)
        lane.front = theta[n - 1 :].clone()
        if self._keep:
            lane.theta.append(theta)

    def lanes(self) -> list:
        """The lanes of the pass in channel order (made by the first block; for the tests)."""
        if self._lanes is None:
            self._start()
        return self._lanes

    def _once(self, name: str, make):
        """``make()`` of the blocks so far, made once: kept until the next block or ``reset()``."""
        if name not in self._done:
            self._done[name] = make()
        return self._done[name]

    def _need(self, name: str) -> None:
        if name not in self._names:
            raise ValueError(f"the describer was made without {name}=True")

    def finish(self) -> list:
        """The eight sums of every channel (Python integers), in channel order."""
        if self.samples_seen != self.find_plan.n_samples:
            raise ValueError(f"the plan was made for {self.find_plan.n_samples} samples and the stream held {self.samples_seen}")
        return self._once("sums", lambda: [add_rows(D.torch_mod().cat(lane.rows).cpu().numpy()) if lane.rows else (0,) * len(SUMS)
                                           for lane in self.lanes()])

    def _gated(self, lane: "_Lane", pos: int, n: int) -> bool:
        """Whether any slice that the samples pos .. pos + n - 1 of the lane's stream lie in is on."""
        p = self.find_plan
        first, last = (min(max(m * lane.plan.decimation - lane.plan.delay, 0) // p.hop, p.frames - 1) // p.slice_frames
                       for m in (pos, pos + n - 1))
        return bool(lane.gate[first : last + 1].any())

    # ---- the layers above: each a one-liner into its module, through the cache ----

    def finish_keying(self) -> list:
        """Per channel the keying rows added by window number (int64[windows][16]), or None where the channel never held 1024
        gated pairs; in channel order."""
        self._need("keying")
        self.finish()
        return self._once("keying", lambda: KY.finish_keying(self.lanes()))

    def keying(self, center_freq: float | None = None, fs_ch: float | None = None) -> list:
        """The ``ChannelKeying`` of every channel, in channel order.  ``fs_ch``: an explicit ``--fs-ch`` of the targets.  The last
        one per centre frequency is kept for the layers above, so that they do not key (and log a dropped decoder) again."""
        rows = self.finish_keying()
        described = self.result(center_freq)
        out = [KY.key_channel(d, lane.kplan, r, lane.centre, self.find_plan.fs, fs_ch)
               for d, lane, r in zip(described.channels, self.lanes(), rows)]
        self._done.setdefault("keyed", {})[center_freq] = list(out)
        return out

    def keying_result(self, center_freq: float | None = None, fs_ch: float | None = None) -> KY.KeyingResult:
        return KY.KeyingResult(channels=self.keying(center_freq, fs_ch), sample_rate=self.find_plan.fs, center_freq=center_freq)

    def finish_identify(self) -> list:
        """Per channel the dict of ``identify.finish_identify``, ``v`` also for a layer above that reads it."""
        self._need("identify")
        above = self._names[self._names.index("identify") + 1 :]
        rates = tuple(r for name in above for r in getattr(_MODULES[name], "PLANE_RATES", ()))
        # (label and baud depend neither on the centre frequency nor on the targets' rate: any keying of this pass will do)
        return self._once("identify", lambda: I.finish_identify(
            self.lanes(), next(iter(self._done.get("keyed", {}).values()), None) or self.keying(), self._keep, rates))

    def protocols(self, center_freq: float | None = None) -> list:
        """The ``ChannelProtocol`` of every channel, in channel order."""
        found = self.finish_identify()
        return I.protocols(self.lanes(), self._done.get("keyed", {}).get(center_freq) or self.keying(center_freq), found)

    def protocol_result(self, center_freq: float | None = None) -> I.ProtocolResult:
        return I.ProtocolResult(channels=self.protocols(center_freq), sample_rate=self.find_plan.fs, center_freq=center_freq)

    def finish_layer(self, name: str) -> list:
        """Per channel the dict of the ``LAYER.finish`` of the protocol layer ``name`` (``flex``, ``dmr``, ...)."""
        self._need(name)
        return self._once(name, lambda: _MODULES[name].LAYER.finish(self.lanes(), self.finish_identify()))

    def layer_result(self, name: str, center_freq: float | None = None):
        """The result object of the protocol layer ``name`` (``FlexResult``, ``DmrResult``, ...)."""
        return _MODULES[name].LAYER.result_of(self.channels, self.lanes(), self.finish_layer(name), self.find_plan.fs, center_freq)

    def result(self, center_freq: float | None = None) -> DescribeResult:
        sums = self.finish()
        out = [describe_channel(self.find_plan, self.fin, ch, gate, s, plan, center_freq)
               for ch, gate, s, plan in zip(self.channels, self.gates, sums, self.plans)]
        return DescribeResult(channels=out, sample_rate=self.find_plan.fs, center_freq=center_freq)

    def stages(self) -> list:
        """One dict per channel: sums, sh, gate, plan and, with ``keep_stages``, ``z`` (complex64, the whole channel stream), ``rows``
        (int64[tiles of every call][8]) and ``calls`` (the samples of every feed); then the keys of every layer above, in chain order
        (``stage_keys`` of its module)."""
        sums = self.finish()
        torch = D.torch_mod()
        out = []
        for j, (lane, s) in enumerate(zip(self.lanes(), sums)):
            d = dict(sums=s, sh=lane.sh, gate=lane.gate, plan=lane.plan)
            for name in self._names[1:]:
                d.update(_MODULES[name].stage_keys(self, j, lane, self._keep))
            if self._keep:
                d["calls"] = list(lane.calls)
                d["z"] = torch.cat(lane.z).cpu().numpy() if lane.z else np.zeros(0, dtype=np.complex64)
                d["rows"] = torch.cat(lane.rows).cpu().numpy().reshape(-1, len(SUMS)) if lane.rows else np.zeros((0, 8), dtype=np.int64)
            out.append(d)
        return out


def _install(layer) -> None:
    """``finish_<name>`` and ``<name>_result`` of ``ChannelDescriber`` for the protocol layer of the table's row ``layer``."""
    name = layer.name

    def finish(self) -> list:
        return self.finish_layer(name)

    def result(self, center_freq: float | None = None):
        return self.layer_result(name, center_freq)

    finish.__doc__ = f"Per channel the dict of ``{name}.finish_{name}`` (DESIGN.md section {layer.section})."
    result.__doc__ = f"The ``{_MODULES[name].LAYER.result.__name__}`` of the pass (DESIGN.md section {layer.section})."
    finish.__name__, result.__name__ = f"finish_{name}", f"{name}_result"
    setattr(ChannelDescriber, finish.__name__, finish)
    setattr(ChannelDescriber, result.__name__, result)


for _layer in ALL_LAYERS[1:]:
    if hasattr(_MODULES[_layer.name], "LAYER"):
        _install(_layer)
