"""What the found channels are (``--find-describe``): from the finder's channel list to a label and a
suggested ``--demod``, ``--bw`` and tuned frequency per channel.

A second pass over the capture: every channel the finder kept goes through a channelizer at its own offset (the channels
that share a decimation through one ``ChannelBank``), and ``iqa_describe_accumulate`` reduces the baseband to eight integer
sums, counting only the samples of the slices in which the finder saw the channel on.  The figures (envelope variation, AM
depth, carrier offset, RMS deviation, carrier line share, in-channel carrier-to-noise ratio) are formed on the host in
float64 from those integers and from the finder's planes; the label and the suggestion follow from fixed rules.  Behind the
quantiser everything is integer: the sums do not depend on how the stream is cut.  No CPU path: without a GPU or the built
library the calls raise ``RuntimeError``.

With ``keying=True`` (``--find-decode``) the same pass also measures whether each channel's discriminator
switches on a symbol clock: ``iqa_quadrature`` and ``iqa_keying_accumulate`` give, per window of 2048 samples, the gated pairs,
the level crossings and the crossings' clock-phase sums at seven candidate bauds.  Fixed rules turn them into ``fsk <baud>`` or
``unkeyed`` and into the side decoders a target of that channel runs with.

With ``identify=True`` beside it (``--find-identify``) the pass keeps every channel's discriminator output
from the keyed-from block on, and ``finish_identify`` searches the channels labelled ``fsk 1600 | 2400 | 3200 | 4800`` for the
frame synchronisation words of their family (``identify.py``).  With ``flex=True`` beside that (``--find-flex``, DESIGN.md section
26) ``finish_flex`` decodes the pages behind the FLEX sync words among those hits (``flex.py``)."""
from __future__ import annotations

import logging
import math
from ctypes import c_int32, c_int64
from dataclasses import asdict, dataclass, field

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P

LOG = logging.getLogger(__name__)

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
_RAW_DTYPE = {"s16": "int16", "u8": "uint8", "f32": "float32"}


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


# ---- keying: the host arithmetic ---------------------------------------------------------------------

# the rules' constants (design constants, as section 22's are)
KEYING_MIN_PAIRS = 1024  # gated pairs of the describe rows before the centre is taken
KEYING_MIN_CROSSINGS = 256
KEYING_MIN_COH = 0.35
KEYING_RATE_LOW, KEYING_RATE_HIGH = 0.25, 0.8  # crossings per second against the baud
AIRBAND_HZ = (117.975e6, 137.0e6)
AIS_BW = 25000.0
POCSAG_BAUDS = (512, 1200, 2400)
FLEX_BAUDS = (1600, 3200)
NFM_RATE, WFM_RATE = 96_000.0, 480_000.0  # the channel rates a target of that mode asks for where --fs-ch is unset


@dataclass
class ChannelKeying:
    offset_hz: float  # the finder's
    freq_hz: float | None
    described: str  # the label of section 22
    fs_ch: float  # the rate of the measured stream
    bauds: list  # the candidates
    coh: list  # per candidate: the coherence of the crossings with its clock; None where skipped or not measured
    rate_hz: float | None  # crossings per second of gated stream
    crossings: int
    pairs: int
    centre: int | None  # c, in 1 / 4096 rad per sample; None where the channel never held 1024 gated pairs
    label: str | None  # "fsk <baud>" or "unkeyed" for an nfm channel, None for every other
    baud: int | None
    decoders: list  # the side decoders a target of this channel runs with
    bw: float | None  # the suggested --bw (section 22's, 25 000 for fsk 9600)
    note: str  # why there is no decoder, where there is none

    def line(self) -> str:
        if self.label is None:
            head = f"not measured ({self.described})"
        else:
            known = [(v, b) for v, b in zip(self.coh, self.bauds) if v is not None]
            if not known or self.rate_hz is None:
                head = f"{self.label} (not measured, {self.crossings} crossings)"
            elif self.baud is not None:
                head = f"{self.label} (coh {self.coh[self.bauds.index(self.baud)]:.2f}, {self.rate_hz:.0f} crossings/s)"
            else:
                best, at = max(known)
                head = f"{self.label} (best coh {best:.2f} at {at}, {self.rate_hz:.0f} crossings/s)"
        if not self.decoders:
            return f"    keying: {head} -> {self.note or 'no decoder'}"
        flags = " ".join(f"--{name}" for name in self.decoders)
        return f"    keying: {head} -> {flags}" + (f" --bw {self.bw:.0f}" if "ais" in self.decoders else "")

    def to_json(self) -> dict:
        return asdict(self)


@dataclass
class KeyingResult:
    channels: list = field(default_factory=list)  # ChannelKeying, in the order of the FindResult's channels
    sample_rate: float = 0.0
    center_freq: float | None = None

    def lines(self) -> list:
        return [ch.line() for ch in self.channels]

    def to_json(self) -> dict:
        return asdict(self)

    @classmethod
    def from_json(cls, data: dict) -> "KeyingResult":
        data = dict(data)
        data["channels"] = [ChannelKeying(**ch) for ch in data.get("channels", [])]
        return cls(**data)


def keying_centre(cr: int, ci: int) -> int:
    """c = rint(atan2(CI, CR) 4096): the mean rotation per sample in the quantiser's units (float64, half-even)."""
    return int(np.rint(math.atan2(int(ci), int(cr)) * P.KEYING_SCALE))


def add_keying_rows(parts, windows: int) -> np.ndarray:
    """int64[windows][16]: the rows of every call (``parts``: (first window, int32[k][16]) each) added by window number."""
    out = np.zeros((int(windows), P.KEYING_SUMS), dtype=np.int64)
    for first, rows in parts:
        rows = np.asarray(rows, dtype=np.int64).reshape(-1, P.KEYING_SUMS)
        out[first : first + rows.shape[0]] += rows
    return out


def _exact_sum(values: np.ndarray) -> int:
    """The sum of int64 values below 2^44 as a Python integer: 2^19 at a time in int64, the partial sums added exactly."""
    step = 1 << 19
    return sum(int(values[a : a + step].sum(dtype=np.int64)) for a in range(0, values.size, step))


def keying_figures(rows, plan: P.KeyingPlan) -> dict:
    """coh per candidate, rate_hz, crossings and pairs from the window rows (added by window number): exact integer sums
    (every term below 2^44), then one float64 quotient each."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, P.KEYING_SUMS)
    pairs, crossings = _exact_sum(rows[:, 0]), _exact_sum(rows[:, 1])
    den = 1024 * 1024 * _exact_sum(rows[:, 1] * rows[:, 1] - rows[:, 1])
    coh = []
    for k, skip in enumerate(plan.skipped):
        if skip or den == 0:
            coh.append(None)
            continue
        c, q = rows[:, 2 + 2 * k], rows[:, 3 + 2 * k]
        coh.append((_exact_sum(c * c + q * q) - 1024 * 1024 * crossings) / den)
    return dict(coh=coh, rate_hz=crossings / pairs * plan.fs_ch if pairs else None, crossings=crossings, pairs=pairs)


def keying_label(coh, rate_hz, crossings: int, plan: P.KeyingPlan) -> tuple:
    """("fsk <baud>", baud) for the lowest candidate whose clock the crossings keep and whose rate fits, else ("unkeyed", None)."""
    if crossings < KEYING_MIN_CROSSINGS or rate_hz is None:
        return "unkeyed", None
    for b, v, skip in zip(plan.bauds, coh, plan.skipped):
        if not skip and v is not None and v >= KEYING_MIN_COH and KEYING_RATE_LOW * b <= rate_hz <= KEYING_RATE_HIGH * b:
            return f"fsk {b}", b
    return "unkeyed", None


def decoders_for(described: str, baud, tuned_hz) -> tuple:
    """(side decoders, note, --bw override or None) of a channel: ``described`` the label of section 22, ``baud`` the keyed rate
    of an nfm channel or None, ``tuned_hz`` the suggested frequency or None."""
    if described == "nfm":
        if baud in POCSAG_BAUDS:
            return ["pocsag"], "", None
        if baud == 9600:
            return ["ais"], "", AIS_BW
        if baud in FLEX_BAUDS:
            return [], "FLEX rates: no decoder here", None
        if baud == 4800:
            return [], "4800 baud (DMR / P25 / NXDN class): no decoder here", None
        return ["ax25", "tones"], "", None
    if described == "wfm":
        return ["rds"], "", None
    if described == "am":
        if tuned_hz is not None and AIRBAND_HZ[0] <= tuned_hz <= AIRBAND_HZ[1]:
            return ["acars"], "", None
        return [], "no decoder outside the airband" if tuned_hz is not None else "no decoder without a tuned frequency", None
    return [], "no decoder", None


def target_rate(sample_rate: float, demod: str | None, fs_ch: float | None = None) -> float:
    """The channel rate a target of ``demod`` runs at: what the pipeline makes of ``--fs-ch`` (unset: the mode's default)."""
    ask = float(fs_ch) if fs_ch is not None else (WFM_RATE if demod == "wfm" else NFM_RATE)
    return P.choose_decimation(float(sample_rate), ask)[1]


def usable_decoders(names, rate: float, where: str = "") -> list:
    """``names`` without the decoders whose plan refuses the channel rate ``rate`` (the refusal is logged)."""
    from .decoders.side import SIDE_DECODERS

    rows = {e.name: e for e in SIDE_DECODERS}
    kept = []
    for name in names:
        try:
            rows[name].plan(rate)
        except ValueError as exc:
            LOG.info("%s--%s dropped: %s", where, name, exc)
            continue
        kept.append(name)
    return kept


def key_channel(desc: ChannelDescription, plan: P.KeyingPlan, rows, centre, sample_rate: float,
                fs_ch: float | None = None) -> ChannelKeying:
    """One channel's keying from its description, its window rows (None: never measured) and its centre."""
    figures = dict(coh=[None] * len(plan.bauds), rate_hz=None, crossings=0, pairs=0)
    if rows is not None and centre is not None:
        figures = keying_figures(rows, plan)
    label = baud = None
    if desc.label == "nfm":
        label, baud = keying_label(figures["coh"], figures["rate_hz"], figures["crossings"], plan)
    names, note, bw = decoders_for(desc.label, baud, desc.tuned_hz)
    where = f"{desc.offset_hz:+.0f} Hz: " if desc.freq_hz is None else f"{desc.freq_hz:.0f} Hz: "
    names = usable_decoders(names, target_rate(sample_rate, desc.demod, fs_ch), where)
    return ChannelKeying(offset_hz=desc.offset_hz, freq_hz=desc.freq_hz, described=desc.label, fs_ch=plan.fs_ch, bauds=list(plan.bauds),
                         centre=centre, label=label, baud=baud, decoders=names, bw=desc.bw if bw is None else bw, note=note, **figures)


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


def accumulate_keying(theta, pos: int, front, centre: int, kplan: P.KeyingPlan, table_dev, plan: P.DescribePlan, find_plan: P.FindPlan,
                      gate_dev):
    """``iqa_keying_accumulate`` for one stretch of a channel's discriminator output (device float32): (first window, the
    device rows int32[windows][16]).  The entry point checks its arguments before it launches (``ValueError``)."""
    n = int(theta.numel())
    rows = D.empty(int(N.lib().iqa_keying_windows(pos, n)) * P.KEYING_SUMS, "int32")
    incs = (c_int32 * len(kplan.incs))(*kplan.incs)
    N.call("iqa_keying_accumulate", N.ptr(theta), c_int64(n), c_int64(pos), N.ptr(front), c_int32(centre), incs, N.ptr(table_dev),
           c_int32(plan.decimation), c_int32(plan.delay), c_int32(find_plan.hop), c_int32(find_plan.slice_frames),
           c_int64(find_plan.frames), c_int32(find_plan.slices), N.ptr(gate_dev), N.ptr(rows), N.stream_ptr())
    return pos // P.KEYING_WINDOW, rows


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
    ``fin`` is ``ChannelFinder.finish()`` of the same capture and ``channels`` the ``FoundChannel``s made from it."""

    def __init__(self, find_plan: P.FindPlan, fin: dict, channels, fmt: str = "s16", iq_order: str = "iq", *, keep_stages: bool = False,
                 keying: bool = False, identify: bool = False, flex: bool = False):
        if fmt not in _RAW_DTYPE:
            raise ValueError(f"Unsupported sample format '{fmt}'")
        if iq_order not in N.ORDER:
            raise ValueError(f"Unsupported iq_order '{iq_order}'")
        if identify and not keying:
            raise ValueError("identify=True needs keying=True")
        if flex and not identify:
            raise ValueError("flex=True needs identify=True")
        self._identify, self._flex = bool(identify), bool(flex)
        self.find_plan, self.fin, self.channels = find_plan, fin, list(channels)
        self.fmt, self.iq_order, self._keep, self._keying = fmt, iq_order, keep_stages, bool(keying)
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
        self._fin = None
        self._kfin = None
        self._ifin = None
        self._xfin = None
        self._keyed: dict = {}  # identify: the last ``keying()`` per centre frequency, so that the protocols do not key again

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
        self._fin = self._kfin = self._ifin = self._xfin = None
        self._keyed = {}
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
            if lane.run[0] >= KEYING_MIN_PAIRS:
                lane.centre = keying_centre(lane.run[1], lane.run[2])
        if lane.centre is not None:
            if lane.keyed_from is None:
                lane.keyed_from = lane.pos
            lane.krows.append(accumulate_keying(theta, lane.pos, lane.front if lane.pos >= 1 else None, lane.centre, lane.kplan,
                                                self._table, lane.plan, self.find_plan, lane.gate_dev))
            if self._identify:
                lane.stored.append(theta)
        lane.front = theta[n - 1 :].clone()
        if self._keep:
            lane.theta.append(theta)

    def lanes(self) -> list:
        """The lanes of the pass in channel order (made by the first block; for the tests)."""
        if self._lanes is None:
            self._start()
        return self._lanes

    def finish(self) -> list:
        """The eight sums of every channel (Python integers), in channel order."""
        if self.samples_seen != self.find_plan.n_samples:
            raise ValueError(f"the plan was made for {self.find_plan.n_samples} samples and the stream held {self.samples_seen}")
        if self._fin is None:
            torch = D.torch_mod()
            self._fin = [add_rows(torch.cat(lane.rows).cpu().numpy()) if lane.rows else (0,) * len(SUMS) for lane in self.lanes()]
        return self._fin

    def _gated(self, lane: "_Lane", pos: int, n: int) -> bool:
        """Whether any slice that the samples pos .. pos + n - 1 of the lane's stream lie in is on."""
        p = self.find_plan
        first, last = (min(max(m * lane.plan.decimation - lane.plan.delay, 0) // p.hop, p.frames - 1) // p.slice_frames
                       for m in (pos, pos + n - 1))
        return bool(lane.gate[first : last + 1].any())

    def finish_keying(self) -> list:
        """Per channel the keying rows added by window number (int64[windows][16]), or None where the channel never held 1024
        gated pairs; in channel order."""
        if not self._keying:
            raise ValueError("the describer was made without keying=True")
        self.finish()
        if self._kfin is None:
            torch = D.torch_mod()
            self._kfin = []
            for lane in self.lanes():
                if lane.centre is None:
                    self._kfin.append(None)
                    continue
                flat = torch.cat([rows for _, rows in lane.krows]).cpu().numpy().reshape(-1, P.KEYING_SUMS)  # one read-back per channel
                ends = np.cumsum([int(rows.numel()) // P.KEYING_SUMS for _, rows in lane.krows])
                parts = [(first, flat[end - int(rows.numel()) // P.KEYING_SUMS : end]) for (first, rows), end in zip(lane.krows, ends)]
                self._kfin.append(add_keying_rows(parts, -(-lane.pos // P.KEYING_WINDOW)))
        return self._kfin

    def keying(self, center_freq: float | None = None, fs_ch: float | None = None) -> list:
        """The ``ChannelKeying`` of every channel, in channel order.  ``fs_ch``: an explicit ``--fs-ch`` of the targets."""
        rows = self.finish_keying()
        described = self.result(center_freq)
        out = [key_channel(d, lane.kplan, r, lane.centre, self.find_plan.fs, fs_ch)
               for d, lane, r in zip(described.channels, self.lanes(), rows)]
        if self._identify:
            self._keyed[center_freq] = list(out)
        return out

    def finish_identify(self) -> list:
        """Per channel a dict of its identification: ``rate`` (R, None where the channel is not one to
        identify), ``plan`` (the ``IdentPlan``, None where the rate does not fit), ``note``, ``hits`` (int64[K][6], the kept sync
        words sorted by (pattern, m), m counted from ``keyed_from``; None where nothing was searched) and, with ``keep_stages``,
        ``v`` and ``score`` (device tensors).  The whole search runs here, on the stored stream as one piece."""
        from . import identify as I

        if not self._identify:
            raise ValueError("the describer was made without identify=True")
        if self._ifin is None:
            torch = D.torch_mod()
            out = []
            # (label and baud depend neither on the centre frequency nor on the targets' rate: any keying of this pass will do)
            for lane, keyed in zip(self.lanes(), next(iter(self._keyed.values())) if self._keyed else self.keying()):
                rate, plan, note = I.family_plan(keyed.label, keyed.baud if keyed.label is not None else None, lane.plan.fs_ch)
                d = dict(rate=rate, plan=plan, note=note, hits=None)
                if plan is not None and lane.centre is not None and lane.stored:
                    theta = lane.stored[0] if len(lane.stored) == 1 else torch.cat(lane.stored)
                    if int(theta.numel()) > P.IDENT_MAX_N:
                        raise ValueError(f"a stored stream of {int(theta.numel())} samples is longer than 2^30")
                    v = I.integrate(theta, plan, lane.centre)
                    score, d["hits"] = I.search(v, plan, I.patterns_for(rate))
                    if self._keep:
                        d.update(v=v, score=score)
                    if self._flex and rate == 1600:
                        d["flex_v"] = v  # (section 26 reads the same plane)
                out.append(d)
            self._ifin = out
        return self._ifin

    def finish_flex(self) -> list:
        """Per channel the output of ``flex.decode_stream`` with ``plan`` (the ``FlexPlan``) and ``note``,
        or a dict of ``note`` alone where nothing is decoded: the channel is not of the 1600 family, its rate does not fit or
        nothing was searched.  It reuses the hits of ``finish_identify`` and runs no second search."""
        from . import flex as X
        from . import identify as I

        if not self._flex:
            raise ValueError("the describer was made without flex=True")
        if self._xfin is None:
            torch = D.torch_mod()
            out = []
            for lane, d in zip(self.lanes(), self.finish_identify()):
                if d["rate"] != 1600:
                    out.append(dict(note="no flex channel"))
                    continue
                try:
                    plan = P.plan_flex(lane.plan.fs_ch)
                except ValueError:
                    plan = None
                if plan is None or d["hits"] is None:
                    out.append(dict(note="rate does not fit" if plan is None or d["plan"] is None else "not measured"))
                    continue
                theta = lane.stored[0] if len(lane.stored) == 1 else torch.cat(lane.stored)
                st = X.decode_stream(theta, plan, lane.centre, d["hits"], I.patterns_for(1600), d["flex_v"])
                st.update(plan=plan, note="")
                out.append(st)
            self._xfin = out
        return self._xfin

    def flex_result(self, center_freq: float | None = None):
        from . import flex as X

        chans = []
        for ch, lane, st in zip(self.channels, self.lanes(), self.finish_flex()):
            freq = None if center_freq is None else center_freq + ch.offset_hz
            if "rows" not in st:
                chans.append(X.FlexChannel(offset_hz=ch.offset_hz, freq_hz=freq, note=st["note"]))
            else:
                chans.append(X.channel_of(st, lane.plan.fs_ch, lane.keyed_from, ch.offset_hz, freq))
        return X.FlexResult(channels=chans, sample_rate=self.find_plan.fs, center_freq=center_freq)

    def protocols(self, center_freq: float | None = None) -> list:
        """The ``ChannelProtocol`` of every channel, in channel order."""
        from . import identify as I

        found = self.finish_identify()
        return [I.protocol_of(keyed, d["hits"], d["plan"], d["rate"], d["note"], lane.keyed_from)
                for keyed, d, lane in zip(self._keyed.get(center_freq) or self.keying(center_freq), found, self.lanes())]

    def protocol_result(self, center_freq: float | None = None):
        from . import identify as I

        return I.ProtocolResult(channels=self.protocols(center_freq), sample_rate=self.find_plan.fs, center_freq=center_freq)

    def keying_result(self, center_freq: float | None = None, fs_ch: float | None = None) -> KeyingResult:
        return KeyingResult(channels=self.keying(center_freq, fs_ch), sample_rate=self.find_plan.fs, center_freq=center_freq)

    def result(self, center_freq: float | None = None) -> DescribeResult:
        sums = self.finish()
        out = [describe_channel(self.find_plan, self.fin, ch, gate, s, plan, center_freq)
               for ch, gate, s, plan in zip(self.channels, self.gates, sums, self.plans)]
        return DescribeResult(channels=out, sample_rate=self.find_plan.fs, center_freq=center_freq)

    def stages(self) -> list:
        """One dict per channel: sums, sh, gate, plan and, with ``keep_stages``, ``z`` (complex64, the whole channel stream) and
        ``rows`` (int64[tiles of every call][8]).  With ``keying``: ``c`` (the centre or None), ``keyed_from`` (the position of the
        first keyed sample), ``keying_rows`` (int64[windows][16], added by window number, or None) and, with ``keep_stages``,
        ``theta`` (float32, the whole discriminator output), ``keying_parts`` ((first window, int32[k][16]) per call) and
        ``calls`` (the samples of every feed).  With ``identify``: ``ident_rate``, ``ident_plan``, ``hits`` (int64[K][6] or None) and,
        with ``keep_stages``, ``v`` (int32[n]) and ``score`` (int32[patterns][n]) of the identified channels, ``stored`` (float32,
        the stored theta: ``theta`` from ``keyed_from`` on).  With ``flex``: ``flex_frames`` ((m, s, mode) per decoded frame, None where
        the channel is no FLEX channel) and, with ``keep_stages``, ``flex_words``, ``flex_raw``, ``flex_status`` ([F][5][4][88]),
        ``flex_chosen``, ``flex_rec16``, ``flex_rec32``, ``flex_ok``, ``flex_v32`` and ``flex_plan``."""
        sums = self.finish()
        torch = D.torch_mod()
        out = []
        krows = self.finish_keying() if self._keying else None
        for j, (lane, s) in enumerate(zip(self.lanes(), sums)):
            d = dict(sums=s, sh=lane.sh, gate=lane.gate, plan=lane.plan)
            if self._keying:
                d.update(c=lane.centre, keyed_from=lane.keyed_from, keying_rows=krows[j], keying_plan=lane.kplan)
                if self._keep:
                    d["theta"] = torch.cat(lane.theta).cpu().numpy() if lane.theta else np.zeros(0, dtype=np.float32)
                    d["keying_parts"] = [(first, rows.cpu().numpy().reshape(-1, P.KEYING_SUMS)) for first, rows in lane.krows]
            if self._identify:
                i = self.finish_identify()[j]
                d.update(ident_rate=i["rate"], ident_plan=i["plan"], hits=i["hits"])
                if self._keep:
                    d["stored"] = torch.cat(lane.stored).cpu().numpy() if lane.stored else np.zeros(0, dtype=np.float32)
                    if "v" in i:
                        d.update(v=i["v"].cpu().numpy(), score=i["score"].cpu().numpy())
            if self._flex:
                x = self.finish_flex()[j]
                d["flex_frames"] = x.get("rows")
                if self._keep and "rows" in x:
                    d.update(flex_plan=x["plan"], flex_rec16=x["rec16"], flex_rec32=x["rec32"], flex_ok=x["ok"], flex_words=x["fixed"],
                             flex_raw=x["raw"], flex_status=x["status"], flex_chosen=x["chosen"],
                             flex_v32=None if x["v32"] is None else x["v32"].cpu().numpy())
            if self._keep:
                d["calls"] = list(lane.calls)
            if self._keep:
                d["z"] = torch.cat(lane.z).cpu().numpy() if lane.z else np.zeros(0, dtype=np.complex64)
                d["rows"] = torch.cat(lane.rows).cpu().numpy().reshape(-1, len(SUMS)) if lane.rows else np.zeros((0, 8), dtype=np.int64)
            out.append(d)
        return out
