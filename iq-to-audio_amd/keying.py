"""Keyed FSK against voice, and the side decoders of a found channel (``--find-decode``): from the window
rows of ``iqa_keying_accumulate`` over a channel's discriminator output in the second pass (``describe.py``) to ``fsk <baud>`` or
``unkeyed`` by fixed rules on exact integer sums, and to the side decoders a target of that channel runs with.  No CPU path."""
from __future__ import annotations

import logging
import math
from ctypes import c_int32, c_int64
from dataclasses import dataclass, field

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P
from .protocol_layer import JsonRecord

LOG = logging.getLogger(__name__)

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
class ChannelKeying(JsonRecord):
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


@dataclass
class KeyingResult(JsonRecord):
    channels: list = field(default_factory=list)  # ChannelKeying, in the order of the FindResult's channels
    sample_rate: float = 0.0
    center_freq: float | None = None
    NESTED = {"channels": ChannelKeying}

    def lines(self) -> list:
        return [ch.line() for ch in self.channels]


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


def key_channel(desc, plan: P.KeyingPlan, rows, centre, sample_rate: float, fs_ch: float | None = None) -> ChannelKeying:
    """One channel's keying from its description (section 22's ``ChannelDescription``), its window rows (None: never measured)
    and its centre."""
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


# ---- the device pass ----------------------------------------------------------------------------------------------------------


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


def finish_keying(lanes) -> list:
    """Per lane of the pass the keying rows added by window number (int64[windows][16]), or None where the channel never held
    1024 gated pairs."""
    torch = D.torch_mod()
    out = []
    for lane in lanes:
        if lane.centre is None:
            out.append(None)
            continue
        flat = torch.cat([rows for _, rows in lane.krows]).cpu().numpy().reshape(-1, P.KEYING_SUMS)  # one read-back per channel
        ends = np.cumsum([int(rows.numel()) // P.KEYING_SUMS for _, rows in lane.krows])
        parts = [(first, flat[end - int(rows.numel()) // P.KEYING_SUMS : end]) for (first, rows), end in zip(lane.krows, ends)]
        out.append(add_keying_rows(parts, -(-lane.pos // P.KEYING_WINDOW)))
    return out


def stage_keys(describer, j: int, lane, keep: bool) -> dict:
    """This layer's keys of ``ChannelDescriber.stages()`` for channel ``j``: ``c`` (the centre or None), ``keyed_from`` (the position
    of the first keyed sample), ``keying_rows`` (int64[windows][16], added by window number, or None), ``keying_plan`` and, with
    ``keep``, ``theta`` (float32, the whole discriminator output) and ``keying_parts`` ((first window, int32[k][16]) per call)."""
    d = dict(c=lane.centre, keyed_from=lane.keyed_from, keying_rows=describer.finish_keying()[j], keying_plan=lane.kplan)
    if keep:
        d["theta"] = D.torch_mod().cat(lane.theta).cpu().numpy() if lane.theta else np.zeros(0, dtype=np.float32)
        d["keying_parts"] = [(first, rows.cpu().numpy().reshape(-1, P.KEYING_SUMS)) for first, rows in lane.krows]
    return d
