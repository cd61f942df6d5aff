"""The side decoders: what runs beside a target's demodulator and ends in a result of its own (DESIGN.md sections 11 to 17).

``SIDE_DECODERS`` is the one place that lists them.  The pipelines, ``ChannelDemod``, the CLI and the batch runners read a
decoder's name, mode, plan, core, per-block source and output from its row; a new decoder is a row here, a keyword on the
constructors and its own module ("Adding a side decoder").  The row order is the order in which a block's
launches and a run's finishes are queued."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

from .. import dsp_plan as P
from .acars import AcarsCore
from .adsb import AdsbCore
from .ais import AisCore
from .ax25 import AfskCore
from .pocsag import PocsagCore
from .rds import RdsCore
from .tones import TonesCore

#: the ``--demod`` spellings a decoder's mode accepts
ACCEPTS = {"nfm": ("nfm", "fm"), "am": ("am",), "wfm": ("wfm",)}


@dataclass(frozen=True)
class SideDecoder:
    name: str  # the keyword, the CLI flag, the result attribute and the ``<stem>.<name>.json`` suffix
    mode: str  # the --demod mode it rides on: "nfm" (also spelt "fm"), "am" or "wfm"
    why: str  # the sentence that completes the mode error
    section: int  # its DESIGN.md section
    plan: Callable  # channel rate -> plan (ValueError where the rate does not fit)
    core: type  # core(plan): process(block input), reset(), finish(), result(**context)
    source: str | None  # what ``ChannelDemod`` feeds the core per block: "theta" (iqa_quadrature, own prev), "envelope"
    #                     (iqa_envelope), or None for rds, whose per-block wiring is ``WfmDemod``'s
    log: Callable  # result -> the run's log line
    lines: Callable  # (result or None, head) -> the lines the CLI prints; ``head`` is "<target frequency> Hz: "
    help: str  # the CLI flag's help text


def _per(items, label: str = ""):
    """The usual ``lines``: one ``line()`` per item of ``result.<items>``, nothing without a result."""
    return lambda res, head: [f"{head}{label}{x.line()}" for x in (getattr(res, items) if res is not None else [])]


def _ais_lines(res, head: str) -> list:
    """A message line, then its !AIVDM sentences as they are (no head: they are fed to chart plotters)."""
    return [line for msg in (res.messages if res is not None else []) for line in [f"{head}{msg.line()}", *msg.nmea]]


SIDE_DECODERS = (
    SideDecoder("rds", "wfm", "RDS rides on a broadcast FM multiplex", 11, P.plan_rds, RdsCore, None,
                lambda r: f"RDS {r.line()}",
                lambda res, head: [head + (res.line() if res is not None else "no RDS")],
                "With --demod wfm: decode RDS (PI, PS, RadioText) of every station and write <output stem>.rds.json."),
    SideDecoder("pocsag", "nfm", "POCSAG is 2-FSK on a narrowband FM channel", 12, P.plan_pocsag, PocsagCore, "theta",
                lambda r: f"POCSAG: {len(r.messages)} message(s), {sum(r.syncs.values())} sync word(s).",
                _per("messages"),
                "With --demod nfm: decode POCSAG pager traffic (512 / 1200 / 2400 baud) of every target, print one line "
                "per message and write <output stem>.pocsag.json."),
    SideDecoder("ax25", "nfm", "AX.25 here is Bell-202 AFSK on a narrowband FM channel", 13, P.plan_afsk, AfskCore, "theta",
                lambda r: f"AX.25: {len(r.frames)} frame(s), {r.crc_ok} CRC-passing candidate(s).",
                _per("frames", "AX25 "),
                "With --demod nfm: decode 1200-baud Bell-202 AX.25 frames (APRS, packet) of every target, print one TNC2-style "
                "line per frame and write <output stem>.ax25.json."),
    SideDecoder("tones", "nfm", "CTCSS and DTMF ride on a narrowband FM voice channel", 14, P.plan_tones, TonesCore, "theta",
                lambda r: f"Tones: {len(r.ctcss)} CTCSS event(s), {len(r.dtmf)} DTMF digit(s).",
                lambda res, head: [head + line for line in (res.lines() if res is not None else [])],
                "With --demod nfm: detect the CTCSS tone and the DTMF digits of every target, print one line per tone "
                "event and digit sequence and write <output stem>.tones.json."),
    SideDecoder("acars", "am", "ACARS is audio MSK on an AM airband carrier", 15, P.plan_acars, AcarsCore, "envelope",
                lambda r: f"ACARS: {len(r.messages)} message(s), {r.crc_ok} CRC-passing candidate(s).",
                _per("messages"),
                "With --demod am: decode ACARS aircraft messages (2400 bit/s MSK on an airband AM channel) of every target, "
                "print one line per message and write <output stem>.acars.json."),
    SideDecoder("ais", "nfm", "AIS is 9600 bit/s GMSK on a narrowband FM channel", 16, P.plan_ais, AisCore, "theta",
                lambda r: f"AIS: {len(r.messages)} message(s), {r.crc_ok} CRC-passing candidate(s).",
                _ais_lines,
                "With --demod nfm: decode AIS ship traffic (9600 bit/s GMSK; 161.975 / 162.025 MHz) of every target, print "
                "one line per message and its !AIVDM sentences and write <output stem>.ais.json.  An unset --bw becomes 25 000."),
    SideDecoder("adsb", "am", "Mode S squitters are pulses on a 1090 MHz AM channel", 17, P.plan_adsb, AdsbCore, "envelope",
                lambda r: f"ADS-B: {len(r.messages)} message(s) of {len(r.aircraft)} aircraft, {r.crc_ok} check-passing position(s).",
                _per("messages"),
                "With --demod am: decode ADS-B / Mode S squitters (1090 MHz; DF11, 17, 18) of every target, print one line per "
                "message and write <output stem>.adsb.json.  An unset --bw and an unset --fs-ch become 2 000 000."),
)

NAMES = tuple(e.name for e in SIDE_DECODERS)


def check_modes(flags: dict, modes, plural: bool) -> None:
    """``ValueError`` for the first decoder (in table order) that is switched on in ``flags`` (name -> bool) while one of
    the targets' ``--demod`` ``modes`` is not the one it rides on.  ``plural``: the wording for several targets."""
    modes = [(m or "").lower() for m in modes]
    for e in SIDE_DECODERS:
        if flags.get(e.name) and any(m not in ACCEPTS[e.mode] for m in modes):
            target = f"{e.mode} targets" if plural else f"{'a' if e.mode == 'wfm' else 'an'} {e.mode} target"
            raise ValueError(f"{e.name}=True needs {target}: {e.why} (--demod {e.mode})")
