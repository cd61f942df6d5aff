"""AIS ship traffic beside narrowband FM: 9600 bit/s GMSK read straight off the discriminator.

Per block ``iqa_ais_filter`` quantises the discriminator output, runs the pulse-matched FIR and appends four bytes per
sample to the run's stored plane; once per run ``iqa_ais_symbols`` reads the plane at 8 sampling phases and
``iqa_ais_frames`` takes a decision level from the training sequence in front of every start flag, walks the HDLC
candidate behind it and keeps those whose CRC holds.  Every frame carries its own check, so timing is found by search and
the level per burst: there is no loop.  Merging, the bit fields and the NMEA sentences are integer host logic on the kept
frames and run on plain numpy arrays as well (``parse_frames``)."""
from __future__ import annotations

from ctypes import c_int32, c_int64
from dataclasses import dataclass, field

import numpy as np

from .. import _dev as D
from .. import _native as N
from .. import dsp_plan as P
from .common import FrameCore, SideStage, group_records, parse_head, phase_planes, stage_records

PHASES = P.AIS_PHASES
MIN_FRAME, MAX_FRAME = 11, 128  # bytes, FCS included
SLOT_BYTES = 128  # IQA_AIS_SLOT_BYTES
SENTENCE_CHARS = 60  # payload characters of one !AIVDM sentence
CHANNEL_A, CHANNEL_B = 161_975_000.0, 162_025_000.0
CHANNEL_REACH = 5_000.0
LON_MISSING, LAT_MISSING = 181 * 600_000, 91 * 600_000
_REVERSED = bytes(int(f"{b:08b}"[::-1], 2) for b in range(256))


class _Bits:
    """A message as one integer, fields read most significant bit first."""

    def __init__(self, raw: bytes):
        body = raw[:-2].translate(_REVERSED)  # a byte goes out least significant bit first
        self.n = 8 * len(body)
        self.value = int.from_bytes(body, "big")

    def u(self, at: int, width: int) -> int:
        return (self.value >> (self.n - at - width)) & ((1 << width) - 1)

    def i(self, at: int, width: int) -> int:
        v = self.u(at, width)
        return v - (1 << width) if v & (1 << (width - 1)) else v

    def text(self, at: int, chars: int) -> str:
        codes = [self.u(at + 6 * k, 6) for k in range(chars)]
        return "".join(chr(c | 0x40) if c < 32 else chr(c) for c in codes).rstrip("@ ")

    def lon(self, at: int):
        v = self.i(at, 28)
        return None if v == LON_MISSING else v / 600_000

    def lat(self, at: int):
        v = self.i(at, 27)
        return None if v == LAT_MISSING else v / 600_000

    def unless(self, at: int, width: int, missing: int, scale: int = 1):
        v = self.u(at, width)
        if v == missing:
            return None
        return v / scale if scale != 1 else v

    def dims(self, at: int) -> dict:
        return dict(to_bow=self.u(at, 9), to_stern=self.u(at + 9, 9), to_port=self.u(at + 18, 6), to_starboard=self.u(at + 24, 6))


def _position(b: _Bits) -> dict:
    turn = b.i(42, 8)
    return dict(status=b.u(38, 4), turn=None if turn == -128 else turn, speed=b.unless(50, 10, 1023, 10), accuracy=b.u(60, 1), lon=b.lon(61),
                lat=b.lat(89), course=b.unless(116, 12, 3600, 10), heading=b.unless(128, 9, 511), second=b.u(137, 6))


def _base_station(b: _Bits) -> dict:
    return dict(year=b.u(38, 14), month=b.u(52, 4), day=b.u(56, 5), hour=b.u(61, 5), minute=b.u(66, 6), second=b.u(72, 6), accuracy=b.u(78, 1),
                lon=b.lon(79), lat=b.lat(107))


def _static(b: _Bits) -> dict:
    return dict(imo=b.u(40, 30), callsign=b.text(70, 7), name=b.text(112, 20), ship_type=b.u(232, 8), **b.dims(240), eta_month=b.u(274, 4),
                eta_day=b.u(278, 5), eta_hour=b.u(283, 5), eta_minute=b.u(288, 6), draught=b.u(294, 8) / 10, destination=b.text(302, 20))


def _class_b(b: _Bits) -> dict:
    return dict(speed=b.unless(46, 10, 1023, 10), accuracy=b.u(56, 1), lon=b.lon(57), lat=b.lat(85), course=b.unless(112, 12, 3600, 10),
                heading=b.unless(124, 9, 511), second=b.u(133, 6))


def _aid(b: _Bits) -> dict:
    return dict(aid_type=b.u(38, 5), name=b.text(43, 20), accuracy=b.u(163, 1), lon=b.lon(164), lat=b.lat(192))


def _static_24(b: _Bits) -> dict:
    part = b.u(38, 2)
    if part == 0:
        return dict(part="A", name=b.text(40, 20))
    if part == 1 and b.n >= 168:
        return dict(part="B", ship_type=b.u(40, 8), vendor=b.text(48, 7), callsign=b.text(90, 7), **b.dims(132))
    return {}


#: type -> (bits the decoded fields need, their reader); a shorter message keeps type, mmsi, raw and nmea only
_TYPES = {1: (168, _position), 2: (168, _position), 3: (168, _position), 4: (168, _base_station), 5: (424, _static), 18: (168, _class_b),
          21: (272, _aid), 24: (160, _static_24)}


def decode_message(raw: bytes) -> dict:
    """One CRC-checked frame (FCS included) -> dict(type, repeat, mmsi, <fields of the decoded types>).  Speed in knots,
    course and heading in degrees, longitude and latitude in degrees (value / 600 000), draught in metres; a "not
    available" value (181 / 91 degrees, speed 1023, course 3600, heading 511, rate of turn -128) is ``None``."""
    b = _Bits(raw)
    out = dict(type=b.u(0, 6), repeat=b.u(6, 2), mmsi=b.u(8, 30))
    need, reader = _TYPES.get(out["type"], (0, None))
    if reader is not None and b.n >= need:
        out.update(reader(b))
    return out


def channel_of(frequency) -> str:
    """"A" within 5 kHz of 161.975 MHz, "B" within 5 kHz of 162.025 MHz, else empty."""
    if frequency is None:
        return ""
    if abs(float(frequency) - CHANNEL_A) <= CHANNEL_REACH:
        return "A"
    if abs(float(frequency) - CHANNEL_B) <= CHANNEL_REACH:
        return "B"
    return ""


def nmea_sentences(raw: bytes, channel: str = "", seq: int = 0) -> list:
    """The ``!AIVDM`` sentences of one frame: six message bits per payload character, at most 60 characters per sentence,
    the fill bits on the last one; ``seq`` is the id a multi-sentence message carries."""
    b = _Bits(raw)
    chars = -(-b.n // 6)
    fill = 6 * chars - b.n
    value = b.value << fill
    payload = ""
    for k in range(chars):
        v = (value >> (6 * (chars - 1 - k))) & 63
        payload += chr(v + 48 if v < 40 else v + 56)
    parts = [payload[k : k + SENTENCE_CHARS] for k in range(0, chars, SENTENCE_CHARS)]
    out = []
    for k, part in enumerate(parts):
        body = f"AIVDM,{len(parts)},{k + 1},{seq if len(parts) > 1 else ''},{channel},{part},{fill if k + 1 == len(parts) else 0}"
        check = 0
        for ch in body.encode("ascii"):
            check ^= ch
        out.append(f"!{body}*{check:02X}")
    return out


@dataclass
class AisMessage:
    time_s: float  # of the first bit behind the start flag
    type: int
    repeat: int
    mmsi: int
    raw: str  # the whole frame, FCS included, as hex
    nmea: list  # !AIVDM sentences
    channel: str  # "A", "B" or "" (from the target frequency)
    hits: int  # sampling phases that decoded it
    fields: dict = field(default_factory=dict)  # the decoded fields of types 1-5, 18, 21, 24

    def line(self) -> str:
        f = self.fields
        parts = [f"AIS {self.type} mmsi={self.mmsi}"]
        if f.get("lat") is not None and f.get("lon") is not None:
            parts.append(f"{abs(f['lat']):.5f}{'N' if f['lat'] >= 0 else 'S'} {abs(f['lon']):.5f}{'E' if f['lon'] >= 0 else 'W'}")
        if f.get("speed") is not None:
            parts.append(f"{f['speed']:.1f}kn")
        if f.get("course") is not None:
            parts.append(f"{f['course']:.1f}°")
        if "year" in f:
            parts.append(f"{f['year']:04d}-{f['month']:02d}-{f['day']:02d} {f['hour']:02d}:{f['minute']:02d}:{f['second']:02d}Z")
        for key in ("name", "callsign", "destination"):
            if f.get(key):
                parts.append(f"{key}={f[key]!r}")
        return " ".join(parts)

    def to_json(self) -> dict:
        return dict(time_s=self.time_s, type=self.type, repeat=self.repeat, mmsi=self.mmsi, **self.fields, channel=self.channel, hits=self.hits,
                    raw=self.raw, nmea=list(self.nmea))


@dataclass
class AisResult:
    messages: list = field(default_factory=list)  # AisMessage, in order of time
    candidates: int = 0  # closed HDLC candidates of >= 11 bytes over all phases
    crc_ok: int = 0  # of those, the ones whose CRC holds

    def to_json(self) -> dict:
        return dict(messages=[m.to_json() for m in self.messages], candidates=self.candidates, crc_ok=self.crc_ok)


def parse_frames(plan: P.AisPlan, records: dict, candidates: int = 0, *, frequency=None) -> AisResult | None:
    """``records``: dict(phase=[k], s=[k], start=[k], nbytes=[k], data=uint8[k, >= nbytes]) in any order (the kept-frame list
    of ``iqa_ais_frames``) -> the run's messages; ``frequency`` (Hz) names the channel of the sentences.  Integer logic only;
    ``None`` where no frame survives."""
    res, start, phase, nbytes, data = parse_head(AisResult, records, candidates, "start", "phase", "nbytes")
    channel, seq = channel_of(frequency), 0
    for at, raw, hits, _ in group_records(start, nbytes, data, plan.L, tie=phase):
        got = decode_message(raw)
        nmea = nmea_sentences(raw, channel, seq)
        if len(nmea) > 1:
            seq = (seq + 1) % 10
        head = {key: got.pop(key) for key in ("type", "repeat", "mmsi")}
        res.messages.append(AisMessage(time_s=at / plan.fs, raw=raw.hex(), nmea=nmea, channel=channel, hits=hits, fields=got, **head))
    return res if res.messages else None


class AisCore(FrameCore):
    """Per-stream device state (``StreamCore``): the carried quantised history (W - 1 values), the absolute position, and the
    growing store of the filter output (one int32 device tensor per block, joined by ``finish``).  ``keep_stages`` also stores
    t, for the tests."""

    bits_entry, frames_entry = "iqa_ais_symbols", "iqa_ais_frames"
    SLOT_BYTES, PHASES, STREAMS = SLOT_BYTES, PHASES, PHASES
    key, plane_keys, plane_dtype = "phase", ("v", "nsym"), "int32"

    def __init__(self, plan: P.AisPlan, *, keep_stages: bool = False):
        super().__init__(plan, plan.W, plan.symbol_count, plan.W - 1, dict(S="int32", t=None))
        self._taps = D.from_numpy(np.ascontiguousarray(plan.taps))
        self.keep_stages = keep_stages

    def _block(self, theta, n: int):
        """One block of the discriminator output (device float32[n], radians per sample)."""
        t, s = D.empty(n, "int32"), D.empty(n, "int32")
        N.call("iqa_ais_filter", N.ptr(theta), c_int64(n), N.ptr(self._hist), c_int32(self.plan.W), N.ptr(self._taps), N.ptr(t), N.ptr(s),
               N.stream_ptr())
        self.store.append("S", s)
        if self.keep_stages:
            self.store.append("t", t)
        return t

    def joined(self) -> dict:
        return dict(S=self.store.joined("S"), t=self.store.joined("t"))

    def finish(self, capacity: int = 256) -> dict:
        """The symbol planes and the kept frames of the stored run: dict(phase, s, start, nbytes, data, candidates, v, nsym,
        count_of), the records as numpy arrays sorted by (phase, s).  A list too short for the kept frames is never used:
        the search is repeated with room for all of them."""
        return self.frames_of(self.store.joined("S"), capacity)

    def result(self, fin=None, *, frequency=None, **context) -> AisResult | None:
        """The run's ``AisResult`` (``None`` without a message); ``frequency`` names the channel of the sentences; ``fin``: a
        ``finish()`` made earlier."""
        fin = self.finish() if fin is None else fin
        return parse_frames(self.plan, fin, fin["candidates"], frequency=frequency)


class AisDecoder(SideStage):
    """The stage API: ``process(block)`` per block of the channel (complex: the channelizer's output, run through
    ``iqa_quadrature`` with this decoder's own ``prev``; or float32: a discriminator output in radians per sample,
    |theta| < 2048 as ``iqa_ais_filter`` requires; a discriminator gives |theta| <= pi), ``finish()`` once (an
    ``AisResult``, or ``None`` without a message), ``stages()`` for the tests.  ``frequency``: the channel's RF frequency
    in Hz, which names the channel in the sentences."""

    def __init__(self, rate: float, *, frequency=None, keep_stages: bool = True):
        super().__init__(AisCore(P.plan_ais(float(rate)), keep_stages=keep_stages), keep=keep_stages, frequency=frequency)
        self.frequency = frequency

    def stages(self) -> dict:
        """Host copies: ``theta`` and ``t`` (with keep_stages), ``S``, ``v`` (8 int32 arrays, each as long as its phase has
        symbols), ``records`` ([(phase, s, start instant, bytes)] sorted) and ``candidates``."""
        fin = self._finished()
        st = self.core.joined()
        return dict(theta=self._inputs_host(), t=None if st["t"] is None else st["t"].cpu().numpy(),
                    S=st["S"].cpu().numpy(), v=phase_planes(self.core, fin), records=stage_records(fin, "phase"), candidates=fin["candidates"])
