"""ADS-B / Mode S squitters beside AM: 1090 MHz pulse position modulation, 2-20 MHz channels.

Per block ``iqa_adsb_quantise`` turns the envelope ``|z|`` (``iqa_envelope`` into a buffer of the decoder's own) into a
uint16 plane, which is stored.  Once per run ``iqa_adsb_search`` tests the preamble rule at every sample position, slices
the 112 bits behind every passing one and keeps those with DF 11, 17 or 18 whose 24-bit check leaves no remainder.  Every
squitter carries its own check, so timing is found by search: there is no loop.  Grouping and the fields of the extended
squitter are integer host logic (float64 for CPR and velocity) and run on plain numpy arrays as well (``parse_frames``)."""
from __future__ import annotations

import ctypes
import logging
import math
from ctypes import c_int32, c_int64
from dataclasses import asdict, dataclass, field

import numpy as np

from .. import _dev as D
from .. import _native as N
from .. import dsp_plan as P
from .common import SideStage, StreamCore, group_records, kept_records, parse_head

LOG = logging.getLogger(__name__)

GENERATOR = 0x1FFF409  # the Mode S parity polynomial, 25 bits
SLOT_BYTES = 14  # IQA_ADSB_SLOT_BYTES
TILE = 2048  # IQA_ADSB_TILE: candidate positions of one workgroup of the search
KEPT_DF = (11, 17, 18)
CHARSET = "#ABCDEFGHIJKLMNOPQRSTUVWXYZ#####_###############0123456789######"
PAIR_WINDOW_S = 10.0  # an even / odd pair further apart gives no global position


def syndrome(data: bytes) -> int:
    """The remainder of the bits of ``data`` (parity field included, MSB first) under the generator."""
    reg = 0
    for byte in data:
        for k in range(7, -1, -1):
            reg = (reg << 1) | ((byte >> k) & 1)
            if reg & 0x1000000:
                reg ^= GENERATOR
    return reg


def cpr_nl(lat: float) -> int:
    """The number of longitude zones at latitude ``lat`` (degrees)."""
    a = abs(lat)
    if a == 0.0:
        return 59
    if a == 87.0:
        return 2
    if a > 87.0:
        return 1
    return int(math.floor(2.0 * math.pi / math.acos(1.0 - (1.0 - math.cos(math.pi / 30.0)) / math.cos(a * math.pi / 180.0) ** 2)))


def cpr_global(even: tuple, odd: tuple, newer_is_odd: bool):
    """Global CPR: ``even`` and ``odd`` are (lat_cpr, lon_cpr); the newer message's parity picks the result.  (lat, lon) in
    degrees, or ``None`` where the two latitudes lie in different longitude zones."""
    le, ge = even[0] / 131072.0, even[1] / 131072.0
    lo, go = odd[0] / 131072.0, odd[1] / 131072.0
    j = math.floor(59.0 * le - 60.0 * lo + 0.5)
    lat_e = 6.0 * (j % 60 + le)
    lat_o = (360.0 / 59.0) * (j % 59 + lo)
    if lat_e >= 270.0:
        lat_e -= 360.0
    if lat_o >= 270.0:
        lat_o -= 360.0
    nl = cpr_nl(lat_e)
    if nl != cpr_nl(lat_o):
        return None
    m = math.floor(ge * (nl - 1) - go * nl + 0.5)
    if newer_is_odd:
        ni = max(nl - 1, 1)
        lat, lon = lat_o, (360.0 / ni) * (m % ni + go)
    else:
        ni = max(nl, 1)
        lat, lon = lat_e, (360.0 / ni) * (m % ni + ge)
    if lon >= 180.0:
        lon -= 360.0
    return lat, lon


@dataclass
class AdsbMessage:
    time_s: float  # of the preamble's first sample
    df: int
    icao: str  # six upper-case hex digits
    raw: str  # the 7 or 14 bytes as hex
    hits: int  # sample positions that decoded it
    level: float  # the mean preamble pulse against full scale
    type_code: int | None  # None for DF11
    category: int | None = None  # TC 1-4
    callsign: str | None = None  # TC 1-4
    altitude_ft: int | None = None  # TC 9-18 with the Q bit set
    cpr_odd: int | None = None  # position messages: the F bit
    lat_cpr: int | None = None
    lon_cpr: int | None = None
    lat: float | None = None  # position messages paired with the other parity inside 10 s
    lon: float | None = None
    speed_kt: float | None = None  # TC 19 subtypes 1, 2
    track_deg: float | None = None
    vertical_rate_fpm: int | None = None

    def line(self) -> str:
        head = f"ADS-B {self.icao}"
        if self.callsign is not None:
            return f"{head} ident {self.callsign}"
        if self.lat_cpr is not None:
            alt = "" if self.altitude_ft is None else f" {self.altitude_ft}ft"
            if self.lat is None:
                return f"{head} pos {'odd' if self.cpr_odd else 'even'} {self.lat_cpr}/{self.lon_cpr}{alt}"
            ns, ew = "N" if self.lat >= 0 else "S", "E" if self.lon >= 0 else "W"
            return f"{head} pos {abs(self.lat):.5f}{ns} {abs(self.lon):.5f}{ew}{alt}"
        if self.speed_kt is not None or self.vertical_rate_fpm is not None:
            parts = [] if self.speed_kt is None else [f"{self.speed_kt:.1f}kn", f"{self.track_deg:.1f}°"]
            parts += [] if self.vertical_rate_fpm is None else [f"{self.vertical_rate_fpm}fpm"]
            return f"{head} vel " + " ".join(parts)
        return f"{head} DF{self.df}" + ("" if self.type_code is None else f" TC{self.type_code}")


@dataclass
class AdsbResult:
    messages: list = field(default_factory=list)  # AdsbMessage, in order of time
    aircraft: list = field(default_factory=list)  # one dict per ICAO address, in ICAO order
    candidates: int = 0  # positions that passed the preamble rule
    crc_ok: int = 0  # kept frames (positions, before grouping)

    def to_json(self) -> dict:
        return asdict(self)


def _bits(value: int, width: int, first: int, last: int) -> int:
    """Bits ``first`` .. ``last`` (1-based, MSB first, inclusive) of a ``width``-bit field."""
    return (value >> (width - last)) & ((1 << (last - first + 1)) - 1)


def parse_me(me: int) -> dict:
    """The decoded fields of a 56-bit ME field (DF17 / 18); only ``type_code`` where the type is outside the scope."""
    tc = me >> 51
    out: dict = dict(type_code=tc)
    if 1 <= tc <= 4:
        out["category"] = _bits(me, 56, 6, 8)
        text = "".join(CHARSET[_bits(me, 56, 9 + 6 * k, 14 + 6 * k)] for k in range(8))
        out["callsign"] = text.replace("_", " ").rstrip(" ")
    elif 9 <= tc <= 18 or 20 <= tc <= 22:
        if tc <= 18:
            alt = _bits(me, 56, 9, 20)
            if alt & 0x10:  # the Q bit: the field's 8th bit
                out["altitude_ft"] = 25 * (((alt >> 5) << 4) | (alt & 0xF)) - 1000
        out["cpr_odd"] = _bits(me, 56, 22, 22)
        out["lat_cpr"] = _bits(me, 56, 23, 39)
        out["lon_cpr"] = _bits(me, 56, 40, 56)
    elif tc == 19 and _bits(me, 56, 6, 8) in (1, 2):
        mult = 4 if _bits(me, 56, 6, 8) == 2 else 1
        s_ew, v_ew = _bits(me, 56, 14, 14), _bits(me, 56, 15, 24)
        s_ns, v_ns = _bits(me, 56, 25, 25), _bits(me, 56, 26, 35)
        s_vr, v_r = _bits(me, 56, 37, 37), _bits(me, 56, 38, 46)
        if v_ew and v_ns:
            vx = mult * (v_ew - 1) * (-1 if s_ew else 1)
            vy = mult * (v_ns - 1) * (-1 if s_ns else 1)
            out["speed_kt"] = math.hypot(vx, vy)
            out["track_deg"] = math.degrees(math.atan2(vx, vy)) % 360.0
        if v_r:
            out["vertical_rate_fpm"] = 64 * (v_r - 1) * (-1 if s_vr else 1)
    return out


def parse_frames(plan: P.AdsbPlan, records: dict, candidates: int = 0) -> AdsbResult | None:
    """``records``: dict(n=[k], nbits=[k], P=[k], data=uint8[k, 14]) in any order (the kept list of ``iqa_adsb_search``) ->
    the run's messages and aircraft.  ``None`` where no message survives."""
    res, at, nbits, level, data = parse_head(AdsbResult, records, candidates, "n", "nbits", "P")
    last_pos: dict = {}  # (icao, parity) -> the latest position message
    craft: dict = {}
    for n, raw, hits, first in group_records(at, nbits // 8, data, plan.L):
        df, p = raw[0] >> 3, int(level[first])
        msg = AdsbMessage(time_s=n / plan.fs, df=df, icao=raw[1:4].hex().upper(), raw=raw.hex(), hits=hits,
                          level=p / (4.0 * plan.h * 65536.0), type_code=None)
        if df in (17, 18):
            for key, value in parse_me(int.from_bytes(raw[4:11], "big")).items():
                setattr(msg, key, value)
            if msg.lat_cpr is not None and 9 <= msg.type_code <= 22:
                other = last_pos.get((msg.icao, 1 - msg.cpr_odd))
                if other is not None and msg.time_s - other.time_s <= PAIR_WINDOW_S:
                    even, odd = (other, msg) if msg.cpr_odd else (msg, other)
                    fix = cpr_global((even.lat_cpr, even.lon_cpr), (odd.lat_cpr, odd.lon_cpr), bool(msg.cpr_odd))
                    if fix is not None:
                        msg.lat, msg.lon = fix
                last_pos[(msg.icao, msg.cpr_odd)] = msg
        res.messages.append(msg)
        ac = craft.setdefault(msg.icao, dict(icao=msg.icao, callsign=None, lat=None, lon=None, altitude_ft=None, speed_kt=None, track_deg=None,
                                             vertical_rate_fpm=None, messages=0, first_s=msg.time_s, last_s=msg.time_s))
        ac["messages"] += 1
        ac["last_s"] = msg.time_s
        for key in ("callsign", "altitude_ft", "speed_kt", "track_deg", "vertical_rate_fpm"):
            if getattr(msg, key) is not None:
                ac[key] = getattr(msg, key)
        if msg.lat is not None:
            ac["lat"], ac["lon"] = msg.lat, msg.lon
    res.aircraft = [craft[key] for key in sorted(craft)]
    return res if res.messages else None


class AdsbCore(StreamCore):
    """Per-stream device state (``StreamCore``, no history): the run's stored q plane (one device tensor per block, uint16
    values held in int16 storage, joined by ``finish``) and the absolute position."""

    def __init__(self, plan: P.AdsbPlan):
        super().__init__(plan, planes=dict(q="int16"))
        self._offsets_host = np.ascontiguousarray(plan.offsets, dtype=np.int32)
        self._offsets = D.from_numpy(self._offsets_host)

    def _block(self, e, n: int) -> None:
        """One block of the envelope (device float32[n], >= 0): quantised into a tensor of the core's own."""
        q = D.empty(n, "int16")
        N.call("iqa_adsb_quantise", N.ptr(e), c_int64(n), N.ptr(q), N.stream_ptr())
        self.store.append("q", q)

    def joined(self):
        return self.store.joined("q")

    def search(self, q, capacity: int, counts, flags=None):
        """One ``iqa_adsb_search`` over the device plane ``q`` -> (list, slots)."""
        lst, slots = D.empty(3 * capacity, "int64"), D.empty(SLOT_BYTES * capacity, "uint8")
        N.call("iqa_adsb_search", N.ptr(q), c_int64(int(q.numel())), N.ptr(self._offsets), self._offsets_host.ctypes.data_as(ctypes.POINTER(c_int32)),
               c_int32(self.plan.h), c_int32(self.plan.span), N.ptr(flags), N.ptr(lst), N.ptr(slots), c_int64(capacity), N.ptr(counts),
               N.stream_ptr())
        return lst, slots

    def finish(self, capacity: int = 256, *, keep_flags: bool = False) -> dict:
        """The kept frames of the stored run: dict(n, nbits, P, data, candidates[, flags]), the records as numpy arrays sorted
        by (n).  A list too short for the kept frames is never used: the search is repeated with room for all of them."""
        q = self.joined()
        n = int(q.numel())
        npos = max(n - self.plan.span + 1, 0)
        flags = D.empty(npos, "uint8") if keep_flags else None
        entries, data, _, passed = kept_records(lambda room, counts: self.search(q, room, counts, flags), capacity, 3, SLOT_BYTES, (0,))
        out = dict(n=entries[:, 0].copy(), nbits=entries[:, 1].copy(), P=entries[:, 2].copy(), data=data, candidates=passed)
        if keep_flags:
            out["flags"] = flags
        return out

    def result(self, fin=None, **context) -> AdsbResult | None:
        """The run's ``AdsbResult`` (``None`` without a message); ``fin``: a ``finish()`` made earlier."""
        fin = self.finish() if fin is None else fin
        return parse_frames(self.plan, fin, fin["candidates"])


class AdsbDecoder(SideStage):
    """The stage API: ``process(block)`` per block of the channel (complex: the channelizer's output, run through
    ``iqa_envelope``; or float32: an envelope), ``finish()`` once (an ``AdsbResult``, or ``None`` without a message),
    ``stages()`` for the tests."""

    source = "envelope"
    finish_args = dict(keep_flags=True)

    def __init__(self, rate: float):
        super().__init__(AdsbCore(P.plan_adsb(float(rate))), keep=True)

    def stages(self) -> dict:
        """Host copies: ``e`` (float32), ``q`` (uint16), ``flags`` (uint8 per candidate position: passed the preamble rule),
        ``records`` ([(n, nbits, P, bytes)] sorted by n) and ``candidates``."""
        fin = self._finished()
        e = self._inputs_host() if self.inputs else np.zeros(0, dtype=np.float32)
        records = [(int(n), int(nb), int(p), fin["data"][k, : int(nb) // 8].tobytes())
                   for k, (n, nb, p) in enumerate(zip(fin["n"], fin["nbits"], fin["P"]))]
        return dict(e=e, q=self.core.joined().cpu().numpy().view(np.uint16), flags=fin["flags"].cpu().numpy(), records=records,
                    candidates=fin["candidates"])
