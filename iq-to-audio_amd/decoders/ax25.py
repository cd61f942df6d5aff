"""AX.25 frames over 1200-baud Bell-202 AFSK beside narrowband FM: APRS, packet, telemetry.

Per block ``iqa_afsk_correlate`` quantises the discriminator output, runs the mark and space tone correlators and appends
one byte per sample (three slicer decisions) to the run's stored plane; once per run ``iqa_afsk_bits`` reads the plane at
8 sampling phases x 3 space gains into 24 NRZI-decoded bit streams and ``iqa_afsk_frames`` walks every HDLC candidate of
every stream and keeps those whose CRC holds.  Every frame carries its own check, so timing and tone balance are found by
search: there is no loop.  Merging, address validation and parsing are integer host logic on the kept frames and run on
plain numpy arrays as well (``parse_frames``)."""
from __future__ import annotations

from ctypes import c_int32, c_int64
from dataclasses import asdict, dataclass, field

import numpy as np

from .. import _dev as D
from .. import _native as N
from .. import dsp_plan as P
from .common import FrameCore, SideStage, group_records, parse_head, phase_planes, stage_records

FLAG = 0x7E
CRC_POLY = 0x8408  # CRC-16/X.25, reflected; init 0xFFFF, final xor 0xFFFF
MIN_FRAME, MAX_FRAME = 17, 330  # bytes, FCS included
SLOT_BYTES = 332  # IQA_AFSK_SLOT_BYTES
VARIANTS = len(P.AFSK_GAINS) * P.AFSK_PHASES
CALL_CHARS = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 ")
CONTROL_UI, PID_NO_LAYER3 = 0x03, 0xF0


def crc16_x25(data: bytes) -> int:
    reg = 0xFFFF
    for byte in data:
        reg ^= byte
        for _ in range(8):
            reg = (reg >> 1) ^ CRC_POLY if reg & 1 else reg >> 1
    return reg ^ 0xFFFF


@dataclass
class Ax25Frame:
    time_s: float  # of the first bit behind the opening flag
    source: str
    dest: str
    path: list  # digipeaters, "*" behind one whose H bit is set
    control: int
    pid: int | None  # None for a frame without a PID field (S and U frames other than UI)
    info: str  # UI frames (control 0x03, PID 0xF0): text, anything outside printable ASCII as U+FFFD; otherwise hex
    raw: str  # the whole frame, FCS included, as hex
    hits: int  # grid points (gain, phase) that decoded it

    def line(self) -> str:
        """TNC2 style: SOURCE>DEST,DIGI*,DIGI:info."""
        return f"{self.source}>{','.join([self.dest] + list(self.path))}:{self.info}"


@dataclass
class Ax25Result:
    frames: list = field(default_factory=list)  # Ax25Frame, in order of time
    candidates: int = 0  # closed HDLC candidates of >= 17 bytes over all grid points
    crc_ok: int = 0  # of those, the ones whose CRC holds
    rejected: int = 0  # merged CRC-passing frames with an invalid address field

    def to_json(self) -> dict:
        return asdict(self)


def _callsign(seven: bytes) -> str | None:
    if any(c & 1 for c in seven[:6]) or any((c >> 1) not in CALL_CHARS for c in seven[:6]):
        return None
    name = bytes(c >> 1 for c in seven[:6]).decode("ascii").rstrip()
    ssid = (seven[6] >> 1) & 15
    return f"{name}-{ssid}" if ssid else name


def parse_frame(raw: bytes):
    """One CRC-checked frame (FCS included) -> dict(source, dest, path, control, pid, info), or ``None`` where the address
    field is invalid: 2 to 10 addresses of 7 bytes, callsign characters ``>> 1`` in A-Z, 0-9, space with a zero low bit, the
    extension bit on the last address and on no other."""
    body = bytes(raw[:-2])
    calls = []
    while True:
        seven = body[7 * len(calls) : 7 * len(calls) + 7]
        if len(seven) < 7:
            return None
        name = _callsign(seven)
        if name is None:
            return None
        calls.append((name, bool(seven[6] & 0x80)))
        if seven[6] & 1:
            break
        if len(calls) == 10:
            return None
    rest = body[7 * len(calls) :]
    if len(calls) < 2 or not rest:
        return None
    control = rest[0]
    has_pid = ((control & 0xEF) == CONTROL_UI or (control & 1) == 0) and len(rest) >= 2
    pid = rest[1] if has_pid else None
    info = rest[2:] if has_pid else rest[1:]
    if control == CONTROL_UI and pid == PID_NO_LAYER3:
        text = "".join(chr(c) if 0x20 <= c <= 0x7E else "�" for c in info)
    else:
        text = info.hex()
    return dict(dest=calls[0][0], source=calls[1][0], path=[c + ("*" if h else "") for c, h in calls[2:]], control=control, pid=pid, info=text)


def parse_frames(plan: P.AfskPlan, records: dict, candidates: int = 0) -> Ax25Result | None:
    """``records``: dict(variant=[k], s=[k], start=[k], nbytes=[k], data=uint8[k, >= nbytes]) in any order (the kept-frame
    list of ``iqa_afsk_frames``) -> the run's frames.  Integer logic only; ``None`` where no frame survives."""
    res, start, variant, nbytes, data = parse_head(Ax25Result, records, candidates, "start", "variant", "nbytes")
    for at, raw, hits, _ in group_records(start, nbytes, data, plan.L, tie=variant):
        got = parse_frame(raw)
        if got is None:
            res.rejected += 1
            continue
        res.frames.append(Ax25Frame(time_s=at / plan.fs, raw=raw.hex(), hits=hits, **got))
    return res if res.frames else None


class AfskCore(FrameCore):
    """Per-stream device state (``StreamCore``): the carried quantised history (L - 1 values), the absolute position, and the
    growing store of the slicer plane (one uint8 device tensor per block, joined by ``finish``).  ``keep_stages`` also stores t
    and the two energy planes, for the tests."""

    bits_entry, frames_entry = "iqa_afsk_bits", "iqa_afsk_frames"
    SLOT_BYTES, PHASES, STREAMS = SLOT_BYTES, P.AFSK_PHASES, VARIANTS
    key, plane_keys, plane_dtype = "variant", ("bits", "nbits"), "uint8"

    def __init__(self, plan: P.AfskPlan, *, keep_stages: bool = False):
        super().__init__(plan, plan.L, plan.bit_count, plan.L - 1, dict(sign="uint8", t=None, E0=None, E1=None))
        self._taps = D.from_numpy(np.ascontiguousarray(plan.taps))
        self.keep_stages = keep_stages

    def _block(self, theta, n: int):
        """One block of the discriminator output (device float32[n], radians per sample)."""
        t, sign = D.empty(n, "int32"), D.empty(n, "uint8")
        e = (D.empty(n, "int64"), D.empty(n, "int64")) if self.keep_stages else (None, None)
        N.call("iqa_afsk_correlate", N.ptr(theta), c_int64(n), N.ptr(self._hist), c_int32(self.plan.L), N.ptr(self._taps), N.ptr(t),
               N.ptr(sign), N.ptr(e[0]), N.ptr(e[1]), N.stream_ptr())
        self.store.append("sign", sign)
        if self.keep_stages:
            for name, plane in (("t", t), ("E0", e[0]), ("E1", e[1])):
                self.store.append(name, plane)
        return t

    def joined(self) -> dict:
        e = (self.store.joined("E0"), self.store.joined("E1"))
        return dict(sign=self.store.joined("sign"), t=self.store.joined("t"), E=None if e[0] is None else dict(zip(P.AFSK_TONES, e)))

    def finish(self, capacity: int = 256) -> dict:
        """The bit streams and the kept frames of the stored run: dict(variant, s, start, nbytes, data, candidates, bits,
        count_of), the records as numpy arrays sorted by (variant, s).  A list too short for the kept frames is never used:
        the search is repeated with room for all of them."""
        return self.frames_of(self.store.joined("sign"), capacity)

    def result(self, fin=None, **context) -> Ax25Result | None:
        """The run's ``Ax25Result`` (``None`` without a frame); ``fin``: a ``finish()`` made earlier."""
        fin = self.finish() if fin is None else fin
        return parse_frames(self.plan, fin, fin["candidates"])


class Ax25Decoder(SideStage):
    """The stage API: ``process(block)`` per block of the channel (complex: the channelizer's output, run through
    ``iqa_quadrature`` with this decoder's own ``prev``; or float32: a discriminator output in radians per sample,
    |theta| < 2048 as ``iqa_afsk_correlate`` requires; a discriminator gives |theta| <= pi),
    ``finish()`` once (an ``Ax25Result``, or ``None`` without a frame), ``stages()`` for the tests."""

    def __init__(self, rate: float, *, keep_stages: bool = True):
        super().__init__(AfskCore(P.plan_afsk(float(rate)), keep_stages=keep_stages), keep=keep_stages)

    def stages(self) -> dict:
        """Host copies: ``theta``, ``t`` and ``E`` (tone -> int64[n]; with keep_stages), ``sign``, ``bits`` (24 uint8 arrays, each
        as long as its phase has bits) and ``records`` ([(variant, s, start instant, bytes)] sorted)."""
        fin = self._finished()
        st = self.core.joined()
        return dict(theta=self._inputs_host(), t=None if st["t"] is None else st["t"].cpu().numpy(),
                    E=None if st["E"] is None else {f: e.cpu().numpy() for f, e in st["E"].items()},
                    sign=st["sign"].cpu().numpy(), bits=phase_planes(self.core, fin), records=stage_records(fin, "variant"),
                    candidates=fin["candidates"])
