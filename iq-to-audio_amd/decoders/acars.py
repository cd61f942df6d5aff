"""ACARS aircraft messages beside AM: 2400 bit/s audio MSK on an airband AM carrier.

Per block only the envelope ``|z|`` is stored (``iqa_envelope`` into a buffer of the decoder's own).  Once per run
``iqa_acars_max`` finds the largest envelope value, the host turns it into one power-of-two scale, ``iqa_acars_detect``
quantises the run, correlates it with one cycle of 1800 Hz and writes one byte per sample (the last bit period advanced the
phase: the bit stayed), ``iqa_acars_bits`` reads that plane at 8 sampling phases and ``iqa_acars_frames`` walks every
candidate behind a ``* SYN SYN SOH`` opener and keeps those whose check sequence holds.  Every block carries its own
check, so timing is found by search: there is no loop.  Merging and parsing are integer host logic on the kept blocks and
run on plain numpy arrays as well (``parse_messages``)."""
from __future__ import annotations

import logging
import math
from ctypes import c_int32, c_int64
from dataclasses import asdict, dataclass, field

import numpy as np

from .. import _dev as D
from .. import _native as N
from .. import dsp_plan as P
from .common import FrameCore, SideStage, group_records, parse_head, phase_planes, stage_records

LOG = logging.getLogger(__name__)

SOH, STX, ETX, ETB = 0x01, 0x02, 0x03, 0x17
CRC_POLY = 0x8408  # CRC-16/KERMIT, reflected; init 0, no final xor
MIN_BODY, MAX_BODY = 13, 240  # bytes behind SOH up to and including ETX / ETB
SLOT_BYTES = 244  # IQA_ACARS_SLOT_BYTES
PHASES = P.ACARS_PHASES


def crc16_kermit(data: bytes) -> int:
    reg = 0
    for byte in data:
        reg ^= byte
        for _ in range(8):
            reg = (reg >> 1) ^ CRC_POLY if reg & 1 else reg >> 1
    return reg


def _text(data: bytes) -> str:
    """Bit 7 stripped; anything outside printable ASCII as U+FFFD."""
    return "".join(chr(c & 0x7F) if 0x20 <= (c & 0x7F) <= 0x7E else "�" for c in data)


@dataclass
class AcarsMessage:
    time_s: float  # of the first bit behind SOH
    mode: str
    address: str  # the 7 characters as sent
    registration: str  # the address without its leading dots
    ack: str
    label: str
    block_id: str
    text: str | None  # None for a block without STX; for a downlink, what follows the message number and the flight id
    msgno: str | None  # downlinks (block id a digit): the 4 characters in front of the flight id
    flight: str | None  # downlinks: the 6 characters behind the message number
    more: bool  # the block ends in ETB: another block of the message follows
    parity_errors: int  # bytes up to ETX / ETB whose parity is even
    raw: str  # the bytes behind SOH up to ETX / ETB and the two check bytes, as hex
    hits: int  # sampling phases that decoded it

    def line(self) -> str:
        parts = [self.address, self.label, self.block_id] + [v for v in (self.msgno, self.flight, self.text) if v]
        return "ACARS " + " ".join(parts)


@dataclass
class AcarsResult:
    messages: list = field(default_factory=list)  # AcarsMessage, in order of time
    candidates: int = 0  # candidates behind an opener that reached ETX / ETB, over all phases
    crc_ok: int = 0  # of those, the ones that were kept

    def to_json(self) -> dict:
        return asdict(self)


def parse_message(raw: bytes) -> dict:
    """One kept block (the bytes behind SOH up to ETX / ETB, then the two check bytes) -> the fields of an ``AcarsMessage``
    but time and hits."""
    body = bytes(raw[:-2])
    out = dict(mode=_text(body[0:1]), address=_text(body[1:8]), ack=_text(body[8:9]), label=_text(body[9:11]), block_id=_text(body[11:12]),
               text=None, msgno=None, flight=None, more=(body[-1] & 0x7F) == ETB,
               parity_errors=sum(1 for c in body if bin(c).count("1") % 2 == 0), raw=bytes(raw).hex())
    out["registration"] = out["address"].lstrip(".")
    if len(body) > MIN_BODY and (body[12] & 0x7F) == STX:
        text = _text(body[13:-1])
        if out["block_id"].isdigit() and len(text) >= 10:
            out["msgno"], out["flight"], text = text[:4], text[4:10], text[10:]
        out["text"] = text
    return out


def parse_messages(plan: P.AcarsPlan, records: dict, candidates: int = 0) -> AcarsResult | None:
    """``records``: dict(phase=[k], s=[k], start=[k], nbytes=[k], data=uint8[k, >= nbytes]) in any order (the kept list of
    ``iqa_acars_frames``) -> the run's messages.  Integer logic only; ``None`` where no message survives."""
    res, start, phase, nbytes, data = parse_head(AcarsResult, records, candidates, "start", "phase", "nbytes")
    for at, raw, hits, _ in group_records(start, nbytes, data, plan.L, tie=phase):
        res.messages.append(AcarsMessage(time_s=at / plan.fs, hits=hits, **parse_message(raw)))
    return res if res.messages else None


def shift_of(emax: float) -> int:
    """14 - floor(log2 emax) for a positive finite float: emax 2^shift lies in [2^14, 2^15)."""
    mant, ex = math.frexp(float(emax))  # emax = mant 2^ex, 0.5 <= mant < 1
    return 14 - (ex - 1)


class AcarsCore(FrameCore):
    """Per-stream device state (``StreamCore``, no history): the run's stored envelope (one float32 device tensor per block,
    joined by ``finish``) and the absolute position.  ``keep_stages`` also stores q, I, Q and y at ``finish``, for the tests."""

    bits_entry, frames_entry = "iqa_acars_bits", "iqa_acars_frames"
    SLOT_BYTES, PHASES, STREAMS = SLOT_BYTES, PHASES, PHASES
    key, plane_keys, plane_dtype = "phase", ("bits", "nbits"), "uint8"

    def __init__(self, plan: P.AcarsPlan, *, keep_stages: bool = False):
        super().__init__(plan, plan.W, plan.bit_count, planes=dict(e="float32"))
        self._taps = D.from_numpy(np.ascontiguousarray(plan.taps))
        self.keep_stages = keep_stages

    def _block(self, e, n: int) -> None:
        """One block of the envelope (device float32[n], finite and >= 0).  The tensor is kept, not copied."""
        self.store.append("e", e)

    def joined(self):
        return self.store.joined("e")

    def finish(self, capacity: int = 64) -> dict:
        """The stages and the kept blocks of the stored run: dict(emax, sh, phase, s, start, nbytes, data, candidates, same,
        bits, nbits, count_of[, q, I, Q, y]), the records as numpy arrays sorted by (phase, s); ``sh`` is ``None`` and nothing
        behind the maximum is launched where the run's envelope is all zero.  A list too short for the kept blocks is never
        used: the search is repeated with room for all of them."""
        plan = self.plan
        e = self.joined()
        n = int(e.numel())
        peak = D.zeros(1, "float32")
        N.call("iqa_acars_max", N.ptr(e), c_int64(n), N.ptr(peak), N.stream_ptr())
        emax = float(peak.item())
        empty = dict(emax=emax, sh=None, phase=np.zeros(0, np.int64), s=np.zeros(0, np.int64), start=np.zeros(0, np.int64),
                     nbytes=np.zeros(0, np.int64), data=np.zeros((0, SLOT_BYTES), np.uint8), candidates=0, same=None, bits=None, nbits=0,
                     count_of=[0] * PHASES)
        if not emax > 0.0 or not math.isfinite(emax):
            if emax != 0.0:
                LOG.warning("ACARS: the envelope is not finite; nothing is decoded.")
            return empty
        sh = shift_of(emax)
        same = D.empty(n, "uint8")
        stages = dict(q=D.empty(n, "int32"), I=D.empty(n, "int32"), Q=D.empty(n, "int32"), y=D.empty(n, "int64")) if self.keep_stages else {}
        N.call("iqa_acars_detect", N.ptr(e), c_int64(n), c_int32(sh), c_int32(plan.W), c_int32(plan.L), N.ptr(self._taps), c_int32(plan.cr),
               c_int32(plan.sr), N.ptr(stages.get("q")), N.ptr(stages.get("I")), N.ptr(stages.get("Q")), N.ptr(stages.get("y")), N.ptr(same),
               N.stream_ptr())
        tail = self.frames_of(same, capacity) if max(self.counts_of(n)) else {}  # (no phase has a bit: nothing more is launched)
        return dict(empty, sh=sh, same=same, **tail, **stages)

    def result(self, fin=None, **context) -> AcarsResult | None:
        """The run's ``AcarsResult`` (``None`` without a message); ``fin``: a ``finish()`` made earlier."""
        fin = self.finish() if fin is None else fin
        return parse_messages(self.plan, fin, fin["candidates"])


class AcarsDecoder(SideStage):
    """The stage API: ``process(block)`` per block of the channel (complex: the channelizer's output, run through
    ``iqa_envelope``; or float32: an envelope, finite and >= 0), ``finish()`` once (an ``AcarsResult``, or ``None`` without
    a message), ``stages()`` for the tests."""

    source = "envelope"

    def __init__(self, rate: float, *, keep_stages: bool = True):
        super().__init__(AcarsCore(P.plan_acars(float(rate)), keep_stages=keep_stages), keep=False)  # (the core stores e itself)

    def stages(self) -> dict:
        """Host copies: ``e``, ``emax``, ``sh``, ``q``, ``I``, ``Q``, ``y`` (with keep_stages), ``same``, ``bits`` (8 uint8
        arrays, each as long as its phase has symbols) and ``records`` ([(phase, s, start instant, bytes)] sorted); the
        stages behind ``sh`` are ``None`` for an all-zero run."""
        fin = self._finished()

        def host(key):
            return None if fin.get(key) is None else fin[key].cpu().numpy()

        return dict(e=self.core.joined().cpu().numpy(), emax=np.float32(fin["emax"]), sh=fin["sh"], q=host("q"), I=host("I"), Q=host("Q"),
                    y=host("y"), same=host("same"), bits=phase_planes(self.core, fin), records=stage_records(fin, "phase"),
                    candidates=fin["candidates"])
