"""The link control and the calls of a DMR channel (``--find-dmr``): from the stored discriminator stream
of a channel and the DMR sync hits that section 25 keeps (``identify.py``) to who talked to whom, on which slot and colour
code, and for how long.

``iqa_dmr_slice`` takes the levels of every burst from its sync word and slices its 264 bits and the 24 bits of the CACH in
front of it; ``iqa_dmr_decode`` reads the TACT (Hamming(7,4)), the slot type (Golay(20,8)) and the payload (BPTC(196,96)) of
every sliced burst.  The host checks the payload (Reed-Solomon(12,9) or CRC-CCITT, ``check_lc`` / ``check_csbk``), reads its
fields (``parse_bursts``) and follows the calls of every slot (``track_calls``): integer logic.  The constants are written
from memory of ETSI TS 102 361-1 and of open-source readers of it, not checked against either here.  Nothing is listened to:
no vocoder, no embedded or short link control.  No CPU path: without a GPU or the built library the device calls raise
``RuntimeError``.

What is DMR's own lives here: the checks, the device calls, the burst parser, the call tracker, the dataclasses,
``decode_stream`` and ``channel_of``.  What every protocol layer shares lives in ``protocol_layer.py``: the stored stream under
``DmrDecoder``, the device call on host rows under ``slice_bursts`` / ``decode_bursts``, the keep rule under ``burst_hits``, the
per-lane loop under ``finish_dmr``, the builder under ``dmr_result``, and ``label`` / ``lines`` / ``to_json`` / ``from_json``."""
from __future__ import annotations

from ctypes import c_int64
from dataclasses import dataclass, field

import numpy as np

from . import dsp_plan as P
from . import identify as I
from . import protocol_layer as L

PATTERNS = tuple(p for p in I.PATTERNS if p.protocol == "dmr")  # bs, ms: a hit with C > 0 is the voice word, with C < 0 the data word
KINDS = ("bs voice", "bs data", "ms voice", "ms data")
SYNC_VOICE = tuple(p.word for p in PATTERNS)
SYNC_DATA = tuple(w ^ 0xAAAAAAAAAAAA for w in SYNC_VOICE)  # every symbol negated: +3 (01) <-> -3 (11)
FIRST, LAST = -66, 77  # the symbols of ``DmrPlan.offsets``
BURST_FIRST, CACH_FIRST = -54, -66
TACT_BITS = (0, 4, 8, 12, 14, 18, 22)  # AT, TC, LCSS1, LCSS0, P0, P1, P2 among the 24 CACH bits
TACT_CHECKS = ((0, 1, 2), (1, 2, 3), (0, 1, 3))  # P0, P1, P2 over d0 .. d3
SLOT_TYPE_BITS = tuple(range(98, 108)) + tuple(range(156, 166))
GOLAY_POLY = 0xC75
GOLAY_MAX_DISTANCE = 3
INTERLEAVE = 181
PAYLOAD_BITS = tuple(range(0, 98)) + tuple(range(166, 264))
ROW_CHECKS = ((0, 1, 2, 3, 5, 7, 8), (1, 2, 3, 4, 6, 8, 9), (2, 3, 4, 5, 7, 9, 10), (0, 1, 2, 4, 6, 7, 10))  # d11 .. d14 of a row
COLUMN_CHECKS = ((0, 1, 3, 5, 6), (0, 1, 2, 4, 6, 7), (0, 1, 2, 3, 5, 7, 8), (0, 2, 4, 5, 8))  # d9 .. d12 of a column
ROUNDS = 5
INFO_INDEX = tuple(range(4, 12)) + tuple(1 + 15 * r + c for r in range(1, 9) for c in range(11))
GF_POLY = 0x11D
RS_GENERATOR = (1, 14, 56, 64)  # x^3 + 14 x^2 + 56 x + 64: the roots alpha, alpha^2, alpha^3
RS_MASK = {1: 0x96, 2: 0x99}  # on bytes 9 .. 11, by data type
CRC_POLY = L.CRC_POLY
CRC_MASK = {3: 0xA5A5, 6: 0xCCCC}
DATA_TYPES = ("pi header", "voice lc header", "terminator lc", "csbk", "mbc header", "mbc continuation", "data header",
              "rate 1/2 data", "rate 3/4 data", "idle", "rate 1 data")
IDLE = 9
FLCO = {0: "group", 3: "private"}
HANG_S = 0.720  # a call with no burst of its slot for longer closes at its last burst
RECORD = P.DMR_RECORD  # TACT status, TACT nibble, slot-type status, distance, byte, payload status, flips, rounds


# ---- the checks and the fields (host, integers) ---------------------------------------------------------------------------------


_EXP, _LOG, gf_mul = L.gf_tables(GF_POLY, 8)
info_bytes, crc_ccitt = L.info_bytes, L.crc_ccitt  # twelve bytes of three information words; CRC_POLY from 0


def rs_remainder(data) -> tuple:
    """The remainder of the bytes ``data`` (the first the highest coefficient) modulo the generator, three bytes."""
    r = [0, 0, 0]
    for byte in data:
        lead = r[0] ^ int(byte)
        r = [r[1] ^ gf_mul(lead, RS_GENERATOR[1]), r[2] ^ gf_mul(lead, RS_GENERATOR[2]), gf_mul(lead, RS_GENERATOR[3])]
    return tuple(r)


def check_lc(info, data_type: int) -> bool:
    """Whether the twelve bytes of a voice LC header (type 1) or a terminator with LC (type 2), with bytes 9 .. 11 unmasked, are
    a multiple of the generator."""
    info = [int(b) for b in info]
    body = info[:9] + [b ^ RS_MASK[data_type] for b in info[9:12]]
    return rs_remainder(body[:9]) == tuple(body[9:12])


def check_csbk(info, data_type: int) -> bool:
    """Whether the complemented CRC-CCITT of bytes 0 .. 9 of a CSBK (type 3) or a data header (type 6) equals bytes 10 .. 11
    unmasked."""
    info = [int(b) for b in info]
    return (crc_ccitt(info[:10]) ^ 0xFFFF) == ((info[10] << 8 | info[11]) ^ CRC_MASK[data_type])


# ---- the device calls ---------------------------------------------------------------------------------------------------------


def slice_bursts(plane, rows, plan: P.DmrPlan) -> tuple:
    """``iqa_dmr_slice`` on a device int32 plane for ``rows`` (int64[K][3]: m, s, kind): (bits uint32[K][9], levels int64[K][3]:
    Sigma, A, flags) on the host.  ``ValueError`` for a sign other than +-1 or a kind over 3, before anything is launched."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))
    if rows.size and not (np.isin(rows[:, 1], (-1, 1)).all() and ((rows[:, 2] >= 0) & (rows[:, 2] <= 3)).all()):
        raise ValueError("iqa_dmr_slice: a hit's sign must be +-1 and its kind 0 .. 3")
    return L.slice_hits("iqa_dmr_slice", plane, rows, plan.offsets, P.DMR_WORDS)


def decode_bursts(bits, kinds) -> tuple:
    """``iqa_dmr_decode`` on ``bits`` (uint32[K][9], host) of the ``kinds`` (K values 0 .. 3): (info uint32[K][3], rec
    int32[K][8]) on the host.  ``ValueError`` for a kind over 3, before anything is launched."""
    bits = np.ascontiguousarray(np.asarray(bits, dtype=np.uint32).reshape(-1, P.DMR_WORDS))
    kinds = np.asarray(kinds, dtype=np.int64).reshape(-1)
    if kinds.shape[0] != bits.shape[0]:
        raise ValueError("iqa_dmr_decode: one kind to a burst")
    if kinds.size and not ((kinds >= 0) & (kinds <= 3)).all():
        raise ValueError("iqa_dmr_decode: a kind must be 0 .. 3")
    k = bits.shape[0]
    return tuple(L.device_rows("iqa_dmr_decode", k, k == 0, bits.view(np.int32), kinds.astype(np.uint8), c_int64(k),
                               L.Out(3, np.uint32), L.Out(RECORD, np.int32)))


# ---- the bursts ---------------------------------------------------------------------------------------------------------------


def burst_hits(hits, pats, half: int) -> np.ndarray:
    """int64[K][3], (m, s, kind) in order of m: of the kept hits (int64[K][6] of section 25, ``pats`` the patterns searched for)
    every hit of a ``dmr`` pattern, less those with a hit of either pattern within +-``half`` that has a larger |C|, or the same
    |C| at a smaller m, or the same m earlier in the table."""
    cand = []
    for p, m, c, _e, _pre, _post in np.asarray(hits, dtype=np.int64).reshape(-1, P.IDENT_RECORD).tolist():
        if pats[p].protocol != "dmr" or c == 0:
            continue
        which = PATTERNS.index(pats[p])
        cand.append((m, -abs(c), which, -1 if c < 0 else 1, 2 * which + (1 if c < 0 else 0)))
    rows = [(m, s, kind) for m, _neg, _which, s, kind in L.strongest_hits(cand, half)]
    return np.array(rows, dtype=np.int64).reshape(-1, 3)


def apply_flags(rec, levels, kinds) -> np.ndarray:
    """``rec`` of ``iqa_dmr_decode`` with the cuts of ``iqa_dmr_slice``'s flags written in: a TACT status of 3 for a bs burst whose
    CACH lies outside the stream, a payload status of 3 for a burst that does."""
    rec = np.array(rec, dtype=np.int32).reshape(-1, RECORD)
    flags, kinds = np.asarray(levels, dtype=np.int64).reshape(-1, 3)[:, 2], np.asarray(kinds, dtype=np.int64).reshape(-1)
    rec[(kinds < 2) & ((flags & 2) == 0), 0] = 3
    rec[(flags & 1) == 0, 5] = 3
    return rec


@dataclass
class DmrBurst(L.JsonRecord):
    time_s: float  # where sync symbol 0 ends, in seconds of the stream
    kind: int  # 0 bs voice, 1 bs data, 2 ms voice, 3 ms data
    slot: int | None  # 1 or 2; None for an ms kind or an unread TACT
    cc: int | None  # the colour code; None for a voice kind or a refused slot type
    data_type: int | None
    type_name: str | None
    checked: bool | None  # the payload's check held (True) or failed, the BPTC included (False); None: nothing to check
    corrected: bool  # the slot type or the payload was corrected
    flco: int | None = None
    fid: int | None = None
    src: int | None = None
    dst: int | None = None
    csbko: int | None = None
    hex: str | None = None  # the 96 information bits

    def line(self) -> str:
        head = f"DMR cc={'?' if self.cc is None else self.cc} ts={'?' if self.slot is None else self.slot}"
        if self.data_type is None:
            return f"{head} {KINDS[self.kind]}"
        tail = "" if self.checked is not False else " (failed)"
        if self.data_type == 3 and self.csbko is not None:
            return f"{head} csbk o=0x{self.csbko:02x} fid=0x{self.fid:02x} {self.hex[4:20]}{tail}"
        if self.flco is not None:
            return f"{head} {self.type_name} {FLCO.get(self.flco, f'flco {self.flco}')} {self.src} -> {self.dst}{tail}"
        return f"{head} {self.type_name} {self.hex or ''}{tail}".rstrip()


def new_counts() -> dict:
    return dict(no_level=0, cut=0, slot_refused=0, bptc_failed=0, check_failed=0, tact_fixed=0, idle=0)


def parse_bursts(rows, levels, info, rec, fs_ch: float, keyed_from: int = 0) -> tuple:
    """(bursts, counts): every burst that was read as a ``DmrBurst``, in order of time, voice kinds included; ``rows`` int64[K][3]
    (m, s, kind), ``levels`` int64[K][3], ``info`` uint32[K][3] and ``rec`` int32[K][8] (``apply_flags``' form).  A cut burst, one
    with A <= 0 and one whose slot type is refused are counted and left out."""
    counts = new_counts()
    out = []
    for (m, _s, kind), (_sigma, amp, flags), words, r in zip(np.asarray(rows).tolist(), np.asarray(levels).tolist(),
                                                               np.asarray(info).tolist(), np.asarray(rec).tolist()):
        if not flags & 1:
            counts["cut"] += 1
            continue
        if amp <= 0:
            counts["no_level"] += 1
            continue
        if r[0] == 1:
            counts["tact_fixed"] += 1
        slot = 1 + ((r[1] >> 2) & 1) if r[0] in (0, 1) else None
        time_s = (int(keyed_from) + m) / fs_ch
        if not kind & 1:
            out.append(DmrBurst(time_s=time_s, kind=kind, slot=slot, cc=None, data_type=None, type_name=None, checked=None, corrected=False))
            continue
        if r[2] == 2:
            counts["slot_refused"] += 1
            continue
        cc, dtype = (r[4] >> 4) & 0xF, r[4] & 0xF
        b = DmrBurst(time_s=time_s, kind=kind, slot=slot, cc=cc, data_type=dtype, corrected=r[2] == 1 or r[5] == 1,
                     type_name=DATA_TYPES[dtype] if dtype < len(DATA_TYPES) else "reserved", checked=None)
        by = info_bytes(words)
        b.hex = "".join(f"{x:02x}" for x in by)
        if r[5] == 2:
            counts["bptc_failed"] += 1
            b.checked, b.hex = False, None
        elif dtype == IDLE:
            counts["idle"] += 1
        elif dtype in RS_MASK:
            b.checked = check_lc(by, dtype)
            if b.checked:
                b.flco, b.fid, b.src, b.dst = by[0] & 0x3F, by[1], by[6] << 16 | by[7] << 8 | by[8], by[3] << 16 | by[4] << 8 | by[5]
        elif dtype in CRC_MASK:
            b.checked = check_csbk(by, dtype)
            if b.checked and dtype == 3:
                b.csbko, b.fid = by[0] & 0x3F, by[1]
        if b.checked is False and r[5] != 2:
            counts["check_failed"] += 1
        out.append(b)
    out.sort(key=lambda b: b.time_s)
    return out, counts


@dataclass
class DmrCall(L.JsonRecord):
    start_s: float
    end_s: float
    slot: int | None
    cc: int | None
    group: bool | None  # None for a late entry: the link control embedded in the voice bursts is not read
    src: int | None
    dst: int | None
    superframes: int
    terminated: bool

    def line(self) -> str:
        who = "late entry" if self.group is None else f"{'group' if self.group else 'private'} {self.src} -> {self.dst}"
        frames = f"{self.superframes} superframe{'' if self.superframes == 1 else 's'}"
        return (f"DMR cc={'?' if self.cc is None else self.cc} ts={'?' if self.slot is None else self.slot} {who} "
                f"{self.end_s - self.start_s:.2f} s ({frames}{'' if self.terminated else ', not terminated'})")


def track_calls(bursts) -> list:
    """The calls of the ``bursts`` (``parse_bursts``' list, in order of time) per slot, in order of their start: a checked voice LC
    header of FLCO 0 or 3 opens a call or confirms the open one of the same (FLCO, src, dst), a voice sync adds a superframe (and
    opens a late entry where none is open), a checked terminator closes it; a slot silent for more than ``HANG_S`` closes its
    call at its last burst."""
    calls, open_, last = [], {}, {}
    for b in bursts:
        call = open_.get(b.slot)
        if call is not None and b.time_s - last[b.slot] > HANG_S:
            del open_[b.slot]  # (its end is its last burst's time already)
            call = None
        last[b.slot] = b.time_s
        if b.data_type is None:  # a voice sync
            if call is None:
                call = open_[b.slot] = DmrCall(b.time_s, b.time_s, b.slot, None, None, None, None, 0, False)
                calls.append(call)
            call.superframes += 1
        elif b.checked and b.data_type == 1 and b.flco in FLCO:
            if call is not None and (call.group, call.src, call.dst) != (b.flco == 0, b.src, b.dst):
                del open_[b.slot]
                call = None
            if call is None:
                call = open_[b.slot] = DmrCall(b.time_s, b.time_s, b.slot, b.cc, b.flco == 0, b.src, b.dst, 0, False)
                calls.append(call)
        elif b.checked and b.data_type == 2 and call is not None:
            call.terminated, call.end_s = True, b.time_s
            if call.cc is None:
                call.cc = b.cc
            del open_[b.slot]
            continue
        if call is not None:
            call.end_s = b.time_s
            if call.cc is None and b.cc is not None:
                call.cc = b.cc
    return calls


# ---- the results --------------------------------------------------------------------------------------------------------------


@dataclass
class DmrChannel(L.JsonRecord, L.ChannelLabel):
    offset_hz: float  # the finder's
    freq_hz: float | None
    kinds: dict = field(default_factory=dict)  # bursts per kind name
    no_level: int = 0  # bursts dropped for A <= 0
    cut: int = 0  # bursts cut by an end of the stream
    slot_refused: int = 0
    bptc_failed: int = 0
    check_failed: int = 0
    tact_fixed: int = 0
    idle: int = 0
    calls: list = field(default_factory=list)  # DmrCall, in order of their start
    bursts: list = field(default_factory=list)  # DmrBurst: the data bursts that are not idle, the failed ones with checked = False
    note: str = ""  # why nothing was decoded
    NESTED = {"calls": DmrCall, "bursts": DmrBurst}

    def lines(self) -> list:
        """One line per call and per checked CSBK, in order of time."""
        items = [(c.start_s, 0, c.line()) for c in self.calls]
        items += [(b.time_s, 1, b.line()) for b in self.bursts if b.data_type == 3 and b.checked]
        return [f"{self.label()}: {line}" for _, _, line in sorted(items)]


@dataclass
class DmrResult(L.JsonRecord, L.ChannelLines):
    channels: list = field(default_factory=list)  # DmrChannel, in the order of the FindResult's channels
    sample_rate: float = 0.0
    center_freq: float | None = None
    NESTED = {"channels": DmrChannel}

    @property
    def calls(self) -> list:
        return [call for ch in self.channels for call in ch.calls]


# ---- one stream ---------------------------------------------------------------------------------------------------------------


def decode_stream(theta, plan: P.DmrPlan, centre: int, hits, pats, v=None) -> dict:
    """Everything behind the sync words of one stored stream (device float32 ``theta``; ``hits`` section 25's kept hits of it
    for the patterns ``pats``): ``rows`` (int64[K][3]: m, s, kind), ``bits`` (uint32[K][9]) and ``levels`` (int64[K][3]) of
    ``iqa_dmr_slice``, ``info`` (uint32[K][3]) and ``rec`` (int32[K][8], the cuts written in) of ``iqa_dmr_decode``, and the plane."""
    rows = burst_hits(hits, pats, plan.ident.half)
    if v is None:
        v = I.integrate(theta, plan.ident, centre)
    bits, levels = slice_bursts(v, rows, plan)
    info, rec = decode_bursts(bits, rows[:, 2])
    return dict(rows=rows, bits=bits, levels=levels, info=info, rec=apply_flags(rec, levels, rows[:, 2]), v=v)


def channel_of(st: dict, fs_ch: float, keyed_from: int, offset_hz: float, freq_hz) -> "DmrChannel":
    """The ``DmrChannel`` of ``decode_stream``'s output."""
    bursts, counts = parse_bursts(st["rows"], st["levels"], st["info"], st["rec"], fs_ch, keyed_from)
    out = DmrChannel(offset_hz=offset_hz, freq_hz=freq_hz, **counts)
    for kind in st["rows"][:, 2].tolist():
        out.kinds[KINDS[kind]] = out.kinds.get(KINDS[kind], 0) + 1
    out.calls = track_calls(bursts)
    out.bursts = [b for b in bursts if b.data_type is not None and (b.data_type != IDLE or b.checked is False)]
    return out


# ---- the layer of the second pass (describe.py) ---------------------------------------------------------------------------------

#: ``finish_dmr`` reads the 4800 family's plane; ``stages()`` shows ``dmr_rows`` ((m, s, kind) per burst, None where the channel is no
#: DMR channel) and, with ``keep_stages``, ``dmr_plan`` and these
LAYER = L.ProtocolLayer("dmr", (4800,), lambda fs_ch, rate: P.plan_dmr(fs_ch), "dmr", decode_stream, channel_of, DmrChannel, DmrResult,
                        keys=("bits", "levels", "info", "rec"))
PLANE_RATES, finish_dmr, dmr_result, stage_keys = LAYER.rates, LAYER.finish, LAYER.result_of, LAYER.stage_keys


class DmrDecoder(L.StoredTheta):
    """A DMR decoder for one discriminator stream from Python (``protocol_layer.StoredTheta``): ``finish()`` gives a
    ``DmrResult`` of one channel, ``stages()`` ``decode_stream``'s output with the plane on the host, and ``hits``."""

    plan_of = staticmethod(P.plan_dmr)
    patterns, layer = PATTERNS, LAYER
