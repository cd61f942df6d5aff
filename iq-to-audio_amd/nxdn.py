"""The link information, the calls and the control messages of an NXDN channel (``--find-nxdn``): from the
stored discriminator stream of a channel and the NXDN frame sync hits that section 25 keeps (``identify.py``), at 4800 or 2400
symbols/s, to who calls whom under which radio access number and for how long, and to what a control channel repeats.

``iqa_nxdn_slice`` takes the levels of every frame from its ten-symbol frame sync word (a least squares fit: the word holds
inner levels), slices the 192 symbols behind it and removes the scrambler; the host reads the LICH from those bits (``lich_fields``)
and forms the class mask of the frame (``decoder_classes``); ``iqa_nxdn_decode`` decodes, by mask, the SACCH, the two FACCH1s or
the outbound CAC through a 16-state Viterbi decoder with erasures for the punctured bits.  The host checks the CRCs, joins the
SACCH parts of a superframe, reads the layer-3 messages (``parse_frames``) and follows the calls (``track_calls``): integer
logic.  The constants are written from memory of the published common air interface and of open-source readers of it, not
checked against either here.  Not decoded: the voice (AMBE+2), UDCH / FACCH2, the inbound CACs, the 48 bits behind the outbound
CAC, and anything enciphered beyond naming the cipher type.  No CPU path: without a GPU or the built library the device calls
raise ``RuntimeError``.

What every protocol layer shares lives in ``protocol_layer.py``: the stored stream under ``NxdnDecoder``, the device call on host
rows under ``slice_frames`` / ``decode_frames``, the keep rule under ``frame_hits``, the per-lane loop under ``finish_nxdn``, the
builder under ``nxdn_result``, and ``label`` / ``lines`` / ``to_json`` / ``from_json`` of the results."""
from __future__ import annotations

from ctypes import c_int64
from dataclasses import dataclass, field

import numpy as np

from . import dsp_plan as P
from . import identify as I
from . import protocol_layer as L

NXDN_PATTERNS = tuple(p for p in I.PATTERNS if p.protocol == "nxdn")  # one word; a hit with C < 0 is the same word, spectrum inverted
SYNC = NXDN_PATTERNS[0].word
SYNC_SYMBOLS = 10
LEVEL_SCALE = 370  # A and Dc are 370 times the outer level and the DC
SCRAMBLER_FIRST = (0, 0, 1, 0, 0, 1, 1, 1, 0)  # one bit per symbol from symbol 10 on: b[n] = b[n - 5] ^ b[n - 9] behind these
HANG_S = 0.360  # a call with no frame for longer closes at its last frame
RECORD = P.NXDN_RECORD  # the mask, the metric of the SACCH or the CAC, of FACCH1-a, of FACCH1-b
NEED_LICH, NEED_FRAME = 18, 192  # the ``valid`` that covers the LICH, and everything behind it
SACCH, FACCH1_A, FACCH1_B, CAC = 1, 2, 4, 8  # the bits of a frame's class mask
#: per block: (info + CRC + tail steps, punctured positions, their period, interleave depth D and columns C)
CODES = {"sacch": (36, (5,), 6, 12, 5), "facch1": (96, (1,), 4, 9, 16), "cac": (175, (3, 11), 14, 12, 25)}
#: per block: (CRC width, polynomial, initial value, the bits it covers)
CRCS = {"sacch": (6, 0x27, 0x3F, 26), "facch1": (12, 0x80F, 0xFFF, 80), "cac": (16, 0x1021, 0xFFFF, 155)}
RF = {0: "RCCH", 1: "RTCH", 2: "RDCH", 3: "RTCH-C"}
FN_CONTROL = {0: "outbound", 1: "long inbound", 2: "2", 3: "short inbound"}
FN_TRAFFIC = {0: "non-superframe", 1: "UDCH", 2: "superframe", 3: "idle"}
CALL_TYPES = {0: "broadcast", 1: "group", 4: "individual", 6: "interconnect"}
VCALL, TX_REL = 0x01, 0x08
MESSAGES = {0x01: "VCALL", 0x03: "VCALL_IV", 0x04: "VCALL_ASSGN", 0x08: "TX_REL", 0x09: "DCALL_HDR", 0x0B: "DCALL_DATA", 0x0C: "DCALL_ACK",
            0x0E: "DCALL_ASSGN", 0x10: "IDLE", 0x11: "DISC", 0x17: "DST_ID_INFO", 0x18: "SITE_INFO", 0x19: "SRV_INFO", 0x1A: "CCH_INFO",
            0x1B: "ADJ_SITE_INFO", 0x20: "REG_RESP"}
CALL_FIELDS = ("emergency", "call_type", "mode", "src", "dst", "cipher", "key")


# ---- the checks and the fields (host, integers) ---------------------------------------------------------------------------------


def scrambler(count: int = P.NXDN_OFFSETS - SYNC_SYMBOLS) -> list:
    """The first ``count`` bits of the scrambler."""
    bits = list(SCRAMBLER_FIRST)
    while len(bits) < count:
        bits.append(bits[-5] ^ bits[-9])
    return bits[:count]


def crc_bits(bits, width: int, poly: int, init: int) -> int:
    """The CRC of ``bits``, the first sent first: MSB first, no final inversion."""
    crc, top = init, 1 << (width - 1)
    for b in bits:
        fed = bool(crc & top) != bool(b)
        crc = (crc << 1) & ((1 << width) - 1)
        if fed:
            crc ^= poly
    return crc


def _value(bits) -> int:
    out = 0
    for b in bits:
        out = out << 1 | b
    return out


def block_of(words, kind: str) -> tuple:
    """(the bits in front of the CRC as one integer, the first the top bit; whether the CRC holds) of a block's words."""
    width, poly, init, covered = CRCS[kind]
    whole = 0
    for w in words:
        whole = whole << 32 | int(w)
    whole >>= 32 * len(words) - covered - width
    data, crc, top, mask = whole >> width, init, 1 << (width - 1), (1 << width) - 1
    for i in range(covered - 1, -1, -1):
        fed = bool(crc & top) != bool(data >> i & 1)
        crc = (crc << 1) & mask
        if fed:
            crc ^= poly
    return data, crc == whole & mask


def _check(words, kind: str) -> bool:
    return block_of(words, kind)[1]


def check_sacch(words) -> bool:
    """Whether the CRC-6 of the 26 SACCH bits equals the six behind them (``words``: the words 0 .. 1 of ``iqa_nxdn_decode``)."""
    return _check(words, "sacch")


def check_facch1(words) -> bool:
    """Whether the CRC-12 of the 80 FACCH1 bits equals the twelve behind them (``words``: a FACCH1's three)."""
    return _check(words, "facch1")


def check_cac(words) -> bool:
    """Whether the CRC-16 of the 155 CAC bits equals the sixteen behind them (``words``: the words 8 .. 13)."""
    return _check(words, "cac")


def lich_of(words) -> tuple:
    """(the LICH byte, whether every second bit of its eight dibits is 1) of a sliced frame's words: the frame bits 20 .. 35."""
    sixteen = (int(words[0]) & 0xFFF) << 4 | int(words[1]) >> 28
    byte = _value((sixteen >> (15 - 2 * k)) & 1 for k in range(8))
    return byte, all((sixteen >> (14 - 2 * k)) & 1 for k in range(8))


def lich_fields(byte: int) -> dict:
    """The named fields of a LICH byte; ``parity_ok``: bit 0 is the XOR of the bits 7 .. 4."""
    return dict(rf=byte >> 6, fn=byte >> 4 & 3, option=byte >> 2 & 3, outbound=byte >> 1 & 1,
                parity_ok=(byte >> 7 ^ byte >> 6 ^ byte >> 5 ^ byte >> 4 ^ byte) & 1 == 0)


def lich_mask(rf: int, fn: int, option: int) -> int:
    """The class mask that a LICH asks for: CAC for an outbound control frame, SACCH and the FACCH1s that the option names
    for a traffic frame, 0 for what is not read (inbound control, UDCH)."""
    if rf == 0:
        return CAC if fn == 0 else 0
    if fn == 1:
        return 0
    return SACCH | {3: 0, 2: FACCH1_A, 1: FACCH1_B, 0: FACCH1_A | FACCH1_B}[option]


def layer3_fields(data, whole: bool = True) -> dict:
    """The fields of a layer-3 message (``data``: its octets): ``type``, ``name`` and ``hex``, and for a VCALL or a TX_REL of
    eight octets or more (``whole``) the call's fields."""
    data = bytes(data)
    kind = data[0] & 0x3F
    out = dict(type=kind, name=MESSAGES.get(kind, f"0x{kind:02X}"), hex=data.hex())
    if whole and kind in (VCALL, TX_REL) and len(data) >= 8:
        out.update(emergency=data[1] >> 7, call_type=data[2] >> 5, mode=data[2] & 7, src=data[3] << 8 | data[4], dst=data[5] << 8 | data[6],
                   cipher=data[7] >> 6, key=data[7] & 0x3F)
    return out


# ---- the device calls ---------------------------------------------------------------------------------------------------------


def slice_frames(plane, rows, plan: P.NxdnPlan) -> tuple:
    """``iqa_nxdn_slice`` on a device int32 plane for ``rows`` (int64[K][2]: m, s): (bits uint32[K][12], descrambled, levels
    int64[K][3]: A, Dc, valid) on the host.  ``ValueError`` for a sign other than +-1, before anything is launched."""
    return L.slice_frames("iqa_nxdn_slice", plane, rows, plan.offsets, P.NXDN_WORDS)


def decode_frames(bits, classes) -> tuple:
    """``iqa_nxdn_decode`` on ``bits`` (uint32[K][12], host) with the class masks ``classes`` (K values: 0, CAC alone, or any
    of SACCH | FACCH1_A | FACCH1_B): (info uint32[K][14], rec int32[K][4]) on the host.  ``ValueError`` for another value, before
    anything is launched."""
    bits = L.word_rows(bits, P.NXDN_WORDS)
    classes = L.frame_classes("iqa_nxdn_decode", bits, classes, "class mask", CAC, "0 .. 7 or 8")
    k = bits.shape[0]
    return tuple(L.device_rows("iqa_nxdn_decode", k, k == 0, bits.view(np.int32), classes.astype(np.uint8), c_int64(k),
                               L.Out(P.NXDN_INFO, np.uint32), L.Out(RECORD, np.int32)))


# ---- the frames ---------------------------------------------------------------------------------------------------------------


def frame_hits(hits, pats, half: int) -> np.ndarray:
    """int64[K][2], (m, s) in order of m: of the kept hits (int64[K][6] of section 25, ``pats`` the patterns searched for) every
    hit of the ``nxdn`` pattern, less those with another within +-``half`` that has a larger |C|, or the same |C| at a smaller
    m (section 29's keep rule)."""
    return L.sync_hits(hits, pats, "nxdn", half)


def decoder_classes(bits, levels) -> np.ndarray:
    """The class mask that picks a frame's decoders: ``lich_mask`` of its LICH where the frame is whole, has a level and the
    LICH holds its parity, else 0 (nothing is read)."""
    out = []
    for words, (amp, _dc, valid) in zip(np.asarray(bits).tolist(), np.asarray(levels).tolist()):
        f = lich_fields(lich_of(words)[0])
        out.append(lich_mask(f["rf"], f["fn"], f["option"]) if valid >= NEED_FRAME and amp > 0 and f["parity_ok"] else 0)
    return np.array(out, dtype=np.uint8)


@dataclass
class NxdnFrame(L.JsonRecord):
    time_s: float  # where sync symbol 0 ends, in seconds of the stream
    lich: int
    rf: int
    fn: int
    option: int
    outbound: int
    cls: int  # ``lich_mask``
    corrected: bool  # a good block was corrected
    ran: int | None = None  # the radio access number of a good SACCH or CAC
    structure: int | None = None  # ... and its structure field
    blocks: list = field(default_factory=list)  # the blocks that were read: [name, the bits in front of the CRC as hex, the CRC held]
    messages: list = field(default_factory=list)  # the layer-3 messages: ``layer3_fields`` with ``via``, the block that brought it

    def kind(self) -> str:
        return f"{RF[self.rf]} {(FN_CONTROL if self.rf == 0 else FN_TRAFFIC)[self.fn]}"


def new_counts() -> dict:
    return dict(no_level=0, cut=0, lich_inner=0, lich_failed=0, sacch_failed=0, facch_failed=0, cac_failed=0, superframe_broken=0, udch=0,
                inbound_cac=0, fixed=0)


def join_superframes(frames) -> int:
    """Joins the SACCH parts of the superframe frames among ``frames`` (``NxdnFrame``s in order of time, each with ``_part``: the
    18 data bits of its good SACCH as an integer, or None): the structures 3, 2, 1, 0 of consecutive traffic frames with one RAN make a
    72-bit message, which the frame of the last part gets (``via`` "sacch").  Returns the superframes that were dropped: one
    with a part that is missing, failed or out of turn counts once, and its other parts are passed over until the next part 3."""
    broken, parts, ran, skipping = 0, [], None, False
    for f in frames:
        if f.rf == 0:
            continue
        part = f._part if f.fn == 2 else None
        if part is not None and f.structure == 3:
            broken += bool(parts)
            parts, ran, skipping = [part], f.ran, False
        elif part is not None and parts and f.structure == 3 - len(parts) and f.ran == ran:
            parts.append(part)
            if f.structure == 0:
                f.messages.append(dict(via="sacch", **layer3_fields((parts[0] << 54 | parts[1] << 36 | parts[2] << 18 | parts[3]).to_bytes(9, "big"))))
                parts = []
        else:
            if f.fn != 2 and not parts:
                continue  # (a frame outside a superframe, between two of them)
            broken += bool(parts) or not skipping
            parts, skipping = [], True
    return broken + bool(parts)


def parse_frames(rows, bits, levels, info, rec, fs_ch: float, keyed_from: int = 0) -> tuple:
    """(frames, counts): every frame whose LICH held its parity as an ``NxdnFrame``, in order of time; ``rows`` int64[K][2] (m, s),
    ``bits`` uint32[K][12], ``levels`` int64[K][3], ``info`` uint32[K][14] and ``rec`` int32[K][4].  A frame cut in front of the end
    of its LICH, one with A <= 0 and one whose LICH fails are counted and left out; a frame cut in front of its end is counted
    and kept without its blocks.  ``fixed`` counts the frames that are kept and were corrected."""
    counts = new_counts()
    out = []
    for (m, _s), words, (amp, _dc, valid), iw, r in zip(np.asarray(rows).tolist(), np.asarray(bits).tolist(), np.asarray(levels).tolist(),
                                                        np.asarray(info).tolist(), np.asarray(rec).tolist()):
        if valid < NEED_LICH:
            counts["cut"] += 1
            continue
        if amp <= 0:
            counts["no_level"] += 1
            continue
        byte, outer = lich_of(words)
        counts["lich_inner"] += not outer
        fields = lich_fields(byte)
        if not fields.pop("parity_ok"):
            counts["lich_failed"] += 1
            continue
        f = NxdnFrame(time_s=(int(keyed_from) + m) / fs_ch, lich=byte, cls=lich_mask(fields["rf"], fields["fn"], fields["option"]), corrected=False, **fields)
        f._part = None
        counts["inbound_cac"] += f.rf == 0 and f.fn != 0
        counts["udch"] += f.rf != 0 and f.fn == 1
        if f.cls and valid < NEED_FRAME:
            counts["cut"] += 1
        elif f.cls & CAC:
            b, ok = block_of(iw[8:14], "cac")
            f.blocks.append(["cac", f"{b:039x}", ok])
            counts["cac_failed"] += not ok
            if ok:
                f.corrected = r[1] > 0
                f.structure, f.ran = b >> 153, b >> 147 & 0x3F
                f.messages.append(dict(via="cac", **layer3_fields((b >> 3 & (1 << 144) - 1).to_bytes(18, "big"))))
        elif f.cls:
            b, ok = block_of(iw[0:2], "sacch")
            f.blocks.append(["sacch", f"{b:07x}", ok])
            counts["sacch_failed"] += not ok
            if ok:
                f.corrected = r[1] > 0
                f.structure, f.ran = b >> 24, b >> 18 & 0x3F
                if f.fn == 2:
                    f._part = b & 0x3FFFF
                elif f.fn == 0:
                    f.messages.append(dict(dict(via="sacch", **layer3_fields(bytes([b >> 10 & 0xFF]), whole=False)), hex=f"{b & 0x3FFFF:05x}"))
            for name, bit, at, slot in (("facch1-a", FACCH1_A, 2, 2), ("facch1-b", FACCH1_B, 5, 3)):
                if not f.cls & bit:
                    continue
                b, ok = block_of(iw[at : at + 3], "facch1")
                f.blocks.append([name, f"{b:020x}", ok])
                counts["facch_failed"] += not ok
                if ok:
                    f.corrected = f.corrected or r[slot] > 0
                    f.messages.append(dict(via=name, **layer3_fields(b.to_bytes(10, "big"))))
        out.append(f)
    out.sort(key=lambda f: f.time_s)
    counts["superframe_broken"] = join_superframes(out)
    for f in out:
        del f._part
        counts["fixed"] += f.corrected
    return out, counts


@dataclass
class NxdnCall(L.JsonRecord):
    start_s: float
    end_s: float
    frames: int
    ran: int | None
    src: int | None
    dst: int | None
    call_type: int | None
    emergency: int | None
    mode: int | None
    cipher: int | None
    key: int | None
    late: bool  # the first frame seen was no non-superframe frame with a VCALL in its FACCH1
    released: bool  # closed by a TX_REL
    conflicts: int  # values of good VCALLs that differ from the first that was seen

    def line(self) -> str:
        parts = ["NXDN"]
        if self.ran is not None:
            parts.append(f"RAN {self.ran}")
        if self.src is not None:
            parts.append(str(self.src))
        if self.dst is not None:
            parts += ["->", str(self.dst)]
        if self.call_type is not None:
            parts.append(CALL_TYPES.get(self.call_type, str(self.call_type)))
        if self.cipher is not None:
            parts.append("clear" if self.cipher == 0 else f"cipher {self.cipher}")
        parts.append(f"{self.end_s - self.start_s:.2f} s ({self.frames} frame{'' if self.frames == 1 else 's'})")
        return " ".join(parts)


def track_calls(frames) -> list:
    """The calls of the traffic frames among ``frames`` (``parse_frames``' list, in order of time), in order of their start: the
    first frame opens one where none is open (``late`` unless it is a non-superframe frame with a VCALL in a FACCH1); the RAN
    of a good SACCH and the fields of every good VCALL fill what is still unknown, and a value that differs from a known one
    counts a conflict and changes nothing; a TX_REL closes the call as released; no frame for more than ``HANG_S`` closes it at
    its last frame."""
    out, call, last = [], None, 0.0
    for f in frames:
        if f.rf == 0:
            continue
        if call is not None and f.time_s - last > HANG_S:
            call = None  # (its end is its last frame's time already)
        last = f.time_s
        vcalls = [msg for msg in f.messages if msg["type"] == VCALL and "src" in msg]
        if call is None:
            late = not (f.fn == 0 and any(msg["via"].startswith("facch1") for msg in vcalls))
            call = NxdnCall(f.time_s, f.time_s, 0, None, None, None, None, None, None, None, None, late, False, 0)
            out.append(call)
        call.frames += 1
        call.end_s = f.time_s
        known = [("ran", f.ran)] if f.ran is not None else []
        for name, value in known + [(name, msg[name]) for msg in vcalls for name in CALL_FIELDS]:
            if getattr(call, name) is None:
                setattr(call, name, value)
            elif getattr(call, name) != value:
                call.conflicts += 1
        if any(msg["type"] == TX_REL for msg in f.messages):
            call.released = True
            call = None
    return out


@dataclass
class NxdnControl(L.JsonRecord):
    ran: int
    type: int
    name: str
    hex: str  # the 18 octets of the message
    count: int
    first_s: float
    last_s: float

    def line(self) -> str:
        return f"NXDN RAN {self.ran} {self.name} {self.hex} x{self.count} {self.first_s:.2f} .. {self.last_s:.2f} s"


def fold_control(frames) -> list:
    """One ``NxdnControl`` per distinct CAC message (RAN, type, hex) of the ``frames``, in order of its first appearance."""
    seen = {}
    for f in frames:
        for msg in f.messages:
            if msg["via"] != "cac":
                continue
            key = (f.ran, msg["type"], msg["hex"])
            if key not in seen:
                seen[key] = NxdnControl(f.ran, msg["type"], msg["name"], msg["hex"], 0, f.time_s, f.time_s)
            seen[key].count += 1
            seen[key].last_s = f.time_s
    return list(seen.values())


# ---- the results --------------------------------------------------------------------------------------------------------------


@dataclass
class NxdnChannel(L.JsonRecord, L.ChannelLabel):
    offset_hz: float  # the finder's
    freq_hz: float | None
    rate: int = 0  # the symbol rate it was read at: 4800 or 2400; 0 where nothing was decoded
    frames: dict = field(default_factory=dict)  # frames per kind ("RTCH superframe", "RCCH outbound", ...)
    no_level: int = 0  # frames dropped for A <= 0
    cut: int = 0  # frames cut by the end of the stream
    lich_inner: int = 0  # frames with a LICH symbol that is no outer level
    lich_failed: int = 0
    sacch_failed: int = 0
    facch_failed: int = 0  # blocks
    cac_failed: int = 0
    superframe_broken: int = 0
    udch: int = 0  # seen, not read
    inbound_cac: int = 0  # seen, not read
    fixed: int = 0  # kept frames in which something was corrected
    inverted: bool = False  # most of its sync hits were negative: the spectrum is inverted
    calls: list = field(default_factory=list)  # NxdnCall, in order of their start
    control: list = field(default_factory=list)  # NxdnControl, in order of first appearance
    note: str = ""  # why nothing was decoded
    NESTED = {"calls": NxdnCall, "control": NxdnControl}

    def lines(self) -> list:
        """One line per call, in order of time, then one per distinct control message."""
        return [f"{self.label()}: {x.line()}" for x in self.calls + self.control]


@dataclass
class NxdnResult(L.JsonRecord, L.ChannelLines):
    channels: list = field(default_factory=list)  # NxdnChannel, in the order of the FindResult's channels
    sample_rate: float = 0.0
    center_freq: float | None = None
    NESTED = {"channels": NxdnChannel}

    @property
    def calls(self) -> list:
        return [c for ch in self.channels for c in ch.calls]


# ---- one stream ---------------------------------------------------------------------------------------------------------------


def decode_stream(theta, plan: P.NxdnPlan, centre: int, hits, pats, v=None) -> dict:
    """Everything behind the frame sync words of one stored stream (device float32 ``theta``; ``hits`` section 25's kept hits of it
    for the patterns ``pats``): ``rows`` (int64[K][2]: m, s), ``bits`` (uint32[K][12]) and ``levels`` (int64[K][3]) of
    ``iqa_nxdn_slice``, ``classes`` (uint8[K]), ``info`` (uint32[K][14]) and ``rec`` (int32[K][4]) of ``iqa_nxdn_decode``, ``rate``
    and the plane."""
    rows = frame_hits(hits, pats, plan.ident.half)
    if v is None:
        v = I.integrate(theta, plan.ident, centre)
    bits, levels = slice_frames(v, rows, plan)
    classes = decoder_classes(bits, levels)
    info, rec = decode_frames(bits, classes)
    return dict(rows=rows, bits=bits, levels=levels, classes=classes, info=info, rec=rec, rate=plan.rate, v=v)


def channel_of(st: dict, fs_ch: float, keyed_from: int, offset_hz: float, freq_hz) -> "NxdnChannel":
    """The ``NxdnChannel`` of ``decode_stream``'s output."""
    frames, counts = parse_frames(st["rows"], st["bits"], st["levels"], st["info"], st["rec"], fs_ch, keyed_from)
    out = NxdnChannel(offset_hz=offset_hz, freq_hz=freq_hz, rate=st["rate"], **counts)
    for f in frames:
        out.frames[f.kind()] = out.frames.get(f.kind(), 0) + 1
    out.inverted = L.mostly_inverted(st["rows"])
    out.calls = track_calls(frames)
    out.control = fold_control(frames)
    return out


# ---- the layer of the second pass (describe.py) ---------------------------------------------------------------------------------

#: ``finish_nxdn`` reads the planes of both NXDN families; ``stages()`` shows ``nxdn_rows`` ((m, s) per frame, None where the channel
#: is no NXDN channel) and, with ``keep_stages``, ``nxdn_plan`` and these
LAYER = L.ProtocolLayer("nxdn", (4800, 2400), P.plan_nxdn, "nxdn", decode_stream, channel_of, NxdnChannel, NxdnResult,
                        keys=("bits", "levels", "classes", "info", "rec"))
PLANE_RATES, finish_nxdn, nxdn_result, stage_keys = LAYER.rates, LAYER.finish, LAYER.result_of, LAYER.stage_keys


class NxdnDecoder(L.StoredTheta):
    """An NXDN decoder for one discriminator stream from Python (``protocol_layer.StoredTheta``) at ``rate`` symbols/s (4800 or
    2400): ``finish()`` gives an ``NxdnResult`` of one channel, ``stages()`` ``decode_stream``'s output with the plane on the
    host, and ``hits``."""

    patterns, layer = NXDN_PATTERNS, LAYER

    def __init__(self, fs_ch: float, centre: int = 0, rate: int = 4800):
        self.rate = int(rate)
        self.plan = P.plan_nxdn(fs_ch, self.rate)
        self.centre = int(centre)
        self.reset()
