"""The network identifiers, the link control and the trunking blocks of a P25 phase 1 channel (``--find-p25``, DESIGN.md section
31): from the stored discriminator stream of a channel and the P25 frame sync hits that section 25 keeps (``identify.py``) to
which system it is (NAC, WACN, system, site), who talks to whom and for how long, and on a control channel which talkgroup was
granted which frequency.

``iqa_p25_slice`` takes the levels of every frame from its sync word and slices the 864 symbols behind it; ``iqa_p25_nid``
finds the nearest codeword of BCH(63,16,23) for the NID; ``iqa_p25_decode`` reads, by DUID, the Hamming(10,6,3) words of an
LDU1, the Golay(24,12,8) words of a TDULC or the three trellis blocks of a TSBK frame.  The host checks the link control
(Reed-Solomon(24,12,13) syndromes) and the blocks (CRC-CCITT), reads their fields (``parse_frames``), follows the calls
(``track_calls``) and folds a control channel's repetitions (``collapse_tsbks``): integer logic.  The constants are written
from memory of TIA-102.BAAA and of open-source readers of it, not checked against either here.  Nothing is listened to: no
vocoder, no HDU body, no LDU2.  No CPU path: without a GPU or the built library the device calls raise ``RuntimeError``.

What every protocol layer shares lives in ``protocol_layer.py``: the stored stream under ``P25Decoder``, the device call on host
rows under ``slice_frames`` / ``decode_nids`` / ``decode_frames``, the keep rule under ``frame_hits``, the per-lane loop under
``finish_p25``, the builder under ``p25_result``, and ``label`` / ``lines`` / ``to_json`` / ``from_json`` of the results."""
from __future__ import annotations

from ctypes import c_int64
from dataclasses import dataclass, field

import numpy as np

from . import dsp_plan as P
from . import identify as I
from . import protocol_layer as L

P25_PATTERNS = tuple(p for p in I.PATTERNS if p.protocol == "p25")  # one word; a hit with C < 0 is the same word, spectrum inverted
SYNC = P25_PATTERNS[0].word
STATUS_EVERY = 36  # the symbols i mod 36 = 35 are status symbols
BCH_POLY = 0o6331141367235453  # derived in the kernel and in the model; the host test holds this copy to both
BCH_MAX_DISTANCE = 11
GOLAY_POLY = 0xC75
GOLAY_MAX_DISTANCE = 3
HAMMING_COLUMNS = (0b1110, 0b1101, 0b1011, 0b0111, 0b0011, 0b1100)  # the parity parts p0 p1 p2 p3 of d0 .. d5
TRELLIS_PAIRS = ((0, 2), (2, 2), (1, 3), (3, 3), (3, 2), (1, 2), (2, 3), (0, 3), (3, 1), (1, 1), (2, 0), (0, 0), (0, 1), (2, 1), (1, 0), (3, 0))
TRELLIS_POINTS = ((0, 15, 12, 3), (4, 11, 8, 7), (13, 2, 1, 14), (9, 6, 5, 10))  # point[state][input]
INTERLEAVE = tuple(x for r in range(4) for k in range(13 if r == 0 else 12) for x in (8 * k + 2 * r, 8 * k + 2 * r + 1))
GF_POLY = 0x43  # x^6 + x + 1
RS_ROOTS = 12  # alpha^1 .. alpha^12
CRC_POLY = L.CRC_POLY
DUIDS = {0x0: "hdu", 0x5: "ldu1", 0xA: "ldu2", 0x3: "tdu", 0xF: "tdulc", 0x7: "tsbk", 0xC: "pdu"}
LCO = {0: "group", 3: "unit"}
HANG_S = 0.360  # a call with no frame for longer closes at its last frame
NID_RECORD = 4  # status, distance, value, parity_ok
RECORD = P.P25_RECORD  # class, then (corrected, refused or unmatched, bits changed) or the three block metrics
LC_FIRST, LC_STEP = 400, 184  # an LDU1's LC group g: data bits 400 + 184 g .. + 39, four Hamming words
TSBK_FIRST, TSBK_BITS = 112, 196  # a TSBK frame's block b: data bits 112 + 196 b .. + 195


def symbol_of(q: int) -> int:
    """The frame symbol of data dibit ``q``: the status symbols skipped."""
    return q + q // (STATUS_EVERY - 1)


NEED_NID = symbol_of(111 // 2) + 1  # the ``valid`` that covers data bit 111
NEED_TDULC = symbol_of(399 // 2) + 1
NEED_LDU1 = symbol_of((LC_FIRST + 5 * LC_STEP + 39) // 2) + 1
NEED_TSBK = tuple(symbol_of((TSBK_FIRST + TSBK_BITS * (b + 1) - 1) // 2) + 1 for b in range(3))


# ---- the checks and the fields (host, integers) ---------------------------------------------------------------------------------


_EXP, _LOG, gf_mul = L.gf_tables(GF_POLY, 6)
info_bytes, crc_ccitt = L.info_bytes, L.crc_ccitt  # the bytes of information words; CRC_POLY from 0


def check_lc(hexbits) -> bool:
    """Whether the 24 hexbits (the first the highest coefficient) have the roots alpha^1 .. alpha^12: a word of RS(24,12,13)."""
    hexbits = [int(h) for h in hexbits]
    for j in range(1, RS_ROOTS + 1):
        acc = 0
        for h in hexbits:  # Horner: acc alpha^j + h, the product by the logarithms
            acc = (_EXP[_LOG[acc] + j] if acc else 0) ^ h
        if acc:
            return False
    return True


def check_tsbk(by) -> bool:
    """Whether the complemented CRC-CCITT of bytes 0 .. 9 of a block equals bytes 10 .. 11."""
    by = [int(b) for b in by]
    return (crc_ccitt(by[:10]) ^ 0xFFFF) == (by[10] << 8 | by[11])


def info_hexbits(words) -> list:
    """The 24 hexbits in the first 144 bits of the information words."""
    value = 0
    for w in list(words)[:5]:
        value = value << 32 | int(w)
    return [(value >> (160 - 6 * (j + 1))) & 0x3F for j in range(24)]


def lc_fields(hexbits) -> dict:
    """The fields of the nine link control bytes in front of the parity hexbits."""
    value = 0
    for h in hexbits[:12]:
        value = value << 6 | int(h)
    by = [(value >> (64 - 8 * j)) & 0xFF for j in range(9)]
    out = dict(lco=by[0] & 0x3F, mfid=by[1], src=None, dst=None, hex="".join(f"{b:02x}" for b in by))
    if out["lco"] == 0:
        out.update(dst=by[4] << 8 | by[5], src=by[6] << 16 | by[7] << 8 | by[8])
    elif out["lco"] == 3:
        out.update(dst=by[3] << 16 | by[4] << 8 | by[5], src=by[6] << 16 | by[7] << 8 | by[8])
    return out


def tsbk_fields(opcode: int, mfid: int, args: int) -> dict:
    """The named fields of a block's 64 argument bits; empty for an opcode that is kept as hex."""
    if mfid != 0:
        return {}
    if opcode == 0x00:
        return dict(kind="group grant", svc=args >> 56, channel=args >> 40 & 0xFFFF, tgid=args >> 24 & 0xFFFF, src=args & 0xFFFFFF)
    if opcode == 0x02:
        return dict(kind="grant update", channel=args >> 48, tgid=args >> 32 & 0xFFFF, channel2=args >> 16 & 0xFFFF, tgid2=args & 0xFFFF)
    if opcode == 0x3A:
        return dict(kind="rfss status", lra=args >> 56, flags=args >> 52 & 0xF, system=args >> 40 & 0xFFF, rfss=args >> 32 & 0xFF,
                    site=args >> 24 & 0xFF, channel=args >> 8 & 0xFFFF, svc=args & 0xFF)
    if opcode == 0x3B:
        return dict(kind="network status", lra=args >> 56, wacn=args >> 36 & 0xFFFFF, system=args >> 24 & 0xFFF, channel=args >> 8 & 0xFFFF,
                    svc=args & 0xFF)
    if opcode == 0x3D:
        return dict(kind="identifier update", id=args >> 60, bandwidth=args >> 51 & 0x1FF, tx_offset=args >> 42 & 0x1FF,
                    spacing=args >> 32 & 0x3FF, base=args & 0xFFFFFFFF)
    return {}


def channel_hz(channel: int, idens: dict):
    """The frequency of a channel ``id (4) | number (12)`` by the identifier updates ``idens`` (id -> (base, spacing)), or None."""
    if channel >> 12 not in idens:
        return None
    base, spacing = idens[channel >> 12]
    return base * 5 + (channel & 0xFFF) * spacing * 125


def _ch(channel: int, idens: dict) -> str:
    hz = channel_hz(channel, idens)
    return f"ch 0x{channel:04x}" + ("" if hz is None else f" ({hz / 1e6:.4f} MHz)")


def tsbk_text(opcode: int, mfid: int, args: int, idens: dict) -> str:
    f = tsbk_fields(opcode, mfid, args)
    kind = f.get("kind")
    if kind == "group grant":
        return f"group grant tg {f['tgid']} src {f['src']} {_ch(f['channel'], idens)}"
    if kind == "grant update":
        return f"grant update tg {f['tgid']} {_ch(f['channel'], idens)}, tg {f['tgid2']} {_ch(f['channel2'], idens)}"
    if kind == "rfss status":
        return f"rfss status system 0x{f['system']:03x} rfss {f['rfss']} site {f['site']} {_ch(f['channel'], idens)}"
    if kind == "network status":
        return f"network status wacn 0x{f['wacn']:05x} system 0x{f['system']:03x} {_ch(f['channel'], idens)}"
    if kind == "identifier update":
        return f"identifier update id {f['id']} base {f['base'] * 5 / 1e6:.4f} MHz spacing {f['spacing'] * 0.125:g} kHz"
    return f"o=0x{opcode:02x} mfid=0x{mfid:02x} {args:016x}"


# ---- the device calls ---------------------------------------------------------------------------------------------------------


def slice_frames(plane, rows, plan: P.P25Plan) -> tuple:
    """``iqa_p25_slice`` on a device int32 plane for ``rows`` (int64[K][2]: m, s): (bits uint32[K][54], levels int64[K][3]: A, Dc,
    valid) on the host.  ``ValueError`` for a sign other than +-1, before anything is launched."""
    return L.slice_frames("iqa_p25_slice", plane, rows, plan.offsets, P.P25_WORDS)


def decode_nids(bits) -> np.ndarray:
    """``iqa_p25_nid`` on ``bits`` (uint32[K][54], host): int32[K][4] (status, distance, value, parity_ok) on the host."""
    bits = L.word_rows(bits, P.P25_WORDS)
    k = bits.shape[0]
    return L.device_rows("iqa_p25_nid", k, k == 0, bits.view(np.int32), c_int64(k), L.Out(NID_RECORD, np.int32))[0]


def decode_frames(bits, duids) -> tuple:
    """``iqa_p25_decode`` on ``bits`` (uint32[K][54], host) of the ``duids`` (K values 0 .. 15): (info uint32[K][9], rec
    int32[K][8]) on the host.  ``ValueError`` for a DUID over 15, before anything is launched."""
    bits = L.word_rows(bits, P.P25_WORDS)
    duids = L.frame_classes("iqa_p25_decode", bits, duids, "DUID", 15, "0 .. 15")
    k = bits.shape[0]
    return tuple(L.device_rows("iqa_p25_decode", k, k == 0, bits.view(np.int32), duids.astype(np.uint8), c_int64(k),
                               L.Out(P.P25_INFO, np.uint32), L.Out(RECORD, np.int32)))


# ---- the frames ---------------------------------------------------------------------------------------------------------------


def frame_hits(hits, pats, half: int) -> np.ndarray:
    """int64[K][2], (m, s) in order of m: of the kept hits (int64[K][6] of section 25, ``pats`` the patterns searched for) every
    hit of the ``p25`` pattern, less those with another within +-``half`` that has a larger |C|, or the same |C| at a smaller
    m (section 29's keep rule)."""
    return L.sync_hits(hits, pats, "p25", half)


def apply_flags(nid, levels) -> np.ndarray:
    """``nid`` of ``iqa_p25_nid`` with the cuts of ``iqa_p25_slice`` written in: a status of 3 for a frame whose ``valid`` does not
    cover the NID."""
    nid = np.array(nid, dtype=np.int32).reshape(-1, NID_RECORD)
    nid[np.asarray(levels, dtype=np.int64).reshape(-1, 3)[:, 2] < NEED_NID, 0] = 3
    return nid


def decoder_duids(nid) -> np.ndarray:
    """The DUID that picks a frame's decoder: the NID's low four bits where its status is 0 or 1, else 0 (nothing is read)."""
    nid = np.asarray(nid, dtype=np.int64).reshape(-1, NID_RECORD)
    return np.where(nid[:, 0] <= 1, nid[:, 2] & 15, 0)


@dataclass
class P25Frame(L.JsonRecord):
    time_s: float  # where sync symbol 0 ends, in seconds of the stream
    nac: int
    duid: int
    name: str  # DUIDS' name, or "reserved"
    corrected: bool  # the NID or a word behind it was corrected
    checked: bool | None  # the link control's check held (True) or failed (False); None: no link control was read
    lco: int | None = None
    mfid: int | None = None
    src: int | None = None
    dst: int | None = None  # the talkgroup (LCO 0) or the destination unit (LCO 3)
    hex: str | None = None  # the nine link control bytes
    blocks: list = field(default_factory=list)  # a TSBK frame's blocks that were read: [the twelve bytes as hex, the CRC held]

    def line(self) -> str:
        head = f"P25 nac=0x{self.nac:03x} {self.name}"
        if self.checked is False:
            return f"{head} (failed)"
        if self.lco in LCO:
            return f"{head} {LCO[self.lco]} {self.src} -> {self.dst}"
        return f"{head} {self.hex or ''}".rstrip()


def new_counts() -> dict:
    return dict(no_level=0, cut=0, nid_refused=0, nid_fixed=0, lc_failed=0, crc_failed=0, golay_refused=0, hamming_unmatched=0)


def parse_frames(rows, levels, nid, info, rec, fs_ch: float, keyed_from: int = 0) -> tuple:
    """(frames, counts): every frame whose NID was read as a ``P25Frame``, in order of time; ``rows`` int64[K][2] (m, s), ``levels``
    int64[K][3], ``nid`` int32[K][4] (``apply_flags``' form), ``info`` uint32[K][9] and ``rec`` int32[K][8].  A frame cut in front of
    the end of its NID, one with A <= 0 and one whose NID is refused are counted and left out; a frame cut in front of the end
    of what its DUID sends is counted and kept without it."""
    counts = new_counts()
    out = []
    for (m, _s), (amp, _dc, valid), (status, _dist, value, _par), words, r in zip(
            np.asarray(rows).tolist(), np.asarray(levels).tolist(), np.asarray(nid).tolist(), np.asarray(info).tolist(), np.asarray(rec).tolist()):
        if status == 3:
            counts["cut"] += 1
            continue
        if amp <= 0:
            counts["no_level"] += 1
            continue
        if status == 2:
            counts["nid_refused"] += 1
            continue
        counts["nid_fixed"] += status == 1
        duid = value & 15
        f = P25Frame(time_s=(int(keyed_from) + m) / fs_ch, nac=value >> 4, duid=duid, name=DUIDS.get(duid, "reserved"),
                     corrected=status == 1, checked=None)
        if duid in (0x5, 0xF):
            if valid < (NEED_LDU1 if duid == 0x5 else NEED_TDULC):
                counts["cut"] += 1
            else:
                counts["hamming_unmatched" if duid == 0x5 else "golay_refused"] += r[2]
                hexbits = info_hexbits(words)
                f.checked, f.corrected = check_lc(hexbits), f.corrected or r[1] > 0
                if f.checked:
                    for key, x in lc_fields(hexbits).items():
                        setattr(f, key, x)
                else:
                    counts["lc_failed"] += 1
        elif duid == 0x7:
            for b in range(3):
                if valid < NEED_TSBK[b]:
                    counts["cut"] += 1
                    break
                by = info_bytes(words[3 * b : 3 * b + 3])
                ok = check_tsbk(by)
                counts["crc_failed"] += not ok
                f.blocks.append(["".join(f"{x:02x}" for x in by), ok])
                f.corrected = f.corrected or r[1 + b] > 0
                if by[0] & 0x80:
                    break
        out.append(f)
    out.sort(key=lambda f: f.time_s)
    return out, counts


@dataclass
class P25Call(L.JsonRecord):
    start_s: float
    end_s: float
    nac: int
    group: bool | None  # None for a late entry: no checked link control was seen
    src: int | None
    dst: int | None
    ldus: int
    terminated: bool

    def line(self) -> str:
        who = "late entry" if self.group is None else f"{'group' if self.group else 'unit'} {self.src} -> {self.dst}"
        frames = f"{self.ldus} ldu{'' if self.ldus == 1 else 's'}"
        return f"P25 nac=0x{self.nac:03x} {who} {self.end_s - self.start_s:.2f} s ({frames}{'' if self.terminated else ', not terminated'})"


VOICE_DUIDS = (0x0, 0x5, 0xA, 0x3, 0xF)


def track_calls(frames) -> list:
    """The calls of the ``frames`` (``parse_frames``' list, in order of time), in order of their start: an HDU or an LDU opens a
    call where none is open (a late entry until ids are known), a checked link control of LCO 0 or 3 in an LDU1 or a TDULC sets
    (group, src, dst), other ids than the open call's close it and open a new one; every LDU adds one; a TDU or a TDULC closes
    the call as terminated; no frame of these kinds for more than ``HANG_S`` closes it at its last frame."""
    calls, call, last = [], None, 0.0
    for f in frames:
        if f.duid not in VOICE_DUIDS:
            continue
        if call is not None and f.time_s - last > HANG_S:
            call = None  # (its end is its last frame's time already)
        last = f.time_s

        def opened():
            new = P25Call(f.time_s, f.time_s, f.nac, None, None, None, 0, False)
            calls.append(new)
            return new

        if f.duid in (0x0, 0x5, 0xA) and call is None:
            call = opened()
        if f.checked and f.lco in LCO and (call is not None or f.duid == 0x5):
            ids = (f.lco == 0, f.src, f.dst)
            if call is not None and call.group is not None and (call.group, call.src, call.dst) != ids:
                call = opened()
            call.group, call.src, call.dst = ids
        if call is None:
            continue
        call.end_s = f.time_s
        if f.duid in (0x5, 0xA):
            call.ldus += 1
        elif f.duid in (0x3, 0xF):
            call.terminated = True
            call = None
    return calls


@dataclass
class P25Tsbk(L.JsonRecord):
    opcode: int
    mfid: int
    args: str  # the 64 argument bits as hex
    nac: int  # of the first frame that carried it
    count: int
    first_s: float
    last_s: float
    text: str  # the fields by name, or the block as hex

    def line(self) -> str:
        return f"P25 nac=0x{self.nac:03x} tsbk {self.text} x{self.count}"


def collapse_tsbks(frames) -> list:
    """The distinct (opcode, mfid, args) of the blocks whose CRC held, in order of their first time, with ``count``, ``first_s`` and
    ``last_s``; a channel's frequency is named where an identifier update of its id was seen on the channel (the first of an id
    holds)."""
    seen, idens = {}, {}
    for f in frames:
        for text, ok in f.blocks:
            if not ok:
                continue
            by = bytes.fromhex(text)
            key = (by[0] & 0x3F, by[1], int.from_bytes(by[2:10], "big"))
            fields = tsbk_fields(*key)
            if fields.get("kind") == "identifier update":
                idens.setdefault(fields["id"], (fields["base"], fields["spacing"]))
            if key in seen:
                seen[key].count += 1
                seen[key].last_s = f.time_s
            else:
                seen[key] = P25Tsbk(key[0], key[1], f"{key[2]:016x}", f.nac, 1, f.time_s, f.time_s, "")
    for key, t in seen.items():
        t.text = tsbk_text(*key, idens)
    return list(seen.values())


# ---- the results --------------------------------------------------------------------------------------------------------------


@dataclass
class P25Channel(L.JsonRecord, L.ChannelLabel):
    offset_hz: float  # the finder's
    freq_hz: float | None
    nacs: dict = field(default_factory=dict)  # frames per NAC ("0x293")
    frames: dict = field(default_factory=dict)  # frames per DUID name
    no_level: int = 0  # frames dropped for A <= 0
    cut: int = 0  # frames cut by the end of the stream
    nid_refused: int = 0
    nid_fixed: int = 0
    lc_failed: int = 0
    crc_failed: int = 0
    golay_refused: int = 0  # words
    hamming_unmatched: int = 0  # words
    inverted: bool = False  # most of its sync hits were negative: the spectrum is inverted
    calls: list = field(default_factory=list)  # P25Call, in order of their start
    tsbks: list = field(default_factory=list)  # P25Tsbk, in order of their first time
    note: str = ""  # why nothing was decoded
    NESTED = {"calls": P25Call, "tsbks": P25Tsbk}

    def lines(self) -> list:
        """One line per call and per distinct TSBK, in order of time."""
        items = [(c.start_s, 0, j, c.line()) for j, c in enumerate(self.calls)]
        items += [(t.first_s, 1, j, t.line()) for j, t in enumerate(self.tsbks)]  # (the blocks of one frame stay in their order)
        return [f"{self.label()}: {line}" for _, _, _, line in sorted(items)]


@dataclass
class P25Result(L.JsonRecord, L.ChannelLines):
    channels: list = field(default_factory=list)  # P25Channel, in the order of the FindResult's channels
    sample_rate: float = 0.0
    center_freq: float | None = None
    NESTED = {"channels": P25Channel}

    @property
    def calls(self) -> list:
        return [call for ch in self.channels for call in ch.calls]


# ---- one stream ---------------------------------------------------------------------------------------------------------------


def decode_stream(theta, plan: P.P25Plan, centre: int, hits, pats, v=None) -> dict:
    """Everything behind the frame sync words of one stored stream (device float32 ``theta``; ``hits`` section 25's kept hits of it
    for the patterns ``pats``): ``rows`` (int64[K][2]: m, s), ``bits`` (uint32[K][54]) and ``levels`` (int64[K][3]) of
    ``iqa_p25_slice``, ``nid`` (int32[K][4], the cuts written in) of ``iqa_p25_nid``, ``info`` (uint32[K][9]) and ``rec``
    (int32[K][8]) of ``iqa_p25_decode``, and the plane."""
    rows = frame_hits(hits, pats, plan.ident.half)
    if v is None:
        v = I.integrate(theta, plan.ident, centre)
    bits, levels = slice_frames(v, rows, plan)
    nid = apply_flags(decode_nids(bits), levels)
    info, rec = decode_frames(bits, decoder_duids(nid))
    return dict(rows=rows, bits=bits, levels=levels, nid=nid, info=info, rec=rec, v=v)


def channel_of(st: dict, fs_ch: float, keyed_from: int, offset_hz: float, freq_hz) -> "P25Channel":
    """The ``P25Channel`` of ``decode_stream``'s output."""
    frames, counts = parse_frames(st["rows"], st["levels"], st["nid"], st["info"], st["rec"], fs_ch, keyed_from)
    out = P25Channel(offset_hz=offset_hz, freq_hz=freq_hz, **counts)
    for f in frames:
        out.nacs[f"0x{f.nac:03x}"] = out.nacs.get(f"0x{f.nac:03x}", 0) + 1
        out.frames[f.name] = out.frames.get(f.name, 0) + 1
    out.inverted = L.mostly_inverted(st["rows"])
    out.calls, out.tsbks = track_calls(frames), collapse_tsbks(frames)
    return out


# ---- the layer of the second pass (describe.py) ---------------------------------------------------------------------------------

#: ``finish_p25`` reads the 4800 family's plane; ``stages()`` shows ``p25_rows`` ((m, s) per frame, None where the channel is no P25
#: channel) and, with ``keep_stages``, ``p25_plan`` and these
LAYER = L.ProtocolLayer("p25", (4800,), lambda fs_ch, rate: P.plan_p25(fs_ch), "p25", decode_stream, channel_of, P25Channel, P25Result,
                        keys=("bits", "levels", "nid", "info", "rec"))
PLANE_RATES, finish_p25, p25_result, stage_keys = LAYER.rates, LAYER.finish, LAYER.result_of, LAYER.stage_keys


class P25Decoder(L.StoredTheta):
    """A P25 decoder for one discriminator stream from Python (``protocol_layer.StoredTheta``): ``finish()`` gives a
    ``P25Result`` of one channel, ``stages()`` ``decode_stream``'s output with the plane on the host, and ``hits``."""

    plan_of = staticmethod(P.plan_p25)
    patterns, layer = P25_PATTERNS, LAYER
