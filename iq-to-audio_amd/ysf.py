"""The frame information and the callsigns of a YSF (System Fusion) channel (``--find-ysf``): from the
stored discriminator stream of a channel and the YSF frame sync hits that section 25 keeps (``identify.py``) to who transmits
to whom, through which repeater, in which mode and for how long.

``iqa_ysf_slice`` takes the levels of every frame from its sync word (a least squares fit: the word holds inner levels) and
slices the 480 symbols behind it; ``iqa_ysf_fich`` decodes the frame information channel (a 16-state Viterbi decoder, four
Golay(24,12,8) words); ``iqa_ysf_decode`` decodes, by class, the data channels of header, terminator, V/D mode 1, V/D mode 2 and
data FR frames through the same Viterbi decoder.  The host checks the CRCs, removes the whitening, reads the callsigns
(``parse_frames``) and follows the transmissions (``track_transmissions``): integer logic.  The constants are written from
memory of the published specification and of open-source readers of it, not checked against either here.  Not decoded: the
voice (VCH, AMBE), the sub-header of voice FR frames, and DT1 / DT2 (GPS, text), whose bytes are kept as hex.  No CPU path:
without a GPU or the built library the device calls raise ``RuntimeError``.

What every protocol layer shares lives in ``protocol_layer.py``: the stored stream under ``YsfDecoder``, the device call on host
rows under ``slice_frames`` / ``decode_fich`` / ``decode_frames``, the keep rule under ``frame_hits``, the per-lane loop under
``finish_ysf``, the builder under ``ysf_result``, and ``label`` / ``lines`` / ``to_json`` / ``from_json`` of the results."""
from __future__ import annotations

from ctypes import c_int64
from dataclasses import dataclass, field

import numpy as np

from . import dsp_plan as P
from . import identify as I
from . import protocol_layer as L

YSF_PATTERNS = tuple(p for p in I.PATTERNS if p.protocol == "ysf")  # one word; a hit with C < 0 is the same word, spectrum inverted
SYNC = YSF_PATTERNS[0].word
SYNC_SYMBOLS = 20
LEVEL_SCALE = 584  # A and Dc are 584 times the outer level and the DC
GOLAY_POLY = 0xC75
GOLAY_MAX_DISTANCE = 3
CRC_POLY = L.CRC_POLY
INTERLEAVE_ROWS = {100: 5, 180: 9}  # coded dibit i of a block of 20 R dibits travels as dibit 20 (i mod R) + i // R
PN9_FIRST = (1, 0, 0, 1, 0, 0, 1, 1, 1)  # the whitening stream: b[n] = b[n - 5] ^ b[n - 9] behind these, MSB first
HANG_S = 0.360  # a transmission with no frame for longer closes at its last frame
FICH_RECORD = P.YSF_FICH_RECORD  # status, Viterbi metric, Golay words corrected, refused, bits changed
RECORD = P.YSF_RECORD  # class, the metric of DCH-a, of DCH-b, 0
NEED_FICH, NEED_DCH = 120, 480  # the ``valid`` that covers the FICH, and any DCH
FI = {0: "header", 1: "communication", 2: "terminator", 3: "test"}
CM = {0: "group", 3: "individual"}
DT = {0: "V/D1", 1: "data FR", 2: "V/D2", 3: "voice FR"}
FIELDS = ("src", "dst", "downlink", "uplink", "rem12", "rem34")
#: the ten-byte fields that a good block brings, by FN: the two halves of a V/D mode 1 block, the one field of a V/D mode 2 block
VD1_FIELDS = {0: ("dst", "src"), 1: ("downlink", "uplink"), 2: ("rem12", "rem34")}
VD2_FIELDS = {0: "dst", 1: "src", 2: "downlink", 3: "uplink", 4: "rem12", 5: "rem34"}


# ---- the checks and the fields (host, integers) ---------------------------------------------------------------------------------


def pn9(count: int) -> bytes:
    """``count`` bytes of the whitening stream."""
    bits = list(PN9_FIRST)
    while len(bits) < 8 * count:
        bits.append(bits[-5] ^ bits[-9])
    return bytes(sum(b << (7 - k) for k, b in enumerate(bits[8 * j : 8 * j + 8])) for j in range(count))


_PN9 = pn9(20)
info_bytes, crc_ccitt = L.info_bytes, L.crc_ccitt  # the bytes of information words; CRC_POLY from 0


def dewhiten(data) -> bytes:
    """The data bytes of a block (at most 20, without the CRC) less the whitening."""
    return bytes(int(b) ^ w for b, w in zip(data, _PN9))


def crc16(data) -> int:
    """The CRC of the FICH and of every DCH: CRC-CCITT from 0, complemented."""
    return crc_ccitt(data) ^ 0xFFFF


def check_fich(words) -> bool:
    """Whether the CRC of the four FICH bytes equals the two behind them (``words``: the two of ``iqa_ysf_fich``)."""
    by = info_bytes(words)
    return crc16(by[:4]) == (by[4] << 8 | by[5])


def fich_fields(words) -> dict:
    """The named fields of the four FICH bytes."""
    b = info_bytes(words)
    return dict(fi=b[0] >> 6, cs=b[0] >> 4 & 3, cm=b[0] >> 2 & 3, bn=b[0] & 3, bt=b[1] >> 6, fn=b[1] >> 3 & 7, ft=b[1] & 7, dev=b[2] >> 6 & 1,
                mr=b[2] >> 3 & 7, voip=b[2] >> 2 & 1, dt=b[2] & 3, sql=b[3] >> 7, sq=b[3] & 0x7F)


def frame_class(fi: int, dt: int) -> int:
    """The class of a frame's data channels: 1 two blocks of 20 bytes (header, terminator, data FR), 2 one (V/D mode 1), 3 one of
    10 bytes (V/D mode 2), 0 nothing is read (voice FR, test)."""
    if fi in (0, 2) or (fi == 1 and dt == 1):
        return 1
    if fi == 1 and dt in (0, 2):
        return 2 if dt == 0 else 3
    return 0


def check_dch(words, size: int) -> bool:
    """Whether the CRC of the ``size`` (20 or 10) bytes as sent equals the two behind them (``words``: a block's six)."""
    by = info_bytes(words)
    return crc16(by[:size]) == (by[size] << 8 | by[size + 1])


def callsign(ten):
    """The text of a ten-byte field less its padding, or None where a byte is not printable ASCII."""
    if any(b < 0x20 or b > 0x7E for b in ten):
        return None
    return bytes(ten).decode("ascii").strip()


def block_fields(cls: int, fi: int, fn: int, second: bool) -> tuple:
    """The names of the ten-byte fields of a good block, in the order of its bytes; empty where the bytes are kept as hex."""
    if cls == 1:
        return (("downlink", "uplink") if second else ("dst", "src")) if fi in (0, 2) or fn == 0 else ()
    if cls == 2:
        return VD1_FIELDS.get(fn, ())
    if cls == 3:
        return (VD2_FIELDS[fn],) if fn in VD2_FIELDS else ()
    return ()


# ---- the device calls ---------------------------------------------------------------------------------------------------------


def slice_frames(plane, rows, plan: P.YsfPlan) -> tuple:
    """``iqa_ysf_slice`` on a device int32 plane for ``rows`` (int64[K][2]: m, s): (bits uint32[K][30], levels int64[K][3]: A, Dc,
    valid) on the host.  ``ValueError`` for a sign other than +-1, before anything is launched."""
    return L.slice_frames("iqa_ysf_slice", plane, rows, plan.offsets, P.YSF_WORDS)


def decode_fich(bits) -> tuple:
    """``iqa_ysf_fich`` on ``bits`` (uint32[K][30], host): (fich uint32[K][2], rec int32[K][5]) on the host."""
    bits = L.word_rows(bits, P.YSF_WORDS)
    k = bits.shape[0]
    return tuple(L.device_rows("iqa_ysf_fich", k, k == 0, bits.view(np.int32), c_int64(k), L.Out(2, np.uint32), L.Out(FICH_RECORD, np.int32)))


def decode_frames(bits, classes) -> tuple:
    """``iqa_ysf_decode`` on ``bits`` (uint32[K][30], host) of the ``classes`` (K values 0 .. 3): (info uint32[K][12], rec
    int32[K][4]) on the host.  ``ValueError`` for a class over 3, before anything is launched."""
    bits = L.word_rows(bits, P.YSF_WORDS)
    classes = L.frame_classes("iqa_ysf_decode", bits, classes, "class", 3, "0 .. 3")
    k = bits.shape[0]
    return tuple(L.device_rows("iqa_ysf_decode", k, k == 0, bits.view(np.int32), classes.astype(np.uint8), c_int64(k),
                               L.Out(P.YSF_INFO, np.uint32), L.Out(RECORD, np.int32)))


# ---- the frames ---------------------------------------------------------------------------------------------------------------


def frame_hits(hits, pats, half: int) -> np.ndarray:
    """int64[K][2], (m, s) in order of m: of the kept hits (int64[K][6] of section 25, ``pats`` the patterns searched for) every
    hit of the ``ysf`` pattern, less those with another within +-``half`` that has a larger |C|, or the same |C| at a smaller
    m (section 29's keep rule)."""
    return L.sync_hits(hits, pats, "ysf", half)


def apply_flags(rec, levels) -> np.ndarray:
    """``rec`` of ``iqa_ysf_fich`` with the cuts of ``iqa_ysf_slice`` written in: a status of 3 for a frame whose ``valid`` does not
    cover the FICH (120 symbols).  A frame that covers its FICH and not its 480 symbols is cut behind it: ``decoder_classes``
    gives it class 0 and ``parse_frames`` counts it."""
    rec = np.array(rec, dtype=np.int32).reshape(-1, FICH_RECORD)
    rec[np.asarray(levels, dtype=np.int64).reshape(-1, 3)[:, 2] < NEED_FICH, 0] = 3
    return rec


def decoder_classes(fich, rec, levels) -> np.ndarray:
    """The class that picks a frame's decoder: ``frame_class`` of its FICH where that was read, has a level and holds its check
    and the frame is whole, else 0 (nothing is read)."""
    out = []
    for words, r, lev in zip(np.asarray(fich).tolist(), np.asarray(rec).tolist(), np.asarray(levels).tolist()):
        f = fich_fields(words)
        out.append(frame_class(f["fi"], f["dt"]) if r[0] != 3 and lev[0] > 0 and lev[2] >= NEED_DCH and check_fich(words) else 0)
    return np.array(out, dtype=np.uint8)


@dataclass
class YsfFrame(L.JsonRecord):
    time_s: float  # where sync symbol 0 ends, in seconds of the stream
    fi: int
    cs: int
    cm: int
    bn: int
    bt: int
    fn: int
    ft: int
    dev: int
    mr: int
    voip: int
    dt: int
    sql: int
    sq: int
    cls: int  # ``frame_class``
    corrected: bool  # the FICH or a good block behind it was corrected
    blocks: list = field(default_factory=list)  # the blocks that were read: [the data bytes less the whitening as hex, the CRC held]
    fields: dict = field(default_factory=dict)  # the ten-byte fields of the good blocks by name: text, or None (not printable)

    def line(self) -> str:
        text = " ".join(f"{k}={v}" for k, v in self.fields.items() if v is not None)
        return f"YSF {FI[self.fi]} {DT[self.dt]} fn={self.fn}/{self.ft} {text}".rstrip()


def new_counts() -> dict:
    return dict(no_level=0, cut=0, fich_failed=0, golay_refused=0, dch_failed=0, fixed=0)


def parse_frames(rows, levels, fich, frec, info, rec, fs_ch: float, keyed_from: int = 0) -> tuple:
    """(frames, counts): every frame whose FICH held its check as a ``YsfFrame``, in order of time; ``rows`` int64[K][2] (m, s),
    ``levels`` int64[K][3], ``fich`` uint32[K][2], ``frec`` int32[K][5] (``apply_flags``' form), ``info`` uint32[K][12] and ``rec``
    int32[K][4].  A frame cut in front of the end of its FICH, one with A <= 0 and one whose FICH fails are counted and left
    out; a frame cut in front of the end of its data channels is counted and kept without them.  ``fixed`` counts the frames
    that are kept and were corrected."""
    counts = new_counts()
    out = []
    for (m, _s), (amp, _dc, valid), words, fr, iw, r in zip(np.asarray(rows).tolist(), np.asarray(levels).tolist(), np.asarray(fich).tolist(),
                                                           np.asarray(frec).tolist(), np.asarray(info).tolist(), np.asarray(rec).tolist()):
        if fr[0] == 3:
            counts["cut"] += 1
            continue
        if amp <= 0:
            counts["no_level"] += 1
            continue
        counts["golay_refused"] += fr[3]
        if not check_fich(words):
            counts["fich_failed"] += 1
            continue
        fields = fich_fields(words)
        f = YsfFrame(time_s=(int(keyed_from) + m) / fs_ch, cls=frame_class(fields["fi"], fields["dt"]), corrected=fr[0] == 1, **fields)
        if f.cls and valid < NEED_DCH:
            counts["cut"] += 1
        elif f.cls:
            size = 10 if f.cls == 3 else 20
            for second in ((0, 1) if f.cls == 1 else (0,)):
                block = iw[6 * second : 6 * second + 6]
                ok = check_dch(block, size)
                data = dewhiten(info_bytes(block)[:size])
                f.blocks.append([data.hex(), ok])
                if not ok:
                    counts["dch_failed"] += 1
                    continue
                f.corrected = f.corrected or r[1 + second] > 0
                for k, name in enumerate(block_fields(f.cls, f.fi, f.fn, bool(second))):
                    f.fields[name] = callsign(data[10 * k : 10 * k + 10])
        counts["fixed"] += f.corrected
        out.append(f)
    out.sort(key=lambda f: f.time_s)
    return out, counts


@dataclass
class YsfTransmission(L.JsonRecord):
    start_s: float
    end_s: float
    frames: int
    src: str | None
    dst: str | None
    downlink: str | None
    uplink: str | None
    rem12: str | None
    rem34: str | None
    cm: int  # of the first frame
    dt: int  # of the first frame
    sq: int | None  # the squelch code of the first frame; None: off
    late: bool  # the first frame seen was no header
    terminated: bool
    conflicts: int  # good blocks that named a field otherwise than the first that named it

    def line(self) -> str:
        parts = ["YSF"]
        if self.src:
            parts.append(self.src)
        if self.dst:
            parts += ["->", "ALL" if set(self.dst) == {"*"} else self.dst]
        if self.downlink or self.uplink:
            parts += ["via", (self.downlink or "") + ("/" + self.uplink if self.uplink else "")]
        if self.cm in CM:
            parts.append(CM[self.cm])
        parts += [DT[self.dt], "sq=off" if self.sq is None else f"sq={self.sq}"]
        parts.append(f"{self.end_s - self.start_s:.2f} s ({self.frames} frame{'' if self.frames == 1 else 's'})")
        return " ".join(parts)


def track_transmissions(frames) -> list:
    """The transmissions of the ``frames`` (``parse_frames``' list, in order of time), in order of their start: the first frame
    opens one where none is open (``late`` unless it is a header) and gives it its call mode, data type and squelch code; every
    good block fills the fields it names that are still unknown, and one that names a known field otherwise counts a conflict
    and changes nothing; a terminator closes it as terminated; no frame for more than ``HANG_S`` closes it at its last frame."""
    out, tx, last = [], None, 0.0
    for f in frames:
        if tx is not None and f.time_s - last > HANG_S:
            tx = None  # (its end is its last frame's time already)
        last = f.time_s
        if tx is None:
            tx = YsfTransmission(f.time_s, f.time_s, 0, None, None, None, None, None, None, f.cm, f.dt, f.sq if f.sql else None, f.fi != 0, False, 0)
            out.append(tx)
        tx.frames += 1
        tx.end_s = f.time_s
        for name, value in f.fields.items():
            if value is None:
                continue
            if getattr(tx, name) is None:
                setattr(tx, name, value)
            elif getattr(tx, name) != value:
                tx.conflicts += 1
        if f.fi == 2:
            tx.terminated = True
            tx = None
    return out


# ---- the results --------------------------------------------------------------------------------------------------------------


@dataclass
class YsfChannel(L.JsonRecord, L.ChannelLabel):
    offset_hz: float  # the finder's
    freq_hz: float | None
    frames: dict = field(default_factory=dict)  # frames per kind ("header", "V/D2", ..., "terminator")
    no_level: int = 0  # frames dropped for A <= 0
    cut: int = 0  # frames cut by the end of the stream
    fich_failed: int = 0
    golay_refused: int = 0  # words
    dch_failed: int = 0  # blocks
    fixed: int = 0  # kept frames in which something was corrected
    inverted: bool = False  # most of its sync hits were negative: the spectrum is inverted
    transmissions: list = field(default_factory=list)  # YsfTransmission, in order of their start
    note: str = ""  # why nothing was decoded
    NESTED = {"transmissions": YsfTransmission}

    def lines(self) -> list:
        """One line per transmission, in order of time."""
        return [f"{self.label()}: {t.line()}" for t in self.transmissions]


@dataclass
class YsfResult(L.JsonRecord, L.ChannelLines):
    channels: list = field(default_factory=list)  # YsfChannel, in the order of the FindResult's channels
    sample_rate: float = 0.0
    center_freq: float | None = None
    NESTED = {"channels": YsfChannel}

    @property
    def transmissions(self) -> list:
        return [t for ch in self.channels for t in ch.transmissions]


# ---- one stream ---------------------------------------------------------------------------------------------------------------


def decode_stream(theta, plan: P.YsfPlan, centre: int, hits, pats, v=None) -> dict:
    """Everything behind the frame sync words of one stored stream (device float32 ``theta``; ``hits`` section 25's kept hits of it
    for the patterns ``pats``): ``rows`` (int64[K][2]: m, s), ``bits`` (uint32[K][30]) and ``levels`` (int64[K][3]) of
    ``iqa_ysf_slice``, ``fich`` (uint32[K][2]) and ``frec`` (int32[K][5], the cuts written in) of ``iqa_ysf_fich``, ``classes``
    (uint8[K]), ``info`` (uint32[K][12]) and ``rec`` (int32[K][4]) of ``iqa_ysf_decode``, and the plane."""
    rows = frame_hits(hits, pats, plan.ident.half)
    if v is None:
        v = I.integrate(theta, plan.ident, centre)
    bits, levels = slice_frames(v, rows, plan)
    fich, frec = decode_fich(bits)
    frec = apply_flags(frec, levels)
    classes = decoder_classes(fich, frec, levels)
    info, rec = decode_frames(bits, classes)
    return dict(rows=rows, bits=bits, levels=levels, fich=fich, frec=frec, classes=classes, info=info, rec=rec, v=v)


def frame_kind(f: YsfFrame) -> str:
    return DT[f.dt] if f.fi == 1 else FI[f.fi]


def channel_of(st: dict, fs_ch: float, keyed_from: int, offset_hz: float, freq_hz) -> "YsfChannel":
    """The ``YsfChannel`` of ``decode_stream``'s output."""
    frames, counts = parse_frames(st["rows"], st["levels"], st["fich"], st["frec"], st["info"], st["rec"], fs_ch, keyed_from)
    out = YsfChannel(offset_hz=offset_hz, freq_hz=freq_hz, **counts)
    for f in frames:
        out.frames[frame_kind(f)] = out.frames.get(frame_kind(f), 0) + 1
    out.inverted = L.mostly_inverted(st["rows"])
    out.transmissions = track_transmissions(frames)
    return out


# ---- the layer of the second pass (describe.py) ---------------------------------------------------------------------------------

#: ``finish_ysf`` reads the 4800 family's plane; ``stages()`` shows ``ysf_rows`` ((m, s) per frame, None where the channel is no YSF
#: channel) and, with ``keep_stages``, ``ysf_plan`` and these
LAYER = L.ProtocolLayer("ysf", (4800,), lambda fs_ch, rate: P.plan_ysf(fs_ch), "ysf", decode_stream, channel_of, YsfChannel, YsfResult,
                        keys=("bits", "levels", "fich", "frec", "classes", "info", "rec"))
PLANE_RATES, finish_ysf, ysf_result, stage_keys = LAYER.rates, LAYER.finish, LAYER.result_of, LAYER.stage_keys


class YsfDecoder(L.StoredTheta):
    """A YSF decoder for one discriminator stream from Python (``protocol_layer.StoredTheta``): ``finish()`` gives a
    ``YsfResult`` of one channel, ``stages()`` ``decode_stream``'s output with the plane on the host, and ``hits``."""

    plan_of = staticmethod(P.plan_ysf)
    patterns, layer = YSF_PATTERNS, LAYER
