"""The pages of a FLEX channel (``--find-flex``): from the stored discriminator stream of a channel and
the sync-1 hits that section 25 keeps (``identify.py``) to the text of its pages.

``iqa_flex_frames`` takes the levels of every frame from its marker and reads the frame information word;
``iqa_flex_words`` slices the eleven data blocks of every frame at 2 or 4 levels, splits the phases, undoes the block
interleave and checks every word as a BCH(31,21) codeword, at five timing shifts.  The host keeps the best shift of every block
(``choose_shifts``) and parses the words (``parse_frames``): integer logic on numpy arrays.  The constants are written from
memory of the FLEX air interface and of multimon-ng's reading of it, not checked against either here.  No CPU path: without
a GPU or the built library the device calls raise ``RuntimeError``.

What is FLEX's own lives here: the device calls, the shifts, the parser, the dataclasses, ``decode_stream`` and ``channel_of``.
What every protocol layer shares lives in ``protocol_layer.py``: the stored stream under ``FlexDecoder``, the per-lane loop
under ``finish_flex``, the builder under ``flex_result``, and ``label`` / ``lines`` / ``to_json`` / ``from_json`` of the results."""
from __future__ import annotations

from ctypes import c_int32, c_int64
from dataclasses import dataclass, field

import numpy as np

from . import _dev as D
from . import dsp_plan as P
from . import identify as I
from . import protocol_layer as L

MARKER = 0xA6C6AAAA
SYNC_B = 0x5939  # bits 48 .. 63 of the 1600 bit/s grid; not read
MODES = I.FLEX_MODES  # (code, name)
MODE_SHAPE = {"1600/2": (1, 2), "1600/4": (1, 4), "3200/2": (2, 2), "3200/4": (2, 4)}  # name -> (u, levels)
PHASES = "ABCD"
ACTIVE = {"1600/2": (0,), "1600/4": (0, 1), "3200/2": (0, 2), "3200/4": (0, 1, 2, 3)}
SHIFT_ORDER = (2, 1, 3, 0, 4)  # ties go to the smaller |d|, then to the negative one
BCH_POLY = 0x769
INFO_MASK = 0x1FFFFF
TYPES = ("secure", "instruction", "tone", "numeric", "special numeric", "alpha", "binary", "numbered numeric")
DIGITS = "0123456789 U -]["
REPLACEMENT = "\ufffd"
RECORD = 6  # int64 values of iqa_flex_frames per hit: sigma, A, raw FIW, fixed FIW, status, valid
WORD_SHAPE = (P.FLEX_SHIFTS, P.FLEX_PHASES, P.FLEX_WORDS)


# ---- words (host, integers) ---------------------------------------------------------------------------------------------------


def rev32(x: int) -> int:
    return int(f"{x & 0xFFFFFFFF:032b}"[::-1], 2)


def syndrome(cw: int) -> int:
    """Section 12's syndrome: the upper 31 bits of ``cw`` modulo g."""
    r = (cw & 0xFFFFFFFF) >> 1
    for i in range(30, 9, -1):
        if (r >> i) & 1:
            r ^= BCH_POLY << (i - 10)
    return r & 0x3FF


def is_codeword(w: int) -> bool:
    """Whether ``w`` (first sent bit as bit 0) is a codeword: rev32(w) has a zero syndrome and even parity."""
    return syndrome(rev32(w)) == 0 and bin(w & 0xFFFFFFFF).count("1") % 2 == 0


def check4(x: int) -> bool:
    """The five nibbles of bits 0 .. 19 plus bit 20, summed: the low four bits of the sum are all set."""
    return (sum((x >> (4 * i)) & 0xF for i in range(5)) + ((x >> 20) & 1)) & 0xF == 0xF


def is_long(a: int) -> bool:
    return a <= 0x8000 or 0x1E0000 < a <= 0x1F0000 or a > 0x1F7FFE


# ---- the device calls ---------------------------------------------------------------------------------------------------------


def frames(plane, hits, plan: P.FlexPlan) -> np.ndarray:
    """``iqa_flex_frames`` on a device int32 plane for ``hits`` (int64[K][2]: m, s): int64[K][6] on the host."""
    hits = np.ascontiguousarray(np.asarray(hits, dtype=np.int64).reshape(-1, 2))
    n, k = int(plane.numel()), hits.shape[0]
    (out,) = L.device_rows("iqa_flex_frames", k, n == 0 or k == 0, plane, c_int64(n), hits, c_int64(k),
                           (c_int32 * P.FLEX_HEADER_OFFSETS)(*plan.header), L.Out(RECORD, np.int64))
    if n == 0 or k == 0:
        out[:, 4] = 3  # (nothing was read: every instant lies outside)
    return out


def words(plane, recs, levels: int, u: int, plan: P.FlexPlan, offsets=None) -> tuple:
    """``iqa_flex_words`` on a device int32 plane for ``recs`` (int64[F][4]: m, s, sigma, A): (fixed uint32[F][5][4][88], raw
    uint32[...], status uint8[...]) on the host.  ``offsets``: the plan's data offsets of ``u`` on the device, where the caller
    holds them."""
    recs = np.ascontiguousarray(np.asarray(recs, dtype=np.int64).reshape(-1, 4))
    n, f = int(plane.numel()), recs.shape[0]
    step = plan.steps[u - 1] if u in (1, 2) else 0
    if offsets is None and u in (1, 2):
        offsets = plan.data[u - 1]  # (a host array: uploaded where anything is read)
    count = P.FLEX_SHIFTS * P.FLEX_PHASES * P.FLEX_WORDS
    fixed, raw, status = (a.reshape((f,) + WORD_SHAPE) for a in L.device_rows(
        "iqa_flex_words", f, n == 0 or f == 0, plane, c_int64(n), recs, c_int64(f), c_int32(levels), c_int32(u), c_int32(step), offsets,
        L.Out(count, np.uint32), L.Out(count, np.uint32), L.Out(count, np.uint8)))
    if n == 0 or f == 0:
        status[...] = 3  # (nothing was read: every instant lies outside)
    return fixed, raw, status


# ---- the shifts ---------------------------------------------------------------------------------------------------------------


def choose_shifts(status, phases) -> np.ndarray:
    """int64[F][11]: per frame and block the shift index e (d = (e - 2) step) with the fewest words of status >= 2 over the
    active ``phases``; ties go to the smaller |d|, then to the negative one."""
    status = np.asarray(status).reshape((-1,) + WORD_SHAPE)
    bad = (status[:, :, list(phases), :] >= 2).reshape(status.shape[0], P.FLEX_SHIFTS, len(phases), P.FLEX_BLOCKS, 8)
    count = bad.sum(axis=(2, 4))  # [F][5][11]
    out = np.zeros((status.shape[0], P.FLEX_BLOCKS), dtype=np.int64)
    best = np.full(out.shape, 1 << 30, dtype=np.int64)
    for e in SHIFT_ORDER:
        better = count[:, e, :] < best
        out[better] = e
        best[better] = count[:, e, :][better]
    return out


def take_shifts(arr, chosen) -> np.ndarray:
    """[F][4][88]: the words of ``arr`` ([F][5][4][88]) at the chosen shift of every block."""
    arr = np.asarray(arr).reshape((-1,) + WORD_SHAPE)
    f = arr.shape[0]
    e = np.repeat(np.asarray(chosen, dtype=np.int64).reshape(f, P.FLEX_BLOCKS), 8, axis=1)  # per word
    return np.take_along_axis(arr, e[:, None, None, :].repeat(P.FLEX_PHASES, axis=2), axis=1)[:, 0]


# ---- the pages ----------------------------------------------------------------------------------------------------------------


@dataclass
class FlexPage(L.JsonRecord):
    time_s: float  # the frame's marker, in seconds of the stream
    cycle: int
    frame: int
    phase: str
    mode: str
    inverted: bool
    capcode: int | None  # None for a long address
    long: bool
    kind: str | None  # the vector's type; None where a long address's vector cannot be read
    text: str | None
    words: list  # the page's words as hex: address, vector, message
    corrected: int  # words of status 1 among them
    damaged: bool  # a message word of status >= 2
    fragment: int | None  # alpha only
    more: bool | None  # alpha only

    def line(self) -> str:
        cap = "long" if self.capcode is None else str(self.capcode)
        head = f"FLEX {self.mode} {self.cycle:02d}.{self.frame:03d}.{self.phase} cap={cap} {self.kind or 'unknown'}"
        if self.text is not None:
            head += f' "{self.text}"'
        return head + (" (damaged)" if self.damaged else "")


def _chars(info: int) -> list:
    return [(info >> (7 * i)) & 0x7F for i in range(3)]


def _alpha(infos, stats) -> tuple:
    """(text, fragment, more, damaged) of an alpha message's words."""
    head_ok = stats[0] <= 1
    fragment = (infos[0] >> 11) & 3 if head_ok else None
    more = bool((infos[0] >> 10) & 1) if head_ok else None
    damaged = not head_ok
    out = []
    for j in range(1, len(infos)):
        if stats[j] >= 2:
            damaged = True
            out.append(REPLACEMENT * 3)
            continue
        chars = _chars(infos[j])
        if j == 1 and fragment == 3:
            chars = chars[1:]
        out.append("".join(chr(c) if 0x20 <= c <= 0x7E else REPLACEMENT for c in chars if c not in (0x00, 0x03)))
    return "".join(out), fragment, more, damaged


def _numeric(infos, skip: int) -> str:
    total = 0
    for j, x in enumerate(infos):
        total |= (x & INFO_MASK) << (21 * j)
    nbits = 21 * len(infos)
    out = []
    for at in range(skip, nbits - 3, 4):
        digit = (total >> at) & 0xF
        if digit != 0xC:
            out.append(DIGITS[digit])
    return "".join(out)


def parse_phase(fixed, status, counts: dict) -> list:
    """The pages of one phase of one frame (``fixed`` uint32[88], ``status`` uint8[88]) as dicts without the frame's fields,
    in order of the address index; ``counts`` is added to."""
    fixed = [int(x) for x in fixed]
    status = [int(x) for x in status]
    info = [w & INFO_MASK for w in fixed]
    if status[0] >= 2:
        counts["biw_lost"] += 1
        return []
    if info[0] in (0, INFO_MASK):
        return []  # an idle phase
    aoff, voff = ((info[0] >> 8) & 3) + 1, (info[0] >> 10) & 0x3F
    if not (aoff <= voff and 2 * voff - aoff <= P.FLEX_WORDS):
        counts["biw_bad"] += 1
        return []
    field_end = 2 * voff - aoff
    pages = []
    i = aoff
    while i < voff:
        at, vec = i, voff + i - aoff
        if status[at] >= 2:  # an address that cannot be read: taken as a short one
            counts["vectors_dropped"] += 1
            i += 1
            continue
        a = info[at]
        long = is_long(a) and at + 1 < voff
        if is_long(a) and not long:  # a long address cut by the end of the address field
            counts["vectors_dropped"] += 1
            i += 1
            continue
        i += 2 if long else 1
        v = info[vec]
        v_ok = status[vec] <= 1 and check4(v)
        used = [at, at + 1, vec] if long else [at, vec]
        if long:
            pages.append(dict(index=at, capcode=None, long=True, kind=TYPES[(v >> 4) & 7] if v_ok else None, text=None,
                              words=[f"{fixed[j]:08x}" for j in used], corrected=sum(status[j] == 1 for j in used), damaged=False,
                              fragment=None, more=None))
            continue
        if not v_ok:
            counts["vectors_dropped"] += 1
            continue
        kind = (v >> 4) & 7
        page = dict(index=at, capcode=a - 0x8000, long=False, kind=TYPES[kind], text=None, damaged=False, fragment=None, more=None)
        if kind in (0, 5, 6):
            start, count = (v >> 7) & 0x7F, (v >> 14) & 0x7F
            if not (start >= field_end and start + count <= P.FLEX_WORDS and count >= 1):
                counts["vectors_dropped"] += 1
                continue
            body = list(range(start, start + count))
            if kind == 5:
                page["text"], page["fragment"], page["more"], page["damaged"] = _alpha([info[j] for j in body], [status[j] for j in body])
            else:
                page["damaged"] = any(status[j] >= 2 for j in body)
        elif kind in (3, 4, 7):
            start, count = (v >> 7) & 0x7F, ((v >> 14) & 7) + 1
            if not (start >= field_end and start + count <= P.FLEX_WORDS):
                counts["vectors_dropped"] += 1
                continue
            body = list(range(start, start + count))
            page["text"] = _numeric([info[j] for j in body], 12 if kind == 7 else 2)
            page["damaged"] = any(status[j] >= 2 for j in body)
        else:
            body = []
        used += body
        page["words"] = [f"{fixed[j]:08x}" for j in used]
        page["corrected"] = sum(status[j] == 1 for j in used)
        pages.append(page)
    return pages


def new_counts() -> dict:
    return dict(fiw_failed=0, biw_lost=0, biw_bad=0, vectors_dropped=0)


def parse_frames(heads, fixed, status) -> tuple:
    """(pages, counts): ``heads`` one dict per frame (``time_s``, ``mode``, ``inverted``, ``fiw`` the fixed frame information
    word, ``fiw_status``), ``fixed`` uint32[F][4][88] and ``status`` uint8[F][4][88] the words at the chosen shifts.  A frame whose
    information word has a status over 1 or fails ``check4`` is counted and skipped.  Pages in order of time, phase, address."""
    counts = new_counts()
    pages = []
    order = sorted(range(len(heads)), key=lambda j: heads[j]["time_s"])
    for j in order:
        h = heads[j]
        x = int(h["fiw"]) & INFO_MASK
        if int(h["fiw_status"]) > 1 or not check4(x):
            counts["fiw_failed"] += 1
            continue
        cycle, frame = (x >> 4) & 0xF, (x >> 8) & 0x7F
        for ph in ACTIVE[h["mode"]]:
            for page in parse_phase(fixed[j][ph], status[j][ph], counts):
                page = dict(page)
                page.pop("index")
                pages.append(FlexPage(time_s=h["time_s"], cycle=cycle, frame=frame, phase=PHASES[ph], mode=h["mode"],
                                      inverted=bool(h["inverted"]), **page))
    return pages, counts


# ---- the results --------------------------------------------------------------------------------------------------------------


@dataclass
class FlexChannel(L.JsonRecord, L.ChannelLabel):
    offset_hz: float  # the finder's
    freq_hz: float | None
    frames: dict = field(default_factory=dict)  # frames per mode
    unknown_mode: int = 0  # sync words whose mode code is none of the four
    no_level: int = 0  # frames dropped for A <= 0
    fiw_failed: int = 0
    biw_lost: int = 0
    biw_bad: int = 0
    vectors_dropped: int = 0
    words: dict = field(default_factory=dict)  # words of the parsed frames' active phases per status ("0" .. "3")
    shifts: dict = field(default_factory=dict)  # blocks per chosen shift ("-2" .. "2", in steps)
    pages: list = field(default_factory=list)  # FlexPage, in order of time, phase, address
    note: str = ""  # why nothing was decoded
    NESTED = {"pages": FlexPage}

    def lines(self) -> list:
        return [f"{self.label()}: {page.line()}" for page in self.pages]


@dataclass
class FlexResult(L.JsonRecord, L.ChannelLines):
    channels: list = field(default_factory=list)  # FlexChannel, in the order of the FindResult's channels
    sample_rate: float = 0.0
    center_freq: float | None = None
    NESTED = {"channels": FlexChannel}

    @property
    def pages(self) -> list:
        return [page for ch in self.channels for page in ch.pages]


# ---- one stream ---------------------------------------------------------------------------------------------------------------


def frame_hits(hits, pats) -> tuple:
    """(rows, unknown): of the kept hits (int64[K][6] of section 25) every ``flex`` hit that counts and has a known mode as
    (m, s, mode), in order of m; the hits of mode ``?``."""
    rows, unknown = [], 0
    for p, m, c, _e, pre, post in np.asarray(hits, dtype=np.int64).reshape(-1, P.IDENT_RECORD).tolist():
        if pats[p].protocol != "flex":
            continue
        a, b = I.flex_words(pre, post, c < 0)
        if not I.flex_counts(a, b):
            continue
        mode = I.flex_mode(a, b)
        if mode == "?":
            unknown += 1
            continue
        rows.append((m, -1 if c < 0 else 1, mode))
    rows.sort()
    return rows, unknown


def decode_stream(theta, plan: P.FlexPlan, centre: int, hits, pats, v16=None) -> dict:
    """Everything behind the sync word of one stored stream (device float32 ``theta``; ``hits`` section 25's kept hits of it):
    the frames (``rows``: m, s, mode), ``rec16`` / ``rec32`` (``iqa_flex_frames`` on v16 for all of them, on v32 for the
    3200-rate ones, zeros elsewhere), ``ok`` (A > 0 on the frame's data plane), ``fixed`` / ``raw`` / ``status``
    ([F][5][4][88]; status 4 throughout for a frame that is not ok), ``chosen`` (int64[F][11]) and the planes."""
    rows, unknown = frame_hits(hits, pats)
    f = len(rows)
    if v16 is None:
        v16 = I.integrate(theta, plan.ident[0], centre)
    ms = np.array([(m, s) for m, s, _ in rows], dtype=np.int64).reshape(-1, 2)
    rec16 = frames(v16, ms, plan)
    fast = [j for j, (_, _, mode) in enumerate(rows) if MODE_SHAPE[mode][0] == 2]
    rec32 = np.zeros((f, RECORD), dtype=np.int64)
    v32 = None
    if fast:
        v32 = I.integrate(theta, plan.ident[1], centre)
        rec32[fast] = frames(v32, ms[fast], plan)
    level = np.array([rec32[j, :2] if j in set(fast) else rec16[j, :2] for j in range(f)], dtype=np.int64).reshape(-1, 2)
    ok = np.array([bool(rec16[j, 5]) and level[j, 1] > 0 for j in range(f)], dtype=bool)
    shape = (f,) + WORD_SHAPE
    fixed, raw, status = np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.uint32), np.full(shape, 4, dtype=np.uint8)
    chosen = np.full((f, P.FLEX_BLOCKS), 2, dtype=np.int64)
    offsets = {}
    for mode, (u, levels) in MODE_SHAPE.items():  # one call per (u, levels) group
        sel = [j for j in range(f) if ok[j] and rows[j][2] == mode]
        if not sel:
            continue
        if u not in offsets:
            offsets[u] = D.from_numpy(plan.data[u - 1])
        recs = np.concatenate([ms[sel], level[sel]], axis=1)
        fixed[sel], raw[sel], status[sel] = words(v16 if u == 1 else v32, recs, levels, u, plan, offsets[u])
        chosen[sel] = choose_shifts(status[sel], ACTIVE[mode])
    return dict(rows=rows, unknown_mode=unknown, rec16=rec16, rec32=rec32, ok=ok, fixed=fixed, raw=raw, status=status, chosen=chosen,
                v16=v16, v32=v32)


def channel_of(st: dict, fs_ch: float, keyed_from: int, offset_hz: float, freq_hz) -> "FlexChannel":
    """The ``FlexChannel`` of ``decode_stream``'s output."""
    rows, ok = st["rows"], st["ok"]
    out = FlexChannel(offset_hz=offset_hz, freq_hz=freq_hz, unknown_mode=st["unknown_mode"], no_level=int(np.count_nonzero(~ok)))
    for _, _, mode in rows:
        out.frames[mode] = out.frames.get(mode, 0) + 1
    sel = [j for j in range(len(rows)) if ok[j]]
    fixed, status = take_shifts(st["fixed"][sel], st["chosen"][sel]), take_shifts(st["status"][sel], st["chosen"][sel])
    heads = [dict(time_s=(int(keyed_from) + rows[j][0]) / fs_ch, mode=rows[j][2], inverted=rows[j][1] < 0, fiw=st["rec16"][j, 3],
                  fiw_status=st["rec16"][j, 4]) for j in sel]
    out.pages, counts = parse_frames(heads, fixed, status)
    out.fiw_failed, out.biw_lost, out.biw_bad, out.vectors_dropped = (counts[k] for k in ("fiw_failed", "biw_lost", "biw_bad", "vectors_dropped"))
    for k, j in enumerate(sel):
        for ph in ACTIVE[rows[j][2]]:
            for s in status[k][ph].tolist():
                out.words[str(s)] = out.words.get(str(s), 0) + 1
        for e in st["chosen"][j].tolist():
            out.shifts[str(e - 2)] = out.shifts.get(str(e - 2), 0) + 1
    return out


# ---- the layer of the second pass (describe.py) ---------------------------------------------------------------------------------


def _stage_keys(x: dict, keep: bool) -> dict:
    """The keys of ``ChannelDescriber.stages()`` from ``x``, ``finish_flex``'s dict of one channel: ``flex_frames`` ((m, s, mode) per
    decoded frame, None where the channel is no FLEX channel) and, with ``keep``, ``flex_words``, ``flex_raw``, ``flex_status``
    ([F][5][4][88]), ``flex_chosen``, ``flex_rec16``, ``flex_rec32``, ``flex_ok``, ``flex_v32`` and ``flex_plan``."""
    d = dict(flex_frames=x.get("rows"))
    if keep and "rows" in x:
        d.update(flex_plan=x["plan"], flex_rec16=x["rec16"], flex_rec32=x["rec32"], flex_ok=x["ok"], flex_words=x["fixed"],
                 flex_raw=x["raw"], flex_status=x["status"], flex_chosen=x["chosen"],
                 flex_v32=None if x["v32"] is None else x["v32"].cpu().numpy())
    return d


#: ``finish_flex`` reads the 1600 family's plane (``v``, its ``v16``)
LAYER = L.ProtocolLayer("flex", (1600,), lambda fs_ch, rate: P.plan_flex(fs_ch), "flex", decode_stream, channel_of, FlexChannel, FlexResult,
                        keys_of=_stage_keys)
PLANE_RATES, finish_flex, flex_result, stage_keys = LAYER.rates, LAYER.finish, LAYER.result_of, LAYER.stage_keys


class FlexDecoder(L.StoredTheta):
    """A FLEX decoder for one discriminator stream from Python (``protocol_layer.StoredTheta``): ``finish()`` gives a
    ``FlexResult`` of one channel, ``stages()`` ``decode_stream``'s output with the planes on the host, and ``hits``."""

    plan_of = staticmethod(P.plan_flex)
    planes = ("v16", "v32")

    def _decode(self, theta) -> tuple:
        pats = I.patterns_for(1600)
        v16 = I.integrate(theta, self.plan.ident[0], self.centre)
        _, hits = I.search(v16, self.plan.ident[0], pats)
        st = decode_stream(theta, self.plan, self.centre, hits, pats, v16)
        st["hits"] = hits
        return st, FlexResult(channels=[channel_of(st, self.plan.fs_ch, 0, 0.0, None)], sample_rate=self.plan.fs_ch)
