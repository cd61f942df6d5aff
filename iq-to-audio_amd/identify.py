"""Which protocol a keyed channel carries (``--find-identify``): from the stored discriminator stream of
a channel that section 23 labels ``fsk 1600 | 2400 | 3200 | 4800`` to the name of its protocol, by its frame synchronisation
words: DMR (base or mobile, voice or data), P25 phase 1, YSF, NXDN at 4800 or 2400 symbols/s, and FLEX with its mode.

``iqa_ident_integrate`` sums the quantised discriminator over one symbol, ``iqa_ident_search`` correlates every sync pattern
of the channel's family at every sample and lists the local maxima that reach a normalised correlation of sqrt(13 / 16);
fixed integer rules on the host turn the hits into a name.  The words and grids below are written from memory of the
published standards, not checked against them here.  Nothing is decoded: no colour code, NAC, talkgroup or page.  No CPU path:
without a GPU or the built library the device calls raise ``RuntimeError``."""
from __future__ import annotations

from ctypes import c_int8, c_int32, c_int64
from dataclasses import dataclass, field

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P
from .decoders.common import search_with_room
from .protocol_layer import JsonRecord, checked_theta, join_theta


@dataclass(frozen=True)
class SyncPattern:
    protocol: str
    positive: str  # the name of a hit with C > 0
    negative: str  # ... with C < 0
    word: int
    symbols: int  # N
    grid: int  # G: symbols between two sync words are a multiple of it
    families: tuple  # the symbol rates it is looked for at
    binary: bool = False  # one bit to a symbol (1 -> +1, 0 -> -1) instead of one dibit


# table order decides ties
PATTERNS = (
    SyncPattern("dmr", "dmr bs voice", "dmr bs data", 0x755FD7DF75F7, 24, 144, (4800,)),
    SyncPattern("dmr", "dmr ms voice", "dmr ms data", 0x7F7D5DD57DFD, 24, 144, (4800,)),
    SyncPattern("p25", "p25", "p25 inverted", 0x5575F5FF77FF, 24, 36, (4800,)),
    SyncPattern("ysf", "ysf", "ysf inverted", 0xD471C9634D, 20, 480, (4800,)),
    SyncPattern("nxdn", "nxdn", "nxdn inverted", 0xCDF59, 10, 192, (4800, 2400)),
    SyncPattern("flex", "flex", "flex inverted", 0xA6C6AAAA, 32, 3000, (1600,), True),
)
PROTOCOLS = ("dmr", "p25", "ysf", "nxdn", "flex")
DIBIT = {0b01: 3, 0b00: 1, 0b10: -1, 0b11: -3}
FAMILY_OF_BAUD = {1600: 1600, 3200: 1600, 2400: 2400, 4800: 4800}  # FLEX sends its first sync word at 1600 bit/s in every mode
FLEX_MODES = ((0x870C, "1600/2"), (0xB068, "1600/4"), (0x7B18, "3200/2"), (0xDEA0, "3200/4"))

# the rules' constants (design constants, as section 23's are)
SEEN_MIN_SYMBOLS = 20  # a single hit counts as "seen" only for a pattern this long
FLEX_MAX_DISTANCE = 3
CAPACITY = 4096  # the hit list's first size; a longer list repeats the search with room for all


def symbols_of(pat: SyncPattern) -> tuple:
    """The symbols of a pattern, first sent first: dibits 01 -> +3, 00 -> +1, 10 -> -1, 11 -> -3, or bits 1 -> +1, 0 -> -1."""
    if pat.binary:
        return tuple(1 if (pat.word >> (pat.symbols - 1 - i)) & 1 else -1 for i in range(pat.symbols))
    return tuple(DIBIT[(pat.word >> (2 * (pat.symbols - 1 - i))) & 3] for i in range(pat.symbols))


def patterns_for(rate: int) -> tuple:
    """The patterns of the family of ``rate`` symbols/s, in table order."""
    return tuple(p for p in PATTERNS if rate in p.families)


# ---- the device calls ---------------------------------------------------------------------------------------------------------


def integrate(theta, plan: P.IdentPlan, centre: int):
    """``iqa_ident_integrate`` over a stored discriminator stream (device float32): the device int32 ``v``."""
    n = int(theta.numel())
    v = D.empty(n, "int32")
    N.call("iqa_ident_integrate", N.ptr(theta), c_int64(n), c_int32(plan.window), c_int32(plan.shift), c_int32(int(centre)), N.ptr(v),
           N.stream_ptr())
    return v


def search(v, plan: P.IdentPlan, pats, capacity: int = CAPACITY):
    """``iqa_ident_search`` over ``v`` for the patterns ``pats``: (the device score planes int32[len(pats)][n], the kept hits as
    int64[K][6] on the host, sorted by (pattern, m)).  A list too short for the kept hits is never used: the search is repeated
    with room for all of them."""
    n = int(v.numel())
    npat = len(pats)
    if n == 0:
        return D.empty(0, "int32").reshape(npat, 0), sort_hits(np.zeros((0, P.IDENT_RECORD), dtype=np.int64))
    table = np.zeros((npat, P.IDENT_MAX_SYMBOLS), dtype=np.int8)
    for j, pat in enumerate(pats):
        table[j, : pat.symbols] = symbols_of(pat)
    offsets = (c_int32 * P.IDENT_OFFSETS)(*plan.offsets)
    symbols = (c_int8 * table.size)(*table.reshape(-1).tolist())
    nsym = (c_int32 * npat)(*[pat.symbols for pat in pats])
    score = D.empty(npat * n, "int32")
    counts = D.zeros(1, "int64")

    def run(room: int):
        lst = D.empty(P.IDENT_RECORD * room, "int64")
        N.call("iqa_ident_search", N.ptr(v), c_int64(n), offsets, c_int32(npat), symbols, nsym, c_int32(plan.half), N.ptr(score),
               N.ptr(lst), c_int64(room), N.ptr(counts), N.stream_ptr())
        return lst

    (lst,), (kept,) = search_with_room([run], counts, max(int(capacity), 1))
    hits = lst[: P.IDENT_RECORD * kept].cpu().numpy().reshape(-1, P.IDENT_RECORD)
    return score.reshape(npat, n), sort_hits(hits)


def sort_hits(hits) -> np.ndarray:
    """int64[K][6] sorted by (pattern, m)."""
    hits = np.asarray(hits, dtype=np.int64).reshape(-1, P.IDENT_RECORD)
    return hits[np.lexsort((hits[:, 1], hits[:, 0]))]


# ---- the rules (host, integers) -------------------------------------------------------------------------------------------------


def _popcount(x: int) -> int:
    return bin(x & 0xFFFF).count("1")


def _in_order(bits: int) -> int:
    """The sixteen bits of ``pre`` / ``post`` (bit k the k-th in time) read as a word sent MSB first, as the sync words are."""
    return int(f"{bits & 0xFFFF:016b}"[::-1], 2)


def flex_words(pre: int, post: int, inverted: bool) -> tuple:
    """(A, B) of a FLEX hit: the sixteen bits in front of the marker and the sixteen behind it, negated for an inverted hit."""
    a, b = _in_order(pre), _in_order(post)
    return ((~a) & 0xFFFF, (~b) & 0xFFFF) if inverted else (a, b)


def flex_counts(a: int, b: int) -> bool:
    """A FLEX hit counts only where the word behind the marker is the negation of the one in front of it, three bits apart at
    the most."""
    return _popcount(a ^ (~b & 0xFFFF)) <= FLEX_MAX_DISTANCE


def flex_mode(a: int, b: int) -> str:
    """The mode whose code lies within three bits of A and ~B together; ``?`` where none does.  (The codes lie more than three
    bits from one another, so no two entries fit one hit.)"""
    for code, name in FLEX_MODES:
        if _popcount(a ^ code) + _popcount((~b & 0xFFFF) ^ code) <= FLEX_MAX_DISTANCE:
            return name
    return "?"


def on_grid(distance: int, grid: int, plan: P.IdentPlan) -> bool:
    """Whether two hits ``distance`` samples apart lie k grid steps apart for an integer k >= 1, within +-h."""
    step = grid * plan.sps
    k = max(1, int(np.rint(distance / step)))
    return any(abs(distance - int(np.rint(j * step))) <= plan.half for j in (k - 1, k, k + 1) if j >= 1)


def decide(hits, pats, plan: P.IdentPlan) -> dict:
    """The rules of section 25 on the kept hits (rows of pattern, m, C, E, pre, post; ``pats`` the patterns searched for):
    ``hits`` per name, ``pairs`` per protocol (a hit and the nearest earlier hit of the same pattern, of either sign, on the
    pattern's grid), the ``protocol`` with the most pairs (ties to table order) as ``confirmed``, else the protocol with the most
    hits of a pattern of twenty symbols or more, else None; ``mode`` for FLEX; ``first_m``, the first hit of that protocol."""
    rows = [tuple(int(x) for x in r) for r in np.asarray(hits, dtype=np.int64).reshape(-1, P.IDENT_RECORD).tolist()]
    rows.sort(key=lambda r: (r[0], r[1]))
    names: dict = {}
    pairs: dict = {}
    total: dict = {}  # hits per protocol
    seen: dict = {}  # ... of the patterns long enough to be seen
    first: dict = {}
    modes: dict = {}
    last_m: dict = {}
    for p, m, c, _e, pre, post in rows:
        pat = pats[p]
        if pat.protocol == "flex":
            a, b = flex_words(pre, post, c < 0)
            if not flex_counts(a, b):
                continue
            mode = flex_mode(a, b)
            modes[mode] = modes.get(mode, 0) + 1
        name = pat.positive if c > 0 else pat.negative
        names[name] = names.get(name, 0) + 1
        total[pat.protocol] = total.get(pat.protocol, 0) + 1
        if pat.symbols >= SEEN_MIN_SYMBOLS:
            seen[pat.protocol] = seen.get(pat.protocol, 0) + 1
        first[pat.protocol] = min(first.get(pat.protocol, m), m)
        if p in last_m and on_grid(m - last_m[p], pat.grid, plan):
            pairs[pat.protocol] = pairs.get(pat.protocol, 0) + 1
        last_m[p] = m
    order = [proto for proto in PROTOCOLS if any(pat.protocol == proto for pat in pats)]
    protocol, confirmed = None, False
    best = max((pairs.get(proto, 0) for proto in order), default=0)
    if best >= 1:
        protocol, confirmed = next(proto for proto in order if pairs.get(proto, 0) == best), True
    else:
        best = max((seen.get(proto, 0) for proto in order), default=0)
        if best >= 1:
            protocol = next(proto for proto in order if seen.get(proto, 0) == best)
    mode = None
    if protocol == "flex":
        known = {k: n for k, n in modes.items() if k != "?"}
        mode = max((name for _, name in FLEX_MODES if name in known), key=lambda name: known[name], default="?")
    return dict(hits=names, pairs=pairs, protocol=protocol, confirmed=confirmed, mode=mode,
                first_m=None if protocol is None else first[protocol], count=0 if protocol is None else total[protocol])


# ---- the results --------------------------------------------------------------------------------------------------------------


@dataclass
class ChannelProtocol(JsonRecord):
    offset_hz: float  # the finder's
    freq_hz: float | None
    baud: int | None  # section 23's keyed rate; None where the channel is not keyed
    family: int | None  # R, the symbol rate searched at; None where the channel is not identified
    hits: dict  # kept sync words per name
    pairs: dict  # on-grid pairs per protocol
    protocol: str | None
    confirmed: bool
    mode: str | None  # FLEX only
    first_s: float | None  # the first sync word of the protocol, in seconds of the capture
    note: str  # why nothing was looked for or found

    def line(self) -> str:
        if self.family is None:
            return f"    protocol: not looked for ({self.note})"
        if self.protocol is None:
            return f"    protocol: none (fsk {self.baud}, {self.note})"
        mine = next(pat for pat in PATTERNS if pat.protocol == self.protocol)
        own = {pat.positive for pat in PATTERNS if pat.protocol == self.protocol} | {pat.negative for pat in PATTERNS if pat.protocol == self.protocol}
        counts = sorted(((n, name) for name, n in self.hits.items() if name in own), key=lambda e: (-e[0], e[1]))
        head = self.protocol + (f" {self.mode}" if self.mode else "") + ("" if self.confirmed else " unconfirmed")
        if self.protocol == "flex":
            frames = sum(n for n, _ in counts)
            return f"    protocol: {head} ({frames} frame{'' if frames == 1 else 's'})"
        short = ", ".join(f"{name[4:] if self.protocol == 'dmr' else name} {n}" for n, name in counts)
        if not self.confirmed:
            return f"    protocol: {head} ({short})"
        n = self.pairs.get(self.protocol, 0)
        return f"    protocol: {head} ({short}; {n} pair{'' if n == 1 else 's'} on the {1000.0 * mine.grid / self.family:g} ms grid)"


@dataclass
class ProtocolResult(JsonRecord):
    channels: list = field(default_factory=list)  # ChannelProtocol, in the order of the FindResult's channels
    sample_rate: float = 0.0
    center_freq: float | None = None
    NESTED = {"channels": ChannelProtocol}

    def lines(self) -> list:
        return [ch.line() for ch in self.channels]


def family_plan(keyed_label: str | None, baud, fs_ch: float) -> tuple:
    """(R, IdentPlan or None, note) of a channel: R is None where the channel is not one to identify (``note`` says what it
    is), the plan None where the rate does not fit."""
    if baud not in FAMILY_OF_BAUD:
        return None, None, keyed_label or "not keyed"
    rate = FAMILY_OF_BAUD[baud]
    try:
        return rate, P.plan_ident(fs_ch, rate), ""
    except ValueError:
        return rate, None, "rate does not fit"


def protocol_of(keyed, hits, plan: P.IdentPlan | None, rate, note: str, keyed_from) -> ChannelProtocol:
    """One channel's ``ChannelProtocol`` from its ``ChannelKeying``, its family and its kept hits (None: nothing searched)."""
    base = dict(offset_hz=keyed.offset_hz, freq_hz=keyed.freq_hz, baud=keyed.baud, family=rate)
    if rate is None:
        return ChannelProtocol(**base, hits={}, pairs={}, protocol=None, confirmed=False, mode=None, first_s=None,
                               note=note if keyed.label is not None else keyed.described)
    if plan is None or hits is None:
        return ChannelProtocol(**base, hits={}, pairs={}, protocol=None, confirmed=False, mode=None, first_s=None,
                               note=note or "not measured")
    d = decide(hits, patterns_for(rate), plan)
    first = None if d["first_m"] is None else (int(keyed_from or 0) + d["first_m"]) / plan.fs_ch
    return ChannelProtocol(**base, hits=d["hits"], pairs=d["pairs"], protocol=d["protocol"], confirmed=d["confirmed"], mode=d["mode"],
                           first_s=first, note="" if d["protocol"] is not None else "no sync word")


# ---- the layer of the second pass (describe.py) ---------------------------------------------------------------------------------


def _stored_theta(lane):
    """A lane's stored discriminator stream as one device tensor (``protocol_layer.join_theta``)."""
    return join_theta(lane.stored)


def finish_identify(lanes, keyed, keep: bool, plane_rates=()) -> list:
    """Per lane of the pass (``keyed``: its ``ChannelKeying``) a dict of its identification: ``rate`` (R, None where the channel is
    not one to identify), ``plan`` (the ``IdentPlan``, None where the rate does not fit), ``note``, ``hits`` (int64[K][6], the kept
    sync words sorted by (pattern, m), m counted from ``keyed_from``; None where nothing was searched), ``v`` (the integrated plane,
    a device tensor) with ``keep`` or where a layer behind this one reads the planes of R (``plane_rates``), and ``score`` with
    ``keep``.  The whole search runs here, on the stored stream as one piece."""
    out = []
    for lane, k in zip(lanes, keyed):
        rate, plan, note = family_plan(k.label, k.baud if k.label is not None else None, lane.plan.fs_ch)
        d = dict(rate=rate, plan=plan, note=note, hits=None)
        if plan is not None and lane.centre is not None and lane.stored:
            theta = checked_theta(lane.stored)
            v = integrate(theta, plan, lane.centre)
            score, d["hits"] = search(v, plan, patterns_for(rate))
            if keep or rate in plane_rates:
                d["v"] = v
            if keep:
                d["score"] = score
        out.append(d)
    return out


def protocols(lanes, keyed, found) -> list:
    """The ``ChannelProtocol`` of every lane from its ``ChannelKeying`` and its dict of ``finish_identify``."""
    return [protocol_of(k, d["hits"], d["plan"], d["rate"], d["note"], lane.keyed_from) for k, d, lane in zip(keyed, found, lanes)]


def stage_keys(describer, j: int, lane, keep: bool) -> dict:
    """This layer's keys of ``ChannelDescriber.stages()`` for channel ``j``: ``ident_rate``, ``ident_plan``, ``hits`` (int64[K][6] or
    None) and, with ``keep``, ``stored`` (float32, the stored theta: ``theta`` from ``keyed_from`` on) and, of the identified
    channels, ``v`` (int32[n]) and ``score`` (int32[patterns][n])."""
    i = describer.finish_identify()[j]
    d = dict(ident_rate=i["rate"], ident_plan=i["plan"], hits=i["hits"])
    if keep:
        d["stored"] = D.torch_mod().cat(lane.stored).cpu().numpy() if lane.stored else np.zeros(0, dtype=np.float32)
        if "v" in i:
            d.update(v=i["v"].cpu().numpy(), score=i["score"].cpu().numpy())
    return d
