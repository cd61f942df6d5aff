"""Numpy oracle of the FLEX page decoding (--find-flex), written from the specification with its own
copy of every constant, and a FLEX encoder: pages -> words with BCH and parity -> interleave -> phases -> symbols -> sync 1,
frame information word and sync 2 -> a rectangular 2- or 4-level FSK theta at +-4800 / +-1600 Hz.  Of the package it uses
nothing; the integrator, the sync search and ``crafted_plane`` are ``ident_model``'s.  Everything behind the integrator is
integer, so the kernels are held to ``frame_records`` and ``words`` bit for bit.  The slicing comes twice: in plain loops
(``words_by_loops``, for single frames) and vectorised; the host test holds the two to each other."""
from __future__ import annotations

import functools
import importlib.util
import math
import sys
from pathlib import Path

import numpy as np


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


IM = _load("ident_model")

MARKER = 0xA6C6AAAA
SYNC_B = 0x5939
MODES = {"1600/2": 0x870C, "1600/4": 0xB068, "3200/2": 0x7B18, "3200/4": 0xDEA0}
SHAPE = {"1600/2": (1, 2), "1600/4": (1, 4), "3200/2": (2, 2), "3200/4": (2, 4)}  # (u, levels)
ACTIVE = {"1600/2": "A", "1600/4": "AB", "3200/2": "AC", "3200/4": "ABCD"}
PHASES = "ABCD"
G = 0x769
MASK = 0x1FFFFF
TYPES = ("secure", "instruction", "tone", "numeric", "special numeric", "alpha", "binary", "numbered numeric")
DIGITS = "0123456789 U -]["
SHIFT_ORDER = (0, -1, 1, -2, 2)
BLOCKS, WORDS, SYMBOLS, DATA_BIT = 11, 88, 2816, 135
FLEX_PATTERN = [p for p in IM.PATTERNS if p[0] == "flex"]


# ---- words -------------------------------------------------------------------------------------------------------------------


def rev(x: int, bits: int) -> int:
    return sum(((x >> i) & 1) << (bits - 1 - i) for i in range(bits))


def remainder(v31: int) -> int:
    r = v31
    for i in range(30, 9, -1):
        if (r >> i) & 1:
            r ^= G << (i - 10)
    return r & 0x3FF


def codeword(info: int) -> int:
    """The 32-bit word of 21 information bits, the first sent bit (bit 0 of ``info``) as bit 0."""
    data = rev(info & MASK, 21)
    v = (data << 10) | remainder(data << 10)
    return rev((v << 1) | (bin(v).count("1") & 1), 32)


SINGLE = {remainder((1 << pos) >> 1): pos for pos in range(1, 32)}


def correct(raw: int) -> tuple:
    """(fixed, status) of a word as sliced: 0 clean, 1 one bit restored, 2 refused."""
    c = rev(raw, 32)
    s, odd = remainder(c >> 1), bin(c).count("1") & 1
    if s == 0:
        return (rev(c ^ 1, 32), 1) if odd else (raw, 0)
    if odd and s in SINGLE:
        return rev(c ^ (1 << SINGLE[s]), 32), 1
    return raw, 2


def check4(x: int) -> bool:
    return (sum((x >> (4 * i)) & 0xF for i in range(5)) + ((x >> 20) & 1)) & 0xF == 0xF


def with_check4(x: int) -> int:
    """``x`` with its low nibble set so that ``check4`` holds."""
    x &= ~0xF
    rest = sum((x >> (4 * i)) & 0xF for i in range(1, 5)) + ((x >> 20) & 1)
    return x | ((0xF - rest) & 0xF)


def is_long(a: int) -> bool:
    return a <= 0x8000 or 0x1E0000 < a <= 0x1F0000 or a > 0x1F7FFE


# ---- the plan ----------------------------------------------------------------------------------------------------------------


def plan(fs_ch: float) -> dict:
    sps = float(fs_ch) / 1600.0
    if not 8.0 <= sps <= 224.0:
        raise ValueError("rate does not fit")
    return dict(fs_ch=float(fs_ch), sps=sps, o16={i: int(round(i * sps)) for i in range(-16, 96)},
                data={u: [int(round((DATA_BIT + (q + 1) / u) * sps)) for q in range(SYMBOLS * u)] for u in (1, 2)},
                step={u: max(1, int(sps / (8 * u))) for u in (1, 2)}, ident={1: IM.plan(fs_ch, 1600), 2: IM.plan(fs_ch, 3200)})


# ---- the frames --------------------------------------------------------------------------------------------------------------


def frame_hits(hits) -> tuple:
    """((m, s, mode) in order of m, hits of unknown mode) of the kept hits of ``ident_model.keep``."""
    rows, unknown = [], 0
    for _p, m, C, _E, pre, post in hits:
        mode = IM.flex_mode(*IM.flex_words(pre, post, C < 0))
        if mode is None:
            continue
        if mode == "?":
            unknown += 1
            continue
        rows.append((int(m), -1 if C < 0 else 1, mode))
    return sorted(rows), unknown


def levels_of(plane, m: int, s: int, pl: dict) -> tuple:
    """(sigma, A, valid) of the marker's 32 bits."""
    n = len(plane)
    sigma = amp = 0
    for i in range(32):
        at = m + pl["o16"][i]
        if not 0 <= at < n:
            return 0, 0, 0
        x = s * int(plane[at])
        sigma += x
        amp += x if (MARKER >> (31 - i)) & 1 else -x
    return sigma, amp, 1


def frame_record(plane, m: int, s: int, pl: dict) -> list:
    """[sigma, A, raw FIW, fixed FIW, status, valid]."""
    n = len(plane)
    sigma, amp, valid = levels_of(plane, m, s, pl)
    if not valid:
        return [0, 0, 0, 0, 3, 0]
    raw = 0
    for j in range(32):
        at = m + pl["o16"][64 + j]
        if not 0 <= at < n:
            return [sigma, amp, 0, 0, 3, 1]
        if 32 * s * int(plane[at]) - sigma > 0:
            raw |= 1 << j
    fixed, status = correct(raw)
    return [sigma, amp, raw, fixed, status, 1]


def frame_records(plane, hits, pl: dict) -> np.ndarray:
    return np.array([frame_record(plane, int(m), int(s), pl) for m, s in hits], dtype=np.int64).reshape(-1, 6)


def slice_symbol(y: int, sigma: int, amp: int, levels: int) -> tuple:
    d = 32 * y - sigma
    return int(d > 0), int(levels == 4 and 3 * abs(d) < 2 * amp)


def words_by_loops(plane, rec, levels: int, u: int, pl: dict) -> tuple:
    """(fixed, raw, status), each [5][4][88] as nested lists, of one frame ``rec`` = (m, s, sigma, A)."""
    m, s, sigma, amp = (int(x) for x in rec)
    n = len(plane)
    per = 256 * u
    fixed = [[[0] * WORDS for _ in range(4)] for _ in range(5)]
    raw = [[[0] * WORDS for _ in range(4)] for _ in range(5)]
    status = [[[4] * WORDS for _ in range(4)] for _ in range(5)]
    for e in range(5):
        d = (e - 2) * pl["step"][u]
        for ph in range(4):
            pair, second = ph // 2, ph % 2
            if (second and levels != 4) or (pair and u != 2):
                continue
            for w in range(WORDS):
                b, col = w // 8, w % 8
                word, outside = 0, False
                for j in range(32):
                    k = 8 * j + col
                    q = b * per + k * u + pair
                    at = m + pl["data"][u][q] + d
                    if not 0 <= at < n:
                        outside = True
                        break
                    word |= slice_symbol(s * int(plane[at]), sigma, amp, levels)[second] << j
                if outside:
                    fixed[e][ph][w], raw[e][ph][w], status[e][ph][w] = 0, 0, 3
                else:
                    raw[e][ph][w] = word
                    fixed[e][ph][w], status[e][ph][w] = correct(word)
    return fixed, raw, status


def words(plane, recs, levels: int, u: int, pl: dict) -> tuple:
    """(fixed uint32[F][5][4][88], raw, status uint8): the vectorised form."""
    plane = np.asarray(plane, dtype=np.int64)
    recs = np.asarray(recs, dtype=np.int64).reshape(-1, 4)
    n = plane.size
    shape = (recs.shape[0], 5, 4, WORDS)
    fixed, raw, status = np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.uint32), np.full(shape, 4, dtype=np.uint8)
    off = np.asarray(pl["data"][u], dtype=np.int64)
    weight = (1 << np.arange(32, dtype=np.int64))[None, :, None]
    for f, (m, s, sigma, amp) in enumerate(recs.tolist()):
        for e in range(5):
            at = m + off + (e - 2) * pl["step"][u]
            inside = (at >= 0) & (at < n)
            y = s * plane[np.clip(at, 0, max(n - 1, 0))] if n else np.zeros_like(at)
            d = 32 * y - sigma
            bits = [(d > 0), (3 * np.abs(d) < 2 * amp)]
            for ph in range(4):
                pair, second = ph // 2, ph % 2
                if (second and levels != 4) or (pair and u != 2):
                    continue
                take = lambda a: a.reshape(BLOCKS, 256, u)[:, :, pair].reshape(BLOCKS, 32, 8)  # noqa: E731  [b][j][col]
                val = (take(bits[second]).astype(np.int64) * weight).sum(axis=1).reshape(WORDS)
                out = ~take(inside).all(axis=1).reshape(WORDS)
                for w in range(WORDS):
                    if out[w]:
                        fixed[f, e, ph, w], raw[f, e, ph, w], status[f, e, ph, w] = 0, 0, 3
                    else:
                        raw[f, e, ph, w] = int(val[w])
                        fixed[f, e, ph, w], status[f, e, ph, w] = correct(int(val[w]))
    return fixed, raw, status


def choose_shifts(status, mode: str) -> list:
    """Per block the shift index e with the fewest words of status >= 2 over the active phases of one frame ([5][4][88]); ties
    to the smaller |d|, then to the negative one."""
    out = []
    for b in range(BLOCKS):
        best = None
        for d in SHIFT_ORDER:
            bad = sum(int(status[d + 2][PHASES.index(p)][w]) >= 2 for p in ACTIVE[mode] for w in range(8 * b, 8 * b + 8))
            if best is None or bad < best[0]:
                best = (bad, d + 2)
        out.append(best[1])
    return out


def take_shifts(arr, chosen) -> np.ndarray:
    """[4][88] of one frame's [5][4][88] at the chosen shifts."""
    arr = np.asarray(arr)
    return np.stack([np.concatenate([arr[chosen[b], ph, 8 * b : 8 * b + 8] for b in range(BLOCKS)]) for ph in range(4)])


# ---- the parser ----------------------------------------------------------------------------------------------------------------


def read_numeric(infos, skip: int) -> str:
    bits = [(x >> i) & 1 for x in infos for i in range(21)]
    out = ""
    for at in range(skip, len(bits) - 3, 4):
        digit = bits[at] | bits[at + 1] << 1 | bits[at + 2] << 2 | bits[at + 3] << 3
        if digit != 0xC:
            out += DIGITS[digit]
    return out


def read_phase(fixed, status) -> tuple:
    """(state, pages) of one phase: state ``ok``, ``idle``, ``biw_lost`` or ``biw_bad``; pages as (capcode or None, kind, text,
    fragment, more, damaged), with ``dropped`` in place of a page whose vector does not hold."""
    info = [int(w) & MASK for w in fixed]
    status = [int(x) for x in status]
    if status[0] >= 2:
        return "biw_lost", []
    if info[0] in (0, MASK):
        return "idle", []
    aoff, voff = ((info[0] >> 8) & 3) + 1, (info[0] >> 10) & 0x3F
    if aoff > voff or 2 * voff - aoff > WORDS:
        return "biw_bad", []
    pages, i = [], aoff
    while i < voff:
        at, vec = i, voff + i - aoff
        if status[at] >= 2 or (is_long(info[at]) and at + 1 >= voff):
            pages.append("dropped")
            i += 1
            continue
        long = is_long(info[at])
        i += 2 if long else 1
        v = info[vec]
        good = status[vec] <= 1 and check4(v)
        if long:
            pages.append((None, TYPES[(v >> 4) & 7] if good else None, None, None, None, False))
            continue
        if not good:
            pages.append("dropped")
            continue
        kind, start = (v >> 4) & 7, (v >> 7) & 0x7F
        count = (v >> 14) & 0x7F if kind in (0, 5, 6) else ((v >> 14) & 7) + 1
        if kind in (1, 2):
            pages.append((info[at] - 0x8000, TYPES[kind], None, None, None, False))
            continue
        if start < 2 * voff - aoff or start + count > WORDS or count < 1:
            pages.append("dropped")
            continue
        body = range(start, start + count)
        damaged = any(status[j] >= 2 for j in body)
        text = fragment = more = None
        if kind == 5:
            head = status[start] <= 1
            fragment, more = ((info[start] >> 11) & 3, bool((info[start] >> 10) & 1)) if head else (None, None)
            text = ""
            for j in list(body)[1:]:
                if status[j] >= 2:
                    text += "\ufffd" * 3
                    continue
                chars = [(info[j] >> (7 * c)) & 0x7F for c in range(3)]
                if j == start + 1 and fragment == 3:
                    chars = chars[1:]
                text += "".join(chr(c) if 0x20 <= c <= 0x7E else "\ufffd" for c in chars if c not in (0, 3))
            damaged = not head or any(status[j] >= 2 for j in list(body)[1:])
        elif kind in (3, 4, 7):
            text = read_numeric([info[j] for j in body], 12 if kind == 7 else 2)
        pages.append((info[at] - 0x8000, TYPES[kind], text, fragment, more, damaged))
    return "ok", pages


def read_fiw(fixed: int, status: int):
    """(cycle, frame) or None."""
    x = int(fixed) & MASK
    if int(status) > 1 or not check4(x):
        return None
    return (x >> 4) & 0xF, (x >> 8) & 0x7F


# ---- the whole oracle on planes -------------------------------------------------------------------------------------------------


def decode_planes(v16, v32, hits, pl: dict) -> dict:
    """From the integrator planes and the kept hits of the ``flex`` pattern to the pages: ``rows``, ``unknown_mode``, ``rec16``,
    ``rec32``, ``ok``, ``fixed`` / ``raw`` / ``status`` ([F][5][4][88]), ``chosen`` ([F][11]), ``pages`` ((m, cycle, frame,
    phase, mode, inverted) + the page of ``read_phase``, without the dropped ones) and ``states`` per (frame, phase)."""
    rows, unknown = frame_hits(hits)
    f = len(rows)
    ms = [(m, s) for m, s, _ in rows]
    rec16 = frame_records(v16, ms, pl)
    rec32 = np.zeros((f, 6), dtype=np.int64)
    for j, (m, s, mode) in enumerate(rows):
        if SHAPE[mode][0] == 2:
            rec32[j] = frame_record(v32, m, s, pl)
    shape = (f, 5, 4, WORDS)
    fixed, raw, status = np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.uint32), np.full(shape, 4, dtype=np.uint8)
    chosen = np.full((f, BLOCKS), 2, dtype=np.int64)
    ok = np.zeros(f, dtype=bool)
    pages, states = [], {}
    for j, (m, s, mode) in enumerate(rows):
        u, levels = SHAPE[mode]
        sigma, amp = (rec32 if u == 2 else rec16)[j, :2]
        ok[j] = bool(rec16[j, 5]) and amp > 0
        if not ok[j]:
            continue
        fx, rw, stt = words(v16 if u == 1 else v32, [(m, s, sigma, amp)], levels, u, pl)
        fixed[j], raw[j], status[j] = fx[0], rw[0], stt[0]
        chosen[j] = choose_shifts(status[j], mode)
        head = read_fiw(rec16[j, 3], rec16[j, 4])
        if head is None:
            states[j] = "fiw_failed"
            continue
        fx, stt = take_shifts(fixed[j], chosen[j]), take_shifts(status[j], chosen[j])
        for p in ACTIVE[mode]:
            state, got = read_phase(fx[PHASES.index(p)], stt[PHASES.index(p)])
            states[(j, p)] = state
            pages += [(m, head[0], head[1], p, mode, s < 0) + page for page in got if page != "dropped"]
            states[(j, p, "dropped")] = sum(page == "dropped" for page in got)
    return dict(rows=rows, unknown_mode=unknown, rec16=rec16, rec32=rec32, ok=ok, fixed=fixed, raw=raw, status=status, chosen=chosen,
                pages=pages, states=states)


def decode_theta(theta, fs_ch: float, c: int = 0) -> dict:
    """The whole oracle on a discriminator stream: section 25's integrator and search, then ``decode_planes``."""
    pl = plan(fs_ch)
    p16, p32 = pl["ident"][1], pl["ident"][2]
    v16 = IM.integrate(theta, c, p16["L"], p16["sh"])
    v32 = IM.integrate(theta, c, p32["L"], p32["sh"])
    _, hits = IM.search(v16, p16, FLEX_PATTERN)
    out = decode_planes(v16, v32, hits, pl)
    out.update(v16=v16, v32=v32, hits=hits, plan=pl)
    return out


def page_key(page) -> tuple:
    """A package ``FlexPage`` in the form of ``decode_planes``'s pages, without m."""
    return (page.cycle, page.frame, page.phase, page.mode, page.inverted, page.capcode, page.kind, page.text, page.fragment, page.more,
            page.damaged)


# ---- the encoder ---------------------------------------------------------------------------------------------------------------

IDLE = (0, MASK)  # the information of the fill words, alternating


def fiw_info(cycle: int, frame: int, high: int = 0) -> int:
    return with_check4(((cycle & 0xF) << 4) | ((frame & 0x7F) << 8) | ((high & 0x3F) << 15))


def numeric_infos(digits: str, skip: int) -> list:
    bits = [0] * skip
    for ch in digits:
        v = DIGITS.index(ch) if ch != " " else 0xA
        bits += [(v >> i) & 1 for i in range(4)]
    count = -(-len(bits) // 21)
    fill = [(0xC >> i) & 1 for i in range(4)]
    while len(bits) + 4 <= 21 * count:
        bits += fill
    bits += [0] * (21 * count - len(bits))
    return [sum(b << i for i, b in enumerate(bits[21 * j : 21 * j + 21])) for j in range(count)]


def alpha_infos(text: str, fragment: int = 3, more: bool = False, signature: int = 0x55) -> list:
    chars = ([signature] if fragment == 3 else []) + [ord(c) for c in text]
    chars += [0x03] * (-len(chars) % 3)
    head = (int(more) << 10) | ((fragment & 3) << 11)
    return [head] + [chars[i] | chars[i + 1] << 7 | chars[i + 2] << 14 for i in range(0, len(chars), 3)]


def phase_infos(pages, *, aoff: int = 1, break_biw: bool = False) -> list:
    """The 88 information words of a phase carrying ``pages``: dicts with ``kind`` (a name of TYPES), ``capcode`` (short) or
    ``address`` (a pair of raw words, long), ``text`` and for alpha ``fragment``, ``more``; ``drop``: its vector fails check4.
    No page: an idle phase.  ``break_biw``: a block information word whose vector offset lies in front of its address offset."""
    if not pages:
        return [IDLE[w % 2] for w in range(WORDS)]
    slots = sum(2 if "address" in p else 1 for p in pages)
    voff = aoff + slots
    out = [None] * WORDS
    out[0] = with_check4(((aoff - 1) << 8) | (((0 if break_biw else voff) & 0x3F) << 10))
    for w in range(1, aoff):
        out[w] = 0
    at, body = aoff, 2 * voff - aoff
    for p in pages:
        kind = TYPES.index(p["kind"])
        vec = voff + at - aoff
        if "address" in p:
            out[at], out[at + 1] = p["address"]
            out[vec + 1] = 0
            at += 2
        else:
            out[at] = p["capcode"] + 0x8000
            at += 1
        infos = []
        if kind == 5:
            infos = alpha_infos(p["text"], p.get("fragment", 3), p.get("more", False))
            v = (kind << 4) | (body << 7) | (len(infos) << 14)
        elif kind in (3, 4, 7):
            infos = numeric_infos(p["text"], 12 if kind == 7 else 2)
            v = (kind << 4) | (body << 7) | ((len(infos) - 1) << 14)
        else:
            v = kind << 4
        out[vec] = with_check4(v) ^ (1 if p.get("drop") else 0)
        out[body : body + len(infos)] = infos
        body += len(infos)
    assert body <= WORDS
    return [IDLE[w % 2] if x is None else x for w, x in enumerate(out)]


def data_levels(mode: str, phases: dict) -> list:
    """The 2816 u symbol levels (+-3, +-1) of a frame: ``phases`` the 88 codewords per active phase letter."""
    u, levels = SHAPE[mode]
    out = []
    for q in range(SYMBOLS * u):
        b, r = divmod(q, 256 * u)
        k, pair = divmod(r, u)
        bit = lambda p: (phases[p][8 * b + k % 8] >> (k // 8)) & 1  # noqa: E731
        a = bit("AC"[pair])
        second = bit("BD"[pair]) if levels == 4 else 0
        out.append({(1, 0): 3, (1, 1): 1, (0, 1): -1, (0, 0): -3}[(a, second)])
    return out


def frame_segments(mode: str, fiw: int, phases: dict) -> list:
    """(level, length in bits of the 1600 grid) from the 32 bits of bit sync in front of the mode code to the frame's end; the
    marker's first bit is segment 48."""
    word = lambda x, n: [3 if (x >> (n - 1 - i)) & 1 else -3 for i in range(n)]  # noqa: E731  MSB first
    code = MODES[mode]
    head = word(0xAAAAAAAA, 32) + word(code, 16) + word(MARKER, 32) + word(code ^ 0xFFFF, 16) + word(SYNC_B, 16)
    head += [3 if (fiw >> j) & 1 else -3 for j in range(32)] + [3 if i % 2 == 0 else -3 for i in range(40)]
    u = SHAPE[mode][0]
    return [(lev, 1.0) for lev in head] + [(lev, 1.0 / u) for lev in data_levels(mode, phases)]


def make_frame(mode: str, cycle: int, frame: int, pages_by_phase: dict, **options) -> tuple:
    """(segments, the words per phase) of a frame; ``pages_by_phase``: the pages per active phase letter (missing: idle)."""
    phases = {p: [codeword(x) for x in phase_infos(pages_by_phase.get(p, []), **options.get(p, {}))] for p in ACTIVE[mode]}
    return frame_segments(mode, codeword(fiw_info(cycle, frame)), phases), phases


def freq_track(frames, fs: float, n: int, ppm: float = 0.0) -> np.ndarray:
    """float64[n]: the deviation in Hz under every sample at the rate ``fs``; ``frames`` a list of (start in seconds of the first
    bit-sync bit, segments); a level l deviates l 1600 Hz, rectangular symbols; 0 elsewhere.  ``ppm``: the sender's clock runs
    fast by it."""
    f = np.zeros(n, dtype=np.float64)
    for start, segments in frames:
        ends = start + np.cumsum([length for _, length in segments]) / (1600.0 * (1.0 + ppm * 1e-6))
        edges = np.concatenate(([start], ends))
        idx = np.ceil(edges * fs - 1e-9).astype(np.int64)
        for (lev, _), a, b in zip(segments, idx[:-1], idx[1:]):
            f[max(a, 0) : max(min(b, n), 0)] = lev * 1600.0
    return f


def synth_theta(frames, fs_ch: float, n: int, *, inverted: bool = False, noise: float = 0.0, seed: int = 1, ppm: float = 0.0) -> np.ndarray:
    """float32[n]: the discriminator output of ``freq_track`` at the channel rate.  ``noise``: the sigma of white Gaussian noise
    on theta, in radians."""
    theta = 2.0 * np.pi * freq_track(frames, fs_ch, n, ppm) / fs_ch
    if noise:
        theta = theta + noise * np.random.default_rng(seed).standard_normal(n)
    return ((-theta) if inverted else theta).astype(np.float32)


FRAME_BITS = 48 + 136 + SYMBOLS  # bits of the 1600 grid from the first bit-sync bit to the frame's end


# ---- the model capture ---------------------------------------------------------------------------------------------------------

K = IM.K
M = K.M
FS, SECS, AMP = IM.FS, IM.SECS, IM.AMP
CAPTURE_START = 0.05  # seconds: the first bit-sync bit of the capture's frame
CAPTURE_PAGES = {"A": [dict(kind="alpha", capcode=1234567, text="MODEL CAPTURE"), dict(kind="numeric", capcode=4242, text="555-0199")],
                 "B": [dict(kind="tone", capcode=77)], "C": [dict(kind="alpha", capcode=99, text="PHASE C", fragment=0, more=True)],
                 "D": [dict(kind="numbered numeric", capcode=5, text="12345")]}
CAPTURE_CHANNELS = (("flex", 200e3), ("voice", 600e3))


@functools.lru_cache(maxsize=1)
def capture(mode: str = "1600/2") -> np.ndarray:
    """int16[n][2]: a model capture in ``ident_model``'s conventions (s16, 2.4 MS/s, 2 s, AMP 0.05, complex noise 30 dB under AMP
    in total, seed 11, DC 0.01): a FLEX channel at +200 kHz carrying one real frame of ``mode`` (cycle 3, frame 45,
    CAPTURE_PAGES) on an otherwise unmodulated carrier, and an NFM voice channel at +600 kHz."""
    n = int(round(FS * SECS))
    t = np.arange(n) / FS
    rng = np.random.default_rng(11)
    sigma = AMP * 10.0 ** (-30.0 / 20.0) / math.sqrt(2.0)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    off = dict(CAPTURE_CHANNELS)
    car = lambda name: np.exp(2j * np.pi * ((off[name] * t) % 1.0))  # noqa: E731
    segments, _ = make_frame(mode, 3, 45, CAPTURE_PAGES)
    x += (AMP / 2.0) * car("flex") * K._fm_of(freq_track([(CAPTURE_START, segments)], FS, n))
    x += (AMP / 2.0) * car("voice") * K._fm_of(2500.0 * M.voice(1, n))
    x += 0.01
    out = np.empty((n, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real * 32768.0), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag * 32768.0), -32768, 32767)
    out.setflags(write=False)
    return out


def model_run(mode: str) -> dict:
    """The whole oracle on the model capture of ``mode``: the numpy finder, the float64 channelizer, section 23's keying and
    label, section 25's identification and this section's pages, per found channel."""
    FD = K.FM
    raw = capture(mode)
    p = FD.plan(FS, raw.shape[0])
    st = FD.run(FD.rows(raw, p), p)
    found = FD.result(p, st["runs"], st["on"], st["mean"], None)
    x = FD.to_complex(raw)
    zs = {}

    def streams(j, dp):
        zs[j] = M.channelize(x, FS, dp["offset_hz"], dp["taps"], dp["D"]).astype(np.complex64)
        return zs[j]

    described = M.describe_run(p, st, found, streams, None, min(raw.shape[0], K.BLOCK_FRAMES))
    out = []
    for j, d in enumerate(described):
        theta = K.quadrature(zs[j])
        k = K.key_stream(zs[j], theta, d["sh"], d["gate"], d["plan"], M.find_args(p), K.calls_of(raw.shape[0], d["plan"]["D"]))
        k["label"], k["baud"] = K.rule(k["coh"], k["rate_hz"], k["crossings"], k["plan"]) if d["label"] == "nfm" else (None, None)
        named = IM.identify_stream(theta, k["c"], k["keyed_from"], k["label"], k["baud"], d["plan"]["fs_ch"])
        pages = None
        if named["rate"] == 1600 and named["plan"] is not None:
            pages = decode_theta(np.asarray(theta)[k["keyed_from"] :], d["plan"]["fs_ch"], k["c"])
        out.append(dict(described=d, keyed=k, named=named, flex=pages))
    return out
