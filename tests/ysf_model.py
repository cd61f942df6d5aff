"""Numpy model and encoder of the YSF (System Fusion) frame decoding (--find-ysf), written from the
specification with its own copy of every constant.  Of the package it uses nothing; the quantiser, the integrator and the sync
search are ``ident_model``'s.  The encoder goes from the FICH fields and the DCH bytes through the CRC, the whitening, the Golay
and the convolutional code and the interleave to the 480 symbols of a frame, then to a rectangular 4-level FSK theta.  The
decoder is plain loops, one function per step: the levels and the slicing, the Viterbi decoder with the stated tie rule, the
nearest Golay word, the records; then the host rules (checks, fields, transmissions) as dicts.  Also the model capture of the
CLI tests: one YSF channel and a voice channel."""
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
K = IM.K
M = K.M

SYNC = 0xD471C9634D
SYNC_SYMBOLS = 20
LEVEL = {0b01: 3, 0b00: 1, 0b10: -1, 0b11: -3}
DIBIT = {v: k for k, v in LEVEL.items()}
YSF_PATTERNS = [p for p in IM.PATTERNS if p[0] == "ysf"]
OFFSETS, WORDS, FICH_RECORD, INFO, RECORD = 480, 30, 5, 12, 4
SCALE = 584
GOLAY_POLY = 0xC75
FAR = 1000
HANG_S = 0.360
DEV = 900.0  # a level of +-1 / +-3 deviates +-900 / +-2700 Hz
NEED_FICH, NEED_DCH = 120, 480
PN9_20 = bytes.fromhex("93D751219C2F6CD0EF0FF83DF1732094ED1E7CD8")
MODES = {0: "V/D1", 1: "data FR", 2: "V/D2", 3: "voice FR"}


def word_bits(word: int, n: int) -> list:
    return [(word >> (n - 1 - i)) & 1 for i in range(n)]


def bits_word(bits) -> int:
    out = 0
    for b in bits:
        out = out << 1 | int(b)
    return out


def bytes_bits(data) -> list:
    return [b for byte in data for b in word_bits(int(byte), 8)]


def sync_levels() -> list:
    return [LEVEL[(SYNC >> (2 * (SYNC_SYMBOLS - 1 - i))) & 3] for i in range(SYNC_SYMBOLS)]


# ---- the codes ----------------------------------------------------------------------------------------------------------------


def golay(data: int) -> int:
    r = data << 11
    for i in range(22, 10, -1):
        if (r >> i) & 1:
            r ^= GOLAY_POLY << (i - 11)
    cw = data << 12 | (r & 0x7FF) << 1
    return cw | bin(cw).count("1") & 1


GOLAY = np.array([golay(d) for d in range(4096)], dtype=np.uint32)


def golay_decode(word: int) -> tuple:
    """(distance, data, refused) of a 24-bit word: the nearest codeword, the smaller data on equal distance."""
    dist = np.bitwise_count(GOLAY ^ np.uint32(word)).astype(np.int64)
    key = int(((dist << 12) | np.arange(4096)).min())
    return (key >> 12, key & 0xFFF, False) if key >> 12 <= 3 else (key >> 12, word >> 12, True)


def crc16(data) -> int:
    """CRC-CCITT from 0, complemented."""
    crc = 0
    for byte in data:
        for i in range(7, -1, -1):
            top = ((crc >> 15) & 1) ^ ((int(byte) >> i) & 1)
            crc = (crc << 1) & 0xFFFF
            if top:
                crc ^= 0x1021
    return crc ^ 0xFFFF


def pn9(count: int) -> bytes:
    """``count`` bytes of the whitening stream: b[n] = b[n - 5] ^ b[n - 9] behind 1 0 0 1 0 0 1 1 1, MSB first."""
    bits = [1, 0, 0, 1, 0, 0, 1, 1, 1]
    while len(bits) < 8 * count:
        bits.append(bits[-5] ^ bits[-9])
    return bytes(bits_word(bits[8 * j : 8 * j + 8]) for j in range(count))


def whiten(data) -> list:
    return [int(a) ^ b for a, b in zip(data, pn9(len(data)))]


def conv_encode(bits) -> list:
    """The sent bits of ``bits`` and four zero tail bits: g1 = d ^ d3 ^ d4, then g2 = d ^ d1 ^ d2 ^ d4."""
    d1 = d2 = d3 = d4 = 0
    out = []
    for d in list(bits) + [0, 0, 0, 0]:
        out += [d ^ d3 ^ d4, d ^ d1 ^ d2 ^ d4]
        d1, d2, d3, d4 = d, d1, d2, d3
    return out


def interleave_at(i: int, rows: int) -> int:
    """The channel dibit of coded dibit ``i`` of a block of 20 ``rows`` dibits."""
    return 20 * (i % rows) + i // rows


def interleave(coded_bits, rows: int) -> list:
    """The channel bits of the coded bits of one block."""
    sent = [0] * len(coded_bits)
    for i in range(len(coded_bits) // 2):
        at = interleave_at(i, rows)
        sent[2 * at], sent[2 * at + 1] = coded_bits[2 * i], coded_bits[2 * i + 1]
    return sent


def deinterleave(channel_bits, rows: int) -> list:
    out = []
    for i in range(len(channel_bits) // 2):
        at = interleave_at(i, rows)
        out += [channel_bits[2 * at], channel_bits[2 * at + 1]]
    return out


def viterbi(coded_bits, smaller: bool = True) -> tuple:
    """(the decoded bits with the tail, the metric, the ties on the surviving path) of the coded bits of one block: sixteen
    states d1 d2 d3 d4 (d1 the top bit), from state 0 to state 0, Hamming metric.  ``smaller``: on equal metrics the predecessor
    with the smaller state index survives, as the specification has it; False is the other rule, by which the tests find a
    word on which the rule matters."""
    steps = len(coded_bits) // 2
    metric = [0] + [FAR] * 15
    back, tied = [], []
    for t in range(steps):
        rx = (coded_bits[2 * t], coded_bits[2 * t + 1])
        new, arg, tie = [], [], []
        for state in range(16):
            d = state >> 3
            cost = []
            for prev in ((state & 7) << 1, (state & 7) << 1 | 1):
                d1, d2, d3, d4 = prev >> 3 & 1, prev >> 2 & 1, prev >> 1 & 1, prev & 1
                cost.append(metric[prev] + (rx[0] != d ^ d3 ^ d4) + (rx[1] != d ^ d1 ^ d2 ^ d4))
            second = cost[1] < cost[0] if smaller else cost[1] <= cost[0]
            new.append(cost[1] if second else cost[0])
            arg.append(1 if second else 0)
            tie.append(cost[0] == cost[1])
        metric = new
        back.append(arg)
        tied.append(tie)
    state, out, ties = 0, [], 0
    for t in range(steps - 1, -1, -1):
        out.append(state >> 3)
        ties += tied[t][state]
        state = (state & 7) << 1 | back[t][state]
    out.reverse()
    return out, metric[0], ties


# ---- the encoder --------------------------------------------------------------------------------------------------------------


def fich_bytes(fi=1, cs=0, cm=0, bn=0, bt=0, fn=0, ft=0, dev=0, mr=0, voip=0, dt=2, sql=0, sq=0) -> list:
    return [fi << 6 | cs << 4 | cm << 2 | bn, bt << 6 | fn << 3 | ft, dev << 6 | mr << 3 | voip << 2 | dt, sql << 7 | sq]


def fich_channel_bits(four, break_crc: bool = False) -> list:
    """The 200 frame bits 40 .. 239 of the four FICH bytes."""
    crc = crc16(four) ^ (1 if break_crc else 0)
    bits = bytes_bits(list(four) + [crc >> 8, crc & 0xFF])
    words = [b for j in range(4) for b in word_bits(int(GOLAY[bits_word(bits[12 * j : 12 * j + 12])]), 24)]
    return interleave(conv_encode(words), 5)


def dch_channel_bits(data, break_crc: bool = False) -> list:
    """The 360 or 200 channel bits of the 20 or 10 data bytes of one DCH block: whitened, the CRC over what is sent."""
    sent = whiten(data)
    crc = crc16(sent) ^ (1 if break_crc else 0)
    return interleave(conv_encode(bytes_bits(sent + [crc >> 8, crc & 0xFF])), 9 if len(data) == 20 else 5)


def frame_class(four) -> int:
    fi, dt = four[0] >> 6, four[2] & 3
    if fi in (0, 2) or (fi == 1 and dt == 1):
        return 1
    if fi == 1 and dt == 0:
        return 2
    if fi == 1 and dt == 2:
        return 3
    return 0


def callsign_bytes(text: str) -> list:
    return list(text.encode("ascii").ljust(10)[:10])


def make_frame(item, rng) -> list:
    """The 480 dibits of one frame of a script: (the four FICH bytes, DCH-a bytes or None, DCH-b bytes or None[, options]); what
    the class does not read is seeded random bits.  Options: ``break_fich`` / ``break_a`` / ``break_b`` spoil a CRC."""
    four, a, b = item[0], item[1], item[2]
    opt = item[3] if len(item) > 3 else {}
    cls = frame_class(four)
    payload = rng.integers(0, 2, 720).tolist()
    part = 40 if cls == 3 else 72
    for data, shift, flag in ((a, 0, "break_a"), (b, 72, "break_b")):
        if data is None or cls == 0 or (shift and cls != 1):
            continue
        sent = dch_channel_bits(data, opt.get(flag, False))
        assert len(sent) == 5 * part
        for j, bit in enumerate(sent):
            payload[144 * (j // part) + shift + j % part] = bit
    bits = word_bits(SYNC, 40) + fich_channel_bits(four, opt.get("break_fich", False)) + payload
    return [bits[2 * i] << 1 | bits[2 * i + 1] for i in range(OFFSETS)]


def station(script, seed: int = 5) -> list:
    """The symbol levels of a station that sends the frames of ``script`` one behind the other; ("random", count) is ``count``
    seeded random symbols without a sync word."""
    rng = np.random.default_rng(seed)
    out = []
    for item in script:
        if item[0] == "random":
            out += (2 * rng.integers(0, 4, item[1]) - 3).tolist()
        else:
            out += [LEVEL[d] for d in make_frame(item, rng)]
    return out


def synth_theta(levels, fs_ch: float, n: int, start_s: float = 0.0, noise: float = 0.0, seed: int = 1) -> np.ndarray:
    """float32[n]: the discriminator output of the rectangular 4-level FSK of ``levels`` at 4800 symbols/s from ``start_s`` on, a
    level l deviating l 900 Hz, 0 elsewhere; ``noise``: the sigma of white Gaussian noise on theta, in radians."""
    f = np.zeros(n, dtype=np.float64)
    edges = start_s + np.arange(len(levels) + 1) / 4800.0
    idx = np.ceil(edges * fs_ch - 1e-9).astype(np.int64)
    for lev, a, b in zip(levels, idx[:-1], idx[1:]):
        f[max(a, 0) : max(min(b, n), 0)] = lev * DEV
    theta = 2.0 * np.pi * f / fs_ch
    if noise:
        theta = theta + noise * np.random.default_rng(seed).standard_normal(n)
    return theta.astype(np.float32)


# ---- the decoder: plan, hits, levels, slicing ----------------------------------------------------------------------------------


def plan(fs_ch: float) -> dict:
    """sps, o[0 .. 479] and ``ident_model``'s plan at 4800; ValueError unless 4 <= sps <= 224."""
    ident = IM.plan(fs_ch, 4800)
    return dict(fs_ch=float(fs_ch), sps=ident["sps"], o=[int(round(i * ident["sps"])) for i in range(OFFSETS)], ident=ident)


def frame_hits(kept, h: int) -> list:
    """(m, s) in order of m from ``ident_model``'s kept hits over YSF_PATTERNS (pattern 0)."""
    cand = [(m, abs(C), 1 if C > 0 else -1) for p, m, C, _E, _pre, _post in kept if p == 0 and C != 0]
    out = []
    for m, a, s in cand:
        if not any(m2 != m and abs(m2 - m) <= h and (a2 > a or (a2 == a and m2 < m)) for m2, a2, _ in cand):
            out.append((m, s))
    return sorted(out)


def levels_of(x, s: int) -> tuple:
    """(A, Dc) of the twenty plane values under the sync word."""
    p, q = sum(x), sum(g * xi for g, xi in zip(sync_levels(), x))
    return s * (15 * q - 9 * p), 31 * p - 3 * q


def slice_by_loops(v, n: int, m: int, s: int, pl: dict) -> tuple:
    """(the 30 words, [A, Dc, valid]) of one hit."""
    o = pl["o"]
    valid = 0 if m + o[0] < 0 else sum(1 for i in range(OFFSETS) if m + o[i] < n)
    if valid < SYNC_SYMBOLS:
        return [0] * WORDS, [0, 0, valid]
    amp, dc = levels_of([int(v[m + o[i]]) for i in range(SYNC_SYMBOLS)], s)
    bits = []
    for i in range(OFFSETS):
        if i >= valid:
            bits += [0, 0]
            continue
        d = s * (SCALE * int(v[m + o[i]]) - dc)
        bits += [1 if d < 0 else 0, 1 if 3 * abs(d) >= 2 * amp else 0]
    return [bits_word(bits[32 * w : 32 * w + 32]) for w in range(WORDS)], [amp, dc, valid]


def slice_all(v, rows, pl: dict) -> tuple:
    """(bits uint32[K][30], levels int64[K][3]) of ``rows`` (m, s)."""
    out = [slice_by_loops(v, len(v), int(m), int(s), pl) for m, s in np.asarray(rows, dtype=np.int64).reshape(-1, 2).tolist()]
    return (np.array([o[0] for o in out], dtype=np.uint32).reshape(-1, WORDS), np.array([o[1] for o in out], dtype=np.int64).reshape(-1, 3))


# ---- the decoder: one frame's coders ----------------------------------------------------------------------------------------------


def record_bits(words) -> list:
    return [b for w in words for b in word_bits(int(w), 32)]


def words_of_dibits(dibits) -> list:
    bits = [b for d in list(dibits)[:OFFSETS] for b in (d >> 1, d & 1)]
    bits += [0] * (2 * OFFSETS - len(bits))
    return [bits_word(bits[32 * w : 32 * w + 32]) for w in range(WORDS)]


def fich_decode(words, smaller: bool = True) -> tuple:
    """(the two words, the five values) of one sliced frame, as ``iqa_ysf_fich`` gives them."""
    frame = record_bits(words)
    decoded, metric, _ = viterbi(deinterleave(frame[40:240], 5), smaller)
    data, corrected, refused, changed = [], 0, 0, 0
    for j in range(4):
        dist, value, bad = golay_decode(bits_word(decoded[24 * j : 24 * j + 24]))
        data += word_bits(value, 12)
        if bad:
            refused += 1
        elif dist:
            corrected += 1
            changed += dist
    status = 2 if refused else 1 if metric or corrected else 0
    return [bits_word(data[:32]), bits_word(data[32:]) << 16], [status, metric, corrected, refused, changed]


def fich_all(bits) -> tuple:
    out = [fich_decode(w) for w in np.asarray(bits).tolist()]
    return (np.array([o[0] for o in out], dtype=np.uint32).reshape(-1, 2), np.array([o[1] for o in out], dtype=np.int32).reshape(-1, FICH_RECORD))


def dch_bits(frame_bits, cls: int, second: bool) -> list:
    """The channel bits of a data channel: of every payload block the first 72 (40 for class 3), or the 72 behind them."""
    part = 40 if cls == 3 else 72
    return [frame_bits[240 + 144 * p + (72 if second else 0) + k] for p in range(5) for k in range(part)]


def decode_frame(words, cls: int, smaller: bool = True) -> tuple:
    """(info, rec, ties): the twelve information words and the four values of one sliced frame, as ``iqa_ysf_decode`` gives
    them, and the ties on the surviving paths."""
    frame = record_bits(words)
    out, rec, ties = [0] * (32 * INFO), [cls if 0 <= cls <= 3 else 0, 0, 0, 0], 0
    for second in ((False, True) if cls == 1 else (False,) if cls in (2, 3) else ()):
        decoded, metric, tie = viterbi(deinterleave(dch_bits(frame, cls, second), 5 if cls == 3 else 9), smaller)
        out[192 * second : 192 * second + len(decoded)] = decoded
        rec[1 + second] = metric
        ties += tie
    return [bits_word(out[32 * w : 32 * w + 32]) for w in range(INFO)], rec, ties


def decode_all(bits, classes) -> tuple:
    """(info uint32[K][12], rec int32[K][4])."""
    out = [decode_frame(w, int(c)) for w, c in zip(np.asarray(bits).tolist(), np.asarray(classes).tolist())]
    return (np.array([o[0] for o in out], dtype=np.uint32).reshape(-1, INFO), np.array([o[1] for o in out], dtype=np.int32).reshape(-1, RECORD))


# ---- the decoder: the host rules --------------------------------------------------------------------------------------------------


def word_bytes(words) -> list:
    return [(int(w) >> sh) & 0xFF for w in words for sh in (24, 16, 8, 0)]


def fich_ok(two) -> bool:
    by = word_bytes(two)
    return crc16(by[:4]) == (by[4] << 8 | by[5])


def apply_flags(frec, levels) -> np.ndarray:
    frec = np.array(frec, dtype=np.int32).reshape(-1, FICH_RECORD)
    for j, lev in enumerate(np.asarray(levels).tolist()):
        if lev[2] < NEED_FICH:
            frec[j, 0] = 3
    return frec


def decoder_classes(fich, frec, levels) -> list:
    """The class that picks a frame's decoder: 0 where the FICH is cut or fails its check, or the frame is cut."""
    out = []
    for two, r, lev in zip(np.asarray(fich).tolist(), np.asarray(frec).tolist(), np.asarray(levels).tolist()):
        out.append(frame_class(word_bytes(two)) if r[0] != 3 and lev[0] > 0 and fich_ok(two) and lev[2] >= NEED_DCH else 0)
    return out


def callsign(ten):
    if any(b < 0x20 or b > 0x7E for b in ten):
        return None
    return bytes(ten).decode("ascii").strip()


def block_fields(cls: int, fi: int, fn: int, second: bool) -> tuple:
    """The names of the two halves (class 3: of the one field) that a good block of a frame brings."""
    if cls == 1:
        return (("downlink", "uplink") if second else ("dst", "src")) if fi in (0, 2) or fn == 0 else ()
    if cls == 2:
        return {0: ("dst", "src"), 1: ("downlink", "uplink"), 2: ("rem12", "rem34")}.get(fn, ())
    if cls == 3:
        return {0: ("dst",), 1: ("src",), 2: ("downlink",), 3: ("uplink",), 4: ("rem12",), 5: ("rem34",)}.get(fn, ())
    return ()


def parse(rows, levels, fich, frec, info, rec, fs_ch: float, start: int = 0) -> tuple:
    """(frames, counts): a dict per frame whose FICH was read, in order of time."""
    counts = dict(no_level=0, cut=0, fich_failed=0, golay_refused=0, dch_failed=0, fixed=0)
    out = []
    for (m, _s), lev, two, fr, words, r in zip(np.asarray(rows).tolist(), np.asarray(levels).tolist(), np.asarray(fich).tolist(),
                                               np.asarray(frec).tolist(), np.asarray(info).tolist(), np.asarray(rec).tolist()):
        if fr[0] == 3:
            counts["cut"] += 1
            continue
        if lev[0] <= 0:
            counts["no_level"] += 1
            continue
        counts["golay_refused"] += fr[3]
        if not fich_ok(two):
            counts["fich_failed"] += 1
            continue
        b = word_bytes(two)[:4]
        f = dict(time_s=(start + m) / fs_ch, fi=b[0] >> 6, cs=b[0] >> 4 & 3, cm=b[0] >> 2 & 3, bn=b[0] & 3, bt=b[1] >> 6, fn=b[1] >> 3 & 7, ft=b[1] & 7,
                 dev=b[2] >> 6 & 1, mr=b[2] >> 3 & 7, voip=b[2] >> 2 & 1, dt=b[2] & 3, sql=b[3] >> 7, sq=b[3] & 0x7F, cls=frame_class(b),
                 corrected=fr[0] == 1, blocks=[], fields={})
        if f["cls"]:
            if lev[2] < NEED_DCH:
                counts["cut"] += 1
            else:
                size = 10 if f["cls"] == 3 else 20
                for second in ((False, True) if f["cls"] == 1 else (False,)):
                    by = word_bytes(words[6 * second : 6 * second + 6])
                    ok = crc16(by[:size]) == (by[size] << 8 | by[size + 1])
                    data = whiten(by[:size])
                    f["blocks"].append([bytes(data).hex(), ok])
                    if not ok:
                        counts["dch_failed"] += 1
                        continue
                    f["corrected"] = f["corrected"] or r[1 + second] > 0
                    for k, name in enumerate(block_fields(f["cls"], f["fi"], f["fn"], second)):
                        f["fields"][name] = callsign(data[10 * k : 10 * k + 10])
        counts["fixed"] += f["corrected"]
        out.append(f)
    return sorted(out, key=lambda f: f["time_s"]), counts


FIELDS = ("src", "dst", "downlink", "uplink", "rem12", "rem34")


def track(frames) -> list:
    """The transmissions as dicts, in order of their start."""
    out, cur, last = [], None, 0.0
    for f in frames:
        if cur is not None and f["time_s"] - last > HANG_S:
            cur = None
        last = f["time_s"]
        if cur is None:
            cur = dict(start_s=f["time_s"], end_s=f["time_s"], frames=0, src=None, dst=None, downlink=None, uplink=None, rem12=None, rem34=None,
                       cm=f["cm"], dt=f["dt"], sq=f["sq"] if f["sql"] else None, late=f["fi"] != 0, terminated=False, conflicts=0)
            out.append(cur)
        cur["frames"] += 1
        cur["end_s"] = f["time_s"]
        for name, value in f["fields"].items():
            if value is None:
                continue
            if cur[name] is None:
                cur[name] = value
            elif cur[name] != value:
                cur["conflicts"] += 1
        if f["fi"] == 2:
            cur["terminated"] = True
            cur = None
    return out


def tx_line(t: dict) -> str:
    parts = ["YSF"]
    if t["src"]:
        parts.append(t["src"])
    if t["dst"]:
        parts += ["->", "ALL" if set(t["dst"]) == {"*"} else t["dst"]]
    if t["downlink"] or t["uplink"]:
        parts += ["via", (t["downlink"] or "") + ("/" + t["uplink"] if t["uplink"] else "")]
    if t["cm"] in (0, 3):
        parts.append("group" if t["cm"] == 0 else "individual")
    parts.append(MODES[t["dt"]])
    parts.append("sq=off" if t["sq"] is None else f"sq={t['sq']}")
    parts.append(f"{t['end_s'] - t['start_s']:.2f} s ({t['frames']} frame{'' if t['frames'] == 1 else 's'})")
    return " ".join(parts)


def decode_plane(v, kept, pl: dict, start: int = 0) -> dict:
    """The whole model behind the sync search on one integrated plane."""
    rows = np.array(frame_hits(kept, pl["ident"]["h"]), dtype=np.int64).reshape(-1, 2)
    bits, levels = slice_all(v, rows, pl)
    fich, frec = fich_all(bits)
    frec = apply_flags(frec, levels)
    classes = decoder_classes(fich, frec, levels)
    info, rec = decode_all(bits, classes)
    frames, counts = parse(rows, levels, fich, frec, info, rec, pl["fs_ch"], start)
    return dict(rows=rows, bits=bits, levels=levels, fich=fich, frec=frec, classes=np.array(classes, dtype=np.uint8), info=info, rec=rec,
                frames=frames, counts=counts, txs=track(frames))


def decode_theta(theta, fs_ch: float, c: int = 0) -> dict:
    pl = plan(fs_ch)
    v = IM.integrate(theta, c, pl["ident"]["L"], pl["ident"]["sh"])
    _, kept = IM.search(v, pl["ident"], YSF_PATTERNS)
    out = decode_plane(v, kept, pl)
    out.update(v=v, kept=kept, plan=pl)
    return out


# ---- the test stream and the model capture ---------------------------------------------------------------------------------------

SRC, DST, DOWN, UP, REM12, REM34 = "JA1YOE", "**********", "JP1YJQ", "JP1YJQ-1", "ABCDE12345", "FGHIJ67890"
CS = {name: callsign_bytes(text) for name, text in (("src", SRC), ("dst", DST), ("downlink", DOWN), ("uplink", UP), ("rem12", REM12), ("rem34", REM34))}
VD2_ORDER = ("dst", "src", "downlink", "uplink", "rem12", "rem34")


def header(fi: int = 0, **opt) -> tuple:
    return (fich_bytes(fi=fi, dt=2, ft=7, sql=1, sq=42), CS["dst"] + CS["src"], CS["downlink"] + CS["uplink"], opt)


def vd2(fn: int, **opt) -> tuple:
    data = CS[VD2_ORDER[fn]] if fn < 6 else [0x30 + fn] * 10
    return (fich_bytes(fi=1, dt=2, fn=fn, ft=7, sql=1, sq=42), data, None, opt)


def vd1(fn: int, **opt) -> tuple:
    data = {0: CS["dst"] + CS["src"], 1: CS["downlink"] + CS["uplink"], 2: CS["rem12"] + CS["rem34"]}.get(fn, [0x41 + fn] * 20)
    return (fich_bytes(fi=1, dt=0, fn=fn, ft=7, sql=1, sq=42), data, None, opt)


def data_fr(fn: int, **opt) -> tuple:
    a, b = (CS["dst"] + CS["src"], CS["downlink"] + CS["uplink"]) if fn == 0 else ([0x61 + fn] * 20, [0x71 + fn] * 20)
    return (fich_bytes(fi=1, dt=1, fn=fn, ft=7, sql=1, sq=42), a, b, opt)


def voice_fr(fn: int = 0) -> tuple:
    return (fich_bytes(fi=1, dt=3, fn=fn, ft=7, sql=1, sq=42), None, None)


#: a transmission: its header, the V/D mode 2 frames 0 .. 7, a V/D mode 1 frame, a data FR frame, a voice FR frame, its terminator
SCRIPT = [header()] + [vd2(fn) for fn in range(8)] + [vd1(1), data_fr(0), voice_fr(), header(fi=2)]
STREAM_START = 0.02
LINE = "YSF JA1YOE -> ALL via JP1YJQ/JP1YJQ-1 group V/D2 sq=42 1.20 s (13 frames)"


def test_stream(fs_ch: float, noise: float = 0.0, seed: int = 3, script=SCRIPT, negate: bool = False) -> np.ndarray:
    levels = station(script)
    n = int((STREAM_START + len(levels) / 4800.0 + 0.02) * fs_ch)
    theta = synth_theta(levels, fs_ch, n, STREAM_START, noise, seed)
    return -theta if negate else theta


FS, SECS, AMP = IM.FS, IM.SECS, IM.AMP
CAPTURE_CHANNELS = (("ysf", 200e3), ("voice", 600e3))


def capture_script() -> list:
    """480 random symbols (the channel filter settles in them, and the station is on the air from the first sample), a
    transmission of ten frames, then a second one until the capture ends."""
    first = [header()] + [vd2(fn) for fn in range(8)] + [header(fi=2)]
    return [("random", 480)] + first + [header()] + [vd2(fn % 8) for fn in range(10)]


@functools.lru_cache(maxsize=1)
def capture() -> np.ndarray:
    """int16[n][2]: a model capture in ``ident_model``'s conventions (s16, 2.4 MS/s, 2 s, AMP 0.05, complex noise 30 dB under AMP
    in total, seed 11, DC 0.01): a YSF channel at +200 kHz that sends ``capture_script()``, and an NFM voice channel at +600 kHz."""
    n = int(round(FS * SECS))
    t = np.arange(n) / FS
    rng = np.random.default_rng(11)
    sigma = AMP * 10.0 ** (-30.0 / 20.0) / math.sqrt(2.0)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    off = dict(CAPTURE_CHANNELS)
    car = lambda name: np.exp(2j * np.pi * ((off[name] * t) % 1.0))  # noqa: E731
    levels = station(capture_script())
    x += (AMP / 2.0) * car("ysf") * IM.fsk_levels(levels, 4800.0, DEV, n)
    x += (AMP / 2.0) * car("voice") * K._fm_of(2500.0 * M.voice(1, n))
    x += 0.01
    out = np.empty((n, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real * 32768.0), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag * 32768.0), -32768, 32767)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=1)
def model_run() -> list:
    """The whole model on the model capture: the numpy finder, the float64 channelizer, section 23's keying and label, section
    25's identification and this section's frames and transmissions, per found channel."""
    FD = K.FM
    raw = capture()
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
        ysf = None
        if named["rate"] == 4800 and named["plan"] is not None:
            pl = plan(d["plan"]["fs_ch"])
            ysf = decode_plane(named["v"], [(0,) + tuple(h[1:]) for h in named["kept"] if IM.family(4800)[h[0]][0] == "ysf"], pl, k["keyed_from"])
        out.append(dict(described=d, keyed=k, named=named, ysf=ysf))
    return out


# ---- crafted words for the coders (the host test and the GPU shapes test share them) -----------------------------------------------


def flipped_words(words, frame_bits) -> list:
    """``words`` with the frame bits ``frame_bits`` flipped."""
    out = [int(w) for w in words]
    for b in frame_bits:
        out[b >> 5] ^= 1 << (31 - (b & 31))
    return out


def dch_frame_bit(cls: int, second: bool, j: int) -> int:
    """The frame bit of channel bit ``j`` of a data channel."""
    part = 40 if cls == 3 else 72
    return 240 + 144 * (j // part) + (72 if second else 0) + j % part


def frame_words(item, seed: int = 2) -> list:
    return words_of_dibits(make_frame(item, np.random.default_rng(seed)))


def coded_frame_bit(cls: int, second: bool, c: int) -> int:
    """The frame bit of coded bit ``c`` (in front of the interleave) of a data channel."""
    return dch_frame_bit(cls, second, 2 * interleave_at(c >> 1, 5 if cls == 3 else 9) + (c & 1))


@functools.lru_cache(maxsize=1)
def tie_flips() -> tuple:
    """Four coded bits of the header's DCH-a whose flips (a burst for the decoder: the interleave spreads it over the frame) make
    the tie rule matter.  The code's free distance is odd, so two paths tie only across an error event of even weight: the first
    input pattern whose coded weight is 8, from coded bit 80 on, and the first four of its eight positions on which the two rules
    give different bits."""
    import itertools

    words = frame_words(header())
    for pattern in range(1, 256, 2):
        coded = conv_encode(word_bits(pattern, pattern.bit_length())[::-1])
        at = [80 + k for k, bit in enumerate(coded) if bit]
        if len(at) != 8:
            continue
        for four in itertools.combinations(at, 4):
            bad = flipped_words(words, [coded_frame_bit(1, False, k) for k in four])
            if decode_frame(bad, 1)[0] != decode_frame(bad, 1, smaller=False)[0]:
                return four
    raise AssertionError("no tie found")


def fich_with_golay_errors(four, errors) -> list:
    """The 30 words of a voice FR frame whose FICH Golay word j holds ``errors[j]`` wrong bits *in front of* the convolutional
    coder, so the Viterbi decoder restores them exactly (metric 0) and the Golay decoder meets them."""
    crc = crc16(four)
    bits = bytes_bits(list(four) + [crc >> 8, crc & 0xFF])
    words = []
    for j in range(4):
        cw = int(GOLAY[bits_word(bits[12 * j : 12 * j + 12])])
        for k in range(errors[j]):
            cw ^= 1 << (23 - (5 * k + j) % 24)
        words += word_bits(cw, 24)
    rng = np.random.default_rng(4)
    frame = word_bits(SYNC, 40) + interleave(conv_encode(words), 5) + rng.integers(0, 2, 720).tolist()
    return words_of_dibits([frame[2 * i] << 1 | frame[2 * i + 1] for i in range(OFFSETS)])


@functools.lru_cache(maxsize=1)
def coder_cases() -> dict:
    """name -> (the 30 words, class): the crafted frames of the coder tests."""
    out = {"header": (frame_words(header()), 1), "terminator": (frame_words(header(fi=2)), 1), "vd1": (frame_words(vd1(0)), 2),
           "vd2": (frame_words(vd2(1)), 3), "data-fr": (frame_words(data_fr(3)), 1), "voice-fr": (frame_words(voice_fr()), 0)}
    head = out["header"][0]
    for k in range(0, 360, 17):  # two flipped channel bits to a block, anywhere
        out[f"dch-two-{k}"] = (flipped_words(head, [dch_frame_bit(1, False, k), dch_frame_bit(1, False, (k + 9) % 360),
                                                    dch_frame_bit(1, True, (k + 100) % 360), dch_frame_bit(1, True, (k + 180) % 360)]), 1)
    for k in range(0, 200, 13):
        out[f"fich-two-{k}"] = (flipped_words(head, [40 + k, 40 + (k + 7) % 200]), 1)
        out[f"vd2-two-{k}"] = (flipped_words(out["vd2"][0], [dch_frame_bit(3, False, k), dch_frame_bit(3, False, (k + 11) % 200)]), 3)
    out["dch-tie"] = (flipped_words(head, [coded_frame_bit(1, False, k) for k in tie_flips()]), 1)
    out["dch-burst"] = (flipped_words(head, [coded_frame_bit(1, True, k) for k in range(100, 112)]), 1)
    four = fich_bytes(fi=1, dt=3, fn=5, ft=6, cm=3, sql=1, sq=99)
    for name, errors in (("golay-0000", (0, 0, 0, 0)), ("golay-3333", (3, 3, 3, 3)), ("golay-4000", (4, 0, 0, 0)), ("golay-0403", (0, 4, 0, 3)),
                         ("golay-1234", (1, 2, 3, 4)), ("golay-4444", (4, 4, 4, 4))):
        out[name] = (fich_with_golay_errors(four, errors), 0)
    for cls in (0, 1, 2, 3, 4, 255):
        out[f"class-{cls}"] = (head, cls)
        out[f"zeros-{cls}"], out[f"ones-{cls}"] = ([0] * WORDS, cls), ([0xFFFFFFFF] * WORDS, cls)
    return out
