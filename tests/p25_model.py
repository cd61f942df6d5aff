"""Numpy oracle and encoder of the P25 phase 1 frame decoding (--find-p25), written from the specification
with its own copy of every constant.  Of the package it uses nothing; the quantiser, the integrator and the sync search are
``ident_model``'s.  The encoder goes from a NID through BCH(63,16,23), from link control through the Reed-Solomon remainder and
the Hamming or Golay words to their places, from a trunking block through the CRC, the trellis and the interleave, then the
status symbols, dibits and a rectangular 4-level FSK theta.  The oracle has one function per step: the slicing in plain loops
(``slice_by_loops``) and vectorised (``slice_all``), the coders per frame in plain integers.  Also the model capture of the CLI
tests: one P25 channel and a voice channel."""
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

SYNC = 0x5575F5FF77FF
LEVEL = {0b01: 3, 0b00: 1, 0b10: -1, 0b11: -3}
P25_PATTERNS = [p for p in IM.PATTERNS if p[0] == "p25"]
OFFSETS, WORDS = 864, 54
STATUS_EVERY, STATUS_VALUE = 36, 2
GOLAY_POLY = 0xC75
HAMMING_COLUMNS = (0b1110, 0b1101, 0b1011, 0b0111, 0b0011, 0b1100)
TRELLIS_PAIRS = ((0, 2), (2, 2), (1, 3), (3, 3), (3, 2), (1, 2), (2, 3), (0, 3), (3, 1), (1, 1), (2, 0), (0, 0), (0, 1), (2, 1), (1, 0), (3, 0))
TRELLIS_POINTS = ((0, 15, 12, 3), (4, 11, 8, 7), (13, 2, 1, 14), (9, 6, 5, 10))
INTERLEAVE = tuple(x for r in range(4) for k in range(13 if r == 0 else 12) for x in (8 * k + 2 * r, 8 * k + 2 * r + 1))
GF_POLY = 0x43
DUIDS = {0x0: "hdu", 0x5: "ldu1", 0xA: "ldu2", 0x3: "tdu", 0xF: "tdulc", 0x7: "tsbk", 0xC: "pdu"}
FRAME_SYMBOLS = {0x0: 396, 0x5: 864, 0xA: 864, 0x3: 72, 0xF: 216}  # a TSBK frame: 180 with one block, 360 with three
HANG_S = 0.360
DEV = 600.0  # a level of +-1 / +-3 deviates +-600 / +-1800 Hz
FAR = 1000


def word_bits(word: int, n: int) -> list:
    return [(word >> (n - 1 - i)) & 1 for i in range(n)]


def bits_word(bits) -> int:
    out = 0
    for b in bits:
        out = out << 1 | int(b)
    return out


def sync_levels() -> list:
    return [LEVEL[(SYNC >> (2 * (23 - i))) & 3] for i in range(24)]


def symbol_of(q: int) -> int:
    return q + q // 35


NEED_NID, NEED_TDULC, NEED_LDU1, NEED_TSBK = 57, 205, 699, (158, 259, 359)  # the host test derives them from symbol_of

# ---- the codes ----------------------------------------------------------------------------------------------------------------


def gf_mul(a: int, b: int) -> int:
    """Russian-peasant product in GF(64) / x^6 + x + 1."""
    out = 0
    while b:
        if b & 1:
            out ^= a
        a <<= 1
        if a & 0x40:
            a ^= GF_POLY
        b >>= 1
    return out


def gf_pow(a: int, e: int) -> int:
    out = 1
    for _ in range(e):
        out = gf_mul(out, a)
    return out


ALPHA = 2


def poly_mul(a, b) -> list:
    """The product of two polynomials over GF(64), highest coefficient first."""
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] ^= gf_mul(x, y)
    return out


@functools.lru_cache(maxsize=1)
def bch_generator() -> int:
    """The least common multiple of the minimal polynomials of alpha^1 .. alpha^22 as an integer, bit k the coefficient of x^k."""
    roots = set()
    for r in range(1, 23):
        e = r
        while e not in roots:
            roots.add(e)
            e = 2 * e % 63
    g = [1]
    for e in sorted(roots):
        g = poly_mul(g, [1, gf_pow(ALPHA, e)])
    assert set(g) <= {0, 1}
    return bits_word(g)


def poly2_mod(value: int, gen: int) -> int:
    """value mod gen over GF(2)."""
    top = gen.bit_length() - 1
    for i in range(value.bit_length() - 1, top - 1, -1):
        if (value >> i) & 1:
            value ^= gen << (i - top)
    return value


def bch_encode(data: int) -> int:
    """The 63-bit codeword of a 16-bit value."""
    return data << 47 | poly2_mod(data << 47, bch_generator())


@functools.lru_cache(maxsize=1)
def bch_codewords() -> np.ndarray:
    """uint64[65536]: the code is linear, so the table is built from the sixteen codewords of single bits."""
    out = np.zeros(1, dtype=np.uint64)
    for k in range(16):
        out = np.concatenate([out, out ^ np.uint64(bch_encode(1 << k))])
    return out  # (index d: built low bit first, so out[d] is the codeword of d)


def nid_bits(nac: int, duid: int) -> list:
    cw = bch_encode(nac << 4 | duid)
    return word_bits(cw, 63) + [bin(cw).count("1") & 1]


def nid_decode(bits64) -> list:
    """[status, distance, value, parity_ok] of the 64 bits."""
    word = bits_word(bits64)
    r = word >> 1
    dist = np.bitwise_count(bch_codewords() ^ np.uint64(r)).astype(np.int64)
    key = int(((dist << 16) | np.arange(65536)).min())
    distance, value = key >> 16, key & 0xFFFF
    status = 0 if distance == 0 else 1 if distance <= 11 else 2
    return [status, distance, r >> 47 if status == 2 else value, 1 - (bin(word).count("1") & 1)]


def golay(data: int) -> int:
    r = poly2_mod(data << 11, GOLAY_POLY)
    cw = data << 12 | r << 1
    return cw | bin(cw).count("1") & 1


GOLAY = tuple(golay(d) for d in range(4096))


def golay_decode(word: int) -> tuple:
    """(distance, data, refused) of a 24-bit word."""
    dist, value = min((bin(word ^ cw).count("1"), d) for d, cw in enumerate(GOLAY))
    return (dist, value, False) if dist <= 3 else (dist, word >> 12, True)


def hamming_encode(six) -> list:
    d = [int(b) for b in six]
    return d + [sum(d[j] * ((HAMMING_COLUMNS[j] >> (3 - e)) & 1) for j in range(6)) & 1 for e in range(4)]


HAMMING_ALL_COLUMNS = HAMMING_COLUMNS + (8, 4, 2, 1)


def hamming_decode(ten) -> tuple:
    """(the six data bits, flag): 0 clean, 1 a bit flipped, 2 unmatched."""
    bits = [int(b) for b in ten]
    syn = 0
    for j, b in enumerate(bits):
        if b:
            syn ^= HAMMING_ALL_COLUMNS[j]
    if syn == 0:
        return bits[:6], 0
    if syn in HAMMING_ALL_COLUMNS:
        bits[HAMMING_ALL_COLUMNS.index(syn)] ^= 1
        return bits[:6], 1
    return bits[:6], 2


def rs_generator() -> list:
    g = [1]
    for j in range(1, 13):
        g = poly_mul(g, [1, gf_pow(ALPHA, j)])
    return g


def rs_parity(twelve) -> list:
    """The twelve parity hexbits: the remainder of the data x^12 modulo the generator."""
    gen = rs_generator()
    work = list(twelve) + [0] * 12
    for i in range(12):
        lead = work[i]
        if lead:
            for j, g in enumerate(gen):
                work[i + j] ^= gf_mul(lead, g)
    return work[12:]


def rs_check(hexbits) -> bool:
    for j in range(1, 13):
        acc, a = 0, gf_pow(ALPHA, j)
        for h in hexbits:
            acc = gf_mul(acc, a) ^ int(h)
        if acc:
            return False
    return True


def crc_ccitt(data) -> int:
    crc = 0
    for byte in data:
        for i in range(7, -1, -1):
            top = ((crc >> 15) & 1) ^ ((byte >> i) & 1)
            crc = (crc << 1) & 0xFFFF
            if top:
                crc ^= 0x1021
    return crc


def trellis_encode(dibits48) -> list:
    """The 98 dibits as sent (interleaved) of 48 information dibits."""
    state, coded = 0, []
    for d in list(dibits48) + [0]:
        coded += TRELLIS_PAIRS[TRELLIS_POINTS[state][d]]
        state = d
    sent = [0] * 98
    for n, at in enumerate(INTERLEAVE):
        sent[at] = coded[n]
    return sent


def trellis_decode(sent98, smaller: bool = True) -> tuple:
    """(the 48 information dibits, the metric) of the 98 dibits as sent.  ``smaller``: the smaller predecessor wins on equal metric,
    as the specification has it; False is the other rule, by which the tests find a word on which the rule matters."""
    coded = [int(sent98[at]) for at in INTERLEAVE]
    metric = [0, FAR, FAR, FAR]
    back = []
    for t in range(49):
        rx = coded[2 * t] << 2 | coded[2 * t + 1]
        new, arg = [], []
        for j in range(4):
            costs = []
            for i in range(4):
                a, b = TRELLIS_PAIRS[TRELLIS_POINTS[i][j]]
                costs.append(metric[i] + bin(rx ^ (a << 2 | b)).count("1"))
            best = min(costs)
            new.append(best)
            arg.append(costs.index(best) if smaller else 3 - costs[::-1].index(best))
        metric = new
        back.append(arg)
    state, inputs = 0, []
    for t in range(48, -1, -1):
        inputs.append(state)
        state = back[t][state]
    inputs.reverse()
    return inputs[:48], metric[0]


# ---- the encoder --------------------------------------------------------------------------------------------------------------


def lc_hexbits(lco: int, src: int, dst: int, mfid: int = 0, svc: int = 0, break_rs: bool = False) -> list:
    """The 24 hexbits of a link control word of LCO 0 (group: dst the talkgroup) or 3 (unit to unit)."""
    if lco == 0:
        nine = [lco, mfid, svc, 0, dst >> 8 & 0xFF, dst & 0xFF, src >> 16 & 0xFF, src >> 8 & 0xFF, src & 0xFF]
    else:
        nine = [lco, mfid, svc, dst >> 16 & 0xFF, dst >> 8 & 0xFF, dst & 0xFF, src >> 16 & 0xFF, src >> 8 & 0xFF, src & 0xFF]
    bits = [b for byte in nine for b in word_bits(byte, 8)]
    data = [bits_word(bits[6 * j : 6 * j + 6]) for j in range(12)]
    parity = rs_parity(data)
    if break_rs:
        parity[0] ^= 0x15
    return data + parity


def tsbk_bytes(opcode: int, mfid: int, args: int, lb: int = 0, p: int = 0, break_crc: bool = False) -> list:
    ten = [lb << 7 | p << 6 | opcode, mfid] + [(args >> (56 - 8 * j)) & 0xFF for j in range(8)]
    crc = crc_ccitt(ten) ^ 0xFFFF ^ (1 if break_crc else 0)
    return ten + [crc >> 8, crc & 0xFF]


def tsbk_block_bits(by) -> list:
    """The 196 data bits of a block of twelve bytes."""
    bits = [b for byte in by for b in word_bits(byte, 8)]
    sent = trellis_encode([bits[2 * j] << 1 | bits[2 * j + 1] for j in range(48)])
    return [b for d in sent for b in (d >> 1, d & 1)]


def frame_data_bits(nac: int, duid: int, body, total_symbols: int) -> list:
    """The data bits of a frame of ``total_symbols`` symbols: sync, NID, ``body``, then zeros."""
    status = total_symbols // STATUS_EVERY
    bits = word_bits(SYNC, 48) + nid_bits(nac, duid) + [int(b) for b in body]
    room = 2 * (total_symbols - status)
    assert len(bits) <= room and total_symbols % STATUS_EVERY == 0
    return bits + [0] * (room - len(bits))


def frame_dibits(data_bits) -> list:
    """The frame's symbols as dibits: a status symbol behind every 35 data dibits."""
    out = []
    for q in range(len(data_bits) // 2):
        out.append(int(data_bits[2 * q]) << 1 | int(data_bits[2 * q + 1]))
        if len(out) % STATUS_EVERY == STATUS_EVERY - 1:
            out.append(STATUS_VALUE)
    return out


def ldu1_body(hexbits, rng) -> list:
    """The data bits 112 .. 1679 of an LDU1: seeded random bits with the 24 Hamming words of the link control in their places."""
    body = rng.integers(0, 2, 1680 - 112).tolist()
    for w, h in enumerate(hexbits):
        first = 400 + 184 * (w // 4) + 10 * (w % 4) - 112
        body[first : first + 10] = hamming_encode(word_bits(h, 6))
    return body


def tdulc_body(hexbits) -> list:
    bits = [b for h in hexbits for b in word_bits(h, 6)]
    return [b for w in range(12) for b in word_bits(GOLAY[bits_word(bits[12 * w : 12 * w + 12])], 24)]


def make_frame(item, nac: int, rng) -> list:
    """The dibits of one frame of a script: ("hdu",), ("ldu1", hexbits), ("ldu2",), ("tdu",), ("tdulc", hexbits), ("tsbk", [twelve
    bytes, ...]) with one or three blocks, ("raw", duid, body bits, symbols)."""
    kind = item[0]
    if kind == "hdu":
        return frame_dibits(frame_data_bits(nac, 0x0, rng.integers(0, 2, 770 - 112).tolist(), 396))
    if kind == "ldu1":
        return frame_dibits(frame_data_bits(nac, 0x5, ldu1_body(item[1], rng), 864))
    if kind == "ldu2":
        return frame_dibits(frame_data_bits(nac, 0xA, rng.integers(0, 2, 1680 - 112).tolist(), 864))
    if kind == "tdu":
        return frame_dibits(frame_data_bits(nac, 0x3, [], 72))
    if kind == "tdulc":
        return frame_dibits(frame_data_bits(nac, 0xF, tdulc_body(item[1]), 216))
    if kind == "tsbk":
        body = [b for by in item[1] for b in tsbk_block_bits(by)]
        return frame_dibits(frame_data_bits(nac, 0x7, body, 180 if len(item[1]) == 1 else 360))
    if kind == "raw":
        return frame_dibits(frame_data_bits(nac, item[1], item[2], item[3]))
    raise ValueError(item)


def station(script, nac: int = 0x293, seed: int = 5) -> list:
    """The symbol levels of a station that sends the frames of ``script`` one behind the other."""
    rng = np.random.default_rng(seed)
    return [LEVEL[d] for item in script for d in make_frame(item, nac, rng)]


def synth_theta(levels, fs_ch: float, n: int, start_s: float = 0.0, noise: float = 0.0, seed: int = 1) -> np.ndarray:
    """float32[n]: the discriminator output of the rectangular 4-level FSK of ``levels`` at 4800 symbols/s from ``start_s`` on, a
    level l deviating l 600 Hz, 0 elsewhere; ``noise``: the sigma of white Gaussian noise on theta, in radians."""
    f = np.zeros(n, dtype=np.float64)
    edges = start_s + np.arange(len(levels) + 1) / 4800.0
    idx = np.ceil(edges * fs_ch - 1e-9).astype(np.int64)
    for lev, a, b in zip(levels, idx[:-1], idx[1:]):
        f[max(a, 0) : max(min(b, n), 0)] = lev * DEV
    theta = 2.0 * np.pi * f / fs_ch
    if noise:
        theta = theta + noise * np.random.default_rng(seed).standard_normal(n)
    return theta.astype(np.float32)


# ---- the oracle: plan, frames, slicing ----------------------------------------------------------------------------------------------


def plan(fs_ch: float) -> dict:
    """sps, o[0 .. 863] and ``ident_model``'s plan at 4800; ValueError unless 4 <= sps <= 224."""
    ident = IM.plan(fs_ch, 4800)
    return dict(fs_ch=float(fs_ch), sps=ident["sps"], o=[int(round(i * ident["sps"])) for i in range(OFFSETS)], ident=ident)


def frame_hits(kept, h: int) -> list:
    """(m, s) in order of m from ``ident_model``'s kept hits over P25_PATTERNS (pattern 0)."""
    cand = [(m, abs(C), 1 if C > 0 else -1) for p, m, C, _E, _pre, _post in kept if p == 0 and C != 0]
    out = []
    for m, a, s in cand:
        if not any(m2 != m and abs(m2 - m) <= h and (a2 > a or (a2 == a and m2 < m)) for m2, a2, _ in cand):
            out.append((m, s))
    return sorted(out)


def slice_by_loops(v, n: int, m: int, s: int, pl: dict) -> tuple:
    """(the 54 words, [A, Dc, valid]) of one hit."""
    o = pl["o"]
    valid = 0 if m + o[0] < 0 else sum(1 for i in range(OFFSETS) if m + o[i] < n)
    if valid < 24:
        return [0] * WORDS, [0, 0, valid]
    sgn = [1 if g > 0 else -1 for g in sync_levels()]
    x = [int(v[m + o[i]]) for i in range(24)]
    p, q = sum(x), sum(g * xi for g, xi in zip(sgn, x))
    amp, dc = s * (12 * q + p), 12 * p + q
    bits = []
    for i in range(OFFSETS):
        if i >= valid:
            bits += [0, 0]
            continue
        d = s * (286 * int(v[m + o[i]]) - dc)
        bits += [1 if d < 0 else 0, 1 if 3 * abs(d) >= 2 * amp else 0]
    return [bits_word(bits[32 * w : 32 * w + 32]) for w in range(WORDS)], [amp, dc, valid]


def slice_all(v, rows, pl: dict) -> tuple:
    """(bits uint32[K][54], levels int64[K][3]) of ``rows`` (m, s), vectorised."""
    v = np.asarray(v, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    n, k = v.size, rows.shape[0]
    o = np.array(pl["o"], dtype=np.int64)
    at = rows[:, :1] + o[None, :]
    inside = (at < n) & (rows[:, :1] >= 0)
    valid = inside.sum(axis=1)
    read = valid >= 24
    y = np.where(inside, v[np.clip(at, 0, max(n - 1, 0))] if n else 0, 0)
    sgn = np.array([1 if g > 0 else -1 for g in sync_levels()], dtype=np.int64)
    p, q = y[:, :24].sum(axis=1), (y[:, :24] * sgn).sum(axis=1)
    amp, dc = np.where(read, rows[:, 1] * (12 * q + p), 0), np.where(read, 12 * p + q, 0)
    d = rows[:, 1:2] * (286 * y - dc[:, None])
    on = inside & read[:, None]
    two = np.stack([(d < 0) & on, (3 * np.abs(d) >= 2 * amp[:, None]) & on], axis=2).reshape(k, 2 * OFFSETS).astype(np.uint64)
    weights = (1 << np.arange(31, -1, -1)).astype(np.uint64)
    bits = (two.reshape(k, WORDS, 32) * weights).sum(axis=2).astype(np.uint32)
    return bits, np.stack([amp, dc, valid], axis=1).astype(np.int64)


# ---- the oracle: one frame's coders -------------------------------------------------------------------------------------------------


def record_bits(words) -> list:
    return [b for w in words for b in word_bits(int(w), 32)]


def data_bits_of(words) -> list:
    """The data bits of a record: the status symbols left out."""
    bits = record_bits(words)
    return [bits[2 * i + k] for i in range(OFFSETS) if i % STATUS_EVERY != STATUS_EVERY - 1 for k in (0, 1)]


def words_of_dibits(dibits) -> list:
    """The 54 words of a frame's symbols as dibits, zeros behind them."""
    bits = [b for d in list(dibits)[:OFFSETS] for b in (d >> 1, d & 1)]
    bits += [0] * (2 * OFFSETS - len(bits))
    return [bits_word(bits[32 * w : 32 * w + 32]) for w in range(WORDS)]


def nid_all(bits) -> np.ndarray:
    """int32[K][4] of ``iqa_p25_nid``."""
    return np.array([nid_decode(data_bits_of(w)[48:112]) for w in np.asarray(bits).tolist()], dtype=np.int32).reshape(-1, 4)


def decode_frame(words, duid: int) -> tuple:
    """(info, rec): the nine information words and the eight values of one sliced frame, as ``iqa_p25_decode`` gives them."""
    data = data_bits_of(words)
    out, rec = [0] * 288, [0] * 8
    if duid == 0xF:
        rec[0] = 2
        for w in range(12):
            word = bits_word(data[112 + 24 * w : 136 + 24 * w])
            dist, value, refused = golay_decode(word)
            out[12 * w : 12 * w + 12] = word_bits(value, 12)
            if refused:
                rec[2] += 1
            elif dist:
                rec[1] += 1
                rec[3] += dist
    elif duid == 0x5:
        rec[0] = 1
        for w in range(24):
            first = 400 + 184 * (w // 4) + 10 * (w % 4)
            six, flag = hamming_decode(data[first : first + 10])
            out[6 * w : 6 * w + 6] = six
            rec[1] += flag == 1
            rec[2] += flag == 2
        rec[3] = rec[1]
    elif duid == 0x7:
        rec[0] = 3
        for b in range(3):
            first = 112 + 196 * b
            sent = [data[first + 2 * j] << 1 | data[first + 2 * j + 1] for j in range(98)]
            dibits, metric = trellis_decode(sent)
            out[96 * b : 96 * b + 96] = [x for d in dibits for x in (d >> 1, d & 1)]
            rec[1 + b] = metric
    return [bits_word(out[32 * w : 32 * w + 32]) for w in range(9)], rec


def decode_all(bits, duids) -> tuple:
    """(info uint32[K][9], rec int32[K][8])."""
    out = [decode_frame(w, int(d)) for w, d in zip(np.asarray(bits).tolist(), np.asarray(duids).tolist())]
    return (np.array([o[0] for o in out], dtype=np.uint32).reshape(-1, 9), np.array([o[1] for o in out], dtype=np.int32).reshape(-1, 8))


def apply_flags(nid, levels) -> np.ndarray:
    nid = np.array(nid, dtype=np.int32).reshape(-1, 4)
    for j, lev in enumerate(np.asarray(levels).tolist()):
        if lev[2] < NEED_NID:
            nid[j, 0] = 3
    return nid


def decoder_duids(nid) -> list:
    return [int(r[2]) & 15 if r[0] <= 1 else 0 for r in np.asarray(nid).tolist()]


# ---- the oracle: checks, fields, calls, blocks --------------------------------------------------------------------------------------


def info_hexbits(words) -> list:
    bits = record_bits(words[:5])
    return [bits_word(bits[6 * j : 6 * j + 6]) for j in range(24)]


def info_bytes(words) -> list:
    return [(int(w) >> sh) & 0xFF for w in words for sh in (24, 16, 8, 0)]


def check_tsbk(by) -> bool:
    return (crc_ccitt(by[:10]) ^ 0xFFFF) == (by[10] << 8 | by[11])


def parse(rows, levels, nid, info, rec, fs_ch: float, start: int = 0) -> tuple:
    """(frames, counts): a dict per frame whose NID was read, in order of time."""
    counts = dict(no_level=0, cut=0, nid_refused=0, nid_fixed=0, lc_failed=0, crc_failed=0, golay_refused=0, hamming_unmatched=0)
    out = []
    for (m, _s), lev, r4, words, r in zip(np.asarray(rows).tolist(), np.asarray(levels).tolist(), np.asarray(nid).tolist(),
                                         np.asarray(info).tolist(), np.asarray(rec).tolist()):
        if r4[0] == 3:
            counts["cut"] += 1
            continue
        if lev[0] <= 0:
            counts["no_level"] += 1
            continue
        if r4[0] == 2:
            counts["nid_refused"] += 1
            continue
        counts["nid_fixed"] += r4[0] == 1
        duid = r4[2] & 15
        f = dict(time_s=(start + m) / fs_ch, nac=r4[2] >> 4, duid=duid, name=DUIDS.get(duid, "reserved"), corrected=r4[0] == 1, checked=None,
                 lco=None, mfid=None, src=None, dst=None, hex=None, blocks=[])
        if duid in (0x5, 0xF):
            if lev[2] < (NEED_LDU1 if duid == 0x5 else NEED_TDULC):
                counts["cut"] += 1
            else:
                counts["hamming_unmatched" if duid == 0x5 else "golay_refused"] += r[2]
                hexbits = info_hexbits(words)
                f["checked"] = rs_check(hexbits)
                f["corrected"] = f["corrected"] or r[1] > 0
                if f["checked"]:
                    by = info_bytes(words)[:9]
                    f.update(lco=by[0] & 63, mfid=by[1], hex=bytes(by).hex())
                    if f["lco"] == 0:
                        f.update(dst=by[4] << 8 | by[5], src=by[6] << 16 | by[7] << 8 | by[8])
                    elif f["lco"] == 3:
                        f.update(dst=by[3] << 16 | by[4] << 8 | by[5], src=by[6] << 16 | by[7] << 8 | by[8])
                else:
                    counts["lc_failed"] += 1
        elif duid == 0x7:
            for b in range(3):
                if lev[2] < NEED_TSBK[b]:
                    counts["cut"] += 1
                    break
                by = info_bytes(words[3 * b : 3 * b + 3])
                ok = check_tsbk(by)
                counts["crc_failed"] += not ok
                f["blocks"].append([bytes(by).hex(), ok])
                f["corrected"] = f["corrected"] or r[1 + b] > 0
                if by[0] & 0x80:
                    break
        out.append(f)
    return sorted(out, key=lambda f: f["time_s"]), counts


def track(frames) -> list:
    """The calls as dicts, in order of their start."""
    calls, cur, last = [], None, 0.0
    for f in frames:
        if f["duid"] not in (0x0, 0x5, 0xA, 0x3, 0xF):
            continue
        if cur is not None and f["time_s"] - last > HANG_S:
            cur = None
        last = f["time_s"]

        def new():
            call = dict(start_s=f["time_s"], end_s=f["time_s"], nac=f["nac"], group=None, src=None, dst=None, ldus=0, terminated=False)
            calls.append(call)
            return call

        if cur is None and f["duid"] in (0x0, 0x5, 0xA):
            cur = new()
        if cur is not None and f["checked"] and f["lco"] in (0, 3):
            who = dict(group=f["lco"] == 0, src=f["src"], dst=f["dst"])
            if cur["group"] is not None and {k: cur[k] for k in who} != who:
                cur = new()
            cur.update(who)
        if cur is None:
            continue
        cur["end_s"] = f["time_s"]
        if f["duid"] in (0x5, 0xA):
            cur["ldus"] += 1
        elif f["duid"] in (0x3, 0xF):
            cur["terminated"] = True
            cur = None
    return calls


def tsbk_text(opcode: int, mfid: int, a: int, idens: dict) -> str:
    def ch(c):
        if c >> 12 not in idens:
            return f"ch 0x{c:04x}"
        base, spacing = idens[c >> 12]
        return f"ch 0x{c:04x} ({(base * 5 + (c & 0xFFF) * spacing * 125) / 1e6:.4f} MHz)"

    if mfid == 0 and opcode == 0x00:
        return f"group grant tg {a >> 24 & 0xFFFF} src {a & 0xFFFFFF} {ch(a >> 40 & 0xFFFF)}"
    if mfid == 0 and opcode == 0x02:
        return f"grant update tg {a >> 32 & 0xFFFF} {ch(a >> 48)}, tg {a & 0xFFFF} {ch(a >> 16 & 0xFFFF)}"
    if mfid == 0 and opcode == 0x3A:
        return f"rfss status system 0x{a >> 40 & 0xFFF:03x} rfss {a >> 32 & 0xFF} site {a >> 24 & 0xFF} {ch(a >> 8 & 0xFFFF)}"
    if mfid == 0 and opcode == 0x3B:
        return f"network status wacn 0x{a >> 36 & 0xFFFFF:05x} system 0x{a >> 24 & 0xFFF:03x} {ch(a >> 8 & 0xFFFF)}"
    if mfid == 0 and opcode == 0x3D:
        return f"identifier update id {a >> 60} base {(a & 0xFFFFFFFF) * 5 / 1e6:.4f} MHz spacing {(a >> 32 & 0x3FF) * 0.125:g} kHz"
    return f"o=0x{opcode:02x} mfid=0x{mfid:02x} {a:016x}"


def collapse(frames) -> list:
    """The distinct blocks whose CRC held as dicts, in order of their first time."""
    seen, idens = {}, {}
    for f in frames:
        for text, ok in f["blocks"]:
            if not ok:
                continue
            by = bytes.fromhex(text)
            key = (by[0] & 63, by[1], int.from_bytes(by[2:10], "big"))
            if key[:2] == (0x3D, 0):
                idens.setdefault(key[2] >> 60, (key[2] & 0xFFFFFFFF, key[2] >> 32 & 0x3FF))
            if key in seen:
                seen[key]["count"] += 1
                seen[key]["last_s"] = f["time_s"]
            else:
                seen[key] = dict(opcode=key[0], mfid=key[1], args=f"{key[2]:016x}", nac=f["nac"], count=1, first_s=f["time_s"],
                                 last_s=f["time_s"], text="")
    for key, t in seen.items():
        t["text"] = tsbk_text(*key, idens)
    return list(seen.values())


def decode_plane(v, kept, pl: dict, start: int = 0) -> dict:
    """The whole oracle behind the sync search on one integrated plane."""
    rows = np.array(frame_hits(kept, pl["ident"]["h"]), dtype=np.int64).reshape(-1, 2)
    bits, levels = slice_all(v, rows, pl)
    nid = apply_flags(nid_all(bits), levels)
    info, rec = decode_all(bits, decoder_duids(nid))
    frames, counts = parse(rows, levels, nid, info, rec, pl["fs_ch"], start)
    return dict(rows=rows, bits=bits, levels=levels, nid=nid, info=info, rec=rec, frames=frames, counts=counts, calls=track(frames),
                tsbks=collapse(frames))


def decode_theta(theta, fs_ch: float, c: int = 0) -> dict:
    pl = plan(fs_ch)
    v = IM.integrate(theta, c, pl["ident"]["L"], pl["ident"]["sh"])
    _, kept = IM.search(v, pl["ident"], P25_PATTERNS)
    out = decode_plane(v, kept, pl)
    out.update(v=v, kept=kept, plan=pl)
    return out


# ---- the test stream and the model capture ---------------------------------------------------------------------------------------

NAC, SRC, TG = 0x293, 2345678, 9
WACN, SYSTEM, RFSS, SITE = 0xBEE00, 0x293, 1, 2
IDEN = 1 << 60 | 100 << 51 | 180 << 42 | 100 << 32 | 169_952_500  # id 1: base 849.7625 MHz, 12.5 kHz steps
CONTROL, VOICE = 0x1001, 0x1064  # channels 1 and 100 of id 1: 849.7750 and 851.0125 MHz
NET = 0 << 56 | WACN << 36 | SYSTEM << 24 | CONTROL << 8 | 0x70
RFSS_ARGS = 0 << 56 | 0 << 52 | SYSTEM << 40 | RFSS << 32 | SITE << 24 | CONTROL << 8 | 0x70
GRANT = 0 << 56 | VOICE << 40 | TG << 24 | SRC
OTHER = 0x0123456789ABCDEF
LC = lc_hexbits(0, SRC, TG)
TSBK_ONE = ("tsbk", [tsbk_bytes(0x3D, 0, IDEN, lb=1)])
TSBK_THREE = ("tsbk", [tsbk_bytes(0x3B, 0, NET), tsbk_bytes(0x3A, 0, RFSS_ARGS), tsbk_bytes(0x00, 0, GRANT, lb=1)])
TSBK_OTHER = ("tsbk", [tsbk_bytes(0x29, 0x90, OTHER, lb=1)])
#: a call of four LDUs with its header and its terminator, then a stretch of a control channel that repeats itself
SCRIPT = ([("hdu",), ("ldu1", LC), ("ldu2",), ("ldu1", LC), ("ldu2",), ("tdulc", LC)]
          + [TSBK_ONE, TSBK_THREE, TSBK_THREE, TSBK_OTHER, TSBK_THREE, TSBK_OTHER])
STREAM_START = 0.02


def test_stream(fs_ch: float, noise: float = 0.0, seed: int = 3, script=SCRIPT, negate: bool = False) -> np.ndarray:
    levels = station(script)
    n = int((STREAM_START + len(levels) / 4800.0 + 0.02) * fs_ch)
    theta = synth_theta(levels, fs_ch, n, STREAM_START, noise, seed)
    return -theta if negate else theta


FS, SECS, AMP = IM.FS, IM.SECS, IM.AMP
CAPTURE_START = 0.0  # the station is on the air from the first sample: a silent lead would key the channel on noise crossings alone
CAPTURE_CHANNELS = (("p25", 200e3), ("voice", 600e3))


def capture_script() -> list:
    """One three-block frame of the control channel (the channel filter settles in it), SCRIPT, then that frame until the capture
    ends."""
    have = len(station([TSBK_THREE] + list(SCRIPT)))
    room = int((SECS - CAPTURE_START) * 4800.0) + 1 - have
    return [TSBK_THREE] + list(SCRIPT) + [TSBK_THREE] * (room // 360 + 1)


@functools.lru_cache(maxsize=1)
def capture() -> np.ndarray:
    """int16[n][2]: a model capture in ``ident_model``'s conventions (s16, 2.4 MS/s, 2 s, AMP 0.05, complex noise 30 dB under AMP
    in total, seed 11, DC 0.01): a P25 channel at +200 kHz that sends ``capture_script()``, and an NFM voice channel at +600 kHz."""
    n = int(round(FS * SECS))
    t = np.arange(n) / FS
    rng = np.random.default_rng(11)
    sigma = AMP * 10.0 ** (-30.0 / 20.0) / math.sqrt(2.0)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    off = dict(CAPTURE_CHANNELS)
    car = lambda name: np.exp(2j * np.pi * ((off[name] * t) % 1.0))  # noqa: E731
    levels = station(capture_script())
    f = np.zeros(n, dtype=np.float64)
    idx = np.ceil((CAPTURE_START + np.arange(len(levels) + 1) / 4800.0) * FS - 1e-9).astype(np.int64)
    for lev, a, b in zip(levels, idx[:-1], idx[1:]):
        f[max(a, 0) : max(min(b, n), 0)] = lev * DEV
    x += (AMP / 2.0) * car("p25") * K._fm_of(f)
    x += (AMP / 2.0) * car("voice") * K._fm_of(2500.0 * M.voice(1, n))
    x += 0.01
    out = np.empty((n, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real * 32768.0), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag * 32768.0), -32768, 32767)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=1)
def model_run() -> list:
    """The whole oracle on the model capture: the numpy finder, the float64 channelizer, section 23's keying and label, section
    25's identification and this section's frames, calls and blocks, per found channel."""
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
        p25 = None
        if named["rate"] == 4800 and named["plan"] is not None:
            pl = plan(d["plan"]["fs_ch"])
            p25 = decode_plane(named["v"], [(0,) + tuple(h[1:]) for h in named["kept"] if IM.family(4800)[h[0]][0] == "p25"], pl, k["keyed_from"])
        out.append(dict(described=d, keyed=k, named=named, p25=p25))
    return out


# ---- crafted words for the coders (the host test and the GPU shapes test share them) -----------------------------------------------


def flipped_words(words, frame_bits) -> list:
    """``words`` with the frame bits ``frame_bits`` flipped."""
    out = [int(w) for w in words]
    for b in frame_bits:
        out[b >> 5] ^= 1 << (31 - (b & 31))
    return out


def frame_bit_of(data_bit: int) -> int:
    """The frame bit of a data bit."""
    return 2 * symbol_of(data_bit >> 1) + (data_bit & 1)


@functools.lru_cache(maxsize=1)
def nid_cases() -> dict:
    """name -> the 54 words: a TDU's NID clean, with every single flip of its 63 code bits and of its parity bit, with eleven flips,
    and with twelve flips that land on another codeword (the first seed that does) and that are refused (the first that are)."""
    rng = np.random.default_rng(1)
    clean = words_of_dibits(make_frame(("tdu",), NAC, rng))
    at = [frame_bit_of(48 + j) for j in range(64)]
    out = {"clean": clean}
    for j in range(64):
        out[f"single-{j}"] = flipped_words(clean, [at[j]])
    out["eleven"] = flipped_words(clean, [at[j] for j in (0, 5, 11, 17, 23, 29, 35, 41, 47, 53, 62)])
    for seed in range(4000):
        if "twelve-other" in out and "twelve-refused" in out:
            break
        pick = np.random.default_rng(seed).choice(63, 12, replace=False).tolist()
        words = flipped_words(clean, [at[j] for j in pick])
        status, _dist, value, _ = nid_decode(data_bits_of(words)[48:112])
        if status == 1 and value != (NAC << 4 | 3):
            out.setdefault("twelve-other", words)
        elif status == 2:
            out.setdefault("twelve-refused", words)
    out["zeros"] = [0] * WORDS
    out["ones"] = [0xFFFFFFFF] * WORDS
    return out


@functools.lru_cache(maxsize=1)
def tie_flips() -> tuple:
    """The first three channel bits of TSBK_THREE's first block (in order of the triples) whose flips make the tie rule matter: the
    two rules give different information dibits."""
    sent = trellis_encode([b[0] << 1 | b[1] for b in zip(*[iter([x for byte in TSBK_THREE[1][0] for x in word_bits(byte, 8)])] * 2)])
    for a in range(0, 196):
        for b in range(a + 1, min(a + 12, 196)):
            for c in range(b + 1, min(b + 12, 196)):
                bad = list(sent)
                for k in (a, b, c):
                    bad[k >> 1] ^= 2 >> (k & 1)
                if trellis_decode(bad)[0] != trellis_decode(bad, smaller=False)[0]:
                    return (a, b, c)
    raise AssertionError("no tie found")


@functools.lru_cache(maxsize=1)
def coder_cases() -> dict:
    """name -> (the 54 words, DUID): the crafted frames of the coder tests."""
    rng = np.random.default_rng(2)
    tdulc = words_of_dibits(make_frame(("tdulc", LC), NAC, rng))
    ldu1 = words_of_dibits(make_frame(("ldu1", lc_hexbits(3, 111, 222)), NAC, rng))
    tsbk = words_of_dibits(make_frame(TSBK_THREE, NAC, rng))
    out = {"tdulc": (tdulc, 0xF), "ldu1": (ldu1, 0x5), "tsbk": (tsbk, 0x7)}
    g = lambda w, k: frame_bit_of(112 + 24 * w + k)  # noqa: E731
    out["golay-single"] = (flipped_words(tdulc, [g(w, (5 * w) % 24) for w in range(12)]), 0xF)
    out["golay-double"] = (flipped_words(tdulc, [g(0, 0), g(0, 23), g(7, 3), g(7, 12)]), 0xF)
    out["golay-triple"] = (flipped_words(tdulc, [g(3, 1), g(3, 9), g(3, 20), g(11, 0), g(11, 11), g(11, 23)]), 0xF)
    out["golay-four"] = (flipped_words(tdulc, [g(5, 2), g(5, 7), g(5, 13), g(5, 19)]), 0xF)
    h = lambda w, k: frame_bit_of(400 + 184 * (w // 4) + 10 * (w % 4) + k)  # noqa: E731
    for k in range(10):
        out[f"hamming-{k}"] = (flipped_words(ldu1, [h(w, k) for w in range(0, 24, 3)]), 0x5)
    # the five syndromes that name no bit: 1111 = 1110 ^ 0001, 1010 = 1000 ^ 0010, 1001 = 1000 ^ 0001, 0110 = 0100 ^ 0010, 0101 = 0100 ^ 0001
    for name, (a, b), w in (("1111", (0, 9), 1), ("1010", (6, 8), 6), ("1001", (6, 9), 11), ("0110", (7, 8), 16), ("0101", (7, 9), 21)):
        out[f"unmatched-{name}"] = (flipped_words(ldu1, [h(w, a), h(w, b)]), 0x5)
    t = lambda b, k: frame_bit_of(112 + 196 * b + k)  # noqa: E731
    for k in range(0, 196, 7):
        out[f"trellis-{k}"] = (flipped_words(tsbk, [t(0, k), t(1, (k + 50) % 196), t(2, (k + 101) % 196)]), 0x7)
    out["trellis-tie"] = (flipped_words(tsbk, [t(0, k) for k in tie_flips()]), 0x7)
    out["trellis-burst"] = (flipped_words(tsbk, [t(1, k) for k in range(40, 48)]), 0x7)
    for duid in (0x0, 0x3, 0xA, 0xC, 0x1, 0x9):
        out[f"other-{duid:x}"] = (ldu1, duid)
    out["zeros-f"], out["ones-f"] = ([0] * WORDS, 0xF), ([0xFFFFFFFF] * WORDS, 0xF)
    out["zeros-5"], out["ones-5"] = ([0] * WORDS, 0x5), ([0xFFFFFFFF] * WORDS, 0x5)
    out["zeros-7"], out["ones-7"] = ([0] * WORDS, 0x7), ([0xFFFFFFFF] * WORDS, 0x7)
    return out
