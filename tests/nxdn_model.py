"""Numpy model and encoder of the NXDN frame decoding (--find-nxdn), written from the specification with
its own copy of every constant.  Of the package it uses nothing; the quantiser, the integrator and the sync search are
``ident_model``'s.  The encoder goes from the LICH fields and the layer-3 octets through the CRC, the convolutional code, the
puncturing, the interleave and the scrambler to the 192 symbols of a frame, then to a rectangular 4-level FSK theta at 4800 or
2400 symbols/s.  The decoder is plain loops, one function per step: the levels, the slicing and the descrambling, the Viterbi
decoder over the depunctured bits with the stated tie rule and its opposite, the records; then the host rules (LICH, checks,
superframes, messages, calls, control lines) as dicts.  Also the model capture of the CLI test: one NXDN channel and a voice
channel."""
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

FSW = 0xCDF59
FSW_SYMBOLS = 10
LEVEL = {0b01: 3, 0b00: 1, 0b10: -1, 0b11: -3}
DIBIT = {v: k for k, v in LEVEL.items()}
NXDN_PATTERNS = [p for p in IM.PATTERNS if p[0] == "nxdn"]
OFFSETS, WORDS, INFO, RECORD = 192, 12, 14, 4
SCALE = 370
FAR = 1000
HANG_S = 0.360
DEV = 900.0  # a level of +-1 / +-3 deviates +-900 / +-2700 Hz
NEED_LICH, NEED_FRAME = 18, 192
SACCH, FACCH1_A, FACCH1_B, CAC = 1, 2, 4, 8
MASK_BYTES = bytes.fromhex("00000082A0888A00A2A8828A820220088A20AAA28208228AAA0828882828000A02822028822AAA202280A88A08A0AA02")
#: kind -> (steps, the punctured j mod period, the period, D, C, the first frame bit of the block (FACCH1: of its first half))
BLOCKS = {"sacch": (36, (5,), 6, 12, 5, 36), "facch1": (96, (1,), 4, 9, 16, 96), "cac": (175, (3, 11), 14, 12, 25, 36)}
#: kind -> (width, polynomial, initial value, the bits in front of the CRC)
CRC = {"sacch": (6, 0x27, 0x3F, 26), "facch1": (12, 0x80F, 0xFFF, 80), "cac": (16, 0x1021, 0xFFFF, 155)}
NAMES = {0x01: "VCALL", 0x03: "VCALL_IV", 0x04: "VCALL_ASSGN", 0x08: "TX_REL", 0x09: "DCALL_HDR", 0x0B: "DCALL_DATA", 0x0C: "DCALL_ACK",
         0x0E: "DCALL_ASSGN", 0x10: "IDLE", 0x11: "DISC", 0x17: "DST_ID_INFO", 0x18: "SITE_INFO", 0x19: "SRV_INFO", 0x1A: "CCH_INFO",
         0x1B: "ADJ_SITE_INFO", 0x20: "REG_RESP"}
CALL_TYPES = {0: "broadcast", 1: "group", 4: "individual", 6: "interconnect"}
RF_NAMES = ("RCCH", "RTCH", "RDCH", "RTCH-C")
FN_NAMES = (("outbound", "long inbound", "2", "short inbound"), ("non-superframe", "UDCH", "superframe", "idle"))


def word_bits(word: int, n: int) -> list:
    return [(word >> (n - 1 - i)) & 1 for i in range(n)]


def bits_word(bits) -> int:
    out = 0
    for b in bits:
        out = out << 1 | int(b)
    return out


def bytes_bits(data) -> list:
    return [b for byte in data for b in word_bits(int(byte), 8)]


def bits_bytes(bits) -> list:
    return [bits_word(bits[8 * j : 8 * j + 8]) for j in range(len(bits) // 8)]


def fsw_levels() -> list:
    return [LEVEL[(FSW >> (2 * (FSW_SYMBOLS - 1 - i))) & 3] for i in range(FSW_SYMBOLS)]


# ---- the codes ----------------------------------------------------------------------------------------------------------------


def pn(count: int = OFFSETS - FSW_SYMBOLS) -> list:
    """The scrambler: 0 0 1 0 0 1 1 1 0, then b[n] = b[n - 5] ^ b[n - 9]; bit k belongs to symbol 10 + k."""
    b = [0, 0, 1, 0, 0, 1, 1, 1, 0]
    for n in range(9, count):
        b.append(b[n - 5] ^ b[n - 9])
    return b[:count]


def scramble_mask() -> list:
    """The scrambler as the 384 frame bits it inverts: the first bit of every symbol whose scrambler bit is 1."""
    out = [0] * (2 * OFFSETS)
    for k, bit in enumerate(pn()):
        out[2 * (FSW_SYMBOLS + k)] = bit
    return out


def crc(bits, kind: str) -> int:
    """MSB first, no final inversion."""
    width, poly, reg, _ = CRC[kind]
    for bit in bits:
        top = (reg >> (width - 1)) & 1
        reg = (reg << 1) & ((1 << width) - 1)
        if top ^ int(bit):
            reg ^= poly
    return reg


def conv_encode(bits) -> list:
    """The coded bits of ``bits`` and four zero tail bits: g1 = d ^ d3 ^ d4 at 2 t, g2 = d ^ d1 ^ d2 ^ d4 at 2 t + 1."""
    d1 = d2 = d3 = d4 = 0
    out = []
    for d in list(bits) + [0, 0, 0, 0]:
        out += [d ^ d3 ^ d4, d ^ d1 ^ d2 ^ d4]
        d1, d2, d3, d4 = d, d1, d2, d3
    return out


def punctured(j: int, kind: str) -> bool:
    _, where, period, _, _, _ = BLOCKS[kind]
    return j % period in where


def channel_index(p: int, kind: str) -> int:
    """The channel bit of the p-th coded bit that is sent."""
    _, _, _, depth, cols, _ = BLOCKS[kind]
    return cols * (p % depth) + p // depth


def to_channel(coded, kind: str) -> list:
    """The channel bits of a block's coded bits: punctured, then interleaved."""
    sent = [c for j, c in enumerate(coded) if not punctured(j, kind)]
    out = [0] * len(sent)
    for p, c in enumerate(sent):
        out[channel_index(p, kind)] = c
    return out


def from_channel(channel, kind: str) -> list:
    """The coded bits of a block's channel bits, None where one was punctured."""
    out, p = [], 0
    for j in range(2 * BLOCKS[kind][0]):
        if punctured(j, kind):
            out.append(None)
        else:
            out.append(channel[channel_index(p, kind)])
            p += 1
    return out


def viterbi(coded, smaller: bool = True) -> tuple:
    """(the decoded bits with the tail, the metric, the ties on the surviving path) of the coded bits of one block (None: a
    punctured bit, which costs nothing on either branch): sixteen states d1 d2 d3 d4 (d1 the top bit), from state 0 to state
    0, Hamming metric.  ``smaller``: on equal metrics the predecessor with the smaller state index survives, as the
    specification has it; False is the other rule."""
    steps = len(coded) // 2
    metric = [0] + [FAR] * 15
    back, tied = [], []
    for t in range(steps):
        rx = (coded[2 * t], coded[2 * t + 1])
        new, arg, tie = [], [], []
        for state in range(16):
            d = state >> 3
            cost = []
            for prev in ((state & 7) << 1, (state & 7) << 1 | 1):
                d1, d2, d3, d4 = prev >> 3 & 1, prev >> 2 & 1, prev >> 1 & 1, prev & 1
                sent = (d ^ d3 ^ d4, d ^ d1 ^ d2 ^ d4)
                cost.append(metric[prev] + sum(1 for r, s in zip(rx, sent) if r is not None and r != s))
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


def lich_byte(rf: int, fn: int, option: int = 0, outbound: int = 1, break_parity: bool = False) -> int:
    top = rf << 6 | fn << 4
    parity = (top >> 7 ^ top >> 6 ^ top >> 5 ^ top >> 4) & 1
    return top | option << 2 | outbound << 1 | (parity ^ (1 if break_parity else 0))


def block_channel_bits(info, kind: str, break_crc: bool = False) -> list:
    """The channel bits of the information bits of one block: its CRC behind them, coded, punctured, interleaved."""
    width, _, _, covered = CRC[kind]
    assert len(info) == covered
    check = crc(info, kind) ^ (1 if break_crc else 0)
    return to_channel(conv_encode(list(info) + word_bits(check, width)), kind)


def sacch_info(structure: int, ran: int, data18) -> list:
    return word_bits(structure, 2) + word_bits(ran, 6) + list(data18)


def cac_info(structure: int, ran: int, octets) -> list:
    return word_bits(structure, 2) + word_bits(ran, 6) + bytes_bits(list(octets) + [0] * (18 - len(octets))) + [0, 0, 0]


def vcall(kind: int = 0x01, src: int = 1234, dst: int = 5678, call_type: int = 1, emergency: int = 0, mode: int = 2, cipher: int = 0, key: int = 0,
          size: int = 10) -> list:
    """The octets of a VCALL (or, with ``kind`` 0x08, a TX_REL)."""
    out = [kind, emergency << 7, call_type << 5 | mode, src >> 8, src & 0xFF, dst >> 8, dst & 0xFF, cipher << 6 | key, 0, 0]
    return out[:size]


def make_frame(item: dict, rng) -> list:
    """The 192 dibits of one frame: ``lich`` (the byte), ``sacch`` (structure, RAN, 18 data bits), ``fa`` / ``fb`` (ten octets of a
    FACCH1 half), ``cac`` (structure, RAN, octets), ``inner`` (a LICH symbol sent as an inner level), ``break`` (the names of
    the blocks whose CRC is spoiled); what is not given is seeded random bits, as the voice is."""
    bits = word_bits(FSW, 20) + [b for k, bit in enumerate(word_bits(item["lich"], 8)) for b in (bit, 0 if item.get("inner") == k else 1)]
    bits += rng.integers(0, 2, 348).tolist()
    spoil = item.get("break", ())
    if item.get("cac") is not None:
        bits[36:336] = block_channel_bits(cac_info(*item["cac"]), "cac", "cac" in spoil)
    if item.get("sacch") is not None:
        bits[36:96] = block_channel_bits(sacch_info(*item["sacch"]), "sacch", "sacch" in spoil)
    for name, at in (("fa", 96), ("fb", 240)):
        if item.get(name) is not None:
            bits[at : at + 144] = block_channel_bits(bytes_bits(item[name]), "facch1", name in spoil)
    assert len(bits) == 2 * OFFSETS
    sent = [b ^ m for b, m in zip(bits, scramble_mask())]
    return [sent[2 * i] << 1 | sent[2 * i + 1] for i in range(OFFSETS)]


def station(script, seed: int = 5) -> list:
    """The symbol levels of a station that sends the frames of ``script`` one behind the other; ("random", count) is ``count``
    seeded random symbols without a sync word."""
    rng = np.random.default_rng(seed)
    out = []
    for item in script:
        if isinstance(item, tuple):
            out += (2 * rng.integers(0, 4, item[1]) - 3).tolist()
        else:
            out += [LEVEL[d] for d in make_frame(item, rng)]
    return out


def synth_theta(levels, fs_ch: float, n: int, start_s: float = 0.0, noise: float = 0.0, seed: int = 1, rate: int = 4800) -> np.ndarray:
    """float32[n]: the discriminator output of the rectangular 4-level FSK of ``levels`` at ``rate`` symbols/s from ``start_s`` on,
    a level l deviating l 900 Hz, 0 elsewhere; ``noise``: the sigma of white Gaussian noise on theta, in radians."""
    f = np.zeros(n, dtype=np.float64)
    edges = start_s + np.arange(len(levels) + 1) / float(rate)
    idx = np.ceil(edges * fs_ch - 1e-9).astype(np.int64)
    for lev, a, b in zip(levels, idx[:-1], idx[1:]):
        f[max(a, 0) : max(min(b, n), 0)] = lev * DEV
    theta = 2.0 * np.pi * f / fs_ch
    if noise:
        theta = theta + noise * np.random.default_rng(seed).standard_normal(n)
    return theta.astype(np.float32)


# ---- the decoder: plan, hits, levels, slicing ----------------------------------------------------------------------------------


def plan(fs_ch: float, rate: int = 4800) -> dict:
    """sps, o[0 .. 191] and ``ident_model``'s plan at ``rate``; ValueError unless the rate is 4800 or 2400 and 4 <= sps <= 224."""
    if rate not in (4800, 2400):
        raise ValueError("no NXDN rate")
    ident = IM.plan(fs_ch, rate)
    return dict(fs_ch=float(fs_ch), rate=rate, sps=ident["sps"], o=[int(round(i * ident["sps"])) for i in range(OFFSETS)], ident=ident)


def frame_hits(kept, h: int) -> list:
    """(m, s) in order of m from ``ident_model``'s kept hits over NXDN_PATTERNS (pattern 0)."""
    cand = [(m, abs(C), 1 if C > 0 else -1) for p, m, C, _E, _pre, _post in kept if p == 0 and C != 0]
    out = []
    for m, a, s in cand:
        if not any(m2 != m and abs(m2 - m) <= h and (a2 > a or (a2 == a and m2 < m)) for m2, a2, _ in cand):
            out.append((m, s))
    return sorted(out)


def levels_of(x, s: int) -> tuple:
    """(A, Dc) of the ten plane values under the frame sync word."""
    p, q = sum(x), sum(g * xi for g, xi in zip(fsw_levels(), x))
    return s * 15 * q, 37 * p


def slice_by_loops(v, n: int, m: int, s: int, pl: dict) -> tuple:
    """(the 12 words, descrambled, [A, Dc, valid]) of one hit."""
    o = pl["o"]
    valid = 0 if m + o[0] < 0 else sum(1 for i in range(OFFSETS) if m + o[i] < n)
    if valid < FSW_SYMBOLS:
        return [0] * WORDS, [0, 0, valid]
    amp, dc = levels_of([int(v[m + o[i]]) for i in range(FSW_SYMBOLS)], s)
    mask = scramble_mask()
    bits = []
    for i in range(OFFSETS):
        if i >= valid:
            bits += [0, 0]
            continue
        d = s * (SCALE * int(v[m + o[i]]) - dc)
        bits += [(1 if d < 0 else 0) ^ mask[2 * i], 1 if 3 * abs(d) >= 2 * amp else 0]
    return [bits_word(bits[32 * w : 32 * w + 32]) for w in range(WORDS)], [amp, dc, valid]


def slice_all(v, rows, pl: dict) -> tuple:
    """(bits uint32[K][12], levels int64[K][3]) of ``rows`` (m, s)."""
    out = [slice_by_loops(v, len(v), int(m), int(s), pl) for m, s in np.asarray(rows, dtype=np.int64).reshape(-1, 2).tolist()]
    return (np.array([o[0] for o in out], dtype=np.uint32).reshape(-1, WORDS), np.array([o[1] for o in out], dtype=np.int64).reshape(-1, 3))


# ---- the decoder: one frame's coders ----------------------------------------------------------------------------------------------


def record_bits(words) -> list:
    return [b for w in words for b in word_bits(int(w), 32)]


def words_of_dibits(dibits, descramble: bool = True) -> list:
    """The twelve words of a frame's dibits as ``iqa_nxdn_slice`` gives them: descrambled."""
    bits = [b for d in list(dibits)[:OFFSETS] for b in (d >> 1, d & 1)]
    bits += [0] * (2 * OFFSETS - len(bits))
    if descramble:
        bits = [b ^ m for b, m in zip(bits, scramble_mask())]
    return [bits_word(bits[32 * w : 32 * w + 32]) for w in range(WORDS)]


def valid_mask(cls: int) -> bool:
    return 0 <= cls <= 7 or cls == 8


#: the blocks of a mask, in the order of the record: (the bit, the kind, its first frame bit, its first info word, its words, its record slot)
LAYOUT = ((SACCH, "sacch", 36, 0, 2, 1), (CAC, "cac", 36, 8, 6, 1), (FACCH1_A, "facch1", 96, 2, 3, 2), (FACCH1_B, "facch1", 240, 5, 3, 3))


def decode_frame(words, cls: int, smaller: bool = True) -> tuple:
    """(info, rec, ties): the fourteen information words and the four values of one sliced frame, as ``iqa_nxdn_decode`` gives
    them, and the ties on the surviving paths."""
    frame = record_bits(words)
    cls = cls if valid_mask(cls) else 0
    out, rec, ties = [0] * (32 * INFO), [cls, 0, 0, 0], 0
    for bit, kind, first, word, _count, slot in LAYOUT:
        if not cls & bit:
            continue
        sent = BLOCKS[kind][3] * BLOCKS[kind][4]
        decoded, metric, tie = viterbi(from_channel(frame[first : first + sent], kind), smaller)
        out[32 * word : 32 * word + len(decoded)] = decoded
        rec[slot] = metric
        ties += tie
    return [bits_word(out[32 * w : 32 * w + 32]) for w in range(INFO)], rec, ties


@functools.lru_cache(maxsize=4096)
def _decode_once(words: tuple, cls: int) -> tuple:
    """``decode_frame`` of words seen before from memory: the loops are slow, and the tests repeat frames."""
    return decode_frame(list(words), cls)


def decode_all(bits, classes) -> tuple:
    """(info uint32[K][14], rec int32[K][4])."""
    out = [_decode_once(tuple(w), int(c)) for w, c in zip(np.asarray(bits).tolist(), np.asarray(classes).tolist())]
    return (np.array([o[0] for o in out], dtype=np.uint32).reshape(-1, INFO), np.array([o[1] for o in out], dtype=np.int32).reshape(-1, RECORD))


# ---- the decoder: the host rules --------------------------------------------------------------------------------------------------


def lich_of(words) -> tuple:
    """(the LICH byte, whether every second bit of its dibits is 1)."""
    frame = record_bits(words[:2])
    return bits_word(frame[20:36:2]), all(frame[21:36:2])


def lich_parts(byte: int) -> dict:
    return dict(rf=byte >> 6, fn=byte >> 4 & 3, option=byte >> 2 & 3, outbound=byte >> 1 & 1)


def lich_parity_ok(byte: int) -> bool:
    return bin(byte >> 4).count("1") % 2 == byte & 1


def lich_mask(byte: int) -> int:
    f = lich_parts(byte)
    if f["rf"] == 0:
        return CAC if f["fn"] == 0 else 0
    if f["fn"] == 1:
        return 0
    return SACCH | (0, FACCH1_B, FACCH1_A, 0)[f["option"]] | (FACCH1_A | FACCH1_B if f["option"] == 0 else 0)


def decoder_classes(bits, levels) -> list:
    out = []
    for words, lev in zip(np.asarray(bits).tolist(), np.asarray(levels).tolist()):
        byte = lich_of(words)[0]
        out.append(lich_mask(byte) if lev[2] >= NEED_FRAME and lev[0] > 0 and lich_parity_ok(byte) else 0)
    return out


def block_ok(words, kind: str) -> tuple:
    """(the bits in front of the CRC, whether the CRC holds) of a block's information words."""
    width, _, _, covered = CRC[kind]
    bits = record_bits(words)[: covered + width]
    return bits[:covered], crc(bits[:covered], kind) == bits_word(bits[covered:])


def hex_of(bits) -> str:
    return format(bits_word(bits), "0%dx" % ((len(bits) + 3) // 4))


def layer3(octets, whole: bool = True) -> dict:
    kind = octets[0] & 0x3F
    out = dict(type=kind, name=NAMES.get(kind, "0x%02X" % kind), hex=bytes(octets).hex())
    if whole and kind in (0x01, 0x08) and len(octets) >= 8:
        out.update(emergency=octets[1] >> 7, call_type=octets[2] >> 5, mode=octets[2] & 7, src=octets[3] << 8 | octets[4],
                   dst=octets[5] << 8 | octets[6], cipher=octets[7] >> 6, key=octets[7] & 0x3F)
    return out


def join(frames, parts) -> int:
    """The superframe rule: ``parts[j]`` the 18 data bits of frame j's good superframe SACCH, else None.  The parts 3, 2, 1, 0 of
    consecutive traffic frames with one RAN give a message to the last one's frame; returns the superframes dropped."""
    broken, have, ran, skipping = 0, [], None, False
    for f, part in zip(frames, parts):
        if f["rf"] == 0:
            continue
        if part is not None and f["structure"] == 3:
            if have:
                broken += 1
            have, ran, skipping = [part], f["ran"], False
        elif part is not None and have and f["structure"] == 3 - len(have) and f["ran"] == ran:
            have.append(part)
            if f["structure"] == 0:
                f["messages"].append(dict(via="sacch", **layer3(bits_bytes([b for p in have for b in p]))))
                have = []
        elif f["fn"] == 2 or have:
            if have or not skipping:
                broken += 1
            have, skipping = [], True
    return broken + (1 if have else 0)


def parse(rows, bits, levels, info, rec, fs_ch: float, start: int = 0) -> tuple:
    """(frames, counts): a dict per frame whose LICH held its parity, in order of time."""
    counts = dict(no_level=0, cut=0, lich_inner=0, lich_failed=0, sacch_failed=0, facch_failed=0, cac_failed=0, superframe_broken=0, udch=0,
                  inbound_cac=0, fixed=0)
    out = []
    for (m, _s), words, lev, iw, r in zip(np.asarray(rows).tolist(), np.asarray(bits).tolist(), np.asarray(levels).tolist(),
                                          np.asarray(info).tolist(), np.asarray(rec).tolist()):
        if lev[2] < NEED_LICH:
            counts["cut"] += 1
            continue
        if lev[0] <= 0:
            counts["no_level"] += 1
            continue
        byte, outer = lich_of(words)
        if not outer:
            counts["lich_inner"] += 1
        if not lich_parity_ok(byte):
            counts["lich_failed"] += 1
            continue
        f = dict(time_s=(start + m) / fs_ch, lich=byte, **lich_parts(byte), cls=lich_mask(byte), corrected=False, ran=None, structure=None,
                 blocks=[], messages=[])
        part = None
        if f["rf"] == 0 and f["fn"] != 0:
            counts["inbound_cac"] += 1
        if f["rf"] != 0 and f["fn"] == 1:
            counts["udch"] += 1
        if f["cls"] and lev[2] < NEED_FRAME:
            counts["cut"] += 1
        else:
            for bit, kind, _first, word, count, slot in LAYOUT:
                if not f["cls"] & bit:
                    continue
                b, ok = block_ok(iw[word : word + count], kind)
                name = kind if kind != "facch1" else "facch1-a" if bit == FACCH1_A else "facch1-b"
                f["blocks"].append([name, hex_of(b), ok])
                if not ok:
                    counts[{"sacch": "sacch_failed", "facch1": "facch_failed", "cac": "cac_failed"}[kind]] += 1
                    continue
                f["corrected"] = f["corrected"] or r[slot] > 0
                if kind == "facch1":
                    f["messages"].append(dict(via=name, **layer3(bits_bytes(b))))
                    continue
                f["structure"], f["ran"] = bits_word(b[0:2]), bits_word(b[2:8])
                if kind == "cac":
                    f["messages"].append(dict(via="cac", **layer3(bits_bytes(b[8:152]))))
                elif f["fn"] == 2:
                    part = b[8:26]
                elif f["fn"] == 0:
                    f["messages"].append(dict(layer3(bits_bytes(b[8:16]), whole=False), via="sacch", hex=hex_of(b[8:26])))
        out.append((f, part))
    out.sort(key=lambda e: e[0]["time_s"])
    frames = [f for f, _ in out]
    counts["superframe_broken"] = join(frames, [p for _, p in out])
    counts["fixed"] = sum(1 for f in frames if f["corrected"])
    return frames, counts


CALL_FIELDS = ("emergency", "call_type", "mode", "src", "dst", "cipher", "key")


def track(frames) -> list:
    """The calls as dicts, in order of their start."""
    out, cur, last = [], None, 0.0
    for f in frames:
        if f["rf"] == 0:
            continue
        if cur is not None and f["time_s"] - last > HANG_S:
            cur = None
        last = f["time_s"]
        vcalls = [x for x in f["messages"] if x["type"] == 0x01 and "src" in x]
        if cur is None:
            opened = f["fn"] == 0 and any(x["via"] in ("facch1-a", "facch1-b") for x in vcalls)
            cur = dict(start_s=f["time_s"], end_s=f["time_s"], frames=0, ran=None, src=None, dst=None, call_type=None, emergency=None, mode=None,
                       cipher=None, key=None, late=not opened, released=False, conflicts=0)
            out.append(cur)
        cur["frames"] += 1
        cur["end_s"] = f["time_s"]
        values = ([("ran", f["ran"])] if f["ran"] is not None else []) + [(name, x[name]) for x in vcalls for name in CALL_FIELDS]
        for name, value in values:
            if cur[name] is None:
                cur[name] = value
            elif cur[name] != value:
                cur["conflicts"] += 1
        if any(x["type"] == 0x08 for x in f["messages"]):
            cur["released"] = True
            cur = None
    return out


def call_line(c: dict) -> str:
    parts = ["NXDN"]
    if c["ran"] is not None:
        parts.append("RAN %d" % c["ran"])
    if c["src"] is not None:
        parts.append(str(c["src"]))
    if c["dst"] is not None:
        parts += ["->", str(c["dst"])]
    if c["call_type"] is not None:
        parts.append(CALL_TYPES.get(c["call_type"], str(c["call_type"])))
    if c["cipher"] is not None:
        parts.append("clear" if c["cipher"] == 0 else "cipher %d" % c["cipher"])
    parts.append("%.2f s (%d frame%s)" % (c["end_s"] - c["start_s"], c["frames"], "" if c["frames"] == 1 else "s"))
    return " ".join(parts)


def fold(frames) -> list:
    """One dict per distinct CAC message (RAN, type, hex), in order of first appearance."""
    seen = {}
    for f in frames:
        for x in f["messages"]:
            if x["via"] != "cac":
                continue
            key = (f["ran"], x["type"], x["hex"])
            if key not in seen:
                seen[key] = dict(ran=f["ran"], type=x["type"], name=x["name"], hex=x["hex"], count=0, first_s=f["time_s"], last_s=f["time_s"])
            seen[key]["count"] += 1
            seen[key]["last_s"] = f["time_s"]
    return list(seen.values())


def control_line(c: dict) -> str:
    return "NXDN RAN %d %s %s x%d %.2f .. %.2f s" % (c["ran"], c["name"], c["hex"], c["count"], c["first_s"], c["last_s"])


def frame_kind(f: dict) -> str:
    return RF_NAMES[f["rf"]] + " " + FN_NAMES[0 if f["rf"] == 0 else 1][f["fn"]]


def decode_plane(v, kept, pl: dict, start: int = 0) -> dict:
    """The whole model behind the sync search on one integrated plane."""
    rows = np.array(frame_hits(kept, pl["ident"]["h"]), dtype=np.int64).reshape(-1, 2)
    bits, levels = slice_all(v, rows, pl)
    classes = decoder_classes(bits, levels)
    info, rec = decode_all(bits, classes)
    frames, counts = parse(rows, bits, levels, info, rec, pl["fs_ch"], start)
    kinds = {}
    for f in frames:
        kinds[frame_kind(f)] = kinds.get(frame_kind(f), 0) + 1
    return dict(rows=rows, bits=bits, levels=levels, classes=np.array(classes, dtype=np.uint8), info=info, rec=rec, frames=frames, counts=counts,
                calls=track(frames), control=fold(frames), kinds=kinds)


def decode_theta(theta, fs_ch: float, c: int = 0, rate: int = 4800) -> dict:
    pl = plan(fs_ch, rate)
    v = IM.integrate(theta, c, pl["ident"]["L"], pl["ident"]["sh"])
    _, kept = IM.search(v, pl["ident"], NXDN_PATTERNS)
    out = decode_plane(v, kept, pl)
    out.update(v=v, kept=kept, plan=pl)
    return out


# ---- the test streams and the model capture ----------------------------------------------------------------------------------------

RAN = 5
VCALL = vcall()
VCALL9 = bytes_bits(vcall(size=9))  # the 72 bits that the four SACCH parts of a superframe carry
TX_REL = vcall(kind=0x08)
OTHER = [0x3B, 1, 2, 3, 4, 5, 6, 7, 8, 9]  # a message type without a name
TRAFFIC, DATA = 1, 2


def header_frame(message=VCALL, **opt) -> dict:
    """A non-superframe frame with ``message`` in both FACCH1s; its SACCH carries the message's first 18 bits."""
    return dict(lich=lich_byte(TRAFFIC, 0, 0), sacch=(0, RAN, bytes_bits(message)[:18]), fa=message, fb=message, **opt)


def voice_frame(part: int, message_bits=VCALL9, **opt) -> dict:
    """Frame 3 - ``part`` of a voice superframe: no FACCH1, SACCH structure ``part`` with its 18 bits of the message."""
    at = 18 * (3 - part)
    return dict(lich=lich_byte(TRAFFIC, 2, 3), sacch=(part, RAN, message_bits[at : at + 18]), **opt)


def second_half_frame(message=OTHER, **opt) -> dict:
    """A non-superframe frame with voice in its first half and a FACCH1 in its second."""
    return dict(lich=lich_byte(TRAFFIC, 0, 1), sacch=(0, RAN, bytes_bits(message)[:18]), fb=message, **opt)


def cac_frame(octets, ran: int = RAN, **opt) -> dict:
    return dict(lich=lich_byte(0, 0, 0), cac=(0, ran, octets), **opt)


SITE_INFO = [0x18, 0x12, 0x34, 0x56, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x0E]
SRV_INFO = [0x19, 0x12, 0x34, 0x56, 0xA0, 0x00, 0x01, 0x02]
IDLE = [0x10]
#: a call: its header, two voice superframes, a frame with a FACCH1 in its second half alone, the release
SCRIPT = [header_frame()] + [voice_frame(p) for p in (3, 2, 1, 0)] * 2 + [second_half_frame(), header_frame(TX_REL)]
CONTROL_SCRIPT = [cac_frame(SITE_INFO), cac_frame(SRV_INFO), cac_frame(IDLE), cac_frame(IDLE), cac_frame(SITE_INFO), cac_frame(IDLE)]
STREAM_START = 0.02
LINE = "NXDN RAN 5 1234 -> 5678 group clear 0.40 s (11 frames)"
CLASSES = [7, 1, 1, 1, 1, 1, 1, 1, 1, 5, 7]
KINDS = {"RTCH non-superframe": 3, "RTCH superframe": 8}
CONTROL_LINES = ["NXDN RAN 5 SITE_INFO " + bytes(SITE_INFO).hex() + " x2 0.02 .. 0.18 s",
                 "NXDN RAN 5 SRV_INFO " + bytes(SRV_INFO + [0] * 10).hex() + " x1 0.06 .. 0.06 s",
                 "NXDN RAN 5 IDLE " + bytes(IDLE + [0] * 17).hex() + " x3 0.10 .. 0.22 s"]


def test_stream(fs_ch: float, noise: float = 0.0, seed: int = 3, script=None, negate: bool = False, rate: int = 4800) -> np.ndarray:
    levels = station(SCRIPT if script is None else script)
    n = int((STREAM_START + len(levels) / float(rate) + 0.02) * fs_ch)
    theta = synth_theta(levels, fs_ch, n, STREAM_START, noise, seed, rate)
    return -theta if negate else theta


FS, SECS, AMP = IM.FS, IM.SECS, IM.AMP
CAPTURE_CHANNELS = (("nxdn", 200e3), ("voice", 600e3))


def capture_script() -> list:
    """192 random symbols (the channel filter settles in them, and the station is on the air from the first sample), the call
    of ``SCRIPT``, then a second call until the capture ends."""
    second = [header_frame(vcall(src=4321, dst=8765, call_type=4, cipher=1, key=9))]
    second += [voice_frame(p, bytes_bits(vcall(src=4321, dst=8765, call_type=4, cipher=1, key=9, size=9))) for p in (3, 2, 1, 0)] * 10
    return [("random", 192)] + SCRIPT + second


@functools.lru_cache(maxsize=1)
def capture() -> np.ndarray:
    """int16[n][2]: a model capture in ``ident_model``'s conventions (s16, 2.4 MS/s, 2 s, AMP 0.05, complex noise 30 dB under AMP
    in total, seed 11, DC 0.01): an NXDN channel at +200 kHz that sends ``capture_script()`` at 4800 symbols/s, and an NFM voice
    channel at +600 kHz."""
    n = int(round(FS * SECS))
    t = np.arange(n) / FS
    rng = np.random.default_rng(11)
    sigma = AMP * 10.0 ** (-30.0 / 20.0) / math.sqrt(2.0)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    off = dict(CAPTURE_CHANNELS)
    car = lambda name: np.exp(2j * np.pi * ((off[name] * t) % 1.0))  # noqa: E731
    levels = station(capture_script())
    x += (AMP / 2.0) * car("nxdn") * IM.fsk_levels(levels, 4800.0, DEV, n)
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
    25's identification and this section's frames, calls and control lines, per found channel."""
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
        nxdn = None
        if named["rate"] in (4800, 2400) and named["plan"] is not None:
            pl = plan(d["plan"]["fs_ch"], named["rate"])
            family = IM.family(named["rate"])
            nxdn = decode_plane(named["v"], [(0,) + tuple(h[1:]) for h in named["kept"] if family[h[0]][0] == "nxdn"], pl, k["keyed_from"])
        out.append(dict(described=d, keyed=k, named=named, nxdn=nxdn))
    return out


# ---- crafted words for the coders (the host test and the GPU shapes test share them) -----------------------------------------------


def flipped_words(words, frame_bits) -> list:
    """``words`` with the frame bits ``frame_bits`` flipped."""
    out = [int(w) for w in words]
    for b in frame_bits:
        out[b >> 5] ^= 1 << (31 - (b & 31))
    return out


def frame_words(item: dict, seed: int = 2) -> list:
    return words_of_dibits(make_frame(item, np.random.default_rng(seed)))


BLOCK_CASES = {"sacch": (voice_frame(3), SACCH, 36, 60), "facch1-a": (header_frame(), FACCH1_A, 96, 144), "facch1-b": (header_frame(), FACCH1_B, 240, 144),
               "cac": (cac_frame(SITE_INFO), CAC, 36, 300)}


@functools.lru_cache(maxsize=None)
def tie_case(name: str = "sacch") -> tuple:
    """(words, mask, flips): a frame with the block ``name`` (of BLOCK_CASES) and the frame bits of it whose flips make the tie rule matter: the two rules decode
    different bits.  Two paths tie across an error event whose sent weight is even, with half of its bits flipped: the first
    input pattern, from step 4 on, whose coded word keeps six bits or fewer behind the puncturing, and the first half of them
    on which the two rules differ.  (Unpunctured the code's lightest event weighs 7; punctured, events of 6 sent bits exist.)"""
    import itertools

    item, mask, first, _sent = BLOCK_CASES[name]
    kind = "facch1" if name.startswith("facch1") else name
    words = frame_words(item)
    size = BLOCKS[kind][0] - 4
    for start in range(4, 24):
        for pattern in range(1, 64, 2):
            info = [0] * start + word_bits(pattern, pattern.bit_length())
            coded = conv_encode(info + [0] * (size - len(info)))
            kept = [j for j, c in enumerate(coded) if c and not punctured(j, kind)]
            if len(kept) % 2 or len(kept) > 6:
                continue
            for half in itertools.combinations(kept, len(kept) // 2):
                flips = tuple(first + channel_index(sum(1 for i in range(j) if not punctured(i, kind)), kind) for j in half)
                bad = flipped_words(words, flips)
                if decode_frame(bad, mask)[0] != decode_frame(bad, mask, smaller=False)[0]:
                    return bad, mask, flips
    raise AssertionError("no tie found")


@functools.lru_cache(maxsize=1)
def coder_cases() -> dict:
    """name -> (the 12 words, mask): the crafted frames of the coder tests."""
    out = {}
    for name, (item, mask, first, sent) in BLOCK_CASES.items():
        words = frame_words(item)
        out[name] = (words, mask)
        for k in range(0, sent, 7):  # one flipped channel bit, anywhere
            out[f"{name}-one-{k}"] = (flipped_words(words, [first + k]), mask)
    head = frame_words(header_frame())
    for cls in list(range(16)) + [16, 17, 200, 255]:
        out[f"class-{cls}"] = (head, cls)
    for cls in (7, 8):
        out[f"zeros-{cls}"], out[f"ones-{cls}"] = ([0] * WORDS, cls), ([0xFFFFFFFF] * WORDS, cls)
    for name in BLOCK_CASES:
        out[f"{name}-tie"] = tie_case(name)[:2]
    return out
