"""Numpy oracle and encoder of the DMR burst decoding (--find-dmr), written from the specification with
its own copy of every constant.  Of the package it uses nothing; the quantiser, the integrator and the sync search are
``ident_model``'s.  The encoder goes from link control or a CSBK through Reed-Solomon or the CRC, the BPTC(196,96) and its
interleave, the slot type, the burst with its sync word and the CACH with its TACT to dibits and a rectangular 4-level FSK
theta.  The oracle has one function per step: the slicing in plain loops (``slice_by_loops``) and vectorised (``slice_all``),
the coders per burst in plain integers.  Also the model capture of the CLI tests: one DMR base channel and a voice channel."""
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

BS_VOICE, MS_VOICE = 0x755FD7DF75F7, 0x7F7D5DD57DFD
BS_DATA, MS_DATA = 0xDFF57D75DF5D, 0xD5D7F77FD757
KINDS = ("bs voice", "bs data", "ms voice", "ms data")
SYNC = (BS_VOICE, BS_DATA, MS_VOICE, MS_DATA)
LEVEL = {0b01: 3, 0b00: 1, 0b10: -1, 0b11: -3}
DMR_PATTERNS = [p for p in IM.PATTERNS if p[0] == "dmr"]
TACT_BITS = (0, 4, 8, 12, 14, 18, 22)
TACT_CHECKS = ((0, 1, 2), (1, 2, 3), (0, 1, 3))
SLOT_TYPE_BITS = tuple(range(98, 108)) + tuple(range(156, 166))
GOLAY_POLY = 0xC75
INTERLEAVE = 181
PAYLOAD_BITS = tuple(range(98)) + tuple(range(166, 264))
ROW_CHECKS = ((0, 1, 2, 3, 5, 7, 8), (1, 2, 3, 4, 6, 8, 9), (2, 3, 4, 5, 7, 9, 10), (0, 1, 2, 4, 6, 7, 10))
COLUMN_CHECKS = ((0, 1, 3, 5, 6), (0, 1, 2, 4, 6, 7), (0, 1, 2, 3, 5, 7, 8), (0, 2, 4, 5, 8))
ROUNDS = 5
INFO_INDEX = tuple(range(4, 12)) + tuple(1 + 15 * r + c for r in range(1, 9) for c in range(11))
GF_POLY = 0x11D
RS_GENERATOR = (1, 14, 56, 64)
RS_MASK = {1: 0x96, 2: 0x99}
CRC_MASK = {3: 0xA5A5, 6: 0xCCCC}
DATA_TYPES = ("pi header", "voice lc header", "terminator lc", "csbk", "mbc header", "mbc continuation", "data header",
              "rate 1/2 data", "rate 3/4 data", "idle", "rate 1 data")
HANG_S = 0.720
DEV = 648.0  # a level of +-1 / +-3 deviates +-648 / +-1944 Hz


def word_bits(word: int, n: int) -> list:
    return [(word >> (n - 1 - i)) & 1 for i in range(n)]


def bits_word(bits) -> int:
    out = 0
    for b in bits:
        out = out << 1 | int(b)
    return out


def sync_levels(word: int) -> list:
    return [LEVEL[(word >> (2 * (23 - i))) & 3] for i in range(24)]


# ---- the codes ----------------------------------------------------------------------------------------------------------------


def gf_mul(a: int, b: int) -> int:
    """Russian-peasant product in GF(2^8) / 0x11D."""
    out = 0
    while b:
        if b & 1:
            out ^= a
        a <<= 1
        if a & 0x100:
            a ^= GF_POLY
        b >>= 1
    return out


def poly_mod(data, gen=RS_GENERATOR) -> list:
    """The remainder of the polynomial ``data`` (highest coefficient first) modulo the monic ``gen``: len(gen) - 1 bytes."""
    work = list(data)
    for i in range(len(work) - (len(gen) - 1)):
        lead = work[i]
        if lead:
            for j, g in enumerate(gen):
                work[i + j] ^= gf_mul(lead, g)
    return work[-(len(gen) - 1):]


def rs_parity(nine) -> list:
    return poly_mod(list(nine) + [0, 0, 0])


def crc_ccitt(data) -> int:
    crc = 0
    for byte in data:
        for i in range(7, -1, -1):
            top = ((crc >> 15) & 1) ^ ((byte >> i) & 1)
            crc = (crc << 1) & 0xFFFF
            if top:
                crc ^= 0x1021
    return crc


def golay(data: int) -> int:
    r = data << 11
    for i in range(18, 10, -1):
        if (r >> i) & 1:
            r ^= GOLAY_POLY << (i - 11)
    cw = data << 12 | (r & 0x7FF) << 1
    return cw | bin(cw).count("1") & 1


GOLAY = tuple(golay(d) for d in range(256))


def slot_type_decode(word: int) -> tuple:
    """(status, distance, byte) of a 20-bit word."""
    dist, value = min((bin(word ^ cw).count("1"), d) for d, cw in enumerate(GOLAY))
    if dist == 0:
        return 0, 0, value
    return (1, dist, value) if dist <= 3 else (2, dist, word >> 12)


def _syndrome(bits, checks, first_parity: int) -> tuple:
    return tuple((sum(bits[j] for j in eq) + bits[first_parity + e]) & 1 for e, eq in enumerate(checks))


def _columns(checks, length: int, first_parity: int) -> dict:
    """syndrome -> position of a single flipped bit."""
    out = {}
    for j in range(length):
        unit = [0] * length
        unit[j] = 1
        out[_syndrome(unit, checks, first_parity)] = j
    return out


H7, H13, H15 = _columns(TACT_CHECKS, 7, 4), _columns(COLUMN_CHECKS, 13, 9), _columns(ROW_CHECKS, 15, 11)


def tact_decode(seven) -> tuple:
    """(status, nibble) of AT, TC, LCSS1, LCSS0, P0, P1, P2."""
    bits = [int(b) for b in seven]
    syn = _syndrome(bits, TACT_CHECKS, 4)
    status = 0
    if any(syn):
        bits[H7[syn]] ^= 1
        status = 1
    return status, bits_word(bits[:4])


def tact_encode(at: int, tc: int, lcss: int) -> list:
    d = [at, tc, (lcss >> 1) & 1, lcss & 1]
    return d + [sum(d[j] for j in eq) & 1 for eq in TACT_CHECKS]


def bptc_encode(info96) -> list:
    """The 196 bits as sent (interleaved) of 96 information bits."""
    D = [0] * 196
    for q, at in enumerate(INFO_INDEX):
        D[at] = int(info96[q])
    for r in range(9):
        row = D[1 + 15 * r : 12 + 15 * r]
        for e, eq in enumerate(ROW_CHECKS):
            D[1 + 15 * r + 11 + e] = sum(row[j] for j in eq) & 1
    for c in range(15):
        col = [D[1 + 15 * r + c] for r in range(9)]
        for e, eq in enumerate(COLUMN_CHECKS):
            D[1 + 15 * (9 + e) + c] = sum(col[j] for j in eq) & 1
    raw = [0] * 196
    for k in range(196):
        raw[(INTERLEAVE * k) % 196] = D[k]
    return raw


def bptc_decode(raw196) -> tuple:
    """(status, flips, rounds, info96) of the 196 bits as sent."""
    D = [int(raw196[(INTERLEAVE * k) % 196]) for k in range(196)]
    flips = rounds = 0
    while rounds < ROUNDS:
        rounds += 1
        now = 0
        for c in range(15):
            syn = _syndrome([D[1 + 15 * r + c] for r in range(13)], COLUMN_CHECKS, 9)
            if any(syn) and syn in H13:
                D[1 + 15 * H13[syn] + c] ^= 1
                now += 1
        for r in range(9):
            syn = _syndrome(D[1 + 15 * r : 16 + 15 * r], ROW_CHECKS, 11)
            if any(syn):
                D[1 + 15 * r + H15[syn]] ^= 1
                now += 1
        flips += now
        if not now:
            break
    ok = not any(any(_syndrome([D[1 + 15 * r + c] for r in range(13)], COLUMN_CHECKS, 9)) for c in range(15))
    ok = ok and not any(any(_syndrome(D[1 + 15 * r : 16 + 15 * r], ROW_CHECKS, 11)) for r in range(9))
    return (0 if ok and not flips else 1 if ok else 2), flips, rounds, [D[at] for at in INFO_INDEX]


# ---- the encoder --------------------------------------------------------------------------------------------------------------


def lc_info(data_type: int, flco: int, src: int, dst: int, fid: int = 0, options: int = 0, pf: int = 0, break_rs: bool = False) -> list:
    """The 96 bits of a voice LC header (type 1) or a terminator with LC (type 2)."""
    nine = [pf << 7 | flco, fid, options, dst >> 16 & 0xFF, dst >> 8 & 0xFF, dst & 0xFF, src >> 16 & 0xFF, src >> 8 & 0xFF, src & 0xFF]
    parity = [p ^ RS_MASK[data_type] for p in rs_parity(nine)]
    if break_rs:
        parity[0] ^= 0x5A
    return [b for byte in nine + parity for b in word_bits(byte, 8)]


def csbk_info(csbko: int, fid: int, data8, data_type: int = 3, lb: int = 1, pf: int = 0) -> list:
    ten = [lb << 7 | pf << 6 | csbko, fid] + list(data8)
    crc = (crc_ccitt(ten) ^ 0xFFFF) ^ CRC_MASK[data_type]
    return [b for byte in ten + [crc >> 8, crc & 0xFF] for b in word_bits(byte, 8)]


def data_burst_bits(kind: int, cc: int, data_type: int, info96) -> list:
    """The 264 bits of a data burst: the payload's halves around the slot type's halves around the sync word."""
    raw, st = bptc_encode(info96), word_bits(GOLAY[cc << 4 | data_type], 20)
    return raw[:98] + st[:10] + word_bits(SYNC[kind], 48) + st[10:] + raw[98:]


def voice_burst_bits(kind: int, rng, sync: bool = True) -> list:
    """A voice burst: 108 vocoder bits either side of the sync word (burst A) or of 48 bits that are none (bursts B .. F)."""
    middle = word_bits(SYNC[kind], 48) if sync else [1, 0] * 24  # (the levels -1: no sync word, no DC)
    return rng.integers(0, 2, 108).tolist() + middle + rng.integers(0, 2, 108).tolist()


def cach_bits(tc: int, rng, at: int = 1, lcss: int = 0) -> list:
    bits = rng.integers(0, 2, 24).tolist()
    for at_bit, b in zip(TACT_BITS, tact_encode(at, tc, lcss)):
        bits[at_bit] = b
    return bits


def levels_of_bits(bits) -> list:
    return [LEVEL[int(bits[2 * j]) << 1 | int(bits[2 * j + 1])] for j in range(len(bits) // 2)]


IDLE_INFO = [0] * 96


def base_station(script, cc: int = 1, seed: int = 5) -> list:
    """The symbol levels of a base station that sends ``script``, one entry per 30 ms slot (144 symbols: CACH, burst), the slots
    alternating 1, 2, 1, ...: None (an idle burst), ("header" | "term", flco, src, dst[, options]), ("csbk", o, fid, data8), "voice"
    (burst A with its sync word), "voice-" (bursts B .. F), ("raw", data_type, info96)."""
    rng = np.random.default_rng(seed)
    out = []
    for j, item in enumerate(script):
        tc = j & 1  # slot = 1 + tc
        if item is None:
            bits = data_burst_bits(1, cc, 9, IDLE_INFO)
        elif item == "voice":
            bits = voice_burst_bits(0, rng)
        elif item == "voice-":
            bits = voice_burst_bits(0, rng, sync=False)
        elif item[0] in ("header", "term"):
            dt = 1 if item[0] == "header" else 2
            bits = data_burst_bits(1, cc, dt, lc_info(dt, item[1], item[2], item[3], **(item[4] if len(item) > 4 else {})))
        elif item[0] == "csbk":
            bits = data_burst_bits(1, cc, 3, csbk_info(item[1], item[2], item[3]))
        elif item[0] == "raw":
            bits = data_burst_bits(1, cc, item[1], item[2])
        else:
            raise ValueError(item)
        out += levels_of_bits(cach_bits(tc, rng) + bits)
    return out


def synth_theta(levels, fs_ch: float, n: int, start_s: float = 0.0, noise: float = 0.0, seed: int = 1) -> np.ndarray:
    """float32[n]: the discriminator output of the rectangular 4-level FSK of ``levels`` at 4800 symbols/s from ``start_s`` on, a
    level l deviating l 648 Hz, 0 elsewhere; ``noise``: the sigma of white Gaussian noise on theta, in radians."""
    f = np.zeros(n, dtype=np.float64)
    edges = start_s + np.arange(len(levels) + 1) / 4800.0
    idx = np.ceil(edges * fs_ch - 1e-9).astype(np.int64)
    for lev, a, b in zip(levels, idx[:-1], idx[1:]):
        f[max(a, 0) : max(min(b, n), 0)] = lev * DEV
    theta = 2.0 * np.pi * f / fs_ch
    if noise:
        theta = theta + noise * np.random.default_rng(seed).standard_normal(n)
    return theta.astype(np.float32)


# ---- the oracle: plan, bursts, slicing --------------------------------------------------------------------------------------------


def plan(fs_ch: float) -> dict:
    """sps, o[-66 .. 77] (a dict by symbol index) and ``ident_model``'s plan at 4800; ValueError unless 4 <= sps <= 224."""
    ident = IM.plan(fs_ch, 4800)
    return dict(fs_ch=float(fs_ch), sps=ident["sps"], o={i: int(round(i * ident["sps"])) for i in range(-66, 78)}, ident=ident)


def burst_hits(kept, h: int) -> list:
    """(m, s, kind) in order of m from ``ident_model``'s kept hits over DMR_PATTERNS (pattern 0 bs, 1 ms)."""
    cand = [(m, abs(C), p, 1 if C > 0 else -1) for p, m, C, _E, _pre, _post in kept if p in (0, 1) and C != 0]
    out = []
    for m, a, p, s in cand:
        beaten = False
        for m2, a2, p2, _ in cand:
            if (m2, p2) != (m, p) and abs(m2 - m) <= h and (a2 > a or (a2 == a and (m2 < m or (m2 == m and p2 < p)))):
                beaten = True
        if not beaten:
            out.append((m, s, 2 * p + (1 if s < 0 else 0)))
    return sorted(out)


def slice_by_loops(v, n: int, m: int, s: int, kind: int, pl: dict) -> tuple:
    """(the nine words, [Sigma, A, flags]) of one hit."""
    o = pl["o"]
    inside = lambda i: 0 <= m + o[i] < n  # noqa: E731
    burst_ok = all(inside(i) for i in range(-54, 78))
    cach_ok = kind < 2 and all(inside(i) for i in range(-66, -54))
    if not burst_ok:
        return [0] * 9, [0, 0, 2 if cach_ok else 0]
    sgn = sync_levels(BS_VOICE if kind < 2 else MS_VOICE)
    x = [int(v[m + o[i]]) for i in range(24)]
    sigma, amp = sum(x), s * sum((1 if g > 0 else -1) * xi for g, xi in zip(sgn, x))
    bits = []
    for i in range(-66, 78):
        if i < -54 and not cach_ok:
            bits += [0, 0]
            continue
        d = 24 * int(v[m + o[i]]) - sigma
        bits += [1 if d < 0 else 0, 1 if 3 * abs(d) >= 2 * amp else 0]
    return [bits_word(bits[32 * w : 32 * w + 32]) for w in range(9)], [sigma, amp, 1 | (2 if cach_ok else 0)]


def slice_all(v, rows, pl: dict) -> tuple:
    """(bits uint32[K][9], levels int64[K][3]) of ``rows`` (m, s, kind), vectorised."""
    v = np.asarray(v, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    n, k = v.size, rows.shape[0]
    o = np.array([pl["o"][i] for i in range(-66, 78)], dtype=np.int64)
    at = rows[:, :1] + o[None, :]  # [K][144]
    inside = (at >= 0) & (at < n)
    burst_ok = inside[:, 12:].all(axis=1)
    cach_ok = (rows[:, 2] < 2) & inside[:, :12].all(axis=1)
    y = np.where(inside, v[np.clip(at, 0, max(n - 1, 0))] if n else 0, 0)
    sgn = np.array([[1 if g > 0 else -1 for g in sync_levels(BS_VOICE if kind < 2 else MS_VOICE)] for kind in rows[:, 2].tolist()],
                   dtype=np.int64).reshape(k, 24)
    sigma = np.where(burst_ok, y[:, 66:90].sum(axis=1), 0)
    amp = np.where(burst_ok, rows[:, 1] * (sgn * y[:, 66:90]).sum(axis=1), 0)
    d = 24 * y - sigma[:, None]
    read = burst_ok[:, None] & np.concatenate([np.repeat(cach_ok[:, None], 12, axis=1), np.ones((k, 132), dtype=bool)], axis=1)
    two = np.stack([(d < 0) & read, (3 * np.abs(d) >= 2 * amp[:, None]) & read], axis=2).reshape(k, 288).astype(np.uint64)
    weights = (1 << np.arange(31, -1, -1)).astype(np.uint64)
    bits = (two.reshape(k, 9, 32) * weights).sum(axis=2).astype(np.uint32)
    levels = np.stack([sigma, amp, burst_ok.astype(np.int64) | (cach_ok.astype(np.int64) << 1)], axis=1)
    return bits, levels


# ---- the oracle: one burst's coders -----------------------------------------------------------------------------------------------


def record_bits(words) -> list:
    return [b for w in words for b in word_bits(int(w), 32)]


def words_of(cach24, burst264) -> list:
    bits = list(cach24) + list(burst264)
    return [bits_word(bits[32 * w : 32 * w + 32]) for w in range(9)]


def decode_burst(words, kind: int) -> tuple:
    """(info, rec): the three information words and the eight values of one sliced burst, as ``iqa_dmr_decode`` gives them."""
    bits = record_bits(words)
    cach, burst = bits[:24], bits[24:]
    rec = [4, 0, 4, 0, 0, 4, 0, 0]
    info = [0] * 96
    if kind < 2:
        rec[0], rec[1] = tact_decode([cach[j] for j in TACT_BITS])
    if kind & 1:
        rec[2], rec[3], rec[4] = slot_type_decode(bits_word(burst[j] for j in SLOT_TYPE_BITS))
        if rec[2] != 2:
            rec[5], rec[6], rec[7], info = bptc_decode([burst[j] for j in PAYLOAD_BITS])
    return [bits_word(info[32 * w : 32 * w + 32]) for w in range(3)], rec


def decode_all(bits, kinds) -> tuple:
    """(info uint32[K][3], rec int32[K][8])."""
    out = [decode_burst(w, int(kind)) for w, kind in zip(np.asarray(bits).tolist(), np.asarray(kinds).tolist())]
    return (np.array([o[0] for o in out], dtype=np.uint32).reshape(-1, 3), np.array([o[1] for o in out], dtype=np.int32).reshape(-1, 8))


def apply_flags(rec, levels, kinds) -> np.ndarray:
    rec = np.array(rec, dtype=np.int32).reshape(-1, 8)
    for j, (lev, kind) in enumerate(zip(np.asarray(levels).tolist(), np.asarray(kinds).tolist())):
        if kind < 2 and not lev[2] & 2:
            rec[j, 0] = 3
        if not lev[2] & 1:
            rec[j, 5] = 3
    return rec


# ---- the oracle: checks, fields, calls ----------------------------------------------------------------------------------------------


def info_bytes(words) -> list:
    return [(int(w) >> sh) & 0xFF for w in words for sh in (24, 16, 8, 0)]


def check_lc(by, data_type: int) -> bool:
    by = list(by[:9]) + [b ^ RS_MASK[data_type] for b in by[9:12]]
    return poly_mod(by) == [0, 0, 0]


def check_csbk(by, data_type: int) -> bool:
    return (crc_ccitt(by[:10]) ^ 0xFFFF) == ((by[10] << 8 | by[11]) ^ CRC_MASK[data_type])


def parse(rows, levels, info, rec, fs_ch: float, start: int = 0) -> tuple:
    """(bursts, counts): a dict per read burst in order of time."""
    counts = dict(no_level=0, cut=0, slot_refused=0, bptc_failed=0, check_failed=0, tact_fixed=0, idle=0)
    out = []
    for (m, _s, kind), lev, words, r in zip(np.asarray(rows).tolist(), np.asarray(levels).tolist(), np.asarray(info).tolist(),
                                            np.asarray(rec).tolist()):
        if not lev[2] & 1:
            counts["cut"] += 1
            continue
        if lev[1] <= 0:
            counts["no_level"] += 1
            continue
        counts["tact_fixed"] += r[0] == 1
        b = dict(time_s=(start + m) / fs_ch, kind=kind, slot=1 + (r[1] >> 2 & 1) if r[0] in (0, 1) else None, cc=None, data_type=None,
                 type_name=None, checked=None, corrected=False, flco=None, fid=None, src=None, dst=None, csbko=None, hex=None)
        if kind & 1:
            if r[2] == 2:
                counts["slot_refused"] += 1
                continue
            by = info_bytes(words)
            dt = r[4] & 15
            b.update(cc=r[4] >> 4, data_type=dt, type_name=DATA_TYPES[dt] if dt < len(DATA_TYPES) else "reserved",
                     corrected=r[2] == 1 or r[5] == 1, hex=bytes(by).hex())
            if r[5] == 2:
                counts["bptc_failed"] += 1
                b.update(checked=False, hex=None)
            elif dt == 9:
                counts["idle"] += 1
            elif dt in (1, 2):
                b["checked"] = check_lc(by, dt)
                if b["checked"]:
                    b.update(flco=by[0] & 63, fid=by[1], dst=by[3] << 16 | by[4] << 8 | by[5], src=by[6] << 16 | by[7] << 8 | by[8])
                else:
                    counts["check_failed"] += 1
            elif dt in (3, 6):
                b["checked"] = check_csbk(by, dt)
                if b["checked"] and dt == 3:
                    b.update(csbko=by[0] & 63, fid=by[1])
                if not b["checked"]:
                    counts["check_failed"] += 1
        out.append(b)
    return sorted(out, key=lambda b: b["time_s"]), counts


def track(bursts) -> list:
    """The calls as dicts, in order of their start."""
    calls, cur, last = [], {}, {}
    for b in bursts:
        slot = b["slot"]
        if slot in cur and b["time_s"] - last[slot] > HANG_S:
            del cur[slot]
        last[slot] = b["time_s"]
        call = cur.get(slot)
        new = lambda **kw: dict(start_s=b["time_s"], end_s=b["time_s"], slot=slot, cc=None, group=None, src=None, dst=None,  # noqa: E731
                                superframes=0, terminated=False, **kw)
        if b["data_type"] is None:
            if call is None:
                call = cur[slot] = new()
                calls.append(call)
            call["superframes"] += 1
        elif b["checked"] and b["data_type"] == 1 and b["flco"] in (0, 3):
            who = dict(group=b["flco"] == 0, src=b["src"], dst=b["dst"])
            if call is not None and {k: call[k] for k in who} != who:
                call = None
            if call is None:
                call = cur[slot] = {**new(), **who, "cc": b["cc"]}
                calls.append(call)
        elif b["checked"] and b["data_type"] == 2 and call is not None:
            call.update(terminated=True, end_s=b["time_s"], cc=b["cc"] if call["cc"] is None else call["cc"])
            del cur[slot]
            continue
        if call is not None:
            call["end_s"] = b["time_s"]
            if call["cc"] is None and b["cc"] is not None:
                call["cc"] = b["cc"]
    return calls


def decode_plane(v, kept, pl: dict, start: int = 0) -> dict:
    """The whole oracle behind the sync search on one integrated plane."""
    rows = np.array(burst_hits(kept, pl["ident"]["h"]), dtype=np.int64).reshape(-1, 3)
    bits, levels = slice_all(v, rows, pl)
    info, rec = decode_all(bits, rows[:, 2])
    rec = apply_flags(rec, levels, rows[:, 2])
    bursts, counts = parse(rows, levels, info, rec, pl["fs_ch"], start)
    return dict(rows=rows, bits=bits, levels=levels, info=info, rec=rec, bursts=bursts, counts=counts, calls=track(bursts))


def decode_theta(theta, fs_ch: float, c: int = 0) -> dict:
    pl = plan(fs_ch)
    v = IM.integrate(theta, c, pl["ident"]["L"], pl["ident"]["sh"])
    _, kept = IM.search(v, pl["ident"], DMR_PATTERNS)
    out = decode_plane(v, kept, pl)
    out.update(v=v, kept=kept, plan=pl)
    return out


# ---- the test stream and the model capture ---------------------------------------------------------------------------------------

SRC, DST = 2345678, 9
#: idle, a header (twice), three superframes on slot 1 with slot 2 idle and one CSBK, a terminator, idle
SCRIPT = ([None, None, ("header", 0, SRC, DST), None, ("header", 0, SRC, DST), ("csbk", 0x3D, 0x00, [0x01, 0x23, 0x45, 0x67, 0x89, 0xAB, 0xCD, 0xEF])]
          + [x for _ in range(3) for x in ("voice", None, "voice-", None, "voice-", None, "voice-", None, "voice-", None, "voice-", None)]
          + [("term", 0, SRC, DST), None, None, None])
STREAM_START = 0.02


def test_stream(fs_ch: float, noise: float = 0.0, seed: int = 3, script=SCRIPT) -> np.ndarray:
    levels = base_station(script)
    n = int((STREAM_START + len(levels) / 4800.0 + 0.02) * fs_ch)
    return synth_theta(levels, fs_ch, n, STREAM_START, noise, seed)


FS, SECS, AMP = IM.FS, IM.SECS, IM.AMP
CAPTURE_START = 0.05
CAPTURE_CHANNELS = (("dmr", 200e3), ("voice", 600e3))


@functools.lru_cache(maxsize=1)
def capture() -> np.ndarray:
    """int16[n][2]: a model capture in ``ident_model``'s conventions (s16, 2.4 MS/s, 2 s, AMP 0.05, complex noise 30 dB under AMP
    in total, seed 11, DC 0.01): a DMR base channel at +200 kHz that sends SCRIPT and idles to the end, and an NFM voice channel
    at +600 kHz."""
    n = int(round(FS * SECS))
    t = np.arange(n) / FS
    rng = np.random.default_rng(11)
    sigma = AMP * 10.0 ** (-30.0 / 20.0) / math.sqrt(2.0)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    off = dict(CAPTURE_CHANNELS)
    car = lambda name: np.exp(2j * np.pi * ((off[name] * t) % 1.0))  # noqa: E731
    slots = int((SECS - CAPTURE_START) / 0.030) + 1
    levels = base_station(list(SCRIPT) + [None] * (slots - len(SCRIPT)))
    f = np.zeros(n, dtype=np.float64)
    idx = np.ceil((CAPTURE_START + np.arange(len(levels) + 1) / 4800.0) * FS - 1e-9).astype(np.int64)
    for lev, a, b in zip(levels, idx[:-1], idx[1:]):
        f[max(a, 0) : max(min(b, n), 0)] = lev * DEV
    x += (AMP / 2.0) * car("dmr") * K._fm_of(f)
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
    25's identification and this section's bursts and calls, per found channel."""
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
        dmr = None
        if named["rate"] == 4800 and named["plan"] is not None:
            pl = plan(d["plan"]["fs_ch"])
            dmr = decode_plane(named["v"], [h for h in named["kept"] if h[0] in (0, 1)], pl, k["keyed_from"])
        out.append(dict(described=d, keyed=k, named=named, dmr=dmr))
    return out


# ---- crafted words for the coders (the host test and the GPU shapes test share them) -----------------------------------------------


def crafted_burst(cc: int = 5, data_type: int = 3, info96=None, kind: int = 1, tc: int = 1, seed: int = 2) -> tuple:
    """(cach24, burst264) of a clean data burst whose payload is 96 seeded random bits unless given."""
    rng = np.random.default_rng(seed)
    info = rng.integers(0, 2, 96).tolist() if info96 is None else list(info96)
    return cach_bits(tc, rng), data_burst_bits(kind, cc, data_type, info)


def flipped(burst264, raw_positions=(), slot_positions=()) -> list:
    """``burst264`` with the payload bits ``raw_positions`` (0 .. 195, as sent) and the slot-type bits ``slot_positions`` (0 .. 19)
    flipped."""
    out = list(burst264)
    for p in raw_positions:
        out[PAYLOAD_BITS[p]] ^= 1
    for p in slot_positions:
        out[SLOT_TYPE_BITS[p]] ^= 1
    return out


def sent_position(r: int, c: int) -> int:
    """Where the bit of row r and column c of the matrix lies among the 196 bits as sent."""
    return (INTERLEAVE * (1 + 15 * r + c)) % 196


@functools.lru_cache(maxsize=1)
def coder_cases() -> dict:
    """name -> (the nine words, kind): the crafted words of the coder tests."""
    cach, burst = crafted_burst()
    out = {"clean": (words_of(cach, burst), 1)}
    for p in range(196):
        out[f"single-{p}"] = (words_of(cach, flipped(burst, [p])), 1)
    out["two-apart"] = (words_of(cach, flipped(burst, [sent_position(2, 3), sent_position(7, 11)])), 1)
    out["unmatched-column"] = (words_of(cach, flipped(burst, [sent_position(1, 4), sent_position(2, 4)])), 1)  # 1110 ^ 0111 = 1001
    # two rounds: the first pair of one column (rows in order) after which the oracle flips in two rounds and ends clean
    for c in range(15):
        for r1 in range(13):
            for r2 in range(r1 + 1, 13):
                if "two-rounds" not in out:
                    bad = flipped(burst, [sent_position(r1, c), sent_position(r2, c)])
                    status, _, rounds, _ = bptc_decode([bad[j] for j in PAYLOAD_BITS])
                    if status == 1 and rounds == 3:
                        out["two-rounds"] = (words_of(cach, flipped(burst, [sent_position(r1, c), sent_position(r2, c)])), 1)
    # a failure: the first seed whose 24 random flips leave the oracle with a syndrome
    for seed in range(100):
        at = np.random.default_rng(seed).choice(196, 24, replace=False).tolist()
        if "fails" not in out and bptc_decode([flipped(burst, at)[j] for j in PAYLOAD_BITS])[0] == 2:
            out["fails"] = (words_of(cach, flipped(burst, at)), 1)
    for p in range(20):
        out[f"slot-single-{p}"] = (words_of(cach, flipped(burst, slot_positions=[p])), 1)
    for trio in ((0, 1, 2), (3, 9, 19), (7, 8, 15), (0, 10, 19)):
        out["slot-triple-" + "-".join(map(str, trio))] = (words_of(cach, flipped(burst, slot_positions=trio)), 1)
    out["slot-four"] = (words_of(cach, flipped(burst, slot_positions=(1, 6, 12, 17))), 1)
    for j, p in enumerate(TACT_BITS):
        bad = list(cach)
        bad[p] ^= 1
        out[f"tact-{j}"] = (words_of(bad, burst), 1)
    rng = np.random.default_rng(9)
    out["voice-bs"] = (words_of(cach, voice_burst_bits(0, rng)), 0)
    out["voice-ms"] = (words_of(cach, voice_burst_bits(2, rng)), 2)
    out["data-ms"] = (words_of(cach, data_burst_bits(3, 15, 6, rng.integers(0, 2, 96).tolist())), 3)
    out["zeros"] = ([0] * 9, 1)
    out["ones"] = ([0xFFFFFFFF] * 9, 1)
    return out
