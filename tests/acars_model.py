"""ACARS model for the tests (a helper module, not a test file): the encoder (odd parity, CRC-16/KERMIT, the block layout
of ARINC 618 as far as DESIGN.md section 15 reads it), a 2400 bit/s MSK -> AM modulator to complex baseband with clock,
noise and tuning knobs, and a plain numpy oracle of DESIGN.md section 15 (stages 1-6).  The protocol constants are written
out here on their own, not imported from the package, so that the encoder checks the decoder."""
from __future__ import annotations

import math

import numpy as np

BAUD = 2400
CENTRE = 1800.0  # the MSK tones are 1200 Hz (the bit changes) and 2400 Hz (the bit stays)
MIN_SPS, MAX_SPS = 8.0, 400.0
TAP_SCALE = 256.0
PHASES = 8
Q_BITS = 15  # 0 <= q <= 2^15, the upper end only where emax lies within 2^-9 of 2^15 / 2^sh
SOH, STX, ETX, ETB, SYN, DEL, NAK = 0x01, 0x02, 0x03, 0x17, 0x16, 0x7F, 0x15
OPENER = bytes([0x2A, 0x16, 0x16, 0x01])  # * SYN SYN SOH with their (odd) parity bits
MIN_BODY, MAX_BODY = 13, 240  # bytes behind SOH up to and including ETX / ETB
CRC_POLY = 0x8408  # x^16 + x^12 + x^5 + 1, reflected


# ---- encoder -----------------------------------------------------------------------------------------------------------


def with_parity(c: int) -> int:
    """7-bit character -> 8 bits, bit 7 chosen so that the number of ones is odd."""
    c &= 0x7F
    return c | (0x80 if bin(c).count("1") % 2 == 0 else 0)


PARITY = bytes(with_parity(c) for c in range(128))


def crc16(data: bytes) -> int:
    """CRC-16/KERMIT: reflected 0x8408, init 0, no final xor."""
    reg = 0
    for byte in data:
        reg ^= byte
        for _ in range(8):
            reg = (reg >> 1) ^ CRC_POLY if reg & 1 else reg >> 1
    return reg


def body_bytes(mode: str, address: str, ack: str, label: str, block_id: str, text: str | None = None, *, etb: bool = False) -> bytes:
    """Mode .. ETX / ETB with parity bits: the bytes the check sequence covers."""
    assert len(mode) == 1 and len(address) == 7 and len(ack) == 1 and len(label) == 2 and len(block_id) == 1
    chars = (mode + address + ack + label + block_id).encode("ascii")
    if text is not None:
        chars += bytes([STX]) + text.encode("ascii")
    chars += bytes([ETB if etb else ETX])
    return bytes(PARITY[c] for c in chars)


def with_bcs(body: bytes) -> bytes:
    reg = crc16(body)
    return body + bytes([reg & 0xFF, reg >> 8])


def message_bytes(body: bytes, *, prekey: int = 16) -> bytes:
    """One transmission: pre-key characters of ones, + *, SYN SYN, SOH, the body, its check sequence, DEL."""
    return bytes([0xFF] * prekey) + bytes([PARITY[0x2B]]) + OPENER + with_bcs(body) + bytes([DEL])


def bits_of(data: bytes) -> np.ndarray:
    """Bytes -> bits, least significant first."""
    return np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8), bitorder="little")


def transitions(bits, first: int = 1) -> np.ndarray:
    """Bits -> transition symbols: 1 where a bit equals the one before it (``first`` in front of the stream)."""
    bits = np.asarray(bits, dtype=np.uint8)
    prev = np.concatenate([np.array([first], dtype=np.uint8), bits[:-1]])
    return (bits == prev).astype(np.uint8)


# ---- modulator ---------------------------------------------------------------------------------------------------------


def modulate(bits, fs: float, *, depth: float = 0.5, scale: float = 0.013, ppm: float = 0.0, sigma: float = 0.0, seed: int = 0,
             offset_hz: float = 0.0, lead: int = 2000, tail: int = 2000) -> np.ndarray:
    """Bits -> continuous-phase MSK audio (a bit that equals the one before it is one cycle of 2400 Hz, a bit that differs
    half a cycle of 1200 Hz; a one in front of the stream) -> AM at ``depth`` on a carrier of 1, ``offset_hz`` off tune, the
    bit clock ``ppm`` fast; ``lead`` / ``tail`` samples without a carrier around it; complex AWGN of ``sigma`` per component
    (against the carrier of 1) over everything; the whole at ``scale``.  complex64 at ``fs``."""
    same = transitions(bits).astype(np.int64)
    rate = BAUD * (1.0 + ppm * 1e-6)
    n = int(math.ceil(same.size * fs / rate))
    idx = np.minimum((np.arange(n, dtype=np.float64) * rate / fs).astype(np.int64), same.size - 1)
    tone = np.where(same[idx] == 1, 2400.0, 1200.0) * (1.0 + ppm * 1e-6)
    audio = np.cos(2.0 * np.pi * np.cumsum(tone) / fs)
    x = (1.0 + depth * audio) * np.exp(2j * np.pi * offset_hz * np.arange(n, dtype=np.float64) / fs)
    x = np.concatenate([np.zeros(lead, dtype=np.complex128), x, np.zeros(tail, dtype=np.complex128)])
    if sigma > 0.0:
        rng = np.random.default_rng(seed)
        x = x + sigma * (rng.normal(size=x.size) + 1j * rng.normal(size=x.size))
    return (scale * x).astype(np.complex64)


def voice_am(n: int, fs: float, *, sigma: float = 0.05, seed: int = 0, scale: float = 0.013) -> np.ndarray:
    """A carrier with voice-band AM (three drifting tones between 300 Hz and 3 kHz) and noise."""
    t = np.arange(n, dtype=np.float64) / fs
    audio = 0.3 * np.sin(2 * np.pi * (400.0 + 150.0 * t) * t) + 0.25 * np.sin(2 * np.pi * 1150.0 * t + 1.0) + 0.2 * np.sin(2 * np.pi * (2500.0 - 90.0 * t) * t)
    rng = np.random.default_rng(seed)
    x = (1.0 + audio) + sigma * (rng.normal(size=n) + 1j * rng.normal(size=n))
    return (scale * x).astype(np.complex64)


def noise_only(n: int, sigma: float, seed: int, scale: float = 0.013) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (scale * sigma * (rng.normal(size=n) + 1j * rng.normal(size=n))).astype(np.complex64)


# ---- oracle ------------------------------------------------------------------------------------------------------------


def plan(fs: float) -> dict:
    fs = float(fs)
    sps = fs / BAUD
    if not (MIN_SPS <= sps <= MAX_SPS):
        raise ValueError("sps out of range")
    L, W = int(np.rint(sps)), int(np.rint(fs / CENTRE))
    k = np.arange(W, dtype=np.float64)
    c = np.rint(TAP_SCALE * np.cos(2.0 * np.pi * CENTRE * k / fs)).astype(np.int64)
    s = np.rint(TAP_SCALE * np.sin(2.0 * np.pi * CENTRE * k / fs)).astype(np.int64)
    psi = 2.0 * np.pi * CENTRE * L / fs
    return dict(fs=fs, sps=sps, L=L, W=W, step=sps / 8.0, c=c, s=s, cr=int(np.rint(TAP_SCALE * np.cos(psi))), sr=int(np.rint(TAP_SCALE * np.sin(psi))))


def envelope(z) -> np.ndarray:
    """Stage 1: |z| in float32 as numpy forms it."""
    return np.abs(np.asarray(z, dtype=np.complex64)).astype(np.float32)


def shift_of(emax) -> int:
    """Stage 2: sh = 14 - floor(log2 emax) for a positive finite float."""
    m, ex = math.frexp(float(emax))  # emax = m 2^ex, 0.5 <= m < 1
    assert m > 0.0
    return 14 - (ex - 1)


def quantise(e, emax=None):
    """Stage 2 -> (q int32, sh, emax); (None, None, 0.0) for an all-zero (or empty) run."""
    e = np.asarray(e, dtype=np.float32)
    emax = np.float32(e.max(initial=0.0)) if emax is None else np.float32(emax)
    if not emax > 0.0:
        return None, None, np.float32(0.0)
    sh = shift_of(emax)
    q = np.rint(np.ldexp(e.astype(np.float64), sh))  # (a power of two: exact in float64; rint is half-even)
    assert q.min(initial=0) >= 0 and q.max(initial=0) <= 2 ** Q_BITS
    return q.astype(np.int32), sh, emax


def correlate(q, pl) -> tuple:
    """Stage 3 -> (I, Q) int64, and the int32 range check of the sums in front of the shift."""
    q = np.asarray(q, dtype=np.int64)
    si, sq = np.convolve(q, pl["c"])[: q.size], np.convolve(q, pl["s"])[: q.size]
    assert max(np.abs(si).max(initial=0), np.abs(sq).max(initial=0)) < 2 ** 31
    return si >> 8, sq >> 8


def detect(I, Q, pl) -> tuple:
    """Stage 3 -> (y int64, same uint8)."""
    L = pl["L"]
    Id, Qd = np.zeros_like(I), np.zeros_like(Q)
    Id[L:], Qd[L:] = I[: max(I.size - L, 0)], Q[: max(Q.size - L, 0)]
    y = pl["cr"] * (Q * Id - I * Qd) - pl["sr"] * (I * Id + Q * Qd)
    assert np.abs(y.astype(np.float64)).max(initial=0.0) < 2.0 ** 62
    return y, (y > 0).astype(np.uint8)


def instants(pl, p: int, n: int) -> np.ndarray:
    """Stage 4: the instants of phase p that lie inside a stream of n samples."""
    i = np.arange(int(n / pl["sps"]) + 3, dtype=np.float64)
    at = pl["W"] - 1 + np.rint((8.0 * i + p) * pl["step"]).astype(np.int64)
    return at[at < n]


def bit_streams(same, pl) -> list:
    """Stage 4 -> 8 (symbols uint8, instants) pairs."""
    same = np.asarray(same, dtype=np.uint8)
    out = []
    for p in range(PHASES):
        at = instants(pl, p, same.size)
        out.append((same[at], at))
    return out


def opener_symbols() -> np.ndarray:
    """The 31 transitions inside the 32 bits of the opener."""
    return transitions(bits_of(OPENER))[1:]


def openers(g) -> np.ndarray:
    """Positions s with g[s - 31 .. s - 1] the opener's transitions (31 <= s <= len(g))."""
    g = np.asarray(g, dtype=np.uint8)
    want = opener_symbols()
    if g.size < want.size:
        return np.zeros(0, dtype=np.int64)
    hit = np.ones(g.size - want.size + 1, dtype=bool)
    for k, v in enumerate(want):
        hit &= g[k : k + hit.size] == v
    return np.flatnonzero(hit) + want.size


def walk(g, s: int):
    """Stage 5 from an opened position -> (bytes body + BCS or None, reached ETX / ETB).  The bit in front of s is the last
    bit of SOH, a zero."""
    b, i, body = 0, int(s), bytearray()

    def byte_at(i, b):
        v = 0
        for k in range(8):
            b ^= 1 - int(g[i + k])
            v |= b << k
        return v, b

    while True:
        if i + 8 > len(g):
            return None, False
        v, b = byte_at(i, b)
        i += 8
        body.append(v)
        if v & 0x7F in (ETX, ETB):
            break
        if len(body) == MAX_BODY:
            return None, False
    if i + 16 > len(g):
        return None, True
    lo, b = byte_at(i, b)
    hi, b = byte_at(i + 8, b)
    if len(body) < MIN_BODY or crc16(bytes(body)) != (lo | (hi << 8)):
        return None, True
    return bytes(body) + bytes([lo, hi]), True


def frames_of(g) -> tuple:
    """Stage 5 on one symbol stream -> ([(s, bytes)] kept, candidates that reached ETX / ETB)."""
    kept, reached = [], 0
    for s in openers(g).tolist():
        got, end = walk(g, s)
        reached += int(end)
        if got is not None:
            kept.append((s, got))
    return kept, reached


def shown(data: bytes) -> str:
    return "".join(chr(c & 0x7F) if 0x20 <= (c & 0x7F) <= 0x7E else "�" for c in data)


def parse(raw: bytes) -> dict:
    """Stage 6 on one CRC-checked record (body + BCS)."""
    body = raw[:-2]
    out = dict(mode=shown(body[0:1]), address=shown(body[1:8]), ack=shown(body[8:9]), label=shown(body[9:11]), block_id=shown(body[11:12]),
               more=(body[-1] & 0x7F) == ETB, parity_errors=sum(1 for c in body if bin(c).count("1") % 2 == 0), raw=raw.hex(),
               text=None, msgno=None, flight=None)
    out["registration"] = out["address"].lstrip(".")
    if len(body) > 13 and body[12] & 0x7F == STX:
        text = shown(body[13:-1])
        if out["block_id"].isdigit() and len(text) >= 10:
            out["msgno"], out["flight"], text = text[:4], text[4:10], text[10:]
        out["text"] = text
    return out


def merge(records, L: int) -> list:
    """[(phase, s, instant, bytes)] -> [(instant, bytes, hits)]: sorted by instant; identical bytes whose start instants
    lie within L of the group's first are one message."""
    out = []
    for p, s, at, raw in sorted(records, key=lambda r: (r[2], r[0])):
        same = [grp for grp in out if grp[1] == raw and at - grp[0] <= L]
        if same:
            same[-1][2] += 1
        else:
            out.append([at, raw, 1])
    return [tuple(grp) for grp in out]


def oracle(e=None, fs: float = 96_000.0, *, q=None) -> dict:
    """Stages 2-6 from an envelope (or from given ``q``)."""
    pl = plan(fs)
    sh = emax = None
    if q is None:
        q, sh, emax = quantise(e)
        if q is None:
            return dict(q=None, sh=None, emax=emax, messages=[], records=[], reached=0)
    q = np.asarray(q, dtype=np.int32)
    I, Q = correlate(q, pl)
    y, same = detect(I, Q, pl)
    streams = bit_streams(same, pl)
    records, reached = [], 0
    for p, (g, at) in enumerate(streams):
        kept, r = frames_of(g)
        reached += r
        records += [(p, s, int(pl["W"] - 1 + np.rint((8.0 * s + p) * pl["step"])), raw) for s, raw in kept]
    records.sort(key=lambda r: (r[0], r[1]))
    messages = [dict(parse(raw), time_s=at / pl["fs"], hits=hits) for at, raw, hits in merge(records, pl["L"])]
    return dict(q=q, sh=sh, emax=emax, I=I, Q=Q, y=y, same=same, bits=[g for g, _ in streams], records=records, reached=reached, messages=messages)


def line(m: dict) -> str:
    parts = [m["address"], m["label"], m["block_id"]] + [m[k] for k in ("msgno", "flight", "text") if m[k]]
    return "ACARS " + " ".join(parts)


# ---- the stream of the round-trip tests (tests/test_acars_host.py, tests/test_gpu_acars.py) ------------------------------

RATES = [96_000.0, 10e6 / 104]
TEXT = "M01AXX0123" + "POS N49035W072017,1234,350,ETA 1312 /FB 0123 the quick brown fox jumps over the lazy dog. " * 2
FIRST = dict(mode="2", address=".N12345", ack="\x15", label="H1", block_id="2", text=TEXT)
SECOND = dict(mode="2", address=".D-ABCD", ack="A", label="Q0", block_id="S", text=None)


def two_message_stream(fs: float, sigma: float, ppm: float, seed: int = 1) -> np.ndarray:
    """Two transmissions in one stream: a downlink with text that ends in ETX, a block without text that ends in ETB."""
    a = modulate(bits_of(message_bytes(body_bytes(**FIRST))), fs, ppm=ppm, sigma=sigma, seed=seed)
    b = modulate(bits_of(message_bytes(body_bytes(**SECOND, etb=True))), fs, ppm=ppm, sigma=sigma, seed=seed + 1)
    return np.concatenate([a, b])


def check_two_messages(msgs) -> None:
    """``msgs``: dicts (the oracle's) or AcarsMessage objects."""
    get = (lambda m, k: m[k]) if isinstance(msgs[0], dict) else getattr
    assert len(msgs) == 2
    one, two = msgs
    assert [get(one, k) for k in ("mode", "address", "registration", "ack", "label", "block_id", "msgno", "flight", "text", "more", "parity_errors")] == [
        "2", ".N12345", "N12345", "�", "H1", "2", "M01A", "XX0123", TEXT[10:], False, 0]
    assert [get(two, k) for k in ("mode", "address", "registration", "ack", "label", "block_id", "msgno", "flight", "text", "more", "parity_errors")] == [
        "2", ".D-ABCD", "D-ABCD", "A", "Q0", "S", None, None, None, True, 0]
    assert get(one, "hits") >= 1 and get(two, "hits") >= 1 and get(one, "time_s") < get(two, "time_s")


# ---- crafted inputs for the edge-shape tests ---------------------------------------------------------------------------


def square_wave(n: int, fs: float, emax: float = 1.0, phase: float = 0.0) -> np.ndarray:
    """A full-scale 0 / emax square wave at 1800 Hz (float32): the largest correlator sums an envelope can give."""
    k = np.arange(n, dtype=np.float64)
    return np.where(np.cos(2.0 * np.pi * CENTRE * k / fs + phase) > 0.0, emax, 0.0).astype(np.float32)


def hand_made_streams() -> list:
    """(name, symbol row, symbols that exist, kept frames expected): the walker's edge cases.  Where fewer symbols exist than
    the row holds, the row goes on with the symbols that would have completed the block, which the walker must not read."""
    body = body_bytes("2", ".N12345", "\x15", "H1", "2", "M01AXX0123hello, world")
    short = body_bytes("2", ".D-ABCD", "A", "_\x7f", "S", None, etb=True)
    assert len(short) == MIN_BODY

    def row(b, *, first=1, lead=8, damage=None):
        data = bytes([0xFF] * 2) + bytes([PARITY[0x2B]]) + OPENER + (with_bcs(b) if damage is None else damage(with_bcs(b))) + bytes([DEL])
        bits = np.concatenate([np.ones(lead, dtype=np.uint8), bits_of(data)])
        if first == 0:
            bits = 1 - bits
        return transitions(bits, first)

    at = 8 + 8 * 7  # the position behind SOH in a row with lead = 8
    out = [("plain", row(body), None, 1), ("inverted", row(body, first=0), None, 1), ("no text, ETB", row(short), None, 1)]
    # a check sequence that holds an ETX: the text is searched for one
    for k in range(4096):
        b = body_bytes("2", ".N12345", "A", "Q0", "3", f"M{k:03d}XX0123")
        reg = crc16(b)
        if ETX in (reg & 0x7F, (reg >> 8) & 0x7F):
            out.append(("ETX inside the BCS", row(b), None, 1))
            break
    else:
        raise AssertionError("no check sequence with an ETX found")
    out.append(("12 bytes", row(short[:11] + short[12:]), None, 0))
    out.append(("13 bytes", row(short), None, 1))
    fill = "".join(chr(0x20 + (7 * k) % 0x5F) for k in range(400))
    long240 = body_bytes("2", ".N12345", "A", "H1", "4", fill[: MAX_BODY - 14])
    long241 = body_bytes("2", ".N12345", "A", "H1", "4", fill[: MAX_BODY - 13])
    assert (len(long240), len(long241)) == (240, 241)
    out += [("240 bytes", row(long240), None, 1), ("241 bytes", row(long241), None, 0)]
    r = row(body)
    end = at + 8 * (len(body) + 2)
    out += [("ends inside the body", r, at + 8 * 20 + 3, 0), ("ends inside the BCS", r, end - 5, 0), ("ends behind the BCS", r, end, 1),
            ("ends on the opener", r, at, 0), ("shorter than the opener", r, 30, 0), ("empty", r, 0, 0)]
    out.append(("wrong BCS", row(body, damage=lambda d: d[:-1] + bytes([d[-1] ^ 0x10])), None, 0))
    out.append(("damaged body", row(body, damage=lambda d: d[:20] + bytes([d[20] ^ 0x04]) + d[21:]), None, 0))
    return [(name, np.asarray(g, dtype=np.uint8), int(g.size if count is None else count), kept) for name, g, count, kept in out]
