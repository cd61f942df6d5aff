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


# ---- edge shapes (tests/test_gpu_acars_shapes.py, tests/test_acars_shapes_host.py) -----------------------------------------
#
# Case tables, block oracles and numpy stand-ins of the four entry points that follow csrc/acars.hip's launch arithmetic and
# can be broken one way at a time.  The ``check_*`` functions hold the comparisons; they take the entry point as a callable,
# so the GPU file passes the device call and the host file the stand-in.

SENT = -7_777_777  # what untouched int32 / int64 output words hold
SENT8 = 0xAA  # ... and untouched bytes
GUARD = 16  # sentinel elements behind every output
TILE, RUN = 2048, 8  # SB_TILE, SB_RUN
MAX_WINDOW, MAX_DELAY = 536, 400
MAX_N, MAX_NBITS = 1 << 40, 1 << 37
SLOT_BYTES = 244
HOSTILE_F32 = np.array([np.nan, np.inf, -np.inf, 3.0e38], dtype=np.float32)
HOSTILE_U8 = np.array([0xFF, 0x80, 0xFE, 0x7F], dtype=np.uint8)
DETECT_SHAPES = ((1, 8), (2, 8), (8, 9), (9, 15), (16, 16), (17, 400), (255, 8), (536, 8), (536, 400))  # (W, L); none is a plan's pair
DETECT_CRSR = ((0, -256), (256, 0), (-256, 256), (181, -181), (1, 0))
DETECT_OUTPUTS = ("qIQy", "", "q", "I", "Q", "y", "Iy")
DTYPES = dict(q=np.int32, I=np.int32, Q=np.int32, y=np.int64, same=np.uint8)
FULL_SUM = 2 ** 15 * 256 * 255  # 2 139 095 040: every settled sum of the full-scale cases


def front_of(dtype) -> int:
    """Elements in front of every view: 16 bytes at least and 4 elements at least, so that offset 0 stays 16-byte aligned."""
    return max(4, 16 // np.dtype(dtype).itemsize)


def sentinel_of(dtype):
    return {1: SENT8, 2: 0xAAAA}.get(np.dtype(dtype).itemsize, SENT)


def wrap32(x):
    return ((np.asarray(x, dtype=np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def s24(x):
    """The low 24 bits, sign-extended: what v_mad_i32_i24 reads of an operand."""
    return ((np.asarray(x, dtype=np.int64) & 0xFFFFFF) ^ 0x800000) - 0x800000


def s16(x):
    return ((np.asarray(x, dtype=np.int64) & 0xFFFF) ^ 0x8000) - 0x8000


def round8(v: int) -> int:
    return (v + RUN - 1) // RUN * RUN


def detect_lengths(L: int) -> tuple:
    T = TILE - round8(L)
    return (7, 8, 9, T - 1, T, T + 1, 2 * T + 3)


def detect_offsets(k: int) -> dict:
    """Element offsets of the views inside their 16-byte aligned allocations for case k: ``same`` goes through all eight byte
    offsets, the others through theirs, not in step."""
    so = k % 8
    return dict(e=(3 * so + 1 + k // 8) % 4, q=(so + 1) % 4, I=(so + 2 + k // 8) % 4, Q=(3 * so) % 4, y=(so // 2 + k // 8) % 2, same=so)


def shape_taps(W: int, seed: int) -> np.ndarray:
    """int16[2][W] in -256 .. 256, arbitrary (not symmetric), both ends of both tables at +-256."""
    t = np.random.default_rng(seed).integers(-256, 257, size=(2, W)).astype(np.int16)
    t[0, 0], t[1, 0] = 256, -256
    if W > 1:
        t[0, -1], t[1, -1] = -256, 256
    return t


def tap_sums_ok(taps) -> bool:
    """The header's bound: a table's positive taps and its negative taps each sum to less than 65 536."""
    t = np.asarray(taps, dtype=np.int64)
    return all(int(np.maximum(r, 0).sum()) < 65_536 and int(np.maximum(-r, 0).sum()) < 65_536 for r in t) and int(np.abs(t).max()) <= 256


def detect_plane(n: int, seed: int) -> np.ndarray:
    """Random float32 in 0 .. 0.25, the largest the float below 0.25 (so sh = 17 and the largest q is 2^15); the first values
    sit on k + 1/2 in units of 2^-17 for even and odd k."""
    rng = np.random.default_rng(seed)
    e = rng.uniform(0.0, 0.25, n).astype(np.float32)
    top = np.nextafter(np.float32(0.25), np.float32(0.0))
    e = np.minimum(e, top)
    ties = ((np.arange(0, 6, dtype=np.float64) + 0.5) / 2.0 ** 17).astype(np.float32)
    e[: min(n, ties.size)] = ties[: min(n, ties.size)]
    e[(seed * 7) % n] = top
    return e


def detect_cases(W: int, L: int) -> list:
    """dict(name, W, L, n, taps, e, sh | None, cr, sr, outputs, offsets, full): random taps at every n x ``same`` offset, the
    optional outputs and (cr, sr) cycling; "all NULL at same offset 3"; and at W = 255 the two full-scale sets (all 2 . 255
    taps +256 / -256, e held at the float below 0.25, cr = sr = +-256)."""
    out = []
    for ni, n in enumerate(detect_lengths(L)):
        for so in range(8):
            k = 8 * ni + so
            seed = 100_000 * W + 100 * L + k
            cr, sr = DETECT_CRSR[k % len(DETECT_CRSR)]
            out.append(dict(name=f"W {W} L {L} n {n} case {k}", W=W, L=L, n=n, taps=shape_taps(W, seed), e=detect_plane(n, seed + 1), sh=None, cr=cr, sr=sr,
                            outputs=DETECT_OUTPUTS[k % len(DETECT_OUTPUTS)], offsets=detect_offsets(k), full=0))
    T = TILE - round8(L)
    out.append(dict(name=f"W {W} L {L} n {T + 1}: every optional output NULL, same at byte offset 3", W=W, L=L, n=T + 1, taps=shape_taps(W, 5), e=detect_plane(T + 1, 6),
                    sh=None, cr=181, sr=-181, outputs="", offsets=dict(detect_offsets(3), same=3), full=0))
    if W == 255:
        top = np.nextafter(np.float32(0.25), np.float32(0.0))
        for sign in (1, -1):
            for j, n in enumerate((300, T + 1, 2 * T + 3)):
                crsr = 256 if (j + (sign < 0)) % 2 == 0 else -256
                out.append(dict(name=f"W {W} L {L} n {n}: all taps {256 * sign}, q = 2^15 everywhere, cr = sr = {crsr}", W=W, L=L, n=n,
                                taps=np.full((2, W), 256 * sign, dtype=np.int16), e=np.full(n, top, dtype=np.float32), sh=None, cr=crsr, sr=crsr,
                                outputs="qIQy", offsets=detect_offsets(j + 3 * (sign < 0)), full=sign))
    return out


def quantiser_cases() -> list:
    """Detector cases that are about q: k + 1/2 for even and odd k, 2^15 - 1/2 and the floats either side of it; and emax =
    2^-149 (sh = 163), 2^-126 (sh = 140) and 3.4028235e38 (sh = -113) with the rest of the plane spread over the 15 bits below
    emax.  W = 9, L = 15, n = T + 1."""
    W, L = 9, 15
    n = TILE - round8(L) + 1
    rng = np.random.default_rng(77)
    out = []
    top = np.nextafter(np.float32(0.25), np.float32(0.0))
    half = np.float32(32767.5 / 2.0 ** 17)
    e = ((rng.integers(0, 2 ** 15, size=n).astype(np.float64) + 0.5) / 2.0 ** 17).astype(np.float32)  # every value a tie
    e[:6] = ((np.arange(6) + 0.5) / 2.0 ** 17).astype(np.float32)
    e[6:10] = [half, np.nextafter(half, np.float32(0.0)), np.nextafter(half, np.float32(1.0)), top]
    out.append(("ties", e, 17))
    tiny = np.float32(2.0 ** -149)
    e = np.where(rng.integers(0, 2, size=n) == 1, tiny, np.float32(0.0)).astype(np.float32)
    e[5] = tiny
    out.append(("emax 2^-149", e, 163))
    k = rng.integers(0, 2 ** 23 + 1, size=n)
    k[:8] = [256, 768, 512 * 5 + 256, 2 ** 23, 2 ** 23 - 256, 255, 257, 0]  # k 2^-9: ties at 1/2, 3/2, 11/2; emax; 2^14 - 1/2
    e = (k.astype(np.float64) * 2.0 ** -149).astype(np.float32)
    out.append(("emax 2^-126", e, 140))
    big = np.float32(3.4028235e38)
    e = (rng.uniform(0.0, 1.0, size=n) * float(big)).astype(np.float32)
    e[3] = big
    out.append(("emax 3.4028235e38", e, -113))
    cases = []
    for j, (name, e, sh) in enumerate(out):
        assert e.dtype == np.float32 and e.size == n and shift_of(e.max()) == sh, name
        cases.append(dict(name=f"quantiser, {name}", W=W, L=L, n=n, taps=shape_taps(W, 900 + j), e=e, sh=sh, cr=181, sr=-181, outputs="qIQy",
                          offsets=detect_offsets(2 * j + 1), full=0))
    return cases


def detect_block(case: dict) -> dict:
    """The oracle on one case -> q, I, Q, y, same, the raw sums and sh; the table's own preconditions asserted."""
    W, L, taps = case["W"], case["L"], np.asarray(case["taps"], dtype=np.int64)
    assert taps.shape == (2, W) and tap_sums_ok(taps), case["name"]
    q, sh, _ = quantise(case["e"])
    assert case["sh"] in (None, sh) and -160 <= sh <= 200
    pl = dict(W=W, L=L, c=taps[0], s=taps[1], cr=case["cr"], sr=case["sr"])
    I, Q = correlate(q, pl)
    y, same = detect(I, Q, pl)
    sums = np.convolve(q.astype(np.int64), taps[0])[: q.size]
    assert np.abs(I).max(initial=0) < 2 ** 23 and np.abs(Q).max(initial=0) < 2 ** 23 and np.abs(y.astype(np.float64)).max(initial=0.0) < 2.0 ** 57
    if case["full"]:
        assert (q == 2 ** 15).all() and (sums[W - 1 :] == case["full"] * FULL_SUM).all() and FULL_SUM == 2_139_095_040 < 2 ** 31
        assert (I[W - 1 :] == case["full"] * 8_355_840).all() and int(np.abs(y).max()) == 2 * 256 * 8_355_840 ** 2
    return dict(q=q, I=I.astype(np.int32), Q=Q.astype(np.int32), y=y, same=same, sh=sh, sums=sums)


def check_detect(case: dict, call) -> None:
    """``call(e_alloc, e_at, n, sh, W, L, taps_alloc, cr, sr, bufs, ats) -> bufs`` after the call: ``bufs`` maps "q", "I",
    "Q", "y" (where asked for) and "same" to allocations filled with sentinels, ``ats`` to the element index of each view."""
    n = case["n"]
    want = detect_block(case)
    offs = case["offsets"]
    e_at = front_of(np.float32) + offs["e"]
    e_alloc = np.concatenate([np.resize(HOSTILE_F32, e_at), case["e"], HOSTILE_F32])
    taps_alloc = np.concatenate([np.asarray(case["taps"], dtype=np.int16).reshape(-1), np.full(8, 32767, dtype=np.int16)])
    keys = list(case["outputs"]) + ["same"]
    ats = {k: front_of(DTYPES[k]) + offs[k] for k in keys}
    bufs = {k: np.full(ats[k] + n + GUARD, sentinel_of(DTYPES[k]), dtype=DTYPES[k]) for k in keys}
    bufs = call(e_alloc, e_at, n, want["sh"], case["W"], case["L"], taps_alloc, case["cr"], case["sr"], bufs, ats)
    assert set(bufs) == set(keys)
    for k in keys:
        got, a, sent = bufs[k], ats[k], sentinel_of(DTYPES[k])
        np.testing.assert_array_equal(got[a : a + n], want[k], err_msg=f"{k}: {case['name']}")
        assert (got[:a] == sent).all() and (got[a + n :] == sent).all(), f"{k} guards: {case['name']}"


def kernel_detect(e, n: int, sh: int, W: int, L: int, taps, cr: int, sr: int, outs: dict, same_alloc, same_at: int, *, operands16: bool = False,
                  y32: bool = False, wide_store_always: bool = False) -> None:
    """k_acars_detect and its launch in numpy, workgroup by workgroup: the staged image of q (zeros in front of the stream and
    behind it), the taps behind tap 0 zero-padded to H, the Lh repeated evaluations in front of a workgroup's outputs, 24-bit
    operands with an int32 accumulator, I and Q by index into the workgroup's 2048, and both flag-store paths -- 8 bytes at
    once where the whole run lies inside n and ``same`` is 8-byte aligned, byte by byte otherwise.  ``outs``: the views of
    "q", "I", "Q", "y" that are given; ``same_alloc`` is the allocation (16-byte aligned), ``same_at`` the view's index in it.
    Breaks: ``operands16`` reads the multiply's operands 16 bits wide (q = 2^15 turns negative); ``y32`` forms y in int32;
    ``wide_store_always`` takes the 8-byte store whatever the address, which a memory path that ignores the low address bits
    rounds down to a multiple of 8."""
    H, Lh = round8(W - 1), round8(L)
    T = TILE - Lh
    ext = s16 if operands16 else s24
    taps = np.asarray(taps, dtype=np.int64).reshape(-1)[: 2 * W].reshape(2, W)
    tp = np.zeros((2, 1 + H), dtype=np.int64)
    tp[:, :W] = taps
    q_all = np.rint(np.ldexp(np.asarray(e[:n], dtype=np.float64), sh)).astype(np.int64)
    aligned = same_at % 8 == 0
    for b in range(-(-n // T)):
        out0 = b * T
        A = out0 - Lh
        i = np.arange(H + TILE)
        a = A - H + i
        img = np.zeros(H + TILE, dtype=np.int64)
        ins = (a >= 0) & (a < n)
        img[ins] = q_all[a[ins]]
        if "q" in outs:
            own = ins & (i >= H + Lh)
            outs["q"][a[own]] = img[own]
        a0 = A + RUN * np.arange(TILE // RUN)
        live = np.repeat((a0 < n) & (a0 + RUN > 0), RUN)
        acc = [np.where(live, wrap32(np.convolve(ext(img), ext(tp[f]))[H : H + TILE]), 0) >> 8 for f in range(2)]  # the workgroup's 2048 I and Q
        for tid in range(Lh // RUN, TILE // RUN):
            i0 = tid * RUN
            if a0[tid] >= n:
                break
            r = np.arange(RUN)
            I, Q, Id, Qd = acc[0][i0 + r], acc[1][i0 + r], acc[0][i0 + r - L], acc[1][i0 + r - L]
            if y32:
                y = wrap32(cr * wrap32(wrap32(Q * Id) - wrap32(I * Qd)) - sr * wrap32(wrap32(I * Id) + wrap32(Q * Qd)))
            else:
                y = cr * (Q * Id - I * Qd) - sr * (I * Id + Q * Qd)
            flag = (y > 0).astype(np.uint8)
            ok = a0[tid] + r < n
            for key, v in (("I", I), ("Q", Q), ("y", y)):
                if key in outs:
                    outs[key][a0[tid] + r[ok]] = v[ok]
            if ok.all() and (aligned or wide_store_always):
                at = (same_at + a0[tid]) // RUN * RUN
                same_alloc[at : at + RUN] = flag
            else:
                same_alloc[same_at + a0[tid] + r[ok]] = flag[ok]


def window_ok(W) -> bool:
    return 1 <= W <= MAX_WINDOW


def step_ok(step) -> bool:
    return 1.0 <= step <= MAX_DELAY / 8.0  # (false for a NaN)


def entry_detect(e_alloc, e_at, n, sh, W, L, taps_alloc, cr, sr, bufs, ats, **breaks):
    """iqa_acars_detect's checks in front of ``kernel_detect``; None stands for a NULL pointer."""
    if n < 0:
        raise ValueError("negative length")
    if not window_ok(W):
        raise ValueError("window must be 1 .. IQA_ACARS_MAX_WINDOW")
    if not 8 <= L <= MAX_DELAY:
        raise ValueError("delay must be 8 .. IQA_ACARS_MAX_SPS")
    if not -160 <= sh <= 200:
        raise ValueError("shift out of range")
    if max(abs(cr), abs(sr)) > 256:
        raise ValueError("|cr|, |sr| must be <= 256")
    if n == 0:
        return bufs
    if e_alloc is None or taps_alloc is None or bufs.get("same") is None:
        raise ValueError("NULL device pointer")
    if n > MAX_N:
        raise ValueError("length out of range")
    outs = {k: bufs[k][ats[k] :] for k in bufs if k != "same"}
    kernel_detect(e_alloc[e_at:], n, sh, W, L, taps_alloc, cr, sr, outs, bufs["same"], ats["same"], **breaks)
    return bufs


def detect_refusals() -> list:
    """(what, n, sh, W, L, cr, sr, e?, taps?, same?, message)."""
    ok = (64, 17, 53, 40, 0, -256)

    def row(what, message, n=64, sh=17, W=53, L=40, cr=0, sr=-256, e=True, taps=True, same=True):
        return (what, n, sh, W, L, cr, sr, e, taps, same, message)

    assert row("", "")[1:7] == ok
    return [row("negative n", "negative", n=-1), row("window 0", "window must be", W=0), row("window 537", "window must be", W=MAX_WINDOW + 1),
            row("delay 7", "delay must be", L=7), row("delay 401", "delay must be", L=MAX_DELAY + 1), row("shift -161", "shift out of range", sh=-161),
            row("shift 201", "shift out of range", sh=201), row("cr 257", "must be <= 256", cr=257), row("sr -257", "must be <= 256", sr=-257),
            row("NULL e", "NULL", e=False), row("NULL taps", "NULL", taps=False), row("NULL same", "NULL", same=False),
            row("n above 2^40", "out of range", n=MAX_N + 1)]


# -- the maximum


MAX_LENGTHS = (1, 255, 256, 257, 4_194_303, 4_194_304, 4_194_305)  # 1024 . 256 . 16 = 4 194 304: behind it a thread takes a 17th round
MAX_GRID, MAX_THREADS = 1024, 256


def max_cases() -> list:
    """dict(name, n, at, kind, offset): the maximum alone at index 0, at n - 1 and (last length) at 4 194 304, the only element
    read in a 17th round; a plane of denormals only (2^-148 against 2^-149 elsewhere, and 2^-149 against zeros), and
    3.4028235e38 against random values; ``e`` a view at element offsets 0 .. 3."""
    out, k = [], 0
    for n in MAX_LENGTHS:
        spots = sorted({0, n - 1})
        for at in spots:
            kinds = ("denormal", "largest") if n < 4_000_000 else (("denormal",) if at == 0 else ("largest",))
            for kind in kinds + (("smallest",) if n in (257, 4_194_305) and at == n - 1 else ()):
                out.append(dict(name=f"n {n} maximum at {at}, {kind}, e offset {(k + 1) % 4}", n=n, at=at, kind=kind, offset=(k + 1) % 4))
                k += 1
    return out


def max_plane(case: dict) -> np.ndarray:
    n, kind = case["n"], case["kind"]
    if kind == "denormal":
        e = np.full(n, 1, dtype=np.uint32).view(np.float32)  # 2^-149
        e[case["at"]] = np.uint32(2).view(np.float32)  # 2^-148
    elif kind == "smallest":
        e = np.zeros(n, dtype=np.float32)
        e[case["at"]] = np.uint32(1).view(np.float32)
    else:
        e = np.resize(np.random.default_rng(n).uniform(0.0, 1.0e30, 4099).astype(np.float32), n)
        e[case["at"]] = np.float32(3.4028235e38)
    return e


def check_max(case: dict, call) -> None:
    """``call(e_alloc, e_at, n, out_alloc, out_at) -> out_alloc`` (uint32 numpy: the float's bit pattern)."""
    e = max_plane(case)
    assert int((e == e.max()).sum()) == 1 and int(np.argmax(e)) == case["at"] and (e >= 0).all()
    e_at = front_of(np.float32) + case["offset"]
    e_alloc = np.concatenate([np.resize(HOSTILE_F32, e_at), e, HOSTILE_F32])
    word = np.uint32(0xDEADBEEF)
    out = call(e_alloc, e_at, case["n"], np.full(4 + 1 + GUARD, word, dtype=np.uint32), 4)
    assert int(out[4]) == int(e.max().view(np.uint32)), case["name"]
    assert (out[:4] == word).all() and (out[5:] == word).all(), case["name"]


def max_reader(n: int, index: int) -> tuple:
    """(block, thread, round) that reads e[index] in k_acars_max's grid for a plane of n."""
    blocks = min(-(-n // (MAX_THREADS * 16)), MAX_GRID)
    stride = blocks * MAX_THREADS
    return (index % stride) // MAX_THREADS, index % MAX_THREADS, index // stride


def entry_max(e_alloc, e_at, n, out_alloc, out_at):
    if n < 0:
        raise ValueError("negative length")
    if out_alloc is None:
        raise ValueError("NULL device pointer")
    if n > MAX_N:
        raise ValueError("length out of range")
    if n > 0 and e_alloc is None:
        raise ValueError("NULL device pointer")
    bits = np.ascontiguousarray(e_alloc[e_at : e_at + n]).view(np.uint32) if n else np.zeros(0, dtype=np.uint32)
    out_alloc[out_at] = bits.max(initial=0)  # non-negative floats order as their bit patterns do
    return out_alloc


def max_refusals() -> list:
    """(what, n, e?, max_out?, message)."""
    return [("negative n", -1, True, True, "negative"), ("NULL max_out", 64, True, False, "NULL"), ("n above 2^40", MAX_N + 1, True, True, "out of range"),
            ("NULL e", 64, False, True, "NULL")]


# -- symbols


BIT_SHAPES = ((1.0, 1), (1.5, 16), (1.25, 11), (5.0, 53), (5.0078125, 54), (50.0, 536))  # (step, W)
BIT_COUNTS = (0, 1, 255, 256, 257)


def bits_block(same, n: int, W: int, step: float, nbits: int, *, floor_half: bool = False) -> tuple:
    """(bits uint8[8, nbits], instants int64[8, nbits], ties bool[8, nbits]); break: ``floor_half`` takes floor(x + 0.5)."""
    x = (8.0 * np.arange(nbits, dtype=np.float64)[None, :] + np.arange(PHASES, dtype=np.float64)[:, None]) * step
    at = W - 1 + (np.floor(x + 0.5) if floor_half else np.rint(x)).astype(np.int64)
    g = np.zeros((PHASES, nbits), dtype=np.uint8)
    ok = at < n
    g[ok] = np.asarray(same)[at[ok]]
    return g, at, np.mod(x, 1.0) == 0.5


def bit_cases() -> list:
    """dict(name, step, W, n, nbits): every count at every shape on planes that end on, one before and one behind the last
    instant, and a plane of W - 2 samples (every symbol reads zero)."""
    out = []
    for step, W in BIT_SHAPES:
        for nbits in BIT_COUNTS:
            last = W - 1 + int(np.rint((8.0 * max(nbits - 1, 0) + 7.0) * step))
            for n in (last + 1, last, last + 2) if nbits else (W + 3,):
                out.append(dict(name=f"step {step} W {W} nbits {nbits} n {n}", step=step, W=W, n=n, nbits=nbits, last=last))
        if W > 2:
            out.append(dict(name=f"step {step} W {W}: a plane of W - 2 samples", step=step, W=W, n=W - 2, nbits=256, last=None))
    return out


def check_bits(case: dict, call, stats: dict | None = None) -> None:
    """``call(same_alloc, n, W, step, nbits, out_buf) -> out_buf`` (uint8 numpy).  The plane is random with its last 80 samples
    ones, so that an instant inside the plane and one behind it read differently; behind n lie bytes that are no symbol."""
    step, W, n, nbits = case["step"], case["W"], case["n"], case["nbits"]
    same = np.random.default_rng(n + nbits).integers(0, 2, size=n).astype(np.uint8)
    same[max(n - 80, 0) :] = 1
    want, at, ties = bits_block(same, n, W, step, nbits)
    if case["last"] is None:
        assert (want == 0).all() and at.min() == W - 1 > n - 1
    elif nbits:
        assert at.max() == case["last"] and int(want[7, -1]) == int(n > case["last"]) and (nbits < 2 or want[6, -1] == 1), case["name"]
    if stats is not None and nbits:
        x = (8.0 * np.arange(nbits)[None, :] + np.arange(PHASES)[:, None]) * step
        s = stats.setdefault(step, dict(ties=0, down=0))
        s["ties"] += int(ties.sum())
        s["down"] += int((ties & (np.rint(x) != np.floor(x + 0.5))).sum())
    buf = np.full(PHASES * nbits + GUARD, SENT8, dtype=np.uint8)
    buf = call(np.concatenate([same, HOSTILE_U8]), n, W, step, nbits, buf)
    np.testing.assert_array_equal(buf[: PHASES * nbits].reshape(PHASES, nbits), want, err_msg=case["name"])
    assert (buf[PHASES * nbits :] == SENT8).all(), case["name"]


def entry_bits(same, n, W, step, nbits, out, **breaks):
    if n < 0 or nbits < 0:
        raise ValueError("negative length")
    if not window_ok(W):
        raise ValueError("window must be 1 .. IQA_ACARS_MAX_WINDOW")
    if not step_ok(step):
        raise ValueError("step must be sps / 8 with 8 <= sps <= IQA_ACARS_MAX_SPS")
    if nbits == 0:
        return out
    if out is None or (n > 0 and same is None):
        raise ValueError("NULL device pointer")
    if n > MAX_N or nbits > MAX_NBITS:
        raise ValueError("length out of range")
    out[: PHASES * nbits] = bits_block(same, n, W, step, nbits, **breaks)[0].reshape(-1)
    return out


def bit_refusals() -> list:
    """(what, n, W, step, nbits, same?, out?, message)."""
    return [("negative n", -1, 53, 5.0, 8, True, True, "negative"), ("negative nbits", 64, 53, 5.0, -1, True, True, "negative"),
            ("window 0", 64, 0, 5.0, 8, True, True, "window must be"), ("window 537", 64, MAX_WINDOW + 1, 5.0, 8, True, True, "window must be"),
            ("step below 1", 64, 53, 0.999, 8, True, True, "step must be"), ("step above 50", 64, 53, 50.01, 8, True, True, "step must be"),
            ("step not a number", 64, 53, float("nan"), 8, True, True, "step must be"), ("NULL same", 64, 53, 5.0, 8, False, True, "NULL"),
            ("NULL bits", 64, 53, 5.0, 8, True, False, "NULL"), ("n above 2^40", MAX_N + 1, 53, 5.0, 8, True, True, "out of range"),
            ("nbits above 2^37", 64, 53, 5.0, MAX_NBITS + 1, True, True, "out of range")]


# -- frames


FRAME_W, FRAME_STEP = 53, 5.0


def _padded(g, nbits: int) -> np.ndarray:
    g = np.asarray(g, dtype=np.uint8)
    assert g.size <= nbits
    return np.concatenate([g, np.ones(nbits - g.size, dtype=np.uint8)])


def early_row() -> np.ndarray:
    """A row that begins with the opener's second symbol: the 31 transitions inside the opener, then the block.  The
    candidate opens at s = 31, the first legal position."""
    body = body_bytes("2", ".N12345", "\x15", "H1", "2", "M01AXX0123hello, world")
    return transitions(bits_of(OPENER + with_bcs(body) + bytes([DEL])))[1:]


def frame_scenarios() -> list:
    """dict(name, planes uint8[8, nbits], count_of[8], kept[8]): eight different rows and counts in one call.
    "counts": nbits, 0, 30, 31, 32 (the opener's last symbol at count - 1 = 30, so s = nb: the walk ends at once although the
    row goes on with the whole block), "ends inside the BCS", "ends behind the BCS", nbits; the rows of phases 2, 3, 4 and 7
    open at s = 31.  "walks k": the hand-made streams of the walker test, eight per call, each with its own count."""
    hand = hand_made_streams()
    by_name = {name: (g, count, kept) for name, g, count, kept in hand}
    plain, early = by_name["plain"][0], early_row()
    inside, behind = by_name["ends inside the BCS"][1], by_name["ends behind the BCS"][1]
    nbits = int(plain.size) + 5
    counts = [(plain, nbits, 1), (plain, 0, 0), (early, 30, 0), (early, 31, 0), (early, 32, 0), (plain, inside, 0), (plain, behind, 1), (early, nbits, 1)]
    out = [dict(name="counts", rows=counts)]
    for k in range(0, len(hand), 8):
        rows = [(g, count, kept) for _, g, count, kept in (hand[k : k + 8] + hand[:8])[:8]]
        out.append(dict(name=f"walks {k // 8}", rows=rows))
    for sc in out:
        rows = sc.pop("rows")
        nb = max(int(r[0].size) for r in rows) + (5 if sc["name"] == "counts" else 0)
        sc.update(planes=np.stack([_padded(r[0], nb) for r in rows]), count_of=[int(min(r[1], nb)) for r in rows], kept=[int(r[2]) for r in rows])
    return out


def instant_of(W: int, step: float, s: int, p: int) -> int:
    return W - 1 + int(np.rint(float(8 * s + p) * step))


def frames_block(planes, count_of, W: int = FRAME_W, step: float = FRAME_STEP) -> tuple:
    """(sorted [(phase, s, instant, bytes)], kept blocks, candidates that reached ETX / ETB) of eight rows with their counts."""
    rows, reached = [], 0
    for p in range(PHASES):
        kept, r = frames_of(np.asarray(planes[p][: count_of[p]], dtype=np.uint8))
        reached += r
        rows += [(p, int(s), instant_of(W, step, int(s), p), raw) for s, raw in kept]
    return sorted(rows), len(rows), reached


def check_frames(sc: dict, call, *, capacity: int = 16) -> None:
    """``call(planes_alloc, nbits, count_of, W, step, capacity, list_buf | None, slots_buf | None, counts_buf) -> (list,
    slots, counts)`` (int64, uint8, int64 numpy).  capacity 0 passes NULL for the list and the slots."""
    planes, count_of = sc["planes"], sc["count_of"]
    nbits = planes.shape[1]
    want, kept, reached = frames_block(planes, count_of)
    assert [sum(1 for r in want if r[0] == p) for p in range(PHASES)] == sc["kept"] and kept > 0 and reached >= kept, sc["name"]
    if sc["name"] == "counts":
        assert count_of[:5] == [nbits, 0, 30, 31, 32] and count_of[7] == nbits and reached == kept + 1
        assert openers(planes[3][:31]).tolist() == [31] and walk(planes[3][:31], 31) == (None, False) and (7, 31) in {(r[0], r[1]) for r in want}
        assert frames_block(planes, [nbits] * PHASES)[1] > kept  # the counts decide, not the planes
    lst = np.full(4 * capacity + GUARD, SENT, dtype=np.int64) if capacity else None
    slots = np.full(capacity * SLOT_BYTES + GUARD, SENT8, dtype=np.uint8) if capacity else None
    counts = np.array([99, 99, SENT, SENT], dtype=np.int64)
    alloc = np.concatenate([np.ascontiguousarray(planes).reshape(-1), HOSTILE_U8])
    lst, slots, counts = call(alloc, nbits, count_of, FRAME_W, FRAME_STEP, capacity, lst, slots, counts)
    assert [int(x) for x in counts] == [kept, reached, SENT, SENT], sc["name"]
    if not capacity:
        return
    k = min(kept, capacity)
    entries, data = lst[: 4 * capacity].reshape(-1, 4), slots[: capacity * SLOT_BYTES].reshape(capacity, -1)
    assert (entries[k:] == SENT).all() and (lst[4 * capacity :] == SENT).all() and (data[k:] == SENT8).all() and (slots[capacity * SLOT_BYTES :] == SENT8).all()
    got = sorted((int(p), int(s), int(at), data[i, : int(nb)].tobytes(), bool((data[i, int(nb) :] == 0).all())) for i, (p, s, at, nb) in enumerate(entries[:k]))
    if kept <= capacity:
        assert got == [r + (True,) for r in want], sc["name"]
    else:
        assert all(g in [r + (True,) for r in want] for g in got) and len(got) == capacity, sc["name"]


OPENER_WANT = ~(0x0116162A ^ (0x0116162A >> 1)) & 0x7FFFFFFF  # bit j - 1: transition j of the opener's 32 bits


def standin_frames_of(g) -> tuple:
    """``frames_of`` written position by position as k_acars_frames goes: the opener as one 31-bit word, the walk byte by
    byte with its bounds against the count."""
    g = [int(x) & 1 for x in g]
    nb = len(g)
    kept, reached = [], 0
    for s in range(31, nb + 1):
        got = 0
        for j in range(1, 32):
            got |= g[s - 32 + j] << (j - 1)
        if got != OPENER_WANT:
            continue
        b, crc, j, out, end = 0, 0, s, bytearray(), False
        while True:
            if j + 8 > nb:
                break
            v = 0
            for k in range(8):
                b ^= g[j + k] ^ 1
                v |= b << k
            j += 8
            out.append(v)
            crc = _crc_step(crc, v)
            if v & 0x7F in (ETX, ETB):
                end = True
                break
            if len(out) == MAX_BODY:
                break
        if not end:
            continue
        reached += 1
        if j + 16 > nb:
            continue
        tail = []
        for _ in range(2):
            v = 0
            for k in range(8):
                b ^= g[j + k] ^ 1
                v |= b << k
            j += 8
            tail.append(v)
        if len(out) >= MIN_BODY and crc == (tail[0] | (tail[1] << 8)):
            kept.append((s, bytes(out) + bytes(tail)))
    return kept, reached


def _crc_step(reg: int, byte: int) -> int:
    reg ^= byte
    for _ in range(8):
        reg = (reg >> 1) ^ CRC_POLY if reg & 1 else reg >> 1
    return reg


def entry_frames(planes, nbits, count_of, W, step, capacity, lst, slots, counts):
    """iqa_acars_frames' checks, the cleared counters and the kernel's results in position order."""
    if nbits < 0 or capacity < 0:
        raise ValueError("negative length")
    if count_of is None:
        raise ValueError("NULL count table")
    if counts is None:
        raise ValueError("NULL device pointer")
    if not window_ok(W):
        raise ValueError("window must be 1 .. IQA_ACARS_MAX_WINDOW")
    if not step_ok(step):
        raise ValueError("step must be sps / 8 with 8 <= sps <= IQA_ACARS_MAX_SPS")
    if any(c < 0 or c > nbits for c in count_of):
        raise ValueError("count_of must be 0 .. nbits")
    if nbits > MAX_NBITS:
        raise ValueError("length out of range")
    if nbits > 0 and (planes is None or (capacity > 0 and (lst is None or slots is None))):
        raise ValueError("NULL device pointer")
    counts[:2] = 0
    if nbits == 0:
        return lst, slots, counts
    k = 0
    for p in range(PHASES):
        kept, reached = standin_frames_of(np.asarray(planes)[p * nbits : p * nbits + count_of[p]])
        counts[1] += reached
        for s, raw in kept:
            counts[0] += 1
            if k < capacity:
                lst[4 * k : 4 * k + 4] = (p, s, instant_of(W, step, s, p), len(raw))
                slots[k * SLOT_BYTES : (k + 1) * SLOT_BYTES] = np.frombuffer(raw.ljust(SLOT_BYTES, b"\0"), dtype=np.uint8)
                k += 1
    return lst, slots, counts


def frame_refusals() -> list:
    """(what, nbits, count_of | None, W, step, capacity, bits?, list?, slots?, counts?, message)."""
    ok = [8] * PHASES
    yes = (True,) * 4
    return [("negative nbits", -1, ok, 53, 5.0, 4) + yes + ("negative",), ("negative capacity", 8, ok, 53, 5.0, -1) + yes + ("negative",),
            ("NULL count table", 8, None, 53, 5.0, 4) + yes + ("NULL count table",), ("NULL counts", 8, ok, 53, 5.0, 4, True, True, True, False, "NULL"),
            ("window 0", 8, ok, 0, 5.0, 4) + yes + ("window must be",), ("window 537", 8, ok, MAX_WINDOW + 1, 5.0, 4) + yes + ("window must be",),
            ("step below 1", 8, ok, 53, 0.999, 4) + yes + ("step must be",), ("step above 50", 8, ok, 53, 50.01, 4) + yes + ("step must be",),
            ("a count above nbits", 8, [8, 8, 8, 9, 8, 8, 8, 8], 53, 5.0, 4) + yes + ("count_of must be",),
            ("a negative count", 8, [8, 8, 8, 8, 8, 8, 8, -1], 53, 5.0, 4) + yes + ("count_of must be",),
            ("nbits above 2^37", MAX_NBITS + 1, ok, 53, 5.0, 4) + yes + ("out of range",), ("NULL bits", 8, ok, 53, 5.0, 4, False, True, True, True, "NULL"),
            ("NULL list", 8, ok, 53, 5.0, 4, True, False, True, True, "NULL"), ("NULL slots", 8, ok, 53, 5.0, 4, True, True, False, True, "NULL")]
