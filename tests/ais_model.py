"""AIS model for the tests (a helper module, not a test file): the encoder (6-bit payload armour, message bit fields,
CRC-16/X.25, bit stuffing, training sequence, flags, NRZI), a GMSK modulator to complex baseband (Gaussian BT 0.4, +-2400 Hz,
fractional samples per bit, clock, tuning and spectrum-sense knobs), and a plain numpy oracle of DESIGN.md section 16
(steps 1-5).  The protocol constants are written out here from ITU-R M.1371 and IEC 61162-1 on their own, not imported from
the package, so that the encoder checks the decoder.  ``self_check`` pins them three ways."""
from __future__ import annotations

import math

import numpy as np

BAUD = 9600
BT = 0.4
DEVIATION = 2400.0  # modulation index 0.5
FLAG_BITS = [0, 1, 1, 1, 1, 1, 1, 0]
CRC_POLY = 0x8408  # x^16 + x^12 + x^5 + 1, reflected
MIN_FRAME, MAX_FRAME = 11, 128  # bytes, FCS included; 128 bytes is five slots
MIN_SPS, MAX_SPS = 5.0, 100.0
THETA_SCALE = 4096.0
TAP_SCALE = 256.0
PHASES = 8
TRAINING = 24  # bits of alternating training in front of the start flag
LEVEL_SPAN = (24, 9)  # the decision level of position s: the sum of v[s-24 .. s-9]
T_PI = 12_868  # rint(float32(pi) 4096): the largest |t| a discriminator produces
CHANNELS = (("A", 161_975_000.0), ("B", 162_025_000.0))
SENTENCE_CHARS = 60

REFERENCE_PAYLOAD = "177KQJ5000G?tO`K>RA1wUbN0TKH"
REFERENCE_SENTENCE = "!AIVDM,1,1,,B,177KQJ5000G?tO`K>RA1wUbN0TKH,0*5C"


# ---- encoder -----------------------------------------------------------------------------------------------------------


def crc16(data: bytes) -> int:
    """CRC-16/X.25: reflected 0x8408, init 0xFFFF, final xor 0xFFFF."""
    reg = 0xFFFF
    for byte in data:
        reg ^= byte
        for _ in range(8):
            reg = (reg >> 1) ^ CRC_POLY if reg & 1 else reg >> 1
    return reg ^ 0xFFFF


def armour(bits) -> tuple:
    """Message bits -> (payload characters, fill bits): six bits per character, first bit most significant."""
    bits = [int(b) for b in bits]
    fill = (-len(bits)) % 6
    bits = bits + [0] * fill
    out = []
    for k in range(0, len(bits), 6):
        v = int("".join(map(str, bits[k : k + 6])), 2)
        out.append(chr(v + 48 if v < 40 else v + 56))
    return "".join(out), fill


def dearmour(payload: str, fill: int = 0) -> list:
    bits = []
    for ch in payload:
        v = ord(ch) - 48
        if v > 40:
            v -= 8
        assert 0 <= v < 64, ch
        bits += [(v >> (5 - k)) & 1 for k in range(6)]
    return bits[: len(bits) - fill]


def field(value: int, width: int) -> list:
    """An integer as ``width`` bits, most significant first; negative values in two's complement."""
    return [((int(value) & ((1 << width) - 1)) >> (width - 1 - k)) & 1 for k in range(width)]


def text_field(text: str, chars: int) -> list:
    """6-bit ASCII: '@' .. '_' are 0 .. 31, ' ' .. '?' are 32 .. 63; padded with '@'."""
    out = []
    for ch in text.upper().ljust(chars, "@")[:chars]:
        c = ord(ch)
        assert 32 <= c < 96, ch
        out += field(c - 64 if c >= 64 else c, 6)
    return out


def deg(value: float) -> int:
    return int(round(value * 600_000.0))


def position_report(mtype: int, mmsi: int, *, status=0, turn=0, speed=0, accuracy=0, lon=181.0, lat=91.0, course=3600, heading=511,
                    second=60, repeat=0, radio=0) -> list:
    """Types 1 / 2 / 3, 168 bits.  speed and course in tenths."""
    return (field(mtype, 6) + field(repeat, 2) + field(mmsi, 30) + field(status, 4) + field(turn, 8) + field(speed, 10) + field(accuracy, 1)
            + field(deg(lon), 28) + field(deg(lat), 27) + field(course, 12) + field(heading, 9) + field(second, 6) + field(0, 2) + field(0, 3)
            + field(0, 1) + field(radio, 19))


def base_station(mmsi: int, utc=(2026, 10, 17, 12, 34, 56), *, accuracy=1, lon=181.0, lat=91.0, repeat=0) -> list:
    """Type 4, 168 bits."""
    y, mo, d, h, mi, s = utc
    return (field(4, 6) + field(repeat, 2) + field(mmsi, 30) + field(y, 14) + field(mo, 4) + field(d, 5) + field(h, 5) + field(mi, 6) + field(s, 6)
            + field(accuracy, 1) + field(deg(lon), 28) + field(deg(lat), 27) + field(1, 4) + field(0, 10) + field(0, 1) + field(0, 19))


def static_data(mmsi: int, *, imo=0, callsign="", name="", ship_type=0, dims=(0, 0, 0, 0), eta=(0, 0, 24, 60), draught=0, destination="",
                repeat=0) -> list:
    """Type 5, 424 bits.  draught in tenths of a metre."""
    return (field(5, 6) + field(repeat, 2) + field(mmsi, 30) + field(0, 2) + field(imo, 30) + text_field(callsign, 7) + text_field(name, 20)
            + field(ship_type, 8) + field(dims[0], 9) + field(dims[1], 9) + field(dims[2], 6) + field(dims[3], 6) + field(1, 4) + field(eta[0], 4)
            + field(eta[1], 5) + field(eta[2], 5) + field(eta[3], 6) + field(draught, 8) + text_field(destination, 20) + field(0, 1) + field(0, 1))


def class_b_report(mmsi: int, *, speed=0, accuracy=0, lon=181.0, lat=91.0, course=3600, heading=511, second=60, repeat=0) -> list:
    """Type 18, 168 bits."""
    return (field(18, 6) + field(repeat, 2) + field(mmsi, 30) + field(0, 8) + field(speed, 10) + field(accuracy, 1) + field(deg(lon), 28)
            + field(deg(lat), 27) + field(course, 12) + field(heading, 9) + field(second, 6) + field(0, 2) + field(0b11100, 5) + field(0, 2)
            + field(0, 20))


def aid_to_navigation(mmsi: int, *, aid_type=0, name="", accuracy=0, lon=181.0, lat=91.0, repeat=0) -> list:
    """Type 21 without a name extension, 272 bits."""
    return (field(21, 6) + field(repeat, 2) + field(mmsi, 30) + field(aid_type, 5) + text_field(name, 20) + field(accuracy, 1)
            + field(deg(lon), 28) + field(deg(lat), 27) + field(0, 30) + field(1, 4) + field(60, 6) + field(0, 1) + field(0, 8) + field(0, 1)
            + field(0, 1) + field(0, 1) + field(0, 1))


def static_part_a(mmsi: int, name: str, repeat=0) -> list:
    """Type 24 part A, 160 bits."""
    return field(24, 6) + field(repeat, 2) + field(mmsi, 30) + field(0, 2) + text_field(name, 20)


def static_part_b(mmsi: int, *, ship_type=0, vendor="", callsign="", dims=(0, 0, 0, 0), repeat=0) -> list:
    """Type 24 part B, 168 bits."""
    return (field(24, 6) + field(repeat, 2) + field(mmsi, 30) + field(1, 2) + field(ship_type, 8) + text_field(vendor, 7) + text_field(callsign, 7)
            + field(dims[0], 9) + field(dims[1], 9) + field(dims[2], 6) + field(dims[3], 6) + field(0, 6))


def reverse8(byte: int) -> int:
    return int(f"{byte:08b}"[::-1], 2)


def frame_bytes(bits) -> bytes:
    """Message bits (a multiple of 8) -> the HDLC frame: every 8 message bits are one byte sent least significant bit
    first, so the frame byte is the message byte reversed; FCS appended low byte first."""
    bits = [int(b) for b in bits]
    assert len(bits) % 8 == 0
    body = bytes(reverse8(int("".join(map(str, bits[k : k + 8])), 2)) for k in range(0, len(bits), 8))
    fcs = crc16(body)
    return body + bytes([fcs & 0xFF, fcs >> 8])


def message_bits(raw: bytes) -> list:
    """A frame (FCS included) -> its message bits."""
    out = []
    for byte in raw[:-2]:
        out += [(byte >> k) & 1 for k in range(8)]
    return out


def stuffed_bits(frame: bytes) -> list:
    out, ones = [], 0
    for byte in frame:
        for k in range(8):
            bit = (byte >> k) & 1
            out.append(bit)
            ones = ones + 1 if bit else 0
            if ones == 5:
                out.append(0)
                ones = 0
    return out


def burst_bits(frame: bytes, *, first: int = 0, post: int = 4) -> np.ndarray:
    """Data bits of one transmission: 24 alternating training bits beginning with ``first`` (the two alignments), the start
    flag, the stuffed frame, the end flag, ``post`` zeros of buffer."""
    bits = [(first + k) & 1 for k in range(TRAINING)] + FLAG_BITS + stuffed_bits(frame) + FLAG_BITS + [0] * post
    return np.array(bits, dtype=np.uint8)


def nrzi(bits, first: int = 1) -> np.ndarray:
    """Data bits -> levels: a zero toggles the level, a one keeps it."""
    out, level = [], first
    for b in np.asarray(bits).tolist():
        if not b:
            level ^= 1
        out.append(level)
    return np.array(out, dtype=np.uint8)


# ---- modulator ---------------------------------------------------------------------------------------------------------


def modulate(bits, fs: float, *, offset_hz: float = 0.0, ppm: float = 0.0, invert: bool = False, sigma: float = 0.0, seed: int = 0,
             lead: int = 1500, tail: int = 1500) -> np.ndarray:
    """Data bits -> NRZI levels +-1 -> a rectangular pulse train at ``fs`` (bit k covers [k, k + 1) fs / rate) -> Gaussian
    filter of BT 0.4 -> FM at +-2400 Hz, the carrier ``offset_hz`` off tune, the bit clock ``ppm`` fast, the deviation sign
    flipped by ``invert`` (an inverted spectrum); ``lead`` / ``tail`` samples without a carrier around it; complex AWGN of
    ``sigma`` per component over everything.  complex64 at ``fs``."""
    levels = 2.0 * nrzi(bits).astype(np.float64) - 1.0
    rate = BAUD * (1.0 + ppm * 1e-6)
    sps = fs / rate
    n = int(math.ceil(levels.size * sps))
    idx = np.minimum((np.arange(n, dtype=np.float64) * rate / fs).astype(np.int64), levels.size - 1)
    sg = math.sqrt(math.log(2.0)) / (2.0 * math.pi * BT) * sps
    half = int(math.ceil(4.0 * sg))
    g = np.exp(-0.5 * (np.arange(-half, half + 1, dtype=np.float64) / sg) ** 2)
    g /= g.sum()
    nrz = np.concatenate([np.full(half, levels[0]), levels[idx], np.full(half, levels[-1])])
    f = np.convolve(nrz, g, mode="valid") * (-DEVIATION if invert else DEVIATION)
    x = np.exp(1j * 2.0 * np.pi * np.cumsum(f + offset_hz) / fs)
    x = np.concatenate([np.zeros(lead, dtype=np.complex128), x, np.zeros(tail, dtype=np.complex128)])
    if sigma > 0.0:
        rng = np.random.default_rng(seed)
        x = x + sigma * (rng.normal(size=x.size) + 1j * rng.normal(size=x.size))
    return x.astype(np.complex64)


def noise_only(n: int, sigma: float, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (sigma * (rng.normal(size=n) + 1j * rng.normal(size=n))).astype(np.complex64)


def voice_carrier(n: int, fs: float, sigma: float, seed: int) -> np.ndarray:
    """An NFM carrier modulated by three drifting audio tones at 3 kHz peak deviation."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / fs
    audio = sum(a * np.sin(2.0 * np.pi * (f0 * t + 40.0 * np.sin(2.0 * np.pi * 0.7 * t + ph))) for a, f0, ph in ((0.5, 310.0, 0.0), (0.3, 930.0, 1.0), (0.2, 2170.0, 2.0)))
    x = np.exp(1j * 2.0 * np.pi * np.cumsum(3000.0 * audio) / fs)
    return (x + sigma * (rng.normal(size=n) + 1j * rng.normal(size=n))).astype(np.complex64)


# ---- oracle ------------------------------------------------------------------------------------------------------------


def theta_of(z) -> np.ndarray:
    """Step 1: the discriminator in float32, as numpy forms it (complex64 product, float32 angle)."""
    z = np.asarray(z, dtype=np.complex64)
    prev = np.concatenate([np.ones(1, dtype=np.complex64), z[:-1]])
    return np.angle(z * np.conj(prev)).astype(np.float32)


def quantise(theta) -> np.ndarray:
    return np.rint(np.asarray(theta, dtype=np.float32).astype(np.float64) * THETA_SCALE).astype(np.int32)


def taps_for(L: int, sps: float) -> np.ndarray:
    """The pulse filter of a window of L samples per bit: a Gaussian of BT 0.4 over 2 L taps, convolved with one bit of ones."""
    sg = math.sqrt(math.log(2.0)) / (2.0 * math.pi * BT) * sps
    k = np.arange(2 * L, dtype=np.float64)
    g = np.exp(-((k - (2 * L - 1) / 2.0) ** 2) / (2.0 * sg * sg))
    gb = np.convolve(g, np.ones(L))
    h = np.rint(TAP_SCALE * gb / gb.max()).astype(np.int64)
    assert h.size == 3 * L - 1 and T_PI * int(np.abs(h).sum()) < 2 ** 31
    return h


def plan(fs: float) -> dict:
    sps = float(fs) / BAUD
    if not (MIN_SPS <= sps <= MAX_SPS):
        raise ValueError("sps out of range")
    L = int(np.rint(sps))
    return dict(fs=float(fs), sps=sps, L=L, W=3 * L - 1, step=sps / 8.0, taps=taps_for(L, sps))


def pulse_filter(t, pl, hist=None) -> np.ndarray:
    """Step 2 (int64), causal from ``hist`` (W - 1 values in front of t[0]; None: zeros)."""
    t = np.asarray(t, dtype=np.int64)
    front = np.zeros(pl["W"] - 1, dtype=np.int64) if hist is None else np.asarray(hist, dtype=np.int64)
    assert front.size == pl["W"] - 1
    s = np.convolve(np.concatenate([front, t]), pl["taps"])[front.size : front.size + t.size]
    assert np.abs(s).max(initial=0) < 2 ** 31
    return s


def instants(pl, p: int, n: int) -> np.ndarray:
    """Symbol instants of phase p that lie inside a stream of n samples."""
    i = np.arange(int(n / pl["sps"]) + 3, dtype=np.float64)
    at = pl["W"] - 1 + np.rint((8.0 * i + p) * pl["step"]).astype(np.int64)
    return at[at < n]


def symbol_planes(S, pl) -> list:
    """Step 3 -> 8 (v int64, instants) pairs."""
    S = np.asarray(S, dtype=np.int64)
    out = []
    for p in range(PHASES):
        at = instants(pl, p, S.size)
        out.append((S[at], at))
    return out


def level_sum(v, s: int) -> int:
    return int(np.asarray(v[s - LEVEL_SPAN[0] : s - LEVEL_SPAN[1] + 1], dtype=np.int64).sum())


def bits_before(v, s: int, total: int) -> list:
    """b[s-22 .. s-1] under the decision level of s."""
    m = [int(16 * int(x) > total) for x in v[s - 23 : s]]
    return [int(m[k + 1] == m[k]) for k in range(22)]


def opens(v, s: int) -> bool:
    if s < 24 or s > len(v):
        return False
    b = bits_before(v, s, level_sum(v, s))
    return b[14:] == FLAG_BITS and all(b[k] != b[k + 1] for k in range(13))


def openers(v) -> np.ndarray:
    """Every position s >= 24 that opens a candidate (vectorised ``opens``)."""
    v = np.asarray(v, dtype=np.int64)
    if v.size < 24:
        return np.zeros(0, dtype=np.int64)
    s = np.arange(24, v.size + 1)
    c = np.concatenate([[0], np.cumsum(v)])
    total = c[s - 8] - c[s - 24]  # v[s-24 .. s-9]
    m = np.stack([16 * v[s - 23 + k] > total for k in range(23)])
    b = m[1:] == m[:-1]  # b[k] = bit s - 22 + k
    ok = np.ones(s.size, dtype=bool)
    for k in range(13):
        ok &= b[k] != b[k + 1]
    for k, want in enumerate(FLAG_BITS):
        ok &= b[14 + k] == bool(want)
    return s[ok]


def walk(v, s: int):
    """Step 4 from an opened position: the frame bytes, or None (abort, too long, cut by the end of the stream)."""
    total = level_sum(v, s)
    out, cur, nb, ones = bytearray(), 0, 0, 0
    prev = int(16 * int(v[s - 1]) > total)

    def bit_at(j):
        return int(int(16 * int(v[j]) > total) == int(16 * int(v[j - 1]) > total))

    for j in range(s, len(v)):
        m = int(16 * int(v[j]) > total)
        bit, prev = int(m == prev), m
        if bit:
            ones += 1
            if ones == 6:
                return bytes(out) if (j + 1 < len(v) and bit_at(j + 1) == 0 and nb == 6) else None
        else:
            if ones == 5:
                ones = 0
                continue
            ones = 0
        cur |= bit << nb
        nb += 1
        if nb == 8:
            if len(out) == MAX_FRAME:
                return None
            out.append(cur)
            cur, nb = 0, 0
    return None


def frames_of(v) -> tuple:
    """Step 4 on one symbol plane -> ([(s, bytes)] kept, candidates closed with >= 11 bytes)."""
    kept, closed = [], 0
    for s in openers(v).tolist():
        got = walk(v, s)
        if got is None or len(got) < MIN_FRAME:
            continue
        closed += 1
        if crc16(got[:-2]) == got[-2] | (got[-1] << 8):
            kept.append((s, got))
    return kept, closed


# ---- step 5: messages ---------------------------------------------------------------------------------------------------


def uint(bits, at: int, width: int) -> int:
    return int("".join(str(b) for b in bits[at : at + width]), 2)


def sint(bits, at: int, width: int) -> int:
    v = uint(bits, at, width)
    return v - (1 << width) if v >> (width - 1) else v


def text(bits, at: int, chars: int) -> str:
    out = ""
    for k in range(chars):
        c = uint(bits, at + 6 * k, 6)
        out += chr(c + 64 if c < 32 else c)
    return out.rstrip("@ ")


def lon_of(raw: int):
    return None if raw == 181 * 600_000 else raw / 600_000


def lat_of(raw: int):
    return None if raw == 91 * 600_000 else raw / 600_000


def tenths(raw: int, missing: int):
    return None if raw == missing else raw / 10


def missing(raw: int, value: int):
    return None if raw == value else raw


def dims(bits, at: int) -> dict:
    return dict(to_bow=uint(bits, at, 9), to_stern=uint(bits, at + 9, 9), to_port=uint(bits, at + 18, 6), to_starboard=uint(bits, at + 24, 6))


NEED = {1: 168, 2: 168, 3: 168, 4: 168, 5: 424, 18: 168, 21: 272, 24: 160}


def decode_fields(bits) -> dict:
    """Message bits -> type, repeat, mmsi and the fields of the decoded types (none where the message is shorter than its type)."""
    out = dict(type=uint(bits, 0, 6), repeat=uint(bits, 6, 2), mmsi=uint(bits, 8, 30))
    t = out["type"]
    if len(bits) < NEED.get(t, 1 << 30):
        return out
    if t in (1, 2, 3):
        out.update(status=uint(bits, 38, 4), turn=missing(sint(bits, 42, 8), -128), speed=tenths(uint(bits, 50, 10), 1023), accuracy=uint(bits, 60, 1),
                   lon=lon_of(sint(bits, 61, 28)), lat=lat_of(sint(bits, 89, 27)), course=tenths(uint(bits, 116, 12), 3600),
                   heading=missing(uint(bits, 128, 9), 511), second=uint(bits, 137, 6))
    elif t == 4:
        out.update(year=uint(bits, 38, 14), month=uint(bits, 52, 4), day=uint(bits, 56, 5), hour=uint(bits, 61, 5), minute=uint(bits, 66, 6),
                   second=uint(bits, 72, 6), accuracy=uint(bits, 78, 1), lon=lon_of(sint(bits, 79, 28)), lat=lat_of(sint(bits, 107, 27)))
    elif t == 5:
        out.update(imo=uint(bits, 40, 30), callsign=text(bits, 70, 7), name=text(bits, 112, 20), ship_type=uint(bits, 232, 8), **dims(bits, 240),
                   eta_month=uint(bits, 274, 4), eta_day=uint(bits, 278, 5), eta_hour=uint(bits, 283, 5), eta_minute=uint(bits, 288, 6),
                   draught=uint(bits, 294, 8) / 10, destination=text(bits, 302, 20))
    elif t == 18:
        out.update(speed=tenths(uint(bits, 46, 10), 1023), accuracy=uint(bits, 56, 1), lon=lon_of(sint(bits, 57, 28)), lat=lat_of(sint(bits, 85, 27)),
                   course=tenths(uint(bits, 112, 12), 3600), heading=missing(uint(bits, 124, 9), 511), second=uint(bits, 133, 6))
    elif t == 21:
        out.update(aid_type=uint(bits, 38, 5), name=text(bits, 43, 20), accuracy=uint(bits, 163, 1), lon=lon_of(sint(bits, 164, 28)),
                   lat=lat_of(sint(bits, 192, 27)))
    elif t == 24:
        part = uint(bits, 38, 2)
        if part == 0:
            out.update(part="A", name=text(bits, 40, 20))
        elif part == 1 and len(bits) >= 168:
            out.update(part="B", ship_type=uint(bits, 40, 8), vendor=text(bits, 48, 7), callsign=text(bits, 90, 7), **dims(bits, 132))
    return out


def channel_of(frequency) -> str:
    if frequency is None:
        return ""
    for name, f in CHANNELS:
        if abs(float(frequency) - f) <= 5000.0:
            return name
    return ""


def checksum(body: str) -> str:
    x = 0
    for ch in body:
        x ^= ord(ch)
    return f"{x:02X}"


def sentences(bits, channel: str, seq: int) -> list:
    """!AIVDM sentences of one message; ``seq`` is the id a multi-sentence message takes."""
    payload, fill = armour(bits)
    parts = [payload[k : k + SENTENCE_CHARS] for k in range(0, len(payload), SENTENCE_CHARS)]
    out = []
    for k, part in enumerate(parts):
        body = f"AIVDM,{len(parts)},{k + 1},{seq if len(parts) > 1 else ''},{channel},{part},{fill if k == len(parts) - 1 else 0}"
        out.append(f"!{body}*{checksum(body)}")
    return out


def merge(records, L: int) -> list:
    """[(phase, s, instant, bytes)] -> [(instant, bytes, hits)]: sorted by instant; identical bytes whose start instants
    differ by <= L from the group's first are one message."""
    out = []
    for p, s, at, raw in sorted(records, key=lambda r: (r[2], r[0])):
        same = [grp for grp in out if grp[1] == raw and at - grp[0] <= L]
        if same:
            same[-1][2] += 1
        else:
            out.append([at, raw, 1])
    return [tuple(grp) for grp in out]


def messages_of(records, pl, frequency=None) -> list:
    out, seq = [], 0
    channel = channel_of(frequency)
    for at, raw, hits in merge(records, pl["L"]):
        bits = message_bits(raw)
        nmea = sentences(bits, channel, seq)
        if len(nmea) > 1:
            seq = (seq + 1) % 10
        out.append(dict(decode_fields(bits), time_s=at / pl["fs"], raw=raw.hex(), nmea=nmea, channel=channel, hits=hits))
    return out


def oracle(theta=None, fs: float = 96_000.0, *, t=None, frequency=None) -> dict:
    """Steps 1-5 from a discriminator output (or from given ``t``)."""
    pl = plan(fs)
    t = quantise(theta) if t is None else np.asarray(t, dtype=np.int32)
    S = pulse_filter(t, pl)
    planes = symbol_planes(S, pl)
    records, closed = [], 0
    for p, (v, at) in enumerate(planes):
        kept, c = frames_of(v)
        closed += c
        records += [(p, s, int(at[s]), raw) for s, raw in kept]
    records.sort(key=lambda r: (r[0], r[1]))
    return dict(t=t, S=S, v=[v for v, _ in planes], records=records, closed=closed, messages=messages_of(records, pl, frequency))


# ---- hand-made symbol planes for the walker tests -------------------------------------------------------------------------


def plane_of(bits, *, high: int = 9000, low: int = -7000, first: int = 1) -> np.ndarray:
    """Data bits -> int32 symbol values: NRZI levels at ``high`` / ``low`` (unequal on purpose: the level is not zero)."""
    return np.where(nrzi(bits, first) == 1, high, low).astype(np.int32)


def with_fcs(body: bytes) -> bytes:
    fcs = crc16(body)
    return body + bytes([fcs & 0xFF, fcs >> 8])


def hand_made_planes() -> list:
    """(name, plane, symbols that exist, frames kept): where fewer symbols exist than the plane holds, the plane goes on with
    the symbols that would have closed the frame, which a walker must not read."""
    frame = with_fcs(bytes([0x7E, 0x7E, 0xFF, 0xFF, 0x7E, 0x3E, 0x7C, 0x00, 0x55, 0xAA, 0xF8, 0x1F]))  # 0x7E and runs of ones in the payload
    stuffed = stuffed_bits(frame)
    head = TRAINING + 8
    bits = burst_bits(frame)
    train = [k & 1 for k in range(TRAINING)]
    out = [("flag in the payload", plane_of(bits), None, 1),
           ("other alignment", plane_of(burst_bits(frame, first=1)), None, 1),
           ("other polarity", plane_of(bits, first=0), None, 1),
           ("abort", plane_of(train + FLAG_BITS + stuffed[:40] + [1] * 7 + stuffed[40:] + FLAG_BITS + [0] * 4), None, 0),
           ("flag off the byte boundary", plane_of(train + FLAG_BITS + stuffed[:43] + FLAG_BITS + stuffed[43:] + FLAG_BITS + [0] * 4), None, 0),
           ("cut inside the frame", plane_of(bits), head + len(stuffed) - 5, 0),
           ("cut inside the closing flag", plane_of(bits), head + len(stuffed) + 7, 0),
           ("cut behind the closing flag", plane_of(bits), head + len(stuffed) + 8, 1),
           ("shorter than the opener", plane_of(bits), 23, 0), ("the opener alone", plane_of(bits), head, 0), ("empty", plane_of(bits), 0, 0)]
    for size, kept in ((10, 0), (11, 1), (128, 1), (129, 0)):
        f = with_fcs(bytes((3 * k + 1) & 0xFF for k in range(size - 2)))
        assert len(f) == size
        out.append((f"{size} bytes", plane_of(burst_bits(f)), None, kept))
    for k in range(head + 50, head + 70):  # a flipped payload bit that leaves the stuffing alone: closed, but the CRC fails
        bad = bits.copy()
        bad[k] ^= 1
        if frames_of(plane_of(bad)) == ([], 1):
            break
    else:
        raise AssertionError("no such bit")
    out.append(("damaged", plane_of(bad), None, 0))
    # 16 v == sum exactly: training symbols 3 / 1 (sum of sixteen = 32), a payload symbol of exactly 2 is level 0
    tie = plane_of(bits, high=3, low=1)
    k = head + 20 + int(np.argmin(nrzi(bits)[head + 20 :]))  # a low symbol: the frame survives iff the tie is read as low
    assert tie[k] == 1
    tie[k] = 2
    out.append(("level tie", tie, None, 1))
    return [(name, np.asarray(v, dtype=np.int32), int(v.size if count is None else count), kept) for name, v, count, kept in out]


def self_check() -> None:
    """The three pins of the constants."""
    assert crc16(b"123456789") == 0x906E
    bits = dearmour(REFERENCE_PAYLOAD)
    assert len(bits) == 168
    got = decode_fields(message_bits(frame_bytes(bits)))
    assert (got["type"], got["mmsi"], got["status"], got["speed"], got["course"], got["heading"], got["second"]) == (1, 477553000, 5, 0.0, 51.0, 181, 15)
    assert abs(got["lat"] - 47.58283333) < 1e-8 and abs(got["lon"] + 122.34583333) < 1e-8
    again = position_report(1, 477553000, status=5, turn=got["turn"], speed=0, accuracy=got["accuracy"], lon=got["lon"], lat=got["lat"], course=510,
                            heading=181, second=15, radio=uint(bits, 149, 19))
    assert again[:143] == bits[:143] and again[149:] == bits[149:]
    assert armour(bits) == (REFERENCE_PAYLOAD, 0)
    assert sentences(bits, "B", 0) == [REFERENCE_SENTENCE]


# ---- edge shapes (tests/test_gpu_ais_shapes.py, tests/test_ais_shapes_host.py) -------------------------------------------
#
# Case tables, block oracles and numpy stand-ins of the three entry points that follow csrc/ais.hip's launch arithmetic and
# can be broken one way at a time.  The ``check_*`` functions hold the comparisons; they take the entry point as a callable,
# so the GPU file passes the device call and the host file the stand-in.

SENT = -7_777_777  # what untouched output words hold
GUARD = 16  # sentinel words behind every output
FRONT = 4  # words in front of every view (16 bytes, so that offset 0 stays 16-byte aligned); sentinels where it is an output
TILE, RUN = 2048, 8  # AI_TILE, AI_RUN
MAX_TAPS = 299
MAX_N, MAX_NSYM = 1 << 40, 1 << 37
SLOT_BYTES = 128
FILTER_WINDOWS = (1, 2, 8, 9, 16, 17, 298, 299)
FILTER_LENGTHS = (7, 8, 9, TILE + 8, 2 * TILE + 5)
HOSTILE_F32 = np.array([np.nan, np.inf, -np.inf, 3.0e38], dtype=np.float32)
HOSTILE_I32 = np.array([2 ** 31 - 1, -(2 ** 31), 2 ** 31 - 1, -(2 ** 31)], dtype=np.int32)


def wrap32(x):
    return ((np.asarray(x, dtype=np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def s24(x):
    """The low 24 bits, sign-extended: what v_mad_i32_i24 reads of an operand."""
    return ((np.asarray(x, dtype=np.int64) & 0xFFFFFF) ^ 0x800000) - 0x800000


def view_offsets() -> list:
    """(theta, hist, t_out, s_out) element offsets inside their allocations: the four s_out offsets, each with theta
    16-byte aligned and not; hist and t_out take all four values as well, not in step with either."""
    out = []
    for s_off in range(4):
        for k, th_off in enumerate((0, 1 + s_off % 3)):
            out.append((th_off, (2 * s_off + k + 1) % 4, (3 * s_off + 2 * k + 2) % 4, s_off))
    return out


def shape_taps(W: int, seed: int) -> np.ndarray:
    """int16[W] in 0 .. 256, arbitrary (not symmetric), both ends at the bound."""
    h = np.random.default_rng(seed).integers(0, 257, size=W).astype(np.int16)
    h[0] = 256
    h[-1] = 256 if W > 1 else h[-1]
    return h


def filter_theta(n: int, W: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    pi32 = np.float32(np.pi)
    th = np.clip(rng.uniform(-np.pi, np.pi, n).astype(np.float32), -pi32, pi32)
    ties = ((np.arange(-6, 6, dtype=np.float64) + 0.5) / 4096.0).astype(np.float32)
    th[: min(n, ties.size)] = ties[: min(n, ties.size)]
    if n > TILE + 4:
        th[TILE - 4 : TILE + 4] = ties[:8]
    return th


def filter_cases(W: int) -> list:
    """dict(name, W, n, taps, theta, hist | None, offsets): arbitrary taps at every n x history x view offsets, and the two
    full-scale sets (all taps 256, theta and history held at +pi / -pi), whose every output is +-12 868 . 256 . W."""
    out = []
    for n in FILTER_LENGTHS:
        for with_hist in (False, True):
            for k, offs in enumerate(view_offsets()):
                seed = 10_000 * W + 10 * n + k + with_hist
                hist = None
                if with_hist:
                    hist = np.random.default_rng(seed + 1).integers(-T_PI, T_PI + 1, size=W - 1).astype(np.int32)
                    if W > 1:
                        hist[0], hist[-1] = T_PI, -T_PI
                out.append(dict(name=f"W {W} n {n} hist {'given' if with_hist else 'NULL'} offsets {offs}", W=W, n=n, taps=shape_taps(W, seed + 2),
                                theta=filter_theta(n, W, seed), hist=hist, offsets=offs, full=0))
    for sign in (1, -1):
        for n, offs in ((TILE + 8, (0, 0, 0, 0)), (2 * TILE + 5, (1, 2, 3, 1)), (9, (2, 1, 0, 3))):
            out.append(dict(name=f"W {W} n {n} all taps 256, theta {'+' if sign > 0 else '-'}pi, offsets {offs}", W=W, n=n, taps=np.full(W, 256, dtype=np.int16),
                            theta=np.full(n, sign * np.float32(np.pi), dtype=np.float32), hist=np.full(W - 1, sign * T_PI, dtype=np.int32),
                            offsets=offs, full=sign))
    return out


def check_filter(case: dict, call) -> None:
    """``call(theta_alloc, th_at, n, hist_alloc | None, h_at, W, taps_alloc, t_alloc, t_at, s_alloc, s_at) -> (t_alloc,
    s_alloc)`` after the call (int32 numpy); ``*_at`` is the element index of the view inside its allocation (FRONT + the
    offset), the outputs arrive filled with SENT."""
    W, n, taps = case["W"], case["n"], case["taps"]
    th_off, h_off, t_off, s_off = case["offsets"]
    want_t = quantise(case["theta"])
    want_s = pulse_filter(want_t, dict(W=W, taps=taps.astype(np.int64)), case["hist"])
    assert taps.min() >= 0 and taps.max() <= 256 and np.abs(want_t).max() <= T_PI
    if case["full"]:
        assert (want_s == case["full"] * T_PI * 256 * W).all() and T_PI * 256 * W < 2 ** 31, case["name"]
    elif n >= 12:
        assert list(want_t[:12]) == [-6, -4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6]  # half-even
    if case["hist"] is not None and W > 1 and not case["full"]:
        assert int(want_s[0]) != int(pulse_filter(want_t, dict(W=W, taps=taps.astype(np.int64)), None)[0]), case["name"]
    theta = np.concatenate([np.resize(HOSTILE_F32, FRONT + th_off), case["theta"], HOSTILE_F32])
    hist = None if case["hist"] is None else np.concatenate([np.resize(HOSTILE_I32, FRONT + h_off), case["hist"], HOSTILE_I32])
    taps_alloc = np.concatenate([taps, np.full(8, 32767, dtype=np.int16)])
    t_alloc = np.full(FRONT + t_off + n + GUARD, SENT, dtype=np.int32)
    s_alloc = np.full(FRONT + s_off + n + GUARD, SENT, dtype=np.int32)
    t_alloc, s_alloc = call(theta, FRONT + th_off, n, hist, FRONT + h_off, W, taps_alloc, t_alloc, FRONT + t_off, s_alloc, FRONT + s_off)
    for got, off, want, what in ((s_alloc, s_off, want_s, "S"), (t_alloc, t_off, want_t, "t")):
        a = FRONT + off
        np.testing.assert_array_equal(got[a : a + n], want, err_msg=f"{what}: {case['name']}")
        assert (got[:a] == SENT).all() and (got[a + n :] == SENT).all(), f"{what} guards: {case['name']}"


def kernel_filter(theta, n: int, hist, W: int, taps, t_out, s_alloc, s_at: int, *, wide_store_always: bool = False) -> None:
    """k_ais_filter and its launch in numpy, tile by tile: the staged image (history, block, zeros), the taps behind tap 0
    zero-padded to H, 24-bit operands and an int32 accumulator, and the two store paths -- 8 words at once where the whole
    run lies inside n and ``s_out`` is 16-byte aligned, element by element otherwise.  ``theta``, ``hist`` and ``t_out``
    are the views; ``s_alloc`` is the allocation (16-byte aligned) and ``s_at`` the view's element index in it.  Break:
    ``wide_store_always`` takes the 16-byte path whatever the address, which a memory path that ignores the low address
    bits rounds down to a multiple of 16 bytes."""
    H = (W - 1 + RUN - 1) // RUN * RUN
    tp = np.zeros(1 + H, dtype=np.int64)
    tp[:W] = np.asarray(taps[:W], dtype=np.int64)
    aligned = (4 * s_at) % 16 == 0
    for b in range(-(-n // TILE)):
        A = b * TILE
        a = A - H + np.arange(H + TILE)
        img = np.zeros(H + TILE, dtype=np.int64)
        if hist is not None:
            sel = (a < 0) & (a >= -(W - 1))
            img[sel] = np.asarray(hist)[(W - 1) + a[sel]]
        ins = (a >= 0) & (a < n)
        img[ins] = quantise(np.asarray(theta)[a[ins]])
        own = ins & (np.arange(H + TILE) >= H)
        if t_out is not None:
            t_out[a[own]] = img[own]
        acc = wrap32(np.convolve(s24(img), s24(tp))[H : H + TILE])  # acc[j] = sum_k tp[k] img[H + j - k]
        for tid in range(TILE // RUN):
            a0 = A + tid * RUN
            if a0 >= n:
                break
            run = acc[tid * RUN : (tid + 1) * RUN]
            if a0 + RUN <= n and (aligned or wide_store_always):
                at = (s_at + a0) // 4 * 4 if not aligned else s_at + a0
                s_alloc[at : at + RUN] = run
            else:
                for r in range(RUN):
                    if a0 + r < n:
                        s_alloc[s_at + a0 + r] = run[r]


def window_ok(W) -> bool:
    return 1 <= W <= MAX_TAPS


def step_ok(step) -> bool:
    return 5.0 / 8.0 <= step <= MAX_SPS / 8.0  # (false for a NaN)


def entry_filter(theta, th_at, n, hist, h_at, W, taps, t_alloc, t_at, s_alloc, s_at, **breaks) -> None:
    """iqa_ais_filter's checks in front of ``kernel_filter``; None stands for a NULL pointer."""
    if n < 0:
        raise ValueError("negative length")
    if not window_ok(W):
        raise ValueError("window must be 1 .. 3 IQA_AIS_MAX_SPS - 1")
    if n == 0:
        return
    if theta is None or taps is None or s_alloc is None:
        raise ValueError("NULL device pointer")
    if n > MAX_N:
        raise ValueError("length out of range")
    kernel_filter(theta[th_at:], n, None if hist is None else hist[h_at:], W, taps, None if t_alloc is None else t_alloc[t_at:], s_alloc, s_at, **breaks)


def filter_refusals() -> list:
    """(what, n, W, theta?, taps?, s_out?, message)."""
    return [("negative n", -1, 29, True, True, True, "negative"), ("window 0", 64, 0, True, True, True, "window must be"),
            ("window 300", 64, MAX_TAPS + 1, True, True, True, "window must be"), ("NULL theta", 64, 29, False, True, True, "NULL"),
            ("NULL taps", 64, 29, True, False, True, "NULL"), ("NULL s_out", 64, 29, True, True, False, "NULL"), ("n above 2^40", MAX_N + 1, 29, True, True, True, "out of range")]


# -- symbols


SYMBOL_COUNTS = (0, 1, 255, 256, 257)
SYMBOL_SHAPES = ((10.0, 29), (6.0, 17), (5.0, 1), (100.0, 299), (10.125, 30))  # (sps, W): steps 1.25 and 0.75 have exact .5 ties


def symbols_block(S, n: int, W: int, step: float, nsym: int) -> tuple:
    """(v int32[8, nsym], instants int64[8, nsym], ties bool[8, nsym]): v = S[instant] where the instant lies inside n."""
    x = (8.0 * np.arange(nsym, dtype=np.float64)[None, :] + np.arange(PHASES, dtype=np.float64)[:, None]) * step
    at = W - 1 + np.rint(x).astype(np.int64)
    v = np.zeros((PHASES, nsym), dtype=np.int32)
    ok = at < n
    v[ok] = np.asarray(S)[at[ok]]
    return v, at, np.mod(x, 1.0) == 0.5


def symbol_cases() -> list:
    """dict(name, sps, W, n, nsym): every count at every shape, on a plane that ends inside the last symbols (so some phases
    read zeros), and a plane shorter than W - 1 (every instant lies beyond it)."""
    out = []
    for sps, W in SYMBOL_SHAPES:
        for nsym in SYMBOL_COUNTS:
            n = W - 1 + int(np.rint(max(nsym - 2, 1) * sps)) + 3
            out.append(dict(name=f"sps {sps} W {W} nsym {nsym} n {n}", sps=sps, W=W, n=n, nsym=nsym))
        if W > 2:
            out.append(dict(name=f"sps {sps} W {W}: a plane of W - 2 samples", sps=sps, W=W, n=W - 2, nsym=256))
    return out


def check_symbols(case: dict, call, stats: dict | None = None) -> None:
    """``call(S_alloc, n, W, step, nsym, v_buf) -> v_buf`` (int32 numpy)."""
    sps, W, n, nsym = case["sps"], case["W"], case["n"], case["nsym"]
    step = sps / 8.0
    S = np.random.default_rng(n + nsym).integers(-(2 ** 31), 2 ** 31, size=n).astype(np.int32)
    S[S == 0] = 1
    want, at, ties = symbols_block(S, n, W, step, nsym)
    if n == W - 2:
        assert (want == 0).all() and at.min() == W - 1 > n - 1
    elif nsym >= 255:
        assert (at >= n).any() and (want[:, : nsym - 4] != 0).all(), case["name"]  # the plane ends inside the last symbols
    if stats is not None and nsym:
        x = (8.0 * np.arange(nsym)[None, :] + np.arange(PHASES)[:, None]) * step
        stats["ties"] = stats.get("ties", 0) + int(ties.sum())
        stats["ties rounded down"] = stats.get("ties rounded down", 0) + int((ties & (np.rint(x) != np.floor(x + 0.5))).sum())
    v_buf = np.full(PHASES * nsym + GUARD, SENT, dtype=np.int32)
    v_buf = call(np.concatenate([S, HOSTILE_I32]), n, W, step, nsym, v_buf)
    np.testing.assert_array_equal(v_buf[: PHASES * nsym].reshape(PHASES, nsym), want, err_msg=case["name"])
    assert (v_buf[PHASES * nsym :] == SENT).all(), case["name"]


def entry_symbols(S, n, W, step, nsym, v_out) -> None:
    if n < 0 or nsym < 0:
        raise ValueError("negative length")
    if not window_ok(W):
        raise ValueError("window must be 1 .. 3 IQA_AIS_MAX_SPS - 1")
    if not step_ok(step):
        raise ValueError("step must be sps / 8 with 5 <= sps <= IQA_AIS_MAX_SPS")
    if nsym == 0:
        return
    if S is None or v_out is None:
        raise ValueError("NULL device pointer")
    if n > MAX_N or nsym > MAX_NSYM:
        raise ValueError("length out of range")
    v_out[: PHASES * nsym] = symbols_block(S, n, W, step, nsym)[0].reshape(-1)


def symbol_refusals() -> list:
    """(what, n, W, step, nsym, S?, v?, message)."""
    return [("negative n", -1, 29, 1.25, 8, True, True, "negative"), ("negative nsym", 64, 29, 1.25, -1, True, True, "negative"),
            ("window 0", 64, 0, 1.25, 8, True, True, "window must be"), ("window 300", 64, MAX_TAPS + 1, 1.25, 8, True, True, "window must be"),
            ("step below 5/8", 64, 29, 0.624, 8, True, True, "step must be"), ("step above 100/8", 64, 29, 12.51, 8, True, True, "step must be"),
            ("step not a number", 64, 29, float("nan"), 8, True, True, "step must be"), ("NULL S", 64, 29, 1.25, 8, False, True, "NULL"),
            ("NULL v", 64, 29, 1.25, 8, True, False, "NULL"), ("n above 2^40", MAX_N + 1, 29, 1.25, 8, True, True, "out of range"),
            ("nsym above 2^37", 64, 29, 1.25, MAX_NSYM + 1, True, True, "out of range")]


# -- frames


FRAME_NSYM = (255, 256, 257)
FRAME_W, FRAME_STEP = 29, 1.25
AFFINE_A = (2 ** 31 - 2) // 16_000  # 134 217: 9000 a + b = 2 147 472 001, just below 2^31 - 1
AFFINE_B = 7_000 * AFFINE_A + 1  # -7000 a + b = 1: every symbol positive


def affine(v) -> np.ndarray:
    out = AFFINE_A * np.asarray(v, dtype=np.int64) + AFFINE_B
    assert out.min() >= 1 and out.max() < 2 ** 31
    return out.astype(np.int32)


def _padded(v, nsym: int, *, right: bool = False) -> np.ndarray:
    v = np.asarray(v, dtype=np.int32)
    assert v.size <= nsym, (v.size, nsym)
    pad = np.full(nsym - v.size, -7000, dtype=np.int32)
    return np.concatenate([pad, v] if right else [v, pad])


def frame_scenarios(nsym: int) -> list:
    """dict(name, planes int32[8, nsym], count_of[8], kept[8]): eight different planes and counts in one call.
    "cuts": the closing flag's last symbol at index nsym - 1 = count - 1 (the frame right-aligned in the plane), at
    count - 1 inside the plane, at count (cut off); counts 0, 23, 24, 25 and nsym; a candidate that opens at s = 24.
    "walks": the hand-made planes of the walker test, one per phase, each with its own count."""
    hand = {name: (v, count, kept) for name, v, count, kept in hand_made_planes()}
    base = hand["flag in the payload"][0]
    end = hand["cut behind the closing flag"][1]  # the index behind the closing flag's last symbol
    assert hand["cut inside the closing flag"][1] == end - 1
    early = base[8:]  # 16 training symbols in front of the flag: the candidate opens at the first position there is
    tie = hand["level tie"][0]
    cuts = [(_padded(base[:end], nsym, right=True), nsym, 1), (_padded(base, nsym), end, 1), (_padded(base, nsym), end - 1, 0), (_padded(tie, nsym), 0, 0),
            (_padded(early, nsym), 23, 0), (_padded(early, nsym), 24, 0), (_padded(early, nsym), 25, 0), (_padded(early, nsym), nsym, 1)]
    names = ("level tie", "other polarity", "other alignment", "damaged", "abort", "flag off the byte boundary", "11 bytes", "10 bytes")
    walks = [(_padded(hand[k][0], nsym), int(hand[k][0].size), hand[k][2]) for k in names]
    out = []
    for name, rows in (("cuts", cuts), ("walks", walks)):
        out.append(dict(name=f"{name}, nsym {nsym}", planes=np.stack([r[0] for r in rows]), count_of=[int(r[1]) for r in rows], kept=[int(r[2]) for r in rows]))
    return out


def instant_of(W: int, step: float, s: int, p: int) -> int:
    return W - 1 + int(np.rint(float(8 * s + p) * step))


def frames_block(planes, count_of, W: int = FRAME_W, step: float = FRAME_STEP) -> tuple:
    """(sorted [(phase, s, instant, bytes)], kept frames, closed candidates) of eight planes with their own counts."""
    rows, closed = [], 0
    for p in range(PHASES):
        kept, c = frames_of(np.asarray(planes[p][: count_of[p]], dtype=np.int64))
        closed += c
        rows += [(p, int(s), instant_of(W, step, int(s), p), raw) for s, raw in kept]
    return sorted(rows), len(rows), closed


def check_frames(sc: dict, call, *, mapped: bool, capacity: int = 16) -> None:
    """``call(planes_alloc, nsym, count_of, W, step, capacity, list_buf, slots_buf, counts_buf) -> (list, slots, counts)``
    (int64, uint8, int64 numpy).  ``mapped``: the planes under v -> a v + b, which leaves every decision 16 v > sum as it
    is; the kept frames must be the unmapped planes'."""
    planes, count_of = sc["planes"], sc["count_of"]
    nsym = planes.shape[1]
    want, kept, closed = frames_block(planes, count_of)
    assert [sum(1 for r in want if r[0] == p) for p in range(PHASES)] == sc["kept"] and kept > 0, sc["name"]
    if "cuts" in sc["name"]:
        assert {0, 23, 24, 25, nsym} <= set(count_of) and (7, 24) in {(r[0], r[1]) for r in want}
        assert frames_block(planes, [nsym] * PHASES)[1] > kept  # the counts decide, not the planes
    if mapped:
        planes = np.stack([affine(v) for v in planes])
        assert frames_block(planes, count_of) == (want, kept, closed) and int(planes.max()) > 2 ** 31 - 16_000
    lst = np.full(4 * capacity + GUARD, SENT, dtype=np.int64)
    slots = np.full(capacity * SLOT_BYTES + GUARD, 0xAA, dtype=np.uint8)
    counts = np.array([99, 99, SENT, SENT], dtype=np.int64)
    alloc = np.concatenate([np.ascontiguousarray(planes).reshape(-1), HOSTILE_I32])
    lst, slots, counts = call(alloc, nsym, count_of, FRAME_W, FRAME_STEP, capacity, lst, slots, counts)
    assert [int(x) for x in counts] == [kept, closed, SENT, SENT], sc["name"]
    entries, data = lst[: 4 * capacity].reshape(-1, 4), slots[: capacity * SLOT_BYTES].reshape(capacity, -1)
    assert (entries[kept:] == SENT).all() and (lst[4 * capacity :] == SENT).all() and (data[kept:] == 0xAA).all() and (slots[capacity * SLOT_BYTES :] == 0xAA).all()
    got = sorted((int(p), int(s), int(at), data[i, : int(nb)].tobytes(), bool((data[i, int(nb) :] == 0).all())) for i, (p, s, at, nb) in enumerate(entries[:kept]))
    assert got == [r + (True,) for r in want], sc["name"]


def standin_frames_of(v, *, level32: bool = False, mul32: bool = False) -> tuple:
    """``frames_of`` written position by position as k_ais_frames goes, with the two places an int32 could creep in."""
    v = [int(x) for x in v]
    kept, closed = [], 0
    for s in range(24, len(v) + 1):
        total = sum(v[s - 24 : s - 8])
        if level32:
            total = int(wrap32(total))

        def m(j, total=total):
            return int((int(wrap32(16 * v[j])) if mul32 else 16 * v[j]) > total)

        b = [int(m(j) == m(j - 1)) for j in range(s - 22, s)]
        if b[14:] != FLAG_BITS or not all(b[k] != b[k + 1] for k in range(13)):
            continue
        out, cur, nb, ones, got = bytearray(), 0, 0, 0, None
        for j in range(s, len(v)):
            bit = int(m(j) == m(j - 1))
            if bit:
                ones += 1
                if ones == 6:
                    if j + 1 < len(v) and m(j + 1) != m(j) and nb == 6:
                        got = bytes(out)
                    break
            else:
                stuffed, ones = ones == 5, 0
                if stuffed:
                    continue
            cur |= bit << nb
            nb += 1
            if nb == 8:
                if len(out) == MAX_FRAME:
                    break
                out.append(cur)
                cur, nb = 0, 0
        if got is None or len(got) < MIN_FRAME:
            continue
        closed += 1
        if crc16(got[:-2]) == got[-2] | (got[-1] << 8):
            kept.append((s, got))
    return kept, closed


def entry_frames(planes, nsym, count_of, W, step, capacity, lst, slots, counts, **breaks) -> None:
    """iqa_ais_frames' checks, the cleared counters and the kernel's results in position order."""
    if nsym < 0 or capacity < 0:
        raise ValueError("negative length")
    if count_of is None:
        raise ValueError("NULL count table")
    if counts is None:
        raise ValueError("NULL device pointer")
    if not window_ok(W):
        raise ValueError("window must be 1 .. 3 IQA_AIS_MAX_SPS - 1")
    if not step_ok(step):
        raise ValueError("step must be sps / 8 with 5 <= sps <= IQA_AIS_MAX_SPS")
    if any(c < 0 or c > nsym for c in count_of):
        raise ValueError("count_of must be 0 .. nsym")
    if nsym > MAX_NSYM:
        raise ValueError("length out of range")
    if nsym > 0 and (planes is None or (capacity > 0 and (lst is None or slots is None))):
        raise ValueError("NULL device pointer")
    counts[:2] = 0
    if nsym == 0:
        return
    k = 0
    for p in range(PHASES):
        kept, closed = standin_frames_of(np.asarray(planes)[p * nsym : p * nsym + count_of[p]], **breaks)
        counts[1] += closed
        for s, raw in kept:
            counts[0] += 1
            if k < capacity:
                lst[4 * k : 4 * k + 4] = (p, s, instant_of(W, step, s, p), len(raw))
                slots[k * SLOT_BYTES : (k + 1) * SLOT_BYTES] = np.frombuffer(raw.ljust(SLOT_BYTES, b"\0"), dtype=np.uint8)
                k += 1


def frame_refusals() -> list:
    """(what, nsym, count_of | None, W, step, capacity, v?, list?, slots?, counts?, message)."""
    ok = [8] * PHASES
    yes = (True,) * 4
    return [("negative nsym", -1, ok, 29, 1.25, 4) + yes + ("negative",), ("negative capacity", 8, ok, 29, 1.25, -1) + yes + ("negative",),
            ("NULL count table", 8, None, 29, 1.25, 4) + yes + ("NULL count table",), ("NULL counts", 8, ok, 29, 1.25, 4, True, True, True, False, "NULL"),
            ("window 0", 8, ok, 0, 1.25, 4) + yes + ("window must be",), ("window 300", 8, ok, MAX_TAPS + 1, 1.25, 4) + yes + ("window must be",),
            ("step below 5/8", 8, ok, 29, 0.624, 4) + yes + ("step must be",), ("step above 100/8", 8, ok, 29, 12.51, 4) + yes + ("step must be",),
            ("a count above nsym", 8, [8, 8, 8, 9, 8, 8, 8, 8], 29, 1.25, 4) + yes + ("count_of must be",),
            ("a negative count", 8, [8, 8, 8, 8, 8, 8, 8, -1], 29, 1.25, 4) + yes + ("count_of must be",),
            ("nsym above 2^37", MAX_NSYM + 1, ok, 29, 1.25, 4) + yes + ("out of range",), ("NULL v", 8, ok, 29, 1.25, 4, False, True, True, True, "NULL"),
            ("NULL list", 8, ok, 29, 1.25, 4, True, False, True, True, "NULL"), ("NULL slots", 8, ok, 29, 1.25, 4, True, True, False, True, "NULL")]
