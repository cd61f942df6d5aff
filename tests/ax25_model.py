"""AX.25 / Bell-202 model for the tests (a helper module, not a test file): the encoder (addresses, CRC-16/X.25, bit
stuffing, flags, NRZI), an AFSK -> FM modulator to complex baseband with space-gain, clock and tuning knobs, and a plain
numpy oracle of DESIGN.md section 13 (steps 1-6).  The protocol constants are written out here from the AX.25 v2.2 text
on their own, not imported from the package, so that the encoder checks the decoder."""
from __future__ import annotations

import math

import numpy as np

BAUD = 1200
MARK, SPACE = 1200.0, 2200.0
FLAG = 0x7E
CRC_POLY = 0x8408  # x^16 + x^12 + x^5 + 1, reflected
CRC_RESIDUE = 0xF0B8  # the register (before the final xor) after a frame and its own FCS
MIN_FRAME, MAX_FRAME = 17, 330  # bytes, FCS included
MIN_SPS, MAX_SPS = 8.0, 400.0
THETA_SCALE = 4096.0
TAP_SCALE = 256.0
PHASES = 8
GAINS = ((1, 1), (1, 4), (4, 1))  # (a, b): d = a E_1200 - b E_2200
DEVIATION = 3000.0  # peak, of the louder tone


# ---- encoder -----------------------------------------------------------------------------------------------------------


def crc16(data: bytes) -> int:
    """CRC-16/X.25: reflected 0x8408, init 0xFFFF, final xor 0xFFFF."""
    reg = 0xFFFF
    for byte in data:
        reg ^= byte
        for _ in range(8):
            reg = (reg >> 1) ^ CRC_POLY if reg & 1 else reg >> 1
    return reg ^ 0xFFFF


def address(call: str, *, last: bool = False, high: bool = False) -> bytes:
    """"N0CALL-7" -> 7 bytes: six characters shifted left by one, then 0 11 SSID and the extension bit; ``high`` sets bit 7
    (the command bit of a destination, the has-been-repeated bit of a digipeater)."""
    name, _, ssid = call.partition("-")
    name = name.upper().ljust(6)
    assert len(name) == 6 and 0 <= int(ssid or 0) <= 15
    return bytes(ord(c) << 1 for c in name) + bytes([0x60 | (int(ssid or 0) << 1) | (0x80 if high else 0) | (1 if last else 0)])


def ui_frame(source: str, dest: str, path=(), info: str | bytes = b"", *, control: int = 0x03, pid: int | None = 0xF0) -> bytes:
    """The frame without flags, FCS appended low byte first.  A path entry ending in "*" has its H bit set."""
    info = info.encode("latin-1") if isinstance(info, str) else bytes(info)
    body = address(dest, high=True) + address(source, last=not path)
    for i, hop in enumerate(path):
        body += address(hop.rstrip("*"), last=i == len(path) - 1, high=hop.endswith("*"))
    body += bytes([control]) + (b"" if pid is None else bytes([pid])) + info
    fcs = crc16(body)
    return body + bytes([fcs & 0xFF, fcs >> 8])


def stuffed_bits(frame: bytes) -> list:
    """Frame bytes LSB first with a zero behind every five consecutive ones."""
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


FLAG_BITS = [0, 1, 1, 1, 1, 1, 1, 0]


def hdlc_bits(frames, *, preamble: int = 30, between: int = 1, postamble: int = 3) -> np.ndarray:
    """Data bits of one transmission: ``preamble`` flags, the frames with ``between`` flags between them, ``postamble``
    flags."""
    bits = FLAG_BITS * preamble
    for i, frame in enumerate(frames):
        if i:
            bits = bits + FLAG_BITS * between
        bits = bits + stuffed_bits(frame)
    bits = bits + FLAG_BITS * postamble
    return np.array(bits, dtype=np.uint8)


def nrzi(bits, first: int = 1) -> np.ndarray:
    """Data bits -> tone bits (1 = mark): a zero toggles the tone, a one keeps it."""
    out, tone = [], first
    for b in np.asarray(bits).tolist():
        if not b:
            tone ^= 1
        out.append(tone)
    return np.array(out, dtype=np.uint8)


# ---- modulator ---------------------------------------------------------------------------------------------------------


def modulate(bits, fs: float, *, space_gain: float = 1.0, offset_hz: float = 0.0, ppm: float = 0.0, sigma: float = 0.0,
             seed: int = 0, lead: int = 2000, tail: int = 2000) -> np.ndarray:
    """Data bits -> NRZI -> continuous-phase Bell-202 audio (mark 1200 Hz, space 2200 Hz at ``space_gain`` times the mark
    amplitude) -> FM (the louder tone peaks at 3 kHz deviation), the carrier ``offset_hz`` off tune, the bit clock ``ppm``
    fast; ``lead`` / ``tail`` samples without a carrier around it; complex AWGN of ``sigma`` per component over everything.
    complex64 at ``fs``."""
    tones = nrzi(bits).astype(np.int64)
    rate = BAUD * (1.0 + ppm * 1e-6)
    n = int(math.ceil(tones.size * fs / rate))
    idx = np.minimum((np.arange(n, dtype=np.float64) * rate / fs).astype(np.int64), tones.size - 1)
    mark = tones[idx] == 1
    audio_phase = 2.0 * np.pi * np.cumsum(np.where(mark, MARK, SPACE)) / fs
    audio = np.where(mark, 1.0, space_gain) * np.cos(audio_phase) / max(1.0, space_gain)
    x = np.exp(1j * 2.0 * np.pi * np.cumsum(DEVIATION * audio + offset_hz) / fs)
    x = np.concatenate([np.zeros(lead, dtype=np.complex128), x, np.zeros(tail, dtype=np.complex128)])
    if sigma > 0.0:
        rng = np.random.default_rng(seed)
        x = x + sigma * (rng.normal(size=x.size) + 1j * rng.normal(size=x.size))
    return x.astype(np.complex64)


def noise_only(n: int, sigma: float, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return (sigma * (rng.normal(size=n) + 1j * rng.normal(size=n))).astype(np.complex64)


# ---- oracle ------------------------------------------------------------------------------------------------------------


def theta_of(z) -> np.ndarray:
    """Step 1: the discriminator in float32, as numpy forms it (complex64 product, float32 angle)."""
    z = np.asarray(z, dtype=np.complex64)
    prev = np.concatenate([np.ones(1, dtype=np.complex64), z[:-1]])
    return np.angle(z * np.conj(prev)).astype(np.float32)


def quantise(theta) -> np.ndarray:
    return np.rint(np.asarray(theta, dtype=np.float32).astype(np.float64) * THETA_SCALE).astype(np.int32)


def plan(fs: float) -> dict:
    sps = float(fs) / BAUD
    if not (MIN_SPS <= sps <= MAX_SPS):
        raise ValueError("sps out of range")
    L = int(np.rint(sps))
    k = np.arange(L, dtype=np.float64)
    taps = {}
    for f in (1200, 2200):
        taps[f] = (np.rint(TAP_SCALE * np.cos(2.0 * np.pi * f * k / fs)).astype(np.int64),
                   np.rint(TAP_SCALE * np.sin(2.0 * np.pi * f * k / fs)).astype(np.int64))
    return dict(fs=float(fs), sps=sps, L=L, step=sps / 8.0, taps=taps)


def correlator_sums(t, pl) -> dict:
    """Step 2 -> {1200: (I, Q), 2200: (I, Q)} (int64), and the int32 range check of the sums."""
    t = np.asarray(t, dtype=np.int64)
    out = {}
    for f, (c, s) in pl["taps"].items():
        i = np.convolve(t, c)[: t.size]
        q = np.convolve(t, s)[: t.size]
        assert max(np.abs(i).max(initial=0), np.abs(q).max(initial=0)) < 2 ** 31
        out[f] = (i, q)
    return out


def energies(t, pl) -> dict:
    """Step 2 -> {1200: E, 2200: E} (int64)."""
    return {f: (i * i + q * q) >> 4 for f, (i, q) in correlator_sums(t, pl).items()}


def sign_plane(E) -> np.ndarray:
    sign = np.zeros(E[1200].size, dtype=np.uint8)
    for g, (a, b) in enumerate(GAINS):
        sign |= ((a * E[1200] - b * E[2200]) > 0).astype(np.uint8) << g
    return sign


def instants(pl, p: int, n: int) -> np.ndarray:
    """Bit instants of phase p that lie inside a stream of n samples."""
    i = np.arange(int(n / pl["sps"]) + 3, dtype=np.float64)
    at = pl["L"] - 1 + np.rint((8.0 * i + p) * pl["step"]).astype(np.int64)
    return at[at < n]


def bit_streams(sign, pl) -> list:
    """Step 4 -> 24 uint8 arrays (variant g * 8 + p) and their instants."""
    sign = np.asarray(sign)
    out = []
    for g in range(len(GAINS)):
        for p in range(PHASES):
            at = instants(pl, p, sign.size)
            m = (sign[at] >> g) & 1
            b = np.ones(m.size, dtype=np.uint8)
            b[1:] = m[1:] == m[:-1]
            out.append((b, at))
    return out


def walk(b, s: int):
    """Step 5 from an opened position: the frame bytes, or None (abort, too long, cut by the end of the stream)."""
    out, cur, nb, ones = bytearray(), 0, 0, 0
    for j in range(s, len(b)):
        bit = int(b[j])
        if bit:
            ones += 1
            if ones == 6:
                return bytes(out) if (j + 1 < len(b) and b[j + 1] == 0 and nb == 6) else None
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


def openers(b) -> np.ndarray:
    b = np.asarray(b, dtype=np.uint8)
    if b.size < 9:
        return np.zeros(0, dtype=np.int64)
    pad = np.concatenate([b, np.full(8, 2, dtype=np.uint8)])  # (2: no bit, so no flag)
    flag = np.ones(b.size + 1, dtype=bool)  # flag[j]: pad[j .. j+7] is the flag
    for k, v in enumerate(FLAG_BITS):
        flag &= pad[k : k + b.size + 1] == v
    s = np.arange(8, b.size + 1)
    return s[flag[s - 8] & ~flag[s]]


def frames_of(b) -> tuple:
    """Step 5 on one bit stream -> ([(s, bytes)] kept, candidates closed with >= 17 bytes)."""
    kept, closed = [], 0
    for s in openers(b).tolist():
        got = walk(b, s)
        if got is None or len(got) < MIN_FRAME:
            continue
        closed += 1
        if crc16(got[:-2]) == got[-2] | (got[-1] << 8):
            kept.append((s, got))
    return kept, closed


def call_of(field: bytes) -> str | None:
    name = "".join(chr(c >> 1) for c in field[:6])
    if any(c & 1 for c in field[:6]) or any(ch not in "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 " for ch in name):
        return None
    ssid = (field[6] >> 1) & 15
    return name.rstrip() + (f"-{ssid}" if ssid else "")


def parse(raw: bytes) -> dict | None:
    """Step 6 on one CRC-checked frame -> dict(source, dest, path, control, pid, info), or None for a bad address field."""
    body = raw[:-2]
    calls = []
    for k in range(10):
        field = body[7 * k : 7 * k + 7]
        if len(field) < 7 or call_of(field) is None:
            return None
        calls.append((call_of(field), bool(field[6] & 0x80)))
        if field[6] & 1:
            break
    else:
        return None
    if len(calls) < 2 or len(body) < 7 * len(calls) + 1:
        return None
    rest = body[7 * len(calls) :]
    control = rest[0]
    ui = control == 0x03 and len(rest) >= 2 and rest[1] == 0xF0
    pid = rest[1] if ((control & 0xEF) == 0x03 or (control & 1) == 0) and len(rest) >= 2 else None
    info = rest[2:] if pid is not None else rest[1:]
    text = "".join(chr(c) if 0x20 <= c <= 0x7E else "�" for c in info) if ui else info.hex()
    return dict(dest=calls[0][0], source=calls[1][0], path=[c + ("*" if h else "") for c, h in calls[2:]], control=control, pid=pid,
                info=text, raw=raw.hex())


def merge(records, L: int) -> list:
    """[(variant, s, instant, bytes)] -> [(instant, bytes, hits)]: sorted by instant; identical bytes whose start instants
    differ by <= L from the group's first are one frame."""
    out = []
    for v, s, at, raw in sorted(records, key=lambda r: (r[2], r[0])):
        same = [grp for grp in out if grp[1] == raw and at - grp[0] <= L]
        if same:
            same[-1][2] += 1
        else:
            out.append([at, raw, 1])
    return [tuple(grp) for grp in out]


def oracle(theta=None, fs: float = 96_000.0, *, t=None) -> dict:
    """Steps 1-6 from a discriminator output (or from given ``t``)."""
    pl = plan(fs)
    t = quantise(theta) if t is None else np.asarray(t, dtype=np.int32)
    E = energies(t, pl)
    sign = sign_plane(E)
    streams = bit_streams(sign, pl)
    records, closed = [], 0
    for v, (b, at) in enumerate(streams):
        kept, c = frames_of(b)
        closed += c
        records += [(v, s, int(at[s]), raw) for s, raw in kept]
    records.sort(key=lambda r: (r[0], r[1]))
    frames, rejected = [], 0
    for at, raw, hits in merge(records, pl["L"]):
        got = parse(raw)
        if got is None:
            rejected += 1
            continue
        frames.append(dict(got, time_s=at / pl["fs"], hits=hits))
    return dict(t=t, E=E, sign=sign, bits=[b for b, _ in streams], records=records, closed=closed, frames=frames, rejected=rejected)


def tnc2(frame: dict) -> str:
    return f"{frame['source']}>{','.join([frame['dest']] + list(frame['path']))}:{frame['info']}"


# ---- crafted inputs for the edge-shape tests (tests/test_ax25_shapes_host.py, tests/test_gpu_ax25_shapes.py) -------------

T_PI = 12_868  # rint(float32(pi) 4096): the largest |t| a discriminator produces
EDGE_RATES = (9_600.0, 12_600.0, 97_200.0, 100_800.0)  # L 8 (step 1), L 10 (sps 10.5, step 21/16), L 81, L 84 (step 10.5)
TIE_RATES = (12_600.0, 97_200.0, 100_800.0)  # (at step 10.125 phase 4 is a tie: 4 x 10.125 = 40.5)
EDGE_WINDOWS = (8, 9, 15, 16, 17, 393, 399, 400)
EDGE_LENGTHS = (1, 7, 8, 9, 15, 2047, 2048, 2049, 2055)
EDGE_FRAME = ("N0CALL-7", "APRS", ["WIDE1-1*", "WIDE2-1"], "!4903.50N/07201.75W-edge rates")


def edge_stream(fs: float) -> np.ndarray:
    return modulate(hdlc_bits([ui_frame(*EDGE_FRAME)]), fs, sigma=0.05, seed=3)


def tie_instants(pl, n: int) -> list:
    """[(i, p)] whose product (8 i + p) step lies exactly on a half and whose instant is inside n samples."""
    out = []
    for p in range(PHASES):
        i = np.arange(instants(pl, p, n).size, dtype=np.float64)
        x = (8.0 * i + p) * pl["step"]
        out += [(int(k), p) for k in np.nonzero(x - np.floor(x) == 0.5)[0]]
    return out


def crafted_theta(L: int, n: int, seed: int) -> np.ndarray:
    """float32[n] over [-pi, pi] at fs = 1200 L: random values, and (where n has room) two stretches of 2 L samples of a
    full-scale square wave pi sign(cos(2 pi f k / fs)), f = 1200 and f = 2200: the correlators' largest sums."""
    rng = np.random.default_rng(seed)
    pi32 = np.float32(np.pi)
    th = np.clip(rng.uniform(-np.pi, np.pi, n).astype(np.float32), -pi32, pi32)
    k = np.arange(2 * L, dtype=np.float64)
    at = 100
    for f in (MARK, SPACE):
        if at + 2 * L <= n:
            th[at : at + 2 * L] = np.where(np.cos(2.0 * np.pi * f * k / (1200.0 * L)) >= 0.0, pi32, -pi32)
        at += 2 * L + 55
    return th


def crafted_history(L: int, seed: int) -> np.ndarray:
    """int32[L - 1] with |v| <= T_PI, both extremes present."""
    h = np.random.default_rng(seed).integers(-T_PI, T_PI + 1, size=L - 1).astype(np.int32)
    h[0], h[-1] = T_PI, -T_PI
    return h


def correlate_block(theta, hist, pl) -> tuple:
    """What ``iqa_afsk_correlate`` owes for one block: (t, {f: E}, sign, {f: (I, Q)})."""
    t = quantise(theta)
    front = np.zeros(pl["L"] - 1, dtype=np.int64) if hist is None else np.asarray(hist, dtype=np.int64)
    assert front.size == pl["L"] - 1
    sums = {f: (i[front.size :], q[front.size :]) for f, (i, q) in correlator_sums(np.concatenate([front, t.astype(np.int64)]), pl).items()}
    E = {f: (i * i + q * q) >> 4 for f, (i, q) in sums.items()}
    return t, E, sign_plane(E), sums


def bits_plane(sign, pl, nbits: int) -> np.ndarray:
    """What ``iqa_afsk_bits`` owes: uint8[24, nbits], the bit streams with zeros where a bit's instant is beyond the plane."""
    out = np.zeros((len(GAINS) * PHASES, nbits), dtype=np.uint8)
    for v, (b, _at) in enumerate(bit_streams(sign, pl)):
        assert b.size <= nbits
        out[v, : b.size] = b
    return out


def bits_case(pl, i: int = 37, p: int = 3, seed: int = 0) -> tuple:
    """(plane, n): a random slicer plane (bytes 0 .. 7) whose last sample is the instant of bit i at phase p."""
    n = int(pl["L"] - 1 + np.rint((8.0 * i + p) * pl["step"])) + 1
    return np.random.default_rng(seed).integers(0, 8, size=n).astype(np.uint8), n
