"""POCSAG model for the tests (a helper module, not a test file): the encoder (BCH(31,21) and parity, frames by address,
idle fill, preamble, batches), a 2-FSK modulator to complex baseband, and a plain numpy oracle of DESIGN.md section 12
(stages 1-5).  The constants and the arithmetic are written out here on their own, not imported from the package, so that
the encoder checks the decoder."""
from __future__ import annotations

import math

import numpy as np

G = 0x769  # x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1
SYNC = 0x7CD215D8
IDLE = 0x7A89C197
BAUDS = (512, 1200, 2400)
DEVIATION = 4500.0
NUMERIC = "0123456789*U -]["
MIN_SPS, MAX_SPS = 8.0, 384.0


# ---- encoder -----------------------------------------------------------------------------------------------------------


def bch_remainder(v31: int) -> int:
    """v31 (31 bits) modulo g, by long division."""
    r = v31
    for i in range(30, 9, -1):
        if (r >> i) & 1:
            r ^= G << (i - 10)
    return r & 0x3FF


def syndrome(cw: int) -> int:
    return bch_remainder(cw >> 1)


def parity(cw: int) -> int:
    return bin(cw & 0xFFFFFFFF).count("1") & 1


def codeword(data21: int) -> int:
    """21 information bits (flag first) -> the 32-bit codeword: 10 check bits, then even parity."""
    v = (data21 << 10) | bch_remainder(data21 << 10)
    return (v << 1) | (bin(v).count("1") & 1)


def address_word(address: int, function: int) -> int:
    return codeword(((address >> 3) & 0x3FFFF) << 2 | (function & 3))


def message_word(bits20: int) -> int:
    return codeword((1 << 20) | (bits20 & 0xFFFFF))


def numeric_bits(text: str) -> list:
    out = []
    for ch in text:
        v = NUMERIC.index(ch)
        out += [(v >> k) & 1 for k in range(4)]  # each digit LSB first
    return out


def alpha_bits(text: str) -> list:
    out = []
    for ch in text:
        out += [(ord(ch) >> k) & 1 for k in range(7)]  # each character LSB first
    return out


def message_words(address: int, function: int, text: str) -> list:
    """The address codeword and the message codewords of one message (numeric for function 0, alpha otherwise); the last
    codeword is padded with the numeric space (0xC) / with zero bits (NUL)."""
    bits = numeric_bits(text) if function == 0 else alpha_bits(text)
    if function == 0:
        while len(bits) % 20:
            bits += [0, 0, 1, 1]  # 0xC LSB first
    else:
        bits += [0] * (-len(bits) % 20)
    words = [address_word(address, function)]
    for i in range(0, len(bits), 20):
        words.append(message_word(int("".join(map(str, bits[i : i + 20])), 2)))
    return words


def batches_of(messages) -> list:
    """[(address, function, text), ...] -> batches of 16 codewords: every address codeword in frame ``address & 7``,
    message codewords behind it (running on into the next batch), idle everywhere else."""
    slots: list = []
    for address, function, text in messages:
        words = message_words(address, function, text)
        at = len(slots)
        while (at % 16) // 2 != (address & 7):
            at += 1
        slots += [IDLE] * (at - len(slots)) + words
    slots += [IDLE] * (-len(slots) % 16)
    if not slots:
        slots = [IDLE] * 16
    return [slots[i : i + 16] for i in range(0, len(slots), 16)]


def transmission_bits(messages, preamble: int = 576) -> np.ndarray:
    """Preamble (alternating, 1 first), then per batch the sync word and 16 codewords, every word MSB first."""
    bits = [(i + 1) & 1 for i in range(preamble)]
    for batch in batches_of(messages):
        for w in [SYNC] + batch:
            bits += [(w >> k) & 1 for k in range(31, -1, -1)]
    return np.array(bits, dtype=np.uint8)


# ---- modulator ---------------------------------------------------------------------------------------------------------


def modulate(bits, fs: float, baud: int, *, inverted: bool = False, offset_hz: float = 0.0, ppm: float = 0.0, sigma: float = 0.0,
             seed: int = 0, lead: int = 3000, tail: int = 3000, amplitude: float = 1.0) -> np.ndarray:
    """2-FSK at +-4.5 kHz, lower frequency = 1 (``inverted`` swaps them), the carrier ``offset_hz`` off tune, the bit clock
    ``ppm`` fast; ``lead`` and ``tail`` samples without a carrier around it; complex AWGN of ``sigma`` per component over
    everything.  complex64 at ``fs``."""
    bits = np.asarray(bits, dtype=np.int64)
    rate = baud * (1.0 + ppm * 1e-6)
    n = int(math.ceil(bits.size * fs / rate))
    idx = np.minimum((np.arange(n, dtype=np.float64) * rate / fs).astype(np.int64), bits.size - 1)
    f = np.where(bits[idx] == 1, -DEVIATION, DEVIATION) * (-1.0 if inverted else 1.0) + offset_hz
    x = amplitude * np.exp(1j * 2.0 * np.pi * np.cumsum(f) / fs)
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
    """Stage 1: the discriminator in float32, as numpy forms it (complex64 product, float32 angle)."""
    z = np.asarray(z, dtype=np.complex64)
    prev = np.concatenate([np.ones(1, dtype=np.complex64), z[:-1]])
    return np.angle(z * np.conj(prev)).astype(np.float32)


def shown(function: int, text: str) -> str:
    """What a decoder shows for a sent message: a numeric message is padded with spaces to whole codewords (5 digits)."""
    return text + " " * (-len(text) % 5) if function == 0 else text


def quantise(theta) -> np.ndarray:
    return np.rint(np.asarray(theta, dtype=np.float32).astype(np.float64) * 2.0 ** 20).astype(np.int32)


def baud_plan(fs: float, baud: int):
    sps = float(fs) / baud
    if sps < MIN_SPS or sps > MAX_SPS:
        return None
    return dict(baud=baud, sps=sps, L=int(np.rint(sps)), h=int(math.floor(sps / 2.0)),
                off=np.rint(np.arange(545, dtype=np.float64) * sps).astype(np.int64))


def integrate(t, L: int) -> np.ndarray:
    c = np.concatenate([np.zeros(L, dtype=np.int64), np.cumsum(np.asarray(t, dtype=np.int64))])
    return (c[L:] - c[:-L]).astype(np.int32)


def sync_search(S, bp, stats: dict | None = None) -> list:
    """Stage 3 -> kept syncs [(n0, Sigma0, inverted, distance)], ascending n0.  ``stats`` collects how many positions pass
    the distance test and how many of those the eye gate removes."""
    S = np.asarray(S, dtype=np.int64)
    off = bp["off"]
    m = S.size - int(off[31])
    if m <= 0:
        return []
    v = np.stack([S[int(off[i]) : int(off[i]) + m] for i in range(32)])
    sigma = v.sum(axis=0)
    x = 32 * v - sigma
    word = np.zeros(m, dtype=np.int64)
    for i in range(32):
        word = (word << 1) | (x[i] < 0)
    diff = word ^ SYNC
    dp = np.zeros(m, dtype=np.int64)
    for k in range(32):
        dp += (diff >> k) & 1
    dn = 32 - dp
    ax = np.abs(x)
    energy = ax.sum(axis=0)
    near = np.minimum(dp, dn) <= 2
    cand = near & (128 * ax.min(axis=0) >= energy)
    if stats is not None:
        stats["near"] = stats.get("near", 0) + int(near.sum())
        stats["gated"] = stats.get("gated", 0) + int((near & ~cand).sum())
    at = np.nonzero(cand)[0]
    kept = []
    for n in at.tolist():
        lo, hi = np.searchsorted(at, n - bp["h"]), np.searchsorted(at, n + bp["h"], side="right")
        others = at[lo:hi]
        e = energy[n]
        if np.any((energy[others] > e) | ((energy[others] == e) & (others < n))):
            continue
        kept.append((n, int(sigma[n]), bool(dn[n] < dp[n]), int(min(dp[n], dn[n]))))
    return kept


SINGLE = {syndrome(1 << pos): pos for pos in range(1, 32)}


def correct(raw: int):
    """-> (word, status): 0 accepted, 1 one bit flipped, 2 uncorrectable (the raw word)."""
    s, p = syndrome(raw), parity(raw)
    if s == 0:
        return (raw ^ 1, 1) if p else (raw, 0)
    if p and s in SINGLE:
        return raw ^ (1 << SINGLE[s]), 1
    return raw, 2


def read_batch(S, bp, n0: int, sigma0: int, inverted: bool):
    """Stage 4 -> (corrected[16], raw[16], status[16])."""
    S = np.asarray(S, dtype=np.int64)
    off = bp["off"]
    fixed, raws, status = [], [], []
    for c in range(16):
        base = 32 * (1 + c)
        if n0 + int(off[base + 31]) > S.size - 1:
            fixed.append(0), raws.append(0), status.append(3)
            continue
        raw = 0
        for b in range(32):
            raw = (raw << 1) | (int(32 * S[n0 + int(off[base + b])] < sigma0) ^ int(inverted))
        w, st = correct(raw)
        fixed.append(w), raws.append(raw), status.append(st)
    return fixed, raws, status


def _numeric(bits) -> str:
    return "".join(NUMERIC[sum(bits[i + k] << k for k in range(4))] for i in range(0, len(bits) - 3, 4))


def _alpha(bits) -> str:
    codes = [sum(bits[i + k] << k for k in range(7)) for i in range(0, len(bits) - 6, 7)]
    while codes and codes[-1] in (0, 3, 4):
        codes.pop()
    return "".join(chr(c) if 0x20 <= c <= 0x7E else "�" for c in codes)


def messages_of(bp, fs: float, batches: list) -> list:
    """Stage 5 on [(n0, inverted, words[16], status[16])] ascending in n0 -> [dict(address, function, text, ...)]."""
    out, cur, bits = [], None, []

    def close():
        nonlocal cur, bits
        if cur is not None:
            cur["payload_bits"] = len(bits)
            cur["text"] = _numeric(bits) if cur["function"] == 0 else _alpha(bits)
            out.append(cur)
        cur, bits = None, []

    last = None
    for n0, inverted, words, status in batches:
        if last is not None and abs(n0 - (last + int(bp["off"][544]))) > bp["h"]:
            close()
        last = n0
        if cur is not None:
            cur["batches"] += 1
        for c in range(16):
            cw, st = int(words[c]), int(status[c])
            if st >= 2 or cw == IDLE:
                close()
            elif cw >> 31 == 0:
                close()
                cur = dict(time_s=(n0 + int(bp["off"][32 * (1 + c)])) / fs, baud=bp["baud"], inverted=bool(inverted),
                           address=((cw >> 13) & 0x3FFFF) << 3 | (c >> 1), function=(cw >> 11) & 3, corrected=int(st == 1), batches=1)
            elif cur is not None:
                cur["corrected"] += int(st == 1)
                bits += [(cw >> s) & 1 for s in range(30, 10, -1)]
    close()
    return out


def oracle(theta=None, fs: float = 96_000.0, *, t=None, stats: dict | None = None) -> dict:
    """Stages 1-5 from a discriminator output (or from given ``t``): ``t``, per baud ``S``, kept syncs, the batches'
    corrected / raw words and status, and all messages in order of time."""
    t = quantise(theta) if t is None else np.asarray(t, dtype=np.int32)
    out = dict(t=t, S={}, syncs={}, batches={}, messages=[], skipped=[])
    for baud in BAUDS:
        bp = baud_plan(fs, baud)
        if bp is None:
            out["skipped"].append(baud)
            continue
        S = integrate(t, bp["L"])
        kept = sync_search(S, bp, stats)
        rows = []
        for n0, sigma0, inverted, _d in kept:
            fixed, raws, status = read_batch(S, bp, n0, sigma0, inverted)
            rows.append((n0, inverted, fixed, raws, status))
        out["S"][baud], out["syncs"][baud] = S, kept
        out["batches"][baud] = dict(words=np.array([r[2] for r in rows], dtype=np.uint32).reshape(-1, 16),
                                    raw=np.array([r[3] for r in rows], dtype=np.uint32).reshape(-1, 16),
                                    status=np.array([r[4] for r in rows], dtype=np.uint8).reshape(-1, 16))
        out["messages"] += messages_of(bp, fs, [(r[0], r[1], r[2], r[4]) for r in rows])
    out["messages"].sort(key=lambda m: (m["time_s"], m["baud"]))
    return out


def triples(messages) -> list:
    """(address, function, text) of dict or dataclass messages."""
    get = (lambda m, k: m[k]) if messages and isinstance(messages[0], dict) else getattr
    return [(get(m, "address"), get(m, "function"), get(m, "text")) for m in messages]


# ---- crafted inputs for the edge-shape tests (tests/test_pocsag_shapes_host.py, tests/test_gpu_pocsag_shapes.py) ---------

T_PI = 3_294_199  # rint(float32(pi) 2^20): the largest |t| a discriminator produces
EDGE_RATES = {  # fs -> (bauds skipped, {baud: offsets i of 545 whose i sps is a half-even tie})
    4_096.0: ([1200, 2400], {512: 0}),
    9_600.0: ([2400], {512: 136, 1200: 0}),
    19_200.0: ([], {512: 272, 1200: 0, 2400: 0}),
    96_600.0: ([], {512: 9, 1200: 272, 2400: 136}),
    196_608.0: ([], {512: 0, 1200: 0, 2400: 0}),
    196_609.0: ([512], {1200: 0, 2400: 0}),
    921_600.0: ([512, 1200], {2400: 0}),
}
EDGE_MESSAGES = [(424242, 0, "0123456789"), (77, 1, "ok")]


def tie_count(sps: float) -> int:
    """How many of the 545 products i sps lie on a half: rint rounds those to even."""
    frac = np.mod(np.arange(545, dtype=np.float64) * sps, 1.0)
    return int((np.abs(frac - 0.5) < 1e-12).sum())


def edge_stream(fs: float) -> np.ndarray:
    """One transmission of EDGE_MESSAGES (one batch) per baud that fits ``fs``, behind one another."""
    bits = transmission_bits(EDGE_MESSAGES)
    parts = []
    for baud in BAUDS:
        if baud_plan(fs, baud) is not None:
            pad = int(3 * fs / baud) + 50
            parts.append(modulate(bits, fs, baud, sigma=0.05, seed=baud, lead=pad, tail=pad))
    return np.concatenate(parts)


def crafted_theta(n: int, l_max: int, seed: int) -> np.ndarray:
    """float32[n] over [-pi, pi]: random values, every fourth one of the form (k + 0.5) / 2^20 (a tie of the quantiser),
    and, where n has room for them, 2 l_max samples held at +pi and 2 l_max at -pi (the integrators' full scale)."""
    rng = np.random.default_rng(seed)
    pi32 = np.float32(np.pi)
    th = np.clip(rng.uniform(-np.pi, np.pi, n).astype(np.float32), -pi32, pi32)
    k = rng.integers(-T_PI + 1, T_PI - 1, size=n)
    ties = ((k.astype(np.float64) + 0.5) / 2.0 ** 20).astype(np.float32)
    assert np.array_equal(ties.astype(np.float64) * 2.0 ** 20, k + 0.5)  # exact in float32
    th[::4] = ties[::4]
    if n >= 100 + 4 * l_max:
        th[50 : 50 + 2 * l_max] = pi32
        th[100 + 2 * l_max : 100 + 4 * l_max] = -pi32
    return th


def crafted_history(hist_len: int, seed: int) -> np.ndarray:
    """int32[hist_len] with |v| <= T_PI, the last third held at +T_PI."""
    rng = np.random.default_rng(seed)
    h = rng.integers(-T_PI, T_PI + 1, size=hist_len).astype(np.int32)
    h[hist_len - hist_len // 3 :] = T_PI
    return h


def integrate_block(theta, hist, hist_len: int, windows) -> tuple:
    """What ``iqa_pocsag_integrate`` owes for one block: t and, per window, S (None where the window is 0)."""
    t = quantise(theta)
    front = np.zeros(hist_len, dtype=np.int64) if hist is None else np.asarray(hist, dtype=np.int64)
    assert front.size == hist_len
    joined = np.concatenate([front, t.astype(np.int64)])
    return t, [None if L == 0 else integrate(joined, L)[hist_len:] for L in windows]


def word_levels(word: int, amplitude: int = 1000, inverted: bool = False) -> list:
    """The 32 integrator levels of a word, first bit first: a 1 is -amplitude (x < 0), ``inverted`` swaps the signs."""
    sign = -1 if inverted else 1
    return [sign * (-amplitude if (word >> k) & 1 else amplitude) for k in range(31, -1, -1)]


def crafted_plane(bp, starts, levels, n: int | None = None, tail: int = 40) -> np.ndarray:
    """An integrator plane built straight from bit levels: for every start a and its list of levels, level i is held over
    [a + off[i], a + off[i + 1]); zeros everywhere else.  Every position of the first bit period then sees the same 32
    values: a plateau of candidates with identical energy.  int32[n] (default: ``tail`` zeros behind the last level)."""
    off = bp["off"]
    size = max(a + int(off[len(lv)]) for a, lv in zip(starts, levels)) + tail
    S = np.zeros(size, dtype=np.int32)
    for a, lv in zip(starts, levels):
        for i, v in enumerate(lv):
            S[a + int(off[i]) : a + int(off[i + 1])] = v
    if n is not None:
        S = S[:n].copy() if n <= size else np.concatenate([S, np.zeros(n - size, dtype=np.int32)])
    return S


def flipped(word: int, positions) -> int:
    """``word`` with the bits at ``positions`` (counted from the first transmitted bit) inverted."""
    for p in positions:
        word ^= 1 << (31 - p)
    return word


def error_words(word: int, triples: int = 500, seed: int = 7) -> dict:
    """Damaged copies of one codeword: all 32 single and all 496 double errors, and ``triples`` distinct triple errors."""
    from itertools import combinations

    rng = np.random.default_rng(seed)
    all3 = list(combinations(range(32), 3))
    pick = rng.choice(len(all3), size=triples, replace=False)
    return dict(clean=[word], single=[flipped(word, (a,)) for a in range(32)],
                double=[flipped(word, c) for c in combinations(range(32), 2)],
                triple=[flipped(word, all3[k]) for k in sorted(pick.tolist())])


def batch_plane(bp, words, lead: int = 40, gap: int = 100, amplitude: int = 1000) -> tuple:
    """``words`` in batches of 16 (the last one filled with idle words), each behind its own sync word, ``gap`` zeros between
    batches -> (plane, starts, batches)."""
    words = list(words) + [IDLE] * (-len(words) % 16)
    batches = [words[i : i + 16] for i in range(0, len(words), 16)]
    span = int(bp["off"][544]) + gap
    starts = [lead + k * span for k in range(len(batches))]
    levels = [sum((word_levels(w, amplitude) for w in [SYNC] + b), []) for b in batches]
    return crafted_plane(bp, starts, levels), starts, batches


def eye_gate_flip(bp, amplitude: int, lead: int = 40) -> tuple:
    """Shrinks the level of the sync word's first bit from ``amplitude`` downwards until the model drops the sync ->
    (the last level kept, the plane at it, the plane one below), or None if the sync is never dropped."""
    base = word_levels(SYNC, amplitude)

    def plane(level):
        return crafted_plane(bp, [lead], [[level] + base[1:]])

    for level in range(amplitude, 0, -1):
        if not sync_search(plane(level - 1), bp):
            return (level, plane(level), plane(level - 1)) if sync_search(plane(level), bp) else None
    return None


def eye_gate_terms(S, bp, n0: int) -> tuple:
    """(128 min |x_i|, E) at position n0."""
    v = np.asarray(S, dtype=np.int64)[n0 + bp["off"][:32]]
    x = 32 * v - v.sum()
    return int(128 * np.abs(x).min()), int(np.abs(x).sum())
