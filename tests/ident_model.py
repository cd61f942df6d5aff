"""Numpy oracle of the protocol identification (--find-identify): one function per step, written from the
specification, with its own copy of the sync words.  Of the package it uses nothing; the quantiser, the keying and the model
conventions are ``keying_model``'s.  Everything behind ``quantise`` is integer, so the kernels are held to ``integrate``,
``score`` and ``keep`` bit for bit.  The steps come twice: in plain Python loops (``*_by_loops``, for small streams) and
vectorised for the model capture; the host test holds the two to each other.  Also a 4-level FSK synthesiser, ``crafted_plane``
(v written straight from symbol levels) and the model capture of the tests: seven channels of known protocol."""
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


K = _load("keying_model")
M = K.M
FM = K.FM

# (protocol, name for C > 0, name for C < 0, word, symbols N, grid G, families, binary)
PATTERNS = (
    ("dmr", "dmr bs voice", "dmr bs data", 0x755FD7DF75F7, 24, 144, (4800,), False),
    ("dmr", "dmr ms voice", "dmr ms data", 0x7F7D5DD57DFD, 24, 144, (4800,), False),
    ("p25", "p25", "p25 inverted", 0x5575F5FF77FF, 24, 36, (4800,), False),
    ("ysf", "ysf", "ysf inverted", 0xD471C9634D, 20, 480, (4800,), False),
    ("nxdn", "nxdn", "nxdn inverted", 0xCDF59, 10, 192, (4800, 2400), False),
    ("flex", "flex", "flex inverted", 0xA6C6AAAA, 32, 3000, (1600,), True),
)
PROTOCOLS = ("dmr", "p25", "ysf", "nxdn", "flex")
LEVEL = {0b01: 3, 0b00: 1, 0b10: -1, 0b11: -3}
FAMILY = {1600: 1600, 3200: 1600, 2400: 2400, 4800: 4800}
MODES = ((0x870C, "1600/2"), (0xB068, "1600/4"), (0x7B18, "3200/2"), (0xDEA0, "3200/4"))
NUM, DEN = 13, 16  # the threshold: 16 C^2 >= 13 Pn E
V_MAX = 64 * 65534


def symbols(pat) -> list:
    """The symbols of a pattern, first sent first."""
    _, _, _, word, n, _, _, binary = pat
    if binary:
        return [1 if (word >> (n - 1 - i)) & 1 else -1 for i in range(n)]
    return [LEVEL[(word >> (2 * (n - 1 - i))) & 3] for i in range(n)]


def family(rate: int) -> list:
    return [p for p in PATTERNS if rate in p[6]]


# ---- the plan ----------------------------------------------------------------------------------------------------------------


def plan(fs_ch: float, rate: int) -> dict:
    """sps, L, h, sh and o[-16 .. 47] (``o`` a dict by symbol index); ValueError unless 4 <= sps <= 224."""
    sps = float(fs_ch) / rate
    if not 4.0 <= sps <= 224.0:
        raise ValueError("rate does not fit")
    L = int(round(sps))  # (Python's round: half-even)
    return dict(fs_ch=float(fs_ch), rate=rate, sps=sps, L=L, h=int(math.floor(sps / 2.0)), sh=max(0, (L - 1).bit_length() - 6),
                o={i: int(round(i * sps)) for i in range(-16, 48)})


# ---- the integrator ----------------------------------------------------------------------------------------------------------


def integrate_by_loops(theta, c: int, L: int, sh: int) -> list:
    t = [int(x) for x in K.quantise(theta)]
    out = []
    for m in range(len(t)):
        s = 0
        for j in range(L):
            if m - j >= 0:
                s += t[m - j] - c
        out.append(s >> sh)  # (Python's shift of a negative integer is arithmetic)
    return out


def integrate(theta, c: int, L: int, sh: int) -> np.ndarray:
    """int64[n]: v = (sum of t - c over the last L samples, none in front of the stream) >> sh."""
    d = K.quantise(theta) - int(c)
    cs = np.concatenate(([0], np.cumsum(d)))
    m = np.arange(d.size)
    return (cs[m + 1] - cs[np.maximum(m + 1 - L, 0)]) >> sh


# ---- the search ----------------------------------------------------------------------------------------------------------------


def score_by_loops(v, pl: dict, pats) -> list:
    """Per pattern the list of 2 |C| + (C < 0) for a candidate, 0 for every other m."""
    v = [int(x) for x in v]
    n = len(v)
    out = []
    for pat in pats:
        sym = symbols(pat)
        pn = sum(s * s for s in sym)
        row = [0] * n
        for m in range(n):
            if m + pl["o"][len(sym) - 1] >= n:
                continue
            C = sum(s * v[m + pl["o"][i]] for i, s in enumerate(sym))
            E = sum(v[m + pl["o"][i]] ** 2 for i in range(len(sym)))
            if E > 0 and DEN * C * C >= NUM * pn * E:
                row[m] = 2 * abs(C) + (1 if C < 0 else 0)
        out.append(row)
    return out


def correlate(v, pl: dict, pat) -> tuple:
    """(C, E) as int64 arrays over the evaluated positions m = 0 .. n - o[N - 1] - 1."""
    v = np.asarray(v, dtype=np.int64)
    sym = symbols(pat)
    k = max(v.size - pl["o"][len(sym) - 1], 0)
    C, E = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
    for i, s in enumerate(sym):
        x = v[pl["o"][i] : pl["o"][i] + k]
        C += s * x
        E += x * x
    return C, E


def score(v, pl: dict, pats) -> np.ndarray:
    """int64[len(pats)][n]."""
    v = np.asarray(v, dtype=np.int64)
    assert v.size == 0 or np.abs(v).max() <= V_MAX  # (then every product below stays inside int64)
    out = np.zeros((len(pats), v.size), dtype=np.int64)
    for j, pat in enumerate(pats):
        C, E = correlate(v, pl, pat)
        pn = sum(s * s for s in symbols(pat))
        cand = (E > 0) & (DEN * C * C >= NUM * pn * E)
        out[j, : C.size] = np.where(cand, 2 * np.abs(C) + (C < 0), 0)
    return out


def keep(v, planes, pl: dict, pats) -> list:
    """The kept hits as (pattern, m, C, E, pre, post), sorted by (pattern, m)."""
    v = [int(x) for x in np.asarray(v).tolist()]
    n = len(v)
    out = []
    for j, pat in enumerate(pats):
        sym = symbols(pat)
        N = len(sym)
        row = np.asarray(planes[j], dtype=np.int64)
        for m in np.flatnonzero(row).tolist():
            mine = int(row[m]) >> 1
            lo, hi = max(m - pl["h"], 0), min(m + pl["h"], n - 1)
            near = row[lo : hi + 1] >> 1
            if int(near.max()) > mine or bool((near[: m - lo] == mine).any()):
                continue
            C = sum(s * v[m + pl["o"][i]] for i, s in enumerate(sym))
            E = sum(v[m + pl["o"][i]] ** 2 for i in range(N))
            pre = sum(1 << k for k in range(16) if 0 <= m + pl["o"][-16 + k] < n and v[m + pl["o"][-16 + k]] > 0)
            post = sum(1 << k for k in range(16) if 0 <= m + pl["o"][N + k] < n and v[m + pl["o"][N + k]] > 0)
            out.append((j, m, C, E, pre, post))
    return out


def search(v, pl: dict, pats) -> tuple:
    planes = score(v, pl, pats)
    return planes, keep(v, planes, pl, pats)


# ---- the rules -----------------------------------------------------------------------------------------------------------------


def popcount(x: int) -> int:
    return bin(x & 0xFFFF).count("1")


def in_order(bits: int) -> int:
    """pre / post (bit k the k-th in time) as a word sent MSB first."""
    return sum(((bits >> k) & 1) << (15 - k) for k in range(16))


def flex_words(pre: int, post: int, inverted: bool) -> tuple:
    a, b = in_order(pre), in_order(post)
    return (a ^ 0xFFFF, b ^ 0xFFFF) if inverted else (a, b)


def flex_mode(a: int, b: int):
    """None where the hit does not count, else its mode or ``?``."""
    if popcount(a ^ b ^ 0xFFFF) > 3:
        return None
    for code, name in MODES:
        if popcount(a ^ code) + popcount(b ^ 0xFFFF ^ code) <= 3:
            return name
    return "?"


def on_grid(d: int, G: int, pl: dict) -> bool:
    k = 1
    while True:
        at = int(round(k * G * pl["sps"]))
        if abs(d - at) <= pl["h"]:
            return True
        if at > d + pl["h"]:
            return False
        k += 1


def decide(hits, pats, pl: dict) -> dict:
    """hits per name, pairs per protocol (a hit against the nearest earlier hit of its pattern), protocol, confirmed, mode,
    first_m."""
    names, pairs, count, seen, first, modes, last = {}, {}, {}, {}, {}, {}, {}
    for j, m, C, _E, pre, post in sorted(hits):
        proto, pos, neg, _, N, G, _, _ = pats[j]
        if proto == "flex":
            mode = flex_mode(*flex_words(pre, post, C < 0))
            if mode is None:
                continue
            modes[mode] = modes.get(mode, 0) + 1
        name = pos if C > 0 else neg
        names[name] = names.get(name, 0) + 1
        count[proto] = count.get(proto, 0) + 1
        if N >= 20:
            seen[proto] = seen.get(proto, 0) + 1
        first.setdefault(proto, m)
        first[proto] = min(first[proto], m)
        if j in last and on_grid(m - last[j], G, pl):
            pairs[proto] = pairs.get(proto, 0) + 1
        last[j] = m
    order = [p for p in PROTOCOLS if any(q[0] == p for q in pats)]
    protocol, confirmed = None, False
    for table, flag in ((pairs, True), (seen, False)):
        best = max([table.get(p, 0) for p in order] or [0])
        if best >= 1:
            protocol, confirmed = [p for p in order if table.get(p, 0) == best][0], flag
            break
    mode = None
    if protocol == "flex":
        known = [(modes[name], -i) for i, (_, name) in enumerate(MODES) if name in modes]
        mode = MODES[-max(known)[1]][1] if known else "?"
    return dict(hits=names, pairs=pairs, protocol=protocol, confirmed=confirmed, mode=mode,
                first_m=None if protocol is None else first[protocol])


# ---- crafted planes ------------------------------------------------------------------------------------------------------------


def crafted_plane(n: int, pl: dict, start: int, levels, first: int = 0, amp: int = 1000, base=None) -> np.ndarray:
    """int64[n]: v written straight from symbol levels.  Symbol ``first + k`` of ``levels`` covers the samples
    start + rint(i sps) .. start + rint((i + 1) sps) - 1, clipped to the plane; ``base``: the plane to write into (else zeros)."""
    v = np.zeros(n, dtype=np.int64) if base is None else np.array(base, dtype=np.int64)
    for k, lev in enumerate(levels):
        i = first + k
        a, b = start + int(round(i * pl["sps"])), start + int(round((i + 1) * pl["sps"]))
        v[max(a, 0) : max(min(b, n), 0)] = int(lev) * amp
    return v


def bits_of(word: int, n: int) -> list:
    return [1 if (word >> (n - 1 - i)) & 1 else -1 for i in range(n)]


# ---- the synthesiser and the model capture -------------------------------------------------------------------------------------

FS, SECS, AMP = K.FS, K.SECS, K.AMP
DEV4 = 648.0  # a level of +-1 / +-3 deviates +-648 / +-1944 Hz
DEV_FLEX = 4800.0
FLEX_AT = (64, 3064)  # the bit index of the marker's first bit: two sync-1 sequences 1.875 s apart
DMR_VOICE_SLOT = 20  # the slot of the voice superframe's first burst; the five behind it carry no sync word
# (name, offset Hz, section 23's keying label, the protocol, confirmed, the FLEX mode)
CHANNELS = (
    ("dmr", -900e3, "fsk 4800", "dmr", True, None), ("p25", -700e3, "fsk 4800", "p25", True, None),
    ("ysf", -500e3, "fsk 4800", "ysf", True, None), ("nxdn", -300e3, "fsk 4800", "nxdn", True, None),
    ("flex", 200e3, "fsk 1600", "flex", True, "3200/4"), ("rand4", 400e3, "fsk 4800", None, False, None),
    ("voice", 600e3, "unkeyed", None, False, None))
NAMES = tuple(c[0] for c in CHANNELS)


def _random_levels(seed: int, count: int) -> np.ndarray:
    return 2 * np.random.default_rng(seed).integers(0, 4, count) - 3


def stream_symbols(name: str, seed: int) -> np.ndarray:
    """The symbol levels of a 4800 symbols/s stream over SECS: random dibits with the protocol's sync words on their grid."""
    count = int(math.ceil(SECS * 4800.0)) + 1
    lev = _random_levels(seed, count)
    by = {p[1]: p for p in PATTERNS}
    if name == "dmr":  # a base station: a burst every 144 symbols, the sync word 60 symbols into it
        word = np.array(symbols(by["dmr bs voice"]))
        for slot in range(count // 144):
            at = slot * 144 + 60
            if at + 24 > count or DMR_VOICE_SLOT < slot <= DMR_VOICE_SLOT + 5:
                continue
            lev[at : at + 24] = word if slot == DMR_VOICE_SLOT else -word
    elif name == "p25":  # a frame sync every 864 symbols (a logical data unit)
        for at in range(0, count - 24, 864):
            lev[at : at + 24] = symbols(by["p25"])
    elif name == "ysf":  # a frame of 480 symbols
        for at in range(0, count - 20, 480):
            lev[at : at + 20] = symbols(by["ysf"])
    elif name == "nxdn":  # a frame of 192 symbols
        for at in range(0, count - 10, 192):
            lev[at : at + 10] = symbols(by["nxdn"])
    else:
        raise ValueError(name)
    return lev


def flex_bits(seed: int, code: int = 0xDEA0) -> np.ndarray:
    """+-1 at 1600 bit/s over SECS: random bits, and at each of FLEX_AT 32 alternating bits, the code, the marker and the negated
    code (every word MSB first)."""
    count = int(math.ceil(SECS * 1600.0)) + 1
    bits = 2 * np.random.default_rng(seed).integers(0, 2, count) - 1
    by = {p[1]: p for p in PATTERNS}
    for at in FLEX_AT:
        bits[at - 48 : at - 16] = bits_of(0xAAAAAAAA, 32)
        bits[at - 16 : at] = bits_of(code, 16)
        bits[at : at + 32] = symbols(by["flex"])
        bits[at + 32 : at + 48] = bits_of(code ^ 0xFFFF, 16)
    return bits


def fsk_levels(levels, baud: float, dev: float, n: int) -> np.ndarray:
    """Rectangular symbols: level l deviates l dev Hz."""
    return K._fm_of(K._symbols(np.asarray(levels, dtype=np.float64) * dev, baud, n))


@functools.lru_cache(maxsize=1)
def capture() -> np.ndarray:
    """int16[n][2]: the model capture in ``keying_model``'s conventions (s16, 2.4 MS/s, 2 s, AMP 0.05, complex noise 30 dB under
    AMP in total, seed 11, DC 0.01)."""
    n = int(round(FS * SECS))
    t = np.arange(n) / FS
    rng = np.random.default_rng(11)
    sigma = AMP * 10.0 ** (-30.0 / 20.0) / math.sqrt(2.0)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    off = {c[0]: c[1] for c in CHANNELS}
    car = lambda name: np.exp(2j * np.pi * ((off[name] * t) % 1.0))  # noqa: E731
    a = AMP / 2.0
    for seed, name in ((31, "dmr"), (32, "p25"), (33, "ysf"), (34, "nxdn")):
        x += a * car(name) * fsk_levels(stream_symbols(name, seed), 4800.0, DEV4, n)
    x += a * car("flex") * fsk_levels(flex_bits(35), 1600.0, DEV_FLEX, n)
    x += a * car("rand4") * fsk_levels(_random_levels(25, int(math.ceil(SECS * 4800.0)) + 1), 4800.0, DEV4, n)
    x += a * car("voice") * K._fm_of(2500.0 * M.voice(1, n))
    x += 0.01
    out = np.empty((n, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real * 32768.0), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag * 32768.0), -32768, 32767)
    out.setflags(write=False)
    return out


def identify_stream(theta, c, keyed_from, label, baud, fs_ch: float) -> dict:
    """The identification of one channel from its whole theta, its centre and section 23's label: ``kept`` the sorted hit list,
    ``hits`` the counts per name."""
    out = dict(rate=None, plan=None, v=None, score=None, kept=None, hits={}, pairs={}, protocol=None, confirmed=False, mode=None,
               first_m=None, note="")
    if label is None or baud not in FAMILY:
        return out
    out["rate"] = FAMILY[baud]
    try:
        pl = plan(fs_ch, out["rate"])
    except ValueError:
        out["note"] = "rate does not fit"
        return out
    pats = family(out["rate"])
    v = integrate(np.asarray(theta)[keyed_from:], c, pl["L"], pl["sh"])
    planes, hits = search(v, pl, pats)
    out.update(plan=pl, v=v, score=planes, kept=hits, **decide(hits, pats, pl))
    return out


@functools.lru_cache(maxsize=1)
def model_run() -> dict:
    """The whole oracle on the model capture, once per session: the numpy finder, the float64 channelizer, the describe sums
    and labels, the keying, and the identification of every channel."""
    raw = capture()
    p = FM.plan(FS, raw.shape[0])
    st = FM.run(FM.rows(raw, p), p)
    found = FM.result(p, st["runs"], st["on"], st["mean"], None)
    x = FM.to_complex(raw)
    zs = {}

    def streams(j, dp):
        zs[j] = M.channelize(x, FS, dp["offset_hz"], dp["taps"], dp["D"]).astype(np.complex64)
        return zs[j]

    described = M.describe_run(p, st, found, streams, None, min(raw.shape[0], K.BLOCK_FRAMES))
    keyed, named = [], []
    for j, d in enumerate(described):
        theta = K.quadrature(zs[j])
        k = K.key_stream(zs[j], theta, d["sh"], d["gate"], d["plan"], M.find_args(p), K.calls_of(raw.shape[0], d["plan"]["D"]))
        k["label"], k["baud"] = K.rule(k["coh"], k["rate_hz"], k["crossings"], k["plan"]) if d["label"] == "nfm" else (None, None)
        keyed.append(k)
        named.append(identify_stream(theta, k["c"], k["keyed_from"], k["label"], k["baud"], d["plan"]["fs_ch"]))
    return dict(p=p, st=st, found=found, described=described, keyed=keyed, named=named)
