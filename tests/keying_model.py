"""Numpy oracle of the keying measurement (--find-decode): one function per step, written from the
specification.  Of the package it uses nothing; the gate, the describe sums and the plain channelizer are ``describe_model``'s.
Everything behind ``quantise`` is integer, so the kernel is held to ``rows`` bit for bit.  Also the model capture of the tests:
thirteen channels of known keying."""
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


M = _load("describe_model")
FM = M.FM
WINDOW = 2048
T_MAX = 32767
BAUDS = (512, 1200, 1600, 2400, 3200, 4800, 9600)
MIN_PAIRS, MIN_CROSSINGS, MIN_COH, RATE_LOW, RATE_HIGH = 1024, 256, 0.35, 0.25, 0.8
BLOCK_FRAMES = 1 << 22  # the raw frames of a block of find_channels

# ---- the plan ----------------------------------------------------------------------------------------------------------------


def plan(fs_ch: float) -> dict:
    """incs (0 where skipped), skipped and the table of a channel rate."""
    skipped = tuple(b >= fs_ch / 4.0 for b in BAUDS)
    incs = tuple(0 if s else int(np.rint(b * 2.0 ** 32 / fs_ch)) for b, s in zip(BAUDS, skipped))
    return dict(fs_ch=float(fs_ch), incs=incs, skipped=skipped, table=table())


def table() -> np.ndarray:
    """int64[1024][2]: rint(1024 cos(2 pi i / 1024)), rint(1024 sin(2 pi i / 1024))."""
    out = np.zeros((1024, 2), dtype=np.int64)
    for i in range(1024):
        out[i] = (round(1024.0 * math.cos(2.0 * math.pi * i / 1024.0)), round(1024.0 * math.sin(2.0 * math.pi * i / 1024.0)))
    return out


# ---- the input ---------------------------------------------------------------------------------------------------------------


def quadrature(z) -> np.ndarray:
    """float32 theta of a whole complex64 stream: the angle of z[m] conj(z[m - 1]) with 1 + 0j in front (float64, rounded once)."""
    z = np.asarray(z, dtype=np.complex64).astype(np.complex128)
    prev = np.concatenate(([1.0 + 0.0j], z[:-1]))
    return np.angle(z * np.conj(prev)).astype(np.float32)


def quantise(theta) -> np.ndarray:
    """clamp(rint(theta 4096), -32767, 32767) in float32, half-even; NaN -> 0.  int64 out."""
    with np.errstate(all="ignore"):
        v = np.rint(np.asarray(theta, dtype=np.float32) * np.float32(4096.0)).astype(np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(v, -T_MAX, T_MAX).astype(np.int64)


def centre(cr: int, ci: int) -> int:
    return int(round(math.atan2(ci, cr) * 4096.0))  # (Python's round: half-even)


def centre_from_rows(describe_rows, calls) -> tuple:
    """(c, the stream position of the first keyed sample) from the describe rows of every call (int64[tiles of every call][8])
    and the calls' lengths: the first call after which NP >= 1024; (None, None) where none is."""
    describe_rows = np.asarray(describe_rows, dtype=np.int64).reshape(-1, 8)
    at = pos = 0
    tot = [0, 0, 0]
    for n in calls:
        k = -(-n // M.TILE)
        part = M.add_rows(describe_rows[at : at + k])
        tot = [tot[0] + part[1], tot[1] + part[5], tot[2] + part[6]]
        if tot[0] >= MIN_PAIRS:
            return centre(tot[1], tot[2]), pos
        at += k
        pos += n
    return None, None


# ---- the rows ----------------------------------------------------------------------------------------------------------------


def windows(pos: int, n: int) -> int:
    return 0 if n <= 0 else (pos + n - 1) // WINDOW - pos // WINDOW + 1


def rows(theta, pos: int, front, c: int, incs, g, *, D, delay, hop, T, F) -> np.ndarray:
    """int64[windows(pos, n)][16] of one call: theta[0] is sample ``pos``, ``front`` the theta in front of it or None."""
    t = quantise(theta)
    n = t.size
    out = np.zeros((windows(pos, n), 16), dtype=np.int64)
    if n == 0:
        return out
    m = pos + np.arange(n, dtype=np.int64)
    gm = M.gate_of(m, g, D=D, delay=delay, hop=hop, T=T, F=F).astype(np.int64)
    s = (t >= c).astype(np.int64)
    if front is None:
        sp, gp = np.concatenate(([0], s[:-1])), np.concatenate(([0], gm[:-1]))
    else:
        assert pos >= 1
        sp = np.concatenate(((quantise([front]) >= c).astype(np.int64), s[:-1]))
        gp = np.concatenate((M.gate_of([pos - 1], g, D=D, delay=delay, hop=hop, T=T, F=F).astype(np.int64), gm[:-1]))
    pair = gm * gp
    cross = pair * (s != sp)
    w = m // WINDOW - pos // WINDOW
    np.add.at(out[:, 0], w, pair)
    np.add.at(out[:, 1], w, cross)
    tab = table()
    at = np.flatnonzero(cross)
    for k, inc in enumerate(incs):
        ph = (m[at].astype(np.uint64) * np.uint64(inc)) & np.uint64(0xFFFFFFFF)  # (the product wraps mod 2^64: its low 32 bits are exact)
        i = (ph >> np.uint64(22)).astype(np.int64)
        np.add.at(out[:, 2 + 2 * k], w[at], tab[i, 0])
        np.add.at(out[:, 3 + 2 * k], w[at], tab[i, 1])
    return out


def rows_by_loops(theta, pos, front, c, incs, g, *, D, delay, hop, T, F) -> dict:
    """The same in plain Python, sample by sample: {window number: [16 sums]} (for small streams)."""
    def q(x):
        x = float(np.float32(x))
        if math.isnan(x):
            return 0
        y = float(np.float32(x) * np.float32(4096.0)) if math.isfinite(x) else x
        if math.isinf(y):
            return T_MAX if y > 0 else -T_MAX
        return int(min(max(round(y), -T_MAX), T_MAX))

    def gate(m):
        r = max(m * D - delay, 0)
        return 1 if g[min(r // hop, F - 1) // T] else 0

    tab = table().tolist()
    out: dict = {}
    last = None if front is None else (q(front) >= c, gate(pos - 1))
    for k, v in enumerate(np.asarray(theta, dtype=np.float32).tolist()):
        m = pos + k
        row = out.setdefault(m // WINDOW, [0] * 16)
        now = (q(v) >= c, gate(m))
        if last is not None and now[1] and last[1]:
            row[0] += 1
            if now[0] != last[0]:
                row[1] += 1
                for j, inc in enumerate(incs):
                    i = ((m * inc) % (1 << 32)) >> 22
                    row[2 + 2 * j] += tab[i][0]
                    row[3 + 2 * j] += tab[i][1]
        last = now
    return out


def add_by_window(parts, n_windows: int) -> np.ndarray:
    """int64[n_windows][16]: the rows of every call ((first window, rows) each) added by window number."""
    out = np.zeros((n_windows, 16), dtype=np.int64)
    for first, r in parts:
        for j, row in enumerate(np.asarray(r, dtype=np.int64).reshape(-1, 16)):
            out[first + j] += row
    return out


def stream_rows(theta, calls, c: int, start: int, incs, g, **find) -> np.ndarray:
    """The window rows of a whole stream cut into ``calls`` (lengths), keyed from position ``start`` (a call's first sample)."""
    theta = np.asarray(theta, dtype=np.float32)
    parts, pos = [], 0
    for n in calls:
        if pos >= start and n > 0:
            front = None if pos == 0 else theta[pos - 1]
            parts.append((pos // WINDOW, rows(theta[pos : pos + n], pos, front, c, incs, g, **find)))
        pos += n
    assert pos == theta.size
    return add_by_window(parts, -(-theta.size // WINDOW))


# ---- the figures, the rule, the decoders -------------------------------------------------------------------------------------


def figures(window_rows, p: dict) -> dict:
    r = [[int(v) for v in row] for row in np.asarray(window_rows, dtype=np.int64).reshape(-1, 16).tolist()]
    pairs, K = sum(x[0] for x in r), sum(x[1] for x in r)
    den = 1024 ** 2 * sum(x[1] ** 2 - x[1] for x in r)
    coh = []
    for k, skip in enumerate(p["skipped"]):
        if skip or den == 0:
            coh.append(None)
        else:
            coh.append((sum(x[2 + 2 * k] ** 2 + x[3 + 2 * k] ** 2 for x in r) - 1024 ** 2 * K) / den)
    return dict(coh=coh, rate_hz=K / pairs * p["fs_ch"] if pairs else None, crossings=K, pairs=pairs)


def rule(coh, rate_hz, crossings, p: dict) -> tuple:
    if crossings < MIN_CROSSINGS or rate_hz is None:
        return "unkeyed", None
    for b, v, skip in zip(BAUDS, coh, p["skipped"]):
        if not skip and v is not None and v >= MIN_COH and RATE_LOW * b <= rate_hz <= RATE_HIGH * b:
            return f"fsk {b}", b
    return "unkeyed", None


def decoders(described: str, baud, tuned_hz) -> list:
    if described == "nfm":
        if baud in (512, 1200, 2400):
            return ["pocsag"]
        if baud == 9600:
            return ["ais"]
        if baud in (1600, 3200, 4800):
            return []
        return ["ax25", "tones"]
    if described == "wfm":
        return ["rds"]
    if described == "am":
        return ["acars"] if tuned_hz is not None and 117.975e6 <= tuned_hz <= 137e6 else []
    return []


# ---- the model capture -------------------------------------------------------------------------------------------------------

FS, SECS, AMP = M.FS, M.SECS, M.AMP
FC_AIR, FC_OUT = 127.0e6, 455.5e6  # centre frequencies that put the AM channel inside and outside the airband
# (name, offset Hz, section 22's label, the keying label, the decoders at FC_AIR).  tone1200, the trap: 2400 crossings a second on
# one clock are thrown out at 2400 by the rate window (rate / B = 1) and taken at 4800 (coherent there too, rate / B = 0.5).
CHANNELS = (
    ("fsk512", -1050e3, "nfm", "fsk 512", ["pocsag"]), ("fsk1200", -950e3, "nfm", "fsk 1200", ["pocsag"]),
    ("fsk2400", -850e3, "nfm", "fsk 2400", ["pocsag"]), ("gmsk9600", -750e3, "nfm", "fsk 9600", ["ais"]),
    ("fsk4_4800", -650e3, "nfm", "fsk 4800", []), ("afsk", -550e3, "nfm", "unkeyed", ["ax25", "tones"]),
    ("voice", -450e3, "nfm", "unkeyed", ["ax25", "tones"]), ("voice_ctcss", -350e3, "nfm", "unkeyed", ["ax25", "tones"]),
    ("tone1200", -250e3, "nfm", "fsk 4800", []), ("fsk_off", -150e3, "nfm", "fsk 1200", ["pocsag"]),
    ("carrier", 100e3, "carrier", None, []), ("am", 250e3, "am", None, ["acars"]), ("wfm", 800e3, "wfm", None, ["rds"]))
NAMES = tuple(c[0] for c in CHANNELS)


def _symbols(values, baud: float, n: int) -> np.ndarray:
    """The symbol under every sample: symbol k covers k / baud <= t < (k + 1) / baud."""
    idx = np.floor(np.arange(n, dtype=np.float64) * (baud / FS) + 1e-9).astype(np.int64)
    return np.asarray(values, dtype=np.float64)[idx]


def _fm_of(freq_hz: np.ndarray) -> np.ndarray:
    return np.exp(2j * np.pi * ((np.cumsum(freq_hz) / FS) % 1.0))


def _fsk2(baud: float, seed: int, n: int, dev: float = 4500.0, off: float = 0.0) -> np.ndarray:
    bits = np.random.default_rng(seed).integers(0, 2, int(math.ceil(SECS * baud)) + 1)
    return _fm_of(_symbols(np.where(bits == 1, dev, -dev), baud, n) + off)


def _gmsk(seed: int, n: int, baud: float = 9600.0, bt: float = 0.4) -> np.ndarray:
    """GMSK, h = 0.5: the +-baud / 4 rectangles through a Gaussian of BT 0.4, formed at a tenth of the rate and held."""
    hold = 10
    sps = FS / hold / baud  # 25
    bits = np.random.default_rng(seed).integers(0, 2, int(math.ceil(SECS * baud)) + 1)
    idx = np.floor(np.arange(n // hold + 1, dtype=np.float64) / sps + 1e-9).astype(np.int64)
    f = np.where(bits[idx] == 1, baud / 4.0, -baud / 4.0)
    sigma = math.sqrt(math.log(2.0)) / (2.0 * math.pi * bt) * sps
    k = np.arange(-int(4 * sigma), int(4 * sigma) + 1, dtype=np.float64)
    h = np.exp(-0.5 * (k / sigma) ** 2)
    f = np.convolve(f, h / h.sum(), mode="same")
    return _fm_of(np.repeat(f, hold)[:n])


def _afsk(seed: int, n: int, dev: float = 3000.0) -> np.ndarray:
    """Bell-202: 1200 baud, a continuous-phase audio tone of 1200 / 2200 Hz, frequency-modulated."""
    bits = np.random.default_rng(seed).integers(0, 2, int(math.ceil(SECS * 1200.0)) + 1)
    tone = _symbols(np.where(bits == 1, 1200.0, 2200.0), 1200.0, n)
    audio = np.sin(2.0 * np.pi * ((np.cumsum(tone) / FS) % 1.0))
    return _fm_of(dev * audio)


@functools.lru_cache(maxsize=1)
def capture() -> np.ndarray:
    """int16[n][2]: the model capture in ``describe_model``'s conventions (AMP 0.05, complex noise 30 dB under AMP in total,
    seed 11, DC 0.01)."""
    n = int(round(FS * SECS))
    t = np.arange(n) / FS
    rng = np.random.default_rng(11)
    sigma = AMP * 10.0 ** (-30.0 / 20.0) / math.sqrt(2.0)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    off = {c[0]: c[1] for c in CHANNELS}
    car = lambda name: np.exp(2j * np.pi * ((off[name] * t) % 1.0))  # noqa: E731
    a = AMP / 2.0
    x += a * car("fsk512") * _fsk2(512.0, 21, n)
    x += a * car("fsk1200") * _fsk2(1200.0, 22, n)
    x += a * car("fsk2400") * _fsk2(2400.0, 23, n)
    x += a * car("gmsk9600") * _gmsk(24, n)
    sym = np.random.default_rng(25).integers(0, 4, int(math.ceil(SECS * 4800.0)) + 1)
    x += a * car("fsk4_4800") * _fm_of(_symbols((2.0 * sym - 3.0) * 648.0, 4800.0, n))
    x += a * car("afsk") * _afsk(26, n)
    x += a * car("voice") * _fm_of(2500.0 * M.voice(1, n))
    x += a * car("voice_ctcss") * _fm_of(2500.0 * M.voice(2, n) + 500.0 * np.sin(2.0 * np.pi * 100.0 * t))
    x += FM._fm(t, off["tone1200"], 1200.0, 3.0, a)
    x += a * car("fsk_off") * _fsk2(1200.0, 27, n, off=0.15 * 4500.0)
    x += (AMP / 3.0) * car("carrier")
    x += a * (1.0 + 0.8 * M.voice(3, n)) * car("am")
    x += FM._fm(t, off["wfm"], 5000.0, 15.0, AMP)
    x += 0.01
    out = np.empty((n, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real * 32768.0), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag * 32768.0), -32768, 32767)
    out.setflags(write=False)
    return out


def calls_of(n_raw: int, D: int) -> list:
    """The channel samples of every block of find_channels: a channelizer's outputs of raw frames a .. b are ceil(b / D) -
    ceil(a / D)."""
    edges = list(range(0, n_raw, BLOCK_FRAMES)) + [n_raw]
    return [-(-b // D) - -(-a // D) for a, b in zip(edges[:-1], edges[1:])]


def key_stream(z, theta, sh: int, g, dp: dict, fp: dict, calls) -> dict:
    """The keying of one channel stream from its complex64 samples (the centre) and its theta (the rows)."""
    kp = plan(dp["fs_ch"])
    find = dict(D=dp["D"], delay=dp["delay"], **fp)
    drows, pos = [], 0
    for n in calls:
        prev = None if pos == 0 else z[pos - 1]
        drows.append(M.rows(z[pos : pos + n], pos, prev, sh, g, **find))
        pos += n
    c, start = centre_from_rows(np.concatenate(drows), calls)
    out = dict(plan=kp, c=c, keyed_from=start, rows=None, coh=[None] * 7, rate_hz=None, crossings=0, pairs=0)
    if c is not None:
        out["rows"] = stream_rows(theta, calls, c, start, kp["incs"], g, **find)
        out.update(figures(out["rows"], kp))
    return out


@functools.lru_cache(maxsize=1)
def model_run() -> dict:
    """The whole oracle on the model capture, once per session: the numpy finder, the float64 channelizer, the describe sums and
    labels, the keying rows, figures and labels."""
    raw = capture()
    p = FM.plan(FS, raw.shape[0])
    st = FM.run(FM.rows(raw, p), p)
    found = FM.result(p, st["runs"], st["on"], st["mean"], None)
    x = FM.to_complex(raw)
    zs = {}

    def streams(j, dp):
        zs[j] = M.channelize(x, FS, dp["offset_hz"], dp["taps"], dp["D"]).astype(np.complex64)
        return zs[j]

    described = M.describe_run(p, st, found, streams, None, min(raw.shape[0], BLOCK_FRAMES))
    keyed = []
    for j, d in enumerate(described):
        k = key_stream(zs[j], quadrature(zs[j]), d["sh"], d["gate"], d["plan"], M.find_args(p), calls_of(raw.shape[0], d["plan"]["D"]))
        k["label"], k["baud"] = rule(k["coh"], k["rate_hz"], k["crossings"], k["plan"]) if d["label"] == "nfm" else (None, None)
        keyed.append(k)
    return dict(p=p, st=st, found=found, described=described, keyed=keyed)
