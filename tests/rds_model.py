"""RDS model for the tests (a helper module, not a test file): the group encoder, the differential encoder, the
shaped-biphase modulator locked to a pilot with a ppm offset, a stereo multiplex builder, and the float64 numpy oracle of
DESIGN.md section 11 (steps 1-6).  The polynomial and the offset words are written out here on their own, not imported
from the package, so that the encoder checks the decoder."""
from __future__ import annotations

import math

import numpy as np

from iq_to_audio_amd import dsp_plan as P

G = 0x5B9  # x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
OFFSETS = {"A": 0x0FC, "B": 0x198, "C": 0x168, "C'": 0x350, "D": 0x1B4}
TD = 1.0 / 1187.5


# ---- encoder -----------------------------------------------------------------------------------------------------------


def crc10(info: int) -> int:
    """(info x^10) mod g, by long division."""
    r = info << 10
    for i in range(25, 9, -1):
        if (r >> i) & 1:
            r ^= G << (i - 10)
    return r & 0x3FF


def block(info: int, offset: str) -> int:
    """A 26-bit block: 16 information bits, then the checkword with the offset word added."""
    return (info << 10) | (crc10(info) ^ OFFSETS[offset])


def syndrome(w: int) -> int:
    return crc10(w >> 10) ^ (w & 0x3FF)


def _b(gtype: int, version: int, tp: int, pty: int, low5: int) -> int:
    return (gtype << 12) | (version << 11) | (tp << 10) | (pty << 5) | (low5 & 0x1F)


def group_0a(pi, seg, ps, *, tp=1, pty=10):
    return [block(pi, "A"), block(_b(0, 0, tp, pty, seg & 3), "B"), block(0xE0CD, "C"),
            block((ord(ps[2 * seg]) << 8) | ord(ps[2 * seg + 1]), "D")]


def group_2a(pi, seg, text, *, flag=0, tp=1, pty=10):
    c = text[4 * seg : 4 * seg + 4]
    return [block(pi, "A"), block(_b(2, 0, tp, pty, (flag << 4) | (seg & 15)), "B"), block((ord(c[0]) << 8) | ord(c[1]), "C"),
            block((ord(c[2]) << 8) | ord(c[3]), "D")]


def group_2b(pi, seg, text, *, flag=0, tp=1, pty=10):
    c = text[2 * seg : 2 * seg + 2]
    return [block(pi, "A"), block(_b(2, 1, tp, pty, (flag << 4) | (seg & 15)), "B"), block(pi, "C'"),
            block((ord(c[0]) << 8) | ord(c[1]), "D")]


def group_4a(pi, *, tp=1, pty=10):
    return [block(pi, "A"), block(_b(4, 0, tp, pty, 1), "B"), block(0xD3A5, "C"), block(0x1234, "D")]


def group_14a(pi, *, tp=1, pty=10):
    return [block(pi, "A"), block(_b(14, 0, tp, pty, 4), "B"), block(0x0BEE, "C"), block(0x54A9, "D")]


PI, PS, RT = 0x54A8, "GFX950FM", "MI355X ON AIR\r  "
RT_SHOWN = "MI355X ON AIR"


def schedule(n_groups: int, pi=PI, ps=PS, rt=RT) -> list:
    """A station's group sequence: 0A and 2A alternate through their four segments, then a 4A and a 14A; period 10."""
    out = []
    for g in range(n_groups):
        r = g % 10
        if r == 8:
            out.append(group_4a(pi))
        elif r == 9:
            out.append(group_14a(pi))
        else:
            out.append(group_0a(pi, r // 2, ps) if r % 2 == 0 else group_2a(pi, r // 2, rt))
    return out


def bits_of(groups: list) -> np.ndarray:
    return np.array([(b >> (25 - i)) & 1 for grp in groups for b in grp for i in range(26)], dtype=np.int64)


def differential(bits: np.ndarray) -> np.ndarray:
    """e[i] = e[i-1] xor bits[i], e[-1] = 0."""
    return np.bitwise_xor.accumulate(np.asarray(bits, dtype=np.int64))


# ---- modulator and multiplex -------------------------------------------------------------------------------------------


def rds_baseband(e: np.ndarray, psi: np.ndarray) -> np.ndarray:
    """Shaped biphase signal at symbol phases ``psi`` (symbol k occupies k <= psi < k + 1): sum_k (2 e[k] - 1) g(psi - k - 1/2)
    with the package's pulse g, peak-normalised."""
    k0 = np.floor(psi).astype(np.int64)
    out = np.zeros(psi.size)
    for dk in range(-4, 5):
        k = k0 + dk
        ok = (k >= 0) & (k < e.size)
        a = np.where(ok, 2 * e[np.clip(k, 0, e.size - 1)] - 1, 0)
        out += a * P.rds_symbol(psi - k - 0.5)
    return out / np.max(np.abs(out))


def multiplex(fs: float, seconds: float, *, ppm: float = 0.0, sigma: float = 0.0, seed: int = 1, rds_level: float = 0.04,
              pilot: float = 0.1, groups: list | None = None, phase: float = 0.7, symbol_phase: float = -0.37):
    """(composite m, transmitted groups): programme L = 0.5 sin 1 kHz, R = 0.5 sin 2.5 kHz at g = 0.9, a pilot ``ppm`` off
    19 kHz, the RDS subcarrier on the pilot's third harmonic with its symbols on the pilot divided by 16, white noise."""
    n = int(round(fs * seconds))
    t = np.arange(n, dtype=np.float64) / fs
    th = 2.0 * math.pi * 19_000.0 * (1.0 + ppm * 1e-6) * t + phase
    lv, rv = 0.5 * np.sin(2 * np.pi * 1000.0 * t), 0.5 * np.sin(2 * np.pi * 2500.0 * t)
    m = 0.45 * (lv + rv) + 0.45 * (lv - rv) * np.sin(2.0 * th) + pilot * np.sin(th)
    psi = th / (2.0 * math.pi * 16.0) + symbol_phase
    if groups is None:
        groups = schedule(int(seconds * 1187.5 / 104) + 2)
    if rds_level:
        m = m + rds_level * rds_baseband(differential(bits_of(groups)), psi) * np.cos(3.0 * th)
    if sigma:
        m = m + sigma * np.random.default_rng(seed).standard_normal(n)
    whole = int(np.floor((psi[-1]) / 104.0))  # groups whose last symbol was sent
    return m, groups[: max(0, min(whole, len(groups)))]


def theta_of(m: np.ndarray, fs: float) -> np.ndarray:
    """The discriminator output that reads as composite ``m``: float32 radians per sample."""
    return (m * (2.0 * math.pi * P.WFM_DEVIATION / fs)).astype(np.float32)


# ---- the float64 oracle ------------------------------------------------------------------------------------------------


def _strided_fir(x: np.ndarray, h: np.ndarray, step: int, chunk: int = 4096, start: int = 0) -> np.ndarray:
    """(h * x)[start::step] of the causal zero-state convolution, by rows of the sliding window."""
    L = h.size
    xp = np.concatenate([np.zeros(L - 1, dtype=x.dtype), x])
    win = np.lib.stride_tricks.sliding_window_view(xp, L)[start::step]  # win[j, i] = x[start + j step - (L-1) + i]
    hr = h[::-1].astype(np.complex128 if np.iscomplexobj(h) or np.iscomplexobj(x) else np.float64)
    out = np.empty(win.shape[0], dtype=hr.dtype)
    for lo in range(0, win.shape[0], chunk):
        out[lo : lo + chunk] = win[lo : lo + chunk] @ hr
    return out


def oracle_baseband(theta: np.ndarray, fs: float, pos: int = 0) -> dict:
    """Steps 2 and 3 up to dev: y, u at the decimated instants, dev, q (float64 from the float32 discriminator values).
    ``pos`` is the absolute index of ``theta[0]``: the stream is ``theta`` with zeros in front of it, the mixer phase comes
    from the absolute index, and the outputs are those at j >= ``j_first`` = ceil(pos / R) (element i is output j_first + i).
    dev of the first output is 0: u in front of it is 0 (the zero prefix), as at the start of a stream."""
    plan = P.plan_rds(fs)
    w = plan.wfm
    n, d, R = theta.size, w.delay, plan.decim
    j_first = -(-int(pos) // R)
    first = j_first * R - int(pos)  # index into theta of the first decimated instant
    m = theta.astype(np.float64) * fs / (2.0 * math.pi * P.WFM_DEVIATION)
    p = _strided_fir(m, w.h_pilot, R, start=first)
    mag = np.abs(p)
    u = np.where(mag < 1e-12, 0.0, p / np.where(mag < 1e-12, 1.0, mag))
    md = np.concatenate([np.zeros(d), m[: n - d]])
    nn = np.arange(n, dtype=np.float64) + float(int(pos))  # absolute indices: exact in float64 below 2^53
    x = md * np.exp(-2j * np.pi * np.mod(plan.f_mix * nn, 1.0))
    y0 = _strided_fir(x, plan.h_matched, R, start=first)
    y = y0 * np.exp(2j * np.pi * np.mod(plan.f_mix * nn[first::R], 1.0)) * np.conj(u) ** 3
    dev = np.zeros(u.size)
    dev[1:] = np.angle(u[1:] * np.conj(u[:-1]) * np.exp(-2j * np.pi * plan.clock_step))
    q = np.rint(dev / (2.0 * np.pi) * 2.0 ** 44).astype(np.int64)
    return dict(plan=plan, y=y, u=u, dev=dev, q=q, j_first=j_first)


def oracle_clock(q: np.ndarray, plan, j_first: int = 0) -> tuple:
    """Phi and psi of the outputs j_first, j_first + 1, ... (Phi starts from 0 at the first of them)."""
    phi = np.cumsum(np.asarray(q, dtype=np.int64))
    j = np.arange(phi.size, dtype=np.float64) + float(int(j_first))
    psi = (j * plan.clock_step + phi.astype(np.float64) * 2.0 ** -44) / 16.0
    return phi, psi


def oracle_symbols(y: np.ndarray, psi: np.ndarray, plan) -> dict:
    """Steps 4 and 5: timing, symbols, bits, words, syndromes."""
    j0 = plan.j0
    e = np.abs(y[j0:]) ** 2
    z = np.sum(e * np.exp(-2j * np.pi * psi[j0:]))
    tau = -np.angle(z) / (2.0 * np.pi)
    r = psi - tau
    fl = np.floor(r)
    j = np.nonzero(fl[1:] > fl[:-1])[0] + 1
    j = j[j > j0]
    k = fl[j]
    s = y[j - 1] + (y[j] - y[j - 1]) * (k - r[j - 1]) / (r[j] - r[j - 1])
    assert np.all(np.diff(k) == 1)
    bits = (np.real(s[1:] * np.conj(s[:-1])) < 0).astype(np.int64)
    words, synd = words_and_syndromes(bits)
    return dict(tau=float(tau), strength=float(abs(z) / np.sum(e)), symbols=s, k_first=int(k[0]) if k.size else 0, bits=bits,
                words=words, syndromes=synd)


def words_and_syndromes(bits: np.ndarray) -> tuple:
    bits = np.asarray(bits, dtype=np.int64)
    if bits.size < 26:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    words = np.zeros(bits.size - 25, dtype=np.int64)
    for i in range(26):
        words |= bits[i : bits.size - 25 + i] << (25 - i)
    r = words & ~0x3FF
    for b in range(25, 9, -1):
        r = np.where((r >> b) & 1 == 1, r ^ (G << (b - 10)), r)
    return words, (r ^ words) & 0x3FF


def oracle_chain(theta: np.ndarray, fs: float) -> dict:
    """The whole chain on the discriminator output ``theta`` at channel rate ``fs`` (group parsing is the package's
    ``parse_groups``: logic on integers, the same code for the oracle's words and the GPU's)."""
    base = oracle_baseband(theta, fs)
    phi, psi = oracle_clock(base["q"], base["plan"])
    out = dict(base, phi=phi, psi=psi)
    out.update(oracle_symbols(base["y"], psi, base["plan"]))
    return out


def align(bits: np.ndarray, sent: np.ndarray, search: int = 400) -> tuple:
    """(offset into ``sent`` at which ``bits`` starts, bit errors there): the best of the first ``search`` offsets."""
    best = (bits.size + 1, 0)
    for o in range(min(search, max(1, sent.size - 200))):
        m = min(bits.size, sent.size - o)
        err = int(np.sum(bits[:m] != sent[o : o + m]))
        best = min(best, (err, o))
    return best[1], best[0]
