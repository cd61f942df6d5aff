"""CTCSS / DTMF model for the tests (a helper module, not a test file): a plain numpy oracle of DESIGN.md section 14 (plan,
quantiser, triangular decimator, tone banks, per-frame decisions, bridge / events / sequences) and an FM synthesiser of a
voice channel (carrier, sub-audible tone, band-limited gaussian "voice", DTMF bursts, carrier offset, noise).  The tone
tables and thresholds are written out here on their own, not imported from the package, so that the model checks it."""
from __future__ import annotations

import math

import numpy as np

RATE = 8000.0
MAX_R = 64
THETA_SCALE = 4096.0
TAP_SCALE = 256.0
NONE = 255
CTCSS = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0, 127.3,
         131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5, 186.2, 189.9, 192.8,
         196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1)
DTMF = (697.0, 770.0, 852.0, 941.0, 1209.0, 1336.0, 1477.0, 1633.0)
KEYS = "123A456B789C*0#D"
FLOOR = 1 << 16
MIN_RUN = 3
SEQUENCE_GAP_S = 2.0


# ---- plan --------------------------------------------------------------------------------------------------------------


def taps_of(tones, n: int, fd: float) -> np.ndarray:
    """int16[len(tones), 2, n]: rint(256 cos), rint(256 sin) of 2 pi f k / fd."""
    k = np.arange(n, dtype=np.float64)
    out = np.zeros((len(tones), 2, n), dtype=np.int16)
    for i, f in enumerate(tones):
        out[i, 0] = np.rint(TAP_SCALE * np.cos(2.0 * np.pi * f * k / fd))
        out[i, 1] = np.rint(TAP_SCALE * np.sin(2.0 * np.pi * f * k / fd))
    return out


def plan(fs: float) -> dict:
    fs = float(fs)
    R = int(math.floor(fs / RATE))
    if not 1 <= R <= MAX_R:
        raise ValueError(f"R = {R}")
    fd = fs / R
    Hd, Hc = int(np.rint(0.01 * fd)), int(np.rint(0.2 * fd))
    return dict(fs=fs, R=R, fd=fd, Hd=Hd, Nd=2 * Hd, Hc=Hc, Nc=2 * Hc, ctcss_taps=taps_of(CTCSS, 2 * Hc, fd), dtmf_taps=taps_of(DTMF, 2 * Hd, fd))


# ---- stages ------------------------------------------------------------------------------------------------------------


def theta_of(z) -> np.ndarray:
    """The discriminator in float32, as numpy forms it (complex64 product, float32 angle), z[-1] = 1."""
    z = np.asarray(z, dtype=np.complex64)
    prev = np.concatenate([np.ones(1, dtype=np.complex64), z[:-1]])
    return np.angle(z * np.conj(prev)).astype(np.float32)


def quantise(theta) -> np.ndarray:
    return np.rint(np.asarray(theta, dtype=np.float32).astype(np.float64) * THETA_SCALE).astype(np.int32)


def decimate(t, R: int) -> np.ndarray:
    """u[m] = floor(sum_j w[j] t[(m+1)R - 1 - j] / R), w the triangle of length 2R - 1: two running sums of R, exactly."""
    t = np.asarray(t, dtype=np.int64)
    M = t.size // R
    if M == 0:
        return np.zeros(0, dtype=np.int32)
    c = np.concatenate([np.zeros(R, dtype=np.int64), np.cumsum(t)])
    box = c[R:] - c[:-R]  # box[n] = t[n-R+1] + .. + t[n]
    c2 = np.concatenate([np.zeros(R, dtype=np.int64), np.cumsum(box)])
    tri = c2[R:] - c2[:-R]  # tri[n] = box[n-R+1] + .. + box[n]
    u = tri[R - 1 :: R][:M] // R  # numpy's // floors
    assert np.abs(u).max(initial=0) < 2 ** 20
    return u.astype(np.int32)


def frames_of(n_frame: int, hop: int, m: int) -> int:
    return 0 if m < n_frame else (m - n_frame) // hop + 1


def bank(u, taps, n_frame: int, hop: int):
    """(E int64[F, tones], P int64[F]): exact int64 correlations of every frame with every tap row."""
    u = np.asarray(u, dtype=np.int64)
    F = frames_of(n_frame, hop, u.size)
    ntones = taps.shape[0]
    if F == 0:
        return np.zeros((0, ntones), dtype=np.int64), np.zeros(0, dtype=np.int64)
    fr = np.lib.stride_tricks.sliding_window_view(u, n_frame)[::hop][:F]  # [F, n_frame]
    flat = taps.reshape(2 * ntones, n_frame).astype(np.int64)
    assert float(np.abs(fr).max()) * 256.0 * n_frame < 2.0 ** 62
    iq = fr @ flat.T  # int64 matmul: exact
    I, Q = iq[:, 0::2], iq[:, 1::2]
    E = (I >> 12) ** 2 + (Q >> 12) ** 2
    return E, np.sum(fr * fr, axis=1)


def decide_ctcss(E) -> np.ndarray:
    E = np.asarray(E, dtype=np.int64).reshape(-1, len(CTCSS))
    out = np.full(E.shape[0], NONE, dtype=np.uint8)
    for i, row in enumerate(E.tolist()):  # python ints: no overflow to think about
        best = max(row)
        k = row.index(best)
        med = sorted(row)[24]
        if (best >> 6) >= med and best >= FLOOR:
            out[i] = k
    return out


def decide_dtmf(E, P, Nd: int) -> np.ndarray:
    E = np.asarray(E, dtype=np.int64).reshape(-1, len(DTMF))
    out = np.full(E.shape[0], NONE, dtype=np.uint8)
    for i, (row, p) in enumerate(zip(E.tolist(), np.asarray(P).reshape(-1).tolist())):
        rows, cols = row[:4], row[4:]
        er, ec = max(rows), max(cols)
        r, c = rows.index(er), cols.index(ec)
        r2 = max(v for k, v in enumerate(rows) if k != r)
        c2 = max(v for k, v in enumerate(cols) if k != c)
        if (er >= 8 * r2 and ec >= 8 * c2 and ec <= 16 * er and er <= 16 * ec and er >= FLOOR and ec >= FLOOR
                and 1024 * (er + ec) >= Nd * p):
            out[i] = 4 * r + c
    return out


# ---- host logic --------------------------------------------------------------------------------------------------------


def bridge(codes) -> list:
    codes = [int(c) for c in codes]
    out = list(codes)
    for i in range(1, len(codes) - 1):
        if codes[i] == NONE and codes[i - 1] == codes[i + 1] != NONE:
            out[i] = codes[i - 1]
    return out


def runs(codes) -> list:
    out, i = [], 0
    while i < len(codes):
        j = i
        while j + 1 < len(codes) and codes[j + 1] == codes[i]:
            j += 1
        if codes[i] != NONE and j - i + 1 >= MIN_RUN:
            out.append((codes[i], i, j))
        i = j + 1
    return out


def parse(pl: dict, ctcss_codes, dtmf_codes):
    """dict(ctcss=[...], dtmf=[...], sequences=[...]) of plain dicts, or None where both event lists are empty."""
    R, fs = pl["R"], pl["fs"]
    ctcss = [dict(tone_hz=CTCSS[k], start_s=i0 * pl["Hc"] * R / fs, end_s=(i1 * pl["Hc"] + pl["Nc"]) * R / fs, frames=i1 - i0 + 1)
             for k, i0, i1 in runs(bridge(ctcss_codes))]
    dtmf = [dict(key=KEYS[k], start_s=i0 * pl["Hd"] * R / fs, end_s=(i1 * pl["Hd"] + pl["Nd"]) * R / fs, frames=i1 - i0 + 1)
            for k, i0, i1 in runs(bridge(dtmf_codes))]
    seqs, last_end = [], None
    for ev in dtmf:
        if last_end is None or ev["start_s"] - last_end > SEQUENCE_GAP_S:
            seqs.append(dict(time_s=ev["start_s"], digits=""))
        seqs[-1]["digits"] += ev["key"]
        last_end = ev["end_s"]
    if not ctcss and not dtmf:
        return None
    return dict(ctcss=ctcss, dtmf=dtmf, sequences=seqs)


def oracle(theta=None, fs: float = 96_000.0, t=None) -> dict:
    """Every stage from the discriminator output (or from a given t)."""
    pl = plan(fs)
    t = quantise(theta) if t is None else np.asarray(t, dtype=np.int32)
    u = decimate(t, pl["R"])
    Ec, _ = bank(u, pl["ctcss_taps"], pl["Nc"], pl["Hc"])
    Ed, Pd = bank(u, pl["dtmf_taps"], pl["Nd"], pl["Hd"])
    cc, dc = decide_ctcss(Ec), decide_dtmf(Ed, Pd, pl["Nd"])
    return dict(plan=pl, t=t, u=u, E_ctcss=Ec, E_dtmf=Ed, P=Pd, ctcss=cc, dtmf=dc, result=parse(pl, cc, dc))


def median_ratios(E) -> np.ndarray:
    """Winner over median of every CTCSS frame (float, for printing)."""
    E = np.asarray(E, dtype=np.float64).reshape(-1, len(CTCSS))
    return E.max(axis=1) / np.maximum(np.sort(E, axis=1)[:, 24], 1.0)


# ---- synthesiser -------------------------------------------------------------------------------------------------------


def voice(n: int, fs: float, rms_hz: float, seed: int) -> np.ndarray:
    """Gaussian noise band-limited to 300 - 3000 Hz (a brick wall in the frequency domain), scaled to ``rms_hz``."""
    if rms_hz <= 0.0 or n == 0:
        return np.zeros(n)
    rng = np.random.default_rng(seed)
    spec = np.fft.rfft(rng.normal(size=n))
    f = np.fft.rfftfreq(n, 1.0 / fs)
    spec[(f < 300.0) | (f > 3000.0)] = 0.0
    v = np.fft.irfft(spec, n)
    return v * (rms_hz / np.sqrt(np.mean(v * v)))


def dtmf_audio(n: int, fs: float, digits: str, *, start_s: float, on_s: float = 0.05, off_s: float = 0.05, row_dev: float = 1000.0,
               col_gain: float = 1.0) -> np.ndarray:
    """The instantaneous deviation (Hz) of DTMF bursts: digit i sounds from start_s + i (on_s + off_s) for on_s; its row
    tone peaks at ``row_dev``, its column tone at ``col_gain`` times that."""
    out = np.zeros(n)
    for i, key in enumerate(digits):
        r, c = divmod(KEYS.index(key), 4)
        a = int(round((start_s + i * (on_s + off_s)) * fs))
        b = min(a + int(round(on_s * fs)), n)
        k = np.arange(b - a, dtype=np.float64) / fs
        out[a:b] += row_dev * np.sin(2.0 * np.pi * DTMF[r] * k) + col_gain * row_dev * np.sin(2.0 * np.pi * DTMF[4 + c] * k)
    return out


def synth(fs: float, secs: float, *, ctcss_hz: float | None = None, ctcss_dev: float = 500.0, voice_rms: float = 0.0, digits: str = "",
          dtmf_start_s: float = 0.5, row_dev: float = 1000.0, col_gain: float = 1.0, offset_hz: float = 0.0, sigma: float = 0.0,
          carrier: float = 1.0, seed: int = 0) -> np.ndarray:
    """complex64 at ``fs``: a carrier of amplitude ``carrier`` (0: none) frequency-modulated by the sum of the parts, plus
    complex gaussian noise of ``sigma`` per component."""
    n = int(round(fs * secs))
    k = np.arange(n, dtype=np.float64) / fs
    dev = np.full(n, float(offset_hz))
    if ctcss_hz is not None:
        dev += ctcss_dev * np.sin(2.0 * np.pi * ctcss_hz * k)
    dev += voice(n, fs, voice_rms, seed + 1000)
    if digits:
        dev += dtmf_audio(n, fs, digits, start_s=dtmf_start_s, row_dev=row_dev, col_gain=col_gain)
    x = carrier * np.exp(2j * np.pi * np.cumsum(dev) / fs)
    if sigma > 0.0:
        rng = np.random.default_rng(seed)
        x = x + sigma * (rng.normal(size=n) + 1j * rng.normal(size=n))
    return x.astype(np.complex64)
