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


# ---- edge shapes (tests/test_gpu_tones_shapes.py, tests/test_tones_shapes_host.py) ---------------------------------------
#
# Case tables, block oracles with a position and a history, and numpy stand-ins of the three entry points that follow
# csrc/tones.hip's launch arithmetic (tiles, LDS image, guards) and can be broken one way at a time.  The ``check_*``
# functions hold the comparisons; they take the entry point as a callable, so the GPU file passes the device call and the
# host file the stand-in.

SPAN, THREADS, LDS_BYTES = 8192, 256, 64 * 1024  # TN_SPAN, TN_THREADS, the default LDS allowance
T_PI = 12_868  # rint(float32(pi) 4096)
SENT = -7_777_777  # what untouched output words hold
GUARD = 16  # sentinel words behind (and, for views, in front of) every output
SHAPE_R = (1, 2, 31, 32, 33, 63, MAX_R)
MAX_N, MAX_POS = 1 << 40, 1 << 50  # the entry point's own limits
BIG_POS = (1 << 40) + 3
MAX_FRAME, MAX_TONES = 6400, 64
MAX_FRAMES = 1 << 30
HOSTILE_F32 = np.array([np.nan, np.inf, -np.inf, 3.0e38], dtype=np.float32)
HOSTILE_I32 = np.array([2 ** 31 - 1, -(2 ** 31), 2 ** 31 - 1, -(2 ** 31)], dtype=np.int32)
BANK_RATES = (8000.0, 519_999.0, 15_999.0, 96_000.0, 10e6 / 104)  # lowest, highest, the longest frame, both stream rates


def tile_outputs(R: int) -> int:
    return min(SPAN // R, THREADS)


def triangle(R: int) -> np.ndarray:
    j = np.arange(2 * R - 1, dtype=np.int64)
    return np.minimum(j + 1, 2 * R - 1 - j)


def shape_theta(n: int, R: int, seed: int) -> np.ndarray:
    """float32[n] over [-pi, pi]: random, 3R of +pi and 3R of -pi from 5R on (any 3R - 2 samples hold a whole window, so
    a sum reaches +-R^2 12 868 at every alignment), and the twelve half-even ties (k + 1/2) / 4096 in front."""
    rng = np.random.default_rng(seed)
    pi32 = np.float32(np.pi)
    th = np.clip(rng.uniform(-np.pi, np.pi, n).astype(np.float32), -pi32, pi32)
    run = np.concatenate([np.full(3 * R, pi32), np.full(3 * R, -pi32)]).astype(np.float32)
    at = min(5 * R + 12, n)
    th[at : at + run.size] = run[: max(0, n - at)]
    ties = ((np.arange(-6, 6, dtype=np.float64) + 0.5) / 4096.0).astype(np.float32)
    th[: min(n, ties.size)] = ties[: min(n, ties.size)]
    return th


def shape_history(R: int, seed: int) -> np.ndarray:
    h = np.random.default_rng(seed).integers(-T_PI, T_PI + 1, size=2 * R - 2).astype(np.int32)
    if h.size:
        h[0], h[-1] = T_PI, -T_PI
    return h


def decimate_block(t, R: int, pos: int, hist=None):
    """(u int32, sums int64) of the outputs a block at absolute ``pos`` completes, m = pos // R .. (pos + n) // R - 1, from
    the 2R - 2 values in front of it (None: zeros).  A plain window product per output; ``decimate`` is the two-boxcar form."""
    t = np.asarray(t, dtype=np.int64)
    back = 2 * R - 2
    front = np.zeros(back, dtype=np.int64) if hist is None else np.asarray(hist, dtype=np.int64)[:back]
    assert front.size == back
    ext = np.concatenate([front, t])  # ext[e] = t at absolute pos - back + e
    m = range(pos // R, (pos + t.size) // R)  # (python ints: pos may be 2^40 + 3)
    if len(m) == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64)
    first = np.array([int((k - 1) * R + 1 - (pos - back)) for k in m], dtype=np.int64)  # the window of m: absolute (m-1)R+1 .. (m+1)R-1
    assert first.min() >= 0 and first.max() + 2 * R - 1 <= ext.size
    sums = np.lib.stride_tricks.sliding_window_view(ext, 2 * R - 1)[first] @ triangle(R)
    assert np.abs(sums).max() <= R * R * T_PI < 2 ** 31
    return (sums // R).astype(np.int32), sums


def decimate_cases(R: int) -> list:
    """dict(name, n, pos, hist, seed): three tiles and a ragged rest at every kind of position; one sample (a block that
    completes no output, and one that completes one from the history alone); blocks whose last sample is a tile's last and
    the next tile's first (a position that is a multiple of R makes the first sample a tile's first)."""
    span = tile_outputs(R) * R
    out = []
    for k, pos in enumerate((0, 5 * R, 7 * R + R // 2 + (R == 1), 9 * R + R - 1, BIG_POS)):
        lengths = [("three tiles and a rest", 3 * span + R + 1), ("one sample", 1)]
        if k in (0, 2, 4):
            lengths += [("ends on a tile's last sample", 3 * span - pos % R), ("ends on a tile's first sample", 3 * span - pos % R + 1)]
        for what, n in lengths:
            for hist in ((False, True) if R > 1 else (False,)):
                out.append(dict(name=f"R {R} pos {pos} {what} hist {'given' if hist else 'NULL'}", R=R, n=n, pos=pos, hist=hist,
                                seed=1000 * R + 10 * len(out)))
    return out


def tiles_of(case: dict) -> int:
    R, span = case["R"], tile_outputs(case["R"]) * case["R"]
    return -(-(case["pos"] % R + case["n"]) // span)


def decimate_inputs(case: dict):
    """(theta allocation, hist allocation or None): the values the call may read, followed by hostile ones."""
    R = case["R"]
    theta = np.concatenate([shape_theta(case["n"], R, case["seed"]), HOSTILE_F32])
    hist = np.concatenate([shape_history(R, case["seed"] + 1), HOSTILE_I32]) if case["hist"] else None
    return theta, hist


def check_decimate(case: dict, call, stats: dict | None = None) -> None:
    """``call(theta_alloc, n, pos, hist_alloc | None, R, t_buf, u_buf) -> (t_buf, u_buf)`` after the call (int32 numpy);
    the buffers arrive filled with SENT.  The oracle's own facts first, then t, u and the guards."""
    R, n, pos = case["R"], case["n"], case["pos"]
    theta, hist = decimate_inputs(case)
    want_t = quantise(theta[:n])
    want_u, sums = decimate_block(want_t, R, pos, None if hist is None else hist[: 2 * R - 2])
    count = (pos + n) // R - pos // R
    assert want_u.size == count and np.abs(want_t).max() <= T_PI
    if n > 1:
        assert tiles_of(case) == (3 if "last sample" in case["name"] else 4), case["name"]
        assert int(sums.max()) == R * R * T_PI and int(sums.min()) == -R * R * T_PI, case["name"]
        assert list(want_t[:12]) == [-6, -4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6]  # half-even
        if R > 1:
            assert int(((sums < 0) & (sums % R != 0)).sum()) > 0, case["name"]  # so floor and truncation differ
    if stats is not None:
        stats["no output"] = stats.get("no output", 0) + (count == 0)
        stats["from the history alone"] = stats.get("from the history alone", 0) + (count == 1 and n == 1 and R > 1)
        stats["negative, not divisible"] = stats.get("negative, not divisible", 0) + int(((sums < 0) & (sums % R != 0)).sum())
    t_buf = np.full(n + GUARD, SENT, dtype=np.int32)
    u_buf = np.full(count + GUARD, SENT, dtype=np.int32)
    t_buf, u_buf = call(theta, n, pos, hist, R, t_buf, u_buf)
    np.testing.assert_array_equal(t_buf[:n], want_t, err_msg=f"t: {case['name']}")
    np.testing.assert_array_equal(u_buf[:count], want_u, err_msg=f"u: {case['name']}")
    assert (t_buf[n:] == SENT).all() and (u_buf[count:] == SENT).all(), case["name"]


def kernel_decimate(theta, n: int, pos: int, hist, R: int, t_out, u_out, *, floor: bool = True, mb_kernel=None, mb_host=None) -> None:
    """k_tones_decimate and its launch in numpy, tile by tile: the LDS image (poisoned where nothing was staged), the t
    stores of a tile's own span, one output per thread.  Breaks: ``floor=False`` truncates the quotient; ``mb_host`` /
    ``mb_kernel`` replace min(8192 // R, 256) in the launcher (grid, LDS bytes, the MB the kernel is given) / inside the
    kernel alone."""
    mbh = tile_outputs(R) if mb_host is None else mb_host
    mb = mbh if mb_kernel is None else mb_kernel
    halo, back = R - 1, 2 * R - 2
    lds_words = halo + mbh * R
    if 4 * lds_words > LDS_BYTES:
        raise RuntimeError("k_tones_decimate: the launch asks for more LDS than a workgroup may have")
    m_first, m_end, end = pos // R, (pos + n) // R, pos + n
    w = triangle(R)
    for b in range(-(-(end - m_first * R) // (mbh * R))):
        m0 = m_first + b * mb
        S = m0 * R
        count = halo + mb * R
        assert count <= lds_words, "a store behind the LDS allocation"
        x = S - halo + np.arange(count, dtype=np.int64)
        img = np.zeros(count, dtype=np.int64)
        inside = (x >= pos) & (x < end)
        at = (x[inside] - pos).astype(np.int64)
        img[inside] = quantise(np.asarray(theta)[at])
        own = inside & (np.arange(count) >= halo)
        t_out[(x[own] - pos).astype(np.int64)] = img[own]
        if hist is not None and R > 1:
            hm = (x < pos) & (x >= pos - back)
            img[hm] = np.asarray(hist)[(x[hm] - (pos - back)).astype(np.int64)]
        tid = np.arange(THREADS)
        live = (tid < mb) & (m0 + tid < m_end)
        if not live.any():
            continue
        sums = np.lib.stride_tricks.sliding_window_view(img, 2 * R - 1)[tid[live] * R] @ w
        assert np.abs(sums).max() < 2 ** 31
        quot = sums // R if floor else np.where(sums < 0, -((-sums) // R), sums // R)
        u_out[m0 + tid[live] - m_first] = quot


def entry_decimate(theta, n, pos, hist, R, t_out, u_out, **breaks) -> None:
    """iqa_tones_decimate's checks in front of ``kernel_decimate``; None stands for a NULL pointer."""
    if n < 0 or pos < 0:
        raise ValueError("negative length or position")
    if not 1 <= R <= MAX_R:
        raise ValueError("R must be 1 .. IQA_TONES_MAX_R")
    if n == 0:
        return
    if n > MAX_N or pos > MAX_POS:
        raise ValueError("length or position out of range")
    if theta is None or t_out is None or ((pos + n) // R > pos // R and u_out is None):
        raise ValueError("NULL device pointer")
    kernel_decimate(theta, n, pos, hist, R, t_out, u_out, **breaks)


def decimate_refusals() -> list:
    """(what, n, pos, R, theta?, t_out?, u_out?, message): calls iqa_tones_decimate must refuse before it launches."""
    return [("R = 0", 64, 0, 0, True, True, True, "R must be"), ("R above the maximum", 64, 0, MAX_R + 1, True, True, True, "R must be"),
            ("negative n", -1, 0, 2, True, True, True, "negative"), ("negative pos", 64, -1, 2, True, True, True, "negative"),
            ("n above 2^40", MAX_N + 1, 0, 2, True, True, True, "out of range"), ("pos above 2^50", 64, MAX_POS + 1, 2, True, True, True, "out of range"),
            ("NULL theta", 64, 0, 2, False, True, True, "NULL"), ("NULL t_out", 64, 0, 2, True, False, True, "NULL"),
            ("NULL u_out with outputs to write", 64, 0, 2, True, True, False, "NULL")]


# -- block invariance


def shape_stream(fs: float, n: int) -> np.ndarray:
    """float32 theta[n] of a 67.0 Hz tone at 500 Hz deviation and the digits 159D from 0.05 s on, straight from the
    instantaneous deviation (no complex detour): theta = 2 pi dev / fs."""
    k = np.arange(n, dtype=np.float64) / fs
    dev = 500.0 * np.sin(2.0 * np.pi * 67.0 * k) + dtmf_audio(n, fs, "159D", start_s=0.05)
    dev += 300.0 * np.random.default_rng(int(fs)).normal(size=n)
    return (2.0 * np.pi * dev / fs).astype(np.float32)


def invariance_case(R: int):
    """(fs, n, schedules): fs = 8000 R; n one CTCSS frame and three tiles and a bit; cuts one before, on and one behind the
    first tile edge, a 1-sample first block, blocks inside the 2R - 2 history, a block that ends on its own second tile
    edge (tiles are laid from the block's m_first R), 1-sample blocks at the end."""
    fs, span = 8000.0 * R, tile_outputs(R) * R
    n = 3200 * R + 3 * span + R + 7
    a = 1 + (2 * R - 3)
    b = a + 5
    c = b + 2 * span - b % R
    schedules = [[0, n], [0, span - 1, n], [0, span, n], [0, span + 1, n], [0, span - 1, span, span + 1, n],
                 [0, 1, a, b, c, c + 1, c + R - 1, n - 2 * span - 3, n - 1, n]]
    for cuts in schedules:
        assert all(x < y for x, y in zip(cuts[:-1], cuts[1:]))
    return fs, n, schedules


def run_blocks(theta, R: int, cuts, decimate) -> dict:
    """TonesCore's carrying of the history around ``decimate(theta_block, pos, hist | None, R) -> (t, u)``."""
    hist, pos, ts, us = None, 0, [], []
    back = 2 * R - 2
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        t, u = decimate(theta[lo:hi], pos, hist, R)
        ts.append(t)
        us.append(u)
        if back:
            prev = np.zeros(back, dtype=np.int32) if hist is None else hist
            hist = np.concatenate([prev, t])[-back:]
        pos += hi - lo
    return dict(t=np.concatenate(ts), u=np.concatenate(us))


def check_invariance(runs: list, want: dict, keys) -> None:
    """Every run equals the oracle (and so the single-block run, runs[0]), stage by stage."""
    assert want["E_ctcss"].shape[0] >= 1 and want["E_dtmf"].shape[0] >= 40
    assert (want["ctcss"] != NONE).any() and (want["dtmf"] != NONE).any()
    for k, st in enumerate(runs):
        for key in keys:
            assert st[key].shape == want[key].shape, (k, key)
            np.testing.assert_array_equal(st[key], want[key], err_msg=f"{key}, schedule {k}")
            np.testing.assert_array_equal(st[key], runs[0][key], err_msg=f"{key}, schedule {k} against the single block")


# -- the banks


def bank_iq(u, taps, n_frame: int, hop: int):
    """(I, Q) int64[F, tones], one plain dot product per frame and tap row."""
    u = np.asarray(u, dtype=np.int64)
    F = frames_of(n_frame, hop, u.size)
    I = np.zeros((F, taps.shape[0]), dtype=np.int64)
    Q = np.zeros_like(I)
    for i in range(F):
        fr = u[i * hop : i * hop + n_frame]
        I[i] = taps[:, 0, :].astype(np.int64) @ fr
        Q[i] = taps[:, 1, :].astype(np.int64) @ fr
    return I, Q


def bank_cases() -> list:
    """dict(name, N, H, taps int16[ntones, 2, N], power, m, F): both banks of every rate of BANK_RATES; the CTCSS bank (50
    tones) without P and the DTMF bank (8 tones, so 9 jobs over 4 waves) with it; M = (F - 1) H + N and one more."""
    out = []
    for fs in BANK_RATES:
        pl = plan(fs)
        for kind, N, H, taps, power, F in (("ctcss", pl["Nc"], pl["Hc"], pl["ctcss_taps"], False, 3), ("dtmf", pl["Nd"], pl["Hd"], pl["dtmf_taps"], True, 5)):
            for extra in (0, 1):
                out.append(dict(name=f"fs {fs:.1f} {kind} N {N} H {H} M = (F-1)H+N+{extra}", N=N, H=H, taps=taps, power=power, m=(F - 1) * H + N + extra,
                                F=F, seed=int(fs) + N + extra))
    return out


def bank_u(case: dict) -> np.ndarray:
    """int32[m], |u| < 2^20: random, with frame 0 set against tone 0 (u = -2047 (c_0 + s_0)) and frame 1 against the last
    tone, so that I and Q of those are large and negative."""
    rng = np.random.default_rng(case["seed"])
    u = rng.integers(-(2 ** 20) + 1, 2 ** 20, size=case["m"]).astype(np.int64)
    N, H, taps = case["N"], case["H"], case["taps"].astype(np.int64)
    u[:N] = -2047 * (taps[0, 0] + taps[0, 1]) + rng.integers(-3, 4, size=N)
    u[N : H + N] = (-2047 * (taps[-1, 0] + taps[-1, 1]) + rng.integers(-3, 4, size=N))[N - H :]
    assert np.abs(u).max() < 2 ** 20
    return u.astype(np.int32)


def check_bank(case: dict, call) -> None:
    """``call(u_alloc, m, N, H, ntones, taps_alloc, E_buf, P_buf | None) -> (E_buf, P_buf)`` (int64 numpy), buffers
    arriving filled with SENT."""
    N, H, m, F, taps = case["N"], case["H"], case["m"], case["F"], case["taps"]
    ntones = taps.shape[0]
    u = bank_u(case)
    assert frames_of(N, H, m) == F and (m - N) % H == (m != (F - 1) * H + N) and ntones == (8 if case["power"] else 50)
    I, Q = bank_iq(u, taps, N, H)
    for x in (I, Q):
        assert int(((x < 0) & (x % 4096 != 0)).sum()) > 0 and np.abs(x).max() < 2 ** 41, case["name"]
    assert I[0, 0] < -(2 ** 31) and Q[0, 0] < -(2 ** 31)  # beyond int32
    want_e = (I >> 12) ** 2 + (Q >> 12) ** 2
    trunc = lambda x: np.where(x < 0, -((-x) // 4096), x // 4096)  # noqa: E731
    assert (trunc(I) ** 2 + trunc(Q) ** 2 != want_e).any(), case["name"]  # so >> 12 and / 4096 differ
    again_e, again_p = bank(u, taps, N, H)
    np.testing.assert_array_equal(again_e, want_e)
    want_p = np.array([int((u[i * H : i * H + N].astype(np.int64) ** 2).sum()) for i in range(F)], dtype=np.int64)
    np.testing.assert_array_equal(again_p, want_p)
    u_alloc = np.concatenate([u, HOSTILE_I32])
    taps_alloc = np.concatenate([np.ascontiguousarray(taps).reshape(-1), np.full(8, 32767, dtype=np.int16)])
    e_buf = np.full(F * ntones + GUARD, SENT, dtype=np.int64)
    p_buf = np.full(F + GUARD, SENT, dtype=np.int64) if case["power"] else None
    e_buf, p_buf = call(u_alloc, m, N, H, ntones, taps_alloc, e_buf, p_buf)
    np.testing.assert_array_equal(e_buf[: F * ntones].reshape(F, ntones), want_e, err_msg=f"E: {case['name']}")
    assert (e_buf[F * ntones :] == SENT).all(), case["name"]
    if case["power"]:
        np.testing.assert_array_equal(p_buf[:F], want_p, err_msg=f"P: {case['name']}")
        assert (p_buf[F:] == SENT).all(), case["name"]


def entry_bank(u, m, N, H, ntones, taps, e_out, p_out, *, shift: bool = True) -> None:
    """iqa_tones_bank's checks and k_tones_bank in numpy (``shift=False``: / 4096 truncating in place of >> 12)."""
    if m < 0:
        raise ValueError("negative length")
    if not 1 <= N <= MAX_FRAME:
        raise ValueError("frame must be 1 .. IQA_TONES_MAX_FRAME")
    if not 1 <= H <= N:
        raise ValueError("hop must be 1 .. frame")
    if not 1 <= ntones <= MAX_TONES:
        raise ValueError("ntones must be 1 .. IQA_TONES_MAX_TONES")
    if m < N:
        return
    if u is None or taps is None or e_out is None:
        raise ValueError("NULL device pointer")
    F = (m - N) // H + 1
    if F > MAX_FRAMES:
        raise ValueError("length out of range")
    tp = np.asarray(taps)[: ntones * 2 * N].reshape(ntones, 2, N)
    I, Q = bank_iq(np.asarray(u)[: (F - 1) * H + N], tp, N, H)
    cut = (lambda x: x >> 12) if shift else (lambda x: np.where(x < 0, -((-x) // 4096), x // 4096))
    e_out[: F * ntones] = (cut(I) ** 2 + cut(Q) ** 2).reshape(-1)
    if p_out is not None:
        for i in range(F):
            p_out[i] = int((np.asarray(u)[i * H : i * H + N].astype(np.int64) ** 2).sum())


def bank_refusals() -> list:
    """(what, m, N, H, ntones, u?, taps?, E?, message)."""
    return [("negative m", -1, 160, 80, 8, True, True, True, "negative"), ("frame 0", 400, 0, 1, 8, True, True, True, "frame must be"),
            ("frame above the maximum", 7000, MAX_FRAME + 1, 80, 8, True, True, True, "frame must be"), ("hop 0", 400, 160, 0, 8, True, True, True, "hop must be"),
            ("hop above the frame", 400, 160, 161, 8, True, True, True, "hop must be"), ("no tone", 400, 160, 80, 0, True, True, True, "ntones must be"),
            ("tones above the maximum", 400, 160, 80, MAX_TONES + 1, True, True, True, "ntones must be"), ("NULL u", 400, 160, 80, 8, False, True, True, "NULL"),
            ("NULL taps", 400, 160, 80, 8, True, False, True, "NULL"), ("NULL E", 400, 160, 80, 8, True, True, False, "NULL"),
            ("frames above 2^30", MAX_FRAMES + 1, 1, 1, 8, True, True, True, "out of range")]


def entry_decide_checks(frames_ctcss, frames_dtmf, frame_dtmf, ec, ed, p, out_c, out_d) -> None:
    """iqa_tones_decide's checks alone (the decisions are ``decide_ctcss`` / ``decide_dtmf``)."""
    if frames_ctcss < 0 or frames_dtmf < 0:
        raise ValueError("negative length")
    if not 1 <= frame_dtmf <= MAX_FRAME:
        raise ValueError("frame must be 1 .. IQA_TONES_MAX_FRAME")
    if frames_ctcss > MAX_FRAMES or frames_dtmf > MAX_FRAMES:
        raise ValueError("length out of range")
    if frames_ctcss > 0 and (ec is None or out_c is None):
        raise ValueError("NULL device pointer")
    if frames_dtmf > 0 and (ed is None or p is None or out_d is None):
        raise ValueError("NULL device pointer")


def decide_refusals() -> list:
    """(what, frames_ctcss, frames_dtmf, frame_dtmf, Ec?, Ed?, P?, out_c?, out_d?, message)."""
    yes = (True,) * 5
    return [("negative CTCSS frames", -1, 2, 160) + yes + ("negative",), ("negative DTMF frames", 2, -1, 160) + yes + ("negative",),
            ("frame 0", 2, 2, 0) + yes + ("frame must be",), ("frame above the maximum", 2, 2, MAX_FRAME + 1) + yes + ("frame must be",),
            ("CTCSS frames above 2^30", MAX_FRAMES + 1, 2, 160) + yes + ("out of range",), ("DTMF frames above 2^30", 2, MAX_FRAMES + 1, 160) + yes + ("out of range",),
            ("NULL Ec", 2, 2, 160, False, True, True, True, True, "NULL"), ("NULL Ed", 2, 2, 160, True, False, True, True, True, "NULL"),
            ("NULL P", 2, 2, 160, True, True, False, True, True, "NULL"), ("NULL CTCSS codes", 2, 2, 160, True, True, True, False, True, "NULL"),
            ("NULL DTMF codes", 2, 2, 160, True, True, True, True, False, "NULL")]
