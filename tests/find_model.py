"""Numpy oracle of the channel finder (--find-channels): one function per stage, written from the
specification and from nothing in the package.  Everything behind ``quantise`` is integer, so the kernels are held to these
functions bit for bit.  Also the model capture of the tests and a numpy-FFT row maker that restates ``spectrum._PsdEngine``
(its last bits differ from rocFFT's, so the GPU tests start from the GPU's own rows)."""
from __future__ import annotations

import math

import numpy as np

C_MIN, C_MAX = -30000, 30000
RECORD = ("lo", "hi", "hot", "peak", "e_peak", "sum_w", "sum_wk", "peak_over")

# ---- the plan ------------------------------------------------------------------------------------------------------------


def plan(fs, n, *, nfft=None, threshold_db=6.0, peak_threshold_db=10.0, floor_hz=1e6, gap_hz=5000.0, dc_guard_hz=1000.0,
         max_slices=256, min_hot=2) -> dict:
    if nfft is None:
        if n < 256:
            raise ValueError("not one frame")
        nfft = 256
        while fs / nfft > 500.0 and nfft < 1 << 18:
            nfft *= 2
        while nfft > 256 and (n - nfft) // (nfft // 2) + 1 < 8:
            nfft //= 2
    if n < nfft:
        raise ValueError("not one frame")
    hop = nfft // 2
    F = (n - nfft) // hop + 1
    T = (F + max_slices - 1) // max_slices
    if T > 65536:
        raise ValueError("slices too long")
    w = np.hanning(nfft)
    bin_hz = fs / nfft
    thr = int(np.rint(100.0 * threshold_db))
    return dict(fs=float(fs), n=int(n), nfft=nfft, hop=hop, F=F, T=T, S=(F + T - 1) // T, bin_hz=bin_hz, dc_bin=nfft // 2,
                scale=nfft * fs * float(np.sum(w ** 2) / nfft) + 1e-18, h=min(int(floor_hz / 2 / bin_hz), 8191), num=1, den=4,
                thr=thr, thr_peak=int(np.rint(100.0 * peak_threshold_db)), thr_act=thr // 2, gap=min(int(gap_hz / bin_hz), 255),
                dc_guard=int(dc_guard_hz / bin_hz) if dc_guard_hz >= 0 else -1, min_hot=min_hot)


# ---- the capture and its rows --------------------------------------------------------------------------------------------

AMP = 0.05
TRUTH = (  # (offset Hz, what) in ascending offset
    (-500e3, "burst"), (-200e3, "weak"), (300e3, "nfm"), (800e3, "wfm"))
BURST = (0.5, 0.7)


def _fm(t, offset, tone, index, amp):
    return amp * np.exp(1j * (2 * np.pi * offset * t + index * np.sin(2 * np.pi * tone * t)))


def capture(fs=2.4e6, secs=2.0, seed=3, carriers=True) -> np.ndarray:
    """int16[n][2]: the model capture (NFM at +300 kHz, a 20 dB weaker one at -200 kHz, a burst at -500 kHz keyed 0.5 .. 0.7 s
    with 2 ms raised-cosine ramps, wide FM at +800 kHz, a DC offset of 0.01, complex noise 30 dB under a carrier in total)."""
    n = int(round(fs * secs))
    t = np.arange(n) / fs
    rng = np.random.default_rng(seed)
    sigma = AMP * 10.0 ** (-30.0 / 20.0) / math.sqrt(2.0)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if carriers:
        x += _fm(t, 300e3, 1000.0, 3.0, AMP)
        x += _fm(t, -200e3, 700.0, 2.5, AMP / 10.0)
        ramp = 2e-3
        key = np.clip((t - BURST[0]) / ramp, 0.0, 1.0) * np.clip((BURST[1] - t) / ramp, 0.0, 1.0)
        x += _fm(t, -500e3, 400.0, 3.0, AMP) * (0.5 - 0.5 * np.cos(np.pi * key))
        x += _fm(t, 800e3, 5000.0, 15.0, AMP)
    x += 0.01
    out = np.empty((n, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real * 32768.0), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag * 32768.0), -32768, 32767)
    return out


def encode(raw_s16: np.ndarray, fmt: str) -> np.ndarray:
    """The int16 capture in another capture format: u8 (rint(x / 256) + 128, offset binary) or f32 (x / 32768)."""
    if fmt == "s16":
        return raw_s16
    if fmt == "u8":
        return np.clip(np.rint(raw_s16 / 256.0) + 128.0, 0, 255).astype(np.uint8)
    if fmt == "f32":
        return (raw_s16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
    raise ValueError(fmt)


def to_complex(raw: np.ndarray, iq_order="iq") -> np.ndarray:
    """The frames as the spectrum kernels read them: float32 components, widened to complex128."""
    raw = raw.reshape(-1, 2)
    if raw.dtype == np.int16:
        a = raw.astype(np.float32) * np.float32(1.0 / 32768.0)
    elif raw.dtype == np.uint8:
        a = (raw.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 128.0)
    else:
        a = raw.astype(np.float32)
    i, q = (a[:, 1], a[:, 0]) if iq_order in ("qi", "qi_inv") else (a[:, 0], a[:, 1])
    if iq_order.endswith("_inv"):
        q = -q
    return i.astype(np.float64) + 1j * q.astype(np.float64)


def rows(raw: np.ndarray, p: dict, iq_order="iq", batch=64) -> np.ndarray:
    """float32[F][nfft]: Hann window, float64 FFT, 10 log10(|X|^2 / scale + 1e-18), fftshift-ed, frame f at f hop."""
    z = to_complex(raw, iq_order)
    nfft, hop, F = p["nfft"], p["hop"], p["F"]
    w = np.hanning(nfft).astype(np.float64)
    out = np.empty((F, nfft), dtype=np.float32)
    inv = 1.0 / p["scale"]
    for f0 in range(0, F, batch):
        f1 = min(F, f0 + batch)
        idx = (np.arange(f0, f1) * hop)[:, None] + np.arange(nfft)[None, :]
        X = np.fft.fft(z[idx] * w, axis=1)
        db = 10.0 * np.log10(np.abs((X.real ** 2 + X.imag ** 2) * inv) + 1e-18)
        out[f0:f1] = np.fft.fftshift(db, axes=1).astype(np.float32)
    return out


# ---- the stages ----------------------------------------------------------------------------------------------------------


def quantise(row: np.ndarray) -> np.ndarray:
    """c = clamp(rint(100.0f row), -30000, 30000): one float32 product, half-even; NaN reads as -30000."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.rint(np.float32(100.0) * np.asarray(row, dtype=np.float32)).astype(np.float64)
    x = np.where(np.isnan(x), float(C_MIN), x)
    return np.clip(x, C_MIN, C_MAX).astype(np.int16)


def new_state(nbins: int, S: int) -> dict:
    return dict(sum=np.zeros(nbins, dtype=np.int64), max=np.full(nbins, C_MIN, dtype=np.int32),
                slice=np.zeros((S, nbins), dtype=np.int32))


def accumulate(state: dict, c: np.ndarray, first_frame: int, T: int) -> dict:
    """Add the frames ``c`` (int[n][nbins], the first one frame ``first_frame`` of the run) into sum, max and the slices."""
    c = np.asarray(c).reshape(-1, state["sum"].size)
    for f in range(c.shape[0]):
        row = c[f].astype(np.int64)
        state["sum"] += row
        state["max"] = np.maximum(state["max"], row).astype(np.int32)
        state["slice"][(first_frame + f) // T] += row.astype(np.int32)
    return state


def accumulate_all(c: np.ndarray, T: int, S: int) -> dict:
    """``accumulate`` of a whole run at once (the sums are integers: the order does not matter)."""
    c = np.asarray(c)
    F, nbins = c.shape
    st = new_state(nbins, S)
    st["sum"] = c.sum(axis=0, dtype=np.int64)
    st["max"] = np.maximum(c.max(axis=0).astype(np.int32), C_MIN).astype(np.int32)
    for s in range(S):
        st["slice"][s] = c[s * T : min(F, (s + 1) * T)].sum(axis=0, dtype=np.int64).astype(np.int32)
    return st


def mean(total: np.ndarray, F: int) -> np.ndarray:
    return np.floor_divide(np.asarray(total, dtype=np.int64), np.int64(F)).astype(np.int32)


def floor(plane: np.ndarray, h: int, num: int, den: int) -> np.ndarray:
    """floor[k]: the value of rank ((hi - lo) num) // den, 0-based ascending, among plane[lo .. hi], the window clipped."""
    plane = np.asarray(plane, dtype=np.int32)
    n = plane.size
    out = np.empty(n, dtype=np.int32)
    if n > 2 * h + 1:  # the interior: full windows, all of one rank
        r = (2 * h * num) // den
        view = np.lib.stride_tricks.sliding_window_view(plane, 2 * h + 1)
        for a in range(0, view.shape[0], 512):
            part = np.partition(view[a : a + 512], r, axis=1)[:, r]
            out[h + a : h + a + part.size] = part
    for k in range(n):
        if n > 2 * h + 1 and h <= k <= n - 1 - h:
            continue
        lo, hi = max(0, k - h), min(n - 1, k + h)
        r = ((hi - lo) * num) // den
        out[k] = np.partition(plane[lo : hi + 1], r)[r]
    return out


def mask(mean_, fmean, max_, fmax, *, thr, thr_peak, gap, dc_bin, dc_guard):
    """(x int32, mask uint8): bit 0 = hot, bit 1 = closed."""
    m, fm, mx, fx = (np.asarray(a, dtype=np.int64) for a in (mean_, fmean, max_, fmax))
    x = np.maximum(m - fm - thr, mx - fx - thr_peak)
    k = np.arange(x.size)
    hot = (x >= 0) & (np.abs(k - dc_bin) > dc_guard)
    far = x.size + 1000
    left = np.maximum.accumulate(np.where(hot, k, -far))  # the nearest hot bin at or below k
    right = np.minimum.accumulate(np.where(hot, k, 2 * far)[::-1])[::-1]  # at or above k
    closed = hot | ((left >= 0) & (right < x.size) & (right - left - 1 <= gap))
    return x.astype(np.int32), (hot.astype(np.uint8) | (closed.astype(np.uint8) << 1))


def runs(mean_, fmean, max_, fmax, mask_bytes, min_hot):
    """(kept records int64[J][8] ascending in lo, the number of all runs)."""
    m, fm, mx, fx = (np.asarray(a, dtype=np.int64) for a in (mean_, fmean, max_, fmax))
    closed = (np.asarray(mask_bytes) & 2) != 0
    hot = (np.asarray(mask_bytes) & 1) != 0
    out, total, k, n = [], 0, 0, closed.size
    while k < n:
        if not closed[k]:
            k += 1
            continue
        lo = k
        while k + 1 < n and closed[k + 1]:
            k += 1
        hi = k
        k += 1
        total += 1
        e = m[lo : hi + 1] - fm[lo : hi + 1]
        w = np.maximum(e, 0)
        at = int(np.argmax(e))  # the lowest index of the maximum
        rec = (lo, hi, int(hot[lo : hi + 1].sum()), lo + at, int(e[at]), int(w.sum()), int((w * np.arange(hi - lo + 1)).sum()),
               int((mx[lo : hi + 1] - fx[lo : hi + 1]).max()))
        if rec[2] >= min_hot:
            out.append(rec)
    return np.asarray(out, dtype=np.int64).reshape(-1, 8), total


def activity(slices, fmean, records, *, T, F, thr_act) -> np.ndarray:
    """on uint8[J][S]: slice s of run j is on iff sum_k (slice[s][k] - T_s fmean[k]) >= T_s B thr_act."""
    slices = np.asarray(slices, dtype=np.int64)
    fm = np.asarray(fmean, dtype=np.int64)
    S = slices.shape[0]
    on = np.zeros((len(records), S), dtype=np.uint8)
    for j, rec in enumerate(records):
        lo, hi = int(rec[0]), int(rec[1])
        for s in range(S):
            Ts = min(T, F - s * T)
            total = int((slices[s, lo : hi + 1] - Ts * fm[lo : hi + 1]).sum())
            on[j, s] = 1 if total >= Ts * (hi - lo + 1) * thr_act else 0
    return on


def result(p: dict, records, on, mean_, center_freq=None) -> list:
    """One dict per kept run, ascending in offset: the fields of ``FoundChannel``."""
    out = []
    for rec, row in zip(np.asarray(records).tolist(), np.asarray(on)):
        lo, hi, hot, peak, e_peak, sw, swk, over = rec
        centroid = lo + (swk / sw if sw > 0 else (hi - lo) / 2.0)
        offset = (centroid - p["dc_bin"]) * p["bin_hz"]
        lens = [min(p["T"], p["F"] - s * p["T"]) for s in range(p["S"])]
        idx = np.flatnonzero(row)
        first = last = None
        if idx.size:
            first = int(idx[0]) * p["T"] * p["hop"] / p["fs"]
            last = min((int(idx[-1]) + 1) * p["T"], p["F"]) * p["hop"] / p["fs"]
        out.append(dict(offset_hz=offset, freq_hz=None if center_freq is None else center_freq + offset,
                        width_hz=(hi - lo + 1) * p["bin_hz"], snr_db=e_peak / 100.0, peak_db=over / 100.0,
                        level_db=int(mean_[peak]) / 100.0, duty=sum(lens[s] for s in idx.tolist()) / p["F"], first_s=first,
                        last_s=last, bursts=int(np.count_nonzero(np.diff(np.concatenate(([0], row.astype(np.int64)))) == 1)),
                        lo_bin=lo, hi_bin=hi))
    return sorted(out, key=lambda d: d["offset_hz"])


def run(rows_f32: np.ndarray, p: dict) -> dict:
    """Every stage of a whole run from its rows."""
    c = quantise(rows_f32)
    st = accumulate_all(c, p["T"], p["S"])
    m = mean(st["sum"], p["F"])
    fmean, fmax = floor(m, p["h"], p["num"], p["den"]), floor(st["max"], p["h"], p["num"], p["den"])
    x, mk = mask(m, fmean, st["max"], fmax, thr=p["thr"], thr_peak=p["thr_peak"], gap=p["gap"], dc_bin=p["dc_bin"], dc_guard=p["dc_guard"])
    rec, total = runs(m, fmean, st["max"], fmax, mk, p["min_hot"])
    on = activity(st["slice"], fmean, rec, T=p["T"], F=p["F"], thr_act=p["thr_act"])
    return dict(c=c, sum=st["sum"], max=st["max"], slice=st["slice"], mean=m, fmean=fmean, fmax=fmax, x=x, mask=mk, runs=rec,
                candidates=total, on=on)


def check_four_channels(p: dict, res: list) -> None:
    """What both the host and the GPU tests ask of the model capture's result: the three narrow centroids within one bin of
    the truth and the wide one within three, the widths, the burst's duty and times within two slices, the others always on."""
    assert len(res) == 4
    slice_s = p["T"] * p["hop"] / p["fs"]
    widths = ((5e3, 8e3), (6e3, 9e3), (13e3, 17e3), (200e3, 240e3))
    for d, (truth, what), (wlo, whi) in zip(res, TRUTH, widths):
        assert abs(d["offset_hz"] - truth) <= (3 if what == "wfm" else 1) * p["bin_hz"], (what, d["offset_hz"])
        assert wlo <= d["width_hz"] <= whi, (what, d["width_hz"])
        if what == "burst":
            assert abs(d["duty"] - 0.10) <= 2 * p["T"] / p["F"], d["duty"]
            assert abs(d["first_s"] - BURST[0]) <= 2 * slice_s and abs(d["last_s"] - BURST[1]) <= 2 * slice_s, (d["first_s"], d["last_s"])
            assert d["bursts"] == 1
        else:
            assert d["duty"] == 1.0 and d["first_s"] == 0.0 and d["last_s"] == p["F"] * p["hop"] / p["fs"] and d["bursts"] == 1, what
