"""Numpy oracle of the channel description (--find-describe): one function per step, written from the
specification.  Of the package it uses only ``dsp_plan.choose_decimation`` and ``dsp_plan.design_channel_filter``, which the
specification names.  Everything behind ``quantise`` is integer, so the kernel is held to ``rows`` bit for bit.  Also a plain
float64 channelizer (mix, filter, decimate) and the model capture of the tests: thirteen channels of known modulation."""
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


FM = _load("find_model")
TILE = 2048
Q_MAX = 32767
SUMS = ("N", "NP", "S1", "S2", "E", "CR", "CI", "A")

# ---- the plan and the gate ---------------------------------------------------------------------------------------------------


def plan(fs: float, offset_hz: float, width_hz: float) -> dict:
    from iq_to_audio_amd import dsp_plan as P

    bw = min(max(2.0 * width_hz, 6000.0), fs / 4.0)
    D, fs_ch = P.choose_decimation(fs, max(2.0 * bw, 12000.0))
    taps = P.design_channel_filter(fs, bw, D)
    return dict(fs=float(fs), offset_hz=float(offset_hz), width_hz=float(width_hz), bw=bw, D=int(D), fs_ch=fs_ch, taps=taps,
                delay=(len(taps) - 1) // 2)


def erode(on) -> np.ndarray:
    """g[s] = on[s - 1] & on[s] & on[s + 1], on[-1] = on[S] = 1."""
    on = [1 if v else 0 for v in np.asarray(on).reshape(-1).tolist()]
    S = len(on)
    at = lambda s: 1 if s < 0 or s >= S else on[s]  # noqa: E731
    return np.array([at(s - 1) & at(s) & at(s + 1) for s in range(S)], dtype=np.uint8)


def gate_of(m, g, *, D, delay, hop, T, F) -> np.ndarray:
    """gate(m) for absolute sample indices m (int64): g[min(max(m D - delay, 0) // hop, F - 1) // T]."""
    m = np.asarray(m, dtype=np.int64)
    r = np.maximum(m * np.int64(D) - np.int64(delay), 0)
    f = np.minimum(r // np.int64(hop), np.int64(F - 1))
    return (np.asarray(g, dtype=np.uint8)[f // np.int64(T)] != 0).astype(np.uint8)


# ---- the quantiser -----------------------------------------------------------------------------------------------------------


def choose_shift(z_block) -> int:
    """sh = clamp(10 - ceil(log2(rms)), -30, 30) from the block's mean power (float64); 15 where it is zero."""
    z = np.asarray(z_block, dtype=np.complex64).astype(np.complex128)
    with np.errstate(all="ignore"):
        power = float(np.mean(z.real ** 2 + z.imag ** 2)) if z.size else 0.0
    if not power > 0.0:
        return 15
    if math.isinf(power):
        return -30
    return int(min(max(10 - math.ceil(math.log2(math.sqrt(power))), -30), 30))


def quantise(x, sh: int) -> np.ndarray:
    """clamp(rint(ldexp(x, sh)), -32767, 32767) in float32, half-even; NaN -> 0, +-inf -> +-32767.  int64 out."""
    with np.errstate(all="ignore"):
        v = np.rint(np.ldexp(np.asarray(x, dtype=np.float32), np.int32(sh)).astype(np.float32)).astype(np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(v, -Q_MAX, Q_MAX).astype(np.int64)


def isqrt(v) -> np.ndarray:
    """floor(sqrt(v)) of int64 values in 0 .. 2^62, exactly."""
    v = np.asarray(v, dtype=np.int64)
    r = np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64)
    for _ in range(2):
        r = np.where(r * r > v, r - 1, r)
        r = np.where((r + 1) * (r + 1) <= v, r + 1, r)
    assert ((r * r <= v) & ((r + 1) * (r + 1) > v)).all()
    return r


# ---- the sums ----------------------------------------------------------------------------------------------------------------


def terms(z, pos: int, prev, sh: int, g, *, D, delay, hop, T, F) -> np.ndarray:
    """int64[n][8]: what every sample of the call z (complex64, z[0] sample ``pos`` of the stream) adds to the eight sums;
    ``prev`` is the sample in front (a complex number) or None."""
    z = np.asarray(z, dtype=np.complex64)
    n = z.size
    out = np.zeros((n, 8), dtype=np.int64)
    if n == 0:
        return out
    qi, qq = quantise(z.real, sh), quantise(z.imag, sh)
    m = pos + np.arange(n, dtype=np.int64)
    gm = gate_of(m, g, D=D, delay=delay, hop=hop, T=T, F=F).astype(np.int64)
    p = qi * qi + qq * qq
    assert p.max() < 1 << 31
    out[:, 0] = gm
    out[:, 2] = gm * p
    out[:, 3] = gm * (p >> 8) ** 2
    out[:, 4] = gm * isqrt(p)
    # the pairs: sample k against k - 1
    if prev is None:
        pi = np.concatenate(([0], qi[:-1]))
        pq = np.concatenate(([0], qq[:-1]))
        gp = np.concatenate(([0], gm[:-1]))
    else:
        assert pos >= 1
        pz = np.asarray([prev], dtype=np.complex64)
        pi = np.concatenate((quantise(pz.real, sh), qi[:-1]))
        pq = np.concatenate((quantise(pz.imag, sh), qq[:-1]))
        gp = np.concatenate((gate_of([pos - 1], g, D=D, delay=delay, hop=hop, T=T, F=F).astype(np.int64), gm[:-1]))
    pair = gm * gp
    out[:, 1] = pair
    out[:, 5] = pair * (qi * pi + qq * pq)
    out[:, 6] = pair * (qq * pi - qi * pq)
    out[:, 7] = pair * isqrt(p * (pi * pi + pq * pq))
    return out


def rows(z, pos: int, prev, sh: int, g, **find) -> np.ndarray:
    """int64[ceil(n / 2048)][8]: the rows of one call."""
    t = terms(z, pos, prev, sh, g, **find)
    n_tiles = -(-t.shape[0] // TILE)
    out = np.zeros((n_tiles, 8), dtype=np.int64)
    for k in range(n_tiles):
        out[k] = t[k * TILE : (k + 1) * TILE].sum(axis=0, dtype=np.int64)
    return out


def add_rows(r) -> tuple:
    """The column sums as Python integers."""
    r = np.asarray(r, dtype=np.int64).reshape(-1, 8)
    return tuple(sum(int(v) for v in r[:, k].tolist()) for k in range(8))


def stream_sums(z, sh: int, g, **find) -> tuple:
    """The eight sums of a whole stream from its start."""
    return add_rows(rows(z, 0, None, sh, g, **find))


def sums_by_loops(z, pos, prev, sh, g, *, D, delay, hop, T, F) -> tuple:
    """The same in plain Python, sample by sample (for small streams)."""
    def q(x):
        x = float(np.float32(x))
        if math.isnan(x):
            return 0
        y = float(np.float32(math.ldexp(x, sh))) if math.isfinite(x) else x  # (float32 ldexp of a float32: exact or rounded once)
        if math.isinf(y):
            return Q_MAX if y > 0 else -Q_MAX
        return int(min(max(round(y), -Q_MAX), Q_MAX))  # Python's round: half-even

    def gate(m):
        r = max(m * D - delay, 0)
        return 1 if g[min(r // hop, F - 1) // T] else 0

    tot = [0] * 8
    last = None if prev is None else (q(complex(prev).real), q(complex(prev).imag), gate(pos - 1))
    for k, v in enumerate(np.asarray(z, dtype=np.complex64).tolist()):
        qi, qq, gm = q(v.real), q(v.imag), gate(pos + k)
        p = qi * qi + qq * qq
        if gm:
            tot[0] += 1
            tot[2] += p
            tot[3] += (p >> 8) ** 2
            tot[4] += math.isqrt(p)
            if last is not None and last[2]:
                pi, pq, _ = last
                cr, ci = qi * pi + qq * pq, qq * pi - qi * pq
                assert cr * cr + ci * ci == p * (pi * pi + pq * pq)
                tot[1] += 1
                tot[5] += cr
                tot[6] += ci
                tot[7] += math.isqrt(p * (pi * pi + pq * pq))
        last = (qi, qq, gm)
    return tuple(tot)


# ---- the figures, the label, the suggestion ----------------------------------------------------------------------------------


def figures(sums, fs_ch: float):
    n, _np, s1, s2, e, cr, ci, a = (int(v) for v in sums)
    if s1 == 0 or e == 0 or a == 0:
        return None
    R = math.hypot(cr, ci) / a
    return dict(env=n * s2 * 65536 / s1 ** 2 - 1.0, depth=math.sqrt(max(2.0 * (n * s1 / e ** 2 - 1.0), 0.0)),
                carrier_hz=math.atan2(ci, cr) * fs_ch / (2.0 * math.pi),
                dev_hz=math.sqrt(max(-2.0 * math.log(R), 0.0)) * fs_ch / (2.0 * math.pi))


def plane_figures(p: dict, st: dict, lo: int, hi: int, g, bw: float):
    g = np.asarray(g) != 0
    if not g.any():
        return None
    Ts = np.array([min(p["T"], p["F"] - s * p["T"]) for s in range(p["S"])], dtype=np.int64)
    m_on = st["slice"].astype(np.int64)[g, lo : hi + 1].sum(axis=0) / float(Ts[g].sum())
    lin = 10.0 ** (m_on / 1000.0)
    lin_f = 10.0 ** (st["fmean"][lo : hi + 1].astype(np.float64) / 1000.0)
    at = int(np.argmax(lin))
    line = float(lin[max(at - 1, 0) : at + 2].sum() / lin.sum())
    return dict(line_share=line, cnr_db=10.0 * math.log10(max(float((lin - lin_f).sum()), 1e-30) / (float(lin_f.mean()) * bw / p["bin_hz"])))


def label(N, cnr_db, width_hz, env, dev_hz, line) -> str:
    if N < 1024 or cnr_db < 26:
        return "unknown"
    if width_hz >= 100_000:
        return "wfm" if env < 0.05 else "unknown"
    if env < 0.02:
        return "carrier" if dev_hz < 50 else "nfm"
    if line >= 0.6:
        return "am"
    if width_hz < 6000:
        return "ssb"
    return "unknown"


def suggest(lab, *, offset_hz, carrier_hz, width_hz, freq_hz, lo, hi, dc_bin, bin_hz):
    """(demod, bw, tuned offset) or (None, None, None)."""
    if lab in ("nfm", "carrier"):
        return "nfm", 25000.0 if width_hz > 16000 else 12500.0, offset_hz + carrier_hz
    if lab == "am":
        return "am", 10000.0, offset_hz + carrier_hz
    if lab == "wfm":
        return "wfm", 250000.0, offset_hz + carrier_hz
    if lab == "ssb":
        if freq_hz is None or freq_hz >= 10e6:
            return "usb", 3000.0, (lo - dc_bin) * bin_hz - 300.0
        return "lsb", 3000.0, (hi + 1 - dc_bin) * bin_hz + 300.0
    return None, None, None


def describe(p: dict, st: dict, ch: dict, g, sums, dp: dict, center_freq=None) -> dict:
    """Everything about one channel ``ch`` (a dict of ``find_model.result``) from its sums."""
    out = dict(offset_hz=ch["offset_hz"], width_hz=ch["width_hz"], samples=int(sums[0]), fs_ch=dp["fs_ch"], env=None, depth=None,
               carrier_hz=None, dev_hz=None, line_share=None, cnr_db=None)
    a, b = figures(sums, dp["fs_ch"]), plane_figures(p, st, ch["lo_bin"], ch["hi_bin"], g, dp["bw"])
    lab = "unknown"
    if a is not None and b is not None:
        out.update(a)
        out.update(b)
        lab = label(out["samples"], out["cnr_db"], ch["width_hz"], out["env"], out["dev_hz"], out["line_share"])
    freq = None if center_freq is None else center_freq + ch["offset_hz"]
    demod, bw, tuned = suggest(lab, offset_hz=ch["offset_hz"], carrier_hz=out["carrier_hz"], width_hz=ch["width_hz"], freq_hz=freq,
                               lo=ch["lo_bin"], hi=ch["hi_bin"], dc_bin=p["dc_bin"], bin_hz=p["bin_hz"])
    out.update(label=lab, freq_hz=freq, demod=demod, bw=bw, tuned_offset_hz=tuned,
               tuned_hz=None if tuned is None or center_freq is None else center_freq + tuned)
    return out


# ---- a plain channelizer -----------------------------------------------------------------------------------------------------


def channelize(x: np.ndarray, fs: float, offset_hz: float, taps: np.ndarray, D: int) -> np.ndarray:
    """complex128[ceil(n / D)]: z[m] = sum_k taps[k] y[m D - k], y[i] = x[i] exp(-2 pi j offset i / fs), nothing in front of the
    stream.  Float64.  A long filter against its decimation goes sample by sample in polyphase form, a short one by FFT."""
    x = np.asarray(x, dtype=np.complex128)
    n, L = x.size, len(taps)
    turns = (np.arange(n, dtype=np.float64) * (offset_hz / fs)) % 1.0
    y = x * np.exp(-2j * np.pi * turns)
    n_out = -(-n // D)
    if D >= 16:
        # z[m] = sum_p sum_j taps[j D + p] y[(m - j) D - p]
        z = np.zeros(n_out, dtype=np.complex128)
        for ph in range(D):
            h = taps[ph::D]
            if h.size == 0:
                continue
            # u[m] = y[m D - ph], zero where the index is negative
            first = 1 if ph > 0 else 0  # u[0] lies in front of the stream for ph > 0
            u = np.zeros(n_out, dtype=np.complex128)
            src = y[first * D - ph :: D][: n_out - first]
            u[first : first + src.size] = src
            z += np.convolve(u, h)[:n_out]
        return z
    size = 1 << (n + L - 1).bit_length()
    full = np.fft.ifft(np.fft.fft(y, size) * np.fft.fft(np.asarray(taps, dtype=np.float64), size))[:n]
    return full[::D].copy()


# ---- the model capture -------------------------------------------------------------------------------------------------------

FS, SECS, AMP = 2.4e6, 2.0, FM.AMP
BURST = FM.BURST
CHANNELS = (  # (name, offset Hz, the label the rules give)
    ("nfm_faint", -1050e3, "unknown"), ("carrier", -900e3, "carrier"), ("nfm_voice", -700e3, "nfm"), ("burst", -550e3, "nfm"),
    ("am_weak", -400e3, "am"), ("nfm_weak", -200e3, "nfm"), ("usb", -50e3, "ssb"), ("am_voice", 100e3, "am"),
    ("nfm_tone", 300e3, "nfm"), ("am_tone", 550e3, "am"), ("fsk", 700e3, "nfm"), ("wfm", 950e3, "wfm"), ("am_faint", 1100e3, "am"))
NAMES = tuple(c[0] for c in CHANNELS)
LABELS = {c[0]: c[2] for c in CHANNELS}


def voice(k: int, n: int, analytic: bool = False) -> np.ndarray:
    """Voice v_k at n samples over SECS: white noise of seed k at 48 kHz, 1 / sqrt(f) on 300 .. 2700 Hz, a 3 Hz syllable gate
    max(sin(2 pi 3 t + phi) + 0.3, 0), peak 1, FFT-interpolated; ``analytic``: its analytic signal (the upper sideband)."""
    rate = 48000
    n0 = int(round(rate * SECS))
    rng = np.random.default_rng(k)
    w = rng.standard_normal(n0)
    phi = rng.uniform(0.0, 2.0 * np.pi)
    f = np.fft.rfftfreq(n0, 1.0 / rate)
    shape = np.zeros_like(f)
    band = (f >= 300.0) & (f <= 2700.0)
    shape[band] = 1.0 / np.sqrt(f[band])
    v = np.fft.irfft(np.fft.rfft(w) * shape, n0)
    t = np.arange(n0) / rate
    v = v * np.maximum(np.sin(2.0 * np.pi * 3.0 * t + phi) + 0.3, 0.0)
    v = v / np.max(np.abs(v))
    V = np.fft.fft(v)
    big = np.zeros(n, dtype=np.complex128)
    half = n0 // 2
    big[:half] = V[:half]
    if analytic:
        big[1:half] *= 2.0
        return np.fft.ifft(big) * (n / n0)
    big[n - half + 1 :] = V[n0 - half + 1 :]
    return np.fft.ifft(big).real * (n / n0)


@functools.lru_cache(maxsize=1)
def capture() -> np.ndarray:
    """int16[n][2]: the model capture with ``find_model``'s conventions (AMP 0.05, complex noise 30 dB under AMP in total, seed
    11, DC 0.01)."""
    n = int(round(FS * SECS))
    t = np.arange(n) / FS
    rng = np.random.default_rng(11)
    sigma = AMP * 10.0 ** (-30.0 / 20.0) / math.sqrt(2.0)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    off = {name: o for name, o, _ in CHANNELS}
    car = lambda name: np.exp(2j * np.pi * ((off[name] * t) % 1.0))  # noqa: E731
    fm = lambda name, tone, index, amp: FM._fm(t, off[name], tone, index, amp)  # noqa: E731
    x += fm("nfm_faint", 1000.0, 3.0, AMP / 40.0)
    x += (AMP / 3.0) * car("carrier")
    x += AMP * car("nfm_voice") * np.exp(2j * np.pi * 2500.0 * np.cumsum(voice(1, n)) / FS)
    ramp = 2e-3
    key = np.clip((t - BURST[0]) / ramp, 0.0, 1.0) * np.clip((BURST[1] - t) / ramp, 0.0, 1.0)
    x += fm("burst", 400.0, 3.0, AMP) * (0.5 - 0.5 * np.cos(np.pi * key))
    x += (AMP / 10.0) * (1.0 + 0.8 * voice(3, n)) * car("am_weak")
    x += fm("nfm_weak", 700.0, 2.5, AMP / 10.0)
    x += (AMP / 2.0) * voice(3, n, analytic=True) * car("usb")
    x += (AMP / 2.0) * (1.0 + 0.8 * voice(2, n)) * car("am_voice")
    x += fm("nfm_tone", 1000.0, 3.0, AMP)
    x += (AMP / 2.0) * (1.0 + 0.5 * np.sin(2.0 * np.pi * 1000.0 * t)) * car("am_tone")
    bits = np.random.default_rng(5).integers(0, 2, int(math.ceil(SECS * 1200.0)))
    freq = np.repeat(np.where(bits == 1, 4500.0, -4500.0), int(round(FS / 1200.0)))[:n]
    x += (AMP / 2.0) * car("fsk") * np.exp(2j * np.pi * np.cumsum(freq) / FS)
    x += fm("wfm", 5000.0, 15.0, AMP)
    x += (AMP / 30.0) * (1.0 + 0.5 * np.sin(2.0 * np.pi * 1000.0 * t)) * car("am_faint")
    x += 0.01
    out = np.empty((n, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real * 32768.0), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag * 32768.0), -32768, 32767)
    out.setflags(write=False)
    return out


def find_args(p: dict) -> dict:
    return dict(hop=p["hop"], T=p["T"], F=p["F"])


def describe_run(p: dict, st: dict, found: list, streams, center_freq=None, first_block: int | None = None) -> list:
    """One dict per found channel (``found``: ``find_model.result``): ``streams(j, dp)`` gives channel j's complex64 stream for
    the plan dp; sh comes from the first ``first_block`` raw frames' outputs (None: the whole stream)."""
    recs = {int(r[0]): j for j, r in enumerate(np.asarray(st["runs"]).tolist())}
    out = []
    for j, ch in enumerate(found):
        dp = plan(p["fs"], ch["offset_hz"], ch["width_hz"])
        g = erode(st["on"][recs[ch["lo_bin"]]])
        z = np.asarray(streams(j, dp), dtype=np.complex64)
        head = z if first_block is None else z[: -(-first_block // dp["D"])]
        sh = choose_shift(head)
        sums = stream_sums(z, sh, g, D=dp["D"], delay=dp["delay"], **find_args(p))
        d = describe(p, st, ch, g, sums, dp, center_freq)
        d.update(sums=sums, sh=sh, gate=g, plan=dp)
        out.append(d)
    return out


@functools.lru_cache(maxsize=1)
def model_run() -> dict:
    """The whole oracle on the model capture, once per session: the finder of ``find_model`` on numpy's rows, the float64
    channelizer, the sums, the figures and the labels (no centre frequency)."""
    raw = capture()
    p = FM.plan(FS, raw.shape[0])
    st = FM.run(FM.rows(raw, p), p)
    found = FM.result(p, st["runs"], st["on"], st["mean"], None)
    x = FM.to_complex(raw)
    streams = lambda j, dp: channelize(x, FS, dp["offset_hz"], dp["taps"], dp["D"])  # noqa: E731
    return dict(p=p, st=st, found=found, described=describe_run(p, st, found, streams))
