"""RDS beside wideband FM: PI, PS and RadioText of a station whose pilot the stereo matrix holds.

The 57 kHz subcarrier is the pilot's third harmonic and the bit clock is the pilot divided by 16, so there is neither a
carrier loop nor a timing loop: per block ``iqa_rds_baseband`` (matched filter at ~19 kHz, pilot phase steps) and
``iqa_rds_clock`` (the exact integer prefix sum of the steps); once per run ``iqa_rds_timing`` (the symbol-clock line),
``iqa_rds_symbols`` (interpolated symbols, differential bits) and ``iqa_rds_syndromes``.  The group parser is host logic on
the words and syndromes and runs on plain numpy arrays as well (``parse_groups``)."""
from __future__ import annotations

import math
from collections import Counter
from ctypes import c_double, c_float, c_int32, c_int64
from dataclasses import asdict, dataclass, field

import numpy as np

from .. import _dev as D
from .. import _native as N
from .. import dsp_plan as P
from .common import carried_history

OFFSET_WORDS = {"A": 0x0FC, "B": 0x198, "C": 0x168, "C'": 0x350, "D": 0x1B4}
CRC_POLY = 0x5B9  # x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1


@dataclass
class RdsResult:
    pi: int | None = None  # programme identification (block A of the accepted groups; the most frequent value)
    pty: int | None = None
    tp: bool | None = None
    ps: str | None = None  # programme service name; None until all four segments were seen
    radiotext: str | None = None
    groups: int = 0  # accepted groups
    groups_by_type: dict = field(default_factory=dict)  # "0A", "2A", ... -> count
    bits: int = 0
    timing: dict | None = None  # tau (symbols) and the strength of the symbol-clock line |Z| / sum |y|^2
    group_offsets: list = field(default_factory=list)  # bit offsets of the accepted groups

    def to_json(self) -> dict:
        return asdict(self)

    def line(self) -> str:
        pi = "----" if self.pi is None else f"{self.pi:04X}"
        return f'PI={pi} PS="{self.ps or ""}" RT="{self.radiotext or ""}" groups={self.groups}'


def _char(b: int) -> str:
    return chr(b) if 0x20 <= b <= 0x7E else "�"


def parse_groups(W, S) -> RdsResult:
    """Words ``W[i]`` (26 bits from bit offset i, first bit most significant) and syndromes ``S[i]`` -> the station's data.
    A group is accepted at i iff S[i] = A, S[i+26] = B, S[i+52] in {C, C'}, S[i+78] = D; no error correction."""
    W = np.asarray(W, dtype=np.int64).reshape(-1)
    S = np.asarray(S, dtype=np.int64).reshape(-1)
    res = RdsResult(bits=int(W.size + 25) if W.size else 0)
    if W.size < 79:
        return res
    m = W.size - 78
    ok = ((S[:m] == OFFSET_WORDS["A"]) & (S[26 : m + 26] == OFFSET_WORDS["B"])
          & ((S[52 : m + 52] == OFFSET_WORDS["C"]) | (S[52 : m + 52] == OFFSET_WORDS["C'"])) & (S[78 : m + 78] == OFFSET_WORDS["D"]))
    starts = np.nonzero(ok)[0]
    pis: Counter = Counter()
    types: Counter = Counter()
    ps = [None] * 8
    rt: dict = {}
    rt_flag = None
    rt_end = None
    for i in starts.tolist():
        a, b, c, d = (int(W[i + 26 * q]) >> 10 for q in range(4))
        pis[a] += 1
        gtype, version = b >> 12, (b >> 11) & 1
        types[f"{gtype}{'AB'[version]}"] += 1
        res.tp, res.pty = bool((b >> 10) & 1), (b >> 5) & 0x1F
        if gtype == 0:
            seg = b & 3
            ps[2 * seg], ps[2 * seg + 1] = _char(d >> 8), _char(d & 0xFF)
        elif gtype == 2:
            flag, seg = (b >> 4) & 1, b & 0xF
            if rt_flag is not None and flag != rt_flag:
                rt, rt_end = {}, None
            rt_flag = flag
            raw = [c >> 8, c & 0xFF, d >> 8, d & 0xFF] if version == 0 else [d >> 8, d & 0xFF]
            for q, byte in enumerate(raw):
                at = len(raw) * seg + q
                if byte == 0x0D:
                    rt_end = at if rt_end is None else min(rt_end, at)
                rt[at] = _char(byte)
    res.groups = int(starts.size)
    res.group_offsets = starts.tolist()
    res.groups_by_type = dict(sorted(types.items()))
    if pis:
        res.pi = pis.most_common(1)[0][0]
    if all(ch is not None for ch in ps):
        res.ps = "".join(ps)
    if rt:
        end = rt_end if rt_end is not None else max(rt) + 1
        res.radiotext = "".join(rt.get(at, " ") for at in range(end)).rstrip(" ")
    return res


class RdsCore:
    """Per-stream device state of the RDS demodulator: the carried discriminator history, the absolute position, the
    clock total, and the growing store of y, q, Phi, psi (one device tensor per block, joined by ``finish``)."""

    def __init__(self, plan: P.RdsPlan):
        self.plan = plan
        self.pilot_dev = D.from_numpy(plan.pilot_packed)
        self.mf_dev = D.from_numpy(plan.mf_packed)
        self.hist_len = plan.hist_len
        assert self.hist_len == int(N.lib().iqa_rds_hist_len(plan.wfm.ntaps, plan.half))
        self._hist = None  # device float32[hist_len]; None = zeros
        self.pos = 0  # absolute index of the next block's first sample
        self.total = D.zeros(1, "int64")
        self._store: list = []  # (y, q, phi, psi) per block

    def process(self, theta) -> None:
        """One block of the discriminator output (device float32[n], radians per sample)."""
        n = int(theta.numel())
        if n == 0:
            return
        pl = self.plan
        nj = int(N.lib().iqa_rds_outputs(self.pos, n, pl.decim))
        if nj:
            y, q = D.empty(nj, "complex64"), D.empty(nj, "int64")
            phi, psi = D.empty(nj, "int64"), D.empty(nj, "float64")
            N.call("iqa_rds_baseband", c_int32(pl.wfm.ntaps), N.ptr(self.pilot_dev), c_int32(pl.half), N.ptr(self.mf_dev),
                   c_int32(pl.decim), c_float(pl.wfm.m_scale), c_double(pl.f_mix), c_double(pl.clock_step), N.ptr(theta), c_int64(n),
                   c_int64(self.pos), N.ptr(self._hist), N.ptr(y), N.ptr(q), N.stream_ptr())
            work = D.empty(int(N.lib().iqa_rds_clock_chunks(nj)), "int64")
            N.call("iqa_rds_clock", N.ptr(q), c_int64(nj), c_int64(-(-self.pos // pl.decim)), c_double(pl.clock_step),
                   N.ptr(self.total), N.ptr(work), N.ptr(phi), N.ptr(psi), N.stream_ptr())
            self._store.append((y, q, phi, psi))
        self._hist = carried_history(self._hist, theta, self.hist_len, "float32")
        self.pos += n

    def joined(self) -> dict:
        torch = D.torch_mod()
        if not self._store:
            return dict(y=D.empty(0, "complex64"), q=D.empty(0, "int64"), phi=D.empty(0, "int64"), psi=D.empty(0, "float64"))
        if len(self._store) > 1:
            self._store = [tuple(torch.cat(col) for col in zip(*self._store))]
        y, q, phi, psi = self._store[0]
        return dict(y=y, q=q, phi=phi, psi=psi)

    def finish(self) -> dict:
        """Timing, symbols, bits, words and syndromes of the stored run (device tensors; ``tau``, ``strength`` floats)."""
        st = self.joined()
        y, psi = st["y"], st["psi"]
        n, j0 = int(y.numel()), self.plan.j0
        out = dict(st, tau=0.0, strength=0.0, symbols=D.empty(0, "complex64"), bits=D.empty(0, "uint8"),
                   words=D.empty(0, "int32"), syndromes=D.empty(0, "int16"), k_first=0)
        if n <= j0 + 1:
            return out
        partials = D.empty(3 * int(N.lib().iqa_rds_timing_partials(n)), "float64")
        z = D.empty(3, "float64")
        N.call("iqa_rds_timing", N.ptr(y), N.ptr(psi), c_int64(n), c_int64(j0), N.ptr(partials), N.ptr(z), N.stream_ptr())
        ends = psi[[j0, n - 1]].cpu().numpy()
        zr, zi, pw = (float(v) for v in z.cpu().numpy())
        tau = -math.atan2(zi, zr) / (2.0 * math.pi)
        out["tau"], out["strength"] = tau, (math.hypot(zr, zi) / pw if pw > 0 else 0.0)
        k_first = int(math.floor(float(ends[0]) - tau)) + 1
        nsym = int(math.floor(float(ends[1]) - tau)) - k_first + 1
        out["k_first"] = k_first
        if nsym < 2:
            return out
        sym, bits = D.zeros(nsym, "complex64"), D.empty(nsym - 1, "uint8")
        N.call("iqa_rds_symbols", N.ptr(y), N.ptr(psi), c_int64(n), c_int64(j0), c_double(tau), c_int64(k_first), c_int64(nsym),
               N.ptr(sym), N.ptr(bits), N.stream_ptr())
        out["symbols"], out["bits"] = sym, bits
        if nsym - 1 >= 26:
            words, synd = D.empty(nsym - 26, "int32"), D.empty(nsym - 26, "int16")
            N.call("iqa_rds_syndromes", N.ptr(bits), c_int64(nsym - 1), N.ptr(words), N.ptr(synd), N.stream_ptr())
            out["words"], out["syndromes"] = words, synd
        return out

    def result(self, fin=None, **context) -> RdsResult | None:
        """The station's ``RdsResult`` (``None`` without an accepted group); ``fin``: a ``finish()`` made earlier."""
        res = result_from(self.finish() if fin is None else fin)
        return res if res.groups else None


def result_from(fin: dict) -> RdsResult:
    """``RdsCore.finish()`` -> the parsed result (one copy of the words and syndromes to the host)."""
    W = fin["words"].cpu().numpy().view(np.uint32)
    S = fin["syndromes"].cpu().numpy().view(np.uint16)
    res = parse_groups(W, S)
    res.bits = int(fin["bits"].numel())
    res.timing = dict(tau=fin["tau"], strength=fin["strength"])
    return res


class RdsDecoder:
    """The stage API: ``process(theta_block)`` per block of the discriminator output (radians per sample, as
    ``iqa_quadrature`` writes it: composite x 2 pi 75 000 / rate), ``finish()`` once.  There is no pilot test here: the
    pipeline reports RDS only for a target whose run is stereo; ``finish`` returns ``None`` when no group was accepted."""

    def __init__(self, rate: float):
        self.plan = P.plan_rds(float(rate))
        self.core = RdsCore(self.plan)
        self._fin = None

    def process(self, theta) -> None:
        self.core.process(D.to_device(theta, "float32"))
        self._fin = None

    def _finished(self) -> dict:
        if self._fin is None:
            self._fin = self.core.finish()
        return self._fin

    def finish(self) -> RdsResult | None:
        return self.core.result(self._finished())

    def stages(self) -> dict:
        """Host copies of every stage: y, q, phi, psi, symbols, bits, words, syndromes (and tau, strength, k_first)."""
        fin = self._finished()
        out = {k: (v.cpu().numpy() if D.is_tensor(v) else v) for k, v in fin.items()}
        out["words"], out["syndromes"] = out["words"].view(np.uint32), out["syndromes"].view(np.uint16)
        return out
