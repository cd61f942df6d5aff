"""CTCSS tones and DTMF digits beside narrowband FM: the signalling of voice channels.

Per block ``iqa_tones_decimate`` quantises the discriminator output and decimates it by R = floor(fs / 8000) with a
triangular window into the run's stored ``u`` (int32 at fd = fs / R, 8 to 16 kHz).  Once per run ``iqa_tones_bank`` runs
the two banks of tone correlators over it (50 CTCSS tones over 0.4 s frames, 8 DTMF tones over 20 ms frames; exact int64
sums) and ``iqa_tones_decide`` turns every frame's energies into one byte.  Bridging single-frame gaps, forming events
and digit sequences is integer host logic on the two byte planes and runs on plain numpy arrays as well
(``parse_tones``)."""
from __future__ import annotations

from ctypes import c_int32, c_int64
from dataclasses import asdict, dataclass, field

import numpy as np

from .. import _dev as D
from .. import _native as N
from .. import dsp_plan as P
from .common import SideStage, StreamCore

NONE = P.TONES_NONE
MIN_RUN = 3  # frames of one code that make an event
SEQUENCE_GAP_S = 2.0  # a digit starting later than this after the one before opens a new sequence


@dataclass
class CtcssEvent:
    tone_hz: float
    start_s: float
    end_s: float
    frames: int

    def line(self) -> str:
        return f"CTCSS {self.tone_hz:.1f} Hz {self.start_s:.2f}-{self.end_s:.2f} s"


@dataclass
class DtmfEvent:
    key: str
    start_s: float
    end_s: float
    frames: int


@dataclass
class DtmfSequence:
    time_s: float  # the start of its first digit
    digits: str

    def line(self) -> str:
        return f"DTMF {self.digits} at {self.time_s:.2f} s"


@dataclass
class TonesResult:
    ctcss: list = field(default_factory=list)  # CtcssEvent, in order of time
    dtmf: list = field(default_factory=list)  # DtmfEvent, in order of time
    sequences: list = field(default_factory=list)  # DtmfSequence

    def to_json(self) -> dict:
        return asdict(self)

    def lines(self) -> list:
        return [e.line() for e in self.ctcss] + [s.line() for s in self.sequences]


def bridge(codes) -> np.ndarray:
    """A frame without a code whose two neighbours carry the same code takes it.  One pass that reads the original plane."""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1)
    out = codes.copy()
    if codes.size >= 3:
        mid = (codes[1:-1] == NONE) & (codes[:-2] == codes[2:]) & (codes[:-2] != NONE)
        out[1:-1][mid] = codes[:-2][mid]
    return out


def runs(codes) -> list:
    """[(code, first frame, last frame)] of the maximal runs of one code != 255 that are at least MIN_RUN frames long."""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1)
    if codes.size == 0:
        return []
    edges = np.flatnonzero(codes[1:] != codes[:-1]) + 1
    first = np.concatenate([[0], edges])
    last = np.concatenate([edges, [codes.size]]) - 1
    return [(int(codes[a]), int(a), int(b)) for a, b in zip(first, last) if codes[a] != NONE and b - a + 1 >= MIN_RUN]


def parse_tones(plan: P.TonesPlan, ctcss_codes, dtmf_codes) -> TonesResult | None:
    """The two byte planes (one code per frame, 255 = none) -> the run's events.  Integer logic only (the times are one
    float64 product and one division each); ``None`` where there is no event."""
    res = TonesResult()
    for code, i0, i1 in runs(bridge(ctcss_codes)):
        res.ctcss.append(CtcssEvent(tone_hz=P.CTCSS_TONES[code], start_s=i0 * plan.Hc * plan.R / plan.fs,
                                    end_s=(i1 * plan.Hc + plan.Nc) * plan.R / plan.fs, frames=i1 - i0 + 1))
    for code, i0, i1 in runs(bridge(dtmf_codes)):
        res.dtmf.append(DtmfEvent(key=P.DTMF_KEYS[code], start_s=i0 * plan.Hd * plan.R / plan.fs,
                                  end_s=(i1 * plan.Hd + plan.Nd) * plan.R / plan.fs, frames=i1 - i0 + 1))
    last_end = None
    for ev in res.dtmf:
        if last_end is None or ev.start_s - last_end > SEQUENCE_GAP_S:
            res.sequences.append(DtmfSequence(time_s=ev.start_s, digits=""))
        res.sequences[-1].digits += ev.key
        last_end = ev.end_s
    return res if (res.ctcss or res.dtmf) else None


class TonesCore(StreamCore):
    """Per-stream device state (``StreamCore``): the carried quantised history (2R - 2 values), the absolute position, and
    the growing store of ``u`` (one int32 device tensor per block, joined by ``finish``).  ``keep_stages`` also stores t, for
    the tests."""

    def __init__(self, plan: P.TonesPlan, *, keep_stages: bool = False):
        super().__init__(plan, 2 * plan.R - 2, dict(u="int32", t=None))
        self._ctcss_taps = D.from_numpy(np.ascontiguousarray(plan.ctcss_taps))
        self._dtmf_taps = D.from_numpy(np.ascontiguousarray(plan.dtmf_taps))
        self.keep_stages = keep_stages

    def _block(self, theta, n: int):
        """One block of the discriminator output (device float32[n], radians per sample)."""
        R = self.plan.R
        t, u = D.empty(n, "int32"), D.empty((self.pos + n) // R - self.pos // R, "int32")
        N.call("iqa_tones_decimate", N.ptr(theta), c_int64(n), c_int64(self.pos), N.ptr(self._hist), c_int32(R), N.ptr(t),
               N.ptr(u) if u.numel() else N.ptr(None), N.stream_ptr())
        if u.numel():
            self.store.append("u", u)
        if self.keep_stages:
            self.store.append("t", t)
        return t

    def joined(self) -> dict:
        return dict(u=self.store.joined("u"), t=self.store.joined("t"))

    def finish(self) -> dict:
        """The banks and the decisions over the stored run, as device tensors: ``E_ctcss`` int64[Fc * 50], ``E_dtmf``
        int64[Fd * 8], ``P`` int64[Fd], ``ctcss`` uint8[Fc], ``dtmf`` uint8[Fd]; and ``m``, ``Fc``, ``Fd``."""
        plan = self.plan
        u = self.joined()["u"]
        m = int(u.numel())
        Fc, Fd = plan.frames(plan.Nc, plan.Hc, m), plan.frames(plan.Nd, plan.Hd, m)
        Ec, Ed, Pw = D.empty(Fc * len(P.CTCSS_TONES), "int64"), D.empty(Fd * len(P.DTMF_TONES), "int64"), D.empty(Fd, "int64")
        ctcss, dtmf = D.empty(Fc, "uint8"), D.empty(Fd, "uint8")
        if Fc:
            N.call("iqa_tones_bank", N.ptr(u), c_int64(m), c_int32(plan.Nc), c_int32(plan.Hc), c_int32(len(P.CTCSS_TONES)),
                   N.ptr(self._ctcss_taps), N.ptr(Ec), N.ptr(None), N.stream_ptr())
        if Fd:
            N.call("iqa_tones_bank", N.ptr(u), c_int64(m), c_int32(plan.Nd), c_int32(plan.Hd), c_int32(len(P.DTMF_TONES)),
                   N.ptr(self._dtmf_taps), N.ptr(Ed), N.ptr(Pw), N.stream_ptr())
        if Fc or Fd:
            N.call("iqa_tones_decide", N.ptr(Ec) if Fc else N.ptr(None), c_int64(Fc), N.ptr(Ed) if Fd else N.ptr(None),
                   N.ptr(Pw) if Fd else N.ptr(None), c_int64(Fd), c_int32(plan.Nd), N.ptr(ctcss) if Fc else N.ptr(None),
                   N.ptr(dtmf) if Fd else N.ptr(None), N.stream_ptr())
        return dict(E_ctcss=Ec, E_dtmf=Ed, P=Pw, ctcss=ctcss, dtmf=dtmf, m=m, Fc=Fc, Fd=Fd)

    def result(self, fin=None, **context) -> TonesResult | None:
        """The run's ``TonesResult`` (``None`` without an event); ``fin``: a ``finish()`` made earlier."""
        fin = self.finish() if fin is None else fin
        return parse_tones(self.plan, fin["ctcss"].cpu().numpy(), fin["dtmf"].cpu().numpy())


class ToneDecoder(SideStage):
    """The stage API: ``process(block)`` per block of the channel (complex: the channelizer's output, run through
    ``iqa_quadrature`` with this decoder's own ``prev``; or float32: a discriminator output in radians per sample,
    |theta| <= pi), ``finish()`` once (a ``TonesResult``, or ``None`` without an event), ``stages()`` for the tests."""

    def __init__(self, rate: float, *, keep_stages: bool = True):
        super().__init__(TonesCore(P.plan_tones(float(rate)), keep_stages=keep_stages), keep=keep_stages)

    def stages(self) -> dict:
        """Host copies: ``theta`` and ``t`` (with keep_stages), ``u``, ``E_ctcss`` int64[Fc, 50], ``E_dtmf`` int64[Fd, 8],
        ``P`` int64[Fd], ``ctcss`` and ``dtmf`` (uint8, one code per frame)."""
        fin = self._finished()
        st = self.core.joined()
        return dict(theta=self._inputs_host(), t=None if st["t"] is None else st["t"].cpu().numpy(), u=st["u"].cpu().numpy(),
                    E_ctcss=fin["E_ctcss"].cpu().numpy().reshape(fin["Fc"], len(P.CTCSS_TONES)),
                    E_dtmf=fin["E_dtmf"].cpu().numpy().reshape(fin["Fd"], len(P.DTMF_TONES)), P=fin["P"].cpu().numpy(),
                    ctcss=fin["ctcss"].cpu().numpy(), dtmf=fin["dtmf"].cpu().numpy())
