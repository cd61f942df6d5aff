"""Carrier squelch of a run's targets (``--squelch``).

The gate looks at the channel itself, not at the audio: per block one kernel adds up the power of the target's channel stream
in integer cells of 256 samples (``iqa_gate_power``); at the end of the run the cells become frames, a noise floor (the run's
tenth percentile) and an open / closed state per frame with hysteresis, a minimum duration, hang and lead
(``iqa_gate_decide``), and one kernel multiplies the channel-rate audio by the gate, with ramps (``iqa_gate_apply``).
Everything behind the quantiser is exact integer arithmetic and independent of how the stream is cut into calls.

    gate = CarrierGate(plan_gate(fs_channel, CarrierSquelch()))
    for z in blocks: gate.process(z)          # device complex64
    gate.finish()
    gated = gate.apply(audio)                 # device float32, a buffer of its own
    for line in gate.result(frequency).lines(): print(line)

There is no CPU path: the stages raise ``RuntimeError`` without a GPU or the built library.
"""
from __future__ import annotations

import math
from ctypes import c_int32, c_int64
from dataclasses import dataclass, field

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P

_POWER_SAMPLES = 65536  # of the first block, for sh: what one workgroup of iqa_mean_power adds without atomics


@dataclass(frozen=True)
class CarrierSquelch:
    """The options of ``dsp_plan.plan_gate`` and ``split``: also write one WAV per transmission."""

    frame_ms: float = P.GATE_DEFAULTS["frame_ms"]
    open_db: float = P.GATE_DEFAULTS["open_db"]
    hyst_db: float = P.GATE_DEFAULTS["hyst_db"]
    hang_ms: float = P.GATE_DEFAULTS["hang_ms"]
    min_ms: float = P.GATE_DEFAULTS["min_ms"]
    lead_ms: float = P.GATE_DEFAULTS["lead_ms"]
    ramp_ms: float = P.GATE_DEFAULTS["ramp_ms"]
    split: bool = False


@dataclass(frozen=True)
class Transmission:
    start: int  # first sample of the channel stream
    end: int  # one behind the last
    start_s: float
    end_s: float
    peak_db: float | None  # 10 log10(max v / floor) over the run's frames
    mean_db: float | None  # likewise from the mean of v over the frames with s2 = 1

    def line(self, prefix: str = "") -> str:
        level = "" if self.mean_db is None else f", {self.mean_db:.1f} dB over the floor"
        return f"{prefix}on {self.start_s:.3f} .. {self.end_s:.3f} s ({self.end_s - self.start_s:.3f} s){level}"

    def to_json(self) -> dict:
        return dict(start=self.start, end=self.end, start_s=self.start_s, end_s=self.end_s, peak_db=self.peak_db, mean_db=self.mean_db)

    @classmethod
    def from_json(cls, d: dict) -> "Transmission":
        return cls(start=int(d["start"]), end=int(d["end"]), start_s=float(d["start_s"]), end_s=float(d["end_s"]),
                   peak_db=d.get("peak_db"), mean_db=d.get("mean_db"))


@dataclass(frozen=True)
class GateResult:
    frequency: float | None
    fs: float
    samples: int
    frame: int  # Lf
    sh: int
    floor: int
    floor_dbfs: float
    duty: float
    transmissions: list = field(default_factory=list)

    def lines(self, prefix: str = "") -> list:
        if not self.transmissions:
            return [f"{prefix}squelch never opened"]
        return [t.line(prefix) for t in self.transmissions]

    def to_json(self) -> dict:
        return dict(frequency=self.frequency, fs=self.fs, samples=self.samples, frame=self.frame, sh=self.sh, floor=self.floor,
                    floor_dbfs=self.floor_dbfs, duty=self.duty, transmissions=[t.to_json() for t in self.transmissions])

    @classmethod
    def from_json(cls, d: dict) -> "GateResult":
        return cls(frequency=d.get("frequency"), fs=float(d["fs"]), samples=int(d["samples"]), frame=int(d["frame"]), sh=int(d["sh"]),
                   floor=int(d["floor"]), floor_dbfs=float(d["floor_dbfs"]), duty=float(d["duty"]),
                   transmissions=[Transmission.from_json(t) for t in d.get("transmissions", [])])


def choose_shift(mean_power: float) -> int:
    """sh = clamp(8 - ceil(log2(rms)), -30, 30): the quantiser's scale, an RMS of about 2^8, which leaves 42 dB of headroom
    under 32767; 15 for a silent block."""
    if not (mean_power > 0.0):  # (zero, or not a number)
        return 15
    if math.isinf(mean_power):
        return -P.GATE_MAX_SHIFT
    rms = math.sqrt(mean_power)
    return int(min(max(8 - math.ceil(math.log2(rms)), -P.GATE_MAX_SHIFT), P.GATE_MAX_SHIFT))


def _db(num: int, den: int) -> float | None:
    return 10.0 * math.log10(num / den) if num > 0 and den > 0 else None


def gate_result(plan: P.GatePlan, n: int, sh: int, floor: int, v, s2, g, frequency: float | None = None) -> GateResult:
    """The transmissions of a run from its integers (host, float64): a maximal run [f0, f1] of ones in ``g`` covers the
    samples [f0 Lf, b), b = (f1 + 1) Lf, or n where f1 is the last frame."""
    v, s2, g = np.asarray(v, dtype=np.int64), np.asarray(s2, dtype=np.uint8), np.asarray(g, dtype=np.uint8)
    n, floor, frames = int(n), int(floor), int(g.size)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], g.astype(np.int8), [0]))))
    out, covered = [], 0
    for f0, f1 in zip(edges[0::2], edges[1::2] - 1):
        f0, f1 = int(f0), int(f1)
        start, end = f0 * plan.frame, n if f1 == frames - 1 else (f1 + 1) * plan.frame
        run, kept = v[f0 : f1 + 1], s2[f0 : f1 + 1] != 0
        top, held = int(run.max()), [int(x) for x in run[kept]]
        mean_db = 10.0 * math.log10(sum(held) / len(held) / floor) if held and sum(held) > 0 else None
        out.append(Transmission(start=start, end=end, start_s=start / plan.fs, end_s=end / plan.fs, peak_db=_db(top, floor), mean_db=mean_db))
        covered += end - start
    floor_dbfs = 10.0 * math.log10(floor / 16.0) - 20.0 * sh * math.log10(2.0)
    return GateResult(frequency=frequency, fs=plan.fs, samples=n, frame=plan.frame, sh=int(sh), floor=floor, floor_dbfs=floor_dbfs,
                      duty=covered / n if n else 0.0, transmissions=out)


class CarrierGate:
    """The gate of one channel stream.  ``sh``: the quantiser's shift; None takes it from the first non-empty block
    (``choose_shift`` of ``iqa_mean_power`` over its first 65536 samples: one read-back per run)."""

    def __init__(self, plan: P.GatePlan, sh: int | None = None):
        self.plan = plan
        self._sh0 = sh
        self.reset()

    def reset(self) -> None:
        self.sh = self._sh0
        self.pos = 0
        self._parts: list = []  # (first cell, device int64[cells of the call]) per call
        self.calls: list = []  # the samples of every call
        self._fin = None
        self._read = None
        self.n = None

    def process(self, z_block) -> None:
        """The cells of the next stretch of the channel stream (device or host complex64)."""
        if self._fin is not None:
            raise ValueError("the gate is finished: reset() starts a new run")
        z = D.to_device(z_block, "complex64")
        n = int(z.numel())
        if n == 0:
            return
        if self.sh is None:
            power = D.empty(1, "float64")
            N.call("iqa_mean_power", N.ptr(z), c_int64(min(n, _POWER_SAMPLES)), c_int64(0), N.ptr(power), N.stream_ptr())
            self.sh = choose_shift(float(power.cpu().numpy()[0]))
        cells = D.empty(int(N.lib().iqa_gate_cells(self.pos, n)), "int64")
        N.call("iqa_gate_power", N.ptr(z), c_int64(n), c_int64(self.pos), c_int32(self.sh), N.ptr(cells), N.stream_ptr())
        self._parts.append((self.pos // P.GATE_CELL, cells))
        self.calls.append(n)
        self.pos += n

    def finish(self, n: int | None = None) -> None:
        """Decide the run: cells added by cell number, frames, floor, state, bounds.  No host round trip."""
        n = self.pos if n is None else int(n)
        if n != self.pos:
            raise ValueError(f"the stream held {self.pos} samples, not {n}")
        if self._fin is not None:
            return
        plan, frames = self.plan, self.plan.frames(n)
        if frames > P.GATE_MAX_FRAMES:
            raise ValueError(f"{frames} frames exceed {P.GATE_MAX_FRAMES}")
        self.n = n
        if self.sh is None:
            self.sh = 15
        fin = dict(cells=D.zeros(-(-n // P.GATE_CELL), "int64"), v=D.zeros(frames, "int64"), floor=D.zeros(1, "int64"),
                   s=D.zeros(frames, "uint8"), s2=D.zeros(frames, "uint8"), g=D.zeros(frames, "uint8"),
                   lo=D.zeros(frames, "int32"), hi=D.zeros(frames, "int32"))
        if n:
            for first, part in self._parts:
                N.call("iqa_gate_add_cells", N.ptr(part), c_int64(part.numel()), N.ptr(fin["cells"][first:]), N.stream_ptr())
            self.decide(fin["cells"], n, plan, fin)
        else:
            fin["floor"].fill_(1)
            fin["lo"].fill_(-1)
            fin["hi"].fill_(-1)
        self._fin = fin

    @staticmethod
    def decide(cells, n: int, plan: P.GatePlan, out: dict | None = None) -> dict:
        """``iqa_gate_decide`` over the cells of a stream of ``n`` samples (device int64, added by cell number): the device
        tensors v, floor, s, s2, g, lo, hi.  The entry point checks its arguments before it launches (``ValueError``)."""
        frames = plan.frames(n)
        if out is None:
            out = dict(v=D.zeros(frames, "int64"), floor=D.zeros(1, "int64"), s=D.zeros(frames, "uint8"), s2=D.zeros(frames, "uint8"),
                       g=D.zeros(frames, "uint8"), lo=D.zeros(frames, "int32"), hi=D.zeros(frames, "int32"))
        work = D.empty(2 * frames, "int32")
        N.call("iqa_gate_decide", N.ptr(cells), c_int64(n), c_int32(plan.frame), c_int32(frames), c_int64(plan.num_open),
               c_int64(plan.num_close), c_int32(min(plan.min_frames, 2**31 - 1)), c_int32(min(plan.hang, 2**31 - 1)),
               c_int32(min(plan.lead, 2**31 - 1)), N.ptr(out["v"]), N.ptr(out["floor"]), N.ptr(out["s"]), N.ptr(out["s2"]),
               N.ptr(out["g"]), N.ptr(out["lo"]), N.ptr(out["hi"]), N.ptr(work), N.stream_ptr())
        return out

    def _finished(self) -> dict:
        if self._fin is None:
            raise ValueError("finish() the gate first")
        return self._fin

    def apply(self, audio):
        """The gated audio (device float32[n], a buffer of its own) of the channel-rate audio of the same stream."""
        fin = self._finished()
        a = D.to_device(audio, "float32")
        if int(a.numel()) != self.n:
            raise ValueError(f"the audio holds {int(a.numel())} samples and the stream held {self.n}")
        out = D.empty(self.n, "float32")
        ramp = D.to_device(self.plan.ramp, "float32") if self.plan.ramp_len else None
        N.call("iqa_gate_apply", N.ptr(a), c_int64(self.n), c_int32(self.plan.frame), c_int32(self.plan.frames(self.n)), N.ptr(fin["g"]),
               N.ptr(fin["lo"]), N.ptr(fin["hi"]), N.ptr(ramp), c_int32(self.plan.ramp_len), N.ptr(out), N.stream_ptr())
        return out

    def _host(self) -> dict:
        """v, floor, s2 and g on the host: one read-back."""
        if self._read is None:
            fin = self._finished()
            torch = D.torch_mod()
            frames = int(fin["g"].numel())
            flat = torch.cat([fin["v"].view(torch.uint8), fin["floor"].view(torch.uint8), fin["s2"], fin["g"]]).cpu().numpy()
            self._read = dict(v=flat[: 8 * frames].view(np.int64), floor=int(flat[8 * frames : 8 * frames + 8].view(np.int64)[0]),
                              s2=flat[8 * frames + 8 : 9 * frames + 8], g=flat[9 * frames + 8 :])
        return self._read

    def result(self, frequency: float | None = None) -> GateResult:
        h = self._host()
        return gate_result(self.plan, self.n, self.sh, h["floor"], h["v"], h["s2"], h["g"], frequency)

    def stages(self) -> dict:
        """cells (added by cell number), v, floor, s, s2, g, lo, hi as numpy arrays, sh, ``parts``: (first cell, the call's
        cells) per call, and ``calls``: the samples of every call."""
        fin = self._finished()
        out = {k: t.cpu().numpy() for k, t in fin.items()}
        out["floor"] = int(out["floor"][0])
        out["sh"] = self.sh
        out["parts"] = [(first, part.cpu().numpy()) for first, part in self._parts]
        out["calls"] = list(self.calls)
        return out
