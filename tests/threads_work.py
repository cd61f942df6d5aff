"""Library-level jobs of ``test_gpu_threads.py`` and of its child process (``threads_first_use_child.py``): each job
prepares its buffers, queues its launches on the CURRENT stream, and hands back host copies of what they wrote -- so the
same job can run serially, from a thread, or as a process's first launch, and the results can be compared bit for bit.
Shapes, lane tables and models are those of ``test_gpu_mfma_exact.py`` and ``test_gpu_rds_shapes.py``."""
from __future__ import annotations

import hashlib

import numpy as np
import test_gpu_mfma_exact as E
import test_gpu_rds_shapes as R

from oracle import mfma_model as M

RG_PACE_WORDS = E.RG_PACE_WORDS


def digest(arrays) -> str:
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.view(np.uint8).reshape(-1))
    return h.hexdigest()


class RingJob:
    """One lane of the contiguous-slot ring kernel at D = 104 (7 k steps, int32 sums): ``…_ring_multi<7>`` raises its
    dynamic-LDS limit at the process's first launch."""

    def __init__(self, who: int):
        self.d, self.ks, self.opb, self.n_out, self.m_first = 104, 7, 256, 256 * 5 + 37, 64 + 500
        self.mp = E.make_plan(64 * self.d - 13, self.d, "s16", True, seed=900 + who)
        self.raw, self.x, self.n_frames, self.consumed = E.setup_capture("s16", self.d, 1, 0, self.ks, 0, 0, self.m_first, self.n_out,
                                                                         self.opb, seed=910 + who)
        self.lane = E.Lane(self.mp, 0, conj=who & 1, scale=(1.0 + 0j, -1j)[who & 1])
        E.device_afrag(self.mp)  # (uploaded here, not by the launch: the helper's table is not made for threads)

    def launch(self):
        E.launch("multi", "s16", self.d, 0, self.ks, self.opb, [self.lane], self.x, self.n_frames, self.consumed, self.m_first, self.n_out)

    def outputs(self):
        return [self.lane.out.cpu().numpy()]

    def check(self):
        E.check_lane(self.lane, 0, self.raw, self.d, self.consumed, self.m_first, self.n_out, "ring d104")


class PerLaneJob:
    """``k_channelize_mfma_s16`` (the per-lane kernel, 16-bit taps) at D = 104: the other kernel that raises its limit."""

    def __init__(self, who: int):
        from iq_to_audio_amd import _dev as D

        N = E._N()
        self.d, self.opb, self.n_out, self.m_first = 104, 512, 2 * 512 + 77, 64 + 500
        self.L = 64 * self.d - 13
        self.mp = E.make_plan(self.L, self.d, "s16", False, seed=920 + who)
        self.consumed = (self.m_first - 64) * self.d + 1 - 11
        self.n_frames = max(E.perlane_frames_needed(self.d, ps.k_first, ps.k_count, self.mp.groups[ps.group].q, self.m_first, self.n_out,
                                                    self.opb, self.consumed) for ps in self.mp.passes)
        raw = E.capture("s16", self.n_frames + 4096, seed=930 + who)
        self.x = D.to_device(raw, "int16")
        self.raw = raw[: 2 * self.n_frames]
        self.prm = N.ChanParams(fmt=0, ntaps=self.L, decimation=self.d, conj_sum=0, rotate=0, reserved=0, rot_step=0, rot_base=12345,
                                out_scale_re=1.0, out_scale_im=0.0)
        E.device_afrag(self.mp)
        self.z = None

    def launch(self):
        self.z = E._perlane_run(self.mp, self.x, self.n_frames, self.consumed, self.m_first, self.n_out, self.opb, self.prm)

    def outputs(self):
        return [self.z.cpu().numpy()]

    def check(self):
        want = M.finish(M.plan_sums(self.mp, self.raw, "s16", self.d, self.consumed, self.m_first, self.n_out, False), self.m_first, 0, 0,
                        0, 12345, 1.0 + 0j)
        E.check_z(self.z, want, 0, "per-lane d104")


class RdsJob:
    """``iqa_rds_baseband`` at the rate with the largest LDS image (1.42 MS/s: 60 408 bytes; the entry point keeps every
    image below 64 KiB and never raises a limit)."""

    FS = 1_420_000.0

    def __init__(self, who: int):
        self.theta, self.want = R.case(self.FS)
        self.got = None

    def launch(self):
        self.got = R.run(self.FS, self.theta)  # (reads its results back: the core's store is host-joined)

    def outputs(self):
        return [self.got["y"], self.got["q"]]

    def check(self):
        R.check_baseband("threads", self.FS, self.got, self.want, R.P.plan_rds(self.FS).j0)


class PairJob:
    """A lane-pair launch with pacing on: four pairs (pace_units = 4) over ranges of 32 outputs.  ``lanes()`` makes a fresh
    table (own outputs) over the shared capture; ``want`` holds the model's z per lane, computed once."""

    def __init__(self, ks: int):
        self.ks, self.d = ks, {13: 208, 9: 144}[ks]
        assert -(-2 * self.d // 32) == ks
        self.opb, self.m_first = 32, 64 + 300
        self.n_out = 32 * 8 * 34 + 32 * 3 + 1
        self.n_lanes = 8
        self.plans = [E.make_plan(64 * self.d - 7 - 5 * i, self.d, "s16", True, seed=940 + ks + i) for i in range(2)]
        self.raw, self.x, self.n_frames, self.consumed = E.setup_capture("s16", self.d, 1, 0, ks, 0, 0, self.m_first, self.n_out, self.opb,
                                                                         seed=950 + ks)
        self.want = [E.model_lane_out(ln, 0, self.raw, self.d, self.consumed, self.m_first, self.n_out) for ln in self.lanes()]
        for mp in self.plans:
            E.device_afrag(mp)

    @property
    def slice_words(self) -> int:
        """The launcher's slice of the pacing buffer: groups * 8 * (n_lanes / 2) words, rounded up to 64."""
        groups = -(-(-(-self.n_out // self.opb)) // 8)
        words = groups * 8 * (self.n_lanes // 2)
        assert words <= RG_PACE_WORDS  # (else the launch runs unpaced)
        return (words + 63) & ~63

    def lanes(self):
        return [E.Lane(self.plans[i % 2], 0, conj=(i // 2) & 1, scale=(1.0 + 0j, 1j, -1j)[i % 3]) for i in range(self.n_lanes)]

    def launch(self, lanes):
        E.launch("pairs", "s16", self.d, 0, self.ks, self.opb, lanes, self.x, self.n_frames, self.consumed, self.m_first, self.n_out)

    def check(self, lanes, what):
        for i, (ln, want) in enumerate(zip(lanes, self.want)):
            E.assert_exact(ln.out, want, f"{what} lane {i}")


FIRST_USE = (RingJob, PerLaneJob, RdsJob)


def first_use_jobs(who: int):
    return [cls(who) for cls in FIRST_USE]
