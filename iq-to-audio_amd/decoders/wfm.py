"""Wideband (broadcast) FM with pilot-locked stereo.

The reference has no such decoder (its modes are nfm / am / usb / lsb); this one follows its plug-in contract.  The
discriminator is ``iqa_quadrature``; the composite m (normalised to 75 kHz deviation), the 19 kHz pilot, its doubled
carrier and both 16.5 kHz low-passes run in ONE kernel per block (``iqa_wfm_stereo``, csrc/wfm.hip), which also writes
the per-tile sums of |p|^2 that the stereo decision reads.
"""
from __future__ import annotations

import math
from ctypes import c_float, c_int32, c_int64

from .. import _dev as D
from .. import _native as N
from .. import dsp_plan as P
from .base import DecoderStats, GpuDecoder, level_dbfs
from .nfm import DeemphasisFilter, QuadratureDemod


class WfmStereoCore:
    """The stereo matrix of one stream: the packed taps on the device and the last 2(N-1) discriminator values, carried
    across calls (zeros at the start)."""

    def __init__(self, plan: P.WfmPlan):
        self.plan = plan
        self.taps_dev = D.from_numpy(plan.taps_packed)
        self.hist_len = 2 * (plan.ntaps - 1)
        self._hist = None  # device float32[hist_len]; None = zeros

    @staticmethod
    def partials_for(n: int) -> int:
        return int(N.lib().iqa_wfm_partials(int(n)))

    def process(self, theta, a_out, b_out, *, m_out=None, partials=None) -> None:
        """theta (device float32[n], radians per sample) -> a, b (and m, the per-tile |p|^2 sums) written in place."""
        n = int(theta.numel())
        if n == 0:
            return
        N.call("iqa_wfm_stereo", c_int32(self.plan.ntaps), N.ptr(self.taps_dev), c_float(self.plan.m_scale), N.ptr(theta),
               c_int64(n), N.ptr(self._hist), N.ptr(m_out), N.ptr(a_out), N.ptr(b_out), N.ptr(partials), N.stream_ptr())
        h = self.hist_len
        if n >= h:
            self._hist = theta[n - h :].clone()
        else:
            prev = self._hist if self._hist is not None else D.zeros(h, "float32")
            self._hist = D.torch_mod().cat([prev[n:], theta])


def stereo_matrix(a, b, left=None, right=None):
    """(L, R) = (a + b, a - b) on the device."""
    n = int(a.numel())
    left = D.empty(n, "float32") if left is None else left
    right = D.empty(n, "float32") if right is None else right
    N.call("iqa_wfm_matrix", N.ptr(a), N.ptr(b), c_int64(n), N.ptr(left), N.ptr(right), N.stream_ptr())
    return left, right


class WidebandFMDecoder(GpuDecoder):
    """Broadcast FM: composite, pilot-locked stereo matrix, 50/75 us de-emphasis per output channel.

    ``stages(z)``: ``demod`` (composite m, 1.0 = 75 kHz deviation), ``mono`` (a = L + R), ``stereo_diff`` (b = L - R),
    ``left``, ``right`` (before de-emphasis).  ``process`` returns ``(audio, stats)``: audio is ``(n, 2)`` float32 (L, R
    de-emphasised) when THIS call's pilot level sqrt(mean |p|^2) is at least ``dsp_plan.WFM_STEREO_LEVEL``, else ``(n,)``
    (a, de-emphasised) -- the stage API decides per call; the pipeline decides once per run.  The left, right and mono
    de-emphasis filters each keep their own state, advanced only by the calls that output them.  There is no fused
    ``iqa_demodulate`` form of this mode (``fused_params`` is not implemented)."""

    name = "wideband_fm"

    def __init__(self, deemph_us: float):
        super().__init__()
        self.deemph_us = deemph_us
        self.discriminator = QuadratureDemod()
        self.plan = None
        self.core = None
        self.deemph = {}
        self.stereo = None  # the last call's decision
        self.pilot_level = None  # the last call's sqrt(mean |p|^2)
        self._partials = None

    def on_rate(self, rate: float) -> None:
        self.plan = P.plan_wfm(rate)
        self.core = WfmStereoCore(self.plan)
        self.deemph = {name: DeemphasisFilter(self.deemph_us, rate) for name in ("left", "right", "mono")}

    def stages(self, z) -> list:
        theta = self.discriminator.process(z)
        n = int(theta.numel())
        m, a, b = D.empty(n, "float32"), D.empty(n, "float32"), D.empty(n, "float32")
        self._partials = D.zeros(max(1, self.core.partials_for(n)), "float64")
        self.core.process(theta, a, b, m_out=m, partials=self._partials)
        left, right = stereo_matrix(a, b)
        return [("demod", m), ("mono", a), ("stereo_diff", b), ("left", left), ("right", right)]

    def process(self, samples):
        if self.rate == 0.0:
            raise RuntimeError("Decoder.setup(sample_rate) must be called before processing data.")
        z = D.to_device(samples, "complex64")
        n = int(z.numel())
        chain = self.stages(z)
        st = dict(chain)
        self.pilot_level = math.sqrt(max(float(self._partials.sum().item()), 0.0) / n) if n else 0.0
        self.stereo = self.pilot_level >= P.WFM_STEREO_LEVEL
        if self.stereo:
            torch = D.torch_mod()
            audio = torch.stack([self.deemph["left"].process(st["left"]), self.deemph["right"].process(st["right"])], dim=1)
        else:
            audio = self.deemph["mono"].process(st["mono"])
        self.stats = DecoderStats(rms_dbfs=level_dbfs(audio.reshape(-1)))
        if n:
            self._held = chain + [("audio", audio)]
        return D.like_input(audio, samples), self.stats
