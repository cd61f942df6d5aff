"""Which precision a target's channelizer runs at: the SSB-with-AGC rule and the precision guard."""
from __future__ import annotations

import math

from .channelizer import _ChannelKernel
from .dsp_plan import dropped_floor

#: Precision guard.  The fixed-point channelizers' error is a fraction of the WIDEBAND level whatever the channel holds
#: (tap rounding x wideband RMS, 1..5 x that on tonal captures) plus a level-independent floor, the low tap byte x low data
#: byte products the int16 kernels drop (MfmaPlan.z_error_rms, dsp_plan.dropped_floor), and the FM discriminator divides by
#: the channel's own level: audio error ~ 0.024 x error / |z|.  An NFM channel whose probed level is below guard x
#: (expected z error) is therefore channelized at the next precision that clears it (measured: a -70 dBFS NFM signal
#: beside a full-scale tone comes out 2.8e-4 RMS off the reference at "fast").  The floor is the largest of three figures of
#: the plan: the RMS for uniform low bytes (a loud, noisy capture), the zero-input response (a stretch whose values stand
#: still: applied at every level, because the level estimate of a warm-up block does not make every stretch loud), and,
#: for a capture below dsp_plan.QUIET_WIDEBAND (128 LSB), the bound for a clean in-channel signal, whose low bytes are
#: coherent with it (exact model: a 50 LSB NFM signal alone in the capture is 1.9e-4 off at "fast", 1.4e-6 at "fine").
PRECISION_GUARD = 1000.0
#: the demodulators that divide by |z| (the discriminator): what the guard protects
FM_MODES = ("nfm", "fm", "wfm")
#: what SSB with the AGC on starts at (``base_precision``)
SSB_AGC_PRECISION = "full"


def is_guarded(demod_mode: str | None) -> bool:
    """Whether the precision guard applies to a target of ``demod_mode``."""
    return (demod_mode or "").lower() in FM_MODES


def pick_precision(kernel_for, base: str, demod_mode: str | None, channel_power, wideband_rms, guard: float | None = None,
                   memo: dict | None = None, floor_scale: float = 1.0) -> str:
    """The cheapest precision, not below ``base``, at which a channel of mean power ``channel_power`` (|z|^2, from the
    mixer-sign probe) in a capture of wideband RMS ``wideband_rms`` keeps the 1e-4 audio bar.  Only NFM is guarded (AM
    and SSB do not divide by |z|).  ``kernel_for(precision)`` returns the planned ``_ChannelKernel``; ``memo`` (a dict the
    caller keeps per channel and sign) remembers each precision's (tap-rounding norm, (floor, zero-input response, coherent
    bound)), so that a batch asks the kernels once, not once per capture.  ``floor_scale``: what one unit of the kernel's full
    scale is worth in the capture's -- 2^shift for a float32 capture run as int16 planes with ``shift`` bits of headroom
    (hi = rint(2^(15 - shift) x)): the tap-rounding term follows the level and is unchanged, the level-independent floor
    grows by that factor, and the planes are quiet (``dsp_plan.QUIET_WIDEBAND``) at 2^shift times the level."""
    levels = _ChannelKernel.PRECISIONS
    guard = PRECISION_GUARD if guard is None else guard
    if not guard or channel_power is None or wideband_rms is None or not is_guarded(demod_mode):
        return base
    level = math.sqrt(max(float(channel_power), 0.0))
    for name in levels[levels.index(base):]:
        if name == "float32":
            break
        known = None if memo is None else memo.get(name)
        if known is None:
            k = kernel_for(name)
            if k.precision != name:  # (this capture format has no such kernel: uint8 "full", float32 anything)
                known = False
            elif not k._mfma_ok:
                known = (0.0, (0.0, 0.0, 0.0))
            else:
                mp = k._ensure_mfma()
                # (a plan that states the uniform floor alone has no quiet-data figures: they count as 0)
                known = (float(mp.err_norm), (float(mp.floor_rms), float(getattr(mp, "zero_rms", 0.0)),
                                              float(getattr(mp, "coherent_rms", 0.0))))
            if memo is not None:
                memo[name] = known
        if known is False:
            continue
        err = math.hypot(known[0] * wideband_rms, floor_scale * dropped_floor(known[1], wideband_rms / floor_scale))
        if err <= 0.0 or level >= guard * err:
            return name
    return "float32"


def base_precision(demod_mode: str | None, agc_enabled: bool) -> str:
    """SSB with the AGC on is ill-conditioned in the reference itself: ``_apply_agc`` adds 0.001*(target/|s| - gain) per
    sample for |s| down to 1e-6 (decoders/ssb.py:75-77), so a z difference of 1e-6 near a zero crossing moves the gain
    by hundreds.  Those targets take the "full" precision (z error below the float32 rounding of z itself); everything
    else starts at "fast"."""
    return SSB_AGC_PRECISION if ((demod_mode or "").lower() in ("usb", "lsb", "ssb") and agc_enabled) else "fast"
