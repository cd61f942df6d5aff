"""Pluggable demodulators on the HIP library (the reference's ``decoders`` package)."""
from __future__ import annotations

from .am import AMDecoder
from .base import Decoder, DecoderStats, GpuDecoder
from .nfm import NarrowbandFMDecoder
from .ssb import SSBDecoder
from .wfm import WidebandFMDecoder

# mode string -> how to build its decoder from (deemph_us, agc_enabled); the AGC switch only reaches the SSB decoder
_BUILDERS = {
    "nfm": lambda deemph_us, agc: NarrowbandFMDecoder(deemph_us=deemph_us),
    "am": lambda deemph_us, agc: AMDecoder(),
    "usb": lambda deemph_us, agc: SSBDecoder(sideband="usb", agc_enabled=agc),
    "lsb": lambda deemph_us, agc: SSBDecoder(sideband="lsb", agc_enabled=agc),
}
_ALIASES = {"fm": "nfm", "ssb": "usb"}
# modes the reference does not have: built only when the caller asks for them (``extensions=True``)
_EXTENSIONS = {
    "wfm": lambda deemph_us, agc: WidebandFMDecoder(deemph_us=deemph_us),
}


def create_decoder(mode: str, *, deemph_us: float, agc_enabled: bool, extensions: bool = False) -> Decoder:
    """The decoder for a ``--demod`` mode (reference decoders/__init__.py:9-24): nfm | fm, am, usb | ssb, lsb; anything
    else is a ``ValueError``, as in the reference.  ``extensions=True`` also builds the modes this project adds: wfm
    (wideband FM stereo, :class:`WidebandFMDecoder`) -- what the pipeline and the CLI pass."""
    key = mode.lower()
    key = _ALIASES.get(key, key)
    build = _BUILDERS.get(key) or (_EXTENSIONS.get(key) if extensions else None)
    if build is None:
        hint = " (an extension mode: create_decoder(..., extensions=True))" if key in _EXTENSIONS else ""
        raise ValueError(f"Unsupported demod mode '{key}'.{hint}")
    return build(deemph_us, agc_enabled)


__all__ = ["Decoder", "DecoderStats", "GpuDecoder", "create_decoder", "NarrowbandFMDecoder", "AMDecoder", "SSBDecoder",
           "WidebandFMDecoder"]
