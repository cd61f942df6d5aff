"""The layers of the second pass over a capture: what ``--find-describe``, ``--find-decode``, ``--find-identify``,
``--find-flex``, ``--find-dmr``, ``--find-p25``, ``--find-ysf`` and ``--find-nxdn`` add to the finder's channel list (DESIGN.md sections
22, 23, 25, 26, 29, 31, 32 and 34).

``FIND_LAYERS`` lists the chain, in order: every row needs the row in front of it.  ``FIND_BRANCHES`` lists the layers that
hang off one row of the chain (``needs``) and off nothing else, in the order of their results, printed lines and files; the
next branch is a row at its end.  ``ALL_LAYERS`` is the chain, then the branches: the one that is looped over.  ``find_channels``,
``ChannelDescriber`` and the CLI read a layer's keyword, flag, result and file suffix from its row; a new protocol layer is a row
here and its own module with its ``LAYER`` ("Adding a layer to the second pass").  Nothing heavy is imported here:
the CLI reads the tables before the GPU is touched."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable


@dataclass(frozen=True)
class FindLayer:
    name: str  # the keyword of ``find_channels`` and, above the first row, of ``ChannelDescriber``
    flag: str  # the CLI dest; the flag is ``--`` + the dest with dashes
    section: int  # its DESIGN.md section
    result: Callable  # (describer, center_freq, fs_ch) -> the layer's result object
    suffix: str  # the result is written to ``<capture stem>.<suffix>.json``
    inline: bool  # line i of ``result.lines()`` goes under channel i's line; False: all its lines follow the channel list
    help: str  # the CLI flag's help text
    needs: str | None = None  # a branch: the name of the chain row it hangs off; None for a row of the chain

    @property
    def option(self) -> str:
        return "--" + self.flag.replace("_", "-")


def _protocol(name: str) -> Callable:
    """The ``result`` of a protocol layer's row: the describer's generic path, by the row's name."""
    return lambda d, fc, fs_ch: d.layer_result(name, fc)


FIND_LAYERS = (
    FindLayer("describe", "find_describe", 22, lambda d, fc, fs_ch: d.result(fc), "describe", True,
              "Find the channels, then measure each one in a second pass: a label (nfm, am, ssb, wfm, carrier, unknown) "
              "and a suggested --demod, --bw and frequency.  Implies --find-channels."),
    FindLayer("keying", "find_decode", 23, lambda d, fc, fs_ch: d.keying_result(fc, fs_ch), "keying", True,
              "Find and describe the channels and measure the keying of each one: whether its discriminator switches on "
              "a symbol clock (fsk 512 ... 9600) and which side decoders fit it.  With --find-top N --find-auto every "
              "target runs with its chosen decoders.  Implies --find-describe."),
    FindLayer("identify", "find_identify", 25, lambda d, fc, fs_ch: d.protocol_result(fc), "protocols", True,
              "Find, describe and key the channels, and name the protocol of every channel keyed at 1600, 2400, 3200 or "
              "4800 baud by its frame synchronisation words: DMR, P25, YSF, NXDN or FLEX with its mode.  Implies "
              "--find-decode."),
    FindLayer("flex", "find_flex", 26, _protocol("flex"), "flex", False,
              "Find, describe, key and identify the channels, and decode the pages of every FLEX channel: capcode, type "
              "and text, one line per page, also written to <capture stem>.flex.json.  Implies --find-identify."),
)


FIND_BRANCHES = (
    FindLayer("dmr", "find_dmr", 29, _protocol("dmr"), "dmr", False,
              "Find, describe, key and identify the channels, and decode the data bursts of every channel that carries DMR "
              "sync words: colour code, slot, link control and CSBKs, one line per call and per CSBK, also written to "
              "<capture stem>.dmr.json.  Implies --find-identify.", needs="identify"),
    FindLayer("p25", "find_p25", 31, _protocol("p25"), "p25", False,
              "Find, describe, key and identify the channels, and decode the frames of every channel that carries P25 phase 1 "
              "frame sync words: NAC, link control and trunking blocks, one line per call and per distinct TSBK, also "
              "written to <capture stem>.p25.json.  Implies --find-identify.", needs="identify"),
    FindLayer("ysf", "find_ysf", 32, _protocol("ysf"), "ysf", False,
              "Find, describe, key and identify the channels, and decode the frames of every channel that carries YSF (System "
              "Fusion) frame sync words: the FICH and the callsigns of the data channels, one line per transmission (source, "
              "destination, repeater, mode, duration), also written to <capture stem>.ysf.json.  No voice.  Implies "
              "--find-identify.", needs="identify"),
    FindLayer("nxdn", "find_nxdn", 34, _protocol("nxdn"), "nxdn", False,
              "Find, describe, key and identify the channels, and decode the frames of every channel that carries NXDN frame "
              "sync words at 4800 or 2400 symbols/s: the LICH, the SACCH, the FACCH1s and the outbound CAC, one line per call "
              "(RAN, source, destination, call type, cipher, duration) and per distinct control message, also written to "
              "<capture stem>.nxdn.json.  No voice.  Implies --find-identify.", needs="identify"),
)

ALL_LAYERS = FIND_LAYERS + FIND_BRANCHES


def active_layers(switches: dict) -> tuple:
    """The rows switched on in ``switches`` (name -> bool): the chain's in chain order, then the branches'.  ``ValueError`` for
    the first row of the chain that is on while the row in front of it is not, then for the first branch that is on while the
    row it needs is not."""
    for below, layer in zip(FIND_LAYERS, FIND_LAYERS[1:]):
        if switches.get(layer.name) and not switches.get(below.name):
            raise ValueError(f"{layer.name}=True needs {below.name}=True")
    for layer in FIND_BRANCHES:
        if switches.get(layer.name) and not switches.get(layer.needs):
            raise ValueError(f"{layer.name}=True needs {layer.needs}=True")
    return tuple(layer for layer in ALL_LAYERS if switches.get(layer.name))
