"""The table of the second pass's layers (``find_layers.FIND_LAYERS``, DESIGN.md "Adding a layer to the second pass") and what
reads it, without a GPU: the rows of the chain and of the branches, the module and the ``LAYER`` declaration behind every row
above the first, the needs-errors of ``find_channels`` and ``ChannelDescriber`` for every broken chain, what a single
``--find-*`` flag switches on, and the help texts."""
from __future__ import annotations

import dataclasses
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import iq_to_audio_amd as A  # noqa: E402
from iq_to_audio_amd import cli  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd import describe as DS  # noqa: E402
from iq_to_audio_amd import protocol_layer as L  # noqa: E402
from iq_to_audio_amd.find_layers import ALL_LAYERS, FIND_BRANCHES, FIND_LAYERS, FindLayer  # noqa: E402

NAMES = ("describe", "keying", "identify", "flex")
BRANCHES = ("dmr", "p25", "ysf", "nxdn")
PROTOCOLS = ("flex",) + BRANCHES  # the layers that are declared by a ``LAYER`` in their module
#: every chain position k >= 1 with exactly one lower keyword j left out
BROKEN = [(k, j) for k in range(1, len(NAMES)) for j in range(k)]


def test_the_table():
    assert all(isinstance(layer, FindLayer) for layer in FIND_LAYERS)
    assert tuple(layer.name for layer in FIND_LAYERS) == NAMES
    assert [layer.flag for layer in FIND_LAYERS] == ["find_describe", "find_decode", "find_identify", "find_flex"]
    assert [layer.suffix for layer in FIND_LAYERS] == ["describe", "keying", "protocols", "flex"]
    assert [layer.section for layer in FIND_LAYERS] == [22, 23, 25, 26]
    assert [layer.inline for layer in FIND_LAYERS] == [True, True, True, False]
    assert all(callable(layer.result) for layer in FIND_LAYERS)
    with pytest.raises(dataclasses.FrozenInstanceError):
        FIND_LAYERS[0].name = "other"
    # nothing heavy: the CLI reads the table before the GPU is touched
    text = Path(sys.modules[FindLayer.__module__].__file__).read_text()
    assert not re.search(r"^\s*(from \.|import torch|import numpy|from numpy|from torch)", text, re.M)


def test_the_branch_table():
    assert all(isinstance(layer, FindLayer) for layer in FIND_BRANCHES)
    assert tuple(layer.name for layer in FIND_BRANCHES) == BRANCHES
    assert [layer.flag for layer in FIND_BRANCHES] == ["find_dmr", "find_p25", "find_ysf", "find_nxdn"]
    assert [layer.suffix for layer in FIND_BRANCHES] == ["dmr", "p25", "ysf", "nxdn"]
    assert [layer.section for layer in FIND_BRANCHES] == [29, 31, 32, 34]
    assert all(layer.needs == "identify" for layer in FIND_BRANCHES) and all(layer.inline is False for layer in FIND_BRANCHES)
    assert all(callable(layer.result) for layer in FIND_BRANCHES)
    with pytest.raises(dataclasses.FrozenInstanceError):
        FIND_BRANCHES[0].name = "other"
    assert ALL_LAYERS == FIND_LAYERS + FIND_BRANCHES
    tuples = [name for name, value in vars(sys.modules[FindLayer.__module__]).items() if isinstance(value, tuple)]
    assert sorted(tuples) == ["ALL_LAYERS", "FIND_BRANCHES", "FIND_LAYERS"]  # one chain, one branch table, their sum


def test_every_layer_above_the_first_has_its_module():
    assert tuple(DS._MODULES) == tuple(layer.name for layer in ALL_LAYERS[1:])
    for layer in ALL_LAYERS[1:]:
        assert DS._MODULES[layer.name] is sys.modules[f"iq_to_audio_amd.{layer.name}"] and callable(DS._MODULES[layer.name].stage_keys)
    assert tuple(name for name, module in DS._MODULES.items() if hasattr(module, "LAYER")) == PROTOCOLS


@pytest.mark.parametrize("name", PROTOCOLS)
def test_a_protocol_module_binds_its_declaration(name):
    module = DS._MODULES[name]
    layer = module.LAYER
    assert isinstance(layer, L.ProtocolLayer) and layer.name == name == module.__name__.rpartition(".")[2]
    assert getattr(module, f"finish_{name}") == layer.finish and getattr(module, f"{name}_result") == layer.result_of
    assert module.stage_keys == layer.stage_keys and module.PLANE_RATES is layer.rates
    assert layer.rates == {"flex": (1600,), "nxdn": (4800, 2400)}.get(name, (4800,))
    assert layer.decode_stream is module.decode_stream and layer.channel_of is module.channel_of
    with pytest.raises(dataclasses.FrozenInstanceError):
        layer.name = "other"
    # the describer's two generic methods, and the named ones installed from the table
    row = next(r for r in ALL_LAYERS if r.name == name)
    for method in (f"finish_{name}", f"{name}_result"):
        assert callable(getattr(A.ChannelDescriber, method)) and f"section {row.section}" in getattr(A.ChannelDescriber, method).__doc__
    plan = P.plan_find(2.4e6, 100_000)
    fin = dict(runs=np.zeros((0, 8), dtype=np.int64), on=np.zeros((0, plan.slices), dtype=np.uint8))
    bare = A.ChannelDescriber(plan, fin, [], keying=True, identify=True)
    for call in (lambda: bare.finish_layer(name), getattr(bare, f"finish_{name}")):
        with pytest.raises(ValueError, match=f"the describer was made without {name}=True"):
            call()
    asked = []
    stub = type("Stub", (), {"layer_result": lambda self, *args: asked.append(args) or "result"})()
    assert row.result(stub, 433.0e6, 48_000.0) == "result" and asked == [(name, 433.0e6)]  # the row's callable goes down the generic path
    made = A.ChannelDescriber(plan, fin, [], keying=True, identify=True, **{name: True})
    assert made._names == ("describe", "keying", "identify", name)


@pytest.mark.parametrize("k,j", BROKEN, ids=[f"{NAMES[k]}-without-{NAMES[j]}" for k, j in BROKEN])
def test_the_first_missing_link_is_reported(k, j):
    on = {name: True for i, name in enumerate(NAMES[: k + 1]) if i != j}
    message = f"{NAMES[j + 1]}=True needs {NAMES[j]}=True"
    with pytest.raises(ValueError, match=re.escape(message)):  # (before the file is opened)
        A.find_channels("nothing.wav", **on)
    if j >= 1:  # ChannelDescriber has no describe keyword
        plan = P.plan_find(2.4e6, 100_000)
        fin = dict(runs=np.zeros((0, 8), dtype=np.int64), on=np.zeros((0, plan.slices), dtype=np.uint8))
        on.pop("describe")
        with pytest.raises(ValueError, match=re.escape(message)):
            A.ChannelDescriber(plan, fin, [], **on)


def test_the_describer_names_the_missing_keyword():
    plan = P.plan_find(2.4e6, 100_000)
    fin = dict(runs=np.zeros((0, 8), dtype=np.int64), on=np.zeros((0, plan.slices), dtype=np.uint8))
    for method, name in (("finish_keying", "keying"), ("finish_identify", "identify"), ("finish_flex", "flex")):
        with pytest.raises(ValueError, match=f"the describer was made without {name}=True"):
            getattr(A.ChannelDescriber(plan, fin, []), method)()


@pytest.mark.parametrize("flag,on", [("--find-describe", {"find_describe"}), ("--find-decode", {"find_decode"}),
                                     ("--find-identify", {"find_identify", "find_decode"}),
                                     ("--find-flex", {"find_flex", "find_identify", "find_decode"})])
def test_what_a_single_flag_switches_on(flag, on):
    args = cli.build_parser().parse_args(["--in", "capture.wav", flag])
    assert cli.check_find_args(cli.build_parser(), args) is True
    assert {layer.flag for layer in FIND_LAYERS if getattr(args, layer.flag)} == on
    assert all(getattr(args, layer.flag) in (True, False) for layer in FIND_LAYERS)
    assert (args.find_channels, args.find_auto, args.find_top) == (False, False, None)


def test_the_help_texts_are_the_rows():
    text = "".join(cli.build_parser().format_help().split())  # (the help is wrapped, also behind a hyphen: without the blanks)
    for layer in FIND_LAYERS:
        assert "--" + layer.flag.replace("_", "-") in text
        assert "".join(layer.help.split()) in text
