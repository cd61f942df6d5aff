"""What the second pass over a capture launches (DESIGN.md sections 22, 23, 25 and 26), as a trace of ``_native.call``, at each
of its four levels: describe, keying, identify, flex.  A level launches nothing of a higher layer, and what it launches of the
lower ones is the lower level's trace exactly: order, names and scalar values.  Per block and lane the order is
``iqa_describe_accumulate``, ``iqa_quadrature``, then ``iqa_keying_accumulate`` once the lane has a centre, and nothing of the
identification or of FLEX runs before the last block is in.  On the model capture of tests/flex_model.py (two channels, one
FLEX frame of 3200/2) in blocks of 2^20 frames: five blocks, the last one short.  Written against constructor keywords, result
methods and ``_native.call`` only, so that the expected sequence is a property of the pass and not of how it is wired inside."""
from __future__ import annotations

import ctypes
import importlib.util
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


FM = _load("flex_model")
FC = 455.5e6
BLOCK = 1 << 20
#: the entry points of every layer, in chain order (the one second-plane ``iqa_ident_integrate`` of flex is told by position)
LAYERS = (("iqa_mean_power", "iqa_describe_"), ("iqa_quadrature", "iqa_keying_"), ("iqa_ident_",), ("iqa_flex_",))
KEYWORDS = ({}, dict(keying=True), dict(keying=True, identify=True), dict(keying=True, identify=True, flex=True))
RESULTS = ("result", "keying_result", "protocol_result", "flex_result")


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _value(arg):
    """A ctypes scalar's value, a pointer as None / True, an array's values."""
    if isinstance(arg, ctypes.c_void_p):
        return None if not arg.value else True
    if isinstance(arg, ctypes.Array):
        return tuple(arg)
    return getattr(arg, "value", None)


def _layer(name: str) -> int:
    return next((k for k, prefixes in enumerate(LAYERS) if name.startswith(prefixes)), -1)


def _blocks(raw):
    flat = raw.reshape(-1)
    for a in range(0, raw.shape[0], BLOCK):
        yield flat[2 * a : 2 * min(raw.shape[0], a + BLOCK)]


@pytest.fixture(scope="module")
def levels(A):
    """Per level: the trace, the index behind every block's calls, and the lanes' ``keyed_from``.  The finder runs once; every
    level has a fresh describer and calls its result methods in chain order."""
    from iq_to_audio_amd import _native
    from iq_to_audio_amd import dsp_plan as P

    raw = FM.capture("3200/2")
    plan = P.plan_find(FM.FS, raw.shape[0])
    finder = A.ChannelFinder(plan, "s16")
    for block in _blocks(raw):
        finder.process(block)
    fin, found = finder.finish(), finder.result(FC)
    assert len(found.channels) == len(FM.CAPTURE_CHANNELS)
    out = []
    real = _native.call
    for level, keywords in enumerate(KEYWORDS):
        calls, ends = [], []

        def recording(name, *args):
            if _layer(name) >= 0:
                calls.append((name, [_value(a) for a in args]))
            return real(name, *args)

        with pytest.MonkeyPatch.context() as patch:
            patch.setattr(_native, "call", recording)
            describer = A.ChannelDescriber(plan, fin, found.channels, "s16", "iq", **keywords)
            for block in _blocks(raw):
                describer.process(block)
                ends.append(len(calls))
            results = [getattr(describer, name)(FC) for name in RESULTS[: level + 1]]
        out.append(dict(calls=calls, ends=ends, keyed_from=[lane.keyed_from for lane in describer.lanes()], results=results))
    return out


def _without_flex(calls):
    """A flex-level trace without flex's calls: its own entry points and the integration of the second plane, the last
    ``iqa_ident_integrate``, which lies behind the search."""
    names = [name for name, _ in calls]
    extra = max(i for i, name in enumerate(names) if name == "iqa_ident_integrate")
    assert "iqa_ident_search" in names[:extra]
    return [c for i, c in enumerate(calls) if i != extra and _layer(c[0]) != 3]


def test_a_level_launches_nothing_of_a_higher_layer(levels):
    for level, run in enumerate(levels):
        seen = {_layer(name) for name, _ in run["calls"]}
        assert seen == set(range(level + 1)), (level, seen)  # (and every layer has something to do on this capture)
    protocols, pages = levels[3]["results"][2], levels[3]["results"][3]
    assert [ch.protocol for ch in protocols.channels] == ["flex", None] and len(pages.pages) >= 1
    assert [ch.label for ch in levels[3]["results"][1].channels] == ["fsk 3200", "unkeyed"]


@pytest.mark.parametrize("level", (1, 2, 3))
def test_a_level_repeats_the_level_below_it(levels, level):
    calls = levels[level]["calls"]
    below = _without_flex(calls) if level == 3 else [c for c in calls if _layer(c[0]) < level]
    assert below == levels[level - 1]["calls"]
    if level == 3:  # the one exception: the second plane of the 3200-rate frame
        assert sum(name == "iqa_ident_integrate" for name, _ in calls) == 1 + sum(name == "iqa_ident_integrate" for name, _ in levels[2]["calls"])


@pytest.mark.parametrize("level", (0, 1, 2, 3))
def test_the_block_phase(levels, level):
    run = levels[level]
    calls, ends = run["calls"], run["ends"]
    lanes = len(FM.CAPTURE_CHANNELS)
    assert len(ends) == 5
    # nothing of the identification or of FLEX before the last block's calls, and nothing else behind them
    assert all(_layer(name) <= 1 for name, _ in calls[: ends[-1]]) and all(_layer(name) >= 2 for name, _ in calls[ends[-1] :])
    pos = [0] * lanes
    first_keyed = [None] * lanes
    for b, (a, e) in enumerate(zip([0] + ends[:-1], ends)):
        block = calls[a:e]
        names = [name for name, _ in block]
        i = 0
        for lane in range(lanes):
            if b == 0:  # iqa_mean_power once per lane, in front of its first block's sums
                assert names[i] == "iqa_mean_power"
                i += 1
            assert names[i] == "iqa_describe_accumulate"
            _, n, at, prev = block[i][1][:4]  # iqa_describe_accumulate(z, n, pos, prev, sh, ...)
            assert n > 0 and at == pos[lane] and (prev is None) == (b == 0)
            i += 1
            if level >= 1:
                assert names[i] == "iqa_quadrature" and block[i][1][1] == n  # iqa_quadrature(z, n, prev, theta, stream)
                i += 1
                if i < len(names) and names[i] == "iqa_keying_accumulate":
                    _, kn, kat, front = block[i][1][:4]  # iqa_keying_accumulate(theta, n, pos, front, centre, ...)
                    assert kn == n and kat == pos[lane] and (front is None) == (pos[lane] == 0)
                    if first_keyed[lane] is None:
                        first_keyed[lane] = pos[lane]
                    i += 1
                else:
                    assert first_keyed[lane] is None  # once the lane has a centre, every block is keyed
            pos[lane] += n
        assert i == len(names)
    assert all(p > 0 for p in pos)
    assert sorted(first_keyed, key=str) == sorted(run["keyed_from"], key=str)
