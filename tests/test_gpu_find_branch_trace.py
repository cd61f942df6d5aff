"""What a branch of the second pass launches (DESIGN.md sections 27, 29, 31, 32 and 34), as a trace of ``_native.call``: per
branch ``b`` of dmr, p25, ysf and nxdn, on the model capture of tests/<b>_model.py (two channels, the first of them ``b``'s) in
blocks of 2^20 frames, three describers behind one finder pass: ``keying, identify`` alone, with ``b`` beside them, and with all
four branches, the results asked for in table order.  (a) A branch adds its own entry points (``iqa_<b>_``) and nothing else: the
trace without them is the trace of ``keying, identify`` alone, in order, names and scalar values, every entry point of the
second pass's layers recorded (tests/test_gpu_find_trace.py's, and the protocol layers'); no plane is integrated for a
branch, it reads section 25's.  (b) All of a branch's calls lie behind the last
block's calls.  (c) A branch's result beside the other three is its result alone.  With all four on, the branches' calls stand
grouped in table order.  Written against constructor keywords, result methods and ``_native.call`` only, so that the expected
sequence is a property of the pass and not of how it is wired inside."""
from __future__ import annotations

import ctypes
import importlib.util
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

BRANCHES = ("dmr", "p25", "ysf", "nxdn")  # the table's order
FC = 433.0e6
BLOCK = 1 << 20
BELOW = dict(keying=True, identify=True)
BELOW_RESULTS = ("keying_result", "protocol_result")
#: the entry points of the second pass's layers: the chain's, then the branches'
RECORDED = ("iqa_mean_power", "iqa_describe_", "iqa_quadrature", "iqa_keying_", "iqa_ident_", "iqa_flex_") + tuple(f"iqa_{b}_" for b in BRANCHES)


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


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


def _branch(name: str) -> int:
    """The place in the table of the branch whose entry point ``name`` is; -1 for any other entry point."""
    return next((k for k, b in enumerate(BRANCHES) if name.startswith(f"iqa_{b}_")), -1)


def _blocks(raw):
    flat = raw.reshape(-1)
    for a in range(0, raw.shape[0], BLOCK):
        yield flat[2 * a : 2 * min(raw.shape[0], a + BLOCK)]


_RUNS: dict = {}


def _runs(A, b: str) -> dict:
    """Of ``b``'s model capture, behind one finder pass: the runs ``below`` (keying, identify), ``alone`` (with ``b``) and ``all``
    (with the four branches), each a fresh describer whose result methods are called in table order: its trace, the index
    behind the last block's calls and its results by name.  Made once per capture and left unchanged."""
    if b in _RUNS:
        return _RUNS[b]
    from iq_to_audio_amd import _native
    from iq_to_audio_amd import dsp_plan as P

    model = _load(f"{b}_model")
    raw = model.capture()
    plan = P.plan_find(model.FS, raw.shape[0])
    finder = A.ChannelFinder(plan, "s16")
    for block in _blocks(raw):
        finder.process(block)
    fin, found = finder.finish(), finder.result(FC)
    assert len(found.channels) == len(model.CAPTURE_CHANNELS)
    real = _native.call
    out = {}
    for tag, branches in (("below", ()), ("alone", (b,)), ("all", BRANCHES)):
        calls = []

        def recording(name, *args):
            if name.startswith(RECORDED):
                calls.append((name, [_value(a) for a in args]))
            return real(name, *args)

        with pytest.MonkeyPatch.context() as patch:
            patch.setattr(_native, "call", recording)
            describer = A.ChannelDescriber(plan, fin, found.channels, "s16", "iq", **BELOW, **{name: True for name in branches})
            for block in _blocks(raw):
                describer.process(block)
            end = len(calls)
            results = {name: getattr(describer, name)(FC) for name in BELOW_RESULTS + tuple(f"{x}_result" for x in branches)}
        out[tag] = dict(calls=calls, end=end, results=results)
    _RUNS[b] = out
    return out


@pytest.mark.parametrize("b", BRANCHES)
def test_a_branch_adds_its_own_calls_and_nothing_else(A, b):
    runs = _runs(A, b)
    below, alone = runs["below"], runs["alone"]
    own = [i for i, (name, _) in enumerate(alone["calls"]) if name.startswith(f"iqa_{b}_")]
    # the capture gives the branch something to do, and it decodes it
    assert own and {_branch(name) for name, _ in alone["calls"]} == {-1, BRANCHES.index(b)}
    channel = alone["results"][f"{b}_result"].channels[0]
    assert channel.note == "" and alone["results"][f"{b}_result"].lines()
    assert {_branch(name) for name, _ in below["calls"]} == {-1} and below["end"] < len(below["calls"])
    # (a) without its entry points the trace is that of keying and identify alone
    assert [c for c in alone["calls"] if _branch(c[0]) < 0] == below["calls"]
    assert alone["end"] == below["end"]
    # (b) all of them behind the last block's calls
    assert min(own) >= alone["end"]
    # the layers below give what they gave without the branch
    for name in BELOW_RESULTS:
        assert alone["results"][name].to_json() == below["results"][name].to_json()


@pytest.mark.parametrize("b", BRANCHES)
def test_a_branch_beside_the_others_gives_its_result_alone(A, b):
    runs = _runs(A, b)
    assert runs["all"]["results"][f"{b}_result"].to_json() == runs["alone"]["results"][f"{b}_result"].to_json()
    for name in BELOW_RESULTS:
        assert runs["all"]["results"][name].to_json() == runs["below"]["results"][name].to_json()


@pytest.mark.parametrize("b", BRANCHES)
def test_all_four_branches_launch_grouped_in_table_order(A, b):
    runs = _runs(A, b)
    below, every = runs["below"], runs["all"]
    assert [c for c in every["calls"] if _branch(c[0]) < 0] == below["calls"] and every["end"] == below["end"]
    assert all(_branch(name) < 0 for name, _ in every["calls"][: every["end"]])
    order = [_branch(name) for name, _ in every["calls"][every["end"] :] if _branch(name) >= 0]
    assert order == sorted(order) and set(order) == set(range(len(BRANCHES)))
    # behind the first call of a branch there is nothing but the branches: the identification lies in front of all of them
    first = next(i for i, (name, _) in enumerate(every["calls"]) if _branch(name) >= 0)
    assert all(_branch(name) >= 0 for name, _ in every["calls"][first:])
    # and what the branch of this capture launches beside the others is what it launches alone
    own = lambda calls: [c for c in calls if _branch(c[0]) == BRANCHES.index(b)]  # noqa: E731
    assert own(every["calls"]) == own(runs["alone"]["calls"])
