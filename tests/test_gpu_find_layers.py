"""What ``find_channels`` returns at each level of the second pass (DESIGN.md sections 21, 22, 23, 25 and 26) on the MI355X:
the bare ``FindResult`` without a flag, then one more result per layer, and every level's results are the next level's without
its last one.  On the model capture of tests/flex_model.py (two channels, one FLEX frame of 3200/2) written as a WAV."""
from __future__ import annotations

import importlib.util
import json
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
KEYWORDS = ("describe", "keying", "identify", "flex")  # in chain order: level k sets the first k


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


@pytest.fixture(scope="module")
def levels(A, tmp_path_factory):
    """``find_channels`` on the capture at the five levels, once each."""
    from iq_to_audio_amd import iqio

    wav = tmp_path_factory.mktemp("layers") / f"model_{int(FC)}Hz.wav"
    iqio.write_wav_iq(wav, FM.capture("3200/2"), int(FM.FS), "s16")
    return [A.find_channels(wav, **{name: True for name in KEYWORDS[:k]}) for k in range(len(KEYWORDS) + 1)]


def test_one_more_result_per_level(A, levels):
    from iq_to_audio_amd.flex import FlexResult
    from iq_to_audio_amd.identify import ProtocolResult

    classes = (A.FindResult, A.DescribeResult, A.KeyingResult, ProtocolResult, FlexResult)
    assert isinstance(levels[0], A.FindResult)
    for k in range(1, len(levels)):
        assert isinstance(levels[k], tuple) and len(levels[k]) == k + 1
        assert [type(r) for r in levels[k]] == list(classes[: k + 1])
    assert levels[1][0] == levels[0] and levels[0].center_freq == FC and len(levels[0].channels) == len(FM.CAPTURE_CHANNELS)
    # on this capture every layer has something to say
    full = levels[-1]
    assert [ch.label for ch in full[2].channels] == ["fsk 3200", "unkeyed"]
    assert [ch.protocol for ch in full[3].channels] == ["flex", None] and len(full[4].pages) >= 1


@pytest.mark.parametrize("k", (1, 2, 3))
def test_a_level_is_the_next_one_without_its_last_result(levels, k):
    assert levels[k] == levels[k + 1][:-1]  # (dataclass ==, result by result)


@pytest.mark.parametrize("k", (0, 1, 2, 3, 4))
def test_the_results_round_trip_through_json(levels, k):
    for r in (levels[k],) if k == 0 else levels[k]:
        assert type(r).from_json(json.loads(json.dumps(r.to_json()))) == r
