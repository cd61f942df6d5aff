"""What the resident runners and the file pipeline launch, and on which stream, as a trace of ``_native.call``.

The other tests pin the RESULTS of this host-side sequencing (most of them bit for bit); this one pins the ORDER of the
native calls and the stream each is queued on, which is what the runners' speed rests on.  Every entry is
``"<entry point>@<stream>"`` with the stream one of ``compute`` (the stream the runner was created on), ``aux``, ``egress``,
``tail`` (``_dev.side_stream``) or ``other`` (a graph's capturing stream); no pointers are recorded.

The expected sequences are literals.  They were recorded by running the scenario functions of this file on commit 2ba9af1
("Squelch a target's audio by channel power during the run"), the last commit before the orchestration was split into
``mixsign.py`` / ``precision.py`` / ``channel_demod.py`` / ``staging.py``; a change that moves a launch, or its stream,
shows up here as a diff of two lists.

Shapes: 2.5 MS/s, the 12.5 kHz filter, D = 26, 0.4 s per capture -- the smallest capture whose ~38 k outputs take the ring
kernel (``mfma_min_outputs`` = 32768).
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

FS, F_OFF, SECS = 2.5e6, 25e3, 0.4


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def record_native_calls(monkeypatch) -> list:
    """Wrap ``_native.call``; returns the list that fills with "entry@stream" per native call, in call order."""
    import torch

    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native

    calls = []
    real = _native.call
    compute = int(torch.cuda.current_stream().cuda_stream)

    def label(raw: int) -> str:
        if raw == compute:
            return "compute"
        for (_, role), s in D._SIDE_STREAMS.items():  # (looked up, never made here: the runners make them in their own order)
            if role in ("aux", "egress", "tail") and int(s.cuda_stream) == raw:
                return role
        return "other"

    def recording(name, *args):
        calls.append(f"{name}@{label(D.current_raw_stream())}")
        return real(name, *args)

    monkeypatch.setattr(_native, "call", recording)
    return calls


@pytest.fixture()
def trace(monkeypatch):
    return record_native_calls(monkeypatch)


@pytest.fixture(scope="module")
def captures():
    """The 0.4 s benchmark capture with its carrier at +f_off and at -f_off (host int16, interleaved)."""
    return {side: O.synth_capture_s16(FS, SECS, side * F_OFF).reshape(-1) for side in (1, -1)}


def _capture_runner(A, **kw):
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.batch import ResidentCaptureRunner

    d, fs_ch = P.choose_decimation(FS, 96_000.0)
    taps = A.design_channel_filter(FS, 12_500.0, d)
    return ResidentCaptureRunner(taps, sample_rate=FS, freq_offset=F_OFF, decimation=d, fs_channel=fs_ch,
                                 chunk=P.tune_chunk_size(FS, 1_048_576), n_frames=int(round(FS * SECS)), **kw)


def _resident(cap):
    import torch

    from iq_to_audio_amd import _dev as D

    dev = D.to_device(cap, "int16")
    torch.cuda.synchronize()
    return dev


# ---- the scenarios: each returns what it recorded ----------------------------------------------------------------------


def scenario_submit_collect(A, captures, trace) -> dict:
    runner, dev = _capture_runner(A), _resident(captures[1])
    del trace[:]
    r = runner.collect(runner.submit(dev))
    assert r["sign"] == 1 and runner.redone == dict(sign=0, precision=0)
    return dict(submit_collect=list(trace))


def scenario_two_resident_in_flight(A, captures, trace) -> dict:
    runner, dev = _capture_runner(A), _resident(captures[1])
    del trace[:]
    tickets = [runner.submit(dev, resident=True), runner.submit(dev, resident=True)]
    queued = len(trace)
    for t in tickets:
        assert runner.collect(t)["sign"] == 1
    return dict(two_resident_submits=trace[:queued], two_resident_collects=trace[queued:])


def scenario_sign_redo(A, captures, trace) -> dict:
    runner, dev = _capture_runner(A), _resident(captures[-1])
    del trace[:]
    ticket = runner.submit(dev)
    queued = len(trace)
    r = runner.collect(ticket)
    assert r["sign"] == -1 and runner.redone == dict(sign=1, precision=0)
    return dict(sign_redo_submit=trace[:queued], sign_redo_collect=trace[queued:])


def scenario_captured(A, captures, trace) -> dict:
    """``submit_captured`` on a fixed buffer, two slots: the first call (the step once the ordinary way, then captured into
    a graph and replayed), the same for the second slot, then the first slot again -- a replay."""
    runner, dev = _capture_runner(A, slots=2), _resident(captures[1])
    del trace[:]
    signs = [runner.collect(runner.submit_captured(dev))["sign"]]
    first = len(trace)
    signs.append(runner.collect(runner.submit_captured(dev))["sign"])
    second = len(trace)
    signs.append(runner.collect(runner.submit_captured(dev))["sign"])
    assert signs == [1, 1, 1] and len(runner._graphs) == 2 and getattr(runner, "replays_redone", 0) == 0
    return dict(captured_first=trace[:first], captured_second_slot=trace[first:second], captured_replay=trace[second:])


def scenario_bank(A, captures, trace) -> dict:
    from iq_to_audio_amd.batch import ResidentBankRunner

    targets = [dict(freq_offset=F_OFF, demod_mode="nfm", bandwidth=12_500.0), dict(freq_offset=-150e3, demod_mode="am", bandwidth=10_000.0),
               dict(freq_offset=400e3, demod_mode="usb", bandwidth=2_800.0, agc_enabled=True)]
    runner, dev = ResidentBankRunner(targets, sample_rate=FS, n_frames=int(round(FS * SECS))), _resident(captures[1])
    del trace[:]
    ticket = runner.submit(dev)
    queued = len(trace)
    res = runner.collect(ticket)
    assert [r["precision"] for r in res] == ["fast", "fast", "full"] and res[0]["sign"] == 1
    return dict(bank_submit=trace[:queued], bank_collect=trace[queued:], bank_redone=dict(runner.redone))


PIPELINE_ENTRIES = ("iqa_f32_split_s16", "iqa_channelize", "iqa_mfma_combine")
BLOCK = 1_048_576  # frames per device block: one reference chunk at 2.5 MS/s, the smallest block the pipeline forms there


def scenario_pipeline_f32(A, tmp_path, trace) -> dict:
    """A cf32 file of four blocks: all k / 32768 (one plane), a non-zero low plane (two planes), all k / 32768 again but
    inside the low plane's history (two planes), a value the planes cannot hold (float32 kernel from there on)."""
    s16 = O.synth_capture_s16(FS, 4 * BLOCK / FS, F_OFF).astype(np.float64)
    assert s16.shape[0] == 4 * BLOCK
    t = np.arange(BLOCK, 2 * BLOCK) / FS
    tone = 12_000.0 / 32768.0 * np.exp(2j * np.pi * F_OFF * t)  # below hi's half step: it lives in the low plane
    s16[BLOCK : 2 * BLOCK, 0] += tone.real
    s16[BLOCK : 2 * BLOCK, 1] += tone.imag
    f32 = (s16 / 32768.0).astype(np.float32)
    f32[3 * BLOCK + BLOCK // 2, 0] = 4.0
    src = tmp_path / "trace_400000000Hz.cf32"
    src.write_bytes(f32.tobytes())
    cfg = A.ProcessingConfig(in_path=src, target_freq=400e6 + F_OFF, input_sample_rate=FS, demod_mode="nfm", mix_sign_override=1,
                             output_path=tmp_path / "trace.wav")
    multi = A.MultiChannelPipeline([cfg])
    multi.owners[0].block_frames_target = BLOCK
    del trace[:]
    multi.run()
    assert (multi.integer_blocks, multi.split_blocks, multi.f32_shift) == (2, 1, 0)
    return dict(pipeline_f32=[c for c in trace if c.split("@")[0].startswith(PIPELINE_ENTRIES)])


# ---- what commit 2ba9af1 records ----------------------------------------------------------------------------------------

EXPECTED = {
    "submit_collect": """
        iqa_channelize_mfma_multi@compute iqa_mean_power_batch@compute iqa_raw_level@compute iqa_channelize@compute
        iqa_channelize_mfma_multi@compute iqa_channelize@compute iqa_demodulate@compute iqa_resample@compute
        iqa_trickle_copy@egress
    """.split(),
    "two_resident_submits": """
        iqa_channelize@aux iqa_channelize_mfma_multi@compute iqa_channelize@aux iqa_channelize_mfma_multi@aux
        iqa_mean_power_batch@aux iqa_raw_level@aux iqa_demodulate@compute iqa_resample@compute iqa_channelize@aux
        iqa_channelize_mfma_multi@compute iqa_channelize@aux iqa_channelize_mfma_multi@aux iqa_mean_power_batch@aux
        iqa_raw_level@aux iqa_trickle_copy@egress iqa_demodulate@compute iqa_resample@compute
    """.split(),
    "two_resident_collects": """
        iqa_trickle_copy@egress
    """.split(),
    "sign_redo_submit": """
        iqa_channelize_mfma_multi@compute iqa_mean_power_batch@compute iqa_raw_level@compute iqa_channelize@compute
        iqa_channelize_mfma_multi@compute iqa_channelize@compute iqa_demodulate@compute iqa_resample@compute
    """.split(),
    "sign_redo_collect": """
        iqa_trickle_copy@egress iqa_channelize@compute iqa_channelize_mfma_multi@compute iqa_channelize@compute
        iqa_demodulate_from_reset@compute iqa_resample@compute iqa_trickle_copy@egress
    """.split(),
    "captured_first": """
        iqa_channelize_mfma_multi@compute iqa_mean_power_batch@compute iqa_raw_level@compute iqa_channelize@compute
        iqa_channelize_mfma_multi@compute iqa_channelize@compute iqa_demodulate@compute iqa_resample@compute
        iqa_trickle_copy@egress iqa_channelize_mfma_multi@other iqa_mean_power_batch@other iqa_raw_level@other
        iqa_channelize@other iqa_channelize_mfma_multi@other iqa_channelize@other iqa_demodulate_from_reset@other
        iqa_resample@other iqa_trickle_copy@other
    """.split(),
    "captured_second_slot": """
        iqa_channelize_mfma_multi@compute iqa_mean_power_batch@compute iqa_raw_level@compute iqa_channelize@compute
        iqa_channelize_mfma_multi@compute iqa_channelize@compute iqa_demodulate@compute iqa_resample@compute
        iqa_trickle_copy@egress iqa_channelize_mfma_multi@other iqa_mean_power_batch@other iqa_raw_level@other
        iqa_channelize@other iqa_channelize_mfma_multi@other iqa_channelize@other iqa_demodulate_from_reset@other
        iqa_resample@other iqa_trickle_copy@other
    """.split(),
    "captured_replay": [],
    "bank_submit": """
        iqa_channelize_mfma_multi@compute iqa_mfma_combine@compute iqa_mfma_combine@compute iqa_mfma_combine@compute
        iqa_mfma_combine@compute iqa_mean_power_batch@compute iqa_raw_level@compute iqa_channelize@compute
        iqa_channelize@compute iqa_channelize@compute iqa_channelize@compute iqa_channelize_mfma_multi@compute
        iqa_mfma_combine@compute iqa_channelize@compute iqa_channelize_mfma@compute iqa_channelize_mfma@compute
        iqa_channelize_mfma@compute iqa_channelize_mfma@compute iqa_channelize_mfma@compute iqa_channelize_mfma@compute
        iqa_channelize_mfma@compute iqa_channelize_mfma@compute iqa_channelize_mfma@compute iqa_channelize_mfma@compute
        iqa_channelize@compute iqa_demodulate@tail iqa_resample@tail iqa_demodulate@tail iqa_resample@tail
        iqa_demodulate@tail iqa_resample@tail
    """.split(),
    "bank_collect": [],
    "bank_redone": {'sign': 0, 'precision': 0},
    "pipeline_f32": """
        iqa_f32_split_s16@compute iqa_channelize@compute iqa_channelize_mfma_multi@compute iqa_channelize@compute
        iqa_f32_split_s16@compute iqa_channelize@compute iqa_channelize_mfma_multi@compute iqa_channelize@compute
        iqa_channelize@compute iqa_channelize_mfma_multi@compute iqa_channelize@compute iqa_f32_split_s16@compute
        iqa_channelize@compute iqa_channelize_mfma_multi@compute iqa_channelize@compute iqa_channelize@compute
        iqa_channelize_mfma_multi@compute iqa_channelize@compute iqa_f32_split_s16@compute iqa_channelize@compute
    """.split(),
}


def _check(got: dict) -> None:
    for key, seq in got.items():
        assert seq == EXPECTED[key], key


def test_capture_runner_submit_and_collect(A, captures, trace):
    _check(scenario_submit_collect(A, captures, trace))


def test_capture_runner_two_resident_captures_in_flight(A, captures, trace):
    _check(scenario_two_resident_in_flight(A, captures, trace))


def test_capture_runner_redoes_a_capture_on_the_other_side(A, captures, trace):
    _check(scenario_sign_redo(A, captures, trace))


def test_capture_runner_captured_step_and_replay(A, captures, trace):
    got = scenario_captured(A, captures, trace)
    assert got["captured_replay"] == []  # a replay is one graph launch: no native call
    _check(got)


def test_bank_runner_submit_and_collect(A, captures, trace):
    _check(scenario_bank(A, captures, trace))


def test_pipeline_float32_planes_block_by_block(A, tmp_path, trace):
    _check(scenario_pipeline_f32(A, tmp_path, trace))
