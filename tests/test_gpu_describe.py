"""The channel description (--find-describe) on the MI355X, on the model capture of
tests/describe_model.py (thirteen channels of known modulation, s16): the eight sums of every channel equal the numpy oracle's,
applied to the GPU's own channelizer output; the labels are the host test's; the figures agree with the oracle's float64
channelizer; cuts of a channel stream into calls (single samples, cuts inside a tile) change no bit; reset; the CLI end to end:
--find-describe beside --find-channels, --find-auto against explicit runs, and the proof that a run without the flags calls no
entry point of the description."""
from __future__ import annotations

import dataclasses
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np
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


M = _load("describe_model")
FM = M.FM
FS = M.FS
FC = 455.5e6
FIGURES = ("cnr_db", "env", "depth", "carrier_hz", "dev_hz", "line_share")


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _blocks(raw):
    from iq_to_audio_amd import find as FD

    flat = raw.reshape(-1)
    for a in range(0, raw.shape[0], FD.BLOCK_FRAMES):  # the blocks find_channels hands over
        yield flat[2 * a : 2 * min(raw.shape[0], a + FD.BLOCK_FRAMES)]


@pytest.fixture(scope="module")
def gpu(A):
    """The model capture through the finder and the describer, once: everything the tests below read."""
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd import find as FD

    raw = M.capture()
    plan = P.plan_find(FS, raw.shape[0])
    finder = A.ChannelFinder(plan, "s16")
    for block in _blocks(raw):
        finder.process(block)
    fin = finder.finish()
    found = finder.result(FC)
    describer = A.ChannelDescriber(plan, fin, found.channels, "s16", "iq", keep_stages=True)
    for block in _blocks(raw):
        describer.process(block)
    return dict(raw=raw, plan=plan, fin=fin, found=found, describer=describer, stages=describer.stages(), result=describer.result(FC),
                first_block=min(raw.shape[0], FD.BLOCK_FRAMES))


def _find_args(plan):
    return dict(hop=plan.hop, T=plan.slice_frames, F=plan.frames)


def test_sums_are_the_oracles(A, gpu):
    plan, fin, found = gpu["plan"], gpu["fin"], gpu["found"]
    assert len(found.channels) == len(M.CHANNELS) == len(gpu["stages"])
    runs = {int(r[0]): j for j, r in enumerate(fin["runs"].tolist())}
    for (name, offset, _), ch, st in zip(M.CHANNELS, found.channels, gpu["stages"]):
        assert abs(ch.offset_hz - offset) <= (3000.0 if name in ("wfm", "usb") else 2 * plan.bin_hz), (name, ch.offset_hz)
        dp = M.plan(FS, ch.offset_hz, ch.width_hz)
        assert (st["plan"].decimation, st["plan"].delay, st["plan"].fs_ch, st["plan"].bw) == (dp["D"], dp["delay"], dp["fs_ch"], dp["bw"])
        z = st["z"]
        assert z.dtype == np.complex64 and z.size == -(-gpu["raw"].shape[0] // dp["D"])
        gate = M.erode(fin["on"][runs[ch.lo_bin]])
        np.testing.assert_array_equal(st["gate"], gate)
        # sh comes from the first block's outputs; the mean power is a float64 sum in another order: not at an edge of ceil
        head = z[: -(-gpu["first_block"] // dp["D"])]
        assert st["sh"] in {M.choose_shift(head * np.float32(k)) for k in (1.0 - 1e-6, 1.0, 1.0 + 1e-6)}, name
        want = M.stream_sums(z, st["sh"], gate, D=dp["D"], delay=dp["delay"], **_find_args(plan))
        print(name, "sh", st["sh"], "D", dp["D"], dict(zip(M.SUMS, want)))
        assert want[0] >= 1024 and st["sums"] == want, name
        assert st["rows"].shape[1] == 8 and M.add_rows(st["rows"]) == want


def test_labels_and_figures(A, gpu):
    got = gpu["result"]
    assert isinstance(got, A.DescribeResult) and (got.sample_rate, got.center_freq) == (FS, FC)
    assert {name: d.label for name, d in zip(M.NAMES, got.channels)} == M.LABELS
    # against the oracle's float64 channelizer, on the GPU finder's own runs where they differ from the oracle's
    ref = M.model_run()
    plan, fin = gpu["plan"], gpu["fin"]
    if not (np.array_equal(ref["st"]["runs"], fin["runs"]) and np.array_equal(ref["st"]["on"], fin["on"])
            and np.array_equal(ref["st"]["slice"], fin["slice"]) and np.array_equal(ref["st"]["fmean"], fin["fmean"])):
        print("the GPU's rows give other planes than numpy's: the oracle's channelizer runs on the GPU finder's result")
        p = FM.plan(FS, gpu["raw"].shape[0])
        found = [dataclasses.asdict(ch) for ch in gpu["found"].channels]
        x = FM.to_complex(gpu["raw"])
        described = M.describe_run(p, fin, found, lambda j, dp: M.channelize(x, FS, dp["offset_hz"], dp["taps"], dp["D"]), FC, gpu["first_block"])
    else:
        described = ref["described"]
    worst = dict.fromkeys(FIGURES, 0.0)
    for name, d, want in zip(M.NAMES, got.channels, described):
        for key in FIGURES:
            a, b = getattr(d, key), want[key]
            # 2 % or 2 Hz; the figures without a unit: 2 % or 0.002, a tenth of the smallest threshold they are held against
            floor = 2.0 if key.endswith("_hz") else 0.002
            worst[key] = max(worst[key], abs(a - b) / max(0.02 * abs(b), floor))
            print(name, key, a, b)
            assert abs(a - b) <= max(0.02 * abs(b), floor), (name, key, a, b)
    print("worst share of the bound", worst)
    for d, ch in zip(got.channels, gpu["found"].channels):
        assert (d.offset_hz, d.freq_hz, d.width_hz) == (ch.offset_hz, ch.freq_hz, ch.width_hz)
        assert (d.demod is None) == (d.label == "unknown") and (d.tuned_hz is None) == (d.demod is None)
    by = dict(zip(M.NAMES, got.channels))
    assert abs(by["carrier"].carrier_hz) < 1.0  # the mixer's sign: the tone rests at 0 Hz
    assert (by["usb"].demod, by["usb"].bw) == ("usb", 3000.0) and by["usb"].tuned_offset_hz < -50e3
    assert (by["fsk"].demod, by["fsk"].bw) == ("nfm", 25000.0) and (by["wfm"].demod, by["wfm"].bw) == ("wfm", 250000.0)
    assert (by["am_tone"].demod, by["am_tone"].bw) == ("am", 10000.0) and by["nfm_faint"].demod is None


def test_cuts_of_a_stream_change_no_bit(A, gpu):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.describe import add_rows

    describer = A.ChannelDescriber(gpu["plan"], gpu["fin"], gpu["found"].channels, "s16", "iq")
    lanes = describer.lanes()
    for j in (1, 3, 6):  # the carrier, the burst, the upper sideband: 24 000, 47 059 and 30 380 samples
        z = D.from_numpy(gpu["stages"][j]["z"])
        lane = lanes[j]
        lane.sh = gpu["stages"][j]["sh"]
        at = 0
        for n in [1, 1, 2046, 2048, 2049, 1000, 1, 7, 4096 + 3, 1, 1 << 30]:  # single samples, cuts inside a tile and at its edges
            n = min(n, int(z.numel()) - at)
            describer.feed(lane, z[at : at + n])
            at += n
        assert at == int(z.numel()) and lane.pos == at and len(lane.rows) == 11
        assert add_rows(D.torch_mod().cat(lane.rows).cpu().numpy()) == gpu["stages"][j]["sums"], j


def test_reset_starts_a_new_run(A, gpu):
    describer = gpu["describer"]
    first = [st["sums"] for st in gpu["stages"]]
    describer.reset()
    assert describer.samples_seen == 0
    describer.process(gpu["raw"][:300_000].reshape(-1))  # part of a run, thrown away
    with pytest.raises(ValueError, match="stream held"):
        describer.finish()
    describer.reset()
    for block in _blocks(gpu["raw"]):
        describer.process(block)
    assert describer.finish() == first
    with pytest.raises(ValueError, match="longer"):
        describer.process(gpu["raw"][:1].reshape(-1))


# ---- the command line --------------------------------------------------------------------------------------------------------


def _count_calls(monkeypatch):
    from iq_to_audio_amd import _native

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith("iqa_describe_"):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    return calls


def test_end_to_end(A, gpu, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import cli, iqio

    calls = _count_calls(monkeypatch)
    dirs = {}
    for tag in ("find", "describe", "auto", "ft"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
        iqio.write_wav_iq(dirs[tag] / "model_455500000Hz.wav", gpu["raw"], int(FS), "s16")
    # a plain --find-channels run calls no entry point of the description
    assert cli.main(["--in", str(dirs["find"] / "model_455500000Hz.wav"), "--find-channels"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert calls == [] and len(plain) == 13 and not list(dirs["find"].glob("*.describe.json"))
    # --find-describe: the same channel lines with an indented line under each, the same channels.json, and describe.json
    assert cli.main(["--in", str(dirs["describe"] / "model_455500000Hz.wav"), "--find-describe"]) == 0
    printed = capsys.readouterr().out.splitlines()
    assert set(calls) == {"iqa_describe_accumulate"} and len(calls) >= 13
    assert printed[0::2] == plain and printed[1::2] == gpu["result"].lines() and all(line.startswith("    ") for line in printed[1::2])
    name = "model_455500000Hz.channels.json"
    assert (dirs["describe"] / name).read_bytes() == (dirs["find"] / name).read_bytes()
    stored = A.DescribeResult.from_json(json.loads((dirs["describe"] / "model_455500000Hz.describe.json").read_text()))
    assert stored == gpu["result"]
    res, des = A.find_channels(dirs["describe"] / "model_455500000Hz.wav", describe=True)
    assert res == gpu["found"] and des == gpu["result"]
    # --find-top 3 --find-auto against three explicit runs with the suggested frequency, mode and bandwidth
    from iq_to_audio_amd.describe import select_auto_targets

    targets, skipped = select_auto_targets(res, des, 3, 12500.0)
    # the two strongest are the NFM channels at -700 and +300 kHz; the two AM channels at +100 and +550 kHz tie for the third
    assert len(targets) == 3 and skipped == [] and {(-700e3, "nfm", 12500.0), (300e3, "nfm", 12500.0)} < {(f - FC, d, b) for f, d, b in targets}
    assert [(f - FC, d, b) for f, d, b in targets if d != "nfm"] in ([(100e3, "am", 10000.0)], [(550e3, "am", 10000.0)])
    del calls[:]
    assert cli.main(["--in", str(dirs["auto"] / "model_455500000Hz.wav"), "--find-top", "3", "--find-auto", "--find-grid", "12500"]) == 0
    assert calls
    names = [f"audio_{int(f)}_48k.wav" for f, _, _ in targets]
    assert sorted(p.name for p in dirs["auto"].glob("audio_*")) == sorted(names)
    for (freq, demod, bw), wav in zip(targets, names):
        assert cli.main(["--in", str(dirs["ft"] / "model_455500000Hz.wav"), "--ft", f"{freq:.0f}", "--demod", demod, "--bw", f"{bw:.0f}"]) == 0
        a, b = (dirs["auto"] / wav).read_bytes(), (dirs["ft"] / wav).read_bytes()
        assert len(a) > 100_000 and a == b, wav
