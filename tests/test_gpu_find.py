"""The channel finder (--find-channels) on the MI355X: for s16, u8 and f32 encodings of the model capture
every integer stage equals the numpy oracle of tests/find_model.py from the GPU's own float32 rows, and so does the result;
block cuts change no bit; a list too short is repeated, never used; reset; the CLI end to end, --find-top against the same
run with --ft, and the proof that a run without the flags calls no entry point of the finder."""
from __future__ import annotations

import dataclasses
import importlib.util
import json
import sys
from ctypes import c_int32, c_int64
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


M = _load("find_model")
FS = 2.4e6
FC = 455.5e6
STAGES = ("sum", "max", "slice", "mean", "fmean", "fmax", "x", "mask", "runs", "on")


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


@pytest.fixture(scope="module")
def raw16():
    return M.capture(FS, 2.0, 3)


@pytest.fixture(scope="module")
def short16(raw16):
    """The first 0.25 s of the model capture (the three steady channels; 145 frames), for the tests that run it several times."""
    return raw16[:600_000]


def _finder(A, raw, fmt="s16", cuts=None, **kwargs):
    from iq_to_audio_amd import dsp_plan as P

    plan = P.plan_find(FS, raw.shape[0])
    finder = A.ChannelFinder(plan, fmt, keep_stages=True, **kwargs)
    flat = raw.reshape(-1)
    at = 0
    for n in list(cuts or []) + [raw.shape[0]]:
        n = min(n, raw.shape[0] - at)
        finder.process(flat[2 * at : 2 * (at + n)])
        at += n
    assert at == raw.shape[0]
    return plan, finder


def _same(a: dict, b: dict, keys=STAGES + ("c",)):
    for key in keys:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["candidates"] == b["candidates"]


@pytest.mark.parametrize("fmt", ["s16", "u8", "f32"])
def test_stages_are_the_oracles(A, raw16, fmt):
    raw = M.encode(raw16, fmt)
    plan, finder = _finder(A, raw, fmt)
    st = finder.stages()
    p = M.plan(FS, raw.shape[0])
    assert st["rows"].dtype == np.float32 and st["rows"].shape == (p["F"], p["nfft"]) == (1170, 8192)
    want = M.run(st["rows"], p)  # from the GPU's own rows
    assert len(want["runs"]) == 4 and want["candidates"] >= 4 and want["on"].any() and (want["mask"] & 1).sum() > 300
    _same(st, want)
    res = finder.result(FC)
    want_res = M.result(p, want["runs"], want["on"], want["mean"], FC)
    assert [dataclasses.asdict(ch) for ch in res.channels] == want_res
    assert (res.sample_rate, res.center_freq, res.seconds, res.nfft, res.bin_hz, res.frames, res.slice_frames, res.slices, res.threshold_db,
            res.peak_threshold_db, res.candidates) == (FS, FC, 2.0, 8192, FS / 8192, 1170, 5, 234, 6.0, 10.0, want["candidates"])
    print(fmt, "runs", want["runs"][:, :2].tolist(), "offsets", [round(d["offset_hz"], 1) for d in want_res], "duty",
          [round(d["duty"], 4) for d in want_res], "snr", [d["snr_db"] for d in want_res])
    M.check_four_channels(p, want_res)
    if fmt == "s16":
        # the rows against numpy's FFT: both are float64 to ~1e-9 dB, so the float32 rows are at most an ulp (< 2e-5 dB) and
        # the centi-dB values at most one step apart
        dc = np.abs(st["c"].astype(np.int32) - M.quantise(M.rows(raw, p)).astype(np.int32))
        print("c against numpy's rows: max |dc|", int(dc.max()), "differing", int(np.count_nonzero(dc)), "of", dc.size)
        assert dc.max() <= 1


def test_block_cuts_change_no_bit(A, short16):
    plan, whole = _finder(A, short16)
    assert (plan.nfft, plan.frames, plan.slices) == (8192, 145, 145)
    a = whole.stages()
    assert len(a["runs"]) == 3 and a["on"].all()
    cuts = [1, 100, 8191, 8192, 4095, 1, 50_001, 3, 123_457, 4096, 2]  # blocks shorter than nfft, single frames, odd sizes
    _, cut = _finder(A, short16, cuts=cuts)
    _same(a, cut.stages())
    # device tensors are taken as they are
    from iq_to_audio_amd import _dev as D

    _, dev = _finder(A, short16, cuts=[])
    dev.reset()
    dev.process(D.to_device(short16.reshape(-1), "int16"))
    _same(a, dev.stages())
    # a stream that ends early or runs on is refused
    _, early = _finder(A, short16[:500_000], cuts=[])
    early.plan = plan
    with pytest.raises(ValueError, match="frames"):
        early.finish()
    with pytest.raises(ValueError, match="longer"):
        whole.process(short16[:1].reshape(-1))


def test_short_list_is_repeated_not_used(A, short16):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    plan, roomy = _finder(A, short16)
    _, tight = _finder(A, short16)
    a, b = roomy.finish(), tight.finish(capacity=1)
    assert len(a["runs"]) == 3
    _same(a, b, STAGES)
    # the entry itself with room for one: the full counts, and nothing behind entry 0
    planes = [D.from_numpy(np.ascontiguousarray(a[key])) for key in ("mean", "fmean", "max", "fmax", "mask")]  # (held until the call is queued)
    lst = D.from_numpy(np.full(3 * 8, -7, dtype=np.int64))
    counts = D.from_numpy(np.array([99, 99], dtype=np.int64))
    N.call("iqa_find_runs", *(N.ptr(t) for t in planes),
           c_int32(plan.nfft), c_int32(plan.min_hot), N.ptr(lst), c_int64(1), N.ptr(counts), N.stream_ptr())
    got = lst.cpu().numpy().reshape(3, 8)
    assert counts.cpu().numpy().tolist() == [3, a["candidates"]]
    assert got[0].tolist() in a["runs"].tolist() and (got[1:] == -7).all()


def test_reset_starts_a_new_run(A, short16):
    plan, finder = _finder(A, short16)
    first = finder.stages()
    finder.reset()
    assert finder.frames_done == 0 and finder.samples_seen == 0
    finder.process(short16[:300_000].reshape(-1))  # half a run, thrown away
    finder.reset()
    finder.process(short16.reshape(-1))
    _same(first, finder.stages())
    # another capture through the same object: noise alone
    noise = M.capture(FS, 0.25, 11, carriers=False)
    finder.reset()
    finder.process(noise.reshape(-1))
    st = finder.stages()
    want = M.run(st["rows"], M.plan(FS, noise.shape[0]))
    _same(st, want)
    assert len(st["runs"]) == 0 and finder.result(FC).lines() == ["no channel found"]


# ---- the command line -----------------------------------------------------------------------------------------------------


def _count_calls(monkeypatch, prefix="iqa_find_"):
    from iq_to_audio_amd import _native

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith(prefix):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    return calls


def test_end_to_end(A, raw16, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import cli, iqio
    from iq_to_audio_amd.find import FindResult

    calls = _count_calls(monkeypatch)
    dirs = {}
    for tag in ("find", "top", "ft"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
        iqio.write_wav_iq(dirs[tag] / "model_455500000Hz.wav", raw16, int(FS), "s16")
    wav = dirs["find"] / "model_455500000Hz.wav"
    # the API, then the same through the CLI
    res = A.find_channels(wav)
    assert res.center_freq == FC and len(res.channels) == 4
    M.check_four_channels(M.plan(FS, raw16.shape[0]), [dataclasses.asdict(ch) for ch in res.channels])
    assert all(ch.freq_hz == FC + ch.offset_hz for ch in res.channels)
    capsys.readouterr()
    assert cli.main(["--in", str(wav), "--find-channels"]) == 0
    printed = capsys.readouterr().out.splitlines()
    assert printed == res.lines() and len(printed) == 4
    assert printed[2].startswith("455800000 Hz: ") and printed[0].endswith("(0.49 .. 0.70 s)")
    js = wav.with_name("model_455500000Hz.channels.json")
    assert FindResult.from_json(json.loads(js.read_text())) == res
    assert not list(dirs["find"].glob("audio_*"))  # nothing was demodulated
    assert set(calls) == {"iqa_find_accumulate", "iqa_find_mean", "iqa_find_floor", "iqa_find_mask", "iqa_find_runs", "iqa_find_activity"}
    # the threshold reaches the plan, and offsets stand in where there is no centre frequency
    assert cli.main(["--in", str(wav), "--find-channels", "--find-threshold", "30"]) == 0
    strict = A.find_channels(wav, threshold_db=30.0)
    assert capsys.readouterr().out.splitlines() == strict.lines() and json.loads(js.read_text())["threshold_db"] == 30.0
    assert strict.threshold_db == 30.0 and len(strict.channels) >= 3
    bare = dirs["find"] / "bare.wav"
    iqio.write_wav_iq(bare, raw16[:600_000], int(FS), "s16")
    assert cli.main(["--in", str(bare), "--find-channels"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert all(line[0] in "+-" for line in lines)
    assert [round(float(line.split(" Hz")[0]) / 2e3) for line in lines] == [-100, 150, 400]
    # --find-top against the same run with --ft
    del calls[:]
    assert cli.main(["--in", str(dirs["ft"] / "model_455500000Hz.wav"), "--demod", "nfm", "--ft", "455800000", "--ft", "456300000"]) == 0
    assert calls == []  # a run without the flags calls no entry point of the finder
    assert not list(dirs["ft"].glob("*.channels.json"))
    assert cli.main(["--in", str(dirs["top"] / "model_455500000Hz.wav"), "--demod", "nfm", "--find-top", "2", "--find-grid", "12500"]) == 0
    assert calls
    for name in ("audio_455800000_48k.wav", "audio_456300000_48k.wav"):
        a, b = (dirs["top"] / name).read_bytes(), (dirs["ft"] / name).read_bytes()
        assert len(a) > 100_000 and a == b, name
    assert sorted(p.name for p in dirs["top"].glob("audio_*")) == ["audio_455800000_48k.wav", "audio_456300000_48k.wav"]
    # nothing found: --find-top logs it and stops
    quiet = dirs["find"] / "quiet_455500000Hz.wav"
    iqio.write_wav_iq(quiet, M.capture(FS, 0.25, 11, carriers=False), int(FS), "s16")
    capsys.readouterr()
    assert cli.main(["--in", str(quiet), "--find-top", "3"]) == 0
    assert capsys.readouterr().out.splitlines() == ["no channel found"] and not list(dirs["find"].glob("audio_*"))
    # --find-top without a centre frequency is a processing error
    assert cli.main(["--in", str(bare), "--find-top", "1"]) == 1
