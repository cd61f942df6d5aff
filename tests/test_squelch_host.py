"""Squelch post-processing (--audio-post): the host-side parts, no GPU needed -- audio WAV I/O, percentile planning,
target gathering, summary aggregates, configuration and CLI validation, and the C ABI's argument checks."""
from __future__ import annotations

import ctypes
import struct
from pathlib import Path

import numpy as np
import pytest

import iq_to_audio_amd as A
import iq_to_audio_amd.squelch as S
from iq_to_audio_amd import cli, iqio

SUBTYPES = ["PCM_U8", "PCM_16", "PCM_24", "PCM_32", "FLOAT"]


@pytest.mark.parametrize("subtype", SUBTYPES)
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_wav_audio_round_trip(tmp_path, subtype, channels):
    rng = np.random.default_rng(channels)
    x = rng.uniform(-1.0, 1.0, (1001, channels)).astype(np.float32)
    x[0] = 1.0
    x[1] = -1.0
    p = tmp_path / "a.wav"
    iqio.write_wav_audio(p, x, 22050, subtype)
    y, rate, sub = iqio.read_wav_audio(p)
    assert (rate, sub, y.shape, y.dtype) == (22050, subtype, x.shape, np.float32)
    if subtype == "FLOAT":
        assert np.array_equal(y, x)
    else:
        bits = iqio.AUDIO_SUBTYPE_BITS[subtype]
        step = 2.0 / (1 << (bits - 1))  # write scale 2^(b-1) - 1, read scale 2^(b-1) (libsndfile's pair)
        assert np.max(np.abs(y - x)) <= step
        # and once more through the writer
        iqio.write_wav_audio(p, y, 22050, subtype)
        y2 = iqio.read_wav_audio(p)[0]
        assert np.max(np.abs(y2 - y)) <= step


def test_wav_audio_reader_normalisation(tmp_path):
    """libsndfile's read normalisation: x / 2^(bits-1), U8 (x-128)/128."""
    def wav(tag, bits, payload, channels=1):
        block = channels * bits // 8
        hdr = b"RIFF" + struct.pack("<I", 36 + len(payload)) + b"WAVE" + b"fmt " + struct.pack(
            "<IHHIIHH", 16, tag, channels, 8000, 8000 * block, block, bits) + b"data" + struct.pack("<I", len(payload))
        p = tmp_path / f"n{tag}_{bits}.wav"
        p.write_bytes(hdr + payload)
        return iqio.read_wav_audio(p)

    y, _, sub = wav(1, 16, np.array([-32768, 16384, 32767], "<i2").tobytes())
    assert sub == "PCM_16" and y[:, 0].tolist() == [-1.0, 0.5, np.float32(32767 / 32768)]
    y, _, sub = wav(1, 8, bytes([0, 128, 255]))
    assert sub == "PCM_U8" and y[:, 0].tolist() == [-1.0, 0.0, np.float32(127 / 128)]
    y, _, sub = wav(1, 24, bytes([0, 0, 0x80, 0, 0, 0x40]))
    assert sub == "PCM_24" and y[:, 0].tolist() == [-1.0, 0.5]
    y, _, sub = wav(1, 32, np.array([-(1 << 31), 1 << 30], "<i4").tobytes())
    assert sub == "PCM_32" and y[:, 0].tolist() == [-1.0, 0.5]
    with pytest.raises(ValueError):
        wav(3, 64, bytes(16))


@pytest.mark.parametrize("n", [1, 2, 7, 144_000, 2_880_000, 1_234_567])
@pytest.mark.parametrize("pct", [0.0, 5.0, 20.0, 37.3, 95.0, 100.0])
def test_percentile_plan_reproduces_numpy(n, pct):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * 30 - 60).astype(np.float32)
    xs = np.sort(x)
    lo, hi, g = S.percentile_plan(n, pct)
    a, b = xs[lo], xs[hi]
    d = b - a
    got = (b - d * (np.float32(1) - g)) if g >= 0.5 else (a + d * g)  # numpy's float32 _lerp, as the kernel does it
    want = np.percentile(x, pct)
    assert got == want and got.dtype == want.dtype


def test_output_path_and_target_gathering(tmp_path):
    cfg = S.SquelchConfig()
    for name in ["b.wav", "a.WAV", "c.flac", "d.ogg", "e.mp3", "f.txt", "g.wav.bak"]:
        (tmp_path / name).write_bytes(b"")
    (tmp_path / "sub.wav").mkdir()
    opts = S.AudioPostOptions(config=cfg)
    got = [p.name for p in S.gather_audio_targets(tmp_path, opts)]
    assert got == ["a.WAV", "b.wav", "c.flac", "d.ogg", "e.mp3"]
    assert S.gather_audio_targets(tmp_path / "f.txt", opts) == []
    assert [p.name for p in S.gather_audio_targets(tmp_path / "b.wav", opts)] == ["b.wav"]
    with pytest.raises(FileNotFoundError):
        S.gather_audio_targets(tmp_path / "nope", opts)
    p = Path("/x/rec_1.wav")
    assert S._derive_output_path(p, opts) == Path("/x/rec_1-cleaned.wav")
    assert S._derive_output_path(p, S.AudioPostOptions(config=cfg, cleaned_suffix="")) == Path("/x/rec_1-cleaned.wav")
    assert S._derive_output_path(p, S.AudioPostOptions(config=cfg, cleaned_suffix="_sq")) == Path("/x/rec_1_sq.wav")
    assert S._derive_output_path(p, S.AudioPostOptions(config=cfg, overwrite=True)) == p


def test_non_wav_files_fail_alone_with_a_clear_error(tmp_path):
    (tmp_path / "a.flac").write_bytes(b"fLaC")
    (tmp_path / "b.wav").write_bytes(b"not a wav")
    calls = []
    summary = S.process_audio_batch(S.gather_audio_targets(tmp_path, S.AudioPostOptions(config=S.SquelchConfig())),
                                    S.AudioPostOptions(config=S.SquelchConfig()),
                                    progress_cb=lambda a, b, p: calls.append((a, b, p.name)))
    assert (summary.processed, summary.failed, summary.total) == (0, 2, 2)
    assert "needs libsndfile" in str(summary.errors[0][1])
    assert isinstance(summary.errors[1][1], ValueError)
    assert calls == [(0, 2, "a.flac"), (1, 2, "b.wav")]  # only the "before" call of a failed file


def test_summary_aggregates_and_config_validation():
    def res(din, dout, bin_, bout):
        return S.SquelchFileResult(Path("i"), Path("o"), 0, 0, din, dout, bin_, bout, -50.0, -44.0, "adaptive", 0.5)

    s = S.SquelchSummary(results=[res(10.0, 4.0, 1000, 400), res(5.0, 5.0, 300, 320)], errors=[(Path("x"), ValueError())])
    assert (s.processed, s.failed, s.total) == (2, 1, 3)
    assert s.aggregate_duration_delta() == pytest.approx(-6.0)
    assert s.aggregate_size_delta() == -580
    cfg = S.SquelchConfig()
    assert (cfg.method, cfg.noise_floor_percentile, cfg.hold_seconds, cfg.trim_trail_seconds) == ("adaptive", 0.2, 0.12, 0.35)
    with pytest.raises(ValueError, match="manual_noise_floor_db"):
        S.SquelchConfig(auto_noise_floor=False).validate()
    with pytest.raises(ValueError, match="Unsupported squelch method"):
        S.SquelchConfig(method="loud").validate()
    S.SquelchConfig(auto_noise_floor=False, manual_noise_floor_db=-40.0).validate()
    with pytest.raises(ValueError, match="shorter"):
        S._windows(1919, 48000.0, cfg)
    assert S._windows(1920, 48000.0, cfg)["window"] == 1920
    with pytest.raises(ValueError):
        S._windows(2303, 48000.0, S.SquelchConfig(method="transient"))  # long window = 4 * 576
    w = S._windows(48000, 48000.0, cfg)
    assert (w["hold"], w["fade"], w["lead"], w["trail"]) == (5760, 480, 7200, 16800)


def test_cli_audio_post_flags_and_validation(tmp_path):
    p = cli.build_parser()
    args = p.parse_args(["--audio-post", "x"])
    assert (args.audio_post_path, args.audio_post_mode, args.audio_post_noise_floor, args.audio_post_percentile,
            args.audio_post_threshold, args.audio_post_lead, args.audio_post_trail, args.audio_post_trim,
            args.audio_post_overwrite, args.audio_post_suffix) == (Path("x"), "adaptive", None, 0.2, 6.0, 0.15, 0.35, True,
                                                                 False, "-cleaned")
    args = p.parse_args(["--audio-post", "x", "--audio-post-no-trim", "--audio-post-overwrite", "--audio-post-mode",
                         "transient", "--audio-post-noise-floor", "-50", "--audio-post-suffix", "_q"])
    assert (args.audio_post_trim, args.audio_post_overwrite, args.audio_post_mode, args.audio_post_noise_floor,
            args.audio_post_suffix) == (False, True, "transient", -50.0, "_q")
    with pytest.raises(SystemExit) as e:
        cli.main(["--audio-post", str(tmp_path), "--benchmark"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        cli.main(["--audio-post", str(tmp_path), "--audio-post-noise-percentile", "1.5"])
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        p.parse_args(["--audio-post", "x", "--audio-post-mode", "loud"])
    # no --in / --ft needed; an empty directory and a missing path are exit code 1
    assert cli.main(["--audio-post", str(tmp_path)]) == 1
    assert cli.main(["--audio-post", str(tmp_path / "missing")]) == 1


def _seg(**kw):
    seg = A.native.SquelchSeg(n=4096, in_off=0, base=0, channels=1, window=64, short_window=8, long_window=64, hold=10,
                              fade=4, lead=0, trail=0)
    for k, v in kw.items():
        setattr(seg, k, v)
    return seg


@pytest.mark.parametrize("bad", [dict(n=10), dict(channels=0), dict(window=0), dict(base=100), dict(fade=-1),
                                 dict(q_index=(ctypes.c_int64 * 6)(0, 0, 0, 0, 0, 4096))])
def test_squelch_abi_rejects_bad_arguments_before_any_launch(bad):
    A.native.build()
    lib = A.native.lib()
    assert lib.iqa_squelch_workspace_bytes(4096, 1) > 4096 * 40
    assert lib.iqa_squelch_workspace_bytes(1000, 1) == -1
    assert lib.iqa_squelch_stage_offset(4096, 1, 2) > 0 and lib.iqa_squelch_stage_offset(4096, 1, 9) == -1
    params = A.native.SquelchParams(method=0, auto_floor=1, trim=1)
    seg = _seg(**bad)
    fake = ctypes.c_void_p(16)  # never dereferenced: the checks come first
    with pytest.raises(ValueError):
        A.native.call("iqa_squelch", ctypes.byref(params), ctypes.byref(seg), 1, fake, fake, fake, fake, fake,
                      ctypes.c_int64(1 << 30), ctypes.c_void_p(0))
    bad_method = A.native.SquelchParams(method=7)
    with pytest.raises(ValueError, match="method"):
        A.native.call("iqa_squelch", ctypes.byref(bad_method), ctypes.byref(_seg()), 1, fake, fake, fake, fake, fake,
                      ctypes.c_int64(1 << 30), ctypes.c_void_p(0))
    with pytest.raises(ValueError, match="workspace"):
        A.native.call("iqa_squelch", ctypes.byref(params), ctypes.byref(_seg()), 1, fake, fake, fake, fake, fake,
                      ctypes.c_int64(16), ctypes.c_void_p(0))
