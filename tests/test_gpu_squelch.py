"""Squelch post-processing (--audio-post) on the MI355X: fixture parity with the reference, stage checks at full size,
batching, device input, the CLI.  Reads only tests/golden/squelch.npz and tests/golden/squelch_edges.npz (made by
tests/golden/gen_squelch.py)."""
from __future__ import annotations

import numpy as np
import pytest
import squelch_model as M

import iq_to_audio_amd.squelch as S
from iq_to_audio_amd import cli, iqio

pytestmark = pytest.mark.gpu


def _cases(golden, fixture):
    """PCM16 byte planes or, where the case says so, float32 input (M.fixture_cases)."""
    for name, x, rate, params, scalars, mask_bits, gain in M.fixture_cases(golden(fixture)):
        yield name, x, rate, S.SquelchConfig(**params), scalars, mask_bits, gain


def test_fixture_parity_with_the_reference(golden):
    for fixture, least in (("squelch.npz", 9), ("squelch_edges.npz", 12)):
        seen = _fixture_parity(golden, fixture)
        assert seen >= least and seen == len(golden(fixture)["cases"]), fixture


def _fixture_parity(golden, fixture):
    seen = 0
    for name, x, rate, cfg, scalars, mask_bits, gain in _cases(golden, fixture):
        y, floor_db, thr_db, st = S.apply_squelch(x, float(rate), cfg, return_stages=True)
        want_floor, want_thr, start, stop = scalars
        assert abs(floor_db - want_floor) <= 1e-4, (name, floor_db, want_floor)
        assert abs(thr_db - want_thr) <= 1e-4, (name, thr_db, want_thr)
        assert (st["start"], st["stop"]) == (int(start), int(stop)), name
        want = (x * gain[:, None])[int(start):int(stop)]
        assert y.dtype == np.float32 and y.shape == want.shape, (name, y.shape, want.shape)
        if y.size:
            assert float(np.max(np.abs(y - want))) <= 1e-6, name
        # the mask may only differ where the GPU's own level is within 1e-3 dB of its threshold
        n = x.shape[0]
        want_mask = np.unpackbits(mask_bits)[:n].astype(bool)
        got_mask = st["mask"].cpu().numpy()
        level = (st["level"] if cfg.method == "transient" else st["envelope_db"]).cpu().numpy()
        thr = st["threshold"].cpu().numpy()
        differ = got_mask != want_mask
        near = np.abs(level - thr) <= 1e-3
        assert not np.any(differ & ~near), (name, int(np.sum(differ & ~near)))
        print(f"{name}: {int(differ.sum())} mask samples differ (all within 1e-3 dB of the threshold)")
        assert int(differ.sum()) == 0, name
        seen += 1
    return seen


def _synthetic(rate=48000, secs=60.0, channels=2, seed=7):
    rng = np.random.default_rng(seed)
    n = int(rate * secs)
    x = rng.standard_normal((n, channels)).astype(np.float32) * np.float32(0.003)
    t = np.arange(n) / rate
    for k in range(40):  # bursts of varied length and level, some shorter than 128 samples
        a = int(rng.integers(0, n - 50_000))
        ln = int(rng.choice([60, 300, 5_000, 20_000, 48_000]))
        amp = float(rng.uniform(0.05, 0.6))
        x[a:a + ln] += (amp * np.sin(2 * np.pi * (300 + 50 * k) * t[a:a + ln]))[:, None].astype(np.float32)
    return x


def _percentile_f32(v, pct):
    return np.percentile(v.astype(np.float32), pct)


@pytest.mark.parametrize("method", ["adaptive", "static", "transient"])
def test_stages_at_full_size_against_numpy_on_the_previous_stage(method):
    rate = 48000
    x = _synthetic(rate)
    cfg = S.SquelchConfig(method=method)
    y, floor_db, thr_db, st = S.apply_squelch(x, float(rate), cfg, return_stages=True)
    env = st["envelope_db"].cpu().numpy()
    # noise floor: np.percentile of the GPU's envelope
    assert floor_db == float(_percentile_f32(env, float(np.clip(cfg.noise_floor_percentile, 0, 1)) * 100.0))
    assert thr_db == floor_db + cfg.threshold_margin_db
    # envelope: float64 box average of the channel mean |x| (np.convolve "same" centring)
    mag = np.mean(np.abs(x), axis=1, dtype=np.float64).astype(np.float32)
    w = st["window"]
    c = np.concatenate(([0.0], np.cumsum(mag, dtype=np.float64)))
    i = np.arange(x.shape[0])
    lo, hi = np.clip(i - w // 2, 0, x.shape[0]), np.clip(i - w // 2 + w, 0, x.shape[0])
    env_ref = np.maximum(-160.0, 20 * np.log10(np.maximum(((c[hi] - c[lo]) / w).astype(np.float32).astype(np.float64), 1e-10)))
    assert np.max(np.abs(env - env_ref.astype(np.float32))) < 1e-3
    mask = st["mask"].cpu().numpy()
    thr = st["threshold"].cpu().numpy()
    if method == "adaptive":
        level = st["level"].cpu().numpy()
        assert np.array_equal(level, env - np.minimum.accumulate(env))
        low, high = _percentile_f32(level, 5.0), _percentile_f32(level, 95.0)
        span = max(high - low, 1e-6)
        score = np.asarray((level - low) / span, dtype=np.float32)
        t32 = np.clip(thr_db + 6.0 * (1.0 - score), thr_db - 6.0, thr_db + 6.0)
        assert np.array_equal(thr, t32)
        assert np.array_equal(mask, env >= t32)
    elif method == "static":
        assert np.array_equal(mask, env >= thr_db)
    else:
        assert np.array_equal(mask, st["level"].cpu().numpy() >= cfg.transient_margin_db)
    assert mask.any() and not mask.all()
    # dilation: exact window counts with the reference's int8 wrap
    h = st["hold"]
    cm = np.concatenate(([0], np.cumsum(mask, dtype=np.int64)))
    n = mask.size
    tail = cm[i + 1] - cm[np.maximum(i - h, 0)]
    head = cm[np.minimum(i + h, n - 1) + 1] - cm[i]
    pos = lambda v: (v & 0xFF).astype(np.uint8).view(np.int8) > 0  # noqa: E731
    dil_ref = mask | pos(tail) | pos(head)
    dil = st["dilated"].cpu().numpy()
    assert np.array_equal(dil, dil_ref)
    # gain: the reference's fade kernel on the edge-padded dilated mask, clipped (float64, on the GPU's dilated mask)
    f = st["fade"]
    ramp = np.arange(f + 1) / f
    k = np.concatenate((ramp[:-1], [1.0], ramp[1:][::-1]))
    padded = np.pad(dil.astype(np.float64), f, mode="edge")
    g_ref = np.clip(np.convolve(padded, k, mode="same")[f:-f], 0, 1)
    gain = st["gain"].cpu().numpy()
    assert np.max(np.abs(gain - g_ref)) < 1e-6
    act = np.flatnonzero(gain > np.float32(1e-3))
    assert st["start"] == max(0, act[0] - int(round(rate * cfg.trim_lead_seconds)))
    assert st["stop"] == min(n, act[-1] + int(round(rate * cfg.trim_trail_seconds)) + 1)
    want = (x * gain[:, None])[st["start"]:st["stop"]]
    assert np.array_equal(y, want)


def _write(path, x, rate, subtype="PCM_16"):
    iqio.write_wav_audio(path, x, rate, subtype)
    return iqio.read_wav_audio(path)[0]


def test_batch_equals_file_by_file(tmp_path):
    cfg = S.SquelchConfig()
    files = []
    for k, (rate, secs, ch, sub) in enumerate([(48000, 7.0, 1, "PCM_16"), (11025, 5.0, 2, "PCM_16"), (22050, 3.3, 1, "FLOAT"),
                                                (48000, 9.1, 2, "PCM_16"), (16000, 4.0, 1, "PCM_24")]):
        x = _synthetic(rate, secs, ch, seed=k)
        p = tmp_path / f"f{k}.wav"
        _write(p, np.clip(x, -1, 1), rate, sub)
        files.append(p)
    (tmp_path / "broken.flac").write_bytes(b"fLaC")
    targets = S.gather_audio_targets(tmp_path, S.AudioPostOptions(config=cfg))
    assert len(targets) == 6
    calls = []
    one = S.process_audio_batch(targets, S.AudioPostOptions(config=cfg, cleaned_suffix="-batch"),
                                progress_cb=lambda a, b, p: calls.append((a, b, p.name)))
    assert one.processed == 5 and one.failed == 1 and "libsndfile" in str(one.errors[0][1])
    assert calls[:2] == [(0, 6, "broken.flac"), (1, 6, "f0.wav")]
    # small budget: one file per launch
    sep = S.process_audio_batch(targets, S.AudioPostOptions(config=cfg, cleaned_suffix="-sep"), batch_bytes_limit=1)
    assert sep.processed == 5
    for a, b in zip(one.results, sep.results):
        assert (a.samples_out, a.noise_floor_db, a.threshold_db) == (b.samples_out, b.noise_floor_db, b.threshold_db)
        assert a.output_path.read_bytes() == b.output_path.read_bytes()
        direct = S.process_audio_file(a.input_path, S.AudioPostOptions(config=cfg, cleaned_suffix="-one"))
        assert direct.output_path.read_bytes() == a.output_path.read_bytes()
        data, rate, sub = iqio.read_wav_audio(a.input_path)
        y, fl, th = S.apply_squelch(data, float(rate), cfg)
        assert fl == a.noise_floor_db and y.shape[0] == a.samples_out
        assert np.array_equal(iqio.read_wav_audio(a.output_path)[0], iqio.read_wav_audio(_encode(tmp_path, y, rate, sub))[0])


def _encode(tmp_path, y, rate, sub):
    p = tmp_path / "enc.wav"
    iqio.write_wav_audio(p, y, rate, sub)
    return p


def test_device_tensor_input_matches_numpy():
    import torch

    x = _synthetic(22050, 8.0, 2, seed=3)
    for method in ("adaptive", "transient"):
        cfg = S.SquelchConfig(method=method, trim_silence=method == "adaptive")
        y, fl, th = S.apply_squelch(x, 22050.0, cfg)
        yd, fld, thd = S.apply_squelch(torch.from_numpy(x).cuda(), 22050.0, cfg)
        assert isinstance(yd, torch.Tensor) and yd.is_cuda
        assert (fl, th) == (fld, thd)
        assert np.array_equal(yd.cpu().numpy(), y)
        ym, _, _ = S.apply_squelch(torch.from_numpy(x[:, 0].copy()).cuda(), 22050.0, cfg)
        assert np.array_equal(ym.cpu().numpy(), S.apply_squelch(x[:, 0], 22050.0, cfg)[0])


def test_cli_audio_post_writes_cleaned_files(tmp_path):
    x = _synthetic(16000, 6.0, 1, seed=11)
    src = tmp_path / "ch1.wav"
    _write(src, np.clip(x, -1, 1), 16000)
    rc = cli.main(["--audio-post", str(tmp_path), "--audio-post-mode", "static", "--audio-post-lead", "0.2"])
    assert rc == 0
    out = tmp_path / "ch1-cleaned.wav"
    got, rate, sub = iqio.read_wav_audio(out)
    assert (rate, sub) == (16000, "PCM_16")
    data, _, _ = iqio.read_wav_audio(src)
    y, _, _ = S.apply_squelch(data, 16000.0, S.SquelchConfig(method="static", trim_lead_seconds=0.2))
    assert np.array_equal(got, iqio.read_wav_audio(_encode(tmp_path, y, 16000, "PCM_16"))[0])
    assert cli.main(["--audio-post", str(tmp_path / "missing")]) == 1


def test_short_input_raises_value_error():
    with pytest.raises(ValueError):
        S.apply_squelch(np.zeros(100, np.float32), 48000.0, S.SquelchConfig())
    with pytest.raises(ValueError):
        S.apply_squelch(np.zeros(48000, np.float32), 48000.0, S.SquelchConfig(auto_noise_floor=False))
    # an all-zero file squelches to nothing
    y, fl, th = S.apply_squelch(np.zeros((48000, 2), np.float32), 48000.0, S.SquelchConfig())
    assert y.shape == (0, 2) and fl == -160.0
