"""The carrier squelch end to end on the MI355X (--squelch): a 2.4 MS/s int16 capture of 3 s with a keyed
NFM channel, a keyed AM voice and an empty target.  For each target the numpy oracle (tests/gate_model.py) applied to the
GPU's own channel stream gives the GPU's cells, frames, floor, states and bounds exactly, and applied to the GPU's own audio
its gated audio exactly; the WAV is the resampler's output of that audio, silent away from the transmissions and the unflagged
run's inside them; block cuts change no bit; a run without the flag calls no gate entry point and writes what it wrote.
(The carriers are keyed and the warm-up chunk holds noise alone, which tells the mixer-sign probe nothing: the sign is given.)"""
from __future__ import annotations

import importlib.util
import json
import sys
import wave
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


G = _load("gate_model")
FS, FC, SECS = 2.4e6, 455.5e6, 3.0
OFFSETS = (300e3, -500e3, 800e3)  # the keyed NFM channel, the keyed AM voice, nothing
MODES = ("nfm", "am", "nfm")
FREQS = [FC + o for o in OFFSETS]
NFM_KEYED = G.MODEL_KEYED
AM_KEYED = (1.0, 2.0)
STAGES = ("cells", "v", "s", "s2", "g", "lo", "hi")


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _capture(seed=23) -> np.ndarray:
    """int16 I/Q: the model's two-tone FM carrier keyed 0.5-1.1 s, 1.8-2.0 s and 2.5-2.52 s at +300 kHz, an AM voice (two
    tones, 50 % depth) keyed 1.0-2.0 s at -500 kHz, and complex noise 30 dB under a carrier in 12.5 kHz."""
    n = int(round(FS * SECS))
    t = np.arange(n, dtype=np.float64) / FS
    amp = 0.2
    x = amp * G.model_carrier(n, FS) * np.exp(2j * np.pi * OFFSETS[0] * t)
    voice = 1.0 + 0.25 * (np.sin(2 * np.pi * 500.0 * t) + np.sin(2 * np.pi * 1300.0 * t))
    key = ((t >= AM_KEYED[0]) & (t < AM_KEYED[1])).astype(np.float64)
    x += amp * key * voice * np.exp(2j * np.pi * OFFSETS[1] * t)
    rng = np.random.default_rng(seed)
    std = amp * np.sqrt(1e-3 * FS / 12_500.0 / 2.0)
    x += std * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    iq = np.column_stack((x.real, x.imag))
    return np.rint(np.clip(iq, -0.999, 0.999) * 32767.0).astype(np.int16)


def _pcm(path: Path) -> np.ndarray:
    with wave.open(str(path), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 48_000)
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


def _count_calls(monkeypatch, prefix="iqa_gate_"):
    from iq_to_audio_amd import _native

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith(prefix):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    return calls


@pytest.fixture(scope="module")
def runs(A, tmp_path_factory):
    """The capture through the multi-channel pipeline in several device blocks, with the squelch and without it; per target
    the GPU's own channel stream, its audio, its gated audio and the gate's stages."""
    from iq_to_audio_amd import iqio

    d = tmp_path_factory.mktemp("gate")
    wav = d / "keyed_455500000Hz.wav"
    iqio.write_wav_iq(wav, _capture(), int(FS), "s16")
    out = dict(wav=wav, dir=d)
    for tag, squelch in (("plain", None), ("gated", A.CarrierSquelch())):
        cfgs = [A.ProcessingConfig(in_path=wav, target_freq=f, demod_mode=m, chunk_size=65_536, mix_sign_override=1, output_path=d / f"{tag}{i}.wav",
                                   dump_iq_path=d / f"{tag}{i}.cf32") for i, (f, m) in enumerate(zip(FREQS, MODES))]
        pipe = A.MultiChannelPipeline(cfgs, squelch=squelch)
        for o in pipe.owners:
            o.block_frames_target = 1_048_576  # several device blocks: cells are cut by the calls
            o.keep_channel_audio = True
        pipe.run()
        out[tag] = dict(pipe=pipe, z=[np.fromfile(c.dump_iq_path, dtype=np.complex64) for c in cfgs],
                        audio=[o.audio_fs_channel.cpu().numpy() for o in pipe.owners], paths=[c.output_path for c in cfgs])
    g = out["gated"]
    g["stages"] = [o.squelch_gate.stages() for o in g["pipe"].owners]
    g["gated_audio"] = [o.squelch_audio.cpu().numpy() for o in g["pipe"].owners]
    g["results"] = g["pipe"].squelch_result
    return out


def test_stages_are_the_oracles_on_the_gpus_own_stream(A, runs):
    g = runs["gated"]
    for i in range(3):
        z, st = g["z"][i], g["stages"][i]
        assert z.size == g["audio"][i].size == 288_000 and len(st["calls"]) >= 3 and sum(st["calls"]) == z.size
        assert any(c % 256 for c in np.cumsum(st["calls"])[:-1])  # a call ends inside a cell
        head = z[: min(st["calls"][0], 65536)]
        assert st["sh"] == G.choose_shift(float(np.mean(head.real.astype(np.float64) ** 2 + head.imag.astype(np.float64) ** 2)))
        p = G.plan(96_000.0)
        want = G.run(z, p, sh=st["sh"], cuts=st["calls"])
        assert st["floor"] == want["floor"]
        for k in STAGES:
            np.testing.assert_array_equal(st[k], want[k], err_msg=f"target {i}: {k}")
        for (first, part), n, pos in zip(st["parts"], st["calls"], np.cumsum([0] + st["calls"])):
            assert first == pos // 256
            np.testing.assert_array_equal(part, G.cells(z[pos : pos + n], int(pos), st["sh"]))
        # the result is the host arithmetic of these integers
        res, model = g["results"][i], G.result(want, z.size, st["sh"], p)
        assert [(t.start, t.end) for t in res.transmissions] == G.transmissions(want["g"], z.size, p["Lf"])
        assert res.floor_dbfs == pytest.approx(model["floor_dbfs"], abs=1e-9) and res.duty == model["duty"] and res.frequency == FREQS[i]
        assert res is g["pipe"].owners[i].squelch_result


def test_gated_audio_is_the_oracles_product(A, runs):
    g, p = runs["gated"], G.plan(96_000.0)
    for i in range(3):
        st, a = g["stages"][i], g["audio"][i]
        np.testing.assert_array_equal(a, runs["plain"]["audio"][i])  # keep_channel_audio hands out the ungated audio
        want = G.apply(a, st["g"], st["lo"], st["hi"], p)
        got = g["gated_audio"][i]
        finite = ~np.isnan(want)
        np.testing.assert_array_equal(got.view(np.uint32)[finite], want.view(np.uint32)[finite])
        np.testing.assert_array_equal(np.isnan(got), ~finite)
        gain = G.gain(st["g"], st["lo"], st["hi"], a.size, p)
        assert (got[gain == 0] == 0).all()


def test_wav_is_the_resampled_gated_audio(A, runs):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.processing import Resampler48k

    g, p = runs["gated"], G.plan(96_000.0)
    rp = P.plan_resampler(96_000.0)
    span = -(-(rp.half_taps + 1) * rp.up // rp.down) + 1  # 48 kHz samples on either side that an input sample reaches
    for i in range(3):
        pcm, plain = _pcm(g["paths"][i]), _pcm(runs["plain"]["paths"][i])
        assert pcm.size == plain.size == rp.n_out(288_000)  # the WAV keeps its length and time axis
        again = Resampler48k(96_000.0).process(D.from_numpy(g["gated_audio"][i]), want="pcm16").cpu().numpy()
        np.testing.assert_array_equal(pcm, again)
        st = g["stages"][i]
        tx = G.transmissions(st["g"], 288_000, p["Lf"])
        far = np.ones(pcm.size, dtype=bool)  # further than the resampler's span from any transmission
        inside = np.zeros(pcm.size, dtype=bool)  # inside one, beyond its ramps and the span
        for a, b in tx:
            far[max(0, a * rp.up // rp.down - span) : b * rp.up // rp.down + span + 1] = False
            inside[(a + p["R"]) * rp.up // rp.down + span : (b - p["R"]) * rp.up // rp.down - span] = True
        assert (pcm[far] == 0).all()
        np.testing.assert_array_equal(pcm[inside], plain[inside])
        assert far.any() and (inside.any() or not tx) and (not tx or np.any(plain[far] != 0))


def test_transmissions_are_where_the_carriers_are(A, runs):
    g, p = runs["gated"], G.plan(96_000.0)
    Lf, frame_s = p["Lf"], p["Lf"] / 96_000.0

    def at(seconds):  # the channel sample of a time of the capture
        return int(round(seconds * 96_000.0))

    nfm, am, empty = g["results"]
    assert len(nfm.transmissions) == 2  # the 20 ms click at 2.5 s is dropped by the minimum duration
    for t, (on, off) in zip(nfm.transmissions, NFM_KEYED[:2]):
        assert at(on) - (p["A"] + 2) * Lf <= t.start <= at(on)
        assert at(off) + p["H"] * Lf <= t.end <= at(off) + (p["H"] + 2) * Lf
        assert t.mean_db > 20.0 and t.peak_db >= t.mean_db
    click = [r for r in G.runs(g["stages"][0]["s"]) if r[0] * frame_s > 2.4]
    assert click and not g["stages"][0]["s2"][int(2.4 / frame_s) :].any()
    assert len(am.transmissions) == 1
    t = am.transmissions[0]
    assert at(AM_KEYED[0]) - (p["A"] + 2) * Lf <= t.start <= at(AM_KEYED[0])
    assert at(AM_KEYED[1]) + p["H"] * Lf <= t.end <= at(AM_KEYED[1]) + (p["H"] + 2) * Lf
    assert empty.transmissions == [] and empty.duty == 0.0 and empty.lines(f"{FREQS[2]:.0f} Hz: ") == [f"{FREQS[2]:.0f} Hz: squelch never opened"]
    silent = _pcm(g["paths"][2])
    assert silent.size == _pcm(runs["plain"]["paths"][2]).size and not silent.any() and _pcm(runs["plain"]["paths"][2]).any()
    # (noise 30 dB under a carrier of 0.2 in 12.5 kHz: -44 dBFS in the channel, and the tenth percentile a little under it)
    assert -50.0 < empty.floor_dbfs < -38.0 and abs(nfm.floor_dbfs - empty.floor_dbfs) < 1.0


def test_block_cuts_change_no_bit_and_reset_gives_a_fresh_run(A, runs):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import dsp_plan as P

    z, st = runs["gated"]["z"][0], runs["gated"]["stages"][0]
    audio = runs["gated"]["audio"][0]
    gate = A.CarrierGate(P.plan_gate(96_000.0), sh=st["sh"])
    z_dev = D.from_numpy(z)
    rng = np.random.default_rng(3)
    for cuts in ([1, 255, 1, 100, 100, 55, 2048, 3], list(rng.integers(1, 256, 40)), [z.size]):  # a sample, blocks shorter than a cell
        cuts = [int(c) for c in cuts]
        cuts.append(z.size - sum(cuts))
        gate.reset()
        assert gate.pos == 0 and gate.calls == []
        with pytest.raises(ValueError, match="finish"):
            gate.stages()
        pos = 0
        for k in cuts:
            gate.process(z_dev[pos : pos + k])
            pos += k
        gate.finish(z.size)
        got = gate.stages()
        assert got["floor"] == st["floor"] and got["sh"] == st["sh"] and got["calls"] == [c for c in cuts if c]
        for k in STAGES:
            np.testing.assert_array_equal(got[k], st[k], err_msg=k)
        np.testing.assert_array_equal(gate.apply(D.from_numpy(audio)).cpu().numpy().view(np.uint32), runs["gated"]["gated_audio"][0].view(np.uint32))
        assert gate.result(FREQS[0]) == runs["gated"]["results"][0]
        with pytest.raises(ValueError, match="finished"):
            gate.process(z_dev[:10])
    # a fresh run on another stream: nothing of the last one is left
    gate.reset()
    gate.process(z_dev[:5000])
    with pytest.raises(ValueError, match="held 5000"):
        gate.finish(4000)
    gate.finish()
    short = gate.stages()
    want = G.run(z[:5000], G.plan(96_000.0), sh=st["sh"])
    for k in STAGES:
        np.testing.assert_array_equal(short[k], want[k], err_msg=k)
    # sh from the first block when none is given
    own = A.CarrierGate(P.plan_gate(96_000.0))
    own.process(z_dev[: st["calls"][0]])
    assert own.sh == st["sh"]
    empty = A.CarrierGate(P.plan_gate(96_000.0))
    empty.finish()
    assert empty.result().transmissions == [] and empty.apply(D.empty(0, "float32")).numel() == 0


def test_unflagged_run_calls_no_gate_entry_and_writes_what_it_wrote(A, runs, tmp_path, monkeypatch):
    from iq_to_audio_amd import iqio
    from iq_to_audio_amd.processing import Resampler48k

    calls = _count_calls(monkeypatch)
    cfg = A.ProcessingConfig(in_path=runs["wav"], target_freq=FREQS[0], demod_mode="nfm", chunk_size=65_536, mix_sign_override=1, output_path=tmp_path / "one.wav")
    one = A.ProcessingPipeline(cfg)
    one.block_frames_target = 1_048_576
    one.keep_channel_audio = True
    one.run()
    assert calls == [] and one.squelch_result is None and one.squelch_gate is None
    # the parent's way of writing it: the resampler's PCM16 of the channel-rate audio
    pcm = Resampler48k(96_000.0).process(one.audio_fs_channel, want="pcm16").cpu().numpy()
    iqio.write_wav_pcm16(tmp_path / "parent.wav", pcm, 48_000)
    assert (tmp_path / "parent.wav").read_bytes() == (tmp_path / "one.wav").read_bytes()
    gated = A.ProcessingPipeline(A.ProcessingConfig(in_path=runs["wav"], target_freq=FREQS[0], demod_mode="nfm", chunk_size=65_536, mix_sign_override=1,
                                                    output_path=tmp_path / "two.wav"), squelch=A.CarrierSquelch())
    gated.block_frames_target = 1_048_576
    gated.run()
    assert {"iqa_gate_power", "iqa_gate_add_cells", "iqa_gate_decide", "iqa_gate_apply"} == set(calls)
    assert calls.count("iqa_gate_decide") == calls.count("iqa_gate_apply") == 1 and calls.count("iqa_gate_power") >= 3
    assert len(gated.squelch_result.transmissions) == 2 and (tmp_path / "two.wav").read_bytes() != (tmp_path / "one.wav").read_bytes()


def test_cli_split_and_side_decoders(A, runs, tmp_path, capsys):
    from iq_to_audio_amd import cli
    from iq_to_audio_amd import dsp_plan as P

    outs = {}
    for tag, extra in (("plain", ["--tones"]), ("gated", ["--tones", "--squelch", "--squelch-split"])):
        d = tmp_path / tag
        d.mkdir()
        wav = d / "keyed_455500000Hz.wav"
        wav.write_bytes(runs["wav"].read_bytes())
        argv = ["--in", str(wav), "--demod", "nfm", "--chunk", "65536", "--mix-sign", "1", *extra]
        for f in FREQS:
            argv += ["--ft", str(f)]
        capsys.readouterr()
        assert cli.main(argv) == 0
        outs[tag] = ([d / f"audio_{int(f)}_48k.wav" for f in FREQS], capsys.readouterr().out)
    plain, gated = outs["plain"][0], outs["gated"][0]
    assert not list((tmp_path / "plain").glob("*.squelch.json")) and not list((tmp_path / "plain").glob("*.tx*.wav"))
    assert " Hz: on " not in outs["plain"][1] and "never opened" not in outs["plain"][1]
    for a, b in zip(plain, gated):  # the side decoders read what they read: their files do not change
        assert a.with_name(a.stem + ".tones.json").read_bytes() == b.with_name(b.stem + ".tones.json").read_bytes()
    assert plain[0].read_bytes() != gated[0].read_bytes() and _pcm(plain[0]).size == _pcm(gated[0]).size
    lines = [l for l in outs["gated"][1].splitlines() if " Hz: on " in l or "squelch never opened" in l]
    rp = P.plan_resampler(96_000.0)
    for i, (f, wav) in enumerate(zip(FREQS, gated)):
        js = json.loads(wav.with_name(wav.stem + ".squelch.json").read_text())
        res = A.GateResult.from_json(js)
        mine = [l for l in lines if l.startswith(f"{f:.0f} Hz: ")]
        assert mine == res.lines(f"{f:.0f} Hz: ")
        parts = sorted(wav.parent.glob(f"{wav.stem}.tx*.wav"))
        assert [p.name for p in parts] == [f"{wav.stem}.tx{k:04d}.wav" for k in range(1, len(res.transmissions) + 1)]
        for part, t in zip(parts, res.transmissions):
            assert _pcm(part).size == rp.n_out(t.end - t.start) and _pcm(part).any()
        if i == 0:
            assert len(parts) == 2 and [(t.start, t.end) for t in res.transmissions] == [(t.start, t.end) for t in runs["gated"]["results"][0].transmissions]
            assert mine[0].startswith(f"{f:.0f} Hz: on 0.4") and " s), " in mine[0] and mine[0].endswith(" dB over the floor")
        if i == 2:
            assert mine == [f"{f:.0f} Hz: squelch never opened"] and parts == [] and not _pcm(wav).any()
