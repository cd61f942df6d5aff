"""The keying measurement (--find-decode) on the MI355X, on the model capture of tests/keying_model.py
(thirteen channels of known keying, s16): the window rows of every channel equal the numpy oracle's, applied to the GPU's own
theta; the centre is the oracle's from the GPU's describe rows; the labels and decoders are the host test's; cuts of a channel
stream into calls change no bit of the per-window sums; reset; the CLI: a run without the flag calls no entry point of the
keying and writes the same two JSON files; and one capture with a pager, a packet burst and a voice channel end to end through
--find-top 3 --find-auto --find-decode against three explicit runs."""
from __future__ import annotations

import importlib.util
import json
import math
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


K = _load("keying_model")
M = K.M
FS = K.FS
FC = K.FC_AIR  # the AM channel lies in the airband


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
    """The model capture through the finder and the keying describer, once: everything the tests below read."""
    from iq_to_audio_amd import dsp_plan as P

    raw = K.capture()
    plan = P.plan_find(FS, raw.shape[0])
    finder = A.ChannelFinder(plan, "s16")
    for block in _blocks(raw):
        finder.process(block)
    fin = finder.finish()
    found = finder.result(FC)
    describer = A.ChannelDescriber(plan, fin, found.channels, "s16", "iq", keep_stages=True, keying=True)
    for block in _blocks(raw):
        describer.process(block)
    return dict(raw=raw, plan=plan, fin=fin, found=found, describer=describer, stages=describer.stages(), result=describer.result(FC),
                keying=describer.keying_result(FC))


def _find_args(plan):
    return dict(hop=plan.hop, T=plan.slice_frames, F=plan.frames)


def test_rows_and_centres_are_the_oracles(A, gpu):
    plan, found = gpu["plan"], gpu["found"]
    assert len(found.channels) == len(K.CHANNELS) == len(gpu["stages"])
    for (name, offset, *_), ch, st in zip(K.CHANNELS, found.channels, gpu["stages"]):
        assert abs(ch.offset_hz - offset) <= (3000.0 if name == "wfm" else 1000.0), (name, ch.offset_hz)
        dp = st["plan"]
        theta, z = st["theta"], st["z"]
        assert theta.dtype == np.float32 and theta.size == z.size == sum(st["calls"]) and st["calls"] == K.calls_of(gpu["raw"].shape[0], dp.decimation)
        # theta is the discriminator of the describer's stream, with a state carried across the blocks
        turn = np.angle(np.exp(1j * (theta.astype(np.float64) - K.quadrature(z).astype(np.float64))))
        assert np.percentile(np.abs(turn), 99) < 1e-3, name
        # the centre: the oracle's rule on the GPU's describe rows
        c, start = K.centre_from_rows(st["rows"], st["calls"])
        assert (st["c"], st["keyed_from"]) == (c, start) and c is not None and start == 0, name
        kp = K.plan(dp.fs_ch)
        assert st["keying_plan"].incs == kp["incs"] and st["keying_plan"].skipped == kp["skipped"]
        want = K.stream_rows(theta, st["calls"], c, start, kp["incs"], st["gate"], D=dp.decimation, delay=dp.delay, **_find_args(plan))
        print(name, "c", c, "K", int(want[:, 1].sum()), "P", int(want[:, 0].sum()), K.figures(want, kp)["coh"])
        assert want[:, 0].sum() >= 1024 and want.shape == (-(-theta.size // 2048), 16)
        np.testing.assert_array_equal(st["keying_rows"], want, err_msg=name)
        # every call's own rows, window by window
        pos = 0
        for (first, rows), n in zip(st["keying_parts"], st["calls"]):
            front = None if pos == 0 else theta[pos - 1]
            assert first == pos // 2048
            np.testing.assert_array_equal(rows, K.rows(theta[pos : pos + n], pos, front, c, kp["incs"], st["gate"], D=dp.decimation, delay=dp.delay,
                                                       **_find_args(plan)), err_msg=name)
            pos += n


def test_labels_and_decoders(A, gpu):
    got = gpu["keying"]
    assert isinstance(got, A.KeyingResult) and (got.sample_rate, got.center_freq) == (FS, FC)
    for (name, _, lab, key, decoders), d, k, st in zip(K.CHANNELS, gpu["result"].channels, got.channels, gpu["stages"]):
        print(name, k.line())
        assert (d.label, k.described, k.label, k.decoders) == (lab, lab, key, decoders), name
        assert (k.offset_hz, k.freq_hz, k.fs_ch, k.centre) == (d.offset_hz, d.freq_hz, d.fs_ch, st["c"])
        kp = K.plan(d.fs_ch)
        f = K.figures(st["keying_rows"], kp)
        assert (k.coh, k.rate_hz, k.crossings, k.pairs) == (f["coh"], f["rate_hz"], f["crossings"], f["pairs"]), name
        assert (k.label, k.baud) == (K.rule(f["coh"], f["rate_hz"], f["crossings"], kp) if lab == "nfm" else (None, None))
        assert k.bw == (25000.0 if decoders == ["ais"] else d.bw)
    by = dict(zip(K.NAMES, got.channels))
    assert by["gmsk9600"].line().endswith("-> --ais --bw 25000") and by["fsk1200"].line().endswith("-> --pocsag")
    assert by["fsk4_4800"].line().endswith("-> 4800 baud (DMR / P25 / NXDN class): no decoder here")
    assert by["wfm"].line() == "    keying: not measured (wfm) -> --rds" and by["am"].line().endswith("-> --acars")
    # outside the airband the AM channel has no decoder
    out = gpu["describer"].keying(K.FC_OUT)
    assert out[K.NAMES.index("am")].decoders == [] and [k.decoders for k in out[:10]] == [k.decoders for k in got.channels[:10]]


def test_cuts_of_a_stream_change_no_bit(A, gpu):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.keying import add_keying_rows

    describer = A.ChannelDescriber(gpu["plan"], gpu["fin"], gpu["found"].channels, "s16", "iq", keying=True)
    lanes = describer.lanes()
    for j in (1, 3, 8):  # 2-FSK 1200, GMSK 9600 and the tone: 369 231, 177 778 and 141 177 samples
        z = D.from_numpy(gpu["stages"][j]["z"])
        lane = lanes[j]
        lane.sh, lane.centre = gpu["stages"][j]["sh"], gpu["stages"][j]["c"]
        at = 0
        for n in [1, 1, 2046, 2048, 2049, 1000, 1, 7, 4099, 1, 1 << 30]:  # single samples, cuts inside a window and at its edges
            n = min(n, int(z.numel()) - at)
            describer.feed(lane, z[at : at + n])
            at += n
        assert at == int(z.numel()) and lane.pos == at and len(lane.krows) == 11 and lane.keyed_from == 0
        rows = add_keying_rows([(first, r.cpu().numpy()) for first, r in lane.krows], -(-at // 2048))
        np.testing.assert_array_equal(rows, gpu["stages"][j]["keying_rows"], err_msg=str(j))


def test_centre_comes_with_the_first_block_of_1024_pairs(A, gpu):
    """A channel whose gate comes on late: the calls in front of the one that brings the describe rows to 1024 pairs are not
    keyed, that call and the ones behind it are; a channel that never gets there has no figures."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import keying as KY

    plan = gpu["plan"]
    describer = A.ChannelDescriber(plan, gpu["fin"], gpu["found"].channels, "s16", "iq", keep_stages=True, keying=True)
    lanes = describer.lanes()
    st = gpu["stages"][1]
    dp, lane = st["plan"], lanes[1]
    find = dict(D=dp.decimation, delay=dp.delay, **_find_args(plan))
    gate = np.zeros(plan.slices, dtype=np.uint8)
    gate[plan.slices // 2 :] = 1
    on = np.flatnonzero(M.gate_of(np.arange(st["z"].size), gate, **find))
    m0 = int(on[0])
    assert 150_000 < m0 < 220_000 and on.size == st["z"].size - m0
    calls = [m0 - 10, 510, 600, 1000]  # 0, 499, 1099 pairs after the first three
    calls.append(st["z"].size - sum(calls))
    lane.sh, lane.gate, lane.gate_dev = st["sh"], gate, D.from_numpy(gate)
    z = D.from_numpy(st["z"])
    at = 0
    for n in calls:
        describer.feed(lane, z[at : at + n])
        at += n
    rows = D.torch_mod().cat(lane.rows).cpu().numpy()
    c, start = K.centre_from_rows(rows, calls)
    assert start == m0 - 10 + 510 and [M.add_rows(r.cpu().numpy())[1] for r in lane.rows[:3]] == [0, 499, 600]
    assert (lane.centre, lane.keyed_from) == (c, start) and len(lane.krows) == 3 and lane.krows[0][0] == start // 2048
    theta = D.torch_mod().cat(lane.theta).cpu().numpy()
    kp = K.plan(dp.fs_ch)
    want = K.stream_rows(theta, calls, c, start, kp["incs"], gate, **find)
    got = KY.add_keying_rows([(first, r.cpu().numpy()) for first, r in lane.krows], -(-at // 2048))
    np.testing.assert_array_equal(got, want)
    assert want[: start // 2048].sum() == 0 and want[:, 0].sum() == st["z"].size - start  # the 510 samples of the second call are not keyed
    # never 1024 pairs: no centre, no rows, and the channel reads unkeyed without figures
    lane = lanes[2]
    lane.gate = np.zeros(plan.slices, dtype=np.uint8)
    lane.sh, lane.gate_dev = gpu["stages"][2]["sh"], D.from_numpy(lane.gate)
    describer.feed(lane, D.from_numpy(gpu["stages"][2]["z"]))
    assert lane.centre is None and lane.krows == [] and lane.keyed_from is None
    k = KY.key_channel(gpu["result"].channels[2], lane.kplan, None, lane.centre, FS)
    assert (k.label, k.coh, k.crossings, k.decoders) == ("unkeyed", [None] * 7, 0, ["ax25", "tones"])


def test_reset_starts_a_new_run(A, gpu):
    describer = gpu["describer"]
    first = [None if r is None else r.copy() for r in describer.finish_keying()]
    centres = [st["c"] for st in gpu["stages"]]
    describer.reset()
    describer.process(gpu["raw"][:300_000].reshape(-1))  # part of a run, thrown away
    describer.reset()
    for block in _blocks(gpu["raw"]):
        describer.process(block)
    again = describer.finish_keying()
    assert [lane.centre for lane in describer.lanes()] == centres
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)


# ---- the command line --------------------------------------------------------------------------------------------------------


def _count_calls(monkeypatch):
    from iq_to_audio_amd import _native

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith("iqa_keying_"):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    return calls


def test_cli_lines_and_files(A, gpu, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import cli, iqio

    calls = _count_calls(monkeypatch)
    stem = f"model_{int(FC)}Hz"
    dirs = {}
    for tag in ("describe", "decode"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
        iqio.write_wav_iq(dirs[tag] / f"{stem}.wav", gpu["raw"], int(FS), "s16")
    # a --find-describe run calls no entry point of the keying
    assert cli.main(["--in", str(dirs["describe"] / f"{stem}.wav"), "--find-describe"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert calls == [] and len(plain) == 26 and not list(dirs["describe"].glob("*.keying.json"))
    # --find-decode: the same lines with the keying line under each pair, the same two JSON files, and keying.json
    assert cli.main(["--in", str(dirs["decode"] / f"{stem}.wav"), "--find-decode"]) == 0
    printed = capsys.readouterr().out.splitlines()
    assert set(calls) == {"iqa_keying_accumulate"} and len(calls) >= 13
    assert printed[0::3] == plain[0::2] and printed[1::3] == plain[1::2] and printed[2::3] == gpu["keying"].lines()
    assert all(line.startswith("    keying: ") for line in printed[2::3])
    for name in (f"{stem}.channels.json", f"{stem}.describe.json"):
        assert (dirs["decode"] / name).read_bytes() == (dirs["describe"] / name).read_bytes(), name
    stored = A.KeyingResult.from_json(json.loads((dirs["decode"] / f"{stem}.keying.json").read_text()))
    assert stored == gpu["keying"]
    res, des, key = A.find_channels(dirs["decode"] / f"{stem}.wav", describe=True, keying=True)
    assert res == gpu["found"] and des == gpu["result"] and key == gpu["keying"]


PAGES = [(1234567, 3, "KEYED FSK 1200"), (424242, 0, "0123456789"), (77, 1, "SECOND BATCH")]
PACKET = ("N0CALL-7", "APRS", ["WIDE1-1"], "!4903.50N/07201.75W-found and decoded")


def _traffic(fs=2.4e6):
    """int16 I/Q: a POCSAG 1200 transmission at +300 kHz that fills the capture, an AX.25 burst at -500 kHz from its start,
    an NFM voice at +800 kHz; describe_model's level and noise rule."""
    PM, XM = _load("pocsag_model"), _load("ax25_model")
    # (64 more alternating bits: the last codeword ends with the batch, and the channel filters' delays need a carrier behind it)
    bits = np.concatenate((PM.transmission_bits(PAGES), np.arange(64, dtype=np.uint8) & 1))
    pager = PM.modulate(bits, fs, 1200, lead=0, tail=0).astype(np.complex128)
    n = pager.size
    t = np.arange(n, dtype=np.float64) / fs
    frame = XM.ui_frame(PACKET[0], PACKET[1], PACKET[2], PACKET[3])
    burst = XM.modulate(XM.hdlc_bits([frame, frame], preamble=40), fs, lead=0, tail=0).astype(np.complex128)[:n]
    packet = np.zeros(n, dtype=np.complex128)
    packet[: burst.size] = burst
    rng = np.random.default_rng(31)
    sigma = M.AMP * 10.0 ** (-30.0 / 20.0) / math.sqrt(2.0)
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x += M.AMP * pager * np.exp(2j * np.pi * ((300e3 * t) % 1.0))
    x += M.AMP * packet * np.exp(2j * np.pi * ((-500e3 * t) % 1.0))
    x += M.AMP * np.exp(2j * np.pi * ((800e3 * t) % 1.0)) * np.exp(2j * np.pi * 2500.0 * np.cumsum(M.voice(1, n)) / fs)
    out = np.empty((n, 2), dtype=np.int16)
    out[:, 0] = np.clip(np.rint(x.real * 32768.0), -32768, 32767)
    out[:, 1] = np.clip(np.rint(x.imag * 32768.0), -32768, 32767)
    return out


def test_end_to_end(A, tmp_path, capsys):
    from iq_to_audio_amd import cli, iqio

    PM, XM = _load("pocsag_model"), _load("ax25_model")
    fs, fc = 2.4e6, 150e6
    raw = _traffic(fs)
    dirs = {}
    for tag in ("auto", "explicit"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
        iqio.write_wav_iq(dirs[tag] / "traffic_150000000Hz.wav", raw, int(fs), "s16")
    wav = dirs["auto"] / "traffic_150000000Hz.wav"
    assert cli.main(["--in", str(wav), "--find-top", "3", "--find-auto", "--find-decode", "--find-grid", "12500"]) == 0
    printed = capsys.readouterr().out
    print(printed)
    key = A.KeyingResult.from_json(json.loads(wav.with_name("traffic_150000000Hz.keying.json").read_text()))
    des = A.DescribeResult.from_json(json.loads(wav.with_name("traffic_150000000Hz.describe.json").read_text()))
    assert [round(k.offset_hz / 12500.0) * 12500.0 for k in key.channels] == [-500e3, 300e3, 800e3]
    assert [(k.label, k.decoders) for k in key.channels] == [("unkeyed", ["ax25", "tones"]), ("fsk 1200", ["pocsag"]), ("unkeyed", ["ax25", "tones"])]
    # the pager message and the frame
    page = json.loads((dirs["auto"] / "audio_150300000_48k.pocsag.json").read_text())
    assert [(m["address"], m["function"], m["text"]) for m in page["messages"]] == [(a, f, PM.shown(f, text)) for a, f, text in PAGES]
    assert f'150300000 Hz: POCSAG1200 addr=1234567 func=3 alpha "{PAGES[0][2]}"' in printed
    packet = json.loads((dirs["auto"] / "audio_149500000_48k.ax25.json").read_text())
    assert packet["frames"] and all((f["source"], f["dest"], f["info"]) == (PACKET[0], PACKET[1], PACKET[3]) for f in packet["frames"])
    assert "149500000 Hz: AX25 N0CALL-7>APRS" in printed
    assert sorted(p.name for p in dirs["auto"].glob("audio_*.json")) == [
        "audio_149500000_48k.ax25.json", "audio_149500000_48k.tones.json", "audio_150300000_48k.pocsag.json",
        "audio_150800000_48k.ax25.json", "audio_150800000_48k.tones.json"]
    # three explicit runs with the suggested --ft, --demod, --bw and decoder flags: the same WAVs and decoder JSON, byte for byte
    for d, k in zip(des.channels, key.channels):
        freq = math.floor(d.tuned_hz / 12500.0 + 0.5) * 12500.0
        argv = ["--in", str(dirs["explicit"] / "traffic_150000000Hz.wav"), "--ft", f"{freq:.0f}", "--demod", d.demod, "--bw", f"{k.bw:.0f}"]
        assert cli.main(argv + [f"--{name}" for name in k.decoders]) == 0
        names = [f"audio_{int(freq)}_48k.wav"] + [f"audio_{int(freq)}_48k.{name}.json" for name in k.decoders]
        for name in names:
            a, b = (dirs["auto"] / name).read_bytes(), (dirs["explicit"] / name).read_bytes()
            assert a == b and len(a) > 3, name
        assert len((dirs["auto"] / names[0]).read_bytes()) > 50_000
