"""POCSAG beside narrowband FM (--demod nfm --pocsag) on the MI355X: every integer stage identical to the numpy oracle of
tests/pocsag_model.py, block invariance bit for bit, the CLI end to end on a capture with a 1200-baud channel, an inverted
512-baud channel off tune and a voice carrier, and the proof that a run without --pocsag calls no POCSAG entry point."""
from __future__ import annotations

import importlib.util
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _load_model():
    name = "pocsag_model"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name("pocsag_model.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load_model()

MESSAGES = [(1234567, 3, "Pump 4 pressure low, call 0171 5550123"), (424242, 0, "0123456789"), (77, 1, "ok")]
SIGMA = 0.2  # complex noise per component against a carrier of 1: the level tests/test_pocsag_host.py settles on the CPU


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _stream(fs: float, seed: int) -> np.ndarray:
    """Three transmissions behind one another: 1200 baud, 512 baud inverted 1.5 kHz low, 2400 baud 1.5 kHz high."""
    bits = M.transmission_bits(MESSAGES)
    short = M.transmission_bits(MESSAGES[1:])
    parts = [M.modulate(bits, fs, 1200, ppm=50.0, sigma=SIGMA, seed=seed),
             M.modulate(short, fs, 512, inverted=True, offset_hz=-1500.0, ppm=-50.0, sigma=SIGMA, seed=seed + 1),
             M.modulate(bits, fs, 2400, offset_hz=1500.0, sigma=SIGMA, seed=seed + 2)]
    return np.concatenate(parts)


def _same_batches(got: dict, want: dict) -> None:
    for baud in M.BAUDS:
        g, kept = got[baud], want["syncs"][baud]
        assert [int(v) for v in g["n0"]] == [k[0] for k in kept], baud
        assert [int(v) for v in g["sigma"]] == [k[1] for k in kept], baud
        assert [bool(v) for v in g["inverted"]] == [k[2] for k in kept], baud
        assert [int(v) for v in g["distance"]] == [k[3] for k in kept], baud
        np.testing.assert_array_equal(g["words"], want["batches"][baud]["words"], err_msg=f"corrected {baud}")
        np.testing.assert_array_equal(g["raw"], want["batches"][baud]["raw"], err_msg=f"raw {baud}")
        np.testing.assert_array_equal(g["status"], want["batches"][baud]["status"], err_msg=f"status {baud}")


def test_stages_are_the_oracles(A):
    """t is the oracle's quantiser of the GPU's own theta, exactly; from the GPU's t, S, the kept syncs, the corrected and
    raw words, the status and the messages are the oracle's.  Integers: no tolerance."""
    from iq_to_audio_amd.decoders.pocsag import PocsagDecoder

    fs = 96_000.0
    z = _stream(fs, seed=21)
    dec = PocsagDecoder(fs)
    dec.process(z)
    st = dec.stages()
    assert st["t"].dtype == np.int32 and st["t"].size == z.size
    np.testing.assert_array_equal(st["t"], M.quantise(st["theta"]))
    dt = np.abs(st["t"].astype(np.int64) - M.quantise(M.theta_of(z)).astype(np.int64))
    print(f"t against numpy's theta: {np.mean(dt != 0):.3%} of {dt.size} samples differ, max |dt| {dt.max()}")
    assert dt.max() <= 1
    want = M.oracle(fs=fs, t=st["t"])
    assert want["skipped"] == []
    for baud in M.BAUDS:
        np.testing.assert_array_equal(st["S"][baud], want["S"][baud], err_msg=f"S {baud}")
    _same_batches(st["batches"], want)
    res = dec.finish()
    assert res is not None and res.bauds_skipped == []
    assert M.triples(res.messages) == M.triples(want["messages"])
    assert [(m.baud, m.inverted, round(m.time_s * fs)) for m in res.messages] == [
        (m["baud"], m["inverted"], round(m["time_s"] * fs)) for m in want["messages"]]
    sent = [(a, f, M.shown(f, t)) for a, f, t in MESSAGES]
    assert M.triples(res.messages) == sent + sent[1:] + sent  # 1200, then 512 (two messages), then 2400
    full, short = len(M.batches_of(MESSAGES)), len(M.batches_of(MESSAGES[1:]))
    assert res.syncs == {512: short, 1200: full, 2400: full} and res.codewords["uncorrectable"] == 0
    print("dc_hz", res.dc_hz, "codewords", res.codewords)


# Deliberate bit errors: (batch, codeword or -1 for the sync word, bit position counted from the LSB).
SINGLE_FLIPS = [(0, 1, 25), (0, 2, 5), (0, 3, 0), (0, 4, 31), (0, 14, 15), (0, 15, 12), (1, 2, 18)]  # data, check, parity, flag bits
DOUBLE_FLIPS = [(0, 5, 20), (0, 5, 7), (1, 14, 0), (1, 14, 30)]  # two in one codeword (idle ones: no message is cut)
SYNC_FLIPS = [(0, -1, 5), (1, -1, 3), (1, -1, 28)]  # distance 1 in the first batch, 2 in the second, 0 in the third
ABSENT_FROM = 13  # the stream ends inside codeword 13 of the third batch


def _damaged_stream(fs: float, baud: int, inverted: bool, seed: int) -> np.ndarray:
    """One transmission of MESSAGES (three batches) with the flips above in its bit periods, cut inside the last batch."""
    bits = M.transmission_bits(MESSAGES).copy()
    assert len(M.batches_of(MESSAGES)) == 3

    def at(batch, word, bit):
        return 576 + 544 * batch + 32 * (1 + word) + (31 - bit)

    for batch, word, bit in SINGLE_FLIPS + DOUBLE_FLIPS + SYNC_FLIPS:
        bits[at(batch, word, bit)] ^= 1
    lead = 3000
    z = M.modulate(bits, fs, baud, inverted=inverted, offset_hz=700.0, sigma=0.05, seed=seed, lead=lead, tail=0)
    return z[: lead + int(at(2, ABSENT_FROM, 20) * fs / baud)]


@pytest.mark.parametrize("fs,baud,inverted", [(96_000.0, 1200, False), (10e6 / 104, 512, True), (96_000.0, 2400, False)])
def test_correction_refusal_absence_and_tolerant_sync(A, fs, baud, inverted):
    """Flipped bit periods reach every branch of the codeword kernel and the tolerant sync match: single errors in data,
    check, parity and flag bits (status 1, the word restored), two errors in one codeword (status 2, raw kept), one and two
    wrong sync bits (distance 1 and 2), a stream that ends inside a batch (status 3).  The oracle's histogram is checked
    first, so that the equality with the GPU below is not a comparison of all-clean words."""
    from iq_to_audio_amd.decoders.pocsag import PocsagDecoder

    z = _damaged_stream(fs, baud, inverted, seed=baud)
    dec = PocsagDecoder(fs)
    dec.process(z)
    st = dec.stages()
    np.testing.assert_array_equal(st["t"], M.quantise(st["theta"]))
    want = M.oracle(fs=fs, t=st["t"])
    status = want["batches"][baud]["status"]
    assert [k[3] for k in want["syncs"][baud]] == [1, 2, 0] and [k[2] for k in want["syncs"][baud]] == [inverted] * 3
    assert all(len(v) == 0 for b, v in want["syncs"].items() if b != baud)
    hist = {v: int((status == v).sum()) for v in range(4)}
    assert hist == {0: 48 - 7 - 2 - 3, 1: len(SINGLE_FLIPS), 2: 2, 3: 16 - ABSENT_FROM}, hist
    sent = M.batches_of(MESSAGES)
    for batch, word, bit in SINGLE_FLIPS:
        assert status[batch, word] == 1
        assert want["batches"][baud]["raw"][batch, word] == sent[batch][word] ^ (1 << bit)
        assert want["batches"][baud]["words"][batch, word] == sent[batch][word]
    for batch, word in {(b, w) for b, w, _ in DOUBLE_FLIPS}:
        assert status[batch, word] == 2 and want["batches"][baud]["words"][batch, word] == want["batches"][baud]["raw"][batch, word] != sent[batch][word]
    assert (status[2, ABSENT_FROM:] == 3).all() and (want["batches"][baud]["words"][2, ABSENT_FROM:] == 0).all()
    # the GPU: identical
    np.testing.assert_array_equal(st["S"][baud], want["S"][baud])
    _same_batches(st["batches"], want)
    res = dec.finish()
    assert res.codewords == dict(ok=hist[0], corrected=hist[1], uncorrectable=hist[2], absent=hist[3])
    assert M.triples(res.messages) == M.triples(want["messages"]) == [(a, f, M.shown(f, t)) for a, f, t in MESSAGES]
    assert [m.corrected for m in res.messages] == [3, 0, 0] and [m.inverted for m in res.messages] == [inverted] * 3
    assert abs(res.dc_hz - 700.0) < 60.0


def test_reset_starts_a_new_run(A):
    """``ChannelDemod.reset`` also clears the POCSAG history, position, stored planes and discriminator state: a reused
    demodulator decodes its second stream as a fresh one does."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.processing import ChannelDemod

    fs = 96_000.0
    first = D.to_device(_stream(fs, seed=21)[:150_000], "complex64")
    second = D.to_device(_damaged_stream(fs, 1200, False, seed=4), "complex64")

    def run(dem, z):
        dem.process(z, np.array([0], dtype=np.int64), D.empty(int(z.numel()), "float32"))

    used = ChannelDemod("nfm", fs, deemph_us=300.0, agc_enabled=True, pocsag=True)
    run(used, first)
    used.reset()
    run(used, second)
    fresh = ChannelDemod("nfm", fs, deemph_us=300.0, agc_enabled=True, pocsag=True)
    run(fresh, second)
    assert used.side["pocsag"].pos == fresh.side["pocsag"].pos == int(second.numel())
    a, b = used.side["pocsag"].finish(), fresh.side["pocsag"].finish()
    assert len(b[1200]["n0"]) == 3
    for baud in M.BAUDS:
        for key in ("n0", "sigma", "inverted", "distance", "words", "raw", "status"):
            np.testing.assert_array_equal(a[baud][key], b[baud][key], err_msg=f"{key} {baud}")
    assert M.triples(used.side_result("pocsag").messages) == M.triples(fresh.side_result("pocsag").messages)


@pytest.mark.parametrize("fs", [96_000.0, 10e6 / 104])
def test_block_invariance(A, fs):
    """One stream as a single block and in uneven cuts (shorter than the carried history, a single sample): bit-identical
    t, S, kept syncs, words and status."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.decoders.pocsag import PocsagDecoder

    z = D.to_device(_stream(fs, seed=5), "complex64")
    n = int(z.numel())
    runs = []
    for cuts in ([0, n], [0, 100_003, 100_004, 101_000, 200_001, n], [0, 7, 2047, 2049, 4096 + 17, 4096 + 60, n - 30_000, n - 1, n]):
        dec = PocsagDecoder(fs)
        assert len(cuts) == 2 or min(b - a for a, b in zip(cuts[:-1], cuts[1:])) < dec.plan.hist_len
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            dec.process(z[lo:hi])
        runs.append(dec.stages())
    assert sum(len(b["n0"]) for b in runs[0]["batches"].values()) == 2 * len(M.batches_of(MESSAGES)) + len(M.batches_of(MESSAGES[1:]))
    for st in runs[1:]:
        np.testing.assert_array_equal(st["theta"], runs[0]["theta"])
        np.testing.assert_array_equal(st["t"], runs[0]["t"])
        for baud in M.BAUDS:
            np.testing.assert_array_equal(st["S"][baud], runs[0]["S"][baud], err_msg=f"S {baud}")
            for key in ("n0", "sigma", "inverted", "distance", "words", "raw", "status"):
                np.testing.assert_array_equal(st["batches"][baud][key], runs[0]["batches"][baud][key], err_msg=f"{key} {baud}")


def test_sync_list_overflow_is_repeated_not_truncated(A):
    """A list shorter than the number of kept syncs reports the full count; nothing is written past the capacity."""
    from ctypes import c_int32, c_int64

    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N
    from iq_to_audio_amd.decoders.pocsag import PocsagDecoder

    fs = 96_000.0
    dec = PocsagDecoder(fs)
    dec.process(_stream(fs, seed=21))
    st = dec.core.joined()
    pb = next(b for b in dec.plan.bauds if b.baud == 1200)
    s = st["S"][1200]
    n = int(s.numel())
    offs = (c_int32 * 32)(*[int(v) for v in pb.offsets[:32]])
    score, count = D.empty(n, "int64"), D.zeros(1, "int64")
    lst = D.from_numpy(np.full(8, -7, dtype=np.int64))
    N.call("iqa_pocsag_sync", N.ptr(s), c_int64(n), offs, c_int32(pb.h), N.ptr(score), N.ptr(lst), c_int64(1), N.ptr(count), N.stream_ptr())
    assert int(count.item()) == len(M.batches_of(MESSAGES)) > 1
    got = lst.cpu().numpy()
    assert (got[4:] == -7).all() and got[0] in [int(v) for v in dec.stages()["batches"][1200]["n0"]]


def _capture(fs=2.4e6, secs=3.0, seed=17):
    """int16 I/Q: a 1200-baud channel at +300 kHz (an alpha and a numeric message), a 512-baud inverted channel whose carrier
    sits 1 kHz above the tuned -500 kHz (both keyed from the first sample, so that the mixer-sign probe sees them), an NFM
    voice carrier (1 kHz tone, 3 kHz deviation) at +800 kHz, complex noise
    40 dB below a carrier."""
    n = int(round(fs * secs))
    t = np.arange(n, dtype=np.float64) / fs
    amp = 0.28
    x = np.zeros(n, dtype=np.complex128)

    def place(bits, baud, f_centre, inverted, start):
        b = M.modulate(bits, fs, baud, inverted=inverted, lead=0, tail=0).astype(np.complex128)[: n - start]
        keyed = np.ones(n, dtype=np.complex128)  # the transmitter is keyed for the whole capture: a bare carrier around the data
        keyed[start : start + b.size] = b
        x[:] += amp * keyed * np.exp(2j * np.pi * f_centre * t)

    place(M.transmission_bits(MESSAGES[:2]), 1200, 300e3, False, int(0.2 * fs))
    place(M.transmission_bits(MESSAGES[1:]), 512, -500e3 + 1000.0, True, int(0.3 * fs))
    x += amp * np.exp(1j * (2 * np.pi * 800e3 * t + 2 * np.pi * 3000.0 / fs * np.cumsum(np.sin(2 * np.pi * 1000.0 * t))))
    rng = np.random.default_rng(seed)
    std = amp * math.sqrt(1e-4 / 2.0)
    x += std * (rng.normal(size=n) + 1j * rng.normal(size=n))
    iq = np.column_stack((x.real, x.imag))
    return np.rint(np.clip(iq, -0.999, 0.999) * 32767.0).astype(np.int16)


def _count_pocsag_calls(monkeypatch):
    from iq_to_audio_amd import _native

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith("iqa_pocsag_"):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    return calls


def test_end_to_end_three_targets(A, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import cli, iqio

    fs, fc = 2.4e6, 150e6
    raw = _capture(fs)
    freqs = [fc + 300e3, fc - 500e3, fc + 800e3]
    outs = {}
    calls = _count_pocsag_calls(monkeypatch)
    for tag, extra in (("plain", []), ("pocsag", ["--pocsag"])):
        d = tmp_path / tag
        d.mkdir()
        wav = d / "pager_150000000Hz.wav"
        iqio.write_wav_iq(wav, raw, int(fs), "s16")
        argv = ["--in", str(wav), "--demod", "nfm", *extra]
        for f in freqs:
            argv += ["--ft", str(f)]
        assert cli.main(argv) == 0
        outs[tag] = [d / f"audio_{int(f)}_48k.wav" for f in freqs]
        if tag == "plain":
            assert calls == []  # a run without --pocsag calls no POCSAG entry point
            assert not list(d.glob("*.pocsag.json"))
    assert {"iqa_pocsag_integrate", "iqa_pocsag_sync", "iqa_pocsag_codewords"} <= set(calls)
    for a, b in zip(outs["plain"], outs["pocsag"]):
        assert a.read_bytes() == b.read_bytes()  # the audio does not change
    printed = capsys.readouterr().out
    js = [json.loads(p.with_name(p.stem + ".pocsag.json").read_text()) for p in outs["pocsag"]]
    print("targets:", js)
    sent = [(a, f, M.shown(f, t)) for a, f, t in MESSAGES]
    assert [(m["address"], m["function"], m["text"]) for m in js[0]["messages"]] == sent[:2]
    assert all(m["baud"] == 1200 and not m["inverted"] for m in js[0]["messages"])
    assert [(m["address"], m["function"], m["text"]) for m in js[1]["messages"]] == sent[1:]
    assert all(m["baud"] == 512 and m["inverted"] for m in js[1]["messages"])
    assert abs(js[1]["dc_hz"] - 1000.0) < 100.0 and abs(js[0]["dc_hz"]) < 100.0
    assert js[2] is None  # the voice carrier
    assert [m["kind"] for m in js[0]["messages"]] == ["alpha", "numeric"]
    assert f'{freqs[0]:.0f} Hz: POCSAG1200 addr=1234567 func=3 alpha "{MESSAGES[0][2]}"' in printed
    assert f'{freqs[1]:.0f} Hz: POCSAG512 addr=424242 func=0 numeric "0123456789"' in printed


def test_pipeline_surface(A, tmp_path, monkeypatch):
    from iq_to_audio_amd import iqio
    from iq_to_audio_amd.batch import ResidentBankRunner

    fs, fc = 2.4e6, 150e6
    wav = tmp_path / "pager_150000000Hz.wav"
    iqio.write_wav_iq(wav, _capture(fs, 2.2), int(fs), "s16")  # (the 1200-baud transmission ends at 2.04 s)

    def cfgs(tag):
        return [A.ProcessingConfig(in_path=wav, target_freq=f, demod_mode="nfm", chunk_size=65_536, output_path=tmp_path / f"{tag}{i}.wav")
                for i, f in enumerate((fc + 300e3, fc + 800e3))]

    calls = _count_pocsag_calls(monkeypatch)
    def several_blocks(pipe):
        for o in getattr(pipe, "owners", [pipe]):
            o.block_frames_target = 1_048_576  # six device blocks: the carried history is exercised
        return pipe

    plain = several_blocks(A.MultiChannelPipeline(cfgs("p")))
    plain.run()
    assert calls == [] and plain.pocsag == [None, None]
    multi = several_blocks(A.MultiChannelPipeline(cfgs("m"), pocsag=True))
    multi.run()
    assert multi.pocsag[1] is None and multi.pocsag[0] is multi.owners[0].pocsag
    sent = [(a, f, M.shown(f, t)) for a, f, t in MESSAGES[:2]]
    assert M.triples(multi.pocsag[0].messages) == sent
    assert calls.count("iqa_pocsag_integrate") >= 2 * 5
    one = A.ProcessingPipeline(cfgs("o")[0], pocsag=True)
    one.run()
    assert M.triples(one.pocsag.messages) == sent
    for i in range(2):
        assert (tmp_path / f"p{i}.wav").read_bytes() == (tmp_path / f"m{i}.wav").read_bytes()
    with pytest.raises(ValueError, match="pocsag"):
        ResidentBankRunner([dict(freq_offset=300e3)], sample_rate=fs, n_frames=1 << 20, pocsag=True)
