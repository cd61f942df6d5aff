"""ACARS beside AM (--demod am --acars) on the MI355X: every integer stage identical to the numpy oracle of
tests/acars_model.py, block invariance bit for bit, the bounded kept list, the detector at its edge shapes on the largest
input, the walker on hand-made symbol streams, the CLI end to end on a capture with an ACARS channel, a voice carrier and an
empty channel, and the proof that a run without --acars calls no ACARS entry point."""
from __future__ import annotations

import importlib.util
import json
import math
import sys
from ctypes import c_double, c_int32, c_int64
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


M = _load("acars_model")

SIGMA = 0.2  # complex noise per component against a carrier of 1: the tested limit (tests/test_acars_host.py)
TILE = 2048  # evaluations of I / Q per workgroup of iqa_acars_detect; its outputs are TILE - (L rounded up to 8)


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _same_stages(st: dict, want: dict) -> None:
    for key in ("I", "Q", "y", "same"):
        assert st[key].dtype == {"I": np.int32, "Q": np.int32, "y": np.int64, "same": np.uint8}[key]
        np.testing.assert_array_equal(st[key], want[key], err_msg=key)
    assert len(st["bits"]) == len(want["bits"]) == 8
    for p in range(8):
        np.testing.assert_array_equal(st["bits"][p], want["bits"][p], err_msg=f"symbols of phase {p}")
    assert st["records"] == want["records"]
    assert st["candidates"] == want["reached"]


def _same_messages(res, want: dict) -> None:
    keys = ("time_s", "mode", "address", "registration", "ack", "label", "block_id", "text", "msgno", "flight", "more", "parity_errors", "raw", "hits")
    got = [] if res is None else res.messages
    assert [tuple(getattr(m, k) for k in keys) for m in got] == [tuple(m[k] for k in keys) for m in want["messages"]]
    assert [m.line() for m in got] == [M.line(m) for m in want["messages"]]
    if res is not None:
        assert (res.candidates, res.crc_ok) == (want["reached"], len(want["records"]))


@pytest.mark.parametrize("ppm", [-50.0, 50.0])
@pytest.mark.parametrize("fs", M.RATES)
def test_stages_are_the_oracles(A, fs, ppm):
    """q is the oracle's quantiser of the GPU's own e and emax, exactly; e, emax and q equal numpy's float32 |z| and what the
    oracle makes of it; from the GPU's q, I, Q, y, same, all 8 symbol streams, the sorted kept list, both counters and the
    parsed result are the oracle's.  Integers: no tolerance."""
    from iq_to_audio_amd.decoders.acars import AcarsDecoder

    for sigma in (0.0, 0.1, SIGMA):
        z = M.two_message_stream(fs, sigma, ppm)
        assert z.size <= 300_000
        dec = AcarsDecoder(fs)
        dec.process(z)
        st = dec.stages()
        assert st["e"].dtype == np.float32 and st["q"].dtype == np.int32 and st["q"].size == z.size
        assert st["emax"] == st["e"].max()
        q, sh, _ = M.quantise(st["e"], st["emax"])
        assert sh == st["sh"]
        np.testing.assert_array_equal(st["q"], q)
        e_np = M.envelope(z)
        differ = st["e"] != e_np
        print(f"fs {fs} sigma {sigma}: e against numpy's |z|: {np.mean(differ):.4%} of {differ.size} samples differ, "
              f"max |de| {np.abs(st['e'].astype(np.float64) - e_np).max():.3g}")
        np.testing.assert_array_equal(st["e"], e_np)
        q_np, sh_np, emax_np = M.quantise(e_np)
        assert (sh_np, emax_np) == (st["sh"], st["emax"])
        np.testing.assert_array_equal(st["q"], q_np)
        want = M.oracle(fs=fs, q=st["q"])
        _same_stages(st, want)
        res = dec.finish()
        _same_messages(res, want)
        M.check_two_messages(res.messages)
        print("hits", [m.hits for m in res.messages], "candidates", res.candidates, "crc_ok", res.crc_ok)


def test_block_invariance(A):
    """One stream as a single block and in uneven cuts (a single sample, shorter than W, a cut inside the message):
    identical stages."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.decoders.acars import AcarsDecoder

    fs = M.RATES[1]
    z = D.to_device(M.two_message_stream(fs, SIGMA, 50.0, seed=5), "complex64")
    n = int(z.numel())
    runs = []
    for cuts in ([0, n], [0, 1, 2, 30, 30_000, 30_001, n - 7, n], [0, 2047, 2049, 4096 + 17, 50_003, n - 1, n]):
        dec = AcarsDecoder(fs)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            dec.process(z[lo:hi])
        assert dec.core.pos == n
        runs.append(dec.stages())
    assert len(runs[0]["records"]) >= 2
    for st in runs[1:]:
        for key in ("e", "q", "I", "Q", "y", "same"):
            np.testing.assert_array_equal(st[key], runs[0][key], err_msg=key)
        for p in range(8):
            np.testing.assert_array_equal(st["bits"][p], runs[0]["bits"][p])
        assert (st["sh"], st["emax"], st["records"], st["candidates"]) == (runs[0]["sh"], runs[0]["emax"], runs[0]["records"], runs[0]["candidates"])
    # an envelope block in place of a complex one
    dec = AcarsDecoder(fs)
    dec.process(runs[0]["e"][:1000])
    dec.process(D.to_device(runs[0]["e"][1000:], "float32"))
    np.testing.assert_array_equal(dec.stages()["same"], runs[0]["same"])
    assert dec.stages()["records"] == runs[0]["records"]


def test_kept_list_overflow_is_repeated_not_truncated(A):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N
    from iq_to_audio_amd.decoders import acars as AC

    fs = 96_000.0
    z = M.two_message_stream(fs, 0.1, 50.0)
    roomy, tight = AC.AcarsDecoder(fs), AC.AcarsDecoder(fs)
    roomy.process(z)
    tight.process(z)
    a, b = roomy.core.finish(), tight.core.finish(capacity=1)
    assert len(a["start"]) > 1
    for key in ("phase", "s", "start", "nbytes", "data"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["candidates"] == b["candidates"]
    M.check_two_messages(AC.parse_messages(tight.plan, b, b["candidates"]).messages)
    # the call itself
    lst = D.from_numpy(np.full(8, -7, dtype=np.int64))
    slots = D.from_numpy(np.full(2 * AC.SLOT_BYTES, 0xAA, dtype=np.uint8))
    counts = D.from_numpy(np.array([99, 99], dtype=np.int64))
    N.call("iqa_acars_frames", N.ptr(a["bits"]), c_int64(a["nbits"]), (c_int64 * 8)(*a["count_of"]), c_int32(roomy.plan.W),
           c_double(roomy.plan.step), N.ptr(lst), N.ptr(slots), c_int64(1), N.ptr(counts), N.stream_ptr())
    assert [int(v) for v in counts.cpu().numpy()] == [len(a["start"]), a["candidates"]]
    got, data = lst.cpu().numpy(), slots.cpu().numpy().reshape(2, -1)
    assert (got[4:] == -7).all() and (data[1] == 0xAA).all()
    rows = [tuple(int(v) for v in r) for r in zip(a["phase"], a["s"], a["start"], a["nbytes"])]
    assert tuple(int(v) for v in got[:4]) in rows
    k = rows.index(tuple(int(v) for v in got[:4]))
    np.testing.assert_array_equal(data[0], a["data"][k])
    assert (data[0][int(got[3]) :] == 0).all()


# ---- the detector's edge shapes ---------------------------------------------------------------------------------------------


def _detect(N, D, e_dev, n, sh, pl, taps_dev, outputs: str):
    """One ``iqa_acars_detect`` call with the named optional outputs (a subset of "qIQy"), every output behind a guard."""
    pad, fill = 16, -77
    bufs = {k: D.from_numpy(np.full(n + pad, fill, dtype=np.int64 if k == "y" else np.int32)) for k in outputs}
    same = D.from_numpy(np.full(n + pad, 0xAA, dtype=np.uint8))
    N.call("iqa_acars_detect", N.ptr(e_dev), c_int64(n), c_int32(sh), c_int32(pl["W"]), c_int32(pl["L"]), N.ptr(taps_dev), c_int32(pl["cr"]),
           c_int32(pl["sr"]), N.ptr(bufs.get("q")), N.ptr(bufs.get("I")), N.ptr(bufs.get("Q")), N.ptr(bufs.get("y")), N.ptr(same), N.stream_ptr())
    out = {k: v.cpu().numpy() for k, v in bufs.items()}
    out["same"] = same.cpu().numpy()
    for k, v in out.items():
        assert (v[n:] == (0xAA if k == "same" else fill)).all(), f"{k}: written past n = {n}"
        out[k] = v[:n]
    return out


@pytest.mark.parametrize("fs", [19_200.0, 21_600.0, 28_800.0, 30_600.0, 41_400.0, 96_000.0, 957_600.0, 960_000.0])
def test_detector_edge_shapes(A, fs):
    """L = 8, 9, 12, 13, 17, 40, 399, 400 with their W (W mod 8 = 3, 4, 0, 1, 7, 5, 4, 5: the middle three sit on, one behind
    and one in front of a tap-group boundary) on a full-scale 0 / emax square wave at 1800 Hz (the largest |I|, |Q| and |y|; the
    host test checks the promised widths on it) at n = 1, W - 1, W, W + L - 1, W + L, one workgroup's outputs - 1, + 0, + 1
    and two of them + 3, with the optional outputs all, none and one of each."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N
    from iq_to_audio_amd import dsp_plan as P

    pl = M.plan(fs)
    plan = P.plan_acars(fs)
    W, L = pl["W"], pl["L"]
    assert (W, L) == (plan.W, plan.L) == {19_200.0: (11, 8), 21_600.0: (12, 9), 28_800.0: (16, 12), 30_600.0: (17, 13), 41_400.0: (23, 17), 96_000.0: (53, 40),
                                          957_600.0: (532, 399), 960_000.0: (533, 400)}[fs]
    T = TILE - (L + 7) // 8 * 8
    taps = D.from_numpy(np.ascontiguousarray(plan.taps))
    sizes = [1, W - 1, W, W + L - 1, W + L, T - 1, T, T + 1, 2 * T + 3]
    combos = ["qIQy", "", "q", "I", "Q", "y", "qIQy", "", "qIQy"]
    for k, (n, outputs) in enumerate(zip(sizes, combos)):
        # q reaches 2^15 - 1 where the wave is high; at the last size emax is the float below a power of two, and q = 2^15
        emax = float(np.nextafter(np.float32(0.25), np.float32(0.0))) if k == len(sizes) - 1 else 0.25 - 2.0 ** -17
        e = M.square_wave(n, fs, emax, phase=0.7 * k)
        if not e.any():
            e[0] = emax
        e_dev = D.from_numpy(e)
        peak = D.from_numpy(np.array([123.0], dtype=np.float32))
        N.call("iqa_acars_max", N.ptr(e_dev), c_int64(n), N.ptr(peak), N.stream_ptr())
        assert np.float32(peak.item()) == e.max()
        q, sh, _ = M.quantise(e)
        assert q.max() == (2 ** 15 if k == len(sizes) - 1 else 2 ** 15 - 1)
        I, Q = M.correlate(q, pl)
        y, same = M.detect(I, Q, pl)
        want = dict(q=q, I=I, Q=Q, y=y, same=same)
        got = _detect(N, D, e_dev, n, sh, pl, taps, outputs)
        assert set(got) == set(outputs) | {"same"}
        for key, v in got.items():
            np.testing.assert_array_equal(v, want[key], err_msg=f"n = {n}, outputs '{outputs}': {key}")
    assert np.abs(I).max() > 2 ** 20 or W < 100  # (the long windows come near the int32 limit of the sums)


def test_all_zero_run_launches_nothing_behind_the_max(A, monkeypatch):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N
    from iq_to_audio_amd.decoders.acars import AcarsDecoder

    calls = _count_calls(monkeypatch)
    for block in (np.zeros(5000, dtype=np.complex64), np.zeros(0, dtype=np.complex64)):
        dec = AcarsDecoder(96_000.0)
        dec.process(block)
        assert dec.finish() is None
        st = dec.stages()
        assert st["sh"] is None and st["emax"] == 0 and st["q"] is None and st["same"] is None and st["records"] == [] and st["candidates"] == 0
    assert calls == ["iqa_acars_max", "iqa_acars_max"]
    peak = D.from_numpy(np.array([5.0], dtype=np.float32))
    N.call("iqa_acars_max", N.ptr(None), c_int64(0), N.ptr(peak), N.stream_ptr())
    assert peak.item() == 0.0


def test_walker_on_hand_made_symbol_streams(A):
    """``iqa_acars_frames`` on the host test's hand-made symbol streams (the same row in all 8 phases): the kept blocks, their
    positions, start instants and bytes, and the count of candidates that reached ETX / ETB are the oracle walker's."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.decoders import acars as AC

    plan = P.plan_acars(96_000.0)
    capacity = 16
    for name, row, count, expect in M.hand_made_streams():
        kept, reached = M.frames_of(row[:count])
        assert len(kept) == expect, name  # the oracle first, so that the equality below is not one of empty lists
        nbits = int(row.size)
        plane = D.from_numpy(np.ascontiguousarray(np.tile(row, (8, 1))))
        lst = D.from_numpy(np.full(4 * capacity, -7, dtype=np.int64))
        slots = D.from_numpy(np.full(capacity * AC.SLOT_BYTES, 0xAA, dtype=np.uint8))
        counts = D.from_numpy(np.array([99, 99], dtype=np.int64))
        N.call("iqa_acars_frames", N.ptr(plane), c_int64(nbits), (c_int64 * 8)(*[count] * 8), c_int32(plan.W), c_double(plan.step), N.ptr(lst),
               N.ptr(slots), c_int64(capacity), N.ptr(counts), N.stream_ptr())
        assert [int(v) for v in counts.cpu().numpy()] == [8 * len(kept), 8 * reached], name
        k = 8 * len(kept)
        entries, data = lst.cpu().numpy().reshape(-1, 4), slots.cpu().numpy().reshape(capacity, -1)
        assert (entries[k:] == -7).all() and (data[k:] == 0xAA).all(), name
        got = sorted((int(p), int(s), int(at), data[i, : int(nb)].tobytes(), bool((data[i, int(nb) :] == 0).all()))
                     for i, (p, s, at, nb) in enumerate(entries[:k]))
        want = sorted((p, s, int(plan.instant(s, p)), raw, True) for p in range(8) for s, raw in kept)
        assert got == want, name


def test_symbol_streams_at_a_tie_rate(A):
    """``iqa_acars_bits`` where rint((8 i + p) step) meets exact .5 ties (28 800 Hz, step 1.5), on a random plane, at lengths
    that end on, before and behind an instant."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N

    pl = M.plan(28_800.0)
    rng = np.random.default_rng(8)
    for n in (0, 1, pl["W"] - 1, pl["W"], 1000, 1001, 1002, 4099):
        same = rng.integers(0, 2, size=n).astype(np.uint8)
        want = M.bit_streams(same, pl)
        nbits = max(g.size for g, _ in want) + 2
        out = D.from_numpy(np.full(8 * nbits + 8, 0xAA, dtype=np.uint8))
        N.call("iqa_acars_bits", N.ptr(D.from_numpy(same) if n else None), c_int64(n), c_int32(pl["W"]), c_double(pl["step"]), c_int64(nbits),
               N.ptr(out), N.stream_ptr())
        got = out.cpu().numpy()
        assert (got[8 * nbits :] == 0xAA).all()
        for p, (g, _) in enumerate(want):
            np.testing.assert_array_equal(got[p * nbits : p * nbits + g.size], g, err_msg=f"n = {n}, phase {p}")
            assert (got[p * nbits + g.size : (p + 1) * nbits] == 0).all()


# ---- the pipelines and the command line ---------------------------------------------------------------------------------------


def _count_calls(monkeypatch, prefix="iqa_acars_"):
    from iq_to_audio_amd import _native

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith(prefix):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    return calls


SHORT = dict(mode="2", address=".N12345", ack="\x15", label="H1", block_id="2", text="M01AXX0123POS N49035W072017,1234,350,ETA 1312")
BARE = dict(mode="2", address=".D-ABCD", ack="A", label="Q0", block_id="S", text=None)
LINES = ["ACARS .N12345 H1 2 M01A XX0123 POS N49035W072017,1234,350,ETA 1312", "ACARS .D-ABCD Q0 S"]


def _capture(fs=2.4e6, secs=0.9, seed=17):
    """int16 I/Q: an AM carrier at +300 kHz with two ACARS transmissions (depth 0.5), an AM voice carrier at -500 kHz, nothing
    at +800 kHz; both carriers are keyed from the first sample, so that the mixer-sign probe sees them; complex noise 40 dB
    below a carrier."""
    n = int(round(fs * secs))
    t = np.arange(n, dtype=np.float64) / fs
    amp = 0.28
    keyed = np.ones(n, dtype=np.complex128)
    at = int(0.1 * fs)
    for body in (M.body_bytes(**SHORT), M.body_bytes(**BARE, etb=True)):
        b = M.modulate(M.bits_of(M.message_bytes(body)), fs, scale=1.0, lead=0, tail=0).astype(np.complex128)
        keyed[at : at + b.size] = b
        at += b.size + int(0.05 * fs)
    assert at < n
    x = amp * keyed * np.exp(2j * np.pi * 300e3 * t)
    voice = 1.0 + 0.4 * np.sin(2 * np.pi * 700.0 * t) + 0.3 * np.sin(2 * np.pi * 1900.0 * t + 1.0)
    x += amp * voice * np.exp(2j * np.pi * -500e3 * t)
    rng = np.random.default_rng(seed)
    std = amp * math.sqrt(1e-4 / 2.0)
    x += std * (rng.normal(size=n) + 1j * rng.normal(size=n))
    iq = np.column_stack((x.real, x.imag))
    return np.rint(np.clip(iq, -0.999, 0.999) * 32767.0).astype(np.int16)


def test_end_to_end_three_targets(A, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import cli, iqio
    from iq_to_audio_amd.batch import ResidentBankRunner

    fs, fc = 2.4e6, 131.5e6
    raw = _capture(fs)
    freqs = [fc + 300e3, fc - 500e3, fc + 800e3]
    outs = {}
    calls = _count_calls(monkeypatch)
    for tag, extra in (("plain", []), ("acars", ["--acars"])):
        d = tmp_path / tag
        d.mkdir()
        wav = d / "airband_131500000Hz.wav"
        iqio.write_wav_iq(wav, raw, int(fs), "s16")
        argv = ["--in", str(wav), "--demod", "am", *extra]
        for f in freqs:
            argv += ["--ft", str(f)]
        assert cli.main(argv) == 0
        outs[tag] = [d / f"audio_{int(f)}_48k.wav" for f in freqs]
        if not extra:
            assert calls == []  # a run without --acars calls no ACARS entry point
            assert not list(d.glob("*.acars.json"))
            capsys.readouterr()
    printed = capsys.readouterr().out
    assert calls.count("iqa_acars_max") == 3 and calls.count("iqa_acars_detect") >= 2 and calls.count("iqa_acars_frames") >= 2
    for a, b in zip(outs["plain"], outs["acars"]):
        assert a.read_bytes() == b.read_bytes()  # the audio does not change
    js = [json.loads(p.with_name(p.stem + ".acars.json").read_text()) for p in outs["acars"]]
    print("targets:", js)
    assert js[1] is None and js[2] is None  # the voice carrier and the empty channel
    got = js[0]["messages"]
    assert [(m["address"], m["registration"], m["label"], m["block_id"], m["msgno"], m["flight"], m["text"], m["more"], m["parity_errors"]) for m in got] == [
        (".N12345", "N12345", "H1", "2", "M01A", "XX0123", SHORT["text"][10:], False, 0), (".D-ABCD", "D-ABCD", "Q0", "S", None, None, None, True, 0)]
    assert [m["raw"] for m in got] == [M.with_bcs(M.body_bytes(**SHORT)).hex(), M.with_bcs(M.body_bytes(**BARE, etb=True)).hex()]
    assert js[0]["crc_ok"] == sum(m["hits"] for m in got) <= js[0]["candidates"] and all(m["hits"] >= 1 for m in got)
    times = [m["time_s"] for m in got]
    assert times == sorted(times) and 0.1 < times[0] < 0.3
    for text in LINES:
        assert f"{freqs[0]:.0f} Hz: {text}" in printed
    assert "ACARS" not in "".join(l for l in printed.splitlines() if not l.startswith(f"{freqs[0]:.0f} Hz"))
    # the pipelines: several device blocks, one target and two
    wav = tmp_path / "plain" / "airband_131500000Hz.wav"

    def cfgs(tag):
        return [A.ProcessingConfig(in_path=wav, target_freq=f, demod_mode="am", chunk_size=65_536, output_path=tmp_path / f"{tag}{i}.wav")
                for i, f in enumerate(freqs[:2])]

    multi = A.MultiChannelPipeline(cfgs("m"), acars=True)
    for o in multi.owners:
        o.block_frames_target = 524_288
    multi.run()
    assert multi.acars[1] is None and multi.acars[0] is multi.owners[0].acars
    assert [m.line() for m in multi.acars[0].messages] == LINES
    one = A.ProcessingPipeline(cfgs("o")[0], acars=True)
    one.run()
    assert [m.raw for m in one.acars.messages] == [m["raw"] for m in got] and [m.line() for m in one.acars.messages] == LINES
    with pytest.raises(ValueError, match="acars"):
        ResidentBankRunner([dict(freq_offset=300e3)], sample_rate=fs, n_frames=1 << 20, acars=True)


def test_reset_starts_a_new_run(A):
    """``ChannelDemod.reset`` also clears the stored envelope and the position; the envelope never lands in the audio buffer."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.processing import ChannelDemod

    fs = 96_000.0
    first = D.to_device(M.two_message_stream(fs, 0.1, 50.0)[:60_000], "complex64")
    second = D.to_device(M.modulate(M.bits_of(M.message_bytes(M.body_bytes(**BARE, etb=True))), fs, sigma=0.1, seed=4), "complex64")

    def run(dem, z):
        out = D.empty(int(z.numel()), "float32")
        dem.process(z, np.array([0], dtype=np.int64), out)
        return out

    used = ChannelDemod("am", fs, deemph_us=300.0, agc_enabled=True, acars=True)
    run(used, first)
    used.reset()
    audio = run(used, second)
    fresh = ChannelDemod("am", fs, deemph_us=300.0, agc_enabled=True, acars=True)
    run(fresh, second)
    plain = ChannelDemod("am", fs, deemph_us=300.0, agc_enabled=True)
    np.testing.assert_array_equal(audio.cpu().numpy(), run(plain, second).cpu().numpy())
    assert used.side["acars"].pos == fresh.side["acars"].pos == int(second.numel()) and plain.side_result("acars") is None
    a, b = used.side["acars"].finish(), fresh.side["acars"].finish()
    assert len(b["start"]) >= 1
    for key in ("phase", "s", "start", "nbytes", "data"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert [m.line() for m in used.side_result("acars").messages] == LINES[1:]
    with pytest.raises(ValueError, match="--demod am"):
        ChannelDemod("nfm", fs, deemph_us=300.0, agc_enabled=True, acars=True)
