"""AX.25 over Bell-202 AFSK beside narrowband FM (--demod nfm --ax25) on the MI355X: every integer stage identical to the
numpy oracle of tests/ax25_model.py, block invariance bit for bit, the bounded frame list, the CLI end to end on a capture
with an APRS channel, a pager channel and a voice carrier, and the proof that a run without --ax25 calls no AFSK entry
point."""
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


M = _load("ax25_model")
PM = _load("pocsag_model")

SIGMA = 0.2  # complex noise per component against a carrier of 1: the tested limit (tests/test_ax25_host.py)
FRAMES = [("N0CALL-7", "APRS", ["WIDE1-1*", "WIDE2-1"], "!4903.50N/07201.75W-Test 001234 of the AFSK decoder, padded out to length..."),
          ("DL1ABC-15", "APDR16", [], ">status ~ with a tilde, {braces} and 7E: ~~~~"),
          ("AB1CDE", "BEACON", ["DB0XYZ-2*"], "T#123,045,067,089,101,123,00001111")]
PAGES = [(1234567, 3, "Pump 4 pressure low"), (424242, 0, "0123456789")]


def _raw(k):
    return M.ui_frame(*FRAMES[k])


def _lines():
    return [f"{s}>{','.join([d] + p)}:{i}" for s, d, p, i in FRAMES]


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _stream(fs: float, seed: int) -> np.ndarray:
    """Three transmissions behind one another: a flat transmitter 50 ppm fast (two frames sharing one flag), a pre-emphasised
    one (space x 2) 50 ppm slow and 500 Hz high, a de-emphasised one (space x 0.5) 700 Hz low; all at SIGMA."""
    parts = [M.modulate(M.hdlc_bits([_raw(0), _raw(1)]), fs, space_gain=1.0, ppm=50.0, sigma=SIGMA, seed=seed),
             M.modulate(M.hdlc_bits([_raw(2)]), fs, space_gain=2.0, ppm=-50.0, offset_hz=500.0, sigma=SIGMA, seed=seed + 1),
             M.modulate(M.hdlc_bits([_raw(1)]), fs, space_gain=0.5, offset_hz=-700.0, sigma=SIGMA, seed=seed + 2)]
    return np.concatenate(parts)


def _same_stages(st: dict, want: dict) -> None:
    for f in (1200, 2200):
        assert st["E"][f].dtype == np.int64
        np.testing.assert_array_equal(st["E"][f], want["E"][f], err_msg=f"E {f}")
    np.testing.assert_array_equal(st["sign"], want["sign"])
    assert len(st["bits"]) == len(want["bits"]) == 24
    for v in range(24):
        np.testing.assert_array_equal(st["bits"][v], want["bits"][v], err_msg=f"bits of variant {v}")
    assert st["records"] == want["records"]
    assert st["candidates"] == want["closed"]


def _same_frames(res, want: dict) -> None:
    got = [] if res is None else res.frames
    assert [(f.source, f.dest, f.path, f.control, f.pid, f.info, f.raw, f.hits) for f in got] == [
        (f["source"], f["dest"], f["path"], f["control"], f["pid"], f["info"], f["raw"], f["hits"]) for f in want["frames"]]
    if res is not None:
        assert (res.candidates, res.crc_ok, res.rejected) == (want["closed"], len(want["records"]), want["rejected"])


@pytest.mark.parametrize("fs", [96_000.0, 10e6 / 104])
def test_stages_are_the_oracles(A, fs):
    """t is the oracle's quantiser of the GPU's own theta, exactly; against numpy's float32 theta it differs by at most 1;
    from the GPU's t, the energy planes, the slicer plane, all 24 bit streams, the sorted kept-frame list and the parsed
    frames are the oracle's.  Integers: no tolerance."""
    from iq_to_audio_amd.decoders.ax25 import Ax25Decoder

    z = _stream(fs, seed=21)
    dec = Ax25Decoder(fs)
    dec.process(z)
    st = dec.stages()
    assert st["t"].dtype == np.int32 and st["t"].size == z.size and st["sign"].dtype == np.uint8
    np.testing.assert_array_equal(st["t"], M.quantise(st["theta"]))
    dt = np.abs(st["t"].astype(np.int64) - M.quantise(M.theta_of(z)).astype(np.int64))
    print(f"fs {fs}: t against numpy's theta: {np.mean(dt != 0):.4%} of {dt.size} samples differ, max |dt| {dt.max()}")
    assert dt.max() <= 1
    want = M.oracle(fs=fs, t=st["t"])
    _same_stages(st, want)
    res = dec.finish()
    _same_frames(res, want)
    assert [f.time_s for f in res.frames] == [f["time_s"] for f in want["frames"]]
    assert [f.line() for f in res.frames] == [_lines()[k] for k in (0, 1, 2, 1)]
    assert [f.raw for f in res.frames] == [_raw(k).hex() for k in (0, 1, 2, 1)]
    print("hits", [f.hits for f in res.frames], "candidates", res.candidates, "crc_ok", res.crc_ok)
    assert all(f.hits >= 1 for f in res.frames) and res.crc_ok == sum(f.hits for f in res.frames) and res.rejected == 0


@pytest.mark.parametrize("fs", [48_000.0, 480_000.0])
def test_other_window_lengths(A, fs):
    """L = 40 and the longest window, L = 400 (the tap tables are padded to a multiple of 8 inside the kernel; 400 and 40 are
    such multiples, so a rate with L = 43 is run as well)."""
    from iq_to_audio_amd.decoders.ax25 import Ax25Decoder

    for rate in (fs, fs * 43.0 / 40.0 if fs < 100_000.0 else fs * 397.0 / 400.0):
        z = M.modulate(M.hdlc_bits([_raw(0)]), rate, offset_hz=300.0, sigma=0.05, seed=3)
        dec = Ax25Decoder(rate)
        assert dec.plan.L == int(np.rint(rate / 1200.0))
        dec.process(z[:5000])
        dec.process(z[5000:])
        st = dec.stages()
        np.testing.assert_array_equal(st["t"], M.quantise(st["theta"]))
        want = M.oracle(fs=rate, t=st["t"])
        _same_stages(st, want)
        assert [f.line() for f in dec.finish().frames] == _lines()[:1]


@pytest.mark.parametrize("fs", [96_000.0, 10e6 / 104])
def test_block_invariance(A, fs):
    """One stream as a single block and in uneven cuts (shorter than the carried history, a single sample): bit-identical
    theta, t, energies, slicer plane, bit streams and kept frames."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.decoders.ax25 import Ax25Decoder

    z = D.to_device(_stream(fs, seed=5), "complex64")
    n = int(z.numel())
    runs = []
    for cuts in ([0, n], [0, 100_003, 100_004, 101_000, 200_001, n], [0, 7, 2047, 2049, 4096 + 17, 4096 + 60, n - 30_000, n - 1, n]):
        dec = Ax25Decoder(fs)
        assert len(cuts) == 2 or min(b - a for a, b in zip(cuts[:-1], cuts[1:])) < dec.core.hist_len
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            dec.process(z[lo:hi])
        assert dec.core.pos == n
        runs.append(dec.stages())
    assert len(runs[0]["records"]) >= 4
    for st in runs[1:]:
        np.testing.assert_array_equal(st["theta"], runs[0]["theta"])
        np.testing.assert_array_equal(st["t"], runs[0]["t"])
        for f in (1200, 2200):
            np.testing.assert_array_equal(st["E"][f], runs[0]["E"][f], err_msg=f"E {f}")
        np.testing.assert_array_equal(st["sign"], runs[0]["sign"])
        for v in range(24):
            np.testing.assert_array_equal(st["bits"][v], runs[0]["bits"][v], err_msg=f"bits of variant {v}")
        assert st["records"] == runs[0]["records"] and st["candidates"] == runs[0]["candidates"]


def test_frame_list_overflow_is_repeated_not_truncated(A):
    """A list of capacity 1 reports the full count and writes nothing past its one entry; ``finish`` then repeats the call
    with room for all and gives the same frames as a run whose list was long enough from the start."""
    from ctypes import c_double, c_int32, c_int64

    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N
    from iq_to_audio_amd.decoders import ax25 as AX

    fs = 96_000.0
    z = _stream(fs, seed=21)
    roomy, tight = AX.Ax25Decoder(fs), AX.Ax25Decoder(fs)
    roomy.process(z)
    tight.process(z)
    a, b = roomy.core.finish(), tight.core.finish(capacity=1)
    assert len(a["start"]) > 1
    for key in ("variant", "s", "start", "nbytes", "data"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["candidates"] == b["candidates"]
    lines = [f.line() for f in AX.parse_frames(tight.plan, b, b["candidates"]).frames]
    assert lines == [_lines()[k] for k in (0, 1, 2, 1)]
    # the call itself
    lst = D.from_numpy(np.full(8, -7, dtype=np.int64))
    slots = D.from_numpy(np.full(2 * AX.SLOT_BYTES, 0xAA, dtype=np.uint8))
    counts = D.from_numpy(np.array([99, 99], dtype=np.int64))
    count_of = (c_int64 * 8)(*a["count_of"])
    N.call("iqa_afsk_frames", N.ptr(a["bits"]), c_int64(a["nbits"]), count_of, c_int32(roomy.plan.L), c_double(roomy.plan.step), N.ptr(lst),
           N.ptr(slots), c_int64(1), N.ptr(counts), N.stream_ptr())
    assert [int(v) for v in counts.cpu().numpy()] == [len(a["start"]), a["candidates"]]
    got, data = lst.cpu().numpy(), slots.cpu().numpy().reshape(2, -1)
    assert (got[4:] == -7).all() and (data[1] == 0xAA).all()
    rows = [tuple(int(v) for v in r) for r in zip(a["variant"], a["s"], a["start"], a["nbytes"])]
    assert tuple(int(v) for v in got[:4]) in rows
    k = rows.index(tuple(int(v) for v in got[:4]))
    np.testing.assert_array_equal(data[0], a["data"][k])
    assert (data[0][int(got[3]) :] == 0).all()


def _with_fcs(body: bytes) -> bytes:
    fcs = M.crc16(body)
    return body + bytes([fcs & 0xFF, fcs >> 8])


def _hand_made_streams() -> list:
    """(name, bit plane row, bits that exist): the streams of tests/test_ax25_host.py's walker test.  Where fewer bits exist
    than the row holds, the row goes on with the bits that would have closed the frame, which the kernel must not read."""
    body = M.ui_frame("AB1CDE", "BEACON", [], b"\x7e\x7e\xff\xff\x7e and \x3e\x7c")[:-2]  # 0x7E and runs of ones in the payload
    frame = _with_fcs(body)
    stuffed = M.stuffed_bits(frame)
    bits = M.hdlc_bits([frame], preamble=3, postamble=2)
    other = M.ui_frame("N0CALL-7", "APRS", ["WIDE1-1*"], ">status")
    out = [("stuffed payload", bits, bits.size),
           ("abort", np.array(M.FLAG_BITS + stuffed[:40] + [1] * 7 + stuffed[40:] + M.FLAG_BITS, dtype=np.uint8), None),
           ("flag off the byte boundary", np.array(M.FLAG_BITS + stuffed[:43] + M.FLAG_BITS + stuffed[43:] + M.FLAG_BITS, dtype=np.uint8), None),
           ("shared flag", M.hdlc_bits([frame, other], preamble=1, between=1, postamble=1), None),
           ("two flags between", M.hdlc_bits([frame, other], preamble=2, between=2, postamble=1), None),
           ("idle flags", M.hdlc_bits([frame], preamble=30, postamble=5), None),
           ("cut inside the frame", bits, 24 + len(stuffed) - 5),
           ("cut inside the closing flag", bits, 24 + len(stuffed) + 7),
           ("cut behind the closing flag", bits, 24 + len(stuffed) + 8),
           ("shorter than a flag", bits, 7), ("one flag", bits, 8), ("empty", bits, 0)]
    for size in (16, 17, 18, 329, 330, 331, 332):
        f = _with_fcs(bytes((3 * k + 1) & 0xFF for k in range(size - 2)))
        assert len(f) == size
        out.append((f"{size} bytes", M.hdlc_bits([f], preamble=2, postamble=1), None))
    bad = bits.copy()
    bad[24 + 50] ^= 1
    out.append(("damaged", bad, None))
    return [(name, np.asarray(row, dtype=np.uint8), int(np.asarray(row).size if count is None else count)) for name, row, count in out]


def test_walker_on_hand_made_bit_streams(A):
    """``iqa_afsk_frames`` on hand-made bit planes (the same row in all 24 variants): the kept frames, their positions, start
    instants and bytes, and the count of closed candidates are the oracle walker's, at the exact 16 / 17 and 330 / 331 byte
    limits, for an abort, a flag off the byte boundary, frames sharing a flag, and streams that end inside a frame, inside
    the closing flag and right behind it."""
    from ctypes import c_double, c_int32, c_int64

    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.decoders import ax25 as AX

    plan = P.plan_afsk(96_000.0)
    capacity = 64
    expect_kept = {"stuffed payload": 1, "abort": 0, "flag off the byte boundary": 0, "shared flag": 2, "two flags between": 2, "idle flags": 1,
                   "cut inside the frame": 0, "cut inside the closing flag": 0, "cut behind the closing flag": 1, "shorter than a flag": 0,
                   "one flag": 0, "empty": 0, "16 bytes": 0, "17 bytes": 1, "18 bytes": 1, "329 bytes": 1, "330 bytes": 1, "331 bytes": 0,
                   "332 bytes": 0, "damaged": 0}
    for name, row, count in _hand_made_streams():
        kept, closed = M.frames_of(row[:count])
        assert len(kept) == expect_kept[name], name  # the oracle first, so that the equality below is not one of empty lists
        nbits = int(row.size)
        plane = D.from_numpy(np.ascontiguousarray(np.tile(row, (AX.VARIANTS, 1))))
        lst = D.from_numpy(np.full(4 * capacity, -7, dtype=np.int64))
        slots = D.from_numpy(np.full(capacity * AX.SLOT_BYTES, 0xAA, dtype=np.uint8))
        counts = D.from_numpy(np.array([99, 99], dtype=np.int64))
        N.call("iqa_afsk_frames", N.ptr(plane), c_int64(nbits), (c_int64 * 8)(*[count] * 8), c_int32(plan.L), c_double(plan.step), N.ptr(lst),
               N.ptr(slots), c_int64(capacity), N.ptr(counts), N.stream_ptr())
        assert [int(v) for v in counts.cpu().numpy()] == [AX.VARIANTS * len(kept), AX.VARIANTS * closed], name
        k = AX.VARIANTS * len(kept)
        entries, data = lst.cpu().numpy().reshape(-1, 4), slots.cpu().numpy().reshape(capacity, -1)
        assert (entries[k:] == -7).all() and (data[k:] == 0xAA).all(), name
        got = sorted((int(v), int(s), int(at), data[i, : int(nb)].tobytes(), bool((data[i, int(nb) :] == 0).all()))
                     for i, (v, s, at, nb) in enumerate(entries[:k]))
        want = sorted((v, s, int(plan.instant(s, v % 8)), raw, True) for v in range(AX.VARIANTS) for s, raw in kept)
        assert got == want, name


def test_reset_starts_a_new_run(A):
    """``ChannelDemod.reset`` also clears the AFSK history, position, stored plane and discriminator state: a reused
    demodulator decodes its second stream as a fresh one does."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.processing import ChannelDemod

    fs = 96_000.0
    first = D.to_device(_stream(fs, seed=21)[:150_000], "complex64")
    second = D.to_device(M.modulate(M.hdlc_bits([_raw(2)]), fs, space_gain=2.0, sigma=0.1, seed=4), "complex64")

    def run(dem, z):
        dem.process(z, np.array([0], dtype=np.int64), D.empty(int(z.numel()), "float32"))

    used = ChannelDemod("nfm", fs, deemph_us=300.0, agc_enabled=True, ax25=True)
    run(used, first)
    used.reset()
    run(used, second)
    fresh = ChannelDemod("nfm", fs, deemph_us=300.0, agc_enabled=True, ax25=True)
    run(fresh, second)
    assert used.side["ax25"].pos == fresh.side["ax25"].pos == int(second.numel())
    a, b = used.side["ax25"].finish(), fresh.side["ax25"].finish()
    assert len(b["start"]) >= 1
    for key in ("variant", "s", "start", "nbytes", "data"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert [f.line() for f in used.side_result("ax25").frames] == [f.line() for f in fresh.side_result("ax25").frames] == _lines()[2:]
    with pytest.raises(ValueError, match="ax25"):
        ChannelDemod("am", fs, deemph_us=300.0, agc_enabled=True, ax25=True)


def _capture(fs=2.4e6, secs=3.0, seed=17):
    """int16 I/Q: an APRS channel at +300 kHz (a flat transmission of two frames, then a pre-emphasised one), a 1200-baud
    POCSAG channel at -500 kHz, an NFM voice carrier (1 kHz tone, 3 kHz deviation) at +800 kHz; every transmitter is keyed
    from the first sample, so that the mixer-sign probe sees it; complex noise 40 dB below a carrier."""
    n = int(round(fs * secs))
    t = np.arange(n, dtype=np.float64) / fs
    amp = 0.28
    x = np.zeros(n, dtype=np.complex128)
    keyed = np.ones(n, dtype=np.complex128)
    at = int(0.2 * fs)
    for frames, gain in (([_raw(0), _raw(1)], 1.0), ([_raw(2)], 2.0)):
        b = M.modulate(M.hdlc_bits(frames), fs, space_gain=gain, lead=0, tail=0).astype(np.complex128)
        keyed[at : at + b.size] = b
        at += b.size + int(0.1 * fs)
    assert at < n
    x += amp * keyed * np.exp(2j * np.pi * 300e3 * t)
    pager = np.ones(n, dtype=np.complex128)
    b = PM.modulate(PM.transmission_bits(PAGES), fs, 1200, lead=0, tail=0).astype(np.complex128)
    pager[int(0.3 * fs) : int(0.3 * fs) + b.size] = b[: n - int(0.3 * fs)]
    x += amp * pager * np.exp(2j * np.pi * -500e3 * t)
    x += amp * np.exp(1j * (2 * np.pi * 800e3 * t + 2 * np.pi * 3000.0 / fs * np.cumsum(np.sin(2 * np.pi * 1000.0 * t))))
    rng = np.random.default_rng(seed)
    std = amp * math.sqrt(1e-4 / 2.0)
    x += std * (rng.normal(size=n) + 1j * rng.normal(size=n))
    iq = np.column_stack((x.real, x.imag))
    return np.rint(np.clip(iq, -0.999, 0.999) * 32767.0).astype(np.int16)


def _count_calls(monkeypatch, prefix="iqa_afsk_"):
    from iq_to_audio_amd import _native

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith(prefix):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    return calls


def test_end_to_end_three_targets(A, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import cli, iqio

    fs, fc = 2.4e6, 144.5e6
    raw = _capture(fs)
    freqs = [fc + 300e3, fc - 500e3, fc + 800e3]
    outs = {}
    calls = _count_calls(monkeypatch)
    for tag, extra in (("plain", []), ("ax25", ["--ax25"]), ("pocsag", ["--pocsag"]), ("both", ["--ax25", "--pocsag"])):
        d = tmp_path / tag
        d.mkdir()
        wav = d / "packet_144500000Hz.wav"
        iqio.write_wav_iq(wav, raw, int(fs), "s16")
        argv = ["--in", str(wav), "--demod", "nfm", *extra]
        for f in freqs:
            argv += ["--ft", str(f)]
        before = len(calls)
        assert cli.main(argv) == 0
        outs[tag] = [d / f"audio_{int(f)}_48k.wav" for f in freqs]
        if "--ax25" not in extra:
            assert len(calls) == before  # a run without --ax25 calls no AFSK entry point
            assert not list(d.glob("*.ax25.json"))
        else:
            assert {"iqa_afsk_correlate", "iqa_afsk_bits", "iqa_afsk_frames"} <= set(calls[before:])
        if tag == "ax25":
            printed = capsys.readouterr().out
        else:
            capsys.readouterr()
    for tag in ("ax25", "pocsag", "both"):
        for a, b in zip(outs["plain"], outs[tag]):
            assert a.read_bytes() == b.read_bytes()  # the audio does not change
    for tag in ("ax25", "both"):
        js = [json.loads(p.with_name(p.stem + ".ax25.json").read_text()) for p in outs[tag]]
        print(tag, "targets:", js)
        assert js[1] is None and js[2] is None  # the pager and the voice carrier
        assert [(f["source"], f["dest"], f["path"], f["info"]) for f in js[0]["frames"]] == [(s, d, p, i) for s, d, p, i in FRAMES]
        assert [f["raw"] for f in js[0]["frames"]] == [_raw(k).hex() for k in range(3)]
        assert all(f["control"] == 3 and f["pid"] == 0xF0 and f["hits"] >= 1 for f in js[0]["frames"]) and js[0]["rejected"] == 0
        assert js[0]["crc_ok"] == sum(f["hits"] for f in js[0]["frames"]) <= js[0]["candidates"]
        times = [f["time_s"] for f in js[0]["frames"]]
        assert times == sorted(times) and 0.2 < times[0] < 0.7
    for line in _lines():
        assert f"{freqs[0]:.0f} Hz: AX25 {line}" in printed
    assert "AX25" not in "".join(l for l in printed.splitlines() if not l.startswith(f"{freqs[0]:.0f} Hz"))
    # --ax25 beside --pocsag leaves the POCSAG results as they are
    for a, b in zip(outs["pocsag"], outs["both"]):
        one, two = (p.with_name(p.stem + ".pocsag.json").read_text() for p in (a, b))
        assert one == two
    pager = json.loads(outs["both"][1].with_name(outs["both"][1].stem + ".pocsag.json").read_text())
    assert [(m["address"], m["function"], m["text"]) for m in pager["messages"]] == [(a, f, PM.shown(f, t)) for a, f, t in PAGES]


def test_pipeline_surface(A, tmp_path, monkeypatch):
    from iq_to_audio_amd import iqio
    from iq_to_audio_amd.batch import ResidentBankRunner

    fs, fc = 2.4e6, 144.5e6
    wav = tmp_path / "packet_144500000Hz.wav"
    iqio.write_wav_iq(wav, _capture(fs, 2.6), int(fs), "s16")

    def cfgs(tag):
        return [A.ProcessingConfig(in_path=wav, target_freq=f, demod_mode="nfm", chunk_size=65_536, output_path=tmp_path / f"{tag}{i}.wav")
                for i, f in enumerate((fc + 300e3, fc + 800e3))]

    calls = _count_calls(monkeypatch)

    def several_blocks(pipe):
        for o in getattr(pipe, "owners", [pipe]):
            o.block_frames_target = 1_048_576  # several device blocks: the carried history is exercised
        return pipe

    plain = several_blocks(A.MultiChannelPipeline(cfgs("p")))
    plain.run()
    assert calls == [] and plain.ax25 == [None, None]
    multi = several_blocks(A.MultiChannelPipeline(cfgs("m"), ax25=True))
    multi.run()
    assert multi.ax25[1] is None and multi.ax25[0] is multi.owners[0].ax25
    assert [f.line() for f in multi.ax25[0].frames] == _lines()
    assert calls.count("iqa_afsk_correlate") >= 2 * 5 and calls.count("iqa_afsk_bits") == 2
    one = A.ProcessingPipeline(cfgs("o")[0], ax25=True)
    one.run()
    assert [f.line() for f in one.ax25.frames] == _lines()
    assert [f.raw for f in one.ax25.frames] == [f.raw for f in multi.ax25[0].frames]
    for i in range(2):
        assert (tmp_path / f"p{i}.wav").read_bytes() == (tmp_path / f"m{i}.wav").read_bytes()
    with pytest.raises(ValueError, match="ax25"):
        ResidentBankRunner([dict(freq_offset=300e3)], sample_rate=fs, n_frames=1 << 20, ax25=True)
