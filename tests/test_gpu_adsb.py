"""ADS-B / Mode S beside AM (--demod am --adsb) on the MI355X: every integer stage identical to the numpy oracle of
tests/adsb_model.py, the search at its edge shapes, block invariance bit for bit, the search entry on hand-made q planes,
the bounded kept list, the CLI end to end on a capture with a squitter channel and an empty one, and the proof that a run
without --adsb calls no ADS-B entry point."""
from __future__ import annotations

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


M = _load("adsb_model")

TILE = 2048  # IQA_ADSB_TILE: candidate positions of one workgroup of iqa_adsb_search


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    from iq_to_audio_amd.decoders import adsb as AD

    assert AD.TILE == TILE
    return pkg


def _same_as_oracle(dec, fs):
    """flags, the sorted records, both counters and the parsed messages equal the oracle's from the GPU's own q."""
    st = dec.stages()
    assert st["q"].dtype == np.uint16 and st["e"].dtype == np.float32 and st["flags"].dtype == np.uint8
    np.testing.assert_array_equal(st["q"], M.quantise(st["e"]))
    want = M.oracle(fs, st["q"])
    np.testing.assert_array_equal(st["flags"], want["flags"])
    assert st["records"] == want["records"]
    assert st["candidates"] == want["candidates"] == int(st["flags"].sum())
    res = dec.finish()
    got = [] if res is None else res.messages
    assert [tuple(getattr(m, k) for k in M.FIELDS) for m in got] == [tuple(m[k] for k in M.FIELDS) for m in want["messages"]]
    if res is not None:
        assert res.aircraft == want["aircraft"] and (res.candidates, res.crc_ok) == (want["candidates"], len(want["records"]))
    return st, want


@pytest.mark.parametrize("fs", M.RATES)
def test_stages_are_the_oracles(A, fs):
    from iq_to_audio_amd.decoders.adsb import AdsbDecoder

    for frac in (0.0, 0.25):
        for sigma in (0.0, 0.1):
            z, _ = M.stream(fs, frac, 50e3, sigma)
            assert z.size <= 300_000
            dec = AdsbDecoder(fs)
            dec.process(z)
            st, want = _same_as_oracle(dec, fs)
            e_np = M.envelope(z)
            differ = st["e"] != e_np
            dq = np.abs(st["q"].astype(np.int64) - M.quantise(e_np).astype(np.int64))
            print(f"fs {fs} frac {frac} sigma {sigma}: e against numpy's |z|: {np.mean(differ):.4%} of {differ.size} samples differ, "
                  f"max |de| {np.abs(st['e'].astype(np.float64) - e_np).max():.3g}, max |dq| {dq.max()}; records {len(want['records'])}, "
                  f"candidates {want['candidates']}")
            assert dq.max() <= 1  # one float32 ulp of e is at most 2^-8 in x
            kept = {r[3] for r in want["records"]}
            assert kept <= set(M.FOUR)
            if frac == 0.0 or fs >= 4e6:
                assert kept == set(M.FOUR)


@pytest.mark.parametrize("fs", [2.0e6, 2.5e6, 4.0e6, 20.0e6])
def test_search_edge_shapes(A, fs):
    """h = 1, 1, 2 and 10.  N = span - 1: nothing; N = span: one position, a frame at 0 ending exactly at N; position counts
    T - 1, T, T + 1, 2 T + 1; a frame at T - 1, T - 8 and T - span / 2 (the preamble in one tile, the data in the next)."""
    from iq_to_audio_amd.decoders.adsb import AdsbDecoder

    pl = M.plan(fs)
    span = pl["span"]
    assert pl["h"] == {2.0e6: 1, 2.5e6: 1, 4.0e6: 2, 20.0e6: 10}[fs]

    def run(n, starts, sigma=0.05):
        z, _ = M.stream(fs, 0.0, 0.0, sigma, frames=[M.IDENT] * len(starts), start=starts)
        z = np.concatenate((z, np.zeros(max(n - z.size, 0), dtype=np.complex64)))[:n]
        dec = AdsbDecoder(fs)
        dec.process(z)
        st, want = _same_as_oracle(dec, fs)
        assert st["flags"].size == max(n - span + 1, 0)
        return want

    assert run(span - 1, [0], 0.0)["records"] == [] and run(span - 1, [0])["flags"].size == 0
    one = run(span, [0], 0.0)
    assert [(r[0], r[1], r[3]) for r in one["records"]] == [(0, 112, M.IDENT)] and one["flags"].tolist() == [1]
    for npos in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        starts = [0, npos - 1] if npos - 1 >= span + 8 else [npos - 1]  # a frame at the last position: it ends exactly at N
        want = run(npos + span - 1, starts)
        assert {r[0] for r in want["records"]} >= set(starts)
    for s in (TILE - 1, TILE - 8, TILE - span // 2):
        want = run(2 * TILE + 1 + span - 1, [s])
        assert s in {r[0] for r in want["records"]}


def test_block_cuts(A):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.decoders.adsb import AdsbDecoder

    fs = 4e6
    z_np, _ = M.stream(fs, 0.25, 50e3, 0.1)
    z = D.to_device(z_np, "complex64")
    n = int(z.numel())
    small = 700  # blocks of 1 and of 7 over the start of the stream, larger ones behind it
    ragged = [0, 1, 2, 30, 31, 1000, 1001, n - 7, n]
    cuts = [[0, n], list(range(0, small)) + [small, n], list(range(0, small, 7)) + [small, n], list(range(0, n, 4096)) + [n], ragged]
    runs = []
    for c in cuts:
        dec = AdsbDecoder(fs)
        for lo, hi in zip(c[:-1], c[1:]):
            dec.process(z[lo:hi])
        assert dec.core.pos == n
        runs.append(dec.stages())
    assert len(runs[0]["records"]) >= 4
    for st in runs[1:]:
        for key in ("e", "q", "flags"):
            np.testing.assert_array_equal(st[key], runs[0][key], err_msg=key)
        assert (st["records"], st["candidates"]) == (runs[0]["records"], runs[0]["candidates"])
    dec = AdsbDecoder(fs)  # an envelope block in place of a complex one
    dec.process(runs[0]["e"][:1000])
    dec.process(D.to_device(runs[0]["e"][1000:], "float32"))
    np.testing.assert_array_equal(dec.stages()["q"], runs[0]["q"])
    assert dec.stages()["records"] == runs[0]["records"]


# ---- the search entry on hand-made q planes ----------------------------------------------------------------------------------

HI, LO = 39_000, 1_000


def _plane(frame: bytes, lead: int = 3) -> np.ndarray:
    """A q plane at 2 MHz (h = 1, o[k] = k, span = 240): the frame's chips at ``lead``, HI where the pulse is, LO elsewhere."""
    q = np.full(lead + 240 + 5, LO, dtype=np.uint16)
    a = M.chips_of(frame)
    q[lead : lead + a.size][a > 0] = HI
    return q


def _search(q: np.ndarray, capacity: int = 8):
    """One ``iqa_adsb_search`` call at 2 MHz with every output behind a guard -> (flags, counts, sorted records, raw slots)."""
    from ctypes import POINTER, c_int32, c_int64

    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import _native as N
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.decoders import adsb as AD

    core = AD.AdsbCore(P.plan_adsb(2e6))
    npos = max(q.size - 240 + 1, 0)
    flags = D.from_numpy(np.full(npos + 16, 0xAA, dtype=np.uint8))
    counts = D.from_numpy(np.array([99, 99], dtype=np.int64))
    lst = D.from_numpy(np.full(3 * capacity, -7, dtype=np.int64))
    slots = D.from_numpy(np.full(14 * capacity, 0xAA, dtype=np.uint8))
    N.call("iqa_adsb_search", N.ptr(D.from_numpy(q.view(np.int16))), c_int64(q.size), N.ptr(core._offsets),
           core._offsets_host.ctypes.data_as(POINTER(c_int32)), c_int32(1), c_int32(240), N.ptr(flags), N.ptr(lst), N.ptr(slots),
           c_int64(capacity), N.ptr(counts), N.stream_ptr())
    f = flags.cpu().numpy()
    assert (f[npos:] == 0xAA).all()
    kept, passed = (int(v) for v in counts.cpu().numpy())
    entries, data = lst.cpu().numpy().reshape(-1, 3), slots.cpu().numpy().reshape(capacity, 14)
    k = min(kept, capacity)
    assert (entries[k:] == -7).all() and (data[k:] == 0xAA).all()
    want = M.search(q, M.plan(2e6))
    np.testing.assert_array_equal(f[:npos], want["flags"])
    assert passed == want["candidates"] and kept == len(want["records"])
    recs = sorted((int(e[0]), int(e[1]), int(e[2]), data[i].tobytes()) for i, e in enumerate(entries[:k]))
    if kept <= capacity:
        assert recs == [(p, nb, lv, raw.ljust(14, b"\0")) for p, nb, lv, raw in want["records"]]
    return f[:npos], (kept, passed), recs


def test_search_on_hand_made_planes(A):
    lead = 3
    base = _plane(M.IDENT, lead)
    flags, counts, recs = _search(base)
    assert counts == (1, 1) and flags[lead] == 1 and recs == [(lead, 112, 4 * HI, M.IDENT)]
    # a tie on each strict inequality fails; one less on the smaller side passes
    for big, small in ((0, 1), (2, 1), (2, 3), (7, 6), (7, 8), (9, 8), (9, 10)):
        q = base.copy()
        q[lead + small] = HI
        assert _search(q)[0][lead] == 0, (big, small)
        q[lead + small] = HI - 1
        assert _search(q)[0][lead] == 1, (big, small)
    assert (4 * HI) % 6 == 0
    for j in (4, 5, 11, 12, 13, 14):
        q = base.copy()
        q[lead + j] = 4 * HI // 6
        assert _search(q)[0][lead] == 0, j
        q[lead + j] = 4 * HI // 6 - 1
        assert _search(q)[0][lead] == 1, j
    # a flat plane, at full scale and at zero: no candidate
    for level in (65535, 0):
        flags, counts, recs = _search(np.full(3 * TILE, level, dtype=np.uint16))
        assert counts == (0, 0) and not flags.any() and recs == []
    # a bit tie reads as 0: on a 0 bit the frame survives, on a 1 bit the check fails
    bits = np.unpackbits(np.frombuffer(M.IDENT, dtype=np.uint8))
    zero, one = int(np.flatnonzero(bits == 0)[7]), int(np.flatnonzero(bits == 1)[7])
    q = base.copy()
    q[lead + 16 + 2 * zero] = HI
    assert _search(q)[2] == [(lead, 112, 4 * HI, M.IDENT)]
    q = base.copy()
    q[lead + 16 + 2 * one + 1] = HI
    assert _search(q)[1] == (0, 1)
    # a frame with syndrome 0 and DF 19 passes the preamble rule and is dropped
    df19 = M.build_frame(19, 0x4840D6, 0x123456789ABCDE)
    assert M.syndrome(df19) == 0
    assert _search(_plane(df19))[1] == (0, 1)
    # a 56-bit DF11 is kept, its slot zero-padded whatever lies behind the frame
    q = _plane(M.DF11)
    q[lead + 16 + 112 :] = np.random.default_rng(3).integers(0, 30_000, size=q.size - (lead + 128)).astype(np.uint16)
    assert _search(q)[2] == [(lead, 56, 4 * HI, M.DF11 + bytes(7))]


def test_quantiser_values(A):
    from iq_to_audio_amd.decoders.adsb import AdsbDecoder

    e = np.array([np.nan, np.inf, 3.0e38, 1.0, 65535.0 / 65536.0, 65534.5 / 65536.0, 65533.5 / 65536.0, 0.5, 2.0 ** -17, 1.5 * 2.0 ** -16,
                  2.5 * 2.0 ** -16, 0.0, 2.0 ** -140], dtype=np.float32)
    dec = AdsbDecoder(2e6)
    dec.process(e)
    q = dec.stages()["q"]
    assert q.tolist() == [65535, 65535, 65535, 65535, 65535, 65534, 65534, 32768, 0, 2, 2, 0, 0]
    np.testing.assert_array_equal(q, M.quantise(e))


def test_kept_list_overflow_is_repeated_not_truncated(A):
    from iq_to_audio_amd.decoders import adsb as AD

    fs = 2e6
    z, _ = M.stream(fs, 0.0, 0.0, 0.05, frames=[M.IDENT, M.POS_EVEN, M.POS_ODD])
    roomy, tight = AD.AdsbDecoder(fs), AD.AdsbDecoder(fs)
    roomy.process(z)
    tight.process(z)
    a, b = roomy.core.finish(), tight.core.finish(capacity=1)
    assert len(a["n"]) == 3
    for key in ("n", "nbits", "P", "data"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["candidates"] == b["candidates"]
    assert [m.raw for m in AD.parse_frames(tight.plan, b, b["candidates"]).messages] == [f.hex() for f in (M.IDENT, M.POS_EVEN, M.POS_ODD)]


# ---- the pipelines and the command line ---------------------------------------------------------------------------------------


def _count_calls(monkeypatch, prefix="iqa_adsb_"):
    from iq_to_audio_amd import _native

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith(prefix):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    return calls


SENT = [M.IDENT, M.POS_ODD, M.POS_EVEN, M.DF11, M.VELOCITY]  # the four frames (the even one newer) and a velocity
LINES = ["ADS-B 4840D6 ident KLM1023", "ADS-B 40621D pos 52.25720N 3.91937E 38000ft", "ADS-B 485020 vel 159.2kn 182.9° -832fpm"]


def _capture(fs=10e6, secs=0.012, offset=3.0e6, seed=17):
    """int16 I/Q at 10 MS/s: squitters at +3 MHz from a transmitter band-limited to +-1 MHz, so that nothing of them lies at
    -0.5 MHz, nor at +0.5 MHz, where the mixer-sign probe may look (a 0.5 us pulse with hard edges reaches every channel of
    the capture, and a replica that decodes is no fault of the decoder's).  Every frame is sent five times, each time one
    input sample later against the 2 MHz grid behind the channelizer (a transponder repeats its squitters; the phase of the
    decimated grid against the pulses is the channel filter's business, not the test's)."""
    n = int(round(fs * secs))
    env = np.zeros(n, dtype=np.float64)
    at = int(0.001 * fs)
    for rep in range(5):
        for frame in SENT:
            a = np.repeat(M.chips_of(frame), 5)  # 5 input samples per half-microsecond chip
            env[at + rep : at + rep + a.size] = a
            at += 2000  # 200 us
    assert at + 2000 < n
    spec = np.fft.fft(env)
    spec[np.abs(np.fft.fftfreq(n, 1.0 / fs)) > 1.0e6] = 0.0
    env = np.fft.ifft(spec).real
    t = np.arange(n, dtype=np.float64) / fs
    x = 0.5 * env * np.exp(2j * np.pi * offset * t)
    rng = np.random.default_rng(seed)
    x += 0.002 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    iq = np.column_stack((x.real, x.imag))
    return np.rint(np.clip(iq, -0.999, 0.999) * 32767.0).astype(np.int16)


def test_end_to_end_two_targets(A, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import cli, iqio
    from iq_to_audio_amd.batch import ResidentBankRunner

    fs, fc = 10e6, 1087e6
    raw = _capture(fs)
    freqs = [fc + 3.0e6, fc - 0.5e6]
    outs = {}
    calls = _count_calls(monkeypatch)
    for tag, extra in (("plain", []), ("adsb", ["--adsb"])):
        d = tmp_path / tag
        d.mkdir()
        wav = d / "squitter_1087000000Hz.wav"
        iqio.write_wav_iq(wav, raw, int(fs), "s16")
        argv = ["--in", str(wav), "--demod", "am", "--fs-ch", "2e6", "--bw", "2e6", *extra]
        for f in freqs:
            argv += ["--ft", str(f)]
        assert cli.main(argv) == 0
        outs[tag] = [d / f"audio_{int(f)}_48k.wav" for f in freqs]
        if not extra:
            assert calls == []  # a run without --adsb calls no ADS-B entry point
            assert not list(d.glob("*.adsb.json"))
            capsys.readouterr()
    printed = capsys.readouterr().out
    assert calls.count("iqa_adsb_quantise") >= 2 and calls.count("iqa_adsb_search") >= 2
    for a, b in zip(outs["plain"], outs["adsb"]):
        assert a.read_bytes() == b.read_bytes()  # the audio does not change
    js = [json.loads(p.with_name(p.stem + ".adsb.json").read_text()) for p in outs["adsb"]]
    print("targets:", js)
    assert js[1] is None  # the empty channel
    got = js[0]["messages"]
    assert {m["raw"] for m in got} == {f.hex() for f in SENT}  # every frame, and no frame that was not sent
    assert [a["icao"] for a in js[0]["aircraft"]] == ["40621D", "4840D6", "485020"]
    assert js[0]["aircraft"][1]["callsign"] == "KLM1023" and js[0]["aircraft"][0]["altitude_ft"] == 38000
    assert js[0]["crc_ok"] == sum(m["hits"] for m in got) <= js[0]["candidates"]
    times = [m["time_s"] for m in got]
    assert times == sorted(times) and 0.0009 < times[0] < 0.0065
    for text in LINES:
        assert f"{freqs[0]:.0f} Hz: {text}" in printed
    assert "ADS-B" not in "".join(l for l in printed.splitlines() if not l.startswith(f"{freqs[0]:.0f} Hz"))
    # the pipelines
    wav = tmp_path / "plain" / "squitter_1087000000Hz.wav"
    cfgs = [A.ProcessingConfig(in_path=wav, target_freq=f, demod_mode="am", bandwidth=2e6, fs_ch_target=2e6, chunk_size=16_384,
                               output_path=tmp_path / f"m{i}.wav") for i, f in enumerate(freqs)]
    multi = A.MultiChannelPipeline(cfgs, adsb=True)
    for o in multi.owners:
        o.block_frames_target = 32_768  # several device blocks
    multi.run()
    assert multi.adsb[1] is None and multi.adsb[0] is multi.owners[0].adsb
    assert [m.raw for m in multi.adsb[0].messages] == [m["raw"] for m in got]
    with pytest.raises(ValueError, match="adsb"):
        ResidentBankRunner([dict(freq_offset=3.0e6)], sample_rate=fs, n_frames=1 << 20, adsb=True)


def test_reset_starts_a_new_run(A):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.processing import ChannelDemod

    fs = 2e6
    first = D.to_device(M.stream(fs, 0.0, 0.0, 0.05)[0], "complex64")
    second = D.to_device(M.stream(fs, 0.0, 0.0, 0.05, frames=[M.VELOCITY])[0], "complex64")

    def run(dem, z):
        out = D.empty(int(z.numel()), "float32")
        dem.process(z, np.array([0], dtype=np.int64), out)
        return out

    used = ChannelDemod("am", fs, deemph_us=300.0, agc_enabled=True, adsb=True)
    run(used, first)
    used.reset()
    audio = run(used, second)
    plain = ChannelDemod("am", fs, deemph_us=300.0, agc_enabled=True)
    np.testing.assert_array_equal(audio.cpu().numpy(), run(plain, second).cpu().numpy())
    assert used.side["adsb"].pos == int(second.numel()) and plain.side_result("adsb") is None
    assert [m.line() for m in used.side_result("adsb").messages] == [LINES[2]]
    with pytest.raises(ValueError, match="--demod am"):
        ChannelDemod("nfm", fs, deemph_us=300.0, agc_enabled=True, adsb=True)
    with pytest.raises(ValueError, match="--fs-ch"):
        ChannelDemod("am", 96_000.0, deemph_us=300.0, agc_enabled=True, adsb=True)
