"""POCSAG beside narrowband FM (--demod nfm --pocsag), the host side: the protocol constants against each other, the numpy
oracle (tests/pocsag_model.py) round trip over baud rates, channel rates, polarities, tuning and clock errors and noise,
no decode from noise, the batch parser on synthetic codewords, the plan, CLI and pipeline validation.  No GPU compute."""
from __future__ import annotations

import importlib.util
import itertools
import sys
from ctypes import c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest

import iq_to_audio_amd as A
from iq_to_audio_amd import dsp_plan as P
from iq_to_audio_amd.decoders import pocsag as PG


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

# Complex noise per component against a carrier of 1 (11 dB carrier to noise in the whole channel rate).  Settled on the
# CPU: the oracle alone decodes every case below at 0.25 with these seeds; 0.2 keeps a margin.
SIGMA = 0.2
MESSAGES = [(1234567, 3, "Pump 4 pressure low, call 0171 5550123"), (424242, 0, "0123456789"), (77, 1, "ok")]
SHORT = MESSAGES[1:]


# ---- constants -----------------------------------------------------------------------------------------------------------


def test_constants_check_each_other():
    """g = 0x769: the sync word and the idle word have zero syndrome, even parity and 16 one-bits, and every single-bit
    error of either is caught; a codeword the model builds has zero syndrome and each of its 32 single-bit errors corrects
    back to it.  Double-bit errors: all 496 of a codeword get status 2 (two flips leave the parity even, and only odd
    words are corrected), so 100 % are refused and 0 % are mis-corrected to a different word."""
    assert (PG.SYNC_WORD, PG.IDLE_WORD, PG.BCH_POLY, PG.NUMERIC) == (M.SYNC, M.IDLE, M.G, M.NUMERIC) == (0x7CD215D8, 0x7A89C197, 0x769, "0123456789*U -][")
    for word in (M.SYNC, M.IDLE):
        assert M.syndrome(word) == 0 and M.parity(word) == 0 and bin(word).count("1") == 16
        for bit in range(32):
            bad = word ^ (1 << bit)
            assert M.syndrome(bad) != 0 or M.parity(bad) == 1
            assert M.correct(bad) == (word, 1)
    assert len(M.SINGLE) == 31 and 0 not in M.SINGLE
    assert M.SYNC ^ 0xFFFFFFFF == 0x832DEA27
    for cw in (M.address_word(1234567, 3), M.message_word(0xABCDE), M.message_word(0)):
        assert M.syndrome(cw) == 0 and M.parity(cw) == 0 and M.correct(cw) == (cw, 0)
        for bit in range(32):
            assert M.correct(cw ^ (1 << bit)) == (cw, 1)
        refused = wrong = 0
        for i, j in itertools.combinations(range(32), 2):
            w, st = M.correct(cw ^ (1 << i) ^ (1 << j))
            assert st == 2 or w != cw
            refused += st == 2
            wrong += st != 2
        print(f"double-bit errors of {cw:08X}: {refused} refused, {wrong} corrected to another word")
        assert (refused, wrong) == (496, 0)


# ---- the oracle ----------------------------------------------------------------------------------------------------------


def _batches_for_parser(out: dict) -> dict:
    return {baud: dict(n0=[k[0] for k in kept], sigma=[k[1] for k in kept], inverted=[k[2] for k in kept],
                       words=out["batches"][baud]["words"], status=out["batches"][baud]["status"])
            for baud, kept in out["syncs"].items()}


@pytest.mark.parametrize("inverted", [False, True])
@pytest.mark.parametrize("fs", [96_000.0, 96_153.846])
@pytest.mark.parametrize("baud", [512, 1200, 2400])
def test_oracle_round_trip(baud, fs, inverted):
    """Every message comes back identical (address, function, text) through the oracle AND through the package's parser
    on the oracle's codewords: carrier +-1.5 kHz off tune, bit clock +-50 ppm, clean and at SIGMA."""
    messages = SHORT if baud == 512 else MESSAGES
    sent = [(a, f, M.shown(f, t)) for a, f, t in messages]
    bits = M.transmission_bits(messages)
    plan = P.plan_pocsag(fs)
    for k, (offset, ppm, sigma) in enumerate([(1500.0, 50.0, 0.0), (-1500.0, -50.0, SIGMA), (1500.0, -50.0, SIGMA), (-1500.0, 50.0, 0.0)]):
        z = M.modulate(bits, fs, baud, inverted=inverted, offset_hz=offset, ppm=ppm, sigma=sigma, seed=100 * baud + k)
        out = M.oracle(M.theta_of(z), fs)
        assert M.triples(out["messages"]) == sent, (offset, ppm, sigma)
        assert all(m["baud"] == baud and m["inverted"] == inverted for m in out["messages"])
        assert {b: len(v) for b, v in out["syncs"].items()} == {b: len(M.batches_of(messages)) if b == baud else 0 for b in M.BAUDS}
        res = PG.parse_batches(plan, _batches_for_parser(out))
        assert M.triples(res.messages) == sent and res.bauds_skipped == []
        assert [(m.time_s, m.baud, m.inverted, m.corrected, m.batches, m.payload_bits) for m in res.messages] == [
            (m["time_s"], m["baud"], m["inverted"], m["corrected"], m["batches"], m["payload_bits"]) for m in out["messages"]]
        assert abs(res.dc_hz - offset) < 60.0, res.dc_hz  # the tuning error, seen through the sync words
        if sigma == 0.0:
            assert res.codewords == dict(ok=16 * len(M.batches_of(messages)), corrected=0, uncorrectable=0, absent=0)


@pytest.mark.parametrize("fs", [96_000.0, 96_153.846])
def test_noise_decodes_nothing(fs):
    """Carrier-less noise as long as the longest round-trip stream: no kept sync at any baud, so the result is None.  With
    these seeds not one position of 3 x 420 000 comes within two bits of the sync word, so the eye gate has nothing to
    remove here; on a real transmission it removes about one in seven of the near positions (the timing skirts)."""
    stats: dict = {}
    for seed in (0, 1):
        out = M.oracle(M.theta_of(M.noise_only(420_000, SIGMA, seed)), fs, stats=stats)
        assert all(len(v) == 0 for v in out["syncs"].values())
        assert PG.parse_batches(P.plan_pocsag(fs), _batches_for_parser(out)) is None
    print("noise:", stats)
    z = M.modulate(M.transmission_bits(MESSAGES), fs, 1200, sigma=SIGMA, seed=3)
    stats = {}
    M.oracle(M.theta_of(z), fs, stats=stats)
    print("signal:", stats)
    assert 0 < stats["gated"] < stats["near"]


def test_eye_gate_and_local_maximum_on_a_hand_made_plane():
    """The search on a synthetic integrator plane: an exact sync pattern is kept once, at its strongest position; a copy
    with one weak bit (under a quarter of the mean eye) is refused; the inverted pattern is kept as inverted."""
    bp = M.baud_plan(96_000.0, 1200)
    S = np.zeros(40_000, dtype=np.int64)

    def put(n0, word, amp, weak=None):
        for i in range(32):
            a = amp // 8 if i == weak else amp
            S[n0 + int(bp["off"][i])] = 1000 + (-a if (word >> (31 - i)) & 1 else a)

    put(5000, M.SYNC, 50_000)
    put(5003, M.SYNC, 40_000)  # the same sync three samples late and weaker: within h, not kept
    put(15_000, M.SYNC, 50_000, weak=7)
    put(25_000, M.SYNC ^ 0xFFFFFFFF, 50_000)
    kept = M.sync_search(S, bp)
    assert [(k[0], k[2], k[3]) for k in kept] == [(5000, False, 0), (25_000, True, 0)]
    assert kept[0][1] == 32 * 1000


# ---- the parser ----------------------------------------------------------------------------------------------------------


def _parse(batches, n0=None, status=None, fs=96_000.0, baud=1200):
    plan = P.plan_pocsag(fs)
    pb = next(b for b in plan.bauds if b.baud == baud)
    k = len(batches)
    n0 = [1000 + i * int(pb.offsets[544]) for i in range(k)] if n0 is None else n0
    status = np.zeros((k, 16), dtype=np.uint8) if status is None else np.asarray(status, dtype=np.uint8)
    got = {baud: dict(n0=n0, sigma=[0] * k, inverted=[False] * k, words=np.array(batches, dtype=np.uint32), status=status)}
    return PG.parse_batches(plan, got), pb


def test_parser_numeric_alpha_and_frames():
    res, pb = _parse(M.batches_of([(8 * 1000 + 2, 0, "12*U -]["), (8 * 2000 + 5, 2, "Hi~")]))
    assert M.triples(res.messages) == [(8002, 0, "12*U -][  "), (16005, 2, "Hi~")]
    assert [m.kind for m in res.messages] == ["numeric", "alpha"] and res.messages[0].payload_bits == 40
    assert res.messages[0].time_s == (1000 + int(pb.offsets[32 * (1 + 4)])) / 96_000.0
    assert res.messages[0].payload == "".join(f"{int(''.join(map(str, M.numeric_bits('12*U -][  ')[i:i + 4])), 2):x}" for i in range(0, 40, 4))
    assert res.codewords == dict(ok=16, corrected=0, uncorrectable=0, absent=0) and res.syncs == {512: 0, 1200: 1, 2400: 0}
    for frame in range(8):  # the three low address bits are the frame the codeword sits in
        res, _ = _parse(M.batches_of([(0x1FFFF8 - 8 * frame + frame, 1, "a")]))
        assert M.triples(res.messages) == [(0x1FFFF8 - 8 * frame + frame, 1, "a")]
    res, _ = _parse(M.batches_of([(9, 1, "caf\x7f\x01!")]))
    assert res.messages[0].text == "caf��!"
    res, _ = _parse(M.batches_of([(9, 3, "end\x03\x04")]))
    assert res.messages[0].text == "end"


def test_parser_across_batches_cuts_and_orphans():
    long_text = "From frame seven on into the next batch."
    assert len(long_text) == 40  # 14 codewords: one in the first batch, 13 in the second
    batches = M.batches_of([(7, 3, long_text)])
    assert len(batches) == 2
    res, pb = _parse(batches)
    assert M.triples(res.messages) == [(7, 3, long_text)] and res.messages[0].batches == 2 and res.orphans == 0
    # the second batch does not continue the first (half a bit and one sample late): the message closes, the rest is orphaned
    late = [1000, 1000 + int(pb.offsets[544]) + pb.h + 1]
    res, _ = _parse(batches, n0=late)
    assert len(res.messages) == 1 and res.messages[0].text == long_text[:2] and res.messages[0].batches == 1
    assert res.orphans == sum(1 for w in batches[1] if w >> 31)
    on_time = [1000, 1000 + int(pb.offsets[544]) + pb.h]
    assert M.triples(_parse(batches, n0=on_time)[0].messages) == [(7, 3, long_text)]
    # an uncorrectable codeword cuts the message; what follows it is orphaned; a corrected one is counted
    status = np.zeros((2, 16), dtype=np.uint8)
    status[1, 2], status[1, 0] = 2, 1
    res, _ = _parse(batches, status=status)
    assert len(res.messages) == 1 and res.messages[0].payload_bits == 20 * 3 and res.messages[0].corrected == 1
    assert res.messages[0].text == long_text[:8] and res.codewords["uncorrectable"] == 1 and res.codewords["corrected"] == 1
    assert res.orphans == sum(1 for w in batches[1][3:] if w >> 31)
    status[:] = 0
    status[1, :] = 3  # the stream ends inside the second batch
    res, _ = _parse(batches, status=status)
    assert res.messages[0].text == long_text[:2] and res.codewords["absent"] == 16 and res.orphans == 0
    # a new address closes the open message; batches arrive in any order
    two = M.batches_of([(3, 0, "11111"), (3, 0, "22222")])
    res, _ = _parse(two)
    assert M.triples(res.messages) == [(3, 0, "11111"), (3, 0, "22222")]
    res, _ = _parse(batches[::-1], n0=[1000 + int(pb.offsets[544]), 1000])
    assert M.triples(res.messages) == [(7, 3, long_text)]
    assert PG.parse_batches(P.plan_pocsag(96_000.0), {}) is None


# ---- the host surface ----------------------------------------------------------------------------------------------------


def test_plan():
    for fs in (96_000.0, 10e6 / 104):
        plan = P.plan_pocsag(fs)
        assert [b.baud for b in plan.bauds] == [512, 1200, 2400] and plan.skipped == ()
        for b in plan.bauds:
            want = M.baud_plan(fs, b.baud)
            assert (b.sps, b.L, b.h) == (want["sps"], want["L"], want["h"]) and b.offsets.dtype == np.int32
            np.testing.assert_array_equal(b.offsets, want["off"])
        assert plan.hist_len == plan.bauds[0].L - 1 == round(fs / 512) - 1 and plan.lengths() == tuple(b.L for b in plan.bauds)
    low = P.plan_pocsag(12_000.0)
    assert low.skipped == (2400,) and [b.baud for b in low.bauds] == [512, 1200] and low.lengths() == (23, 10, 0)
    assert P.plan_pocsag(400_000.0).skipped == (512,)
    with pytest.raises(ValueError, match="POCSAG"):
        P.plan_pocsag(3_000.0)
    assert P.POCSAG_MAX_SPS >= 256


def test_cli_and_pipeline_validation(tmp_path, capsys):
    from iq_to_audio_amd import cli
    from iq_to_audio_amd.batch import ResidentBankRunner, ResidentCaptureRunner, demodulate_sharded

    with pytest.raises(SystemExit) as exc:
        cli.main(["--in", str(tmp_path / "x.wav"), "--ft", "1e6", "--pocsag", "--demod", "am"])
    assert exc.value.code == 2 and "--pocsag needs --demod nfm" in capsys.readouterr().err
    assert cli.build_parser().parse_args(["--in", "x.wav"]).pocsag is False
    wfm = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="wfm")
    nfm = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="nfm")
    with pytest.raises(ValueError, match="pocsag"):
        A.ProcessingPipeline(wfm, pocsag=True)
    with pytest.raises(ValueError, match="pocsag"):
        A.MultiChannelPipeline([nfm, wfm], pocsag=True)
    assert A.ProcessingPipeline(nfm, pocsag=True).pocsag_enabled and not A.ProcessingPipeline(nfm).pocsag_enabled
    assert all(o.pocsag_enabled for o in A.MultiChannelPipeline([nfm, nfm], pocsag=True).owners)
    assert len(A.ProcessingConfig.__dataclass_fields__) == 23
    with pytest.raises(ValueError, match="pocsag"):
        ResidentBankRunner([dict(freq_offset=25e3)], sample_rate=2.5e6, n_frames=1 << 20, pocsag=True)
    with pytest.raises(ValueError, match="pocsag"):
        ResidentCaptureRunner(np.ones(8), sample_rate=2.5e6, freq_offset=25e3, decimation=26, fs_channel=2.5e6 / 26, chunk=1 << 20,
                              n_frames=1 << 20, pocsag=True)
    with pytest.raises(ValueError, match="pocsag"):
        demodulate_sharded([dict(freq_offset=25e3)], sample_rate=2.5e6, n_frames=1 << 20, axis="channels", pocsag=True)


def test_c_abi_refuses_bad_arguments():
    """The argument checks come before any launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null = c_void_p(0)
    windows = (c_int32 * 3)(188, 80, 40)
    outs = (c_void_p * 3)(8, 8, 8)  # (never dereferenced: every call below is refused before a launch)
    with pytest.raises(ValueError, match="hist_len"):
        N.call("iqa_pocsag_integrate", null, c_int64(16), null, c_int32(10), windows, null, outs, null)
    with pytest.raises(ValueError, match="window"):
        N.call("iqa_pocsag_integrate", null, c_int64(16), null, c_int32(10), (c_int32 * 3)(0, 0, 385), null, outs, null)
    with pytest.raises(ValueError, match="no active baud"):
        N.call("iqa_pocsag_integrate", null, c_int64(16), null, c_int32(10), (c_int32 * 3)(0, 0, 0), null, outs, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_pocsag_integrate", null, c_int64(16), null, c_int32(187), windows, null, outs, null)
    N.call("iqa_pocsag_integrate", null, c_int64(0), null, c_int32(187), windows, null, outs, null)  # nothing to do
    offs = (c_int32 * 32)(*range(0, 32 * 80, 80))
    with pytest.raises(ValueError, match="ascend"):
        N.call("iqa_pocsag_sync", null, c_int64(8), (c_int32 * 32)(*range(31, -1, -1)), c_int32(40), null, null, c_int64(0), c_void_p(8), null)
    with pytest.raises(ValueError, match="offsets"):
        N.call("iqa_pocsag_sync", null, c_int64(8), (c_int32 * 32)(*range(0, 32 * 400, 400)), c_int32(40), null, null, c_int64(0), c_void_p(8), null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_pocsag_sync", null, c_int64(8), offs, c_int32(40), null, null, c_int64(0), null, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_pocsag_codewords", null, c_int64(8), null, c_int64(1), null, null, null, null, null)
    N.call("iqa_pocsag_codewords", null, c_int64(8), null, c_int64(0), null, null, null, null, null)
