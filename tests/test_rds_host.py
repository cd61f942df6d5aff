"""RDS beside wideband FM (--demod wfm --rds), the host side: the plan against its specification, the check word and
offset words, the float64 oracle chain (tests/rds_model.py) on a modelled multiplex, the group parser on synthetic words,
CLI and pipeline validation, the C ABI's argument checks.  No GPU compute here."""
from __future__ import annotations

import ctypes
import importlib.util
import math
import sys
from ctypes import c_double, c_float, c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest

import iq_to_audio_amd as A
from iq_to_audio_amd import dsp_plan as P
from iq_to_audio_amd import iqio
from iq_to_audio_amd.decoders import rds as R


def _load_model():
    name = "rds_model"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name("rds_model.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load_model()


# ---- the plan ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("fs,decim,half", [(240_000.0, 13, 405), (480_000.0, 25, 809), (10e6 / 21, 25, 803), (128_000.0, 7, 216)])
def test_plan_meets_its_specification(fs, decim, half):
    plan = P.plan_rds(fs)
    assert plan.decim == decim == int(round(fs / 19_000.0))
    assert plan.half == half == math.ceil(2.0 * fs / 1187.5)
    assert fs / plan.decim / 1187.5 >= 15.0  # samples per symbol at the decimated rate
    h = plan.h_matched
    assert h.size == 2 * half + 1 and h[half] == 0.0
    np.testing.assert_array_equal(h, -h[::-1])
    assert abs(float(np.sum(h * h)) - 1.0) < 1e-12
    k = np.arange(h.size)
    want = P.rds_symbol(-(k - half) / (fs / 1187.5))
    np.testing.assert_allclose(h / np.linalg.norm(h), want / np.linalg.norm(want), atol=1e-12)
    assert plan.j0 == math.ceil((2 * (plan.wfm.ntaps - 1) + 2 * half) / decim)
    assert plan.hist_len == 2 * half + 2 * (plan.wfm.ntaps - 1)
    assert plan.f_mix == 57_000.0 / fs and plan.clock_step == 19_000.0 * decim / fs
    np.testing.assert_array_equal(plan.mf_packed, h[:half].astype(np.float32))
    d = plan.wfm.delay
    np.testing.assert_array_equal(plan.pilot_packed, np.concatenate([plan.wfm.h_pilot.real[: d + 1],
                                                                     plan.wfm.h_pilot.imag[: d + 1]]).astype(np.float32))


def test_pulse_is_the_transform_of_the_cosine_rolloff():
    """h(x) = integral of cos(pi f / 4) cos(2 pi f x) over |f| <= 2 (f in 1/td, x in symbols); h(0) = 8 / pi ... numerically."""
    f = np.linspace(-2.0, 2.0, 200_001)
    for x in (0.0, 0.125, 0.3, 1.0, 1.7):
        num = np.trapezoid(np.cos(np.pi * f / 4.0) * np.cos(2 * np.pi * f * x), f)
        assert abs(num - float(P.rds_pulse(x))) < 1e-8, x
    x = np.linspace(-3, 3, 601)
    np.testing.assert_allclose(P.rds_symbol(x), -P.rds_symbol(-x), atol=1e-14)


ISI_BOUND = 1e-3


def test_pulse_pair_is_isi_free_at_480k():
    """(g * g) of the truncated +-2-symbol filter pair, sampled at non-zero whole-symbol offsets, against its peak.  The
    sampling instants fall between taps (404.21 samples per symbol), so the correlation is taken on a 16x finer grid of the
    same +-2-symbol truncation.  Measured on the CPU: 3.9e-4 of the peak (the bound is the issue's 1e-3)."""
    fs, over = 480_000.0, 16
    spp = fs / 1187.5 * over
    half = math.ceil(2.0 * spp)
    g = P.rds_symbol(-(np.arange(2 * half + 1) - half) / spp)
    c = np.correlate(g, g, mode="full")  # lag l at index l + 2 half
    peak = c[2 * half]
    worst = 0.0
    for s in (1, 2, 3, 4):
        at = s * spp
        lo = int(math.floor(at))
        if lo + 1 > 2 * half:
            break
        v = c[2 * half + lo] + (c[2 * half + lo + 1] - c[2 * half + lo]) * (at - lo)
        worst = max(worst, abs(v) / peak)
    print("ISI of the truncated pulse pair:", worst)
    assert worst < ISI_BOUND, worst


# ---- check word --------------------------------------------------------------------------------------------------------


def test_crc_and_offset_words():
    assert R.OFFSET_WORDS == M.OFFSETS and R.CRC_POLY == M.G
    rng = np.random.default_rng(3)
    for name, off in M.OFFSETS.items():
        for info in [0, 0xFFFF, 0x54A8] + rng.integers(0, 1 << 16, size=5).tolist():
            w = M.block(int(info), name)
            assert M.syndrome(w) == off
            bits = np.array([(w >> (25 - i)) & 1 for i in range(26)])
            words, synd = M.words_and_syndromes(bits)
            assert words.tolist() == [w] and synd.tolist() == [off]
            for flip in range(26):  # a single flipped bit never leaves the syndrome at the block's offset word
                assert M.syndrome(w ^ (1 << flip)) != off, (name, flip)


# ---- the oracle chain on the model's multiplex -------------------------------------------------------------------------


@pytest.mark.parametrize("sigma", [0.0, 0.02])
@pytest.mark.parametrize("ppm", [50.0, -50.0])
@pytest.mark.parametrize("fs", [240_000.0, 10e6 / 21])
def test_oracle_decodes_the_model_multiplex(fs, ppm, sigma):
    m, sent = M.multiplex(fs, 4.0, ppm=ppm, sigma=sigma, seed=7)
    o = M.oracle_chain(M.theta_of(m, fs), fs)
    off, errors = M.align(o["bits"], M.bits_of(sent + M.schedule(len(sent) + 1)[len(sent):]))
    print(f"fs {fs:.0f} ppm {ppm:+.0f} sigma {sigma}: tau {o['tau']:+.4f} strength {o['strength']:.3f} offset {off} "
          f"errors {errors} of {o['bits'].size}")
    assert errors == 0
    res = R.parse_groups(o["words"], o["syndromes"])
    assert res.groups >= len(sent) - 3, (res.groups, len(sent))
    assert len(sent) >= 44
    assert (res.pi, res.ps, res.radiotext) == (M.PI, M.PS, M.RT_SHOWN)
    assert res.tp is True and res.pty == 10
    assert set(res.groups_by_type) == {"0A", "2A", "4A", "14A"}
    assert sum(res.groups_by_type.values()) == res.groups
    assert all((b - a) % 104 == 0 for a, b in zip(res.group_offsets, res.group_offsets[1:]))


@pytest.mark.parametrize("fs", [240_000.0, 128_000.0])
def test_oracle_baseband_at_an_absolute_position(fs):
    """``oracle_baseband(theta, fs, pos=...)`` is the oracle of the stream with ``pos`` zeros written out in front of
    ``theta``, restricted to j >= ceil(pos / R): the same y (to the rounding of a float64 dot product whose rows sit
    elsewhere in the matrix: 1e-12 of rms(y)) and the same q (to one count of 2^-44 cycle, 3.6e-13 rad, where that
    rounding moves a value across a half) -- and the same clock from the same q."""
    plan = P.plan_rds(fs)
    R = plan.decim
    pos = 1000 * R + 3
    n = (plan.j0 + 150) * R + 5
    m, _ = M.multiplex(fs, n / fs, ppm=40.0, sigma=0.01, seed=2)
    theta = M.theta_of(m, fs)
    got = M.oracle_baseband(theta, fs, pos=pos)
    whole = M.oracle_baseband(np.concatenate([np.zeros(pos, np.float32), theta]), fs)
    j_first = -(-pos // R)
    assert got["j_first"] == j_first == 1001 and whole["j_first"] == 0
    assert got["y"].size == whole["y"].size - j_first == A.native.lib().iqa_rds_outputs(pos, theta.size, R)
    assert np.all(whole["y"][: j_first - 1] == 0) and np.all(whole["q"][:j_first] == 0)
    scale = float(np.sqrt(np.mean(np.abs(whole["y"][j_first + plan.j0 :]) ** 2)))
    assert scale > 1e-3
    assert np.abs(got["y"] - whole["y"][j_first:]).max() <= 1e-12 * scale
    assert got["q"][0] == 0 and got["dev"][0] == 0.0
    assert np.abs(got["q"] - whole["q"][j_first:]).max() <= 1
    # a position that is a multiple of R, and the default, keep the first output at the block's first sample
    assert M.oracle_baseband(theta, fs, pos=7 * R)["j_first"] == 7
    same = M.oracle_baseband(theta, fs)
    np.testing.assert_array_equal(same["y"], M.oracle_baseband(theta, fs, pos=0)["y"])
    # the clock of outputs j_first ...: the statement on absolute j, Phi from 0
    phi, psi = M.oracle_clock(got["q"], plan, j_first=j_first)
    phi_w, psi_w = M.oracle_clock(np.concatenate([np.zeros(j_first, np.int64), got["q"]]), plan)
    np.testing.assert_array_equal(phi, phi_w[j_first:])
    np.testing.assert_array_equal(psi, psi_w[j_first:])


# ---- the parser --------------------------------------------------------------------------------------------------------


def _ws(groups, corrupt=None):
    bits = M.bits_of(groups)
    if corrupt is not None:
        bits[corrupt] ^= 1
    return M.words_and_syndromes(bits)


def test_parse_groups_on_synthetic_words():
    groups = M.schedule(12)
    res = R.parse_groups(*_ws(groups))
    assert res.groups == 12 and res.group_offsets == [104 * i for i in range(12)]
    assert (res.pi, res.ps, res.radiotext) == (M.PI, M.PS, M.RT_SHOWN)
    assert res.groups_by_type == {"0A": 5, "14A": 1, "2A": 5, "4A": 1}
    assert res.bits == 12 * 104
    # one corrupted bit (block C of group 5) drops exactly that group
    res = R.parse_groups(*_ws(groups, corrupt=5 * 104 + 52 + 7))
    assert res.groups == 11 and 5 * 104 not in res.group_offsets
    # three of the four PS segments: no name yet
    res = R.parse_groups(*_ws([M.group_0a(M.PI, s, M.PS) for s in (0, 1, 3)]))
    assert res.groups == 3 and res.ps is None and res.pi == M.PI and res.radiotext is None
    # a change of the text A/B flag clears the buffer
    old, new = "OLD TEXT HERE!!!", "NEW\r            "
    seq = [M.group_2a(M.PI, s, old, flag=0) for s in range(4)] + [M.group_2a(M.PI, 0, new, flag=1)]
    assert R.parse_groups(*_ws(seq[:4])).radiotext == old
    assert R.parse_groups(*_ws(seq)).radiotext == "NEW"
    # 2B: two characters per segment from block D, block C' repeats the PI
    text = "SHORT 2B\r       "
    res = R.parse_groups(*_ws([M.group_2b(M.PI, s, text) for s in range(8)]))
    assert res.groups == 8 and res.groups_by_type == {"2B": 8} and res.radiotext == "SHORT 2B"
    # bytes outside 0x20 .. 0x7E read as U+FFFD
    res = R.parse_groups(*_ws([M.group_0a(M.PI, s, "AB\x07DEF\xe9H") for s in range(4)]))
    assert res.ps == "AB�DEF�H"
    # nothing to parse
    assert R.parse_groups(np.zeros(0, np.uint32), np.zeros(0, np.uint16)).groups == 0
    assert R.parse_groups(np.zeros(500, np.uint32), np.zeros(500, np.uint16)).groups == 0


def test_result_line_and_json():
    res = R.parse_groups(*_ws(M.schedule(10)))
    assert res.line() == 'PI=54A8 PS="GFX950FM" RT="MI355X ON AIR" groups=10'
    js = res.to_json()
    assert js["pi"] == M.PI and js["ps"] == M.PS and js["radiotext"] == M.RT_SHOWN and js["groups"] == 10
    assert set(js) >= {"pi", "pty", "tp", "ps", "radiotext", "groups", "groups_by_type", "bits", "timing"}


# ---- CLI, pipeline validation --------------------------------------------------------------------------------------------


def test_cli_rds_needs_wfm(capsys):
    from iq_to_audio_amd import cli

    for mode in (["--demod", "nfm"], [], ["--demod", "am"]):
        with pytest.raises(SystemExit) as exc:
            cli.main(["--in", "x.wav", "--ft", "100e6", "--rds", *mode])
        assert exc.value.code == 2
        assert "--rds" in capsys.readouterr().err
    args = cli.build_parser().parse_args(["--in", "x.wav", "--ft", "100e6", "--demod", "wfm", "--rds"])
    assert args.rds is True
    assert cli.build_parser().parse_args(["--in", "x.wav", "--ft", "100e6", "--demod", "wfm"]).rds is False


def test_rds_with_a_non_wfm_target_is_rejected_before_any_launch(tmp_path):
    wav = tmp_path / "cap_100000000Hz.wav"
    iqio.write_wav_iq(wav, np.zeros(2 * 24_000, dtype=np.int16), 2_400_000, "s16")
    nfm = A.ProcessingConfig(in_path=wav, target_freq=100.3e6, demod_mode="nfm", output_path=tmp_path / "o.wav")
    wfm = A.ProcessingConfig(in_path=wav, target_freq=100.3e6, demod_mode="wfm", bandwidth=250_000.0, fs_ch_target=480_000.0,
                             deemph_us=50.0, output_path=tmp_path / "w.wav")
    with pytest.raises(ValueError, match="rds"):
        A.ProcessingPipeline(nfm, rds=True)
    with pytest.raises(ValueError, match="rds"):
        A.MultiChannelPipeline([wfm, nfm], rds=True)
    assert A.ProcessingPipeline(wfm, rds=True).rds_enabled and A.ProcessingPipeline(wfm).rds_enabled is False
    assert A.ProcessingPipeline(wfm).rds is None and A.MultiChannelPipeline([wfm], rds=True).rds is None
    assert not (tmp_path / "o.wav").exists()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------


def test_abi_entries_reject_bad_arguments_without_a_gpu():
    lib = A.native.lib()
    assert lib.iqa_abi_version() == 1
    assert lib.iqa_rds_hist_len(693, 809) == 2 * 809 + 2 * 692 and lib.iqa_rds_hist_len(2, 809) == 0
    assert lib.iqa_rds_outputs(0, 25, 25) == 1 and lib.iqa_rds_outputs(1, 25, 25) == 1 and lib.iqa_rds_outputs(1, 24, 25) == 0
    assert lib.iqa_rds_outputs(0, 26, 25) == 2 and lib.iqa_rds_outputs(50, 100, 25) == 4 and lib.iqa_rds_outputs(0, 0, 25) == 0
    assert lib.iqa_rds_timing_partials(0) == 0 and lib.iqa_rds_timing_partials(1025) == 2
    assert lib.iqa_rds_clock_chunks(0) == 0 and lib.iqa_rds_clock_chunks(4096) == 1 and lib.iqa_rds_clock_chunks(4097) == 2
    # LDS: every rate the stereo matrix admits fits; the limits of the header fit at the smallest tile
    for fs in (128_000.0, 240_000.0, 480_000.0, 1_000_000.0, 1_400_000.0):
        plan = P.plan_rds(fs)
        assert 0 < lib.iqa_rds_lds_bytes(plan.wfm.ntaps, plan.half, plan.decim) <= 64 * 1024 - 64, fs
    assert 0 < lib.iqa_rds_lds_bytes(P.WFM_MAX_TAPS, P.RDS_MAX_HALF, P.RDS_MAX_DECIM) <= 64 * 1024 - 64
    buf = (ctypes.c_float * 64)()
    ok = ctypes.cast(buf, c_void_p)
    null = c_void_p(0)

    def baseband(ntaps=693, half=809, decim=25, n=100, pos=0, pilot=ok, mf=ok, theta=ok, y=ok, q=ok, scale=1.0, f_mix=0.11875):
        A.native.call("iqa_rds_baseband", c_int32(ntaps), pilot, c_int32(half), mf, c_int32(decim), c_float(scale), c_double(f_mix),
                      c_double(0.99), theta, c_int64(n), c_int64(pos), null, y, q, null)

    for bad in (0, 1, 2, 692, P.WFM_MAX_TAPS + 2, -5):
        with pytest.raises(ValueError):
            baseband(ntaps=bad)
        assert "ntaps" in lib.iqa_last_error().decode()
    for bad in (0, -1, P.RDS_MAX_HALF + 1):
        with pytest.raises(ValueError):
            baseband(half=bad)
        assert "half_taps" in lib.iqa_last_error().decode()
    for bad in (0, -3, P.RDS_MAX_DECIM + 1):
        with pytest.raises(ValueError):
            baseband(decim=bad)
        assert "decimation" in lib.iqa_last_error().decode()
    with pytest.raises(ValueError):
        baseband(n=-1)
    assert "negative" in lib.iqa_last_error().decode()
    with pytest.raises(ValueError):
        baseband(pos=-1)
    for kw in ("pilot", "mf", "theta", "y", "q"):
        with pytest.raises(ValueError):
            baseband(**{kw: null})
        assert "NULL" in lib.iqa_last_error().decode()
    with pytest.raises(ValueError):
        baseband(scale=float("inf"))
    with pytest.raises(ValueError):
        baseband(f_mix=float("nan"))

    def clock(n=8, q=ok, total=ok, work=ok, phi=ok, psi=ok, j=0):
        A.native.call("iqa_rds_clock", q, c_int64(n), c_int64(j), c_double(0.99), total, work, phi, psi, null)

    with pytest.raises(ValueError):
        clock(n=-1)
    with pytest.raises(ValueError):
        clock(j=-1)
    for kw in ("q", "total", "work", "phi", "psi"):
        with pytest.raises(ValueError):
            clock(**{kw: null})
        assert "NULL" in lib.iqa_last_error().decode()
    with pytest.raises(ValueError):
        A.native.call("iqa_rds_timing", ok, ok, c_int64(-1), c_int64(0), ok, ok, null)
    for args in ((null, ok, ok, ok), (ok, null, ok, ok), (ok, ok, null, ok), (ok, ok, ok, null)):
        with pytest.raises(ValueError):
            A.native.call("iqa_rds_timing", args[0], args[1], c_int64(8), c_int64(0), args[2], args[3], null)
        assert "NULL" in lib.iqa_last_error().decode()
    with pytest.raises(ValueError):
        A.native.call("iqa_rds_symbols", ok, ok, c_int64(-1), c_int64(0), c_double(0.0), c_int64(0), c_int64(4), ok, ok, null)
    with pytest.raises(ValueError):
        A.native.call("iqa_rds_symbols", ok, ok, c_int64(8), c_int64(0), c_double(float("nan")), c_int64(0), c_int64(4), ok, ok, null)
    for args in ((null, ok, ok, ok), (ok, null, ok, ok), (ok, ok, null, ok), (ok, ok, ok, null)):
        with pytest.raises(ValueError):
            A.native.call("iqa_rds_symbols", args[0], args[1], c_int64(8), c_int64(0), c_double(0.0), c_int64(0), c_int64(4), args[2],
                          args[3], null)
        assert "NULL" in lib.iqa_last_error().decode()
    with pytest.raises(ValueError):
        A.native.call("iqa_rds_syndromes", ok, c_int64(-1), ok, ok, null)
    for args in ((null, ok, ok), (ok, null, ok), (ok, ok, null)):
        with pytest.raises(ValueError):
            A.native.call("iqa_rds_syndromes", args[0], c_int64(64), args[1], args[2], null)
        assert "NULL" in lib.iqa_last_error().decode()
    # zero-length calls are no-ops, as for the other entry points
    A.native.call("iqa_rds_clock", null, c_int64(0), c_int64(0), c_double(0.99), null, null, null, null, null)
    A.native.call("iqa_rds_syndromes", null, c_int64(25), null, null, null)
