"""The carrier squelch without a GPU (--squelch): the plan at its rate classes and its refusals, the numpy
oracle of tests/gate_model.py on the model stream (two transmissions, the click dropped) and on noise alone, every rule on both
sides of equality, the package's host arithmetic against the oracle, the CLI's usage errors, the entry points' argument checks
and the signatures."""
from __future__ import annotations

import importlib.util
import inspect
import math
import sys
from ctypes import c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


G = _load("gate_model")

import iq_to_audio_amd as A  # noqa: E402
from iq_to_audio_amd import cli  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd import gate as GT  # noqa: E402

RATES = (8_000.0, 25_599.0, 25_600.0, 96_000.0, 96_153.8, 480_000.0, 2_000_000.0)


# ---- the plan -----------------------------------------------------------------------------------------------------------------


def test_plan_at_96k_is_the_issues():
    p = P.plan_gate(96_000.0)
    assert (p.frame, p.num_open, p.num_close, p.hang, p.min_frames, p.lead, p.ramp_len) == (768, 4077, 2572, 38, 5, 3, 480)
    assert p.ramp.dtype == np.float32 and p.ramp.size == 480 and not p.ramp.flags.writeable
    assert p.ramp[0] == np.float32(1 / 481) and p.ramp[-1] == np.float32(480 / 481)
    assert (p.frames(0), p.frames(767), p.frames(768), p.frames(2 * 768 - 1), p.frames(288_000)) == (1, 1, 1, 1, 375)


@pytest.mark.parametrize("fs", RATES)
def test_plan_equals_the_oracles(fs):
    p, want = P.plan_gate(fs, A.CarrierSquelch()), G.plan(fs)
    assert (p.frame, p.hang, p.min_frames, p.lead, p.ramp_len, p.num_open, p.num_close) == tuple(
        want[k] for k in ("Lf", "H", "M", "A", "R", "num_open", "num_close"))
    np.testing.assert_array_equal(p.ramp, want["ramp"])
    assert p.frame % 256 == 0 and p.frame == 256 * max(1, int(fs * 10.0 / 1000 / 256))


def test_plan_frame_classes():
    assert [P.plan_gate(fs).frame for fs in RATES] == [256, 256, 256, 768, 768, 4608, 19968]
    assert P.plan_gate(8_000.0).min_frames == 2 and P.plan_gate(2_000_000.0).hang == math.ceil(0.3 * 2e6 / 19968)
    zero = P.plan_gate(96_000.0, A.CarrierSquelch(hang_ms=0.0, min_ms=0.0, lead_ms=0.0, ramp_ms=0.0))
    assert (zero.hang, zero.min_frames, zero.lead, zero.ramp_len, zero.ramp.size) == (0, 1, 0, 0, 0)
    assert P.plan_gate(96_000.0, A.CarrierSquelch(open_db=30.0)).num_open == 1_024_000


@pytest.mark.parametrize("opts, what", [
    (dict(open_db=2.0), "hyst_db < open_db"), (dict(open_db=30.5), "hyst_db < open_db"), (dict(hyst_db=-0.1), "hyst_db < open_db"),
    (dict(hyst_db=6.0), "hyst_db < open_db"), (dict(hang_ms=-1.0), "hang_ms"), (dict(hang_ms=10_001.0), "hang_ms"),
    (dict(min_ms=-1.0), "min_ms"), (dict(lead_ms=10_001.0), "lead_ms"), (dict(ramp_ms=-0.5), "ramp_ms"), (dict(frame_ms=20_000.0), "frame_ms"),
    (dict(open_db=float("nan")), "finite")])
def test_plan_refuses(opts, what):
    with pytest.raises(ValueError, match=what):
        P.plan_gate(96_000.0, A.CarrierSquelch(**opts))
    if "finite" not in what:
        with pytest.raises(ValueError):
            G.plan(96_000.0, **opts)


def test_plan_refuses_a_frame_past_2_20_and_a_bad_rate():
    with pytest.raises(ValueError, match="exceeds"):
        P.plan_gate(2_000_000.0, A.CarrierSquelch(frame_ms=1_000.0))
    assert P.plan_gate(2_000_000.0, A.CarrierSquelch(frame_ms=524.288)).frame == 1 << 20
    for fs in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="positive"):
            P.plan_gate(fs)


# ---- the oracle's own pieces ----------------------------------------------------------------------------------------------------


def test_oracle_quantiser_and_cells():
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 40000.0, -40000.0, np.nan, np.inf, -np.inf, 32767.5, 1e-30], dtype=np.float32)
    assert G.quantise(x, 0).tolist() == [0, 2, 2, 0, -2, 32767, -32767, 0, 32767, -32767, 32767, 0]
    assert G.quantise(np.float32(3.0), -1).tolist() == 2 and G.quantise(np.float32(1.0), 30).tolist() == 32767
    cases = ((0, -5), (0, 0), (0, 1), (0, 256), (0, 257), (255, 1), (255, 2), (1000, 3 * 2048 + 5), (1 << 35, 1))
    assert [G.n_cells(p, n) for p, n in cases] == [0, 0, 1, 1, 2, 1, 2, 25, 1]
    z = (np.arange(600) % 7 + 1j * (np.arange(600) % 5)).astype(np.complex64)
    whole = G.cells(z, 0, 0)
    assert whole.tolist() == [int(G.power(z[a : a + 256], 0).sum()) for a in (0, 256, 512)]
    parts, pos = [], 0
    for k in (1, 254, 2, 300, 43):
        parts.append((pos // 256, G.cells(z[pos : pos + k], pos, 0)))
        pos += k
    np.testing.assert_array_equal(G.add_cells(parts, 600), whole)
    assert (G.choose_shift(0.0), G.choose_shift(float("nan")), G.choose_shift(float("inf")), G.choose_shift(1.0), G.choose_shift(1e-4)) == (15, 15, -30, 8, 14)  # (rms 0.01: ceil(log2) = -6)
    assert [GT.choose_shift(x) for x in (0.0, float("inf"), 1.0, 1e-4, 3.9, 4.0, 4.1, 1e30, 1e-30)] == [
        G.choose_shift(x) for x in (0.0, float("inf"), 1.0, 1e-4, 3.9, 4.0, 4.1, 1e30, 1e-30)]


def test_oracle_frames():
    c = np.arange(1, 10, dtype=np.int64) * 1000
    assert G.frames(c[:1], 100, 768).tolist() == [16 * 1000 // 100]  # n < Lf: one frame of n samples
    assert G.frames(c[:6], 2 * 768 - 1, 768).tolist() == [16 * 21000 // 1535]  # one long frame
    assert G.frames(c[:6], 2 * 768, 768).tolist() == [16 * 6000 // 768, 16 * 15000 // 768]
    assert G.frames(c, 2 * 768 + 700, 768).tolist() == [16 * 6000 // 768, 16 * 39000 // 1468]


def test_oracle_gain_against_loops():
    for R, n in ((0, 3000), (100, 3000), (700, 2999), (480, 256 * 11 + 5)):
        p = dict(Lf=256, R=R, ramp=np.array([np.float32((k + 1) / (R + 1)) for k in range(R)], dtype=np.float32))
        F = max(1, n // 256)
        g = np.zeros(F, dtype=np.uint8)
        g[0:3] = 1
        g[5:6] = 1
        g[F - 2 :] = 1
        lo, hi = G.bounds(g)
        np.testing.assert_array_equal(G.gain(g, lo, hi, n, p), G.gain_loops(g, lo, hi, n, p))
        a = np.linspace(-1, 1, n).astype(np.float32)
        a[::50] = np.nan
        out = G.apply(a, g, lo, hi, p)
        closed = np.repeat(g == 0, 256)
        assert (out[: closed.size][closed] == 0).all() and not np.isnan(out[: closed.size][closed]).any()


# ---- the model stream ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cn_db", (8, 10, 20, 40))
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_model_stream_has_two_transmissions(cn_db, seed):
    p = G.plan(G.MODEL_FS)
    z = G.model_stream(cn_db, seed)
    d = G.run(z, p)
    assert G.runs(d["g"]) == [(59, 175), (222, 287)]
    tx = G.transmissions(d["g"], z.size, p["Lf"])
    assert [(a / 96000.0, b / 96000.0) for a, b in tx] == [(0.472, 1.408), (1.776, 2.304)]
    # the 20 ms click opens the squelch (s) and is dropped by the minimum duration (s2)
    click = [r for r in G.runs(d["s"]) if r[0] >= 300]
    assert click and all(b - a + 1 < p["M"] for a, b in click) and not d["s2"][300:].any()
    # the package's host arithmetic gives the oracle's result
    plan = P.plan_gate(G.MODEL_FS)
    res, want = GT.gate_result(plan, z.size, d["sh"], d["floor"], d["v"], d["s2"], d["g"], frequency=1.0e8), G.result(d, z.size, d["sh"], p)
    assert [(t.start, t.end) for t in res.transmissions] == tx
    for t, w in zip(res.transmissions, want["transmissions"]):
        assert (t.start_s, t.end_s) == (w["start_s"], w["end_s"])
        assert t.peak_db == pytest.approx(w["peak_db"], abs=1e-9) and t.mean_db == pytest.approx(w["mean_db"], abs=1e-9)
        assert cn_db - 1.0 < t.mean_db < cn_db + 1.5 or cn_db == 40  # (at 40 dB the floor sits at the quantiser: known limit)
    assert res.duty == want["duty"] == (tx[0][1] - tx[0][0] + tx[1][1] - tx[1][0]) / z.size
    assert res.floor_dbfs == pytest.approx(want["floor_dbfs"], abs=1e-9) and -41.0 < res.floor_dbfs < -39.0
    assert res.lines("100000000 Hz: ")[0].startswith("100000000 Hz: on 0.472 .. 1.408 s (0.936 s), ") and res.lines()[0].endswith(" dB over the floor")
    again = A.GateResult.from_json(res.to_json())
    assert again == res and isinstance(again.transmissions[0], A.Transmission)


@pytest.mark.parametrize("seed", (1, 2, 3, 4, 5, 6))
def test_noise_alone_never_opens(seed):
    p = G.plan(G.MODEL_FS)
    z = G.model_stream(None, seed)
    d = G.run(z, p)
    assert not d["s"].any() and not d["g"].any() and (d["lo"] == -1).all() and (d["hi"] == -1).all()
    over = 10 * math.log10(int(d["v"].max()) / d["floor"])
    assert 1.6 <= over <= 2.2, over  # against 4 dB (close) and 6 dB (open)
    res = GT.gate_result(P.plan_gate(G.MODEL_FS), z.size, d["sh"], d["floor"], d["v"], d["s2"], d["g"])
    assert res.transmissions == [] and res.duty == 0.0 and res.lines("7 Hz: ") == ["7 Hz: squelch never opened"]


def test_cuts_change_nothing_in_the_oracle():
    p = G.plan(G.MODEL_FS)
    z = G.model_stream(20, 1)[:40_000]
    whole = G.run(z, p, sh=12)
    cut = G.run(z, p, sh=12, cuts=[1, 255, 100, 100, 56, 2048, 3, 40_000 - 2563])
    for k in ("cells", "v", "s", "s2", "g", "lo", "hi"):
        np.testing.assert_array_equal(whole[k], cut[k])


# ---- every rule on both sides of equality ------------------------------------------------------------------------------------


def test_open_and_close_at_equality():
    for k in (1, 3, 1000):
        floor = 1024 * k
        assert G.state([4077 * k], floor, 4077, 2572).tolist() == [1]  # 1024 v == num_open floor opens
        assert G.state([4077 * k - 1], floor, 4077, 2572).tolist() == [0]
        assert G.state([4077 * k, 2572 * k], floor, 4077, 2572).tolist() == [1, 1]  # 1024 v == num_close floor keeps
        assert G.state([4077 * k, 2572 * k - 1], floor, 4077, 2572).tolist() == [1, 0]
        assert G.state([2572 * k, 4077 * k - 1], floor, 4077, 2572).tolist() == [0, 0]  # hold of a closed state stays closed
    assert G.state([5000, 3000, 3000, 2000, 3000, 5000, 3000], 1024, 4077, 2572).tolist() == [1, 1, 1, 0, 0, 1, 1]


def test_minimum_duration_at_equality():
    M = 5
    s = np.zeros(30, dtype=np.uint8)
    s[2 : 2 + M - 1] = 1
    s[10 : 10 + M] = 1
    s[30 - M + 1 :] = 1  # M - 1 frames at the end
    assert G.runs(G.min_duration(s, M)) == [(10, 14)]
    assert G.runs(G.min_duration(s, M - 1)) == [(2, 5), (10, 14), (26, 29)] and G.runs(G.min_duration(s, 1)) == G.runs(s)
    assert not G.min_duration(np.ones(4, dtype=np.uint8), 5).any() and G.min_duration(np.ones(5, dtype=np.uint8), 5).all()


def test_hang_and_lead_at_equality():
    H, A_, M = 38, 3, 5
    for gap, merged in ((H + A_, True), (H + A_ + 1, False)):
        s2 = np.zeros(120, dtype=np.uint8)
        s2[10 : 10 + M] = 1
        second = 10 + M + gap
        s2[second : second + M] = 1
        g = G.hang_lead(s2, H, A_)
        want = [(7, second + M - 1 + H)] if merged else [(7, 14 + H), (second - A_, second + M - 1 + H)]
        assert G.runs(g) == want, gap
    s2 = np.zeros(20, dtype=np.uint8)
    s2[[0, 19]] = 1
    assert G.runs(G.hang_lead(s2, 0, 0)) == [(0, 0), (19, 19)]  # H = A = 0
    assert G.runs(G.hang_lead(s2, 2, 1)) == [(0, 2), (18, 19)]  # runs at both ends
    assert G.hang_lead(s2, 100, 100).all()  # H and A larger than F
    lo, hi = G.bounds(G.hang_lead(s2, 2, 1))
    assert lo.tolist() == [0] * 3 + [-1] * 15 + [18] * 2 and hi.tolist() == [3] * 3 + [-1] * 15 + [20] * 2
    assert G.transmissions(G.hang_lead(s2, 2, 1), 20 * 256 + 100, 256) == [(0, 768), (18 * 256, 20 * 256 + 100)]


def test_floor_rank_and_clamp():
    assert G.floor_of([7]) == 7 and G.floor_of([9, 3, 5, 8, 7, 6, 4, 10, 11, 12]) == 3  # rank 0 for F <= 10
    assert G.floor_of([9, 3, 5, 8, 7, 6, 4, 10, 11, 12, 13]) == 4  # rank 1 at F = 11
    assert G.floor_of(np.arange(100, 0, -1)) == 10 and G.floor_of(np.arange(101, 0, -1)) == 11
    assert G.floor_of([0, 0, 0]) == 1 and G.floor_of(np.zeros(50, dtype=np.int64)) == 1  # clamped at 1
    # with the floor clamped at 1, v = 3 keeps (3072 >= 2572) and v = 4 opens (4096 >= 4077)
    d = G.decide(np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 64, 48, 32, 0], dtype=np.int64), 14 * 256, dict(G.plan(96000.0), Lf=256, M=1, H=0, A=0))
    assert d["floor"] == 1 and d["v"][10:13].tolist() == [4, 3, 2] and d["s"][9:].tolist() == [0, 1, 1, 0, 0]


def test_ramp_zero_and_result_of_an_empty_run():
    p = dict(G.plan(96000.0, ramp_ms=0.0), Lf=256)
    g = np.array([0, 1, 1, 0], dtype=np.uint8)
    lo, hi = G.bounds(g)
    assert G.gain(g, lo, hi, 1024, p).tolist() == [0.0] * 256 + [1.0] * 512 + [0.0] * 256
    res = GT.gate_result(P.plan_gate(96000.0), 0, 15, 1, np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint8))
    assert res.transmissions == [] and res.duty == 0.0


# ---- the CLI and the package surface -----------------------------------------------------------------------------------------


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        cli.main(argv)
    assert exc.value.code == 2
    return capsys.readouterr().err


def test_cli_refuses_misuse(capsys):
    base = ["--in", "capture.wav", "--ft", "455800000"]
    assert "--squelch-db needs --squelch." in _usage_error(base + ["--squelch-db", "8"], capsys)
    assert "--squelch-hang needs --squelch." in _usage_error(base + ["--squelch-hang", "100"], capsys)
    assert "--squelch-split needs --squelch." in _usage_error(base + ["--squelch-split"], capsys)
    assert "--squelch cannot be combined with --demod wfm." in _usage_error(base + ["--squelch", "--demod", "wfm"], capsys)
    assert "--squelch cannot be combined with --demod none." in _usage_error(base + ["--squelch", "--demod", "none"], capsys)
    assert "--squelch cannot be combined with --benchmark." in _usage_error(["--squelch", "--benchmark"], capsys)
    assert "--squelch cannot be combined with --audio-post." in _usage_error(["--squelch", "--audio-post", "x"], capsys)
    assert "--squelch cannot be combined with --probe-only." in _usage_error(base + ["--squelch", "--probe-only"], capsys)
    for flags in (["--find-channels"], ["--find-describe"], ["--find-decode"]):
        assert "--squelch needs --find-top" in _usage_error(["--in", "capture.wav", "--squelch"] + flags, capsys)
    for value in ("2", "1", "30.5", "nan"):
        assert "--squelch-db must be greater than 2 and at most 30." in _usage_error(base + ["--squelch", "--squelch-db", value], capsys)
    for value in ("-1", "10001", "nan"):
        assert "--squelch-hang must lie in 0 .. 10000 ms." in _usage_error(base + ["--squelch", "--squelch-hang", value], capsys)


def test_cli_builds_the_options():
    parser = cli.build_parser()

    def options(extra, finding=False):
        return cli.check_squelch_args(parser, parser.parse_args(["--in", "capture.wav"] + extra), finding)

    assert options(["--ft", "1"]) is None
    assert options(["--ft", "1", "--squelch"]) == A.CarrierSquelch()
    assert options(["--ft", "1", "--squelch", "--squelch-db", "9.5", "--squelch-hang", "0", "--squelch-split"]) == A.CarrierSquelch(
        open_db=9.5, hang_ms=0.0, split=True)
    assert options(["--find-top", "3", "--find-auto", "--find-decode", "--squelch", "--squelch-db", "30"], True).open_db == 30.0
    assert options(["--ft", "1", "--squelch", "--demod", "am", "--pocsag"]) == A.CarrierSquelch()  # (the side flags are checked elsewhere)


def test_signatures_and_surface():
    for cls in (A.ProcessingPipeline, A.MultiChannelPipeline):
        params = inspect.signature(cls.__init__).parameters
        assert params["squelch"].default is None and params["squelch"].kind is inspect.Parameter.KEYWORD_ONLY
        flags = {k for k, p in params.items() if p.kind is p.KEYWORD_ONLY and p.default is False}
        assert flags == {"rds", "pocsag", "ax25", "tones", "acars", "ais", "adsb"}
    from iq_to_audio_amd import batch

    assert all("squelch" not in inspect.signature(fn).parameters for _, fn in inspect.getmembers(batch, inspect.isfunction))
    from dataclasses import fields

    assert len(fields(A.ProcessingConfig)) == 23
    assert [f.name for f in fields(A.CarrierSquelch)] == ["frame_ms", "open_db", "hyst_db", "hang_ms", "min_ms", "lead_ms", "ramp_ms", "split"]
    assert A.CarrierSquelch().split is False and {k: getattr(A.CarrierSquelch(), k) for k in G.DEFAULTS} == G.DEFAULTS
    for name in ("process", "finish", "apply", "result", "stages", "reset"):
        assert callable(getattr(A.CarrierGate, name))
    assert A.plan_gate is P.plan_gate and A.GatePlan is P.GatePlan
    cfg = A.ProcessingConfig(in_path=Path("capture.wav"), target_freq=1.0e8)
    assert A.ProcessingPipeline(cfg).squelch is None and A.ProcessingPipeline(cfg).squelch_result is None
    assert A.ProcessingPipeline(cfg, squelch=A.CarrierSquelch(open_db=8.0)).squelch.open_db == 8.0
    for mode in ("wfm", "none"):
        bad = A.ProcessingConfig(in_path=Path("capture.wav"), target_freq=1.0e8, demod_mode=mode)
        with pytest.raises(ValueError, match="squelch cannot gate"):
            A.ProcessingPipeline(bad, squelch=A.CarrierSquelch())
        with pytest.raises(ValueError, match="squelch cannot gate"):
            A.MultiChannelPipeline([cfg, bad], squelch=A.CarrierSquelch())
        A.MultiChannelPipeline([cfg, bad], squelch=[A.CarrierSquelch(), None])
    with pytest.raises(ValueError, match="one entry per target"):
        A.MultiChannelPipeline([cfg], squelch=[A.CarrierSquelch(), None])
    with pytest.raises(ValueError, match="CarrierSquelch or None"):
        A.ProcessingPipeline(cfg, squelch=True)
    with pytest.raises(ValueError, match="hyst_db < open_db"):
        A.ProcessingPipeline(cfg, squelch=A.CarrierSquelch(open_db=1.0))


def test_c_abi_refuses_bad_arguments():
    """The library has the entry points, and the argument checks come before the launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some, other = c_void_p(0), c_void_p(16), c_void_p(4096)  # (never dereferenced: every call below is refused, or has nothing to do)
    for name in ("iqa_gate_cells", "iqa_gate_power", "iqa_gate_add_cells", "iqa_gate_decide", "iqa_gate_apply"):
        assert hasattr(N.lib(), name) and name in N.EXPORTS
    assert N.lib().iqa_abi_version() == 1 == N.ABI_VERSION
    header = (Path(__file__).resolve().parent.parent / "include" / "iqa_hotpath.h").read_text()
    assert "#define IQA_GATE_CELL 256" in header and "#define IQA_ABI_VERSION 1" in header and "#define IQA_GATE_MAX_NUM 1024000" in header
    assert (P.GATE_CELL, P.GATE_MAX_FRAME, P.GATE_MAX_FRAMES, P.GATE_MAX_SHIFT) == (256, 1 << 20, 1 << 24, 30)
    count = N.lib().iqa_gate_cells
    cases = ((0, -5), (0, 0), (0, 1), (0, 256), (0, 257), (255, 1), (255, 2), (1000, 3 * 2048 + 5), (1 << 35, 1), ((1 << 35) + 255, 257), (-1, 5))
    assert [count(p, n) for p, n in cases] == [G.n_cells(p, n) for p, n in cases[:-1]] + [0]
    i32, i64 = c_int32, c_int64

    def power(z=some, n=100, pos=0, sh=0, cells=some):
        N.call("iqa_gate_power", z, i64(n), i64(pos), i32(sh), cells, null)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(pos=-1), "negative"), (dict(sh=31), "-30 .. 30"), (dict(sh=-31), "-30 .. 30"),
                         (dict(pos=1 << 62), "2\\^62"), (dict(pos=(1 << 62) - 100), "2\\^62"), (dict(z=null), "NULL"), (dict(cells=null), "NULL"),
                         (dict(z=c_void_p(12)), "8-byte aligned")):
        with pytest.raises(ValueError, match=what):
            power(**kwargs)
    power(z=null, n=0, cells=null)  # nothing to do: no pointer is touched
    with pytest.raises(ValueError, match="negative"):
        N.call("iqa_gate_add_cells", some, i64(-1), some, null)
    with pytest.raises(ValueError, match="NULL"):
        N.call("iqa_gate_add_cells", null, i64(1), some, null)
    N.call("iqa_gate_add_cells", null, i64(0), null, null)

    def decide(cells=some, n=7680, Lf=768, F=10, num_open=4077, num_close=2572, M=5, H=38, A=3, out=(some,) * 8):
        N.call("iqa_gate_decide", cells, i64(n), i32(Lf), i32(F), i64(num_open), i64(num_close), i32(M), i32(H), i32(A), *out, null)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(Lf=0), "multiple of 256"), (dict(Lf=700), "multiple of 256"),
                         (dict(Lf=(1 << 20) + 256), "multiple of 256"), (dict(F=9), "max\\(1, n / Lf\\)"), (dict(F=11), "max\\(1, n / Lf\\)"),
                         (dict(n=767, F=0), "max\\(1, n / Lf\\)"), (dict(n=1 << 62, F=1), "2\\^62"), (dict(n=256 << 24, Lf=256, F=1 << 24, num_open=0), "num_open"),
                         (dict(n=256 * ((1 << 24) + 1), Lf=256, F=(1 << 24) + 1), "IQA_GATE_MAX_FRAMES"), (dict(num_open=1_024_001), "num_open"),
                         (dict(num_close=0), "num_close"), (dict(num_close=4078), "num_close"), (dict(M=0), "M must"), (dict(H=-1), "M must"),
                         (dict(A=-1), "M must"), (dict(cells=null), "NULL"), (dict(out=(some,) * 7 + (null,)), "NULL"),
                         (dict(out=(null,) + (some,) * 7), "NULL")):
        with pytest.raises(ValueError, match=what):
            decide(**kwargs)
    decide(cells=null, n=0, F=1, out=(null,) * 8)

    def apply(a=some, n=7680, Lf=768, F=10, g=some, lo=some, hi=some, ramp=some, R=480, out=other):
        N.call("iqa_gate_apply", a, i64(n), i32(Lf), i32(F), g, lo, hi, ramp, i32(R), out, null)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(Lf=100), "multiple of 256"), (dict(F=3), "max\\(1, n / Lf\\)"), (dict(R=-1), "R must"),
                         (dict(a=null), "NULL"), (dict(g=null), "NULL"), (dict(lo=null), "NULL"), (dict(hi=null), "NULL"), (dict(out=null), "NULL"),
                         (dict(ramp=null), "NULL ramp"), (dict(out=some), "buffer of its own")):
        with pytest.raises(ValueError, match=what):
            apply(**kwargs)
    apply(a=null, n=0, F=1, g=null, lo=null, hi=null, ramp=null, out=null)
