"""The channel finder (--find-channels), the host side: the plan, the numpy oracle (tests/find_model.py)
against plain loops on small planes, the oracle alone on the model capture (four channels come back where they were put, with
their widths and the burst's times; noise alone gives nothing), the host arithmetic of the package against the oracle's, the
CLI's flag checks and target selection, the C ABI.  No GPU compute."""
from __future__ import annotations

import dataclasses
import importlib.util
import sys
from ctypes import c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest

import iq_to_audio_amd as A
from iq_to_audio_amd import cli
from iq_to_audio_amd import dsp_plan as P
from iq_to_audio_amd import find as FD


def _load(name):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, Path(__file__).with_name(name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


M = _load("find_model")
FS = 2.4e6


@pytest.fixture(scope="module")
def reference():
    """The model capture through the oracle, once: (plan dict, stages, result dicts)."""
    raw = M.capture(FS, 2.0, 3)
    p = M.plan(FS, raw.shape[0])
    st = M.run(M.rows(raw, p), p)
    return p, st, M.result(p, st["runs"], st["on"], st["mean"], 455.5e6)


# ---- plan ----------------------------------------------------------------------------------------------------------------


def test_plan_defaults_of_the_reference_capture():
    plan = P.plan_find(FS, 4_800_000)
    assert (plan.nfft, plan.hop, plan.frames, plan.half, plan.gap, plan.slice_frames, plan.slices) == (8192, 4096, 1170, 1706, 17, 5, 234)
    assert (plan.thr, plan.thr_peak, plan.thr_act, plan.dc_bin, plan.dc_guard, plan.min_hot, plan.num, plan.den) == (600, 1000, 300, 4096, 3, 2, 1, 4)
    assert plan.bin_hz == FS / 8192 and plan.max_slices == 256
    w = np.hanning(8192)
    assert plan.scale == 8192 * FS * float(np.sum(w ** 2) / 8192) + 1e-18
    model = M.plan(FS, 4_800_000)
    for mine, theirs in (("nfft", "nfft"), ("hop", "hop"), ("frames", "F"), ("slice_frames", "T"), ("slices", "S"), ("half", "h"),
                         ("thr", "thr"), ("thr_peak", "thr_peak"), ("thr_act", "thr_act"), ("gap", "gap"), ("dc_guard", "dc_guard"),
                         ("scale", "scale"), ("bin_hz", "bin_hz"), ("dc_bin", "dc_bin"), ("min_hot", "min_hot")):
        assert getattr(plan, mine) == model[theirs], mine


def test_plan_default_nfft_and_halving():
    long = 1 << 26
    for fs, nfft in ((48_000.0, 256), (127_999.0, 256), (128_000.0, 256), (128_001.0, 512), (250_000.0, 512), (1e6, 2048), (2.4e6, 8192),
                     (2.5e6, 8192), (10e6, 32768), (50e6, 131072), (65.536e6, 131072), (100e6, 262144), (400e6, 262144)):
        plan = P.plan_find(fs, long)
        assert plan.nfft == nfft and plan.nfft == M.plan(fs, long)["nfft"], fs
        assert fs / plan.nfft <= 500.0 or plan.nfft == 1 << 18
        assert fs / plan.nfft > 250.0 or plan.nfft == 256
    # halving while fewer than 8 frames fit: 8 frames of nfft need 4.5 nfft samples
    assert P.plan_find(2.4e6, 36_864).nfft == 8192 and P.plan_find(2.4e6, 36_864).frames == 8
    assert P.plan_find(2.4e6, 36_863).nfft == 4096
    assert P.plan_find(2.4e6, 1152).nfft == 256 and P.plan_find(2.4e6, 1151).nfft == 256
    short = P.plan_find(2.4e6, 256)
    assert (short.nfft, short.frames, short.slice_frames, short.slices) == (256, 1, 1, 1)
    for n in (36_864, 36_863, 5000, 1152, 256):
        assert P.plan_find(2.4e6, n).nfft == M.plan(2.4e6, n)["nfft"]
    # an explicit nfft is taken as it is
    assert P.plan_find(2.4e6, 36_863, nfft=8192).frames == 7
    assert P.plan_find(2.4e6, 100_000, nfft=16).half == 3


def test_plan_errors():
    for n in (0, 255):
        with pytest.raises(ValueError, match="not one frame"):
            P.plan_find(2.4e6, n)
    with pytest.raises(ValueError, match="not one frame"):
        P.plan_find(2.4e6, 8191, nfft=8192)
    with pytest.raises(ValueError, match="power of two"):
        P.plan_find(2.4e6, 100_000, nfft=1000)
    with pytest.raises(ValueError, match="power of two"):
        P.plan_find(2.4e6, 1 << 22, nfft=1 << 19)
    # T <= 65536: 256 slices of 65536 frames of 256 bins at a hop of 128 are the longest run at that nfft
    most = 256 * 65536
    ok = P.plan_find(48_000.0, (most - 1) * 128 + 256)
    assert (ok.frames, ok.slice_frames, ok.slices) == (most, 65536, 256)
    with pytest.raises(ValueError, match="more than 65536"):
        P.plan_find(48_000.0, most * 128 + 256)
    for bad in (dict(threshold_db=0.0), dict(threshold_db=-1.0), dict(peak_threshold_db=float("nan")), dict(floor_hz=0.0),
                dict(gap_hz=-1.0), dict(max_slices=0), dict(min_hot=0)):
        with pytest.raises(ValueError):
            P.plan_find(2.4e6, 100_000, **bad)
    for fs in (0.0, -1.0, float("inf")):
        with pytest.raises(ValueError, match="sample rate"):
            P.plan_find(fs, 100_000)


def test_plan_slices_when_frames_do_not_divide():
    for frames, T, S in ((1, 1, 1), (256, 1, 256), (257, 2, 129), (511, 2, 256), (513, 3, 171), (1170, 5, 234), (1000, 4, 250)):
        plan = P.plan_find(48_000.0, (frames - 1) * 128 + 256, nfft=256)
        assert (plan.frames, plan.slice_frames, plan.slices) == (frames, T, S)
        assert sum(plan.slice_len(s) for s in range(S)) == frames and 1 <= plan.slice_len(S - 1) <= T
    plan = P.plan_find(48_000.0, 1023 * 128 + 256, nfft=256, max_slices=10)
    assert (plan.frames, plan.slice_frames, plan.slices, plan.slice_len(9)) == (1024, 103, 10, 97)
    # the clips and the guard
    assert P.plan_find(400e6, 1 << 26, nfft=1 << 18, floor_hz=1e9).half == 8191
    assert P.plan_find(48_000.0, 1 << 20, nfft=1 << 14, gap_hz=5000.0).gap == 255
    assert P.plan_find(2.4e6, 100_000, dc_guard_hz=-1.0).dc_guard == -1 and P.plan_find(2.4e6, 100_000, dc_guard_hz=0.0).dc_guard == 0
    assert P.plan_find(2.4e6, 100_000, threshold_db=4.35).thr == 435 and P.plan_find(2.4e6, 100_000, threshold_db=4.35).thr_act == 217


# ---- the oracle against plain loops --------------------------------------------------------------------------------------


def test_quantiser_rule():
    row = np.array([0.0, 0.004, 0.005, 0.015, 0.025, -0.005, -0.015, 1.234, -99.999, 300.0, 300.005, -300.005, 299.995, 1e30, -1e30,
                    np.inf, -np.inf, np.nan], dtype=np.float32)
    c = M.quantise(row)
    assert c.dtype == np.int16
    want = [int(np.clip(np.rint(np.float32(100.0) * v), -30000, 30000)) if np.isfinite(v) else 0 for v in row]
    want[-3], want[-2], want[-1] = 30000, -30000, -30000
    assert c.tolist() == want
    assert c[1] == 0 and c[7] == 123 and c[9] == 30000 and c[10] == 30000 and c[11] == -30000 and c[12] in (29999, 30000)
    # exact ties go to the even side: 0.125 * 100 = 12.5 -> 12, 0.375 * 100 = 37.5 -> 38, in float32 exactly
    assert M.quantise(np.array([0.125, 0.375, -0.125, -0.375], dtype=np.float32)).tolist() == [12, 38, -12, -38]


def test_oracle_stages_against_loops():
    rng = np.random.default_rng(5)
    c = rng.integers(-30000, 30001, size=(23, 37)).astype(np.int16)
    T, S = 4, 6
    whole = M.accumulate_all(c, T, S)
    st = M.new_state(37, S)
    for a, b in ((0, 1), (1, 3), (3, 10), (10, 23)):  # cuts inside slices
        M.accumulate(st, c[a:b], a, T)
    for key in ("sum", "max", "slice"):
        np.testing.assert_array_equal(st[key], whole[key])
        assert st[key].dtype == whole[key].dtype
    assert whole["slice"][5].tolist() == c[20:23].astype(np.int64).sum(axis=0).tolist()
    m = M.mean(whole["sum"], 23)
    assert m.tolist() == [int(v) // 23 for v in whole["sum"].tolist()] and (whole["sum"] < 0).any()
    for h, num, den in ((0, 1, 4), (3, 1, 4), (5, 0, 1), (5, 1, 1), (18, 1, 4), (40, 1, 2)):
        got = M.floor(m, h, num, den)
        for k in range(37):
            lo, hi = max(0, k - h), min(36, k + h)
            assert got[k] == sorted(m[lo : hi + 1].tolist())[((hi - lo) * num) // den], (h, num, den, k)
    hot_at = [0, 1, 5, 9, 20, 36]
    x0 = np.full(37, -1, dtype=np.int32)
    x0[hot_at] = 0
    zeros = np.zeros(37, dtype=np.int32)
    for gap in (0, 2, 3, 10, 15):
        x, mk = M.mask(x0, zeros, zeros - 5, zeros, thr=0, thr_peak=0, gap=gap, dc_bin=18, dc_guard=-1)
        np.testing.assert_array_equal(x, x0)
        for k in range(37):
            closed = k in hot_at or any(a < k < b and b - a - 1 <= gap for a in hot_at for b in hot_at)
            assert mk[k] == (1 if k in hot_at else 0) | (2 if closed else 0), (gap, k)
    _, mk = M.mask(x0, zeros, zeros - 5, zeros, thr=0, thr_peak=0, gap=3, dc_bin=5, dc_guard=4)
    assert [k for k in range(37) if mk[k] & 1] == [0, 20, 36]


def test_oracle_runs_and_activity_by_hand():
    mean = np.array([0, 9, 9, 0, 0, 7, -3, 8, 0, 0, 5, 0], dtype=np.int32)
    fmean = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], dtype=np.int32)
    mx = mean + 10
    fmax = fmean + 2
    mk = np.array([0, 3, 3, 0, 0, 3, 2, 3, 0, 0, 3, 0], dtype=np.uint8)
    rec, total = M.runs(mean, fmean, mx, fmax, mk, 2)
    assert total == 3
    assert rec.tolist() == [[1, 2, 2, 1, 8, 16, 8, 16], [5, 7, 2, 7, 7, 13, 14, 15]]  # (the tie at 1, 2 goes to 1; w of bin 6 is 0)
    rec1, _ = M.runs(mean, fmean, mx, fmax, mk, 1)
    assert rec1[:, 0].tolist() == [1, 5, 10]
    slices = np.zeros((2, 12), dtype=np.int32)
    slices[0, 5:8] = [10, 10, 12]  # T_0 = 3: sum = 32 - 3 * 3 = 23 against 3 * 3 * thr_act
    slices[1, 5:8] = [4, 4, 4]  # T_1 = 2: sum = 12 - 2 * 3 = 6 against 2 * 3 * thr_act
    assert M.activity(slices, fmean, rec, T=3, F=5, thr_act=1).tolist() == [[0, 0], [1, 1]]
    assert M.activity(slices, fmean, rec, T=3, F=5, thr_act=2).tolist() == [[0, 0], [1, 0]]


# ---- the oracle on the model capture -------------------------------------------------------------------------------------


def test_reference_capture_gives_its_four_channels(reference):
    p, st, res = reference
    assert (p["nfft"], p["h"], p["gap"], p["T"], p["S"]) == (8192, 1706, 17, 5, 234)
    assert st["candidates"] == 4 and len(st["runs"]) == 4  # four runs, none dropped
    assert st["runs"][:, :2].tolist() == [[2380, 2399], [3401, 3426], [5095, 5145], [6451, 7203]]
    assert [round(d["offset_hz"]) for d in res] == [-500006, -199991, 300000, 800563]
    M.check_four_channels(p, res)
    assert all(d["freq_hz"] == 455.5e6 + d["offset_hz"] for d in res)
    # the weak carrier is 20 dB under the strong one and the strong one leads
    assert abs((res[2]["snr_db"] - res[1]["snr_db"]) - 20.0) < 1.0
    assert max(res, key=lambda d: d["snr_db"]) is res[2] and res[0]["snr_db"] < 10.0 < res[0]["peak_db"]
    assert round(res[0]["duty"], 3) == 0.103 and round(res[0]["first_s"], 3) == 0.495 and round(res[0]["last_s"], 3) == 0.700


def test_package_host_arithmetic_equals_the_oracle(reference):
    p, st, res = reference
    plan = P.plan_find(FS, p["n"])
    got = FD.channels_from_records(plan, st["runs"], st["on"], st["mean"], 455.5e6)
    assert [dataclasses.asdict(ch) for ch in got] == res
    assert [dataclasses.asdict(ch) for ch in FD.channels_from_records(plan, st["runs"], st["on"], st["mean"])] == \
        M.result(p, st["runs"], st["on"], st["mean"], None)
    lines = [ch.line() for ch in got]
    assert lines[0] == "454999994 Hz: 5859 Hz wide, 6.5 dB over the floor, on 10 % (0.49 .. 0.70 s)"
    assert lines[2] == "455800000 Hz: 14941 Hz wide, 63.5 dB over the floor, on 100 % (0.00 .. 2.00 s)"
    assert FD.channels_from_records(plan, st["runs"], st["on"], st["mean"])[0].line().startswith("-500006 Hz: ")
    full = FD.FindResult(channels=got, sample_rate=FS, center_freq=455.5e6, seconds=2.0, nfft=8192, bin_hz=plan.bin_hz, frames=1170,
                         slice_frames=5, slices=234, threshold_db=6.0, peak_threshold_db=10.0, candidates=4)
    import json

    assert FD.FindResult.from_json(json.loads(json.dumps(full.to_json()))) == full
    assert full.lines() == lines and FD.FindResult().lines() == ["no channel found"]
    assert FD.channels_from_records(plan, np.zeros((0, 8), dtype=np.int64), np.zeros((0, 234), dtype=np.uint8), st["mean"]) == []
    # a run that is never on, and one kept without any weight
    rec = np.array([[10, 19, 2, 12, -5, 0, 0, 1200]], dtype=np.int64)
    ch = FD.channels_from_records(plan, rec, np.zeros((1, 234), dtype=np.uint8), st["mean"])[0]
    assert (ch.duty, ch.first_s, ch.last_s, ch.bursts) == (0.0, None, None, 0) and ch.offset_hz == (14.5 - 4096) * plan.bin_hz
    assert ch.line().endswith("on 0 %")


def test_noise_alone_gives_nothing():
    """The model capture without its carriers, and a shorter one with another seed: no hot bin.  Largest mean - fmean outside
    the DC guard 75 and 191 centi-dB (against 600), largest max - fmax 415 and 445 (against 1000)."""
    for kwargs, e_most, over_most in ((dict(secs=2.0, seed=3), 75, 415), (dict(secs=0.3, seed=11), 191, 445)):
        raw = M.capture(FS, carriers=False, **kwargs)
        p = M.plan(FS, raw.shape[0])
        st = M.run(M.rows(raw, p), p)
        out = np.abs(np.arange(p["nfft"]) - p["dc_bin"]) > p["dc_guard"]
        e, over = (st["mean"] - st["fmean"])[out], (st["max"] - st["fmax"])[out]
        print(kwargs, "largest mean - fmean", int(e.max()), "largest max - fmax", int(over.max()))
        assert int((st["mask"] & 1).sum()) == 0 and st["candidates"] == 0 and len(st["runs"]) == 0
        assert int(e.max()) < p["thr"] // 2 and int(over.max()) < p["thr_peak"] * 3 // 4  # well clear of the thresholds
        assert (int(e.max()), int(over.max())) == (e_most, over_most)
        assert (st["mean"] - st["fmean"])[p["dc_bin"]] > p["thr"]  # the DC offset is there, and guarded


# ---- CLI -----------------------------------------------------------------------------------------------------------------


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        cli.main(argv)
    assert exc.value.code == 2
    return capsys.readouterr().err


def test_cli_refuses_misuse(capsys):
    base = ["--in", "capture.wav"]
    for flag in (["--find-channels"], ["--find-top", "2"]):
        assert f"{flag[0]} cannot be combined with --ft." in _usage_error(base + flag + ["--ft", "455800000"], capsys)
        assert f"{flag[0]} cannot be combined with --benchmark." in _usage_error(base + flag + ["--benchmark"], capsys)
        assert f"{flag[0]} cannot be combined with --audio-post." in _usage_error(base + flag + ["--audio-post", "x"], capsys)
        assert f"{flag[0]} cannot be combined with --probe-only." in _usage_error(base + flag + ["--probe-only"], capsys)
    assert "--find-grid cannot be combined with --ft." in _usage_error(base + ["--find-grid", "12500", "--ft", "5e6"], capsys)
    assert "--find-threshold cannot be combined with --benchmark." in _usage_error(["--find-threshold", "5", "--benchmark"], capsys)
    for n in ("0", "6", "-1"):
        assert "--find-top must be between 1 and 5." in _usage_error(base + ["--find-top", n], capsys)
    for v in ("0", "-12500", "nan"):
        assert "--find-grid must be positive." in _usage_error(base + ["--find-top", "2", "--find-grid", v], capsys)
        assert "--find-threshold must be positive." in _usage_error(base + ["--find-channels", "--find-threshold", v], capsys)
    assert "--find-grid needs --find-top." in _usage_error(base + ["--find-channels", "--find-grid", "12500"], capsys)
    assert "--find-threshold needs --find-channels or --find-top." in _usage_error(base + ["--find-threshold", "5"], capsys)
    assert "--find-channels needs --in." in _usage_error(["--find-channels"], capsys)
    # without a find flag nothing changed: --ft is still required
    assert "Provide at least one --ft" in _usage_error(base, capsys)
    args = cli.build_parser().parse_args(base + ["--ft", "5e6"])
    assert (args.find_channels, args.find_top, args.find_grid, args.find_threshold) == (False, None, None, None)
    assert cli.check_find_args(cli.build_parser(), args) is False


def _channel(freq, snr):
    return FD.FoundChannel(offset_hz=freq - 455.5e6, freq_hz=freq, width_hz=1e4, snr_db=snr, peak_db=snr, level_db=-60.0, duty=1.0,
                           first_s=0.0, last_s=1.0, bursts=1, lo_bin=0, hi_bin=1)


def test_target_selection():
    res = FD.FindResult(channels=[_channel(454_999_994.0, 6.5), _channel(455_300_009.2, 43.9), _channel(455_799_999.9, 63.5),
                                  _channel(456_300_563.2, 58.6)], center_freq=455.5e6)
    assert FD.select_targets(res, 1) == [455_800_000.0]
    assert FD.select_targets(res, 2) == [455_800_000.0, 456_300_563.0]  # ascending, whatever the order of strength
    assert FD.select_targets(res, 2, 12_500.0) == [455_800_000.0, 456_300_000.0]
    assert FD.select_targets(res, 3, 12_500.0) == [455_300_000.0, 455_800_000.0, 456_300_000.0]
    assert FD.select_targets(res, 5, 25_000.0) == [455_000_000.0, 455_300_000.0, 455_800_000.0, 456_300_000.0]
    assert FD.select_targets(res, 5, 1e6) == [455e6, 456e6]  # duplicates after rounding are dropped
    # ties go to the lower frequency
    tie = FD.FindResult(channels=[_channel(100e6, 20.0), _channel(101e6, 30.0), _channel(102e6, 30.0), _channel(103e6, 20.0)])
    assert FD.select_targets(tie, 1) == [101e6] and FD.select_targets(tie, 3) == [100e6, 101e6, 102e6]
    # halves go up, on either side of zero offset
    assert FD.select_targets(FD.FindResult(channels=[_channel(6250.0, 1.0), _channel(18_750.0, 2.0)]), 2, 12_500.0) == [12_500.0, 25_000.0]
    with pytest.raises(ValueError, match="centre"):
        FD.select_targets(FD.FindResult(channels=[dataclasses.replace(_channel(1e6, 1.0), freq_hz=None)]), 1)
    assert FD.select_targets(FD.FindResult(), 3) == []


def test_package_surface():
    for name in ("ChannelFinder", "find_channels", "FindResult", "FoundChannel"):
        assert getattr(A, name) is getattr(FD, name)
    text = Path(FD.__file__).read_text()
    assert "scipy" not in text and "oracle" not in text
    with pytest.raises(ValueError, match="format"):
        FD.ChannelFinder(P.plan_find(FS, 100_000), "s8")
    with pytest.raises(ValueError, match="iq_order"):
        FD.ChannelFinder(P.plan_find(FS, 100_000), "s16", "qq")
    assert len(A.ProcessingConfig.__dataclass_fields__) == 23


# ---- C ABI ---------------------------------------------------------------------------------------------------------------


def test_c_abi_refuses_bad_arguments():
    """The library has the six entry points, and their argument checks come before any launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some = c_void_p(0), c_void_p(8)  # (never dereferenced: every call below is refused, or has nothing to do)
    names = ("iqa_find_accumulate", "iqa_find_mean", "iqa_find_floor", "iqa_find_mask", "iqa_find_runs", "iqa_find_activity")
    for name in names:
        assert hasattr(N.lib(), name) and name in N.EXPORTS
    assert N.lib().iqa_abi_version() == 1
    header = (Path(__file__).resolve().parent.parent / "include" / "iqa_hotpath.h").read_text()
    for macro in ("IQA_FIND_MAX_HALF 8191", "IQA_FIND_MAX_GAP 255", "IQA_FIND_MAX_SLICE_FRAMES 65536", "IQA_FIND_C_MIN (-30000)"):
        assert f"#define {macro}" in header
    i32, i64 = c_int32, c_int64

    def acc(rows=some, n=4, nbins=16, first=0, T=5, S=2, total=some, most=some, sl=some):
        N.call("iqa_find_accumulate", rows, i32(n), i32(nbins), i64(first), i32(T), i32(S), total, most, sl, null, null)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(nbins=-1), "negative"), (dict(first=-1), "negative"), (dict(T=0), "slice_frames"),
                         (dict(T=65537), "slice_frames"), (dict(S=0), "n_slices"), (dict(first=7), "past the last slice"),
                         (dict(n=11), "past the last slice"), (dict(rows=null), "NULL"), (dict(total=null), "NULL"), (dict(most=null), "NULL"),
                         (dict(sl=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            acc(**kwargs)
    acc(rows=null, n=0, total=null, most=null, sl=null)  # nothing to do
    acc(rows=null, nbins=0, total=null, most=null, sl=null)
    with pytest.raises(ValueError, match="frames must be"):
        N.call("iqa_find_mean", some, i32(16), i64(0), some, null)
    with pytest.raises(ValueError, match="negative"):
        N.call("iqa_find_mean", some, i32(-1), i64(5), some, null)
    for a, b in ((null, some), (some, null)):
        with pytest.raises(ValueError, match="NULL"):
            N.call("iqa_find_mean", a, i32(16), i64(5), b, null)
    N.call("iqa_find_mean", null, i32(0), i64(5), null, null)
    for half, num, den, what in ((-1, 1, 4, "half"), (8192, 1, 4, "half"), (5, -1, 4, "rank"), (5, 5, 4, "rank"), (5, 0, 0, "rank"),
                                 (5, 1, 65537, "rank")):
        with pytest.raises(ValueError, match=what):
            N.call("iqa_find_floor", some, i32(16), i32(half), i32(num), i32(den), some, null)
    for a, b in ((null, some), (some, null)):
        with pytest.raises(ValueError, match="NULL"):
            N.call("iqa_find_floor", a, i32(16), i32(5), i32(1), i32(4), b, null)
    with pytest.raises(ValueError, match="negative"):
        N.call("iqa_find_floor", some, i32(-4), i32(5), i32(1), i32(4), some, null)
    N.call("iqa_find_floor", null, i32(0), i32(5), i32(1), i32(4), null, null)

    def mask(ptrs=(some,) * 6, nbins=16, thr=600, thr_peak=1000, gap=17, dc_bin=8):
        N.call("iqa_find_mask", *ptrs[:4], i32(nbins), i32(thr), i32(thr_peak), i32(gap), i32(dc_bin), i32(3), *ptrs[4:], null)

    for kwargs, what in ((dict(gap=-1), "gap"), (dict(gap=256), "gap"), (dict(thr=1 << 20), "threshold"), (dict(thr_peak=-(1 << 20)), "threshold"),
                         (dict(dc_bin=-1), "dc_bin"), (dict(nbins=-1), "negative")):
        with pytest.raises(ValueError, match=what):
            mask(**kwargs)
    for k in range(6):
        with pytest.raises(ValueError, match="NULL"):
            mask(ptrs=tuple(null if i == k else some for i in range(6)))
    mask(ptrs=(null,) * 6, nbins=0)

    def runs(ptrs=(some,) * 5, nbins=16, min_hot=2, lst=some, cap=4, counts=some):
        N.call("iqa_find_runs", *ptrs, i32(nbins), i32(min_hot), lst, i64(cap), counts, null)

    for kwargs, what in ((dict(nbins=-1), "negative"), (dict(cap=-1), "negative"), (dict(min_hot=0), "min_hot"), (dict(counts=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            runs(**kwargs)

    def act(ptrs=(some,) * 3, J=2, nbins=16, F=9, T=5, S=2, thr_act=300, on=some):
        N.call("iqa_find_activity", *ptrs, i64(J), i32(nbins), i64(F), i32(T), i32(S), i32(thr_act), on, null)

    for kwargs, what in ((dict(J=-1), "negative"), (dict(nbins=-1), "negative"), (dict(T=0), "slice_frames"), (dict(T=65537), "slice_frames"),
                         (dict(S=0), "n_slices"), (dict(F=11), "ceil"), (dict(F=5), "ceil"), (dict(F=0), "ceil"), (dict(thr_act=1 << 20), "threshold"),
                         (dict(on=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            act(**kwargs)
    for k in range(3):
        with pytest.raises(ValueError, match="NULL"):
            act(ptrs=tuple(null if i == k else some for i in range(3)))
    act(ptrs=(null,) * 3, J=0, on=null)  # no run: nothing to do
    act(ptrs=(null,) * 3, nbins=0, on=null)
