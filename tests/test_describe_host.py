"""The channel description (--find-describe), the host side: the numpy oracle (tests/describe_model.py)
against plain loops on small streams, the plan at its clamps, the oracle alone on the model capture (thirteen channels come
back with the labels and figures the modulation put there), every rule's boundary, the suggestions, the package's host
arithmetic against the oracle's, the CLI's flag checks, the C ABI.  No GPU compute."""
from __future__ import annotations

import dataclasses
import importlib.util
import math
import sys
from ctypes import c_int32, c_int64, c_void_p
from pathlib import Path

import numpy as np
import pytest

import iq_to_audio_amd as A
from iq_to_audio_amd import cli
from iq_to_audio_amd import describe as DS
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


M = _load("describe_model")
FS = M.FS


@pytest.fixture(scope="module")
def model():
    """The model capture through the oracle, once per session: name -> the channel's description."""
    run = M.model_run()
    assert len(run["found"]) == len(M.CHANNELS)  # the finder keeps exactly the thirteen runs
    by_name = {}
    for (name, offset, _), ch, d in zip(M.CHANNELS, run["found"], run["described"]):
        assert abs(ch["offset_hz"] - offset) <= (3000.0 if name in ("wfm", "usb") else 2 * run["p"]["bin_hz"]), (name, ch["offset_hz"])
        by_name[name] = d
    return run, by_name


# ---- the oracle against plain loops ----------------------------------------------------------------------------------------


def test_oracle_sums_against_loops():
    rng = np.random.default_rng(1)
    find = dict(D=7, delay=11, hop=16, T=3, F=10)  # S = 4 slices of 48 raw frames; the last one short and clamped
    g = np.array([1, 0, 1, 1], dtype=np.uint8)
    z = (rng.standard_normal(300) + 1j * rng.standard_normal(300)).astype(np.complex64) * np.float32(0.01)
    z[5] = complex(np.nan, 1.0)
    z[6] = complex(np.inf, -np.inf)
    z[7] = 1e6  # past the clamp
    z[8] = complex(2.5, 3.5) / 2 ** 12  # exact ties at sh = 12: 2.5 -> 2, 3.5 -> 4
    for sh in (12, 0, -30, 30):
        for pos, prev in ((0, None), (3, None), (3, complex(0.003, -0.004)), (40, complex(np.nan, np.inf))):
            want = M.sums_by_loops(z, pos, prev, sh, g, **find)
            got = M.add_rows(M.rows(z, pos, prev, sh, g, **find))
            assert got == want, (sh, pos, prev)
    assert M.quantise(np.float32([2.5, 3.5, -2.5, np.nan, np.inf, -np.inf, 40000.0, -40000.0]) / np.float32(4096.0), 12).tolist() == [
        2, 4, -2, 0, 32767, -32767, 32767, -32767]
    # the gate: slice edges at raw frames 48, 96, 144; sample m at raw frame max(7 m - 11, 0)
    m = np.arange(40)
    want = [g[min(max(7 * k - 11, 0) // 16, 9) // 3] for k in range(40)]
    assert M.gate_of(m, g, **find).tolist() == want and want[:9] == [1] * 9 and want[9] == 0
    # the cut of a stream into calls changes nothing
    whole = M.add_rows(M.rows(z, 0, None, 12, g, **find))
    parts = [0, 1, 2, 100, 101, 300]
    tot = [0] * 8
    for a, b in zip(parts, parts[1:]):
        tot = [t + v for t, v in zip(tot, M.add_rows(M.rows(z[a:b], a, None if a == 0 else z[a - 1], 12, g, **find)))]
    assert tuple(tot) == whole


def test_oracle_isqrt_and_erosion():
    roots = np.array([0, 1, 2, 3, 65535, 46340, (1 << 31) - 1, 2147352578], dtype=np.int64)
    for v in np.concatenate((roots * roots, roots * roots - 1, roots * roots + 1, [2 * 32767 ** 2, (2 * 32767 ** 2) ** 2])).tolist():
        if 0 <= v < 1 << 62:
            assert int(M.isqrt(np.array([v]))[0]) == math.isqrt(v), v
    assert M.erode([1, 1, 1]).tolist() == [1, 1, 1] and M.erode([0, 1, 1, 1, 0, 1]).tolist() == [0, 0, 1, 0, 0, 0]
    assert M.erode([1]).tolist() == [1] and M.erode([0]).tolist() == [0] and M.erode([1, 0]).tolist() == [0, 0]
    for on in ([1, 1, 0, 1, 1, 1, 0], [0, 0], [1, 1, 1, 1]):
        assert DS.erode_gate(on).tolist() == M.erode(on).tolist() and DS.erode_gate(on).dtype == np.uint8


# ---- the plan ----------------------------------------------------------------------------------------------------------------


def test_plan_at_its_clamps():
    p = P.plan_describe(FS, 300e3, 14941.0)  # an NFM channel: twice its width
    assert (p.bw, p.decimation, p.fs_ch, p.delay) == (29882.0, 40, 60000.0, (len(p.taps) - 1) // 2)
    np.testing.assert_array_equal(p.taps, P.design_channel_filter(FS, 29882.0, 40))
    assert not p.taps.flags.writeable
    narrow = P.plan_describe(FS, -900e3, 879.0)  # the lower clamps: 6 kHz of filter, 12 kHz of rate
    assert (narrow.bw, narrow.decimation, narrow.fs_ch) == (6000.0, 200, 12000.0)
    wide = P.plan_describe(FS, 950e3, 400e3)  # the upper clamp: a quarter of the capture
    assert (wide.bw, wide.decimation, wide.fs_ch) == (600e3, 2, 1.2e6)
    edge = P.plan_describe(FS, 0.0, 3000.0)  # 2 width = 6000 exactly
    assert edge.bw == 6000.0 and P.plan_describe(FS, 0.0, 3000.5).bw == 6001.0
    for name in ("bw", "fs_ch", "delay"):
        for a, b in ((p, M.plan(FS, 300e3, 14941.0)), (wide, M.plan(FS, 950e3, 400e3))):
            assert getattr(a, name) == b[name]
    assert p.decimation == M.plan(FS, 300e3, 14941.0)["D"]
    for args, what in (((0.0, 0.0, 1e3), "sample rate"), ((FS, 0.0, 0.0), "width"), ((FS, 0.0, math.nan), "width"),
                       ((FS, 1.3e6, 1e3), "offset"), ((FS, math.inf, 1e3), "offset")):
        with pytest.raises(ValueError, match=what):
            P.plan_describe(*args)


# ---- the model capture -------------------------------------------------------------------------------------------------------


def test_model_capture_gives_its_labels(model):
    run, by_name = model
    for name in M.NAMES:
        d = by_name[name]
        print(name, d["label"], {k: (None if d[k] is None else round(d[k], 4)) for k in ("cnr_db", "env", "depth", "carrier_hz", "dev_hz", "line_share")},
              "N", d["samples"], "sh", d["sh"])
    assert {name: by_name[name]["label"] for name in M.NAMES} == M.LABELS
    assert sorted(set(M.LABELS.values())) == ["am", "carrier", "nfm", "ssb", "unknown", "wfm"]
    # the documented limit: the faint NFM channel stays under the 26 dB and its noise shows in env
    assert by_name["nfm_faint"]["cnr_db"] < 26.0 and by_name["nfm_faint"]["env"] > 0.02
    assert by_name["am_faint"]["cnr_db"] >= 26.0


def test_model_capture_figures(model):
    _, d = model
    for name, want in (("nfm_tone", 3.0 * 1000.0), ("nfm_weak", 2.5 * 700.0), ("burst", 3.0 * 400.0)):
        assert abs(d[name]["dev_hz"] / (want / math.sqrt(2.0)) - 1.0) <= 0.03, (name, d[name]["dev_hz"])
    assert abs(d["fsk"]["dev_hz"] / 4500.0 - 1.0) <= 0.03, d["fsk"]["dev_hz"]
    for name in ("am_tone", "am_faint"):
        assert abs(d[name]["env"] - 0.401) <= 0.02, (name, d[name]["env"])
    assert abs(d["am_tone"]["depth"] - 0.5) <= 0.03, d["am_tone"]["depth"]
    assert abs(d["carrier"]["carrier_hz"]) < 1.0, d["carrier"]["carrier_hz"]
    # the eroded gate keeps the burst's ramps out
    assert d["burst"]["env"] < 0.005 and 0 < d["burst"]["samples"] < 0.1 * 2.0 * d["burst"]["fs_ch"]


def test_package_host_arithmetic_equals_the_oracle(model):
    run, _ = model
    p, st = run["p"], run["st"]
    plan = P.plan_find(FS, p["n"])
    assert (plan.hop, plan.slice_frames, plan.frames, plan.slices, plan.dc_bin) == (p["hop"], p["T"], p["F"], p["S"], p["dc_bin"])
    fin = dict(runs=st["runs"], on=st["on"], slice=st["slice"], fmean=st["fmean"], mean=st["mean"])
    for fc in (None, 455.5e6, 7.1e6):
        chans = FD.channels_from_records(plan, st["runs"], st["on"], st["mean"], fc)
        for ch, want in zip(chans, run["described"]):
            dp = P.plan_describe(FS, ch.offset_hz, ch.width_hz)
            got = DS.describe_channel(plan, fin, ch, want["gate"], want["sums"], dp, fc)
            ref = M.describe(p, st, dataclasses.asdict(ch), want["gate"], want["sums"], want["plan"], fc)
            for key, value in dataclasses.asdict(got).items():  # (float64 from the same integers: a few roundings apart at most)
                same = value == ref[key] if not isinstance(value, float) else abs(value - ref[key]) <= 1e-12 * max(abs(value), 1.0)
                assert same, (ch.offset_hz, key, value, ref[key])
            assert got.line().startswith(f"    {got.label}: ")
    z = np.float32([3e-4, 4e-4])
    for power, sh in ((0.0, 15), (math.nan, 15), (math.inf, -30), (1.0, 10), (1.0001, 9), (2.0 ** -20, 20), (1e-30, 30), (1e30, -30),
                      (float(np.mean(z.astype(np.float64) ** 2) * 2), M.choose_shift(z[:1] + 1j * z[1:]))):
        assert DS.choose_shift(power) == sh, power
    assert M.choose_shift(np.zeros(4, dtype=np.complex64)) == 15 and M.choose_shift(np.ones(4, dtype=np.complex64)) == 10
    big = np.array([[1 << 56, -(1 << 40), 5, 0, 0, 0, 0, 0]] * 300, dtype=np.int64)
    assert DS.add_rows(big) == M.add_rows(big) == (300 << 56, -300 << 40, 1500, 0, 0, 0, 0, 0) and 300 << 56 > 1 << 63


# ---- the rules ---------------------------------------------------------------------------------------------------------------


def test_every_rule_at_its_boundary():
    for label in (DS.label_of, M.label):
        fm = dict(N=5000, cnr_db=40.0, width_hz=12e3, env=0.001, dev_hz=2000.0, line=0.2)

        def at(**change):
            a = {**fm, **change}
            return label(a["N"], a["cnr_db"], a["width_hz"], a["env"], a["dev_hz"], a["line"])

        assert at() == "nfm"
        assert at(N=1023) == "unknown" and at(N=1024) == "nfm"
        assert at(cnr_db=25.999) == "unknown" and at(cnr_db=26.0) == "nfm"
        assert at(width_hz=100_000.0) == "wfm" and at(width_hz=99_999.0) == "nfm"
        assert at(width_hz=2e5, env=0.0499) == "wfm" and at(width_hz=2e5, env=0.05) == "unknown"
        assert at(env=0.0199) == "nfm" and at(env=0.02) == "unknown"  # (wide for ssb, no line for am)
        assert at(dev_hz=49.9) == "carrier" and at(dev_hz=50.0) == "nfm"
        assert at(env=0.4, line=0.6) == "am" and at(env=0.4, line=0.599) == "unknown"
        assert at(env=0.4, line=0.599, width_hz=5999.0) == "ssb" and at(env=0.4, line=0.599, width_hz=6000.0) == "unknown"
        assert at(env=0.4, line=0.9, width_hz=3000.0) == "am"  # am comes before ssb
        assert at(N=10, width_hz=2e5) == "unknown" and at(cnr_db=10.0, env=0.4, line=0.9) == "unknown"  # the first rule comes first
    assert DS.label_of(5000, None, 12e3, None, None, None) == "unknown"
    # a zero S1, E or A makes the channel unknown
    ok = (5000, 4999, 10 ** 9, 10 ** 12, 10 ** 6, 10 ** 8, 10 ** 7, 10 ** 9)
    assert DS.stream_figures(ok, 12e3) is not None and M.figures(ok, 12e3) is not None
    for k in (2, 4, 7):
        zero = tuple(0 if i == k else v for i, v in enumerate(ok))
        assert DS.stream_figures(zero, 12e3) is None and M.figures(zero, 12e3) is None


def test_suggestions_and_tuned_offsets():
    base = dict(offset_hz=300e3, carrier_hz=-12.5, width_hz=12e3, freq_hz=455.8e6, dc_bin=4096, bin_hz=FS / 8192)
    for suggest, lo_hi in ((DS.suggestion, ("lo_bin", "hi_bin")), (M.suggest, ("lo", "hi"))):
        def s(label, **change):
            a = {**base, lo_hi[0]: 5100, lo_hi[1]: 5112, **change}
            return suggest(label, **a)

        assert s("nfm") == ("nfm", 12500.0, 300e3 - 12.5) and s("carrier") == ("nfm", 12500.0, 300e3 - 12.5)
        assert s("nfm", width_hz=16000.0)[1] == 12500.0 and s("nfm", width_hz=16000.1)[1] == 25000.0
        assert s("am") == ("am", 10000.0, 300e3 - 12.5) and s("wfm") == ("wfm", 250000.0, 300e3 - 12.5)
        assert s("unknown") == (None, None, None)
        # usb / lsb: the amateur convention, from the run's edges
        usb_at, lsb_at = (5100 - 4096) * FS / 8192 - 300.0, (5112 + 1 - 4096) * FS / 8192 + 300.0
        assert s("ssb") == ("usb", 3000.0, usb_at) and s("ssb", freq_hz=None) == ("usb", 3000.0, usb_at)
        assert s("ssb", freq_hz=10e6) == ("usb", 3000.0, usb_at) and s("ssb", freq_hz=9_999_999.0) == ("lsb", 3000.0, lsb_at)


def _found(freq, snr, fc=455.5e6):
    return FD.FoundChannel(offset_hz=freq - fc, freq_hz=freq, width_hz=1e4, snr_db=snr, peak_db=snr, level_db=-60.0, duty=1.0, first_s=0.0,
                           last_s=1.0, bursts=1, lo_bin=0, hi_bin=1)


def _about(ch, label, demod=None, bw=None, shift=0.0):
    known = demod is not None
    return DS.ChannelDescription(offset_hz=ch.offset_hz, freq_hz=ch.freq_hz, width_hz=ch.width_hz, label=label, samples=5000, fs_ch=24e3, cnr_db=40.0,
                                 env=0.0, depth=0.0, carrier_hz=shift, dev_hz=1e3, line_share=0.3, demod=demod, bw=bw,
                                 tuned_offset_hz=ch.offset_hz + shift if known else None, tuned_hz=ch.freq_hz + shift if known else None)


def test_auto_target_selection():
    chans = [_found(455.0e6, 50.0), _found(455.3e6, 70.0), _found(455.8e6, 60.0), _found(456.3e6, 65.0)]
    abouts = [_about(chans[0], "am", "am", 10000.0, 40.0), _about(chans[1], "unknown"), _about(chans[2], "nfm", "nfm", 12500.0, -300.0),
              _about(chans[3], "wfm", "wfm", 250000.0)]
    res, des = FD.FindResult(channels=chans, center_freq=455.5e6), DS.DescribeResult(channels=abouts, sample_rate=FS, center_freq=455.5e6)
    targets, skipped = DS.select_auto_targets(res, des, 2)
    assert targets == [(455_799_700.0, "nfm", 12500.0), (456.3e6, "wfm", 250000.0)] and skipped == [chans[1]]
    targets, skipped = DS.select_auto_targets(res, des, 5, 12500.0)  # every known one, on the grid, ascending
    assert targets == [(455.0e6, "am", 10000.0), (455.8e6, "nfm", 12500.0), (456.3e6, "wfm", 250000.0)] and skipped == [chans[1]]
    assert DS.select_auto_targets(res, des, 1) == ([(456.3e6, "wfm", 250000.0)], [chans[1]])
    none = DS.DescribeResult(channels=[_about(c, "unknown") for c in chans], sample_rate=FS, center_freq=455.5e6)
    assert DS.select_auto_targets(res, none, 3) == ([], chans[1:2] + chans[3:4] + chans[2:3] + chans[0:1])
    with pytest.raises(ValueError, match="centre"):
        DS.select_auto_targets(res, DS.DescribeResult(channels=abouts, sample_rate=FS), 2)


# ---- the CLI and the package surface -----------------------------------------------------------------------------------------


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        cli.main(argv)
    assert exc.value.code == 2
    return capsys.readouterr().err


def test_cli_refuses_misuse(capsys):
    base = ["--in", "capture.wav"]
    for flag in (["--find-describe"], ["--find-top", "2", "--find-auto"]):
        name = flag[0]
        assert f"{name} cannot be combined with --ft." in _usage_error(base + flag + ["--ft", "455800000"], capsys)
        assert f"{name} cannot be combined with --benchmark." in _usage_error(base + flag + ["--benchmark"], capsys)
        assert f"{name} cannot be combined with --audio-post." in _usage_error(base + flag + ["--audio-post", "x"], capsys)
        assert f"{name} cannot be combined with --probe-only." in _usage_error(base + flag + ["--probe-only"], capsys)
    assert "--find-auto needs --find-top." in _usage_error(base + ["--find-auto"], capsys)
    assert "--find-auto needs --find-top." in _usage_error(base + ["--find-describe", "--find-auto"], capsys)
    assert "--find-auto cannot be combined with --pocsag." in _usage_error(base + ["--find-top", "2", "--find-auto", "--pocsag"], capsys)
    assert "--find-describe needs --in." in _usage_error(["--find-describe"], capsys)
    assert "--find-grid needs --find-top." in _usage_error(base + ["--find-describe", "--find-grid", "12500"], capsys)
    # --find-describe implies --find-channels: a threshold is accepted with it alone
    args = cli.build_parser().parse_args(base + ["--find-describe", "--find-threshold", "8"])
    assert cli.check_find_args(cli.build_parser(), args) is True and (args.find_describe, args.find_auto) == (True, False)
    args = cli.build_parser().parse_args(base + ["--ft", "5e6"])
    assert (args.find_describe, args.find_auto) == (False, False) and cli.check_find_args(cli.build_parser(), args) is False


def test_package_surface():
    for name in ("ChannelDescriber", "ChannelDescription", "DescribeResult"):
        assert getattr(A, name) is getattr(DS, name)
    text = Path(DS.__file__).read_text()
    assert "scipy" not in text and "import oracle" not in text and "from oracle" not in text
    assert len(A.ProcessingConfig.__dataclass_fields__) == 23
    plan = P.plan_find(FS, 100_000)
    fin = dict(runs=np.zeros((0, 8), dtype=np.int64), on=np.zeros((0, plan.slices), dtype=np.uint8))
    with pytest.raises(ValueError, match="format"):
        DS.ChannelDescriber(plan, fin, [], "s8")
    with pytest.raises(ValueError, match="iq_order"):
        DS.ChannelDescriber(plan, fin, [], "s16", "qq")
    with pytest.raises(ValueError, match="no run of this finder"):
        DS.ChannelDescriber(plan, fin, [_found(455.8e6, 30.0)])
    res = DS.DescribeResult(channels=[_about(_found(455.8e6, 30.0), "nfm", "nfm", 12500.0), _about(_found(455.9e6, 30.0), "unknown")],
                            sample_rate=FS, center_freq=455.5e6)
    assert DS.DescribeResult.from_json(res.to_json()) == res
    assert res.lines()[0].endswith("-> --demod nfm --bw 12500 at 455800000 Hz") and res.lines()[1].startswith("    unknown: C/N 40.0 dB")


def test_c_abi_refuses_bad_arguments():
    """The library has the two entry points, and the argument checks come before the launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some = c_void_p(0), c_void_p(8)  # (never dereferenced: every call below is refused, or has nothing to do)
    for name in ("iqa_describe_accumulate", "iqa_describe_tiles"):
        assert hasattr(N.lib(), name) and name in N.EXPORTS
    assert N.lib().iqa_abi_version() == 1
    header = (Path(__file__).resolve().parent.parent / "include" / "iqa_hotpath.h").read_text()
    assert "#define IQA_DESCRIBE_MAX_SHIFT 30" in header and P.DESCRIBE_MAX_SHIFT == 30 and P.DESCRIBE_TILE == M.TILE == 2048
    tiles = N.lib().iqa_describe_tiles
    assert [tiles(n) for n in (-5, 0, 1, 2047, 2048, 2049, 3 * 2048 + 5, 1 << 36)] == [0, 0, 1, 1, 1, 2, 4, 1 << 25]
    i32, i64 = c_int32, c_int64

    def acc(z=some, n=100, pos=0, prev=null, sh=12, D=40, delay=1600, hop=4096, T=5, F=1170, S=234, gate=some, out=some):
        N.call("iqa_describe_accumulate", z, i64(n), i64(pos), prev, i32(sh), i32(D), i32(delay), i32(hop), i32(T), i64(F), i32(S), gate,
               out, null)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(pos=-1), "negative"), (dict(n=(1 << 36) + 1), "n out of range"), (dict(sh=31), "sh must"),
                         (dict(sh=-31), "sh must"), (dict(D=0), "D and hop"), (dict(hop=0), "D and hop"), (dict(delay=-1), "delay"),
                         (dict(T=0), "T must"), (dict(T=65537), "T must"), (dict(F=0), "ceil"), (dict(S=0), "ceil"), (dict(S=233), "ceil"),
                         (dict(S=235), "ceil"), (dict(F=1171), "ceil"), (dict(pos=1 << 60), "2\\^62"), (dict(pos=(1 << 62) // 40 - 99), "2\\^62"),
                         (dict(prev=some), "prev must be NULL at pos 0"), (dict(z=null), "NULL"), (dict(gate=null), "NULL"), (dict(out=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            acc(**kwargs)
    acc(z=null, n=0, gate=null, out=null)  # nothing to do: no pointer is touched
    acc(z=null, n=0, pos=7, prev=some, gate=null, out=null)
