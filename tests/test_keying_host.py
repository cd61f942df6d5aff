"""The keying measurement without a GPU (--find-decode): the numpy oracle of tests/keying_model.py against
plain Python loops, the model capture's runs, labels and decoders, the package's host arithmetic against the oracle, every rule
on both sides of its threshold, the skipped candidates, the dropped-decoder path, the centre rule, the partial rows of cut
windows, the CLI's usage errors and the entry point's argument checks."""
from __future__ import annotations

import importlib.util
import logging
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


K = _load("keying_model")
M = K.M

import iq_to_audio_amd as A  # noqa: E402
from iq_to_audio_amd import cli  # noqa: E402
from iq_to_audio_amd import describe as DS  # noqa: E402
from iq_to_audio_amd import keying as KY  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402

FIND = dict(D=40, delay=1600, hop=4096, T=5, F=1170)  # a find plan's figures: S = 234 slices of 5 frames
S = 234


def _stream(seed: int, n: int, flips: float = 0.2) -> np.ndarray:
    """A theta that crosses its centre now and then, with noise."""
    rng = np.random.default_rng(seed)
    sign = np.where(np.cumsum(rng.random(n) < flips) % 2 == 0, 1.0, -1.0)
    return (sign * 0.5 + 0.05 * rng.standard_normal(n)).astype(np.float32)


# ---- the oracle against loops -------------------------------------------------------------------------------------------------


def test_oracle_rows_against_loops():
    rng = np.random.default_rng(1)
    kp = K.plan(60000.0)
    for trial, (pos, n, front) in enumerate(((0, 5000, False), (2047, 3, True), (2048, 2048, False), (4090, 4200, True), (1, 1, True))):
        g = (rng.random(S) < 0.7).astype(np.uint8)
        theta = _stream(10 + trial, n)
        theta[:: 97] = np.nan
        fr = np.float32(-0.4) if front else None
        c = (0, 300, -12868, 12868, 7)[trial]
        got = K.rows(theta, pos, fr, c, kp["incs"], g, **FIND)
        want = K.rows_by_loops(theta, pos, fr, c, kp["incs"], g, **FIND)
        assert got.shape == (K.windows(pos, n), 16) and sorted(want) == list(range(pos // 2048, pos // 2048 + got.shape[0]))
        for j, w in enumerate(sorted(want)):
            assert got[j].tolist() == want[w], (trial, w)
    assert [K.windows(p, n) for p, n in ((0, 0), (5, -1), (0, 1), (0, 2048), (0, 2049), (2047, 2), (2047, 1), (100, 3 * 2048 + 5))] == [0, 0, 1, 1, 2, 2, 1, 4]


def test_oracle_quantiser_table_and_plan():
    q = K.quantise(np.array([0.0, 0.5 / 4096, 1.5 / 4096, 2.5 / 4096, -0.5 / 4096, np.nan, np.inf, -np.inf, 7.9999, -8.0, 3.14159274], dtype=np.float32))
    assert q.tolist() == [0, 0, 2, 2, 0, 0, 32767, -32767, 32767, -32767, 12868]
    t = K.table()
    assert t[0].tolist() == [1024, 0] and t[256].tolist() == [0, 1024] and t[512].tolist() == [-1024, 0] and t[768].tolist() == [0, -1024]
    assert np.abs(t[:, 0] ** 2 + t[:, 1] ** 2 - 1024 ** 2).max() <= 2 * 1024
    for fs_ch in (12000.0, 19200.0, 40000.0, 48000.0, 184615.38461538462, 800000.0):
        mine, pkg = K.plan(fs_ch), P.plan_keying(fs_ch)
        assert pkg.incs == mine["incs"] and pkg.skipped == mine["skipped"] and pkg.bauds == K.BAUDS == P.KEYING_BAUDS == A.KEYING_BAUDS
        np.testing.assert_array_equal(pkg.table, t)
        assert pkg.table.dtype == np.int16 and pkg.table.shape == (1024, 2) and all(0 <= i < 1 << 30 for i in pkg.incs)
    # skipped: B >= fs_ch / 4, the edge included
    assert P.plan_keying(12000.0).skipped == (False, False, False, False, True, True, True)
    assert P.plan_keying(19200.0).skipped == (False, False, False, False, False, True, True) and P.plan_keying(19200.0).incs[5:] == (0, 0)
    assert P.plan_keying(19200.1).skipped[5] is False
    assert P.plan_keying(40000.0).incs[1] == round(1200 * 2 ** 32 / 40000)
    with pytest.raises(ValueError, match="positive"):
        P.plan_keying(0.0)


def test_cut_windows_add_up():
    """A window cut by two calls gets a partial row from each; added by window number they are the uncut rows."""
    g = (np.random.default_rng(2).random(S) < 0.8).astype(np.uint8)
    kp = K.plan(48000.0)
    theta = _stream(3, 9000, 0.3)
    whole = K.stream_rows(theta, [9000], 40, 0, kp["incs"], g, **FIND)
    cuts = [1, 1, 2046, 2048, 2049, 1000, 1, 7, 1847]
    assert sum(cuts) == 9000
    np.testing.assert_array_equal(K.stream_rows(theta, cuts, 40, 0, kp["incs"], g, **FIND), whole)
    # the package's adder is the oracle's
    parts, pos = [], 0
    for n in cuts:
        parts.append((pos // 2048, K.rows(theta[pos : pos + n], pos, None if pos == 0 else theta[pos - 1], 40, kp["incs"], g, **FIND)))
        pos += n
    np.testing.assert_array_equal(KY.add_keying_rows(parts, 5), whole)
    # without the front value the pair across the cut is lost: the front is what makes the cut invisible
    lost = K.add_by_window([(0, K.rows(theta[:100], 0, None, 40, kp["incs"], g, **FIND)), (0, K.rows(theta[100:2048], 100, None, 40, kp["incs"], g, **FIND))], 1)
    assert lost[0, 0] in (whole[0, 0], whole[0, 0] - 1)
    # keyed from a later call on: the calls in front contribute nothing
    late = K.stream_rows(theta, [3000, 6000], 40, 3000, kp["incs"], g, **FIND)
    assert late[0].tolist() == [0] * 16 and late[1].sum() != 0 and (late[2:] == whole[2:]).all() and late[1, 0] < whole[1, 0]


def test_centre_rule():
    assert [K.centre(cr, ci) for cr, ci in ((1, 0), (0, 1), (-1, 0), (1, 1), (1000, -1))] == [0, 6434, 12868, 3217, -4]
    for cr, ci in ((1, 0), (0, 1), (-1, 0), (1, 1), (1000, -1), (-3, -4), (123456789012345, 98765432109876)):
        assert KY.keying_centre(cr, ci) == K.centre(cr, ci) and abs(K.centre(cr, ci)) <= 12868
    # the first call after which the describe rows hold 1024 pairs gives the centre, and the keying begins with that call
    row = lambda np_, cr, ci: [0, np_, 0, 0, 0, cr, ci, 0]  # noqa: E731
    rows = np.array([row(500, 10, 0), row(400, 10, 0), row(100, 0, 20), row(24, 0, 0), row(2000, -500, 0)], dtype=np.int64)
    assert K.centre_from_rows(rows, [2048, 4096, 100, 2048]) == (K.centre(20, 20), 6144)  # 1000 pairs after two calls, 1024 after the third
    assert K.centre_from_rows(rows[:3], [2048, 4096]) == (None, None)  # never 1024: no centre, no keying figures
    assert K.centre_from_rows(rows[4:], [2048]) == (12868, 0)


# ---- the model capture -------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def model():
    return K.model_run()


def test_model_capture_gives_its_runs_and_labels(model):
    """The numpy finder gives exactly the thirteen channels; section 22's labels and the keying labels are the table's."""
    found, described, keyed = model["found"], model["described"], model["keyed"]
    assert len(found) == len(K.CHANNELS) == 13
    for (name, offset, lab, key, _), ch, d, k in zip(K.CHANNELS, found, described, keyed):
        assert abs(ch["offset_hz"] - offset) <= (3000.0 if name == "wfm" else 1000.0), (name, ch["offset_hz"])
        print(name, d["label"], k["label"], k["c"], k["crossings"], k["pairs"], k["rate_hz"], k["coh"])
        assert d["label"] == lab and k["label"] == key, name
        assert k["c"] is not None and k["keyed_from"] == 0 and k["pairs"] >= 1024, name
    by = dict(zip(K.NAMES, keyed))
    # the figures the rules rest on, against the thresholds: at the true baud far over 0.35, everything unkeyed far under it
    for name, baud in (("fsk512", 512), ("fsk1200", 1200), ("fsk2400", 2400), ("gmsk9600", 9600), ("fsk4_4800", 4800), ("fsk_off", 1200)):
        k = by[name]
        assert k["coh"][K.BAUDS.index(baud)] >= 0.7 and 0.4 <= k["rate_hz"] / baud <= 0.6, name
        assert all(v < 0.35 / 2 for b, v in zip(K.BAUDS, k["coh"]) if b < baud), name  # nothing under the true baud
    for name in ("afsk", "voice", "voice_ctcss"):
        assert max(abs(v) for v in by[name]["coh"]) < 0.35 / 4, name
    # the off-centre channel: the finder's centroid and the centre together sit on the signal's middle, 675 Hz beside the
    # nominal frequency, within a tenth of the deviation
    j = K.NAMES.index("fsk_off")
    middle = found[j]["offset_hz"] + by["fsk_off"]["c"] / 4096.0 * described[j]["plan"]["fs_ch"] / (2.0 * np.pi)
    assert abs(middle - (K.CHANNELS[j][1] + 675.0)) <= 450.0, middle
    # the trap: a 1200 Hz tone crosses 2400 times a second, all on one clock.  At 2400 the rate window throws it out (rate / B =
    # 1); the rule as it stands then takes it at 4800, where the same crossings are coherent and rate / B = 0.5 (DESIGN.md
    # section 23, known limits): it ends without a decoder instead of as a pager
    trap = by["tone1200"]
    assert trap["coh"][3] >= 0.9 and abs(trap["rate_hz"] / 2400.0 - 1.0) < 0.01 and trap["coh"][1] < 0.1
    assert K.rule(trap["coh"][:5] + [None, None], trap["rate_hz"], trap["crossings"], trap["plan"]) == ("unkeyed", None)


def test_model_capture_decoders(model):
    from iq_to_audio_amd.keying import decoders_for

    for fc in (K.FC_AIR, K.FC_OUT):
        for (name, offset, lab, key, want), d, k in zip(K.CHANNELS, model["described"], model["keyed"]):
            tuned = fc + d["tuned_offset_hz"]
            if name == "am" and fc == K.FC_OUT:
                want = []
            assert K.decoders(lab, k["baud"], tuned) == want, (name, fc)
            names, note, bw = decoders_for(lab, k["baud"], tuned)
            assert names == want and (bw == 25000.0) == (want == ["ais"]) and bool(note) == (not want), (name, fc)
    assert decoders_for("nfm", 1600, None)[1] == decoders_for("nfm", 3200, None)[1] == "FLEX rates: no decoder here"
    assert decoders_for("nfm", 4800, None)[1] == "4800 baud (DMR / P25 / NXDN class): no decoder here"
    assert decoders_for("am", None, None)[0] == [] and decoders_for("am", None, 117.975e6)[0] == ["acars"] == decoders_for("am", None, 137e6)[0]
    assert decoders_for("am", None, 117.974e6)[0] == [] == decoders_for("am", None, 137.001e6)[0]
    for lab in ("carrier", "ssb", "unknown"):
        assert decoders_for(lab, None, 120e6) == ([], "no decoder", None)
    assert "adsb" not in {n for lab in DS.LABELS for b in (None,) + K.BAUDS for n in decoders_for(lab, b, 1090e6)[0]}


def test_package_host_arithmetic_equals_the_oracle(model):
    for name, d, k in zip(K.NAMES, model["described"], model["keyed"]):
        kp = P.plan_keying(d["plan"]["fs_ch"])
        got, want = KY.keying_figures(k["rows"], kp), K.figures(k["rows"], k["plan"])
        assert got == want, name
        assert KY.keying_label(got["coh"], got["rate_hz"], got["crossings"], kp) == K.rule(want["coh"], want["rate_hz"], want["crossings"], k["plan"])


def _about(label: str, demod=None, bw=None, tuned=None, freq=455.8e6):
    return A.ChannelDescription(offset_hz=3e5, freq_hz=freq, width_hz=11000.0, label=label, samples=90000, fs_ch=48000.0, cnr_db=40.0, env=0.001,
                                depth=0.03, carrier_hz=0.0, dev_hz=3000.0, line_share=0.2, demod=demod, bw=bw, tuned_offset_hz=None if tuned is None else 3e5,
                                tuned_hz=tuned)


def _rows(per_window, fs_ch=48000.0, baud_at=1, coherent=True, pairs=2047):
    """Window rows with ``per_window`` crossings each: all on one phase of candidate ``baud_at``'s clock, or none coherent."""
    out = np.zeros((len(per_window), 16), dtype=np.int64)
    for w, k in enumerate(per_window):
        out[w, 0], out[w, 1] = pairs, k
        out[w, 2 + 2 * baud_at] = 1024 * k if coherent else 0
    return out


def test_every_rule_at_its_boundary():
    kp = P.plan_keying(48000.0)
    lab = lambda coh, rate, K_: KY.keying_label(coh, rate, K_, kp)  # noqa: E731
    none = [0.0] * 7
    at = lambda k, v: none[:k] + [v] + none[k + 1 :]  # noqa: E731
    # 256 crossings
    assert lab(at(1, 0.9), 600.0, 255) == ("unkeyed", None) and lab(at(1, 0.9), 600.0, 256) == ("fsk 1200", 1200)
    # 0.35
    assert lab(at(1, np.nextafter(0.35, 0.0)), 600.0, 1000) == ("unkeyed", None) and lab(at(1, 0.35), 600.0, 1000) == ("fsk 1200", 1200)
    # 0.25 B and 0.8 B
    assert lab(at(1, 0.9), 300.0, 1000) == ("fsk 1200", 1200) and lab(at(1, 0.9), np.nextafter(300.0, 0.0), 1000) == ("unkeyed", None)
    assert lab(at(1, 0.9), 960.0, 1000) == ("fsk 1200", 1200) and lab(at(1, 0.9), np.nextafter(960.0, 1e9), 1000) == ("unkeyed", None)
    # the lowest candidate wins: a clock of 1200 is coherent at 2400, 4800 and 9600 too
    harmonics = [0.0, 0.98, 0.0, 0.96, 0.0, 0.98, 0.95]
    assert lab(harmonics, 600.0, 1000) == ("fsk 1200", 1200)
    assert lab(harmonics, 1300.0, 1000) == ("fsk 2400", 2400)  # only where the rate does not fit the lower one
    assert lab([0.9] * 7, 256.0, 1000) == ("fsk 512", 512)
    # a skipped candidate is never taken, whatever stands in its place
    low = P.plan_keying(12000.0)
    assert KY.keying_label([0.0, 0.0, 0.0, 0.0, 0.9, 0.9, 0.9], 1600.0, 1000, low) == ("unkeyed", None)
    assert KY.keying_label([0.0, 0.0, 0.0, 0.0, None, None, None], 1600.0, 1000, low) == ("unkeyed", None)
    # the figures from rows: crossings all on one phase give 1, none coherent gives -1 / (K - 1) per window, den = 0 gives None
    f = KY.keying_figures(_rows([20, 30, 10]), kp)
    assert f["coh"][1] == 1.0 and f["crossings"] == 60 and f["pairs"] == 3 * 2047 and f["rate_hz"] == 60 / (3 * 2047) * 48000.0
    assert f["coh"][0] == (0 - 1024 ** 2 * 60) / (1024 ** 2 * (20 * 19 + 30 * 29 + 10 * 9))
    assert KY.keying_figures(_rows([1, 1, 0]), kp)["coh"] == [None] * 7 and KY.keying_figures(_rows([]), kp)["rate_hz"] is None
    assert KY.keying_figures(_rows([20]), low)["coh"][4:] == [None] * 3
    # the largest window: 2048 crossings on one phase, exact in Python integers
    assert KY.keying_figures(_rows([2048] * 4, pairs=2048), kp)["coh"][1] == 1.0


def test_key_channel_and_the_dropped_decoder(caplog):
    kp = P.plan_keying(48000.0)
    nfm = _about("nfm", "nfm", 12500.0, 455.8e6)
    k = KY.key_channel(nfm, kp, _rows([30] * 10), 12, 2.4e6)
    assert (k.label, k.baud, k.decoders, k.bw, k.centre, k.crossings) == ("fsk 1200", 1200, ["pocsag"], 12500.0, 12, 300)
    assert k.line() == f"    keying: fsk 1200 (coh 1.00, {300 / 20470 * 48000.0:.0f} crossings/s) -> --pocsag"
    k = KY.key_channel(nfm, kp, _rows([300] * 10, baud_at=6), 0, 2.4e6)
    assert (k.label, k.decoders, k.bw) == ("fsk 9600", ["ais"], 25000.0) and k.line().endswith("-> --ais --bw 25000")
    # fs_ch as the pipeline resolves it: an explicit --fs-ch 24000 leaves AIS too few samples per bit, and the decoder is dropped
    with caplog.at_level(logging.INFO, logger="iq_to_audio_amd.keying"):
        k = KY.key_channel(nfm, kp, _rows([300] * 10, baud_at=6), 0, 2.4e6, fs_ch=24000.0)
    assert (k.label, k.decoders) == ("fsk 9600", []) and "--ais dropped: AIS at 9600 bit/s needs 5 to 100 samples per bit" in caplog.text
    assert KY.target_rate(2.4e6, "nfm") == 96000.0 and KY.target_rate(2.4e6, "wfm") == 480000.0 and KY.target_rate(2.4e6, "am", 24000.0) == 24000.0
    assert KY.usable_decoders(["rds"], 96000.0) == [] and KY.usable_decoders(["rds"], 480000.0) == ["rds"]
    assert KY.usable_decoders(["ax25", "tones"], 8000.0) == ["tones"]
    for baud_at, per, note in ((2, 30, "FLEX rates: no decoder here"), (5, 100, "4800 baud (DMR / P25 / NXDN class): no decoder here")):
        k = KY.key_channel(nfm, kp, _rows([per] * 10, baud_at=baud_at), 0, 2.4e6)
        assert k.decoders == [] and k.line().endswith("-> " + note), k.line()
    # unkeyed, and a channel that never held 1024 pairs: no figures, unkeyed
    k = KY.key_channel(nfm, kp, _rows([30] * 10, coherent=False), 0, 2.4e6)
    assert (k.label, k.decoders) == ("unkeyed", ["ax25", "tones"]) and "best coh" in k.line() and k.line().endswith("-> --ax25 --tones")
    k = KY.key_channel(nfm, kp, None, None, 2.4e6)
    assert (k.label, k.baud, k.centre, k.coh, k.rate_hz, k.crossings) == ("unkeyed", None, None, [None] * 7, None, 0) and "not measured" in k.line()
    # the other labels are not keyed FM
    k = KY.key_channel(_about("wfm", "wfm", 250000.0, 98.1e6), kp, _rows([30] * 10), 0, 2.4e6)
    assert (k.label, k.decoders) == (None, ["rds"]) and k.line() == "    keying: not measured (wfm) -> --rds"
    assert KY.key_channel(_about("am", "am", 10000.0, 131.55e6), kp, _rows([3]), 0, 2.4e6).decoders == ["acars"]
    assert KY.key_channel(_about("am", "am", 10000.0, 455.8e6), kp, _rows([3]), 0, 2.4e6).decoders == []
    assert KY.key_channel(_about("unknown"), kp, None, None, 2.4e6).line() == "    keying: not measured (unknown) -> no decoder"
    res = A.KeyingResult(channels=[KY.key_channel(nfm, kp, _rows([30] * 10), 12, 2.4e6), KY.key_channel(_about("unknown"), kp, None, None, 2.4e6)],
                         sample_rate=2.4e6, center_freq=455.5e6)
    assert A.KeyingResult.from_json(res.to_json()) == res and len(res.lines()) == 2
    import json

    assert A.KeyingResult.from_json(json.loads(json.dumps(res.to_json()))) == res


def test_auto_targets_carry_their_decoders():
    from iq_to_audio_amd.find import FindResult, FoundChannel

    def found(freq, snr):
        return FoundChannel(offset_hz=freq - 455.5e6, freq_hz=freq, width_hz=11000.0, snr_db=snr, peak_db=snr, level_db=-50.0, duty=1.0,
                            first_s=0.0, last_s=2.0, bursts=1, lo_bin=0, hi_bin=1)

    res = FindResult(channels=[found(455.6e6, 20.0), found(455.7e6, 30.0), found(455.8e6, 10.0)], center_freq=455.5e6)
    des = A.DescribeResult(channels=[_about("nfm", "nfm", 12500.0, 455.6e6), _about("nfm", "nfm", 25000.0, 455.7e6), _about("unknown")], center_freq=455.5e6)
    plain = DS.select_auto_targets(res, des, 2)
    assert plain == ([(455.6e6, "nfm", 12500.0), (455.7e6, "nfm", 25000.0)], [])
    with_decoders = DS.select_auto_targets(res, des, 2, extras=[("pocsag",), ("ais",), ()])
    assert with_decoders == ([(455.6e6, "nfm", 12500.0, ("pocsag",)), (455.7e6, "nfm", 25000.0, ("ais",))], [])


# ---- the CLI and the package surface -----------------------------------------------------------------------------------------


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        cli.main(argv)
    assert exc.value.code == 2
    return capsys.readouterr().err


def test_cli_refuses_misuse(capsys):
    base = ["--in", "capture.wav"]
    assert "--find-decode cannot be combined with --ft." in _usage_error(base + ["--find-decode", "--ft", "455800000"], capsys)
    assert "--find-decode cannot be combined with --benchmark." in _usage_error(base + ["--find-decode", "--benchmark"], capsys)
    assert "--find-decode cannot be combined with --audio-post." in _usage_error(base + ["--find-decode", "--audio-post", "x"], capsys)
    assert "--find-decode cannot be combined with --probe-only." in _usage_error(base + ["--find-decode", "--probe-only"], capsys)
    assert "--find-decode needs --in." in _usage_error(["--find-decode"], capsys)
    assert "--find-auto needs --find-top." in _usage_error(base + ["--find-decode", "--find-auto"], capsys)
    for name in ("pocsag", "ais", "rds"):  # the decoders are chosen, not given
        assert f"--find-auto cannot be combined with --{name}." in _usage_error(base + ["--find-top", "2", "--find-auto", "--find-decode", f"--{name}"], capsys)
    # --find-decode implies --find-describe and --find-channels: a threshold is accepted with it alone
    args = cli.build_parser().parse_args(base + ["--find-decode", "--find-threshold", "8"])
    assert cli.check_find_args(cli.build_parser(), args) is True and (args.find_decode, args.find_describe) == (True, False)
    args = cli.build_parser().parse_args(base + ["--find-describe"])
    assert args.find_decode is False


def test_package_surface():
    for name in ("ChannelKeying", "KeyingResult"):
        assert getattr(A, name) is getattr(KY, name)
    assert A.plan_keying is P.plan_keying and A.KEYING_BAUDS == (512, 1200, 1600, 2400, 3200, 4800, 9600)
    for module in (DS, KY):
        text = Path(module.__file__).read_text()
        assert "scipy" not in text and "import oracle" not in text and "from oracle" not in text
    plan = P.plan_find(2.4e6, 100_000)
    fin = dict(runs=np.zeros((0, 8), dtype=np.int64), on=np.zeros((0, plan.slices), dtype=np.uint8))
    with pytest.raises(ValueError, match="without keying=True"):
        DS.ChannelDescriber(plan, fin, []).finish_keying()
    with pytest.raises(ValueError, match="keying=True needs describe=True"):
        A.find_channels("nothing.wav", keying=True)


def test_c_abi_refuses_bad_arguments():
    """The library has the two entry points, and the argument checks come before the launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some = c_void_p(0), c_void_p(8)  # (never dereferenced: every call below is refused, or has nothing to do)
    for name in ("iqa_keying_accumulate", "iqa_keying_windows"):
        assert hasattr(N.lib(), name) and name in N.EXPORTS
    assert N.lib().iqa_abi_version() == 1
    header = (Path(__file__).resolve().parent.parent / "include" / "iqa_hotpath.h").read_text()
    assert "#define IQA_KEYING_BAUDS 7" in header and "#define IQA_KEYING_SUMS 16" in header and "#define IQA_ABI_VERSION 1" in header
    assert (P.KEYING_WINDOW, P.KEYING_SUMS, len(P.KEYING_BAUDS)) == (2048, 16, 7)
    windows = N.lib().iqa_keying_windows
    cases = ((0, -5), (0, 0), (0, 1), (0, 2048), (0, 2049), (2047, 1), (2047, 2), (100, 3 * 2048 + 5), (1 << 35, 1), ((1 << 35) + 2047, 2049), (0, 1 << 36))
    assert [windows(p, n) for p, n in cases] == [K.windows(p, n) for p, n in cases] == [0, 0, 1, 1, 2, 1, 2, 4, 1, 2, 1 << 25]
    i32, i64 = c_int32, c_int64
    good = (c_int32 * 7)(*P.plan_keying(48000.0).incs)

    def acc(theta=some, n=100, pos=0, front=null, c=0, inc=good, cs=some, D=40, delay=1600, hop=4096, T=5, F=1170, S=234, gate=some, out=some):
        N.call("iqa_keying_accumulate", theta, i64(n), i64(pos), front, i32(c), inc, cs, i32(D), i32(delay), i32(hop), i32(T), i64(F), i32(S),
               gate, out, null)

    def incs(k, v):
        a = list(good)
        a[k] = v
        return (c_int32 * 7)(*a)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(pos=-1), "negative"), (dict(n=(1 << 36) + 1), "n out of range"), (dict(c=32768), "centre"),
                         (dict(c=-32768), "centre"), (dict(inc=incs(0, 1 << 30)), "clock step"), (dict(inc=incs(6, -1)), "clock step"),
                         (dict(inc=None), "inc must"), (dict(D=0), "D and hop"), (dict(hop=0), "D and hop"), (dict(delay=-1), "delay"),
                         (dict(T=0), "T must"), (dict(T=65537), "T must"), (dict(F=0), "ceil"), (dict(S=0), "ceil"), (dict(S=233), "ceil"),
                         (dict(S=235), "ceil"), (dict(F=1171), "ceil"), (dict(pos=1 << 60), "2\\^62"), (dict(pos=(1 << 62) // 40 - 99), "2\\^62"),
                         (dict(front=some), "front must be NULL at pos 0"), (dict(theta=null), "NULL"), (dict(cs=null), "NULL"),
                         (dict(gate=null), "NULL"), (dict(out=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            acc(**kwargs)
    acc(theta=null, n=0, cs=null, gate=null, out=null, inc=None)  # nothing to do: no pointer is touched
    acc(theta=null, n=0, pos=7, front=some, cs=null, gate=null, out=null)
    acc(theta=null, n=0, c=32767, inc=incs(3, (1 << 30) - 1), cs=null, gate=null, out=null)
