"""The NXDN frame decoding (--find-nxdn) on the MI355X: ``NxdnDecoder`` on the synthesised test stream at
160 000 Hz (a header frame with a VCALL in both FACCH1s, two voice superframes, a frame with a FACCH1 in its second half alone
and the release: 11 frames, 0.44 s), clean, at the noise level that tests/test_nxdn_host.py finds, negated and at 2400 symbols/s:
the plane, the hits, the bits, the levels, the class masks, the information words, the records, the frames, the calls and the
control lines equal the model's of tests/nxdn_model.py, applied to the GPU's own integrator plane; a stream cut unevenly gives
identical output; a control stream gives its folded lines; the CLI on a model capture with an NXDN channel: --find-nxdn prints
the calls and writes nxdn.json, a --find-identify run calls no entry point of this section and writes the same four JSON files,
and ysf and nxdn together return both results in table order.  Every comparison is of integers and exact."""
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


NM = _load("nxdn_model")
IM = NM.IM
FS = 160_000.0
FC = 433.0e6
NOISE = 0.06  # test_nxdn_host.py's: the largest at which the model alone still decodes every frame of this stream
#: case -> (the arguments of the model's test stream, the symbol rate)
CASES = {"clean": (dict(), 4800), "noise": (dict(noise=NOISE), 4800), "negated": (dict(negate=True), 4800), "rate2400": (dict(rate=2400), 2400),
         "control": (dict(script=NM.CONTROL_SCRIPT), 4800)}
CLEAN = dict(no_level=0, cut=0, lich_inner=0, lich_failed=0, sacch_failed=0, facch_failed=0, cac_failed=0, superframe_broken=0, udch=0,
             inbound_cac=0, fixed=0)
STAGES = ("rows", "bits", "levels", "classes", "info", "rec")


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


@pytest.fixture(scope="module")
def runs(A):
    """Every case through ``NxdnDecoder`` once, and the model on the GPU's own plane."""
    out = {}
    for case, (args, rate) in CASES.items():
        theta = NM.test_stream(FS, **args)
        dec = A.NxdnDecoder(FS, rate=rate)
        dec.process(theta)
        result = dec.finish()
        st = dec.stages()
        pl = NM.plan(FS, rate)
        _, kept = IM.search(st["v"], pl["ident"], NM.NXDN_PATTERNS)
        out[case] = dict(theta=theta, result=result, st=st, plan=pl, kept=kept, want=NM.decode_plane(st["v"], kept, pl))
    return out


def _equals_the_model(A, r, rate):
    """The stages, the frames, the calls and the control lines of one run, held to the model value for value."""
    st, want, pl = r["st"], r["want"], r["plan"]
    np.testing.assert_array_equal(st["v"], IM.integrate(r["theta"], 0, pl["ident"]["L"], pl["ident"]["sh"]))  # the plane and the hits are section 25's
    assert st["hits"].tolist() == [list(h) for h in r["kept"]]
    for name in STAGES:
        assert st[name].shape == want[name].shape and st[name].dtype == want[name].dtype, name
        np.testing.assert_array_equal(st[name], want[name], err_msg=name)
    (ch,) = r["result"].channels
    frames, counts = A.nxdn.parse_frames(st["rows"], st["bits"], st["levels"], st["info"], st["rec"], FS)
    assert [f.to_json() for f in frames] == want["frames"] and counts == want["counts"]
    assert [c.to_json() for c in ch.calls] == want["calls"] and [c.to_json() for c in ch.control] == want["control"]
    assert ch.frames == want["kinds"] and ch.rate == rate and st["rate"] == rate
    assert {k: getattr(ch, k) for k in CLEAN} == want["counts"]
    assert r["result"].lines() == ["+0 Hz: " + NM.call_line(c) for c in want["calls"]] + ["+0 Hz: " + NM.control_line(c) for c in want["control"]]
    assert A.NxdnResult.from_json(json.loads(json.dumps(r["result"].to_json()))) == r["result"]


@pytest.mark.parametrize("case", ["clean", "noise", "negated"])
def test_decoder_equals_the_model(A, runs, case):
    r = runs[case]
    want = r["want"]
    # the model's expectation first: every frame of the script, one call with every field
    assert len(want["rows"]) == 11 and set(want["rows"][:, 1].tolist()) == ({-1} if case == "negated" else {1})
    assert want["classes"].tolist() == NM.CLASSES and want["kinds"] == NM.KINDS
    (call,) = want["calls"]
    assert NM.call_line(call) == NM.LINE and (call["late"], call["released"], call["conflicts"]) == (False, True, 0) and want["control"] == []
    changed = int(want["rec"][:, 1:].sum())
    print(case, "channel bits changed", changed, "fixed", want["counts"]["fixed"], "lich_inner", want["counts"]["lich_inner"])
    if case == "noise":
        assert changed > 0 and want["counts"] == dict(CLEAN, fixed=want["counts"]["fixed"], lich_inner=want["counts"]["lich_inner"])
    else:
        assert changed == 0 and want["counts"] == CLEAN  # all counters zero
    _equals_the_model(A, r, 4800)
    assert r["result"].channels[0].inverted == (case == "negated")


def test_the_negated_stream_gives_the_same_frames(runs):
    clean, neg = runs["clean"], runs["negated"]
    np.testing.assert_array_equal(neg["st"]["v"], -clean["st"]["v"])  # (no shift at this rate)
    assert neg["st"]["rows"][:, 0].tolist() == clean["st"]["rows"][:, 0].tolist() and set(neg["st"]["rows"][:, 1].tolist()) == {-1}
    for name in STAGES[1:]:
        flip = np.array([1, -1, 1]) if name == "levels" else 1  # (the DC of a negated plane is the DC negated)
        np.testing.assert_array_equal(neg["st"][name] * flip, clean["st"][name], err_msg=name)
    a, b = clean["result"].channels[0], neg["result"].channels[0]
    assert (a.calls, a.frames) == (b.calls, b.frames) and (a.inverted, b.inverted) == (False, True)


def test_the_same_stream_at_2400_symbols(A, runs):
    r, clean = runs["rate2400"], runs["clean"]
    want = r["want"]
    assert len(want["rows"]) == 11 and want["classes"].tolist() == NM.CLASSES and want["counts"] == CLEAN
    (call,) = want["calls"]
    assert NM.call_line(call) == NM.LINE.replace("0.40 s", "0.80 s") and (call["late"], call["released"], call["conflicts"]) == (False, True, 0)
    _equals_the_model(A, r, 2400)
    # the same frames as at 4800 symbols/s: every bit behind the slicer, and every frame less its time
    for name in ("bits", "classes", "info", "rec"):
        np.testing.assert_array_equal(r["st"][name], clean["st"][name], err_msg=name)
    strip = lambda frames: [dict(f, time_s=0) for f in frames]  # noqa: E731
    assert strip(want["frames"]) == strip(clean["want"]["frames"])


def test_uneven_cuts_give_identical_output(A, runs):
    r = runs["noise"]
    dec = A.NxdnDecoder(FS)
    at = 0
    for n in (1, 2047, 2049, 1 << 30):
        dec.process(r["theta"][at : at + n])
        at += n
    assert dec.finish() == r["result"]
    st = dec.stages()
    for name in ("v", "hits") + STAGES:
        np.testing.assert_array_equal(st[name], r["st"][name], err_msg=name)
    dec.reset()
    assert dec.finish().channels[0].calls == [] and dec.stages()["rows"].shape == (0, 2)


def test_the_control_stream_gives_its_folded_lines(A, runs):
    r = runs["control"]
    want = r["want"]
    assert want["classes"].tolist() == [8] * 6 and want["counts"] == CLEAN and want["calls"] == [] and want["kinds"] == {"RCCH outbound": 6}
    assert [NM.control_line(c) for c in want["control"]] == NM.CONTROL_LINES
    assert [(c["name"], c["count"]) for c in want["control"]] == [("SITE_INFO", 2), ("SRV_INFO", 1), ("IDLE", 3)]
    _equals_the_model(A, r, 4800)
    assert r["result"].lines() == ["+0 Hz: " + line for line in NM.CONTROL_LINES]


def test_cli_lines_and_files(A, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import _native, cli, iqio

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith(("iqa_nxdn_", "iqa_ysf_", "iqa_p25_", "iqa_dmr_", "iqa_flex_", "iqa_ident_")):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    raw = NM.capture()
    stem = f"model_{int(FC)}Hz"
    dirs = {}
    for tag in ("identify", "nxdn"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
        iqio.write_wav_iq(dirs[tag] / f"{stem}.wav", raw, int(NM.FS), "s16")
    # a --find-identify run calls no entry point of this section
    assert cli.main(["--in", str(dirs["identify"] / f"{stem}.wav"), "--find-identify"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert sorted(calls) == ["iqa_ident_integrate", "iqa_ident_search"] and not list(dirs["identify"].glob("*.nxdn.json"))
    assert len(plain) == 4 * len(NM.CAPTURE_CHANNELS) and plain[2].startswith("    keying: fsk 4800")
    assert plain[3].startswith("    protocol: nxdn (") and "on the 40 ms grid" in plain[3]
    # --find-nxdn: the same lines, the calls behind them, the same four JSON files, and nxdn.json
    calls.clear()
    assert cli.main(["--in", str(dirs["nxdn"] / f"{stem}.wav"), "--find-nxdn"]) == 0
    printed = capsys.readouterr().out.splitlines()
    assert sorted(calls) == ["iqa_ident_integrate", "iqa_ident_search", "iqa_nxdn_decode", "iqa_nxdn_slice"]
    assert printed[: len(plain)] == plain
    got = printed[len(plain) :]
    # (tests/test_nxdn_host.py holds the model to these: the call of the test stream with its release, then a second one until
    # the capture ends)
    want = [NM.LINE, "NXDN RAN 5 4321 -> 8765 individual cipher 1 1.48 s (38 frames)"]
    assert len(got) == len(want) and all(line.endswith(": " + w) for line, w in zip(got, want)), got
    freq = int(round(FC + 200e3))
    assert all(abs(int(line.split(" Hz: ")[0]) - freq) <= 1000 for line in got)
    for name in (f"{stem}.channels.json", f"{stem}.describe.json", f"{stem}.keying.json", f"{stem}.protocols.json"):
        assert (dirs["nxdn"] / name).read_bytes() == (dirs["identify"] / name).read_bytes(), name
    assert not any(list(dirs["nxdn"].glob(f"*.{x}.json")) for x in ("flex", "dmr", "p25", "ysf"))
    stored = A.NxdnResult.from_json(json.loads((dirs["nxdn"] / f"{stem}.nxdn.json").read_text()))
    assert stored.lines() == got and [ch.note for ch in stored.channels] == ["", "no nxdn channel"] and stored.center_freq == FC
    ch = stored.channels[0]
    assert ch.rate == 4800 and ch.inverted is False and ch.frames["RTCH superframe"] >= 44 and ch.frames["RTCH non-superframe"] == 4
    assert (ch.sacch_failed, ch.facch_failed, ch.cac_failed, ch.no_level, ch.udch) == (0, 0, 0, 0, 0)
    assert [(c.late, c.released, c.conflicts, c.ran, c.key) for c in ch.calls] == [(False, True, 0, 5, 0), (False, False, 0, 5, 9)]
    assert abs(ch.calls[0].start_s - (192 + 1) / 4800.0) < 2e-3
    # the two newest branches of the table at once, in table order; neither entry point of this section without the layer
    calls.clear()
    six = A.find_channels(dirs["nxdn"] / f"{stem}.wav", describe=True, keying=True, identify=True, nxdn=True, ysf=True)
    assert len(six) == 6 and [type(x).__name__ for x in six[4:]] == ["YsfResult", "NxdnResult"] and six[5] == stored
    assert [c.note for c in six[4].channels] == ["", "no ysf channel"] and six[4].channels[0].transmissions == []
    calls.clear()
    five = A.find_channels(dirs["nxdn"] / f"{stem}.wav", describe=True, keying=True, identify=True, ysf=True)
    assert len(five) == 5 and five[4] == six[4] and "iqa_ysf_slice" in calls and not [c for c in calls if c.startswith("iqa_nxdn_")]
