"""The YSF frame decoding (--find-ysf) on the MI355X: ``YsfDecoder`` on the synthesised test stream at
160 000 Hz (a header, V/D mode 2 frames 0 .. 7, a V/D mode 1 frame, a data FR frame, a voice FR frame and the terminator: 13
frames, 1.3 s), clean, at the noise level that tests/test_ysf_host.py finds and negated: the plane, the hits, the bits, the
levels, the FICHs, the classes, the information words, the records, the frames and the transmissions equal the model's of
tests/ysf_model.py, applied to the GPU's own integrator plane; a stream cut unevenly gives identical output; the CLI on a model
capture with a YSF channel: --find-ysf prints the transmissions and writes ysf.json, a --find-identify run calls no entry point
of this section and writes the same four JSON files, and flex, dmr, p25 and ysf together return all four results.  Every
comparison is of integers and exact."""
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


YM = _load("ysf_model")
IM = YM.IM
FS = 160_000.0
FC = 433.0e6
NOISE = 0.12  # test_ysf_host.py's: the largest at which the model alone still decodes every frame of this stream
CASES = ["clean", "noise", "negated"]
CLEAN = dict(no_level=0, cut=0, fich_failed=0, golay_refused=0, dch_failed=0, fixed=0)
KINDS = {"header": 1, "V/D2": 8, "V/D1": 1, "data FR": 1, "voice FR": 1, "terminator": 1}
STAGES = ("rows", "bits", "levels", "fich", "frec", "classes", "info", "rec")


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


@pytest.fixture(scope="module")
def runs(A):
    """Every case through ``YsfDecoder`` once, and the model on the GPU's own plane."""
    out = {}
    for case in CASES:
        theta = YM.test_stream(FS, noise=NOISE if case == "noise" else 0.0, negate=case == "negated")
        dec = A.YsfDecoder(FS)
        dec.process(theta)
        result = dec.finish()
        st = dec.stages()
        pl = YM.plan(FS)
        _, kept = IM.search(st["v"], pl["ident"], YM.YSF_PATTERNS)
        out[case] = dict(theta=theta, result=result, st=st, plan=pl, kept=kept, want=YM.decode_plane(st["v"], kept, pl))
    return out


@pytest.mark.parametrize("case", CASES)
def test_decoder_equals_the_model(A, runs, case):
    r = runs[case]
    st, want, pl = r["st"], r["want"], r["plan"]
    # the model's expectation first: every frame of the script, one transmission with every callsign
    assert len(want["rows"]) == 13 and set(want["rows"][:, 1].tolist()) == ({-1} if case == "negated" else {1})
    assert want["classes"].tolist() == [1] + [3] * 8 + [2, 1, 0, 1]
    (tx,) = want["txs"]
    assert YM.tx_line(tx) == YM.LINE and (tx["late"], tx["terminated"], tx["conflicts"]) == (False, True, 0)
    changed = int(want["frec"][:, 1].sum()) + int(want["rec"][:, 1:3].sum())
    print(case, "fich bits", int(want["frec"][:, 1].sum()), "golay refused", want["counts"]["golay_refused"], "dch bits", int(want["rec"][:, 1:3].sum()),
          "fixed", want["counts"]["fixed"])
    if case == "noise":
        assert changed > 0 and want["counts"] == dict(CLEAN, fixed=want["counts"]["fixed"], golay_refused=want["counts"]["golay_refused"])
    else:
        assert changed == 0 and want["counts"] == CLEAN  # all counters zero
    # the plane and the hits are section 25's
    np.testing.assert_array_equal(st["v"], IM.integrate(r["theta"], 0, pl["ident"]["L"], pl["ident"]["sh"]))
    assert st["hits"].tolist() == [list(h) for h in r["kept"]]
    # all three entries, value for value
    for name in STAGES:
        assert st[name].shape == want[name].shape and st[name].dtype == want[name].dtype, name
        np.testing.assert_array_equal(st[name], want[name], err_msg=name)
    # the frames and the transmissions
    (ch,) = r["result"].channels
    frames, counts = A.ysf.parse_frames(st["rows"], st["levels"], st["fich"], st["frec"], st["info"], st["rec"], FS)
    assert [f.to_json() for f in frames] == want["frames"] and counts == want["counts"]
    assert [t.to_json() for t in ch.transmissions] == want["txs"]
    assert ch.frames == KINDS and ch.inverted == (case == "negated")
    assert {k: getattr(ch, k) for k in CLEAN} == want["counts"]
    assert r["result"].lines() == ["+0 Hz: " + YM.LINE]
    assert A.YsfResult.from_json(json.loads(json.dumps(r["result"].to_json()))) == r["result"]


def test_the_negated_stream_gives_the_same_frames(runs):
    clean, neg = runs["clean"], runs["negated"]
    np.testing.assert_array_equal(neg["st"]["v"], -clean["st"]["v"])  # (no shift at this rate)
    assert neg["st"]["rows"][:, 0].tolist() == clean["st"]["rows"][:, 0].tolist() and set(neg["st"]["rows"][:, 1].tolist()) == {-1}
    for name in STAGES[1:]:
        flip = np.array([1, -1, 1]) if name == "levels" else 1  # (the DC of a negated plane is the DC negated)
        np.testing.assert_array_equal(neg["st"][name] * flip, clean["st"][name], err_msg=name)
    a, b = clean["result"].channels[0], neg["result"].channels[0]
    assert (a.transmissions, a.frames) == (b.transmissions, b.frames) and (a.inverted, b.inverted) == (False, True)


def test_uneven_cuts_give_identical_output(A, runs):
    r = runs["noise"]
    dec = A.YsfDecoder(FS)
    at = 0
    for n in (1, 2047, 2049, 1 << 30):
        dec.process(r["theta"][at : at + n])
        at += n
    assert dec.finish() == r["result"]
    st = dec.stages()
    for name in ("v", "hits") + STAGES:
        np.testing.assert_array_equal(st[name], r["st"][name], err_msg=name)
    dec.reset()
    assert dec.finish().channels[0].transmissions == [] and dec.stages()["rows"].shape == (0, 2)


def test_cli_lines_and_files(A, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import _native, cli, iqio

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith(("iqa_ysf_", "iqa_p25_", "iqa_dmr_", "iqa_flex_", "iqa_ident_")):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    raw = YM.capture()
    stem = f"model_{int(FC)}Hz"
    dirs = {}
    for tag in ("identify", "ysf"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
        iqio.write_wav_iq(dirs[tag] / f"{stem}.wav", raw, int(YM.FS), "s16")
    # a --find-identify run calls no entry point of this section
    assert cli.main(["--in", str(dirs["identify"] / f"{stem}.wav"), "--find-identify"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert sorted(calls) == ["iqa_ident_integrate", "iqa_ident_search"] and not list(dirs["identify"].glob("*.ysf.json"))
    assert len(plain) == 4 * len(YM.CAPTURE_CHANNELS) and plain[2].startswith("    keying: fsk 4800")
    assert plain[3].startswith("    protocol: ysf (") and "18 pairs on the 100 ms grid" in plain[3]
    # --find-ysf: the same lines, the transmissions behind them, the same four JSON files, and ysf.json
    calls.clear()
    assert cli.main(["--in", str(dirs["ysf"] / f"{stem}.wav"), "--find-ysf"]) == 0
    printed = capsys.readouterr().out.splitlines()
    assert sorted(calls) == ["iqa_ident_integrate", "iqa_ident_search", "iqa_ysf_decode", "iqa_ysf_fich", "iqa_ysf_slice"]
    assert printed[: len(plain)] == plain
    got = printed[len(plain) :]
    # (tests/test_ysf_host.py holds the model to these: ten frames with their terminator, then nine until the capture ends, the
    # last of them cut behind its FICH)
    want = ["YSF JA1YOE -> ALL via JP1YJQ/JP1YJQ-1 group V/D2 sq=42 0.90 s (10 frames)",
            "YSF JA1YOE -> ALL via JP1YJQ/JP1YJQ-1 group V/D2 sq=42 0.80 s (9 frames)"]
    assert len(got) == len(want) and all(line.endswith(": " + w) for line, w in zip(got, want)), got
    freq = int(round(FC + 200e3))
    assert all(abs(int(line.split(" Hz: ")[0]) - freq) <= 1000 for line in got)
    for name in (f"{stem}.channels.json", f"{stem}.describe.json", f"{stem}.keying.json", f"{stem}.protocols.json"):
        assert (dirs["ysf"] / name).read_bytes() == (dirs["identify"] / name).read_bytes(), name
    assert not any(list(dirs["ysf"].glob(f"*.{x}.json")) for x in ("flex", "dmr", "p25"))
    stored = A.YsfResult.from_json(json.loads((dirs["ysf"] / f"{stem}.ysf.json").read_text()))
    assert stored.lines() == got and [ch.note for ch in stored.channels] == ["", "no ysf channel"] and stored.center_freq == FC
    ch = stored.channels[0]
    assert ch.frames == {"header": 2, "V/D2": 16, "terminator": 1} and ch.inverted is False
    assert {k: getattr(ch, k) for k in CLEAN} == dict(CLEAN, cut=1, fixed=ch.fixed)
    assert [(t.late, t.terminated, t.conflicts, t.rem12, t.rem34) for t in ch.transmissions] == [
        (False, True, 0, YM.REM12, YM.REM34), (False, False, 0, YM.REM12, YM.REM34)]
    assert abs(ch.transmissions[0].start_s - (480 + 1) / 4800.0) < 2e-3
    # every branch of the table at once, in table order
    eight = A.find_channels(dirs["ysf"] / f"{stem}.wav", describe=True, keying=True, identify=True, flex=True, dmr=True, p25=True, ysf=True)
    assert len(eight) == 8 and eight[7] == stored
    assert [type(x).__name__ for x in eight[4:]] == ["FlexResult", "DmrResult", "P25Result", "YsfResult"]
    assert [c.note for c in eight[4].channels] == ["no flex channel"] * 2 and eight[6].channels[0].calls == []
    five = A.find_channels(dirs["ysf"] / f"{stem}.wav", describe=True, keying=True, identify=True, ysf=True)
    assert len(five) == 5 and five[4] == stored


def test_no_ysf_call_with_the_layer_off(A, tmp_path, monkeypatch):
    from iq_to_audio_amd import _native, iqio

    calls = []
    real = _native.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    path = tmp_path / "model.wav"
    iqio.write_wav_iq(path, YM.capture(), int(YM.FS), "s16")
    out = A.find_channels(path, describe=True, keying=True, identify=True, p25=True)
    assert len(out) == 5 and "iqa_ident_search" in calls and "iqa_p25_slice" in calls and not [c for c in calls if c.startswith("iqa_ysf_")]
