"""The P25 phase 1 frame decoding (--find-p25) on the MI355X: ``P25Decoder`` on the synthesised test stream
at 160 000 Hz, clean, at the noise level that tests/test_p25_host.py finds and negated: the plane, the hits, the bits, the
levels, the NIDs, the information words, the records, the frames, the calls and the TSBKs equal the numpy oracle's of
tests/p25_model.py, applied to the GPU's own integrator plane; a stream cut unevenly gives identical output; the CLI on a model
capture with a P25 channel: --find-p25 prints the call and the distinct TSBKs and writes p25.json, a --find-identify run calls
no entry point of this section and writes the same four JSON files, and flex, dmr and p25 together return all three results.
Every comparison is of integers and exact."""
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


PM = _load("p25_model")
IM = PM.IM
FS = 160_000.0
FC = 850.8125e6
NOISE = 0.05  # test_p25_host.py's: the largest at which the oracle alone still decodes every frame
CASES = ["clean", "noise", "negated"]
CLEAN = dict(no_level=0, cut=0, nid_refused=0, nid_fixed=0, lc_failed=0, crc_failed=0, golay_refused=0, hamming_unmatched=0)
TSBK_LINES = ["identifier update id 1 base 849.7625 MHz spacing 12.5 kHz", "network status wacn 0xbee00 system 0x293 ch 0x1001 (849.7750 MHz)",
              "rfss status system 0x293 rfss 1 site 2 ch 0x1001 (849.7750 MHz)", "group grant tg 9 src 2345678 ch 0x1064 (851.0125 MHz)",
              "o=0x29 mfid=0x90 0123456789abcdef"]


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


@pytest.fixture(scope="module")
def runs(A):
    """Every case through ``P25Decoder`` once, and the oracle on the GPU's own plane."""
    out = {}
    for case in CASES:
        theta = PM.test_stream(FS, noise=NOISE if case == "noise" else 0.0, negate=case == "negated")
        dec = A.P25Decoder(FS)
        dec.process(theta)
        result = dec.finish()
        st = dec.stages()
        pl = PM.plan(FS)
        _, kept = IM.search(st["v"], pl["ident"], PM.P25_PATTERNS)
        out[case] = dict(theta=theta, result=result, st=st, plan=pl, kept=kept, want=PM.decode_plane(st["v"], kept, pl))
    return out


@pytest.mark.parametrize("case", CASES)
def test_decoder_equals_the_oracle(A, runs, case):
    r = runs[case]
    st, want, pl = r["st"], r["want"], r["plan"]
    # the oracle's expectation first: every frame of the script, one call, the five distinct blocks
    assert len(want["rows"]) == 12 and set(want["rows"][:, 1].tolist()) == ({-1} if case == "negated" else {1})
    assert want["counts"] == dict(CLEAN, nid_fixed=want["counts"]["nid_fixed"])
    assert [f["name"] for f in want["frames"]] == ["hdu", "ldu1", "ldu2", "ldu1", "ldu2", "tdulc"] + ["tsbk"] * 6
    (call,) = want["calls"]
    assert (call["nac"], call["group"], call["src"], call["dst"], call["ldus"], call["terminated"]) == (PM.NAC, True, PM.SRC, PM.TG, 4, True)
    assert [(t["text"], t["count"]) for t in want["tsbks"]] == list(zip(TSBK_LINES, (1, 3, 3, 3, 2)))
    changed = int(want["nid"][:, 1].sum()) + int(want["rec"][:6, 1].sum())
    print(case, "nid bits", int(want["nid"][:, 1].sum()), "nid fixed", want["counts"]["nid_fixed"], "words corrected", int(want["rec"][:6, 1].sum()))
    assert (changed > 0) == (case == "noise")
    # the plane and the hits are section 25's
    np.testing.assert_array_equal(st["v"], IM.integrate(r["theta"], 0, pl["ident"]["L"], pl["ident"]["sh"]))
    assert st["hits"].tolist() == [list(h) for h in r["kept"]]
    # all three entries, value for value
    for name in ("rows", "bits", "levels", "nid", "info", "rec"):
        assert st[name].shape == want[name].shape and st[name].dtype == want[name].dtype, name
        np.testing.assert_array_equal(st[name], want[name], err_msg=name)
    # the frames, the calls and the blocks
    (ch,) = r["result"].channels
    frames, counts = A.p25.parse_frames(st["rows"], st["levels"], st["nid"], st["info"], st["rec"], FS)
    assert [f.to_json() for f in frames] == want["frames"] and counts == want["counts"]
    assert [c.to_json() for c in ch.calls] == want["calls"] and [t.to_json() for t in ch.tsbks] == want["tsbks"]
    assert ch.nacs == {"0x293": 12} and ch.frames == {"hdu": 1, "ldu1": 2, "ldu2": 2, "tdulc": 1, "tsbk": 6}
    assert (ch.cut, ch.no_level, ch.nid_refused, ch.lc_failed, ch.crc_failed, ch.inverted) == (0, 0, 0, 0, 0, case == "negated")
    assert r["result"].lines() == ["+0 Hz: P25 nac=0x293 group 2345678 -> 9 0.80 s (4 ldus)"] + [
        f"+0 Hz: P25 nac=0x293 tsbk {text} x{n}" for text, n in zip(TSBK_LINES, (1, 3, 3, 3, 2))]
    assert A.P25Result.from_json(json.loads(json.dumps(r["result"].to_json()))) == r["result"]


def test_the_negated_stream_gives_the_same_frames(runs):
    clean, neg = runs["clean"], runs["negated"]
    np.testing.assert_array_equal(neg["st"]["v"], -clean["st"]["v"])  # (no shift at this rate)
    assert neg["st"]["rows"][:, 0].tolist() == clean["st"]["rows"][:, 0].tolist() and set(neg["st"]["rows"][:, 1].tolist()) == {-1}
    for name in ("bits", "nid", "info", "rec"):
        np.testing.assert_array_equal(neg["st"][name], clean["st"][name], err_msg=name)
    a, b = clean["result"].channels[0], neg["result"].channels[0]
    assert (a.calls, a.tsbks, a.nacs, a.frames) == (b.calls, b.tsbks, b.nacs, b.frames) and (a.inverted, b.inverted) == (False, True)


def test_uneven_cuts_give_identical_output(A, runs):
    r = runs["noise"]
    dec = A.P25Decoder(FS)
    at = 0
    for n in (1, 2047, 2049, 1 << 30):
        dec.process(r["theta"][at : at + n])
        at += n
    assert dec.finish() == r["result"]
    st = dec.stages()
    for name in ("v", "hits", "rows", "bits", "levels", "nid", "info", "rec"):
        np.testing.assert_array_equal(st[name], r["st"][name], err_msg=name)
    dec.reset()
    assert dec.finish().channels[0].calls == [] and dec.stages()["rows"].shape == (0, 2)


def test_cli_lines_and_files(A, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import _native, cli, iqio

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith(("iqa_p25_", "iqa_dmr_", "iqa_flex_", "iqa_ident_")):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    raw = PM.capture()
    stem = f"model_{int(FC)}Hz"
    dirs = {}
    for tag in ("identify", "p25"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
        iqio.write_wav_iq(dirs[tag] / f"{stem}.wav", raw, int(PM.FS), "s16")
    # a --find-identify run calls no entry point of this section
    assert cli.main(["--in", str(dirs["identify"] / f"{stem}.wav"), "--find-identify"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert sorted(calls) == ["iqa_ident_integrate", "iqa_ident_search"] and not list(dirs["identify"].glob("*.p25.json"))
    assert len(plain) == 4 * len(PM.CAPTURE_CHANNELS) and plain[2].startswith("    keying: fsk 4800")
    assert plain[3].startswith("    protocol: p25 (") and "22 pairs on the 7.5 ms grid" in plain[3]
    # --find-p25: the same lines, the call and the blocks behind them, the same four JSON files, and p25.json
    calls.clear()
    assert cli.main(["--in", str(dirs["p25"] / f"{stem}.wav"), "--find-p25"]) == 0
    printed = capsys.readouterr().out.splitlines()
    assert sorted(calls) == ["iqa_ident_integrate", "iqa_ident_search", "iqa_p25_decode", "iqa_p25_nid", "iqa_p25_slice"]
    assert printed[: len(plain)] == plain
    got = printed[len(plain) :]
    # (tests/test_p25_host.py holds the oracle to these: the capture opens with the control channel's frame, the last one is cut)
    want = [f"P25 nac=0x293 tsbk {TSBK_LINES[1]} x14", f"P25 nac=0x293 tsbk {TSBK_LINES[2]} x14", f"P25 nac=0x293 tsbk {TSBK_LINES[3]} x13",
            "P25 nac=0x293 group 2345678 -> 9 0.80 s (4 ldus)", f"P25 nac=0x293 tsbk {TSBK_LINES[0]} x1", f"P25 nac=0x293 tsbk {TSBK_LINES[4]} x2"]
    assert len(got) == len(want) and all(line.endswith(": " + w) for line, w in zip(got, want)), got
    freq = int(round(FC + 200e3))
    assert all(abs(int(line.split(" Hz: ")[0]) - freq) <= 1000 for line in got)
    for name in (f"{stem}.channels.json", f"{stem}.describe.json", f"{stem}.keying.json", f"{stem}.protocols.json"):
        assert (dirs["p25"] / name).read_bytes() == (dirs["identify"] / name).read_bytes(), name
    assert not list(dirs["p25"].glob("*.flex.json")) and not list(dirs["p25"].glob("*.dmr.json"))
    stored = A.P25Result.from_json(json.loads((dirs["p25"] / f"{stem}.p25.json").read_text()))
    assert stored.lines() == got and [ch.note for ch in stored.channels] == ["", "no p25 channel"] and stored.center_freq == FC
    ch = stored.channels[0]
    assert ch.nacs == {"0x293": 23} and ch.frames == {"hdu": 1, "ldu1": 2, "ldu2": 2, "tdulc": 1, "tsbk": 17} and ch.inverted is False
    assert (ch.cut, ch.no_level, ch.nid_refused, ch.lc_failed, ch.crc_failed) == (1, 0, 0, 0, 0)
    assert abs(ch.calls[0].start_s - (360 + 1) / 4800.0) < 2e-3
    # every branch of the table at once, in table order
    seven = A.find_channels(dirs["p25"] / f"{stem}.wav", describe=True, keying=True, identify=True, flex=True, dmr=True, p25=True)
    assert len(seven) == 7 and seven[6] == stored and [type(x).__name__ for x in seven[4:]] == ["FlexResult", "DmrResult", "P25Result"]
    assert [c.note for c in seven[4].channels] == ["no flex channel"] * 2 and seven[5].channels[0].calls == []
    five = A.find_channels(dirs["p25"] / f"{stem}.wav", describe=True, keying=True, identify=True, p25=True)
    assert len(five) == 5 and five[4] == stored
