"""The DMR burst decoding (--find-dmr) on the MI355X: ``DmrDecoder`` on the synthesised test stream at
160 000 Hz, clean and at the noise level that tests/test_dmr_host.py finds: the bits, the levels, the information words, the
records, the bursts and the calls equal the numpy oracle's of tests/dmr_model.py, applied to the GPU's own integrator plane; a
stream cut unevenly gives identical output; the CLI on a model capture with a DMR base channel: --find-dmr prints the call and
the CSBK and writes dmr.json, a --find-identify run calls no entry point of this section and writes the same four JSON files,
and --find-flex --find-dmr returns both results.  Every comparison is of integers and exact."""
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


DM = _load("dmr_model")
IM = DM.IM
FS = 160_000.0
FC = 439.3125e6
NOISE = 0.06  # test_dmr_host.py's: the largest at which the oracle alone still decodes every burst
CASES = [0.0, NOISE]


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


@pytest.fixture(scope="module")
def runs(A):
    """Every case through ``DmrDecoder`` once, and the oracle on the GPU's own plane."""
    out = {}
    for noise in CASES:
        theta = DM.test_stream(FS, noise=noise)
        dec = A.DmrDecoder(FS)
        dec.process(theta)
        result = dec.finish()
        st = dec.stages()
        pl = DM.plan(FS)
        _, kept = IM.search(st["v"], pl["ident"], DM.DMR_PATTERNS)
        out[noise] = dict(theta=theta, result=result, st=st, plan=pl, kept=kept, want=DM.decode_plane(st["v"], kept, pl))
    return out


@pytest.mark.parametrize("noise", CASES)
def test_decoder_equals_the_oracle(A, runs, noise):
    r = runs[noise]
    st, want, pl = r["st"], r["want"], r["plan"]
    # the oracle's expectation first: every burst of the script, one call, the CSBK
    assert len(want["rows"]) == 31 and want["rows"][:, 2].tolist().count(0) == 3 and want["rows"][:, 2].tolist().count(1) == 28
    assert want["counts"] == dict(no_level=0, cut=0, slot_refused=0, bptc_failed=0, check_failed=0, idle=24, tact_fixed=want["counts"]["tact_fixed"])
    (call,) = want["calls"]
    assert (call["slot"], call["cc"], call["group"], call["src"], call["dst"], call["superframes"], call["terminated"]) == (1, 1, True, DM.SRC, DM.DST, 3, True)
    assert [(b["data_type"], b["slot"], b["checked"]) for b in want["bursts"] if b["data_type"] not in (None, 9)] == [
        (1, 1, True), (1, 1, True), (3, 2, True), (2, 1, True)]
    flips = int(want["rec"][:, 6].sum())
    print("noise", noise, "flips", flips, "slot-type distance", int(want["rec"][:, 3].sum()), "tact fixed", want["counts"]["tact_fixed"])
    assert (flips > 0) == (noise > 0)
    # the plane and the hits are section 25's
    np.testing.assert_array_equal(st["v"], IM.integrate(r["theta"], 0, pl["ident"]["L"], pl["ident"]["sh"]))
    assert st["hits"].tolist() == [list(h) for h in r["kept"]]
    # both entries, value for value
    for name in ("rows", "bits", "levels", "info", "rec"):
        assert st[name].shape == want[name].shape and st[name].dtype == want[name].dtype, name
        np.testing.assert_array_equal(st[name], want[name], err_msg=name)
    # the bursts and the calls
    (ch,) = r["result"].channels
    bursts, counts = A.dmr.parse_bursts(st["rows"], st["levels"], st["info"], st["rec"], FS)
    assert [b.to_json() for b in bursts] == want["bursts"] and counts == want["counts"]
    assert [c.to_json() for c in ch.calls] == want["calls"]
    assert [b.to_json() for b in ch.bursts] == [b for b in want["bursts"] if b["data_type"] not in (None, 9)]
    assert ch.kinds == {"bs data": 28, "bs voice": 3} and (ch.idle, ch.cut, ch.no_level, ch.bptc_failed) == (24, 0, 0, 0)
    assert r["result"].lines() == ["+0 Hz: DMR cc=1 ts=1 group 2345678 -> 9 1.20 s (3 superframes)",
                                   "+0 Hz: DMR cc=1 ts=2 csbk o=0x3d fid=0x00 0123456789abcdef"]
    assert A.DmrResult.from_json(json.loads(json.dumps(r["result"].to_json()))) == r["result"]


def test_uneven_cuts_give_identical_output(A, runs):
    r = runs[NOISE]
    dec = A.DmrDecoder(FS)
    at = 0
    for n in (1, 2047, 2049, 1 << 30):
        dec.process(r["theta"][at : at + n])
        at += n
    assert dec.finish() == r["result"]
    st = dec.stages()
    for name in ("v", "hits", "rows", "bits", "levels", "info", "rec"):
        np.testing.assert_array_equal(st[name], r["st"][name], err_msg=name)
    dec.reset()
    assert dec.finish().channels[0].calls == [] and dec.stages()["rows"].shape == (0, 3)


def test_cli_lines_and_files(A, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import _native, cli, iqio

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith(("iqa_dmr_", "iqa_flex_", "iqa_ident_")):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    raw = DM.capture()
    stem = f"model_{int(FC)}Hz"
    dirs = {}
    for tag in ("identify", "dmr"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
        iqio.write_wav_iq(dirs[tag] / f"{stem}.wav", raw, int(DM.FS), "s16")
    # a --find-identify run calls no entry point of this section
    assert cli.main(["--in", str(dirs["identify"] / f"{stem}.wav"), "--find-identify"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert sorted(calls) == ["iqa_ident_integrate", "iqa_ident_search"] and not list(dirs["identify"].glob("*.dmr.json"))
    assert len(plain) == 4 * len(DM.CAPTURE_CHANNELS) and plain[2].startswith("    keying: fsk 4800")
    assert plain[3].startswith("    protocol: dmr (bs data 47, bs voice 3; 49 pairs on the 30 ms grid)")
    # --find-dmr: the same lines, the call and the CSBK behind them, the same four JSON files, and dmr.json
    calls.clear()
    assert cli.main(["--in", str(dirs["dmr"] / f"{stem}.wav"), "--find-dmr"]) == 0
    printed = capsys.readouterr().out.splitlines()
    assert sorted(calls) == ["iqa_dmr_decode", "iqa_dmr_slice", "iqa_ident_integrate", "iqa_ident_search"]
    assert printed[: len(plain)] == plain
    got = printed[len(plain) :]
    want = ["DMR cc=1 ts=1 group 2345678 -> 9 1.20 s (3 superframes)", "DMR cc=1 ts=2 csbk o=0x3d fid=0x00 0123456789abcdef"]
    assert len(got) == 2 and all(line.endswith(": " + w) for line, w in zip(got, want)), got
    freq = int(round(FC + 200e3))
    assert all(abs(int(line.split(" Hz: ")[0]) - freq) <= 1000 for line in got)
    for name in (f"{stem}.channels.json", f"{stem}.describe.json", f"{stem}.keying.json", f"{stem}.protocols.json"):
        assert (dirs["dmr"] / name).read_bytes() == (dirs["identify"] / name).read_bytes(), name
    assert not list(dirs["dmr"].glob("*.flex.json"))
    stored = A.DmrResult.from_json(json.loads((dirs["dmr"] / f"{stem}.dmr.json").read_text()))
    assert stored.lines() == got and [ch.note for ch in stored.channels] == ["", "no dmr channel"] and stored.center_freq == FC
    ch = stored.channels[0]
    assert ch.kinds == {"bs data": 47, "bs voice": 3} and (ch.cut, ch.idle, ch.no_level, ch.slot_refused, ch.bptc_failed, ch.check_failed) == (1, 42, 0, 0, 0, 0)
    assert abs(ch.calls[0].start_s - (DM.CAPTURE_START + (2 * 144 + 66 + 1) / 4800.0)) < 2e-3
    # both branches of the table at once
    six = A.find_channels(dirs["dmr"] / f"{stem}.wav", describe=True, keying=True, identify=True, flex=True, dmr=True)
    assert len(six) == 6 and six[5] == stored and type(six[4]).__name__ == "FlexResult" and [c.note for c in six[4].channels] == ["no flex channel"] * 2
    five = A.find_channels(dirs["dmr"] / f"{stem}.wav", describe=True, keying=True, identify=True, dmr=True)
    assert len(five) == 5 and five[4] == stored
    assert len(A.find_channels(dirs["dmr"] / f"{stem}.wav", describe=True, keying=True, identify=True)) == 4
