"""The FLEX page decoding (--find-flex) on the MI355X: ``FlexDecoder`` on synthesised frames of every mode
at 25 600 Hz (sps 16): the frame records, every word, raw and status array, the chosen shifts and the pages equal the numpy
oracle's of tests/flex_model.py, applied to the GPU's own integrator planes; a stream cut unevenly gives identical output; the
CLI on a model capture with a FLEX channel carrying a real frame: --find-flex prints the pages and writes flex.json, a
--find-identify run calls no entry point of this section and writes the same four JSON files."""
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


FM = _load("flex_model")
IM = FM.IM
FS = 25_600.0
FC = 455.5e6
NOISE = 0.4  # test_flex_host.py's: the oracle alone still decodes every page
CLI_MODE = "3200/2"  # section 23 labels it fsk 3200 on the model capture (DESIGN.md section 26 lists all four)
PAGES = {"A": [dict(kind="alpha", capcode=1234567, text="HELLO FLEX"), dict(kind="numeric", capcode=4242, text="555-0199 U[3]")],
         "B": [dict(kind="tone", capcode=77), dict(kind="alpha", capcode=8, text="dropped", drop=True)],
         "C": [dict(kind="alpha", capcode=99, text="no signature", fragment=0, more=True)],
         "D": [dict(kind="numbered numeric", capcode=5, text="12345"), dict(kind="tone", address=(0x1F8000, 0x12345))]}
PPM = 44.0  # test_flex_host.py's: the last block of a 3200/4 frame needs a shift
# (mode, inverted, noise, frames, the sender's clock error in ppm)
CASES = [("1600/2", False, NOISE, 1, 0.0), ("1600/4", True, NOISE, 1, 0.0), ("3200/2", False, 0.0, 2, 0.0), ("3200/4", False, NOISE, 2, 0.0),
         ("3200/4", True, 0.0, 1, PPM)]


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _theta(mode, inverted, noise, frames, ppm):
    sent = []
    for k in range(frames):
        segments, _ = FM.make_frame(mode, 3, 45 + k, PAGES if k == 0 else {"A": PAGES["A"][:1]})
        sent.append((0.03 + k * (FM.FRAME_BITS / 1600.0 + 0.01), segments))
    n = int((0.05 + frames * (FM.FRAME_BITS / 1600.0 + 0.01) + 0.04) * FS)
    return FM.synth_theta(sent, FS, n, inverted=inverted, noise=noise, seed=7, ppm=ppm)


@pytest.fixture(scope="module")
def runs(A):
    """Every case through ``FlexDecoder`` once, and the oracle on the GPU's own planes."""
    out = {}
    for case in CASES:
        theta = _theta(*case)
        dec = A.FlexDecoder(FS)
        dec.process(theta)
        result = dec.finish()
        st = dec.stages()
        pl = FM.plan(FS)
        want = FM.decode_planes(st["v16"], st["v32"], [tuple(h) for h in st["hits"].tolist()], pl)
        out[case] = dict(theta=theta, result=result, st=st, want=want, plan=pl)
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{'inv' if c[1] else 'pos'}-{c[2]}-{c[3]}-{c[4]:g}")
def test_decoder_equals_the_oracle(A, runs, case):
    mode, inverted, noise, frames, ppm = case
    r = runs[case]
    st, want, pl = r["st"], r["want"], r["plan"]
    # the planes and the hits are section 25's
    p16, p32 = pl["ident"][1], pl["ident"][2]
    np.testing.assert_array_equal(st["v16"], IM.integrate(r["theta"], 0, p16["L"], p16["sh"]))
    assert (st["v32"] is not None) == (mode[:4] == "3200")
    if st["v32"] is not None:
        np.testing.assert_array_equal(st["v32"], IM.integrate(r["theta"], 0, p32["L"], p32["sh"]))
    _, kept = IM.search(st["v16"], p16, FM.FLEX_PATTERN)
    assert st["hits"].tolist() == [list(h) for h in kept]
    # the frames, their records and every word
    assert st["rows"] == want["rows"] and len(st["rows"]) == frames and all(row[1:] == (-1 if inverted else 1, mode) for row in st["rows"])
    assert st["unknown_mode"] == want["unknown_mode"] == 0 and st["ok"].tolist() == want["ok"].tolist() == [True] * frames
    np.testing.assert_array_equal(st["rec16"], want["rec16"])
    np.testing.assert_array_equal(st["rec32"], want["rec32"])
    for name in ("fixed", "raw", "status"):
        assert st[name].shape == (frames, 5, 4, 88) and st[name].dtype == want[name].dtype
        np.testing.assert_array_equal(st[name], want[name], err_msg=name)
    np.testing.assert_array_equal(st["chosen"], want["chosen"])
    assert st["chosen"].tolist() == ([[2] * 10 + [1]] if ppm else [[2] * 11] * frames)
    print(case, "status", np.unique(st["status"], return_counts=True), "chosen", st["chosen"].tolist())
    # the pages
    (ch,) = r["result"].channels
    assert [FM.page_key(p) for p in ch.pages] == [p[1:] for p in want["pages"]]
    assert [p.time_s for p in ch.pages] == [p[0] / FS for p in want["pages"]]
    sent = [p for p in ("ABCD") if p in FM.ACTIVE[mode]]
    first = [(p.phase, p.capcode, p.kind, p.text) for p in ch.pages if p.frame == 45]
    assert first == [(ph, None if "address" in pg else pg["capcode"], pg["kind"], None if "address" in pg else pg.get("text"))
                     for ph in sent for pg in PAGES[ph] if not pg.get("drop")]
    assert ch.frames == {mode: frames} and (ch.unknown_mode, ch.no_level, ch.fiw_failed, ch.biw_lost, ch.biw_bad) == (0, 0, 0, 0, 0)
    assert ch.vectors_dropped == (1 if "B" in sent else 0) and sum(ch.shifts.values()) == 11 * frames
    assert sum(ch.words.values()) == 88 * len(sent) * frames and set(ch.words) <= {"0", "1", "2"}
    assert A.FlexResult.from_json(json.loads(json.dumps(r["result"].to_json()))) == r["result"]


def test_uneven_cuts_give_identical_output(A, runs):
    case = CASES[3]
    r = runs[case]
    dec = A.FlexDecoder(FS)
    at = 0
    for n in (1, 2047, 2049, 1 << 30):
        dec.process(r["theta"][at : at + n])
        at += n
    assert dec.finish() == r["result"]
    st = dec.stages()
    for name in ("v16", "v32", "hits", "rec16", "rec32", "fixed", "raw", "status", "chosen"):
        np.testing.assert_array_equal(st[name], r["st"][name], err_msg=name)
    dec.reset()
    assert dec.finish().channels[0].pages == [] and dec.stages()["rows"] == []


def test_cli_lines_and_files(A, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import _native, cli, iqio

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith("iqa_flex_") or name.startswith("iqa_ident_"):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    raw = FM.capture(CLI_MODE)
    stem = f"model_{int(FC)}Hz"
    dirs = {}
    for tag in ("identify", "flex"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
        iqio.write_wav_iq(dirs[tag] / f"{stem}.wav", raw, int(FM.FS), "s16")
    # a --find-identify run calls no entry point of this section
    assert cli.main(["--in", str(dirs["identify"] / f"{stem}.wav"), "--find-identify"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert sorted(calls) == ["iqa_ident_integrate", "iqa_ident_search"] and not list(dirs["identify"].glob("*.flex.json"))
    assert len(plain) == 4 * len(FM.CAPTURE_CHANNELS) and plain[2].startswith("    keying: fsk 3200") and plain[3] == f"    protocol: flex {CLI_MODE} unconfirmed (1 frame)"
    # --find-flex: the same lines, the pages behind them, the same four JSON files, and flex.json
    calls.clear()
    assert cli.main(["--in", str(dirs["flex"] / f"{stem}.wav"), "--find-flex"]) == 0
    printed = capsys.readouterr().out.splitlines()
    # (a 3200-rate frame: the levels are taken on both planes, and the second plane is integrated here)
    assert sorted(calls) == ["iqa_flex_frames"] * 2 + ["iqa_flex_words"] + ["iqa_ident_integrate"] * 2 + ["iqa_ident_search"]
    assert printed[: len(plain)] == plain
    freq = int(round(FC + 200e3))
    want = [f'FLEX {CLI_MODE} 03.045.A cap=1234567 alpha "MODEL CAPTURE"', f'FLEX {CLI_MODE} 03.045.A cap=4242 numeric "555-0199"',
            f'FLEX {CLI_MODE} 03.045.C cap=99 alpha "PHASE C"']
    got = printed[len(plain) :]
    assert len(got) == 3 and all(line.endswith(": " + w) for line, w in zip(got, want)), got
    assert all(abs(int(line.split(" Hz: ")[0]) - freq) <= 1000 for line in got)
    for name in (f"{stem}.channels.json", f"{stem}.describe.json", f"{stem}.keying.json", f"{stem}.protocols.json"):
        assert (dirs["flex"] / name).read_bytes() == (dirs["identify"] / name).read_bytes(), name
    stored = A.FlexResult.from_json(json.loads((dirs["flex"] / f"{stem}.flex.json").read_text()))
    assert stored.lines() == got and [ch.note for ch in stored.channels] == ["", "no flex channel"] and stored.center_freq == FC
    flexch = stored.channels[0]
    assert flexch.frames == {CLI_MODE: 1} and flexch.words == {"0": 176} and abs(flexch.pages[0].time_s - (FM.CAPTURE_START + 49 / 1600.0)) < 2e-3
    five = A.find_channels(dirs["flex"] / f"{stem}.wav", describe=True, keying=True, identify=True, flex=True)
    assert len(five) == 5 and five[4] == stored
    assert len(A.find_channels(dirs["flex"] / f"{stem}.wav", describe=True, keying=True, identify=True)) == 4
