"""The protocol identification (--find-identify) on the MI355X, on the model capture of tests/ident_model.py
(seven channels of known protocol, s16): the integrator's output, the score planes and the sorted hit lists of every identified
channel equal the numpy oracle's, applied to the GPU's own stored theta and centre; the labels are the host test's; a stream fed
in uneven blocks gives the same hits; the CLI: a --find-decode run calls no entry point of the identification and writes the
same three JSON files as a --find-identify run, which prints the protocol lines and writes protocols.json."""
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


IM = _load("ident_model")
K = IM.K
FS = IM.FS
FC = 455.5e6


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _blocks(raw):
    from iq_to_audio_amd import find as FD

    flat = raw.reshape(-1)
    for a in range(0, raw.shape[0], FD.BLOCK_FRAMES):  # the blocks find_channels hands over
        yield flat[2 * a : 2 * min(raw.shape[0], a + FD.BLOCK_FRAMES)]


@pytest.fixture(scope="module")
def gpu(A):
    """The model capture through the finder and the identifying describer, once: everything the tests below read."""
    from iq_to_audio_amd import dsp_plan as P

    raw = IM.capture()
    plan = P.plan_find(FS, raw.shape[0])
    finder = A.ChannelFinder(plan, "s16")
    for block in _blocks(raw):
        finder.process(block)
    fin = finder.finish()
    found = finder.result(FC)
    describer = A.ChannelDescriber(plan, fin, found.channels, "s16", "iq", keep_stages=True, keying=True, identify=True)
    for block in _blocks(raw):
        describer.process(block)
    return dict(raw=raw, plan=plan, fin=fin, found=found, describer=describer, stages=describer.stages(), result=describer.result(FC),
                keying=describer.keying_result(FC), protocols=describer.protocol_result(FC))


def test_planes_and_hits_are_the_oracles(A, gpu):
    assert len(gpu["found"].channels) == len(IM.CHANNELS) == len(gpu["stages"])
    for (name, offset, keying, *_), ch, k, st in zip(IM.CHANNELS, gpu["found"].channels, gpu["keying"].channels, gpu["stages"]):
        assert abs(ch.offset_hz - offset) <= 1000.0 and k.label == keying, (name, ch.offset_hz, k.label)
        np.testing.assert_array_equal(st["stored"], st["theta"][st["keyed_from"] :])
        if name == "voice":
            assert st["ident_rate"] is None and st["ident_plan"] is None and st["hits"] is None and "v" not in st
            continue
        plan = st["ident_plan"]
        pl = IM.plan(st["plan"].fs_ch, st["ident_rate"])
        assert (plan.window, plan.half, plan.shift, plan.offsets) == (pl["L"], pl["h"], pl["sh"], tuple(pl["o"][i] for i in range(-16, 48)))
        pats = IM.family(st["ident_rate"])
        v = IM.integrate(st["stored"], st["c"], pl["L"], pl["sh"])
        assert v.size == st["theta"].size - st["keyed_from"] >= 300_000
        np.testing.assert_array_equal(st["v"], v, err_msg=name)
        planes, kept = IM.search(v, pl, pats)
        print(name, "candidates", [int(np.count_nonzero(row)) for row in planes], "kept", len(kept))
        assert st["score"].shape == planes.shape and st["score"].dtype == np.int32
        np.testing.assert_array_equal(st["score"], planes, err_msg=name)
        assert len(kept) >= 2 and st["hits"].tolist() == [list(h) for h in kept], name


def test_labels_are_the_host_tests(A, gpu):
    got = gpu["protocols"]
    assert isinstance(got, A.ProtocolResult) and (got.sample_rate, got.center_freq) == (FS, FC)
    for (name, _, keying, protocol, confirmed, mode), k, ch, st in zip(IM.CHANNELS, gpu["keying"].channels, got.channels, gpu["stages"]):
        print(name, ch.line())
        assert (ch.protocol, ch.confirmed, ch.mode) == (protocol, confirmed, mode), name
        assert (ch.offset_hz, ch.freq_hz, ch.baud) == (k.offset_hz, k.freq_hz, k.baud)
        if name == "voice":
            assert (ch.family, ch.hits, ch.pairs, ch.first_s, ch.line()) == (None, {}, {}, None, "    protocol: not looked for (unkeyed)")
            continue
        want = IM.decide([tuple(h) for h in st["hits"].tolist()], IM.family(ch.family), IM.plan(st["plan"].fs_ch, ch.family))
        assert (ch.hits, ch.pairs) == (want["hits"], want["pairs"]), name
        assert ch.first_s == (None if want["first_m"] is None else (st["keyed_from"] + want["first_m"]) / st["plan"].fs_ch)
    by = dict(zip(IM.NAMES, got.channels))
    assert by["dmr"].hits["dmr bs voice"] == 1 and by["dmr"].hits["dmr bs data"] >= 55 and by["dmr"].pairs["dmr"] >= 55
    assert by["dmr"].line().startswith("    protocol: dmr (bs data ") and by["dmr"].line().endswith(" pairs on the 30 ms grid)")
    assert by["flex"].line() == "    protocol: flex 3200/4 (2 frames)" and by["rand4"].line() == "    protocol: none (fsk 4800, no sync word)"
    assert abs(by["flex"].first_s - (IM.FLEX_AT[0] + 1) / 1600.0) < 2e-3  # the end of the marker's first bit, behind the channel filter's delay


def test_uneven_blocks_give_the_same_hits(A, gpu):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import identify as I

    describer = A.ChannelDescriber(gpu["plan"], gpu["fin"], gpu["found"].channels, "s16", "iq", keying=True, identify=True)
    lanes = describer.lanes()
    for j in (0, 3, 4):  # DMR, NXDN and FLEX
        st = gpu["stages"][j]
        z = D.from_numpy(st["z"])
        lane = lanes[j]
        lane.sh, lane.centre = st["sh"], st["c"]
        at = 0
        for n in [1, 2047, 2049, 1 << 30]:
            n = min(n, int(z.numel()) - at)
            describer.feed(lane, z[at : at + n])
            at += n
        assert at == int(z.numel()) and len(lane.stored) == 4 and lane.keyed_from == 0
        theta = D.torch_mod().cat(lane.stored)
        np.testing.assert_array_equal(theta.cpu().numpy(), st["stored"])
        v = I.integrate(theta, st["ident_plan"], lane.centre)
        _, hits = I.search(v, st["ident_plan"], I.patterns_for(st["ident_rate"]))
        np.testing.assert_array_equal(hits, st["hits"])
    describer.reset()
    assert all(lane.stored == [] for lane in describer.lanes())


def test_cli_lines_and_files(A, gpu, tmp_path, monkeypatch, capsys):
    from iq_to_audio_amd import _native, cli, iqio

    calls = []
    real = _native.call

    def counting(name, *args):
        if name.startswith("iqa_ident_"):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_native, "call", counting)
    stem = f"model_{int(FC)}Hz"
    dirs = {}
    for tag in ("decode", "identify"):
        dirs[tag] = tmp_path / tag
        dirs[tag].mkdir()
        iqio.write_wav_iq(dirs[tag] / f"{stem}.wav", gpu["raw"], int(FS), "s16")
    # a --find-decode run calls no entry point of the identification
    assert cli.main(["--in", str(dirs["decode"] / f"{stem}.wav"), "--find-decode"]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert calls == [] and len(plain) == 3 * len(IM.CHANNELS) and not list(dirs["decode"].glob("*.protocols.json"))
    # --find-identify: the same lines with the protocol line under each, the same three JSON files, and protocols.json
    assert cli.main(["--in", str(dirs["identify"] / f"{stem}.wav"), "--find-identify"]) == 0
    printed = capsys.readouterr().out.splitlines()
    assert sorted(calls) == ["iqa_ident_integrate"] * 6 + ["iqa_ident_search"] * 6
    assert [printed[i::4] for i in range(3)] == [plain[i::3] for i in range(3)] and printed[3::4] == gpu["protocols"].lines()
    assert all(line.startswith("    protocol: ") for line in printed[3::4])
    for name in (f"{stem}.channels.json", f"{stem}.describe.json", f"{stem}.keying.json"):
        assert (dirs["identify"] / name).read_bytes() == (dirs["decode"] / name).read_bytes(), name
    stored = A.ProtocolResult.from_json(json.loads((dirs["identify"] / f"{stem}.protocols.json").read_text()))
    assert stored == gpu["protocols"]
    res, des, key, named = A.find_channels(dirs["identify"] / f"{stem}.wav", describe=True, keying=True, identify=True)
    assert res == gpu["found"] and des == gpu["result"] and key == gpu["keying"] and named == gpu["protocols"]
    assert len(A.find_channels(dirs["identify"] / f"{stem}.wav", describe=True, keying=True)) == 3
