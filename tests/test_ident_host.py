"""The protocol identification without a GPU (--find-identify): the constants' self-checks, the plan against
the oracle's, the numpy oracle of tests/ident_model.py against plain Python loops, the model capture's protocols, the package's
host rules against the oracle's, every rule on both sides of its constant, the FLEX mode at distances 3 and 4, the
search-with-room path at capacity 1, the new usage errors and the entry points' argument checks."""
from __future__ import annotations

import importlib.util
import sys
from ctypes import c_int8, c_int32, c_int64, c_void_p
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


IM = _load("ident_model")
K = IM.K

import iq_to_audio_amd as A  # noqa: E402
from iq_to_audio_amd import cli  # noqa: E402
from iq_to_audio_amd import describe as DS  # noqa: E402
from iq_to_audio_amd import keying as KY  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd import identify as I  # noqa: E402

# the facts of the oracle on the model capture: (kept hits per name, on-grid pairs per protocol)
MODEL_FACTS = {
    "dmr": ({"dmr bs data": 60, "dmr bs voice": 1, "nxdn": 3, "nxdn inverted": 3}, {"dmr": 60}),
    "p25": ({"p25": 12, "nxdn": 5, "nxdn inverted": 3}, {"p25": 11}),
    "ysf": ({"ysf": 20, "nxdn": 2, "nxdn inverted": 1}, {"ysf": 19}),
    "nxdn": ({"nxdn": 58, "nxdn inverted": 3}, {"nxdn": 38}),
    "flex": ({"flex": 2}, {"flex": 1}),
    "rand4": ({"nxdn": 3, "nxdn inverted": 1}, {}),
}


# ---- the constants and the plan -----------------------------------------------------------------------------------------------


def test_constants_check_themselves():
    by = {p.positive: p for p in I.PATTERNS}
    assert [(p.protocol, p.positive, p.negative, p.word, p.symbols, p.grid, p.families, p.binary) for p in I.PATTERNS] == list(IM.PATTERNS)
    for p, q in zip(I.PATTERNS, IM.PATTERNS):
        assert list(I.symbols_of(p)) == IM.symbols(q) and len(IM.symbols(q)) == p.symbols <= P.IDENT_MAX_SYMBOLS
    # the DMR data words are the voice words xor 0xAAAAAAAAAAAA: every dibit's first bit flipped, which negates every symbol
    for name in ("dmr bs voice", "dmr ms voice"):
        data = by[name].word ^ 0xAAAAAAAAAAAA
        levels = [IM.LEVEL[(data >> (2 * (23 - i))) & 3] for i in range(24)]
        assert levels == [-s for s in I.symbols_of(by[name])]
    assert by["dmr bs voice"].word ^ 0xAAAAAAAAAAAA == 0xDFF57D75DF5D and by["dmr ms voice"].word ^ 0xAAAAAAAAAAAA == 0xD5D7F77FD757
    for name in ("dmr bs voice", "dmr ms voice", "p25"):
        assert set(I.symbols_of(by[name])) == {-3, 3}
    assert bin(by["flex"].word).count("1") == 16 and set(I.symbols_of(by["flex"])) == {-1, 1}
    assert I.symbols_of(by["nxdn"]) == (-3, 1, -3, 3, -3, -3, 3, 3, -1, 3)
    assert I.DIBIT == IM.LEVEL == {1: 3, 0: 1, 2: -1, 3: -3} and I.FAMILY_OF_BAUD == IM.FAMILY and I.FLEX_MODES == IM.MODES
    codes = [c for c, _ in I.FLEX_MODES]
    assert min(bin(a ^ b).count("1") for a in codes for b in codes if a != b) > 2 * I.FLEX_MAX_DISTANCE  # no hit fits two modes
    assert [p.positive for p in I.patterns_for(4800)] == ["dmr bs voice", "dmr ms voice", "p25", "ysf", "nxdn"]
    assert [p.positive for p in I.patterns_for(2400)] == ["nxdn"] and [p.positive for p in I.patterns_for(1600)] == ["flex"]


@pytest.mark.parametrize("fs_ch, rate, L, h, sh", [(19_200.0, 4800, 4, 2, 0), (160_000.0, 4800, 33, 16, 0), (96_600.0, 4800, 20, 10, 0),
                                                   (358_400.0, 1600, 224, 112, 2), (218_181.81818181818, 1600, 136, 68, 2),
                                                   (312_000.0, 4800, 65, 32, 1)])
def test_plan_is_the_oracles(fs_ch, rate, L, h, sh):
    got, want = P.plan_ident(fs_ch, rate), IM.plan(fs_ch, rate)
    assert (got.window, got.half, got.shift) == (want["L"], want["h"], want["sh"]) == (L, h, sh) and got.sps == want["sps"]
    assert got.offsets == tuple(want["o"][i] for i in range(-16, 48)) and [got.o(i) for i in (-16, 0, 47)] == [want["o"][i] for i in (-16, 0, 47)]
    assert got.o(0) == 0 and len(got.offsets) == P.IDENT_OFFSETS and ((L * 65534) >> sh) <= IM.V_MAX
    if fs_ch == 96_600.0:  # 20.125 samples to a symbol: the ties at i = 4 (80.5), 12 (241.5), -4 go to the even neighbour
        assert (got.o(4), got.o(12), got.o(20), got.o(-4), got.o(-12)) == (80, 242, 402, -80, -242)


def test_plan_refuses_rates_that_do_not_fit():
    for fs_ch, rate in ((19_199.0, 4800), (358_401.0, 1600), (6_399.0, 1600), (1_075_201.0, 4800), (9_599.0, 2400)):
        with pytest.raises(ValueError, match="must be 4 .. 224"):
            P.plan_ident(fs_ch, rate)
        with pytest.raises(ValueError, match="does not fit"):
            IM.plan(fs_ch, rate)
        assert I.family_plan("fsk x", {1600: 1600, 2400: 2400, 4800: 4800}[rate], fs_ch) == (rate, None, "rate does not fit")
    for fs_ch, rate in ((19_200.0, 4800), (358_400.0, 1600)):
        P.plan_ident(fs_ch, rate)
    with pytest.raises(ValueError, match="positive"):
        P.plan_ident(0.0, 4800)
    assert I.family_plan("fsk 1200", 1200, 96_000.0) == (None, None, "fsk 1200") and I.family_plan("unkeyed", None, 96_000.0)[0] is None
    assert I.family_plan("fsk 3200", 3200, 96_000.0)[1] == P.plan_ident(96_000.0, 1600)


# ---- the oracle against loops ---------------------------------------------------------------------------------------------------


def test_oracle_against_loops():
    rng = np.random.default_rng(3)
    theta = (0.4 * rng.standard_normal(700)).astype(np.float32)
    theta[[5, 77]] = [np.nan, np.inf]
    for L, sh, c in ((4, 0, 0), (33, 0, 300), (224, 2, -32767), (65, 1, 12)):
        assert IM.integrate(theta, c, L, sh).tolist() == IM.integrate_by_loops(theta, c, L, sh)
    pl = IM.plan(24_000.0, 4800)  # 5 samples to a symbol
    pats = IM.family(4800)
    levels = IM.symbols(pats[0]) + [1, -3] + [-s for s in IM.symbols(pats[4])]
    clean = IM.crafted_plane(400, pl, 100, levels, amp=700)
    noisy = clean + rng.integers(-150, 150, 400)
    assert IM.score(noisy, pl, pats).tolist() == IM.score_by_loops(noisy, pl, pats) and IM.score(noisy, pl, pats).any()
    planes, kept = IM.search(clean, pl, pats)
    assert planes.tolist() == IM.score_by_loops(clean, pl, pats)
    assert [(j, m) for j, m, *_ in kept] == [(0, 100), (4, 100 + pl["o"][26])] and kept[0][2] > 0 > kept[1][2]


# ---- the model capture ---------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def model():
    return IM.model_run()


def test_model_capture_names_its_protocols(model):
    assert len(model["found"]) == len(IM.CHANNELS)
    for (name, offset, keying, protocol, confirmed, mode), ch, d, k, nm in zip(IM.CHANNELS, model["found"], model["described"], model["keyed"],
                                                                               model["named"]):
        assert abs(ch["offset_hz"] - offset) <= 1000.0 and d["label"] == "nfm" and k["label"] == keying, name
        print(name, d["plan"]["fs_ch"], k["label"], nm["hits"], nm["pairs"], nm["protocol"], nm["mode"])
        if name == "voice":  # not keyed: nothing is searched
            assert nm["rate"] is None and nm["kept"] is None
            continue
        # the oracle's own facts first
        assert (nm["hits"], nm["pairs"]) == MODEL_FACTS[name], name
        assert nm["rate"] == (1600 if name == "flex" else 4800) and k["keyed_from"] == 0
        assert (nm["protocol"], nm["confirmed"], nm["mode"]) == (protocol, confirmed, mode), name
    rand = model["named"][IM.NAMES.index("rand4")]
    assert all(IM.family(4800)[j][4] < 20 for j, *_ in rand["kept"])  # not one kept hit of a pattern of twenty symbols or more
    flex = model["named"][IM.NAMES.index("flex")]
    m0, m1 = (m for _, m, *_ in flex["kept"])
    assert abs((m1 - m0) - round(3000 * flex["plan"]["sps"])) <= 2 and [IM.flex_words(h[4], h[5], False) for h in flex["kept"]] == [(0xDEA0, 0x215F)] * 2
    dmr = model["named"][IM.NAMES.index("dmr")]
    voice = [m for j, m, C, *_ in dmr["kept"] if j == 0 and C > 0]
    assert len(voice) == 1 and abs(voice[0] - (IM.DMR_VOICE_SLOT * 144 + 60 + 1) * dmr["plan"]["sps"]) < 2 * dmr["plan"]["sps"]


def test_package_rules_equal_the_oracle(model):
    for name, k, nm, d in zip(IM.NAMES, model["keyed"], model["named"], model["described"]):
        rate, plan, note = I.family_plan(k["label"], k["baud"], d["plan"]["fs_ch"])
        assert rate == nm["rate"]
        keyed = KY.ChannelKeying(offset_hz=1.0, freq_hz=None, described="nfm", fs_ch=d["plan"]["fs_ch"], bauds=[], coh=[], rate_hz=None, crossings=0,
                                 pairs=0, centre=k["c"], label=k["label"], baud=k["baud"], decoders=[], bw=None, note="")
        if rate is None:
            got = I.protocol_of(keyed, None, plan, rate, note, None)
            assert (got.protocol, got.family, got.line()) == (None, None, "    protocol: not looked for (unkeyed)")
            continue
        got = I.decide(np.array(nm["kept"], dtype=np.int64), I.patterns_for(rate), plan)
        for key in ("hits", "pairs", "protocol", "confirmed", "mode", "first_m"):
            assert got[key] == nm[key], (name, key)
        ch = I.protocol_of(keyed, np.array(nm["kept"], dtype=np.int64).reshape(-1, 6), plan, rate, note, k["keyed_from"])
        assert (ch.protocol, ch.confirmed, ch.mode, ch.hits, ch.pairs) == (nm["protocol"], nm["confirmed"], nm["mode"], nm["hits"], nm["pairs"])
        assert ch.first_s == (None if nm["first_m"] is None else nm["first_m"] / d["plan"]["fs_ch"])
        line = {"dmr": "    protocol: dmr (bs data 60, bs voice 1; 60 pairs on the 30 ms grid)",
                "p25": "    protocol: p25 (p25 12; 11 pairs on the 7.5 ms grid)", "ysf": "    protocol: ysf (ysf 20; 19 pairs on the 100 ms grid)",
                "nxdn": "    protocol: nxdn (nxdn 58, nxdn inverted 3; 38 pairs on the 40 ms grid)",
                "flex": "    protocol: flex 3200/4 (2 frames)", "rand4": "    protocol: none (fsk 4800, no sync word)"}[name]
        assert ch.line() == line
        assert A.ChannelProtocol(**ch.to_json()) == ch
    res = A.ProtocolResult(channels=[ch], sample_rate=2.4e6, center_freq=None)
    assert A.ProtocolResult.from_json(res.to_json()) == res and res.lines() == [ch.line()]


# ---- every rule on both sides of its constant -----------------------------------------------------------------------------------


def _hit(j, m, C=1000, pre=0, post=0):
    return (j, m, C, 1, pre, post)


def _both(hits, rate, fs_ch):
    pl, plan = IM.plan(fs_ch, rate), P.plan_ident(fs_ch, rate)
    want = IM.decide(hits, IM.family(rate), pl)
    got = I.decide(np.array(hits, dtype=np.int64).reshape(-1, 6), I.patterns_for(rate), plan)
    for key in ("hits", "pairs", "protocol", "confirmed", "mode", "first_m"):
        assert got[key] == want[key], key
    return want


def test_threshold_on_equality():
    pl = IM.plan(19_200.0, 1600)  # 12 samples to a symbol
    flex = IM.family(1600)
    sym = IM.symbols(flex[0])
    for k, kept in ((5, True), (6, True), (7, False), (8, False)):  # 16 (32 - k) >= 416: on equality at k = 6
        lev = list(sym)
        for i in range(k):
            lev[3 * i + 1] = 0
        v = IM.crafted_plane(600, pl, 50, lev, amp=-900)
        planes, hits = IM.search(v, pl, flex)
        assert (planes[0, 50] != 0) == kept and planes.tolist() == IM.score_by_loops(v, pl, flex)
        assert [(m, C) for _, m, C, *_ in hits] == ([(50, -900 * (32 - k))] if kept else [])
    pats = IM.family(4800)
    pl = IM.plan(24_000.0, 4800)
    p25 = IM.symbols(pats[2])
    for k, kept in ((4, True), (5, False)):  # 16 * 9 (24 - k)^2 >= 13 * 216 (24 - k): k <= 4.5
        lev = [0 if i < k else s for i, s in enumerate(p25)]
        planes, hits = IM.search(IM.crafted_plane(400, pl, 20, lev, amp=11), pl, pats)
        assert (planes[2, 20] != 0) == kept and bool(hits) == kept


def test_keep_window_and_grid_windows():
    pl = IM.plan(24_000.0, 4800)  # h = 2
    pats = IM.family(4800)
    row = np.zeros((5, 300), dtype=np.int64)
    row[0, [10, 12, 20, 23, 30, 31, 32, 40]] = [2 * 50, 2 * 60, 2 * 50, 2 * 60, 2 * 70, 2 * 70 + 1, 2 * 70, 2 * 5]
    kept = IM.keep(np.zeros(300, dtype=np.int64), row, pl, pats)
    assert [m for _, m, *_ in kept] == [12, 20, 23, 30, 40]  # within +-h the larger wins, at h + 1 both stay; a plateau keeps its first
    # the pair rule: a distance within +-h of rint(k G sps), k >= 1
    fs = 160_000.0
    pl = IM.plan(fs, 4800)
    step = round(144 * pl["sps"])
    for d, on in ((step, True), (step + 16, True), (step - 16, True), (step + 17, False), (step - 17, False), (round(5 * 144 * pl["sps"]) + 16, True),
                  (round(5 * 144 * pl["sps"]) - 17, False), (16, False), (0, False)):
        assert IM.on_grid(d, 144, pl) == I.on_grid(d, 144, P.plan_ident(fs, 4800)) == on, d
        res = _both([_hit(0, 1000), _hit(0, 1000 + d, -1000)], 4800, fs)  # a voice and a data word: either sign
        assert (res["protocol"], res["confirmed"], res["pairs"]) == ("dmr", on, {"dmr": 1} if on else {})
        assert res["hits"] == {"dmr bs voice": 1, "dmr bs data": 1}
    # hits of two patterns do not pair
    res = _both([_hit(0, 1000), _hit(1, 1000 + step)], 4800, fs)
    assert (res["confirmed"], res["pairs"], res["protocol"]) == (False, {}, "dmr")


def test_seen_confirmed_and_ties():
    fs = 160_000.0
    pl = IM.plan(fs, 4800)
    g = lambda j: round(IM.family(4800)[j][5] * pl["sps"])  # noqa: E731
    assert _both([], 4800, fs)["protocol"] is None
    res = _both([_hit(3, 500)], 4800, fs)  # twenty symbols: seen
    assert (res["protocol"], res["confirmed"], res["first_m"]) == ("ysf", False, 500)
    assert _both([_hit(4, 500), _hit(4, 900), _hit(4, 1000, -5)], 4800, fs)["protocol"] is None  # nxdn is never merely seen
    res = _both([_hit(4, 500), _hit(4, 500 + g(4))], 4800, fs)
    assert (res["protocol"], res["confirmed"]) == ("nxdn", True)
    # a confirmed protocol beats any number of seen hits; the most pairs win; ties go to table order
    res = _both([_hit(2, 10), _hit(2, 300), _hit(2, 700), _hit(4, 500), _hit(4, 500 + g(4))], 4800, fs)
    assert (res["protocol"], res["hits"]["p25"]) == ("nxdn", 3)
    res = _both([_hit(3, 0), _hit(3, g(3)), _hit(3, 2 * g(3)), _hit(2, 5), _hit(2, 5 + g(2))], 4800, fs)
    assert (res["protocol"], res["pairs"]) == ("ysf", {"ysf": 2, "p25": 1})
    res = _both([_hit(3, 0), _hit(3, g(3)), _hit(2, 5), _hit(2, 5 + g(2)), _hit(1, 7), _hit(1, 7 + g(1))], 4800, fs)
    assert res["protocol"] == "dmr"
    res = _both([_hit(3, 0), _hit(2, 5)], 4800, fs)
    assert (res["protocol"], res["confirmed"]) == ("p25", False)
    res = _both([_hit(3, 0), _hit(3, 77), _hit(2, 5)], 4800, fs)
    assert res["protocol"] == "ysf"
    # nxdn at 2400 symbols/s
    pl2 = IM.plan(96_000.0, 2400)
    res = _both([_hit(0, 40), _hit(0, 40 + round(192 * pl2["sps"]))], 2400, 96_000.0)
    assert (res["protocol"], res["confirmed"]) == ("nxdn", True)


def _time_bits(word):
    """pre / post of a sixteen-bit word sent MSB first: bit k the k-th in time."""
    return sum(((word >> (15 - k)) & 1) << k for k in range(16))


def test_flex_mode_distances():
    fs = 19_200.0
    flip = lambda word, bits: word ^ sum(1 << b for b in bits)  # noqa: E731
    for code, name in IM.MODES:
        for wrong_a, wrong_b, counts, mode in (((), (), True, name), ((1, 9), (4,), True, name), ((0, 5, 15), (), True, name), ((), (2, 3, 11), True, name),
                                               ((1, 9), (4, 6), False, None), ((0, 5, 15, 7), (), False, None), ((3,), (3,), True, name),
                                               ((3, 8), (3, 8), True, "?"), ((3, 8, 12), (3, 8, 12), True, "?")):
            a, b = flip(code, wrong_a), flip(code ^ 0xFFFF, wrong_b)
            # (A xor ~B counts the bits where the two copies differ: an error in both at one place goes unseen there, twice in the mode)
            assert IM.flex_mode(a, b) == mode and I.flex_counts(a, b) == counts, (name, wrong_a, wrong_b)
            if counts:
                assert I.flex_mode(a, b) == mode
            for inverted in (False, True):
                pre, post = (_time_bits(a), _time_bits(b)) if not inverted else (_time_bits(a ^ 0xFFFF), _time_bits(b ^ 0xFFFF))
                assert I.flex_words(pre, post, inverted) == IM.flex_words(pre, post, inverted) == (a, b)
                res = _both([_hit(0, 100, -7 if inverted else 7, pre, post)], 1600, fs)
                want = ("flex", False, mode, {"flex inverted" if inverted else "flex": 1}) if counts else (None, False, None, {})
                assert (res["protocol"], res["confirmed"], res["mode"], res["hits"]) == want
    # the mode of a channel: the most frequent known one
    pre = lambda code: _time_bits(code)  # noqa: E731
    post = lambda code: _time_bits(code ^ 0xFFFF)  # noqa: E731
    step = round(3000 * 12.0)
    hits = [_hit(0, 100, 7, pre(0x7B18), post(0x7B18)), _hit(0, 100 + step, 7, pre(0xDEA0), post(0xDEA0)), _hit(0, 100 + 2 * step, 7, pre(0xDEA0), post(0xDEA0)),
            _hit(0, 100 + 3 * step, 7, pre(0x1234), post(0x1234)), _hit(0, 100 + 4 * step + 30, 7, pre(0x1234), post(0x1235))]
    res = _both(hits, 1600, fs)
    assert (res["protocol"], res["confirmed"], res["mode"], res["hits"], res["pairs"]) == ("flex", True, "3200/4", {"flex": 5}, {"flex": 3})


def test_lines():
    mk = lambda **kw: I.ChannelProtocol(**{**dict(offset_hz=0.0, freq_hz=None, baud=4800, family=4800, hits={}, pairs={}, protocol=None,  # noqa: E731
                                                  confirmed=False, mode=None, first_s=None, note=""), **kw})
    assert mk(hits={"dmr bs data": 431, "dmr bs voice": 12, "nxdn": 2}, pairs={"dmr": 440}, protocol="dmr", confirmed=True).line() == \
        "    protocol: dmr (bs data 431, bs voice 12; 440 pairs on the 30 ms grid)"
    assert mk(baud=3200, family=1600, hits={"flex": 31}, pairs={"flex": 30}, protocol="flex", confirmed=True, mode="3200/4").line() == \
        "    protocol: flex 3200/4 (31 frames)"
    assert mk(note="no sync word").line() == "    protocol: none (fsk 4800, no sync word)"
    assert mk(note="rate does not fit").line() == "    protocol: none (fsk 4800, rate does not fit)"
    assert mk(hits={"ysf inverted": 1}, protocol="ysf").line() == "    protocol: ysf unconfirmed (ysf inverted 1)"
    assert mk(baud=1600, family=1600, hits={"flex": 1}, protocol="flex", mode="?").line() == "    protocol: flex ? unconfirmed (1 frame)"
    assert mk(baud=None, family=None, note="wfm").line() == "    protocol: not looked for (wfm)"
    assert mk(baud=2400, family=2400, hits={"nxdn": 2}, pairs={"nxdn": 1}, protocol="nxdn", confirmed=True).line() == \
        "    protocol: nxdn (nxdn 2; 1 pair on the 80 ms grid)"


# ---- the search that may need more room ----------------------------------------------------------------------------------------


def test_search_with_room_at_capacity_one():
    """``decoders.common.search_with_room`` around a search that behaves as ``iqa_ident_search`` does: it fills what the list
    holds and counts every kept hit.  At capacity 1 with three hits the call is repeated with room for three."""
    import torch

    from iq_to_audio_amd.decoders.common import search_with_room

    pl = IM.plan(24_000.0, 4800)
    pats = IM.family(4800)
    v = IM.crafted_plane(900, pl, 30, IM.symbols(pats[2]))
    v = IM.crafted_plane(900, pl, 330, [-s for s in IM.symbols(pats[3])], base=v)
    v = IM.crafted_plane(900, pl, 600, IM.symbols(pats[2]), base=v)
    _, hits = IM.search(v, pl, pats)
    assert [(j, m) for j, m, *_ in hits] == [(2, 30), (2, 600), (3, 330)]
    counts, rooms = torch.zeros(1, dtype=torch.int64), []

    def run(room):
        rooms.append(room)
        counts[0] = len(hits)
        return hits[::-1][:room]  # (in no particular order, and never more than the list holds)

    (lst,), (kept,) = search_with_room([run], counts, 1)
    assert rooms == [1, 3] and kept == 3 and I.sort_hits(lst).tolist() == [list(h) for h in hits]
    rooms.clear()
    (lst,), (kept,) = search_with_room([run], counts, 3)
    assert rooms == [3] and kept == 3


# ---- the CLI, the package surface, the C ABI ------------------------------------------------------------------------------------


def _usage_error(argv, capsys):
    with pytest.raises(SystemExit) as exc:
        cli.main(argv)
    assert exc.value.code == 2
    return capsys.readouterr().err


def test_cli_refuses_misuse(capsys):
    base = ["--in", "capture.wav"]
    assert "--find-identify cannot be combined with --ft." in _usage_error(base + ["--find-identify", "--ft", "455800000"], capsys)
    assert "--find-identify cannot be combined with --benchmark." in _usage_error(base + ["--find-identify", "--benchmark"], capsys)
    assert "--find-identify cannot be combined with --audio-post." in _usage_error(base + ["--find-identify", "--audio-post", "x"], capsys)
    assert "--find-identify cannot be combined with --probe-only." in _usage_error(base + ["--find-identify", "--probe-only"], capsys)
    assert "--find-identify needs --in." in _usage_error(["--find-identify"], capsys)
    assert "--find-auto needs --find-top." in _usage_error(base + ["--find-identify", "--find-auto"], capsys)
    assert "--find-auto cannot be combined with --pocsag." in _usage_error(base + ["--find-top", "2", "--find-auto", "--find-identify", "--pocsag"], capsys)
    assert "--find-decode cannot be combined with --ft." in _usage_error(base + ["--find-decode", "--find-identify", "--ft", "1e6"], capsys)
    # --find-identify implies --find-decode: a threshold is accepted with it alone
    args = cli.build_parser().parse_args(base + ["--find-identify", "--find-threshold", "8"])
    assert args.find_decode is False
    assert cli.check_find_args(cli.build_parser(), args) is True and (args.find_identify, args.find_decode, args.find_describe) == (True, True, False)
    args = cli.build_parser().parse_args(base + ["--find-decode"])
    assert cli.check_find_args(cli.build_parser(), args) is True and args.find_identify is False


def test_package_surface():
    for name in ("ChannelProtocol", "ProtocolResult"):
        assert getattr(A, name) is getattr(I, name)
    assert A.plan_ident is P.plan_ident and A.IdentPlan is P.IdentPlan
    text = Path(I.__file__).read_text()
    assert "scipy" not in text and "import oracle" not in text and "from oracle" not in text
    plan = P.plan_find(2.4e6, 100_000)
    fin = dict(runs=np.zeros((0, 8), dtype=np.int64), on=np.zeros((0, plan.slices), dtype=np.uint8))
    with pytest.raises(ValueError, match="identify=True needs keying=True"):
        DS.ChannelDescriber(plan, fin, [], identify=True)
    with pytest.raises(ValueError, match="without identify=True"):
        DS.ChannelDescriber(plan, fin, [], keying=True).finish_identify()
    with pytest.raises(ValueError, match="identify=True needs keying=True"):
        A.find_channels("nothing.wav", describe=True, identify=True)
    with pytest.raises(ValueError, match="keying=True needs describe=True"):
        A.find_channels("nothing.wav", keying=True, identify=True)


def test_c_abi_refuses_bad_arguments():
    """The library has the two entry points, and the argument checks come before the launch, so they run without a GPU."""
    from iq_to_audio_amd import _native as N

    null, some = c_void_p(0), c_void_p(8)  # (never dereferenced: every call below is refused, or has nothing to do)
    for name in ("iqa_ident_integrate", "iqa_ident_search"):
        assert hasattr(N.lib(), name) and name in N.EXPORTS
    assert N.lib().iqa_abi_version() == 1
    header = (Path(__file__).resolve().parent.parent / "include" / "iqa_hotpath.h").read_text()
    for text in ("#define IQA_IDENT_MIN_SPS 4", "#define IQA_IDENT_MAX_SPS 224", "#define IQA_IDENT_OFFSETS 64", "#define IQA_IDENT_MAX_SYMBOLS 32",
                 "#define IQA_IDENT_MAX_PATTERNS 8", "#define IQA_IDENT_RECORD 6", "#define IQA_ABI_VERSION 1"):
        assert text in header
    assert (P.IDENT_MIN_SPS, P.IDENT_MAX_SPS, P.IDENT_OFFSETS, P.IDENT_MAX_SYMBOLS, P.IDENT_RECORD, P.IDENT_MAX_N) == (4, 224, 64, 32, 6, 1 << 30)
    i32, i64 = c_int32, c_int64

    def integ(theta=some, n=100, L=33, sh=0, c=0, v=some):
        N.call("iqa_ident_integrate", theta, i64(n), i32(L), i32(sh), i32(c), v, null)

    for kwargs, what in ((dict(n=-1), "negative"), (dict(n=(1 << 30) + 1), "2\\^30"), (dict(L=3), "L must"), (dict(L=225), "L must"), (dict(sh=-1), "sh must"),
                         (dict(sh=9), "sh must"), (dict(L=65, sh=0), "sh must"), (dict(L=224, sh=1), "sh must"), (dict(c=32768), "centre"),
                         (dict(c=-32768), "centre"), (dict(theta=null), "NULL"), (dict(v=null), "NULL")):
        with pytest.raises(ValueError, match=what):
            integ(**kwargs)
    integ(theta=null, v=null, n=0)  # nothing to do: no pointer is touched
    integ(theta=null, v=null, n=0, L=224, sh=2, c=-32767)

    plan = P.plan_ident(160_000.0, 4800)
    pats = I.patterns_for(4800)
    table = np.zeros((len(pats), 32), dtype=np.int8)
    for j, pat in enumerate(pats):
        table[j, : pat.symbols] = I.symbols_of(pat)

    def srch(v=some, n=5000, offsets=plan.offsets, npat=len(pats), symbols=table, nsym=tuple(p.symbols for p in pats), half=16, score=some,
             lst=some, capacity=8, count=some):
        off = None if offsets is None else (c_int32 * 64)(*offsets)
        sym = None if symbols is None else (c_int8 * symbols.size)(*symbols.reshape(-1).tolist())
        ns = None if nsym is None else (c_int32 * len(nsym))(*nsym)
        N.call("iqa_ident_search", v, i64(n), off, i32(npat), sym, ns, i32(half), score, lst, i64(capacity), count, null)

    def offs(k, value):
        o = list(plan.offsets)
        o[k] = value
        return tuple(o)

    def syms(p, i, value):
        t = table.copy()
        t[p, i] = value
        return t

    wide = P.plan_ident(358_400.0, 1600)
    for kwargs, what in ((dict(n=-1), "negative"), (dict(capacity=-1), "negative"), (dict(n=(1 << 30) + 1), "2\\^30"), (dict(offsets=None), "NULL offsets"),
                         (dict(symbols=None), "NULL offsets"), (dict(nsym=None), "NULL offsets"), (dict(npat=0), "npat"), (dict(npat=9), "npat"),
                         (dict(half=-1), "half"), (dict(half=225), "half"), (dict(offsets=offs(16, 1)), "o\\[0\\]"), (dict(offsets=offs(20, 100)), "ascend"),
                         (dict(offsets=offs(63, 1567 + 200)), "step"), (dict(nsym=(24, 24, 24, 0, 10)), "1 .. IQA_IDENT_MAX_SYMBOLS"),
                         (dict(nsym=(24, 24, 33, 20, 10)), "1 .. IQA_IDENT_MAX_SYMBOLS"), (dict(symbols=syms(0, 0, 0)), "symbol must"),
                         (dict(symbols=syms(4, 9, 2)), "symbol must"), (dict(symbols=syms(1, 23, -5)), "symbol must"),
                         (dict(offsets=tuple(i * 225 for i in range(-16, 48)), npat=1, nsym=(32,), symbols=table[:1] | 1), "31 IQA_IDENT_MAX_SPS"),
                         (dict(v=null), "NULL device"), (dict(score=null), "NULL device"), (dict(lst=null), "NULL device"), (dict(count=null), "NULL device")):
        with pytest.raises(ValueError, match=what):
            srch(**kwargs)
    srch(v=null, n=0, score=null, lst=null, count=null)  # nothing to do: no pointer is touched
    srch(v=null, n=0, score=null, lst=null, count=null, offsets=wide.offsets, half=112, capacity=0)
