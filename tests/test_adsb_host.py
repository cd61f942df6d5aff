"""ADS-B / Mode S beside AM (--demod am --adsb), the host side: the protocol constants pinned on published frames, the
numpy oracle (tests/adsb_model.py) alone over channel rates, sub-sample offsets, carrier offsets and noise, no frame kept
on noise and on a voice carrier, ``plan_adsb`` against the oracle's plan, ``parse_frames`` against the oracle's parser
(grouping, the pairing window, the NL mismatch, the None fields, the aircraft table) and the command line's usage errors.
No GPU needed."""
from __future__ import annotations

import importlib.util
import json
import sys
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


M = _load("adsb_model")
OFFGRID = json.loads((Path(__file__).parent / "golden" / "adsb_offgrid.json").read_text())


def _records(frames, starts, level=100_000):
    """Kept-list records as ``parse_frames`` takes them, and as the oracle's parser does."""
    rows = [(int(s), 8 * len(f), level, bytes(f)) for f, s in zip(frames, starts)]
    rec = dict(n=[r[0] for r in rows], nbits=[r[1] for r in rows], P=[r[2] for r in rows],
               data=np.array([list(r[3].ljust(14, b"\0")) for r in rows], dtype=np.uint8).reshape(len(rows), 14))
    return rec, rows


def _parse_both(fs, frames, starts):
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.decoders import adsb as AD

    rec, rows = _records(frames, starts)
    res, want = AD.parse_frames(P.plan_adsb(fs), rec, 7), M.parse(rows, M.plan(fs))
    got = [] if res is None else res.messages
    assert [tuple(getattr(m, k) for k in M.FIELDS) for m in got] == [tuple(m[k] for k in M.FIELDS) for m in want["messages"]]
    if res is not None:
        assert res.aircraft == want["aircraft"] and (res.candidates, res.crc_ok) == (7, len(rows))
    return res


# ---- constants ------------------------------------------------------------------------------------------------------------


def test_published_frames_pin_the_constants():
    from iq_to_audio_amd.decoders import adsb as AD

    for frame in M.PUBLISHED:
        assert M.syndrome(frame) == 0 and AD.syndrome(frame) == 0
    bad = bytearray(M.IDENT)
    bad[-1] ^= 1
    assert M.syndrome(bytes(bad)) == 1 and AD.syndrome(bytes(bad)) == 1
    assert M.syndrome(M.DF11) == 0 and len(M.DF11) == 7 and M.DF11[0] >> 3 == 11
    assert M.build_frame(17, 0x4840D6, int.from_bytes(M.IDENT[4:11], "big")) == M.IDENT
    ident = _parse_both(2e6, [M.IDENT], [0]).messages[0]
    assert (ident.icao, ident.type_code, ident.callsign, ident.df) == ("4840D6", 4, "KLM1023", 17)
    assert ident.line() == "ADS-B 4840D6 ident KLM1023"
    # the pair: both parities at 38 000 ft; the newer message's parity picks the position
    odd = _parse_both(2e6, [M.POS_EVEN, M.POS_ODD], [0, 1000]).messages
    assert [(m.altitude_ft, m.cpr_odd, m.lat_cpr, m.lon_cpr) for m in odd] == [(38000, 0, 93000, 51372), (38000, 1, 74158, 50194)]
    assert odd[0].lat is None and (odd[1].lat, odd[1].lon) == (52.26578017412606, 3.938912527901786)
    even = _parse_both(2e6, [M.POS_ODD, M.POS_EVEN], [0, 1000]).messages
    assert (even[1].lat, even[1].lon) == (52.2572021484375, 3.91937255859375)
    assert even[1].line() == "ADS-B 40621D pos 52.25720N 3.91937E 38000ft"
    vel = _parse_both(2e6, [M.VELOCITY], [0]).messages[0]
    assert (vel.type_code, vel.vertical_rate_fpm) == (19, -832)
    assert abs(vel.speed_kt - 159.2011) < 5e-5 and abs(vel.track_deg - 182.8804) < 5e-5 and vel.speed_kt == float(np.hypot(-8, -159))
    assert vel.line() == "ADS-B 485020 vel 159.2kn 182.9° -832fpm"
    sub3 = _parse_both(2e6, [M.VELOCITY_3], [0]).messages[0]  # TC 19 subtype 3: the common fields only
    assert (sub3.icao, sub3.type_code, sub3.speed_kt, sub3.track_deg, sub3.vertical_rate_fpm) == ("A05F21", 19, None, None, None)


# ---- the oracle alone -----------------------------------------------------------------------------------------------------


def test_oracle_grid():
    """144 cases of four frames.  No kept frame ever differs from a transmitted one; every case on the grid (offset 0) and
    every case at 4 MHz and above decodes all four; off the grid at 2 - 2.5 MHz exactly the committed table decodes."""
    table, share = {}, []
    for fs in M.RATES:
        for frac in M.OFFSETS:
            for carrier in M.CARRIERS:
                for sigma in M.SIGMAS:
                    clean, every = M.case_decodes(fs, frac, carrier, sigma)
                    assert clean, (fs, frac, carrier, sigma)
                    if frac == 0.0 or fs >= 4e6:
                        assert every, (fs, frac, carrier, sigma)
                    else:
                        table[f"{fs / 1e6:g}|{frac}|{carrier:g}|{sigma}"] = every
                        share.append(every)
    print(f"off the grid at 2 - 2.5 MHz: {sum(share)} of {len(share)} cases decode all four frames")
    assert table == OFFGRID


@pytest.mark.parametrize("kind", ["noise", "voice"])
def test_two_seconds_without_a_squitter_keep_nothing(kind):
    fs, n = 2e6, 4_000_000
    rng = np.random.default_rng(11)
    z = 0.05 * (rng.normal(size=n) + 1j * rng.normal(size=n))
    if kind == "voice":
        t = np.arange(n) / fs
        z = 0.01 * z + 0.4 * (1.0 + 0.4 * np.sin(2 * np.pi * 700.0 * t) + 0.3 * np.sin(2 * np.pi * 1900.0 * t + 1.0)) * np.exp(2j * np.pi * 3e3 * t)
    out = M.decode(z.astype(np.complex64), fs)
    print(f"{kind}: {out['candidates']} of {out['flags'].size} positions pass the preamble rule ({out['candidates'] / out['flags'].size:.3e})")
    assert out["records"] == [] and out["messages"] == []


# ---- the plan ---------------------------------------------------------------------------------------------------------------


def test_plan_matches_the_oracle_and_refuses_other_rates():
    from iq_to_audio_amd import dsp_plan as P

    for fs in M.RATES + [2.2e6, 3.3e6, 7.77e6, 19.99e6]:
        got, want = P.plan_adsb(fs), M.plan(fs)
        assert (got.h, got.span, got.L, got.sps) == (want["h"], want["span"], want["L"], want["sps"])
        assert got.offsets.dtype == np.int32 and got.offsets.shape == (240,) and (got.offsets == want["o"]).all()
        assert got.span <= 2400 and 6 * got.h * 65535 < 2 ** 31
    assert (P.plan_adsb(2.5e6).offsets[:5] == [0, 1, 2, 4, 5]).all()  # 1.25, 3.75: rint; 2.5: half-even
    for fs in (1.99e6, 20.01e6):
        with pytest.raises(ValueError, match="--fs-ch"):
            P.plan_adsb(fs)


# ---- parse_frames -----------------------------------------------------------------------------------------------------------


def test_grouping_and_hits():
    fs = 4e6  # L = 4
    res = _parse_both(fs, [M.IDENT, M.IDENT, M.DF11, M.IDENT, M.IDENT, M.IDENT], [100, 101, 102, 104, 105, 110])
    assert [(m.raw, m.hits, m.time_s) for m in res.messages] == [(M.IDENT.hex(), 3, 100 / fs), (M.DF11.hex(), 1, 102 / fs), (M.IDENT.hex(), 1, 105 / fs),
                                                                  (M.IDENT.hex(), 1, 110 / fs)]
    assert res.messages[1].type_code is None and res.messages[1].line() == "ADS-B 4840D6 DF11"
    assert res.messages[0].level == 100_000 / (4.0 * 2 * 65536.0)
    # unsorted input, numpy arrays
    rec, _ = _records([M.IDENT, M.IDENT], [9, 8])
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.decoders import adsb as AD

    one = AD.parse_frames(P.plan_adsb(fs), {k: np.asarray(v) for k, v in rec.items()})
    assert len(one.messages) == 1 and one.messages[0].hits == 2 and one.messages[0].time_s == 8 / fs
    assert AD.parse_frames(P.plan_adsb(fs), _records([], [])[0]) is None


def test_pairing_window_and_nl_mismatch():
    fs = 2e6
    inside = _parse_both(fs, [M.POS_EVEN, M.POS_ODD], [0, int(10.0 * fs)]).messages
    assert inside[1].lat is not None
    outside = _parse_both(fs, [M.POS_EVEN, M.POS_ODD], [0, int(10.0 * fs) + 1]).messages
    assert outside[1].lat is None and outside[1].line() == "ADS-B 40621D pos odd 74158/50194 38000ft"
    # another aircraft's even message does not pair
    other = bytearray(M.POS_EVEN[:11])
    other[3] ^= 1
    alien = _parse_both(fs, [M.with_parity(bytes(other)), M.POS_ODD], [0, 500]).messages
    assert alien[1].lat is None
    # latitudes in different longitude zones: no position
    def pos(odd, lat_cpr, lon_cpr):
        return M.build_frame(17, 0xABCDEF, (11 << 51) | (0xC38 << 36) | (odd << 34) | (lat_cpr << 17) | lon_cpr)

    found = None
    for lat_o in range(0, 131072, 997):
        got = M.global_position((93000, 51372), (lat_o, 50194), True)
        if got is None:
            found = lat_o
            break
    assert found is not None
    mism = _parse_both(fs, [pos(0, 93000, 51372), pos(1, found, 50194)], [0, 500])
    assert mism.messages[1].lat is None and mism.aircraft[0]["lat"] is None and mism.aircraft[0]["altitude_ft"] == 38000


def test_none_fields_and_the_aircraft_table():
    fs = 2e6
    q0 = M.build_frame(17, 0x123456, (11 << 51) | (0xC28 << 36) | (93000 << 17) | 51372)  # Q = 0: no altitude
    tc20 = M.build_frame(18, 0x123456, (20 << 51) | (0xC38 << 36) | (1 << 34) | (74158 << 17) | 50194)  # GNSS height: altitude None
    zero_v = M.build_frame(17, 0x123456, (19 << 51) | (1 << 48))  # every V field zero
    sub2 = M.build_frame(17, 0x0000AB, (19 << 51) | (2 << 48) | (1 << 42) | (3 << 32) | (0 << 31) | (4 << 21) | (0 << 19) | (11 << 10))
    tc28 = M.build_frame(17, 0x0000AB, (28 << 51) | 12345)
    df19 = M.build_frame(19, 0x0000AB, (4 << 51) | 12345)
    assert M.syndrome(df19) == 0
    res = _parse_both(fs, [q0, tc20, zero_v, sub2, tc28, M.IDENT, M.DF11], [0, 300, 600, 900, 1200, 1500, 1800])
    m = res.messages
    assert (m[0].altitude_ft, m[0].lat_cpr, m[0].cpr_odd) == (None, 93000, 0)
    assert (m[1].df, m[1].type_code, m[1].altitude_ft, m[1].cpr_odd) == (18, 20, None, 1) and m[1].lat is not None
    assert (m[2].speed_kt, m[2].track_deg, m[2].vertical_rate_fpm) == (None, None, None)
    assert (m[3].speed_kt, m[3].track_deg, m[3].vertical_rate_fpm) == (float(np.hypot(-8, 12)), float(np.degrees(np.arctan2(-8, 12)) % 360), 640)
    assert (m[4].type_code, m[4].callsign, m[4].lat_cpr) == (28, None, None)
    assert [a["icao"] for a in res.aircraft] == ["0000AB", "123456", "4840D6"]
    assert res.aircraft[0] == dict(icao="0000AB", callsign=None, lat=None, lon=None, altitude_ft=None, speed_kt=m[3].speed_kt, track_deg=m[3].track_deg,
                                   vertical_rate_fpm=640, messages=2, first_s=900 / fs, last_s=1200 / fs)
    assert res.aircraft[1]["lat"] == m[1].lat and res.aircraft[1]["messages"] == 3
    assert res.aircraft[2]["callsign"] == "KLM1023" and res.aircraft[2]["messages"] == 2 and res.aircraft[2]["last_s"] == 1800 / fs
    assert json.loads(json.dumps(res.to_json()))["messages"][5]["callsign"] == "KLM1023"
    assert M.nl(0) == 59 and M.nl(87) == 2 and M.nl(87.5) == 1 and M.nl(-52.3) == M.nl(52.3) == 36


# ---- the surface ----------------------------------------------------------------------------------------------------------


def test_cli_usage_errors_and_defaults(tmp_path, capsys):
    from iq_to_audio_amd import cli

    for mode in ("nfm", "usb", "wfm", "none"):
        with pytest.raises(SystemExit) as exc:
            cli.main(["--in", str(tmp_path / "x.wav"), "--ft", "1e6", "--adsb", "--demod", mode])
        assert exc.value.code == 2 and "--adsb needs --demod am" in capsys.readouterr().err
    with pytest.raises(SystemExit) as exc:
        cli.main(["--in", str(tmp_path / "x.wav"), "--ft", "1e6", "--adsb"])  # (the default --demod is nfm)
    assert exc.value.code == 2 and "--adsb needs --demod am" in capsys.readouterr().err
    parse = lambda *argv: cli.resolve_mode_defaults(cli.build_parser().parse_args(["--in", "x.wav", *argv]))
    a = parse("--demod", "am", "--adsb")
    assert a.adsb and (a.bandwidth, a.fs_ch) == (2_000_000.0, 2_000_000.0)
    a = parse("--demod", "am", "--adsb", "--bw", "3e6", "--fs-ch", "4e6")
    assert (a.bandwidth, a.fs_ch) == (3e6, 4e6)
    a = parse("--demod", "am")
    assert not a.adsb and (a.bandwidth, a.fs_ch) == (12_500.0, 96_000.0)
    a = parse("--demod", "am", "--acars")
    assert (a.bandwidth, a.fs_ch) == (12_500.0, 96_000.0)


def test_pipelines_take_the_flag_and_check_the_mode(tmp_path):
    import iq_to_audio_amd as A
    from iq_to_audio_amd import batch

    am = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="am")
    nfm = A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode="nfm")
    assert A.ProcessingPipeline(am, adsb=True).adsb_enabled and not A.ProcessingPipeline(am).adsb_enabled
    assert all(o.adsb_enabled for o in A.MultiChannelPipeline([am, am], adsb=True).owners)
    for make in (lambda: A.ProcessingPipeline(nfm, adsb=True), lambda: A.MultiChannelPipeline([am, nfm], adsb=True)):
        with pytest.raises(ValueError, match="--demod am"):
            make()
    with pytest.raises(ValueError, match="adsb"):
        batch.reject_side_decoders(adsb=True)
    batch.reject_side_decoders(adsb=False)
    assert len(A.ProcessingConfig.__dataclass_fields__) == 23
