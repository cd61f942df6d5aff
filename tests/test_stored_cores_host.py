"""What the side decoders' parsers and ``stages()`` share (``decoders/common.py``: ``parse_head``, ``stage_records``) and the
JSON mixin of the protocol layers' results (``protocol_layer.JsonRecord``), on plain numpy arrays and dataclasses: the expected
values are written out by hand.  No GPU compute."""
from __future__ import annotations

import json

import numpy as np

from iq_to_audio_amd import dmr as DM
from iq_to_audio_amd import flex as FX
from iq_to_audio_amd.decoders import common as C
from iq_to_audio_amd.decoders.acars import AcarsResult
from iq_to_audio_amd.decoders.ax25 import Ax25Result

SLOT = 8
ROWS = np.array([[0x10, 0x11, 0xEE, 0xEE, 0xEE, 0xEE, 0xEE, 0xEE],
                 [0x20, 0x21, 0x22, 0x23, 0x24, 0xEE, 0xEE, 0xEE],
                 [0x30, 0x31, 0x32, 0xEE, 0xEE, 0xEE, 0xEE, 0xEE]], dtype=np.uint8)  # 0xEE: what a slot holds behind its frame
THREE = dict(phase=[1, 0, 0], s=[4, 9, 2], start=[300, 100, 200], nbytes=[2, 5, 3], data=ROWS)  # in no order


def _first(records: dict, k: int) -> dict:
    return {key: np.asarray(col)[:k] for key, col in records.items()}


def test_parse_head_of_no_record():
    for data in (np.zeros((0, SLOT), dtype=np.uint8), [], np.zeros(0, dtype=np.uint8)):
        res, start, phase, nbytes, got = C.parse_head(AcarsResult, dict(start=[], phase=[], nbytes=[], data=data), 5, "start", "phase", "nbytes")
        assert res == AcarsResult(messages=[], candidates=5, crc_ok=0)
        for col in (start, phase, nbytes):
            assert col.shape == (0,) and col.dtype == np.int64
        assert got.shape == (0, 0) and got.dtype == np.uint8


def test_parse_head_of_one_and_of_three_records():
    res, start, variant, nbytes, data = C.parse_head(Ax25Result, dict(_first(THREE, 1), variant=[23]), 2, "start", "variant", "nbytes")
    assert res == Ax25Result(frames=[], candidates=2, crc_ok=1, rejected=0)
    assert (start.tolist(), variant.tolist(), nbytes.tolist()) == ([300], [23], [2])
    assert data.shape == (1, SLOT) and data.tobytes() == ROWS[0].tobytes()
    # lists, a flat data plane and a numpy count: what the callers hand in
    flat = dict(THREE, start=tuple(THREE["start"]), nbytes=np.array(THREE["nbytes"], dtype=np.int32), data=ROWS.reshape(-1).tolist())
    for records in (THREE, flat):
        res, start, phase, nbytes, data = C.parse_head(AcarsResult, records, np.int64(7), "start", "phase", "nbytes")
        assert res == AcarsResult(messages=[], candidates=7, crc_ok=3) and type(res.candidates) is int and type(res.crc_ok) is int
        assert (start.tolist(), phase.tolist(), nbytes.tolist()) == ([300, 100, 200], [1, 0, 0], [2, 5, 3])  # as given: nothing is sorted
        assert all(col.dtype == np.int64 and col.shape == (3,) for col in (start, phase, nbytes))
        assert data.dtype == np.uint8 and data.shape == (3, SLOT) and np.array_equal(data, ROWS)
    # the names are the caller's (ADS-B: n, nbits, P)
    res, at, nbits, level, data = C.parse_head(AcarsResult, dict(n=[9, 3], nbits=[112, 56], P=[70000, 5], data=ROWS[:2]), 0, "n", "nbits", "P")
    assert (at.tolist(), nbits.tolist(), level.tolist(), res.crc_ok, data.shape) == ([9, 3], [112, 56], [70000, 5], 2, (2, SLOT))


def test_stage_records():
    empty = dict(phase=np.zeros(0, np.int64), s=np.zeros(0, np.int64), start=np.zeros(0, np.int64), nbytes=np.zeros(0, np.int64),
                 data=np.zeros((0, SLOT), np.uint8))
    assert C.stage_records(empty, "phase") == []
    fin = {key: np.asarray(col) for key, col in THREE.items()}
    want = [(1, 4, 300, b"\x10\x11"), (0, 9, 100, b"\x20\x21\x22\x23\x24"), (0, 2, 200, b"\x30\x31\x32")]
    assert C.stage_records(_first(fin, 1), "phase") == want[:1]
    got = C.stage_records(fin, "phase")
    assert got == want and all(type(v) is int for rec in got for v in rec[:3])
    assert C.stage_records(dict(fin, variant=fin["phase"] + 8), "variant") == [(p + 8, s, at, raw) for p, s, at, raw in want]


PAGE_KEYS = ["time_s", "cycle", "frame", "phase", "mode", "inverted", "capcode", "long", "kind", "text", "words", "corrected", "damaged",
             "fragment", "more"]
FLEX_CHANNEL_KEYS = ["offset_hz", "freq_hz", "frames", "unknown_mode", "no_level", "fiw_failed", "biw_lost", "biw_bad", "vectors_dropped",
                     "words", "shifts", "pages", "note"]
CALL_KEYS = ["start_s", "end_s", "slot", "cc", "group", "src", "dst", "superframes", "terminated"]
BURST_KEYS = ["time_s", "kind", "slot", "cc", "data_type", "type_name", "checked", "corrected", "flco", "fid", "src", "dst", "csbko", "hex"]
DMR_CHANNEL_KEYS = ["offset_hz", "freq_hz", "kinds", "no_level", "cut", "slot_refused", "bptc_failed", "check_failed", "tact_fixed", "idle",
                    "calls", "bursts", "note"]
RESULT_KEYS = ["channels", "sample_rate", "center_freq"]


def test_flex_result_json_round_trip():
    page = FX.FlexPage(time_s=1.875, cycle=3, frame=17, phase="A", mode="1600/2", inverted=False, capcode=1234567, long=False,
                       kind="alpha", text="HELLO", words=["0012d687", "00001234"], corrected=1, damaged=False, fragment=3, more=False)
    ch = FX.FlexChannel(offset_hz=-12500.0, freq_hz=929_612_500.0, frames={"1600/2": 1}, words={"0": 87, "1": 1}, shifts={"0": 11},
                        pages=[page])
    x = FX.FlexResult(channels=[ch], sample_rate=2_400_000.0, center_freq=929_625_000.0)
    data = x.to_json()
    assert list(data) == RESULT_KEYS and list(data["channels"][0]) == FLEX_CHANNEL_KEYS and list(data["channels"][0]["pages"][0]) == PAGE_KEYS
    assert data["channels"][0]["pages"][0] == page.to_json() and type(data["channels"][0]["pages"][0]) is dict
    back = FX.FlexResult.from_json(json.loads(json.dumps(data)))
    assert back == x and type(back.channels[0]) is FX.FlexChannel and type(back.channels[0].pages[0]) is FX.FlexPage
    assert back.lines() == x.lines() == ['929612500 Hz: FLEX 1600/2 03.017.A cap=1234567 alpha "HELLO"']
    assert FX.FlexResult.from_json({}) == FX.FlexResult() and FX.FlexChannel.from_json(dict(offset_hz=1.0, freq_hz=None)).pages == []
    assert FX.FlexChannel(offset_hz=-12500.0, freq_hz=None).label() == "-12500 Hz"


def test_dmr_result_json_round_trip():
    call = DM.DmrCall(start_s=0.5, end_s=1.22, slot=1, cc=7, group=True, src=1001, dst=91, superframes=2, terminated=True)
    burst = DM.DmrBurst(time_s=0.25, kind=1, slot=2, cc=7, data_type=3, type_name="csbk", checked=True, corrected=False, fid=0, csbko=0x3D,
                        hex="bd00" + "00" * 10)
    ch = DM.DmrChannel(offset_hz=6250.0, freq_hz=None, kinds={"bs data": 1}, idle=4, calls=[call], bursts=[burst])
    x = DM.DmrResult(channels=[ch], sample_rate=1_000_000.0)
    data = x.to_json()
    assert list(data) == RESULT_KEYS and list(data["channels"][0]) == DMR_CHANNEL_KEYS
    assert list(data["channels"][0]["calls"][0]) == CALL_KEYS and list(data["channels"][0]["bursts"][0]) == BURST_KEYS
    assert data["channels"][0]["calls"][0] == call.to_json() and data["channels"][0]["bursts"][0] == burst.to_json()
    back = DM.DmrResult.from_json(json.loads(json.dumps(data)))
    assert back == x and type(back.channels[0]) is DM.DmrChannel
    assert type(back.channels[0].calls[0]) is DM.DmrCall and type(back.channels[0].bursts[0]) is DM.DmrBurst
    assert back.lines() == x.lines() == ["+6250 Hz: DMR cc=7 ts=2 csbk o=0x3d fid=0x00 0000000000000000",
                                         "+6250 Hz: DMR cc=7 ts=1 group 1001 -> 91 0.72 s (2 superframes)"]
    assert DM.DmrResult.from_json({}) == DM.DmrResult()
