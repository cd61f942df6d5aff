"""The side-decoder table (decoders/side.py), the host side: the mode errors and the batch runners' rejection character for
character as they were before the table existed (the strings below are literals copied from that code), the table's names
against the CLI's flags and the constructors' keywords, the table's order, and ``group_records`` against the grouping loop
the four decoder modules used to repeat.  No GPU compute."""
from __future__ import annotations

import inspect

import numpy as np
import pytest

import iq_to_audio_amd as A
from iq_to_audio_amd import batch, cli
from iq_to_audio_amd.decoders.common import group_records
from iq_to_audio_amd.decoders.side import SIDE_DECODERS, check_modes
from iq_to_audio_amd.processing import ChannelDemod

#: name -> (a mode it accepts, a mode it refuses, the singular error, the plural error): literals of the code before the table
MODE_ERRORS = {
    "rds": ("wfm", "nfm", "rds=True needs a wfm target: RDS rides on a broadcast FM multiplex (--demod wfm)",
            "rds=True needs wfm targets: RDS rides on a broadcast FM multiplex (--demod wfm)"),
    "pocsag": ("nfm", "am", "pocsag=True needs an nfm target: POCSAG is 2-FSK on a narrowband FM channel (--demod nfm)",
               "pocsag=True needs nfm targets: POCSAG is 2-FSK on a narrowband FM channel (--demod nfm)"),
    "ax25": ("nfm", "am", "ax25=True needs an nfm target: AX.25 here is Bell-202 AFSK on a narrowband FM channel (--demod nfm)",
             "ax25=True needs nfm targets: AX.25 here is Bell-202 AFSK on a narrowband FM channel (--demod nfm)"),
    "tones": ("nfm", "usb", "tones=True needs an nfm target: CTCSS and DTMF ride on a narrowband FM voice channel (--demod nfm)",
              "tones=True needs nfm targets: CTCSS and DTMF ride on a narrowband FM voice channel (--demod nfm)"),
    "acars": ("am", "nfm", "acars=True needs an am target: ACARS is audio MSK on an AM airband carrier (--demod am)",
              "acars=True needs am targets: ACARS is audio MSK on an AM airband carrier (--demod am)"),
    "ais": ("nfm", "wfm", "ais=True needs an nfm target: AIS is 9600 bit/s GMSK on a narrowband FM channel (--demod nfm)",
            "ais=True needs nfm targets: AIS is 9600 bit/s GMSK on a narrowband FM channel (--demod nfm)"),
    "adsb": ("am", "fm", "adsb=True needs an am target: Mode S squitters are pulses on a 1090 MHz AM channel (--demod am)",
             "adsb=True needs am targets: Mode S squitters are pulses on a 1090 MHz AM channel (--demod am)"),
}
REJECTED = "{}=True is not supported by the resident batch runners or sharded runs: use ProcessingPipeline / MultiChannelPipeline"
ORDER = ("rds", "pocsag", "ax25", "tones", "acars", "ais", "adsb")  # rds, then the order of a block's launches


def _raises_exactly(text, fn, *args, **kwargs):
    with pytest.raises(ValueError) as exc:
        fn(*args, **kwargs)
    assert str(exc.value) == text


def _config(tmp_path, mode):
    return A.ProcessingConfig(in_path=tmp_path / "x.wav", target_freq=1e6, demod_mode=mode)


def test_table_rows_and_order():
    assert tuple(e.name for e in SIDE_DECODERS) == ORDER == tuple(MODE_ERRORS)
    assert [e.section for e in SIDE_DECODERS] == list(range(11, 18))
    assert {e.name: e.source for e in SIDE_DECODERS} == dict(rds=None, pocsag="theta", ax25="theta", tones="theta", acars="envelope",
                                                             ais="theta", adsb="envelope")
    assert {e.name: e.mode for e in SIDE_DECODERS} == {name: row[0] for name, row in MODE_ERRORS.items()}
    with pytest.raises(Exception):  # frozen rows
        SIDE_DECODERS[0].name = "other"
    assert len(A.ProcessingConfig.__dataclass_fields__) == 23


@pytest.mark.parametrize("name", ORDER)
def test_mode_errors_are_the_old_strings(name, tmp_path):
    good, bad, singular, plural = MODE_ERRORS[name]
    _raises_exactly(singular, check_modes, {name: True}, [bad], plural=False)
    _raises_exactly(plural, check_modes, {name: True}, [good, bad], plural=True)
    _raises_exactly(singular, check_modes, {name: True}, [None], plural=False)
    check_modes({name: True}, [good, good.upper()], plural=True)
    check_modes({name: False}, [bad], plural=False)
    if good == "nfm":
        check_modes({name: True}, ["fm"], plural=False)  # nfm's other spelling, as the constructors took it
    # the constructors raise them: before anything touches a device or the file
    _raises_exactly(singular, A.ProcessingPipeline, _config(tmp_path, bad), **{name: True})
    _raises_exactly(plural, A.MultiChannelPipeline, [_config(tmp_path, good), _config(tmp_path, bad)], **{name: True})
    pipe = A.ProcessingPipeline(_config(tmp_path, good), **{name: True})
    assert getattr(pipe, name + "_enabled") is True and getattr(pipe, name) is None and pipe.side_enabled == {name: True}
    multi = A.MultiChannelPipeline([_config(tmp_path, good)] * 2, **{name: True})
    assert getattr(multi, name) is None and all(o.side_enabled == {name: True} for o in multi.owners)
    assert A.ProcessingPipeline(_config(tmp_path, good)).side_enabled == {}


@pytest.mark.parametrize("name", ORDER[1:])
def test_batch_rejection_is_the_old_string(name):
    _raises_exactly(REJECTED.format(name), batch.reject_side_decoders, **{name: True})
    _raises_exactly(REJECTED.format(name), batch.ResidentBankRunner, [dict(freq_offset=25e3)], sample_rate=2.5e6, n_frames=1 << 20,
                    **{name: True})
    _raises_exactly(REJECTED.format(name), batch.demodulate_sharded, [dict(freq_offset=25e3)], sample_rate=2.5e6, n_frames=1 << 20,
                    axis="channels", **{name: True})
    _raises_exactly(REJECTED.format(name), batch.ResidentCaptureRunner, np.ones(8), sample_rate=2.5e6, freq_offset=25e3, decimation=26,
                    fs_channel=2.5e6 / 26, chunk=1 << 20, n_frames=1 << 20, **{name: True})


def test_batch_rejection_returns_for_all_false():
    assert batch.reject_side_decoders() is None
    assert batch.reject_side_decoders(**{name: False for name in ORDER}) is None


def _flag_keywords(fn) -> set:
    """The keyword-only parameters of ``fn`` that default to False: its flags."""
    return {k for k, p in inspect.signature(fn).parameters.items() if p.kind is p.KEYWORD_ONLY and p.default is False}


def test_names_are_the_cli_flags_and_the_keywords(capsys):
    names = set(ORDER)
    parser = cli.build_parser()
    decoder_flags = {a.dest for a in parser._actions if a.option_strings == [f"--{a.dest}"] and a.const is True and a.dest in names}
    assert decoder_flags == names
    for e in SIDE_DECODERS:  # the help texts moved into the table verbatim
        assert [a.help for a in parser._actions if a.dest == e.name] == [e.help] and e.help.startswith(f"With --demod {e.mode}: ")
        assert f"<output stem>.{e.name}.json" in e.help
        with pytest.raises(SystemExit) as exc:
            cli.main(["--in", "x.wav", "--ft", "1e6", f"--{e.name}", "--demod", "usb"])
        assert exc.value.code == 2 and f"--{e.name} needs --demod {e.mode}." in capsys.readouterr().err
    for fn in (A.ProcessingPipeline.__init__, A.MultiChannelPipeline.__init__):
        assert _flag_keywords(fn) == names
    for fn in (ChannelDemod.__init__, batch.ResidentCaptureRunner.__init__, batch.ResidentBankRunner.__init__, batch.demodulate_sharded):
        assert _flag_keywords(fn) & (names | {"rds"}) == names - {"rds"}


def _old_groups(start, tie, nbytes, data, reach) -> list:
    """The loop ax25.py, acars.py and ais.py held before ``group_records`` (adsb.py: the same without a tie-break key)."""

    def group_of(groups, raw, at):
        for grp in reversed(groups):
            if at - grp[0] > reach:
                return None
            if grp[1] == raw:
                return grp
        return None

    groups: list = []
    for k in np.lexsort((tie, start)).tolist():
        raw, at = data[k, : int(nbytes[k])].tobytes(), int(start[k])
        grp = group_of(groups, raw, at)
        if grp is None:
            groups.append([at, raw, 1])
        else:
            grp[2] += 1
    return groups


def test_group_records_matches_the_old_loop():
    reach = 80
    frame_a, frame_b = b"\x10\x20\x30\x40", b"\x10\x20\x30"  # (b: a prefix of a -- the length decides, not the row)
    recs = [  # (start, tie-break key, bytes), deliberately out of order
        (1000, 3, frame_a),
        (1080, 0, frame_a),  # a duplicate inside the reach (1080 - 1000 == reach): joins the group that opened at 1000
        (1081, 1, frame_a),  # just outside it: a group of its own ...
        (1100, 2, frame_a),  # ... which this one joins (the LATEST group with these bytes; 1000 is out of reach anyway)
        (1000, 1, frame_b),  # equal start instants, different keys and bytes: walked by key
        (1000, 2, frame_a),
        (1000, 0, frame_b),
        (5000, 0, frame_b),  # far behind everything
    ]
    start = np.array([r[0] for r in recs], dtype=np.int64)
    tie = np.array([r[1] for r in recs], dtype=np.int64)
    nbytes = np.array([len(r[2]) for r in recs], dtype=np.int64)
    data = np.zeros((len(recs), 6), dtype=np.uint8)
    for k, r in enumerate(recs):
        data[k, : len(r[2])] = np.frombuffer(r[2], dtype=np.uint8)
        data[k, len(r[2]) :] = 0xEE  # (bytes behind a record's length never count)
    old = _old_groups(start, tie, nbytes, data, reach)
    new = group_records(start, nbytes, data, reach, tie=tie)
    assert [g[:3] for g in new] == old
    assert old == [[1000, frame_b, 2], [1000, frame_a, 3], [1081, frame_a, 2], [5000, frame_b, 1]]
    assert [recs[g[3]][:2] for g in new] == [(1000, 0), (1000, 2), (1081, 1), (5000, 0)]  # the first record of each
    # without a key (adsb): ties in the order given
    plain = group_records(start, nbytes, data, reach)
    assert [g[:3] for g in plain] == _old_groups(start, np.arange(len(recs)), nbytes, data, reach)
    assert group_records(start[:0], nbytes[:0], data[:0], reach) == []
