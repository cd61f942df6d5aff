"""What the side decoders launch, as a trace of ``_native.call``: per block and target the calls of the table in
``decoders/side.py`` in table order behind the demodulator's, every NFM decoder with a ``prev`` of its own that it keeps
for the whole run, every entry given the block's output count, the finishes in the same order, and nothing at all with no
flag set.  Written against constructor keywords, result attributes and ``_native.call`` only, so that the expected
sequence is a property of the pipelines and not of how they are wired inside."""
from __future__ import annotations

import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIDE_PREFIXES = ("iqa_pocsag_", "iqa_afsk_", "iqa_tones_", "iqa_acars_", "iqa_ais_", "iqa_adsb_")
DEMOD = ("iqa_demodulate", "iqa_demodulate_from_reset")
PER_BLOCK = {"iqa_pocsag_integrate", "iqa_afsk_correlate", "iqa_tones_decimate", "iqa_ais_filter", "iqa_adsb_quantise"}
#: the NFM decoders' calls of one block and target behind the demodulator's, in table order
NFM_BLOCK = ["iqa_quadrature", "iqa_pocsag_integrate", "iqa_quadrature", "iqa_afsk_correlate", "iqa_quadrature", "iqa_tones_decimate",
             "iqa_quadrature", "iqa_ais_filter"]
#: one target's finish in table order; a search is repeated once where its first list was too short (POCSAG: one search per
#: baud rate the plan runs), and the codewords are read once per baud rate that kept a sync -- that much depends on the data
NFM_FINISH = (r"(iqa_pocsag_sync ){1,6}(iqa_pocsag_codewords ){0,3}"
              r"iqa_afsk_bits iqa_afsk_frames (iqa_afsk_frames )?"
              r"iqa_tones_bank iqa_tones_bank iqa_tones_decide "
              r"iqa_ais_symbols iqa_ais_frames (iqa_ais_frames )?")


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _value(arg):
    return getattr(arg, "value", None)


@pytest.fixture()
def trace(monkeypatch):
    """[(name, argument values)] of every demodulator, discriminator, envelope and side-decoder entry, in call order."""
    from iq_to_audio_amd import _native

    calls = []
    real = _native.call

    def recording(name, *args):
        if name in DEMOD or name in ("iqa_quadrature", "iqa_envelope") or name.startswith(SIDE_PREFIXES):
            calls.append(("iqa_demodulate" if name in DEMOD else name, [_value(a) for a in args]))
        return real(name, *args)

    monkeypatch.setattr(_native, "call", recording)
    return calls


def _noise_capture(path, fs: float, frames: int, seed: int) -> None:
    from iq_to_audio_amd import iqio

    rng = np.random.default_rng(seed)
    iqio.write_wav_iq(path, rng.integers(-6000, 6001, size=2 * frames, dtype=np.int16), int(fs), "s16")


def _run(A, tmp_path, tag, *, fs, fc, frames, block, offsets, mode, flags, **cfg):
    wav = tmp_path / f"noise_{int(fc)}Hz.wav"
    if not wav.exists():
        _noise_capture(wav, fs, frames, seed=5)
    cfgs = [A.ProcessingConfig(in_path=wav, target_freq=fc + off, demod_mode=mode, chunk_size=65_536, output_path=tmp_path / f"{tag}{i}.wav",
                               **cfg) for i, off in enumerate(offsets)]
    multi = A.MultiChannelPipeline(cfgs, **flags)
    for o in multi.owners:
        o.block_frames_target = block
    results = multi.run()
    return multi, results


def _blocks(calls, per_block: list, targets: int):
    """Split the trace's block phase into [(block, target)] -> the calls of one demodulator call and what follows it; returns
    (those groups in order, the index where the finish phase begins)."""
    last = max(i for i, (name, _) in enumerate(calls) if name == "iqa_demodulate")
    end = last + 1 + len(per_block)
    names = [name for name, _ in calls[:end]]
    step = 1 + len(per_block)
    assert end % (step * targets) == 0 and names == (["iqa_demodulate"] + per_block) * (end // step)
    return [calls[i : i + step] for i in range(0, end, step)], end


def test_nfm_four_decoders_two_targets(A, tmp_path, trace):
    fs, fc = 2.4e6, 455.5e6
    chunk = 1_048_576  # what a 65 536 request becomes at 2.4 MS/s: a block is a whole number of chunks
    frames = 2 * chunk + 400_000  # three blocks, the last one shorter; 1.04 s: one CTCSS frame (0.4 s) at least
    decim = 25
    plain, _ = _run(A, tmp_path, "p", fs=fs, fc=fc, frames=frames, block=chunk, offsets=(300e3, -500e3), mode="nfm", flags={})
    assert [name for name, _ in trace] == ["iqa_demodulate"] * 6  # no side entry, no discriminator, no envelope
    assert plain.pocsag == plain.ax25 == plain.tones == plain.ais == [None, None]
    del trace[:]

    flags = dict(pocsag=True, ax25=True, tones=True, ais=True)
    multi, results = _run(A, tmp_path, "m", fs=fs, fc=fc, frames=frames, block=chunk, offsets=(300e3, -500e3), mode="nfm", flags=flags)
    assert [r.fs_channel for r in results] == [96_000.0] * 2 and [r.decimation for r in results] == [decim] * 2
    groups, end = _blocks(trace, NFM_BLOCK, targets=2)
    assert len(groups) == 3 * 2  # block-major, the targets in their order inside a block

    # every side entry is given the block's output count, and the blocks add up to the run
    counts = [g[0][1][2] for g in groups]  # iqa_demodulate(params, z, n, ...)
    assert counts[0::2] == counts[1::2] and min(counts[0], counts[2]) > counts[4] > 0 and sum(counts[0::2]) == -(-frames // decim)
    for g, n in zip(groups, counts):
        assert [args[1] for _, args in g[1:]] == [n] * len(NFM_BLOCK)

    # iqa_quadrature(z, n, prev, theta, stream): four prevs per target, each the same in every block, all eight distinct
    prevs = [[args[2] for name, args in g if name == "iqa_quadrature"] for g in groups]
    assert all(len(p) == 4 and None not in p and 0 not in p for p in prevs)
    assert prevs[0] == prevs[2] == prevs[4] and prevs[1] == prevs[3] == prevs[5]
    assert len(set(prevs[0]) | set(prevs[1])) == 8
    # ... reads the block the demodulator read, and writes a buffer of its own that the decoder's launch then reads
    for g in groups:
        z, audio = g[0][1][1], g[0][1][8]
        thetas = [args[3] for name, args in g if name == "iqa_quadrature"]
        assert all(args[0] == z for name, args in g if name == "iqa_quadrature")
        assert audio not in thetas
        assert [args[0] for name, args in g if name in PER_BLOCK] == thetas

    # the finishes: target by target, each in table order
    finish = " ".join(name for name, _ in trace[end:]) + " "
    assert re.fullmatch(f"({NFM_FINISH}){{2}}", finish), finish
    assert not any(name in ("iqa_quadrature", "iqa_envelope", "iqa_demodulate") or name in PER_BLOCK for name, _ in trace[end:])
    assert all(len(getattr(multi, name)) == 2 for name in flags)
    assert all(getattr(multi, name)[0] is getattr(multi.owners[0], name) for name in flags)


def test_am_acars(A, tmp_path, trace):
    fs, fc = 960e3, 131.5e6
    chunk = 262_144  # a 65 536 request at 960 kS/s
    frames = 2 * chunk + 100_000
    multi, results = _run(A, tmp_path, "a", fs=fs, fc=fc, frames=frames, block=chunk, offsets=(100e3,), mode="am", flags=dict(acars=True))
    assert results[0].fs_channel == 96_000.0
    groups, end = _blocks(trace, ["iqa_envelope"], targets=1)
    assert len(groups) == 3
    for (_, dem), (_, env) in groups:  # iqa_demodulate(params, z, n, state, starts, n_chunks, peak, sumsq, out, ...); iqa_envelope(z, n, e, stream)
        n, audio = dem[2], dem[8]
        assert env[0] == dem[1] and env[1] == n and not audio <= env[2] < audio + 4 * n  # never the audio slice
    assert sum(dem[2] for (_, dem), _ in groups) == -(-frames // 10)
    finish = [name for name, _ in trace[end:]]  # no ACARS entry point before the finish; there, the maximum comes first
    assert finish and finish[0] == "iqa_acars_max" and all(name.startswith("iqa_acars_") for name in finish)
    assert not any(name.startswith("iqa_acars_") for name, _ in trace[:end])
    assert len(multi.acars) == 1 and multi.acars[0] is multi.owners[0].acars


def test_am_adsb(A, tmp_path, trace):
    fs, fc = 4e6, 1089.5e6
    chunk = 2_097_152  # a 65 536 request at 4 MS/s
    frames = 2 * chunk + 300_000
    multi, results = _run(A, tmp_path, "s", fs=fs, fc=fc, frames=frames, block=chunk, offsets=(0.5e6,), mode="am", flags=dict(adsb=True),
                          bandwidth=2e6, fs_ch_target=2e6)
    assert results[0].fs_channel == 2e6
    groups, end = _blocks(trace, ["iqa_envelope", "iqa_adsb_quantise"], targets=1)
    assert len(groups) == 3
    for (_, dem), (_, env), (_, quant) in groups:  # iqa_adsb_quantise(e, n, q, stream)
        n, audio = dem[2], dem[8]
        assert env[0] == dem[1] and env[1] == quant[1] == n and quant[0] == env[2] and not audio <= env[2] < audio + 4 * n
    assert sum(dem[2] for (_, dem), _, _ in groups) == -(-frames // 2)
    finish = [name for name, _ in trace[end:]]
    assert finish in (["iqa_adsb_search"], ["iqa_adsb_search"] * 2)  # (twice where the first list was too short)
    assert len(multi.adsb) == 1 and multi.adsb[0] is multi.owners[0].adsb
