"""float32 captures as int16 planes: the two conversion kernels against a numpy statement of their arithmetic, and the
pipeline's per-block choice (one plane / two planes / float32 fallback) across block transitions, pinned output by
output.

``iqa_f32_split_s16`` (S = 2^(15 - shift)): hi = rint(S x), lo = rint(32768 (S x - hi)), both in float32 with ties to
even; flag bit 0 when hi is outside [-32768, 32767] or x is a NaN, bit 1 when some lo != 0.  ``iqa_f32_to_s16_exact``:
the int16 copy x * 32768, flag 1 when some value is not k / 32768 with k in int16 range.

The pipeline forms z = 2^shift (z(hi) + 2^-15 z(lo)) block by block; the low plane's channelizers carry their own L-1
frames of history, which reach the first (L-1)/D outputs of the NEXT block even when that block's own low plane is all
zeros.  The structural oracle here runs both planes through independently built int16 channelizers on every block; its
"history dropped" twin is what a pipeline that skips the low plane of such blocks would give.
"""
from __future__ import annotations

import time

import numpy as np
import pytest

from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


# ---- the conversion kernels ------------------------------------------------------------------------------------------

GRID_PASS = 256 * 16 * 256 * 4  # values one grid-stride pass of either kernel covers (4096 blocks x 256 threads x float4)
SHIFTS = (0, 1, 3, 8, 15)
LENGTHS = (1, 2, 3, 4, 5, 7, 1023, GRID_PASS + 6)


def _f32(v) -> np.ndarray:
    return np.asarray(v, dtype=np.float32)


def ref_split(x: np.ndarray, shift: int):
    """(hi, lo, flag, accepted) of iqa_f32_split_s16, in float32 arithmetic as the kernel states it."""
    x = _f32(x)
    with np.errstate(invalid="ignore", over="ignore"):
        sc = x * np.float32(2.0 ** (15 - shift))
        h = np.rint(sc)
        lo = np.rint((sc - h) * np.float32(32768.0))
        ok = (h >= -32768.0) & (h <= 32767.0)  # (NaN: False)
    flag = (0 if ok.all() else 1) | (2 if np.any(lo != 0.0) else 0)  # (NaN != 0: True, as in the kernel)
    hi16 = np.where(ok, h, 0).astype(np.int16)
    lo16 = np.where(ok, lo, 0).astype(np.int16)
    return hi16, lo16, flag, ok


def ref_exact(x: np.ndarray):
    x = _f32(x)
    with np.errstate(invalid="ignore", over="ignore"):
        sc = x * np.float32(32768.0)
        r = np.rint(sc)
        ok = (r == sc) & (r >= -32768.0) & (r <= 32767.0)
    return np.where(ok, r, 0).astype(np.int16), (0 if ok.all() else 1), ok


def _dev_split(A, x: np.ndarray, shift: int):
    import torch

    xd = torch.from_numpy(_f32(x)).cuda()
    hi = torch.full((x.size,), 0x5a5a, dtype=torch.int16, device="cuda")
    lo = torch.full((x.size,), 0x5a5a, dtype=torch.int16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    N = A.native
    from ctypes import c_int32, c_int64

    N.call("iqa_f32_split_s16", N.ptr(xd), c_int64(x.size), c_int32(shift), N.ptr(hi), N.ptr(lo), N.ptr(flag), N.stream_ptr())
    return hi.cpu().numpy(), lo.cpu().numpy(), int(flag.item())


def _dev_exact(A, x: np.ndarray):
    import torch

    xd = torch.from_numpy(_f32(x)).cuda()
    out = torch.full((x.size,), 0x5a5a, dtype=torch.int16, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    N = A.native
    from ctypes import c_int64

    N.call("iqa_f32_to_s16_exact", N.ptr(xd), c_int64(x.size), N.ptr(out), N.ptr(flag), N.stream_ptr())
    return out.cpu().numpy(), int(flag.item())


def _edge_values(shift: int) -> list:
    """Values where a conversion can go wrong, for planes with ``shift`` bits of headroom."""
    up = np.float32(2.0 ** (shift - 15))  # x = sc * up, exact (a power of two, no value leaves the normal range)

    def at(sc):
        return _f32(sc) * up

    tiny = np.nextafter(np.float32(0), np.float32(1))
    vals = [0.0, -0.0, tiny, -tiny, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny, 1.0, -1.0, 1.0 - 2.0 ** -16,
            32767.0 / 32768.0, -32768.0 / 32768.0]
    for edge in (32767.5, -32768.5):  # hi's rounding boundaries: 32767.5 -> 32768 (out), -32768.5 -> -32768 (in)
        e = _f32(edge)
        vals += [at(e), at(np.nextafter(e, np.float32(np.inf))), at(np.nextafter(e, np.float32(-np.inf)))]
    vals += [at(32768.0), at(-32769.0)]  # one step outside, lo = 0: flag exactly 1
    # lo ties: (S x - hi) * 32768 = k + 1/2 rounds to even; hi ties: S x = m + 1/2 -> lo = +-16384
    for sc in (5 + 1 / 65536, 5 + 3 / 65536, -7 - 5 / 65536, 2.5, 3.5, -2.5, -3.5, 0.5, -0.5, 100 + 32767 / 65536,
               -100 - 32769 / 65536):
        vals.append(at(sc))
    vals += [np.nan, np.inf, -np.inf, 3.0e38, -3.0e38]
    return [np.float32(v) for v in vals]


def _random_fill(rng, n: int, shift: int) -> np.ndarray:
    """Uniform over the accepted range, plus a share of small magnitudes (log-uniform down to 2^-40)."""
    x = rng.uniform(-0.9999, 0.9999, n) * 2.0 ** shift
    small = rng.random(n) < 0.25
    x[small] = np.sign(x[small]) * 2.0 ** rng.uniform(-40, -0.01, int(small.sum())) * 2.0 ** shift
    return _f32(x)


def _check_split(A, x: np.ndarray, shift: int, label: str) -> int:
    hi, lo, flag = _dev_split(A, x, shift)
    rh, rl, rflag, ok = ref_split(x, shift)
    assert flag == rflag, (label, shift, flag, rflag)
    bad = np.flatnonzero(ok & ((hi != rh) | (lo != rl)))
    assert bad.size == 0, (label, shift, bad[:8], x[bad[:8]], hi[bad[:8]], rh[bad[:8]], lo[bad[:8]], rl[bad[:8]])
    # reconstruction of every accepted value, in float64
    rec = 2.0 ** shift * (hi[ok].astype(np.float64) + lo[ok].astype(np.float64) / 32768.0) / 32768.0
    err = np.abs(rec - x[ok].astype(np.float64))
    assert err.size == 0 or err.max() <= 2.0 ** (shift - 31), (label, shift, float(err.max()))
    assert np.all(np.abs(lo[ok].astype(np.int32)) <= 16384)
    return flag


@pytest.mark.parametrize("shift", SHIFTS)
def test_split_matches_numpy_bit_for_bit(A, shift):
    """Random fill at every length (vector body, the 1..3-value tail, a second grid-stride pass), and every edge value
    alone (in the vector body and in the tail) and all together: hi, lo bit-exact, the flag word exact."""
    rng = np.random.default_rng(100 + shift)
    for n in LENGTHS:
        x = _random_fill(rng, n, shift)
        assert _check_split(A, x, shift, f"random n={n}") in (0, 2)
    edges = _edge_values(shift)
    seen = set()
    for v in edges:
        for where in (0, 4):  # index 0: first float4; index 4 of 5 values: the tail
            x = np.zeros(5, np.float32)
            x[where] = v
            seen.add(_check_split(A, x, shift, f"edge {v!r} at {where}"))
    assert seen == {0, 1, 2, 3}  # every flag combination occurred
    x = _f32(np.concatenate([_random_fill(rng, 4096, shift), edges, _random_fill(rng, 3, shift)]))
    assert _check_split(A, x, shift, "edges together") == 3
    # the boundaries themselves, stated once more as the header states them
    e_hi, e_lo = _f32(32767.5) * np.float32(2.0 ** (shift - 15)), _f32(-32768.5) * np.float32(2.0 ** (shift - 15))
    assert _dev_split(A, np.full(4, e_hi), shift)[2] & 1 == 1  # rint(32767.5) = 32768: does not fit
    assert _dev_split(A, np.full(4, e_lo), shift)[2] & 1 == 0  # rint(-32768.5) = -32768: fits
    assert _dev_split(A, np.full(4, np.nextafter(e_lo, np.float32(-np.inf))), shift)[2] & 1 == 1


@pytest.mark.parametrize("shift", (0, 8))
def test_split_flags_one_bad_value_wherever_it_sits(A, shift):
    """A clean array (every value on the hi grid: flag 0) of one grid-stride pass + 6 values, with ONE value that does
    not fit (flag exactly 1) or ONE value with lo != 0 (flag exactly 2) placed in the tail, in the last lane of a wave,
    or where only the second grid-stride iteration reaches it."""
    rng = np.random.default_rng(7)
    n = GRID_PASS + 6
    clean = _f32(rng.integers(-32768, 32768, n) * 2.0 ** (shift - 15))
    assert _check_split(A, clean, shift, "clean") == 0
    places = {"tail": n - 1, "last lane of a wave": 4 * (7 * 256 + 191) + 3, "second grid-stride pass": GRID_PASS + 1}
    for where, i in places.items():
        for value, want in ((2.0 ** shift, 1), (np.nan, 3), (clean[i] + np.float32(2.0 ** (shift - 20)), 2)):
            x = clean.copy()
            x[i] = value
            assert _check_split(A, x, shift, where) == want, (where, value)


@pytest.mark.parametrize("n", LENGTHS)
def test_to_s16_exact_matches_numpy(A, n):
    """iqa_f32_to_s16_exact: a bit-exact copy of every k / 32768, flag 1 exactly when some value is not of that form
    (subnormals included: x * 32768 of one is not an integer, so it is flagged)."""
    rng = np.random.default_rng(n)
    k = rng.integers(-32768, 32768, n)
    x = _f32(k / 32768.0)
    out, flag = _dev_exact(A, x)
    assert flag == 0 and np.array_equal(out, k.astype(np.int16))
    for i in sorted({0, n // 2, n - 1}):  # one bad value: first float4 / body / tail (or second grid-stride pass)
        for v in (np.nextafter(x[i], np.float32(2)), np.float32(1.0), np.float32(np.nan), np.float32(1.4e-45)):
            if v == x[i]:
                continue
            y = x.copy()
            y[i] = v
            got, f = _dev_exact(A, y)
            want, rf, ok = ref_exact(y)
            assert f == rf == 1, (i, v)
            assert np.array_equal(got[ok], want[ok])
    if n == GRID_PASS + 6:
        y = x.copy()
        y[GRID_PASS + 2] = np.float32(0.3)
        assert _dev_exact(A, y)[1] == 1


def test_to_s16_exact_edge_values(A):
    for v in _edge_values(0):
        for where in (0, 4):
            x = np.zeros(5, np.float32)
            x[where] = v
            out, flag = _dev_exact(A, x)
            want, rflag, ok = ref_exact(x)
            assert flag == rflag, (v, where, flag, rflag)
            assert np.array_equal(out[ok], want[ok]), (v, where)
    assert _dev_exact(A, _f32([-1.0, 32767 / 32768, 0.0, -0.0, 1 / 32768]))[1] == 0
    assert _dev_exact(A, _f32([1.0]))[1] == 1 and _dev_exact(A, _f32([1.0 - 2.0 ** -16]))[1] == 1


# ---- the pipeline across block transitions -----------------------------------------------------------------------------

FS, FC = 2.5e6, 400e6
BLOCK = 1_048_576  # frames per device block (= one reference chunk at this rate)
TOL = 1e-7  # structural oracle: max |dz| on every output
LO_UNITS = 12_000.0  # in-band tone carried by an S block's low plane (below hi's half step: hi is the capture's k)


def _capture(kinds: list, ragged: int, offsets: list, shift1: bool) -> np.ndarray:
    """Interleaved float32 frames, one block per kind: I = k / 32768, S = (k + tone) / 32768 with an in-band tone of
    LO_UNITS / 32768 split over the targets (it lives in the low plane), Z = zeros, O = an I block with one value the
    planes cannot hold.  ``ragged``: frames of the last block when it is short.  ``shift1``: +-1.0 in the warm-up chunk."""
    lens = [BLOCK] * len(kinds)
    if ragged:
        lens[-1] = ragged
    total = sum(lens)
    s16 = O.synth_capture_s16(FS, total / FS, offsets[0]).astype(np.float64)
    assert s16.shape[0] == total
    t = np.arange(total) / FS
    tone = sum(LO_UNITS / 32768.0 / len(offsets) * np.exp(1j * (2 * np.pi * f * t + 0.3 * i)) for i, f in enumerate(offsets))
    x = np.empty((total, 2))
    pos = 0
    for kind, n in zip(kinds, lens):
        sl = slice(pos, pos + n)
        if kind == "Z":
            x[sl] = 0.0
        else:
            x[sl] = s16[sl]
            if kind == "S":
                x[sl, 0] += tone[sl].real
                x[sl, 1] += tone[sl].imag
        pos += n
    f32 = (x / 32768.0).astype(np.float32)
    pos = 0
    for kind, n in zip(kinds, lens):
        if kind == "O":
            f32[pos + n // 2, 0] = 4.0  # rint(4 * 2^(15 - shift)) > 32767 for shift <= 1
        pos += n
    if shift1:
        f32[5] = (1.0, -1.0)
    return f32.reshape(-1), lens


def _run(A, tmp_path, f32, specs, *, integer_path=True, tag="p"):
    src = tmp_path / f"{tag}_{int(FC)}Hz.cf32"
    src.write_bytes(f32.tobytes())
    cfgs = [A.ProcessingConfig(in_path=src, target_freq=FC + off, input_sample_rate=FS, fs_ch_target=fsch, demod_mode=mode,
                               mix_sign_override=1, output_path=tmp_path / f"{tag}{i}.wav", dump_iq_path=tmp_path / f"{tag}{i}.cf32")
            for i, (off, fsch, mode) in enumerate(specs)]
    multi = A.MultiChannelPipeline(cfgs)
    for o in multi.owners:
        o.block_frames_target = BLOCK
        o.keep_channel_audio = True
        o.f32_integer_path = integer_path
    multi.run()
    zs = [np.fromfile(c.dump_iq_path, dtype=np.complex64) for c in cfgs]
    return multi, zs


def _structural(A, f32, lens, shift, specs, precisions, n_blocks):
    """z of the first ``n_blocks`` blocks from both planes (numpy split at ``shift``), each through int16 channelizers built
    as the pipeline builds them (a ChannelBank per decimation and plane; hi at the target's precision, lo at "fast"),
    BOTH planes on every block -> (z, z with the low plane's history dropped, block starts in outputs) per target."""
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd import dsp_plan as P

    hi, lo, flag, _ = ref_split(f32, shift)
    assert not flag & 1 or n_blocks < len(lens)
    targets = []
    for (off, fsch, _), prec in zip(specs, precisions):
        d, _ = P.choose_decimation(FS, fsch)
        taps = A.design_channel_filter(FS, 12_500.0, d)
        mk = lambda p: A.Channelizer(taps, sample_rate=FS, freq_offset=off, mix_sign=1, decimation=d, fmt="s16", precision=p)  # noqa: E731
        targets.append((d, mk(prec), mk("fast")))
    banks = []
    for d in sorted({t[0] for t in targets}):
        idx = [i for i, t in enumerate(targets) if t[0] == d]
        banks.append((idx, A.ChannelBank([targets[i][1] for i in idx]), A.ChannelBank([targets[i][2] for i in idx])))
    z_ok = [[] for _ in targets]
    z_drop = [[] for _ in targets]
    pos = 0
    for b in range(n_blocks):
        sl = slice(2 * pos, 2 * (pos + lens[b]))
        lo_zero = not np.any(lo[sl])
        h_dev, l_dev = D.to_device(hi[sl], "int16"), D.to_device(lo[sl], "int16")
        for idx, bank_hi, bank_lo in banks:
            for i, zh, zl in zip(idx, bank_hi.process(h_dev), bank_lo.process(l_dev)):
                zh = zh.cpu().numpy().astype(np.complex128)
                zl = zl.cpu().numpy().astype(np.complex128)
                z_ok[i].append(2.0 ** shift * (zh + 2.0 ** -15 * zl))
                z_drop[i].append(2.0 ** shift * zh if lo_zero else z_ok[i][-1])
        pos += lens[b]
    starts = []
    for d, _, _ in targets:
        edges = np.cumsum([0] + list(lens))
        starts.append([-(-int(e) // d) for e in edges])
    return [np.concatenate(z) for z in z_ok], [np.concatenate(z) for z in z_drop], starts


def _rms(v) -> float:
    return float(np.sqrt(np.mean(np.abs(v) ** 2))) if np.size(v) else 0.0


NFM96, NFM48, USB96 = (25e3, 96_000.0, "nfm"), (-180e3, 48_000.0, "nfm"), (25e3, 96_000.0, "usb")

# name: (kinds, ragged last block, targets, shift1, (integer_blocks, split_blocks), fallback, history lost, float64 oracle)
SEQUENCES = {
    "S-S-I": (["S", "S", "I"], 0, [USB96, NFM96], False, (1, 2), False, True, True),
    "S-S-Z": (["S", "S", "Z"], 0, [USB96, NFM96], False, (1, 2), False, True, True),
    "I-S-I": (["I", "S", "I"], 0, [NFM96], False, (2, 1), False, True, False),
    "S-S-ragged": (["S", "S", "I"], 1000, [NFM96], False, (1, 2), False, True, False),
    "S-S-O": (["S", "S", "O"], 0, [NFM96], False, (0, 2), True, False, False),
    "shift1-S-S-Z": (["S", "S", "Z"], 0, [NFM96], True, (1, 2), False, True, False),
    "two-banks-I-S-Z-I": (["I", "S", "Z", "I"], 0, [USB96, (NFM48[0], NFM48[1], "usb"), NFM96], False, (3, 1), False, True, True),
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_float32_block_transitions_against_both_oracles(A, tmp_path, monkeypatch, name):
    """Each device block of a cf32 capture takes one plane, two planes or (from the first block the planes cannot hold
    on) the float32 kernel.  The run's z must be the structural oracle's on EVERY output (1e-7), the fallback blocks
    those of a float32-kernel run; the oracle's history-dropped twin must differ by >= 20x that at the block heads (the
    test can see the defect); and on some sequences the float64 chain: for a USB target with the AGC on (its hi plane at
    "full": z error below the float32 rounding of z) the first 64 outputs after each block boundary no worse than 3x the
    settled rest; for an NFM target at the same offset the audio within 2e-5 RMS (SSB audio with the AGC on is
    ill-conditioned in the reference itself: see processing.base_precision) -- outside Z blocks and the 2048 outputs after
    one: an all-zero block has no FM phase, the reference's discriminator sees exact zeros and the "fast" kernel its
    level-independent floor (MfmaPlan.floor_rms, ~1e-5 of full scale, turning with the mixer)."""
    from iq_to_audio_amd import processing as PR

    kinds, ragged, specs, shift1, counts, fallback, lost, f64 = SEQUENCES[name]
    t0 = time.perf_counter()
    if len({s[1] for s in specs}) > 1:  # (the D = 52 bank's 20 k outputs per block take the matrix cores too)
        monkeypatch.setattr(PR._ChannelKernel, "mfma_min_outputs", 16384)
    offsets = list(dict.fromkeys(s[0] for s in specs))
    f32, lens = _capture(kinds, ragged, offsets, shift1)
    multi, zs = _run(A, tmp_path, f32, specs)
    shift = multi.f32_shift
    assert shift == (1 if shift1 else 0)
    assert (multi.integer_blocks, multi.split_blocks) == counts
    kernels = [o.channelizer_kernel for o in multi.owners]
    if fallback or ragged:
        assert kernels == ["k_channelize_v1"] * len(specs), kernels
    else:
        assert all(k.startswith("k_channelize_mfma_s16") for k in kernels), kernels
    n_fb = next((b for b, k in enumerate(kinds) if k == "O"), len(kinds))
    precisions = [o.channelizer_precision for o in multi.owners]
    z_ok, z_drop, starts = _structural(A, f32, lens, shift, specs, precisions, n_fb)
    if fallback:
        _, zs32 = _run(A, tmp_path, f32, specs, integer_path=False, tag="f")
    report = []
    for ti, z in enumerate(zs):
        st = starts[ti]
        assert z.size == st[-1]
        dz = np.abs(z[: st[n_fb]] - z_ok[ti])
        assert dz.max() <= TOL, (name, ti, float(dz.max()), int(np.argmax(dz)))
        if fallback:
            d32 = np.abs(z[st[n_fb]:] - zs32[ti][st[n_fb]:])
            assert d32.max() <= TOL, (name, ti, float(d32.max()))
        heads = np.zeros(z.size, bool)
        for b in range(1, len(lens)):
            heads[st[b] : st[b] + 64] = True
        gap = np.abs(z_ok[ti] - z_drop[ti])
        teeth = float(gap.max())
        away = np.flatnonzero(~heads[: st[n_fb]] & (gap > 0))
        where = ", ".join(f"{int(i - st[np.searchsorted(st, i, 'right') - 1])}:{gap[i]:.1e}" for i in away[:4])
        if lost:
            assert teeth >= 20 * TOL, (name, ti, teeth)
            assert float(gap[~heads[: st[n_fb]]].max(initial=0.0)) < TOL, (name, ti, where)  # the defect lives at the heads
        line = (f"{name} target {ti}: max|dz| structural {dz.max():.1e}, history-dropped twin off by {teeth:.1e} at block heads"
                f" (away from them: {away.size} outputs {where})")
        if f64:
            off, fsch, mode = specs[ti]
            want = O.run_chain(f32, sample_rate=FS, freq_offset=off, fs_ch_target=fsch, demod_mode=mode, fmt="f32",
                               mix_sign_override=1, keep_decimated=True)
            assert want.decimated.size == z.size
            if mode == "usb":
                assert precisions[ti] == "full"
                e = z.astype(np.complex128) - want.decimated
                head, rest = _rms(e[heads]), _rms(e[~heads])
                assert head <= 3.0 * rest, (name, ti, head, rest)
                line += f"; float64 oracle: z rms head {head:.2e} / settled {rest:.2e}"
            else:
                audio = multi.owners[ti].audio_fs_channel.cpu().numpy()
                assert audio.size == want.audio.size
                phase = np.ones(audio.size, bool)
                for b, kind in enumerate(kinds):
                    if kind == "Z":
                        phase[st[b] : st[b + 1] + 2048] = False
                aerr = _rms((audio - want.audio)[phase])
                assert aerr < 2e-5, (name, ti, aerr)
                line += f"; float64 oracle: audio rms {aerr:.2e}"
        report.append(line)
    print("\n".join(report) + f"\n{name}: {time.perf_counter() - t0:.1f} s")
