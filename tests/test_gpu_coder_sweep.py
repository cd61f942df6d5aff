"""The error-correcting decoders of the protocol layers (``iqa_p25_nid``, ``iqa_p25_decode``, ``iqa_dmr_decode``, ``iqa_ysf_fich``,
``iqa_ysf_decode``, ``iqa_nxdn_decode``; DESIGN.md sections 29, 31, 32, 34) on the MI355X over whole codebooks, every error pattern
up to and one beyond each code's guarantee, and dense random errors on random messages through every trellis.  The words come
from tests/coder_sweep_model.py; the kernels are held to its batch references (which tests/test_coder_sweep_host.py holds to the
per-word models) and, where the code's algebra gives the answer, to that as well.  Every entry point is called straight through
the binding with sentinels behind its outputs; every comparison is of integers and exact; a mismatch names the first word or
block and its flips.

    sweep                          kernel           reaches
    all 65 536 NIDs, both parities k_p25_nid        every entry of the hi and lo tables as the answer, the parity flag
    BCH weight 1 .. 11, 12 .. 16   k_p25_nid        the guarantee on codewords of the whole book; another codeword; refusal
    all 4096 Golay words           k_p25_decode     every hi and lo entry, every word position of a TDULC
                                   k_ysf_fich       every hi and lo entry, every slot, every lane's sixteen hi rows
    Golay weight 1 .. 3, 4         k_p25_decode,    the guarantee and the refusal on every pattern; rec sums over mixed words
                                   k_ysf_fich, k_dmr_decode (Golay(20,8), weight 1 .. 3 on 16 bytes, 4 on 2)
    all 256 slot-type bytes        k_dmr_decode     every codeword as the answer
    all 1024 words x 24 positions  k_p25_decode     Hamming(10,6) exhaustively, errors and the five unnamed syndromes included
    all 128 TACT words             k_dmr_decode     Hamming(7,4) exhaustively
    BPTC single flips, 64 messages k_dmr_decode     every matrix bit restored; the one bit outside the matrix
    BPTC weight 2 .. 12            k_dmr_decode     rounds 2 .. 5, corrected, miscorrected and failed
    dense FICH                     k_ysf_fich       100 steps (NW = 4), four trellises to a wave, the last wave partly empty
    dense DCH, classes 1 2 3 mixed k_ysf_decode     180 and 100 steps (NW = 6), two frames of different classes to a wave
    dense SACCH / FACCH1 / CAC     k_nxdn_decode    36, 96, 175 steps with erasures at NW = 2, 3, 6; three trellises to a wave
    dense TSBK blocks              k_p25_decode     the scalar four-state trellis, three blocks to a workgroup
"""
from __future__ import annotations

import importlib.util
import sys
from ctypes import c_int64
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


CS = _load("coder_sweep_model")
PM, DM, YM, NM = CS.PM, CS.DM, CS.YM, CS.NM
SENTINEL, TAIL = 0x5A5A5A5A, 64


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def _call(A, name, words, width, selector, sizes):
    """The entry point ``name`` straight through the binding in one launch: the records uint32[K][width], the selector bytes (or
    None), and an int32[K][size] output per size, each in a buffer with sentinels behind it."""
    import torch

    N = A.native
    words = np.array(words, dtype=np.uint32).reshape(-1, width)
    k = words.shape[0]
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    args = [N.ptr(bits)]
    if selector is not None:
        selector_dev = torch.from_numpy(np.array(selector, dtype=np.uint8)).cuda()
        assert selector_dev.numel() == k
        args.append(N.ptr(selector_dev))
    outs = [torch.full((size * k + TAIL,), SENTINEL, dtype=torch.int32, device="cuda") for size in sizes]
    N.call(name, *args, c_int64(k), *[N.ptr(o) for o in outs], N.stream_ptr())
    torch.cuda.synchronize()
    for o, size in zip(outs, sizes):
        assert (o[size * k :] == SENTINEL).all(), "a sentinel behind an output was overwritten"
    return [o[: size * k].cpu().numpy().reshape(k, size) for o, size in zip(outs, sizes)]


def _nid(A, words):
    return _call(A, "iqa_p25_nid", words, 54, None, (4,))[0]


def _p25(A, words, duids):
    info, rec = _call(A, "iqa_p25_decode", words, 54, duids, (9, 8))
    return info.view(np.uint32), rec


def _dmr(A, words, kinds):
    info, rec = _call(A, "iqa_dmr_decode", words, 9, kinds, (3, 8))
    return info.view(np.uint32), rec


def _fich(A, words):
    fich, rec = _call(A, "iqa_ysf_fich", words, 30, None, (2, 5))
    return fich.view(np.uint32), rec


def _ysf(A, words, classes):
    info, rec = _call(A, "iqa_ysf_decode", words, 30, classes, (12, 4))
    return info.view(np.uint32), rec


def _nxdn(A, words, masks):
    info, rec = _call(A, "iqa_nxdn_decode", words, 12, masks, (14, 4))
    return info.view(np.uint32), rec


def _same(got, want, what, where):
    """got == want, exactly; a mismatch names the first row by ``where(row)``."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        row = int(np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0])
        raise AssertionError(f"{what}: first at row {row}, {where(row)}: got {got[row].tolist()}, want {want[row].tolist()}")
    np.testing.assert_array_equal(got, want)


def _hex(values) -> str:
    return " ".join(f"{int(v):x}" for v in np.asarray(values).reshape(-1))


# ---- whole codebooks, clean ------------------------------------------------------------------------------------------------------


def test_every_nid_value_clean_and_with_its_parity_bit_flipped(A):
    book = CS.nid_codebook()
    values = book["values"]
    zeros = np.zeros_like(values)
    where = lambda row: f"NID value 0x{row:04x}"  # noqa: E731
    _same(_nid(A, book["words"]), np.stack([zeros, zeros, values, zeros + 1], axis=1), "clean", where)
    _same(_nid(A, book["words_parity"]), np.stack([zeros, zeros, values, zeros], axis=1), "parity bit flipped", where)


def _golay_where(sweep):
    return lambda row: (f"words of data {_hex(sweep['data'][row])} under the patterns {_hex(sweep['pattern'][row])} "
                        f"(flips {[CS.flips_of(CS.bits_of_int(p, 24)) for p in sweep['pattern'][row]]})")


def _check_p25_golay(A, sweep):
    info, rec = _p25(A, sweep["words"], sweep["duids"])
    dist, data, refused = CS.golay_expected(sweep["data"], sweep["pattern"], sweep["sent"])
    want_info, want_rec = CS.p25_golay_records(data, dist, refused)  # by the algebra: restored up to weight 3, refused at 4
    _same(rec, want_rec, "rec", _golay_where(sweep))
    _same(info, want_info, "info", _golay_where(sweep))
    ref_info, ref_rec = CS.p25_reference(sweep["words"], sweep["duids"])
    _same(rec, ref_rec, "rec against the model", _golay_where(sweep))
    _same(info, ref_info, "info against the model", _golay_where(sweep))
    return rec


def test_every_golay_word_in_a_tdulc(A):
    sweep = CS.p25_golay_codebook()
    assert sorted(set(sweep["data"].reshape(-1).tolist())) == list(range(4096))
    rec = _check_p25_golay(A, sweep)
    assert (rec == [2, 0, 0, 0, 0, 0, 0, 0]).all()


def _check_fich_golay(A, sweep):
    fich, rec = _fich(A, sweep["words"])
    dist, data, refused = CS.golay_expected(sweep["data"], sweep["pattern"], sweep["sent"])
    want_fich, want_rec = CS.ysf_fich_records(data, dist, refused, np.zeros(data.shape[0], dtype=np.int64))  # the trellis: metric 0
    _same(rec, want_rec, "rec", _golay_where(sweep))
    _same(fich, want_fich, "fich", _golay_where(sweep))
    ref_fich, ref_rec, _, _ = CS.ysf_fich_reference(sweep["words"])
    _same(rec, ref_rec, "rec against the model", _golay_where(sweep))
    _same(fich, ref_fich, "fich against the model", _golay_where(sweep))
    return rec


def test_every_golay_word_in_a_fich(A):
    sweep = CS.ysf_fich_codebook()
    assert sorted(set(sweep["data"].reshape(-1).tolist())) == list(range(4096))
    assert not _check_fich_golay(A, sweep).any()


def test_every_slot_type_byte(A):
    sweep = CS.dmr_slot_codebook()
    info, rec = _dmr(A, sweep["words"], sweep["kinds"])
    where = lambda row: f"slot type 0x{row:02x}"  # noqa: E731
    zeros = np.zeros(256, dtype=np.int64)
    _same(rec[:, 2:], np.stack([zeros, zeros, sweep["data"], zeros, zeros, zeros + 1], axis=1), "rec", where)
    _same(info, CS.words_of_bits(sweep["info"]), "info", where)
    ref_info, ref_rec = CS.dmr_reference(sweep["words"], sweep["kinds"])
    _same(rec, ref_rec, "rec against the model", where)
    _same(info, ref_info, "info against the model", where)


def test_every_ten_bit_word_at_every_hamming_position(A):
    sweep = CS.p25_hamming_sweep()
    assert all(sorted(sweep["ten"][:, p].tolist()) == list(range(1024)) for p in range(24))
    # by the algebra: a codeword is clean, a codeword with one bit flipped is restored, every other word is left alone
    six, flag = CS.bits_of_int(np.arange(1024), 10)[:, :6].copy(), np.full(1024, 2)
    for d in range(64):
        cw = PM.bits_word(PM.hamming_encode(PM.word_bits(d, 6)))
        six[cw], flag[cw] = CS.bits_of_int(d, 6), 0
        for j in range(10):
            six[cw ^ 1 << j], flag[cw ^ 1 << j] = CS.bits_of_int(d, 6), 1
    assert np.bincount(flag).tolist() == [64, 640, 320]
    info, rec = _p25(A, sweep["words"], sweep["duids"])
    want_info, want_rec = CS.p25_hamming_records(six[sweep["ten"]], flag[sweep["ten"]])
    where = lambda row: f"the ten-bit words {_hex(sweep['ten'][row])}"  # noqa: E731
    _same(rec, want_rec, "rec", where)
    _same(info, want_info, "info", where)
    ref_info, ref_rec = CS.p25_reference(sweep["words"], sweep["duids"])
    _same(rec, ref_rec, "rec against the model", where)
    _same(info, ref_info, "info against the model", where)


def test_every_tact_word(A):
    sweep = CS.dmr_tact_codebook()
    status, nibble = np.full(128, -1), np.full(128, -1)
    for n in range(16):  # Hamming(7,4) is perfect: a codeword or one bit from one
        cw = PM.bits_word(DM.tact_encode(n >> 3, n >> 2 & 1, n & 3))
        status[cw], nibble[cw] = 0, n
        for j in range(7):
            status[cw ^ 1 << j], nibble[cw ^ 1 << j] = 1, n
    assert status.min() == 0 and np.bincount(status).tolist() == [16, 112]
    info, rec = _dmr(A, sweep["words"], sweep["kinds"])
    where = lambda row: f"TACT word {row:07b}"  # noqa: E731
    _same(rec, np.stack([status, nibble] + [np.full(128, v) for v in (4, 0, 0, 4, 0, 0)], axis=1), "rec", where)
    assert not info.any()
    _same(rec, CS.dmr_reference(sweep["words"], sweep["kinds"])[1], "rec against the model", where)


# ---- every pattern up to the guarantee, and one beyond ---------------------------------------------------------------------------


def test_every_golay_pattern_of_weight_1_to_4_in_a_tdulc(A):
    sweep = CS.p25_golay_patterns()
    weight = np.bitwise_count(sweep["pattern"].astype(np.uint32))
    assert np.bincount(weight.reshape(-1))[1:].tolist() == [8 * 24, 8 * 276, 8 * 2024, 2 * 10626]
    rec = _check_p25_golay(A, sweep)
    assert rec[:, 2].sum() == 2 * 10626 and rec[:, 1].sum() == 8 * 2324 and rec[:, 3].sum() == 8 * (24 + 2 * 276 + 3 * 2024)


def test_every_golay_pattern_of_weight_1_to_4_in_a_fich(A):
    sweep = CS.ysf_golay_patterns()
    assert sweep["words"].shape[0] % 4 != 0  # the last wave is partly empty
    rec = _check_fich_golay(A, sweep)
    assert rec[:, 3].sum() == 2 * 10626 and rec[:, 2].sum() == 8 * 2324 + 1 and not rec[:, 1].any() and sorted(set(rec[:, 0].tolist())) == [1, 2]


def test_every_slot_type_pattern_of_weight_1_to_4(A):
    sweep = CS.dmr_golay_patterns()
    weight = np.bitwise_count(sweep["pattern"].astype(np.uint32))
    assert np.bincount(weight)[1:].tolist() == [16 * 20, 16 * 190, 16 * 1140, 2 * 4845]
    info, rec = _dmr(A, sweep["words"], sweep["kinds"])
    where = lambda row: (f"slot type 0x{sweep['data'][row]:02x} under the pattern 0x{sweep['pattern'][row]:05x} "  # noqa: E731
                         f"(flips {CS.flips_of(CS.bits_of_int(sweep['pattern'][row], 20))})")
    dist, data, refused = CS.golay_expected(sweep["data"], sweep["pattern"], sweep["sent"])
    clean = np.stack([0 * dist, 0 * dist, 0 * dist + 1], axis=1)
    want = np.concatenate([np.stack([np.where(refused, 2, 1), dist, data], axis=1), np.where(refused[:, None], [4, 0, 0], clean)], axis=1)
    _same(rec[:, 2:], want, "rec", where)
    _same(info, np.where(refused[:, None], 0, CS.words_of_bits(sweep["info"][None, :])).astype(np.uint32), "info", where)
    ref_info, ref_rec = CS.dmr_reference(sweep["words"], sweep["kinds"])
    _same(rec, ref_rec, "rec against the model", where)
    _same(info, ref_info, "info against the model", where)


def test_bch_patterns_up_to_the_guarantee_and_beyond(A):
    sweep = CS.nid_patterns()
    nid = _nid(A, sweep["words"])
    where = lambda row: f"NID value 0x{sweep['values'][row]:04x} with the code bits {CS.flips_of(sweep['pattern'][row])} flipped"  # noqa: E731
    sure = sweep["guaranteed"]
    want = np.stack([0 * sweep["weight"] + 1, sweep["weight"], sweep["values"], 1 - (sweep["weight"] & 1)], axis=1)
    _same(nid[sure], want[sure], "weight 1 .. 11", where)  # by the algebra: distance 23 restores eleven flips
    ref = CS.nid_reference(sweep["bits"])
    _same(nid, ref, "against the model", where)
    assert sorted(set(nid[~sure, 0].tolist())) == [1, 2]


def test_bptc_every_single_flip(A):
    sweep = CS.bptc_singles()
    info, rec = _dmr(A, sweep["words"], sweep["kinds"])
    where = lambda row: f"message {row // 196} with the sent bit {sweep['flip'][row]} flipped"  # noqa: E731
    _same(info, CS.words_of_bits(sweep["info"]), "info", where)
    seen = (sweep["flip"] != 0).astype(np.int64)  # (sent bit 0 is D[0], outside the matrix: its flip goes unseen and the burst is clean)
    _same(rec[:, 5:], np.stack([seen, seen, 1 + seen], axis=1), "status, flips, rounds", where)
    assert (rec[:, 2:4] == 0).all()


def test_bptc_random_patterns_of_weight_2_to_12(A):
    sweep = CS.bptc_random()
    info, rec = _dmr(A, sweep["words"], sweep["kinds"])
    where = lambda row: f"message {_hex(CS.words_of_bits(sweep['info'][row : row + 1]))} with the sent bits {CS.flips_of(sweep['pattern'][row])} flipped"  # noqa: E731
    ref_info, ref_rec = CS.dmr_reference(sweep["words"], sweep["kinds"])
    _same(rec, ref_rec, "rec", where)
    _same(info, ref_info, "info", where)
    assert sorted(set(rec[:, 5].tolist())) == [1, 2] and (rec[:, 7] >= 3).sum() >= 50 and rec[:, 7].max() == 5


# ---- dense errors through every trellis --------------------------------------------------------------------------------------------


def _block_where(name, block):
    return lambda row: f"{name} block {row} (frame {block['rows'][row]}) with the coded bits {CS.flips_of(block['pattern'][row])} flipped"


def _check_conv_block(name, block, decoded, metric, free_distance_seven):
    """What holds of a decoded block without a model: its metric is the distance, over the sent bits, from what arrived to the
    re-encoding of the decoded bits, and no more than the flips; it ends in four zeros; unpunctured, three flips or fewer are
    put right (free distance 7)."""
    where = _block_where(name, block)
    again = CS.conv_encode_batch(decoded)
    _same(metric, ((again != block["coded"]) & block["sent"]).sum(axis=1), f"{name}: the metric is the distance to the re-encoded path", where)
    assert (metric <= block["flips"]).all(), (name, where(int(np.flatnonzero(metric > block["flips"])[0])))
    assert not decoded[:, -4:].any(), name
    if free_distance_seven:
        few = block["flips"] <= 3
        _same(decoded[few], block["message"][few], f"{name}: three flips or fewer", lambda row: where(int(np.flatnonzero(few)[row])))
        _same(metric[few], block["flips"][few], f"{name}: three flips or fewer, the metric", lambda row: where(int(np.flatnonzero(few)[row])))


def test_dense_errors_through_the_fich_trellis(A):
    sweep = CS.ysf_fich_trellis()
    block = sweep["blocks"]["fich"]
    assert sweep["words"].shape[0] % 4 != 0
    fich, rec = _fich(A, sweep["words"])
    where = _block_where("fich", block)
    ref_fich, ref_rec, _, _ = CS.ysf_fich_reference(sweep["words"])
    _same(rec, ref_rec, "rec", where)
    _same(fich, ref_fich, "fich", where)
    assert (rec[:, 1] <= block["flips"]).all()
    few = np.flatnonzero(block["flips"] <= 3)  # free distance 7: the sent FICH with metric = flips, no Golay word touched
    zeros = np.zeros(few.size, dtype=np.int64)
    _same(rec[few], np.stack([(block["flips"][few] > 0).astype(np.int64), block["flips"][few], zeros, zeros, zeros], axis=1), "three flips or fewer",
          lambda row: where(int(few[row])))
    no = np.zeros((few.size, 4), dtype=np.int64)
    _same(fich[few], CS.ysf_fich_records(sweep["data"][few], no, no.astype(bool), zeros)[0], "three flips or fewer, the data", lambda row: where(int(few[row])))


def test_dense_errors_through_the_dch_trellises(A):
    sweep = CS.ysf_dch_trellis()
    assert sweep["words"].shape[0] % 2 == 1
    info, rec = _ysf(A, sweep["words"], sweep["classes"])
    ref_info, ref_rec, _ = CS.ysf_reference(sweep["words"], sweep["classes"])
    bits = CS.bits_of_words(info)
    for name, block in sweep["blocks"].items():
        rows, at = block["rows"], slice(block["first_bit"], block["first_bit"] + block["steps"])
        _same(rec[rows, block["slot"]], ref_rec[rows, block["slot"]], f"{name}: the metric", _block_where(name, block))
        _same(bits[rows, at], CS.bits_of_words(ref_info)[rows, at], f"{name}: the bits", _block_where(name, block))
        _check_conv_block(name, block, bits[rows, at], rec[rows, block["slot"]], True)
    _same(rec, ref_rec, "rec", lambda row: f"frame {row} of class {sweep['classes'][row]}")
    _same(info, ref_info, "info", lambda row: f"frame {row} of class {sweep['classes'][row]}")  # (zeros wherever no block lies, too)


def test_dense_errors_through_the_punctured_nxdn_trellises(A):
    sweep = CS.nxdn_trellis()
    info, rec = _nxdn(A, sweep["words"], sweep["masks"])
    ref_info, ref_rec, _ = CS.nxdn_reference(sweep["words"], sweep["masks"])
    bits = CS.bits_of_words(info)
    for name, block in sweep["blocks"].items():
        rows, at = block["rows"], slice(block["first_bit"], block["first_bit"] + block["steps"])
        _same(rec[rows, block["slot"]], ref_rec[rows, block["slot"]], f"{name}: the metric", _block_where(name, block))
        _same(bits[rows, at], CS.bits_of_words(ref_info)[rows, at], f"{name}: the bits", _block_where(name, block))
        _check_conv_block(name, block, bits[rows, at], rec[rows, block["slot"]], False)
    _same(rec, ref_rec, "rec", lambda row: f"frame {row} of mask {sweep['masks'][row]}")
    _same(info, ref_info, "info", lambda row: f"frame {row} of mask {sweep['masks'][row]}")


def test_dense_errors_through_the_p25_trellis(A):
    sweep = CS.p25_trellis()
    info, rec = _p25(A, sweep["words"], sweep["duids"])
    ref_info, ref_rec = CS.p25_reference(sweep["words"], sweep["duids"])
    bits = CS.bits_of_words(info)
    for b, (name, block) in enumerate(sweep["blocks"].items()):
        where = lambda row, block=block, name=name: f"{name} of frame {row} with the sent bits {CS.flips_of(block['pattern'][row])} flipped"  # noqa: E731
        _same(rec[:, 1 + b], ref_rec[:, 1 + b], f"{name}: the metric", where)
        _same(info[:, 3 * b : 3 * b + 3], ref_info[:, 3 * b : 3 * b + 3], f"{name}: the bits", where)
        two = bits[:, 96 * b : 96 * b + 96].reshape(-1, 48, 2)
        again = CS.p25_trellis_encode_batch(two[:, :, 0] << 1 | two[:, :, 1])  # (with the flush dibit: the path ends in state 0)
        again = np.stack([again >> 1, again & 1], axis=2).reshape(-1, 196)
        _same(rec[:, 1 + b], (again != block["bits"]).sum(axis=1), f"{name}: the metric is the distance to the re-encoded path", where)
        assert (rec[:, 1 + b] <= block["flips"]).all(), name
        clean = block["flips"] == 0
        _same(two[clean, :, 0] << 1 | two[clean, :, 1], block["message"][clean], f"{name}: no flips", lambda row: "a clean block")
    _same(rec, ref_rec, "rec", lambda row: f"frame {row}")
