"""tests/coder_sweep_model.py on the host: every batch reference equals the per-word model of its layer on sampled words and on
the models' own ``coder_cases()`` / ``nid_cases()``; the algebraic facts that tests/test_gpu_coder_sweep.py leans on (the Golay
tables' minimum distance 8, the free distance 7 of the K = 5 code) follow from the models alone; and the committed seeds meet
the conditions on the sweeps' inputs: the outcome mix of the words beyond a code's guarantee, the share of trellis blocks that
decode off the sent message, the ties on their surviving paths, and flips on both sides of every survivor-word boundary."""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np


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
SAMPLES = 200


def _pick(count: int, samples: int = SAMPLES, seed: int = 1) -> np.ndarray:
    return np.sort(np.random.default_rng(seed).choice(count, min(samples, count), replace=False))


# ---- the batch references against the per-word models ---------------------------------------------------------------------------


def test_records_and_patterns():
    words = np.random.default_rng(0).integers(0, 1 << 32, (5, 9), dtype=np.uint32)
    bits = CS.bits_of_words(words)
    assert bits.tolist() == [DM.record_bits(w) for w in words.tolist()]
    np.testing.assert_array_equal(CS.words_of_bits(bits), words)
    assert CS.int_of_bits(CS.bits_of_int([0x293, 5], 12)).tolist() == [0x293, 5]
    for n, low, high, count in ((24, 1, 3, 2324), (24, 4, 4, 10626), (20, 1, 3, 1350), (20, 4, 4, 4845)):
        p = CS.patterns(n, low, high)
        assert p.shape == (count, n) and len({tuple(r) for r in p.tolist()}) == count and p.sum(axis=1).min() == low and p.sum(axis=1).max() == high
    weights = np.arange(40) % 17
    assert CS.random_patterns(np.random.default_rng(0), 63, weights).sum(axis=1).tolist() == weights.tolist()


def test_bch_batch_is_the_model():
    sweep = CS.nid_patterns()
    at = _pick(sweep["weight"].size)
    cases = np.array(list(PM.nid_cases().values()), dtype=np.uint32)
    words = np.concatenate([sweep["words"][at], cases, CS.nid_codebook()["words"][::997], CS.nid_codebook()["words_parity"][::1499]])
    np.testing.assert_array_equal(CS.p25_nid_reference(words), PM.nid_all(words))
    np.testing.assert_array_equal(CS.nid_reference(sweep["bits"][at]), CS.p25_nid_reference(sweep["words"][at]))
    assert CS.nid_bits([PM.NAC << 4 | 3]).tolist() == [PM.nid_bits(PM.NAC, 3)]


def test_p25_batch_is_the_model():
    cases = PM.coder_cases()
    words, duids = np.array([c[0] for c in cases.values()], dtype=np.uint32), [c[1] for c in cases.values()]
    for sweep in (CS.p25_golay_patterns(), CS.p25_golay_codebook(), CS.p25_hamming_sweep(), CS.p25_trellis()):
        at = _pick(sweep["words"].shape[0], 70)  # 840 Golay words, 1680 Hamming words, 210 trellis blocks
        words, duids = np.concatenate([words, sweep["words"][at]]), duids + sweep["duids"][at].tolist()
    info, rec = CS.p25_reference(words, duids)
    want_info, want_rec = PM.decode_all(words, duids)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rec, want_rec)


def test_p25_encoders_and_expectations_are_the_model():
    sweep = CS.p25_trellis()
    for name, block in sweep["blocks"].items():
        for j in _pick(CS.FRAMES, 20):
            clean = PM.trellis_encode(block["message"][j].tolist())
            assert CS.p25_trellis_encode_batch(block["message"][j : j + 1])[0].tolist() == clean, (name, j)
            bad = [b for d in clean for b in (d >> 1, d & 1)]
            for k in CS.flips_of(block["pattern"][j]):
                bad[k] ^= 1
            assert block["bits"][j].tolist() == bad and block["flips"][j] == len(CS.flips_of(block["pattern"][j]))
    # the records are the model's records with the model's flips: flipped_words takes the pattern off again, and the model's
    # codewords stand at the model's places
    golay = CS.p25_golay_patterns()
    for f in _pick(golay["words"].shape[0], 20):
        flips = [int(CS.P25_GOLAY_AT[w][k]) for w in range(12) for k in range(24) if (int(golay["pattern"][f][w]) >> (23 - k)) & 1]
        got = PM.flipped_words(golay["words"][f], flips)
        assert PM.data_bits_of(got)[112:400] == [b for d in golay["data"][f] for b in PM.word_bits(PM.GOLAY[d], 24)], f


def test_dmr_batch_is_the_model():
    cases = DM.coder_cases()
    words, kinds = np.array([c[0] for c in cases.values()], dtype=np.uint32), [c[1] for c in cases.values()]
    for sweep, samples in ((CS.dmr_golay_patterns(), 200), (CS.dmr_slot_codebook(), 50), (CS.dmr_tact_codebook(), 128), (CS.bptc_singles(), 200),
                           (CS.bptc_random(), 200)):
        at = _pick(sweep["words"].shape[0], samples)
        words, kinds = np.concatenate([words, sweep["words"][at]]), kinds + sweep["kinds"][at].tolist()
    info, rec = CS.dmr_reference(words, kinds)
    want_info, want_rec = DM.decode_all(words, kinds)
    np.testing.assert_array_equal(info, want_info)
    np.testing.assert_array_equal(rec, want_rec)
    sweep = CS.bptc_random()
    for j in _pick(4000, 50):
        assert CS.bptc_encode_batch(sweep["info"][j : j + 1])[0].tolist() == DM.bptc_encode(sweep["info"][j].tolist())
        status, flips, rounds, info96 = (x[0] for x in CS.bptc_reference(sweep["raw"][j : j + 1]))
        assert (status, flips, rounds, info96.tolist()) == DM.bptc_decode(sweep["raw"][j].tolist())


def test_ysf_batch_is_the_model():
    cases = YM.coder_cases()
    words, classes = np.array([c[0] for c in cases.values()], dtype=np.uint32), [c[1] for c in cases.values()]
    dch = CS.ysf_dch_trellis()
    at = _pick(dch["words"].shape[0], 210)  # 70 frames of each class: 280 blocks
    words, classes = np.concatenate([words, dch["words"][at]]), classes + dch["classes"][at].tolist()
    info, rec, ties = CS.ysf_reference(words, classes)
    want = [YM.decode_frame(w, c) for w, c in zip(words.tolist(), classes)]
    assert info.tolist() == [w[0] for w in want] and rec.tolist() == [w[1] for w in want] and ties.sum(axis=1).tolist() == [w[2] for w in want]
    fich_words = np.concatenate([np.array([c[0] for c in cases.values()], dtype=np.uint32), CS.ysf_fich_trellis()["words"][_pick(CS.FRAMES, 120)],
                                 CS.ysf_golay_patterns()["words"][_pick(9962, 100)], CS.ysf_fich_codebook()["words"][::41]])
    fich, frec, _, _ = CS.ysf_fich_reference(fich_words)
    want_fich, want_frec = YM.fich_all(fich_words)
    np.testing.assert_array_equal(fich, want_fich)
    np.testing.assert_array_equal(frec, want_frec)
    # the encoder and the places of a data channel are the model's
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, (3, 176), dtype=np.uint8)
    tail = np.concatenate([bits, np.zeros((3, 4), dtype=np.uint8)], axis=1)
    assert CS.conv_encode_batch(tail).tolist() == [YM.conv_encode(b) for b in bits.tolist()] == [NM.conv_encode(b) for b in bits.tolist()]
    item = YM.header()
    frame = YM.record_bits(YM.frame_words(item))
    for second, data in ((False, item[1]), (True, item[2])):
        sent = YM.whiten(data)
        coded = YM.conv_encode(YM.bytes_bits(sent + [YM.crc16(sent) >> 8, YM.crc16(sent) & 0xFF]))
        assert [frame[b] for b in CS.ysf_dch_at(1, second)] == coded
    # a Golay pattern in front of the coder comes back with metric 0, as fich_with_golay_errors has it
    assert YM.fich_all([YM.coder_cases()["golay-1234"][0]])[1][0].tolist() == [2, 0, 3, 1, 6]


def test_nxdn_batch_is_the_model():
    cases = NM.coder_cases()
    words, masks = np.array([c[0] for c in cases.values()], dtype=np.uint32), [c[1] for c in cases.values()]
    sweep = CS.nxdn_trellis()
    at = _pick(sweep["words"].shape[0], 200)  # 40 frames of each mask: 280 blocks
    words, masks = np.concatenate([words, sweep["words"][at]]), masks + sweep["masks"][at].tolist()
    info, rec, ties = CS.nxdn_reference(words, masks)
    want = [NM.decode_frame(w, c) for w, c in zip(words.tolist(), masks)]
    assert info.tolist() == [w[0] for w in want] and rec.tolist() == [w[1] for w in want] and ties.sum(axis=1).tolist() == [w[2] for w in want]
    # the places of a block are the model's: a clean frame of the model reads as the model's coded bits
    for name, (item, mask, first, _sent) in NM.BLOCK_CASES.items():
        kind = "facch1" if name.startswith("facch1") else name
        frame, at = np.array(NM.record_bits(NM.frame_words(item))), CS.nxdn_at(kind, first)
        info_bits = CS.bits_of_words(np.array([NM.decode_frame(NM.frame_words(item), mask)[0]], dtype=np.uint32))[0]
        word = [w for bit, k, f, w, _c, _s in NM.LAYOUT if bit == mask][0]
        coded = np.array(NM.conv_encode(info_bits[32 * word : 32 * word + at.size // 2 - 4].tolist()))
        assert (frame[at[at >= 0]] == coded[at >= 0]).all() and [a < 0 for a in at] == [NM.punctured(j, kind) for j in range(at.size)], name


# ---- the algebra that the GPU tests lean on -------------------------------------------------------------------------------------


def test_the_golay_tables_lie_eight_apart():
    for book, size in ((CS.GOLAY24, 4096), (CS.GOLAY24_YSF, 4096), (CS.GOLAY20, 256)):
        assert book.size == size
        # linear: the word of d is the sum of the words of its bits, so the least distance is the least nonzero weight
        basis = book[1 << np.arange(size.bit_length() - 1)]
        d = np.arange(size)
        total = np.zeros(size, dtype=np.uint32)
        for k, b in enumerate(basis):
            total ^= np.where((d >> k) & 1, b, 0).astype(np.uint32)
        np.testing.assert_array_equal(total, book)
        assert int(np.bitwise_count(book[1:]).min()) == 8
    np.testing.assert_array_equal(CS.GOLAY24, CS.GOLAY24_YSF)
    data, pattern = CS.golay24_pattern_words()
    sent = CS.GOLAY24[data] ^ pattern.astype(np.uint32)
    at = _pick(data.size, 2000)
    got, want = CS.golay_reference(sent[at]), CS.golay_expected(data[at], pattern[at], sent[at])
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def test_the_free_distance_of_the_k5_code_is_seven():
    best = {}
    for n in range(1, 9):
        inputs = CS.bits_of_int(np.arange(1 << (n - 1), 1 << n), n)  # every input of n bits that begins with a 1
        coded = CS.conv_encode_batch(np.concatenate([inputs, np.zeros((inputs.shape[0], 4), dtype=np.uint8)], axis=1))
        best[n] = int(coded.sum(axis=1).min())
    assert min(best.values()) == 7 and best[1] == 7, best  # (an error event begins with a 1 and ends in four zeros)


# ---- the conditions on the sweeps (on the inputs, by the reference alone) ----------------------------------------------------------------


def test_nid_sweep_mix():
    sweep = CS.nid_patterns()
    assert np.bincount(sweep["weight"][sweep["guaranteed"]]).tolist() == [0] + [256] * 11 and (~sweep["guaranteed"]).sum() == 2048
    assert sorted(set(sweep["weight"][~sweep["guaranteed"]].tolist())) == [12, 13, 14, 15, 16]
    assert len(set((sweep["values"][sweep["guaranteed"]] >> 8).tolist())) >= 250  # the codewords come from the whole book: nearly every hi row
    beyond = np.flatnonzero(~sweep["guaranteed"])
    got = CS.nid_reference(sweep["bits"][beyond])
    other = (got[:, 0] == 1) & (got[:, 2] != sweep["values"][beyond])
    refused = got[:, 0] == 2
    assert other.sum() >= 20 and refused.sum() >= 20, (int(other.sum()), int(refused.sum()))
    book = CS.nid_codebook()
    assert book["values"].size == 65536 and (book["words"] != book["words_parity"]).sum() == 65536


def test_bptc_sweep_mix():
    sweep = CS.bptc_random()
    status, flips, rounds, info = CS.bptc_reference(sweep["raw"])
    # all three statuses occur in the BPTC sweeps: 1 and 2 here (no pattern of weight 2 .. 12 can leave a clean word: the code's
    # distance is 9, and a tenth flip would have to be the one bit outside the matrix), 0 below at the unseen single flip
    assert sorted(set(status.tolist())) == [1, 2] and min((status == 1).sum(), (status == 2).sum()) >= 400, np.bincount(status).tolist()
    assert ((status == 1) & (info != sweep["info"]).any(axis=1)).any()  # and "corrected" onto another message is among them
    assert (rounds >= 3).sum() >= 50, int((rounds >= 3).sum())
    assert sweep["weight"].min() == 2 and sweep["weight"].max() == 12 and (sweep["pattern"].sum(axis=1) == sweep["weight"]).all()
    double = sweep["weight"] == 2
    assert (status[double] == 2).any()  # no restoration can be claimed above weight 1: two syndromes may name no bit
    singles = CS.bptc_singles()
    assert singles["flip"].size == 64 * 196 and len({r.tobytes() for r in singles["info"][::196]}) == 64
    at = np.union1d(_pick(singles["flip"].size), np.flatnonzero(singles["flip"] == 0))
    status, flips, rounds, info = CS.bptc_reference(singles["raw"][at])
    assert sorted(set(status.tolist())) == [0, 1]
    seen = singles["flip"][at] != 0  # (sent bit 0 is D[0], which lies outside the matrix: its flip goes unseen)
    np.testing.assert_array_equal(info, singles["info"][at])
    assert status.tolist() == seen.astype(int).tolist() and flips.tolist() == seen.astype(int).tolist() and rounds.tolist() == (1 + seen).tolist()


def _boundaries(steps: int) -> list:
    return sorted({0, steps - 1} | {t for w in range(32, steps, 32) for t in (w - 1, w)})


def _check_block_class(name, block, decoded, ties, steps_hit, words: bool = True):
    count = block["flips"].size
    assert count >= 1024, name
    wrong = (decoded != block["message"]).any(axis=1)
    assert 4 * wrong.sum() >= count, (name, int(wrong.sum()), count)
    assert (ties > 0).sum() >= 100, (name, int((ties > 0).sum()))
    need = _boundaries(steps_hit.shape[1]) if words else [0, steps_hit.shape[1] - 1]
    assert steps_hit[:, need].any(axis=0).all(), (name, need)
    assert block["flips"].min() == 0 and (block["pattern"].sum(axis=1) == block["flips"]).all(), name


def test_ysf_trellis_sweep_conditions():
    sweep = CS.ysf_fich_trellis()
    block = sweep["blocks"]["fich"]
    _, _, ties, decoded = CS.ysf_fich_reference(sweep["words"])
    assert block["flips"].max() == 30 and sweep["words"].shape[0] % 4 != 0
    _check_block_class("fich", block, decoded, ties, CS.conv_flip_steps(block["pattern"]))
    sweep = CS.ysf_dch_trellis()
    assert sweep["words"].shape[0] % 2 == 1
    info, _, ties = CS.ysf_reference(sweep["words"], sweep["classes"])
    bits = CS.bits_of_words(info)
    for name, block in sweep["blocks"].items():
        decoded = bits[block["rows"], block["first_bit"] : block["first_bit"] + block["steps"]]
        assert block["flips"].max() == int(0.15 * 2 * block["steps"])
        _check_block_class(name, block, decoded, ties[block["rows"], block["slot"] - 1], CS.conv_flip_steps(block["pattern"]))
    assert sorted(sweep["blocks"]) == ["class1-a", "class1-b", "class2-a", "class3-a"]


def test_nxdn_trellis_sweep_conditions():
    sweep = CS.nxdn_trellis()
    assert sweep["words"].shape[0] % 2 == 1 and sorted(set(sweep["masks"].tolist())) == [1, 2, 4, 7, 8]
    info, _, ties = CS.nxdn_reference(sweep["words"], sweep["masks"])
    bits = CS.bits_of_words(info)
    for name, block in sweep["blocks"].items():
        decoded = bits[block["rows"], block["first_bit"] : block["first_bit"] + block["steps"]]
        assert block["flips"].max() == int(0.15 * block["sent"].sum()) and not (block["pattern"][:, ~block["sent"]]).any(), name
        _check_block_class(name, block, decoded, ties[block["rows"], block["slot"]], CS.conv_flip_steps(block["pattern"]))
    assert sorted(sweep["blocks"]) == sorted(CS.NXDN_CLASSES) and {b["steps"] for b in sweep["blocks"].values()} == {36, 96, 175}


def test_p25_trellis_sweep_conditions():
    sweep = CS.p25_trellis()
    for b, (name, block) in enumerate(sweep["blocks"].items()):
        two = block["bits"].reshape(-1, 98, 2)
        decoded, _, ties = CS.p25_trellis_reference(two[:, :, 0] << 1 | two[:, :, 1])
        assert block["flips"].max() == 29
        _check_block_class(name, block, decoded, ties, CS.p25_flip_steps(block["pattern"]), words=False)
