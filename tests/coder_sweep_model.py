"""Batch forms of the coder models of the four protocol layers (tests/p25_model.py, dmr_model.py, ysf_model.py, nxdn_model.py)
and the generators of the coder sweeps: whole codebooks, every error pattern up to and one beyond each code's guarantee, and
dense random errors on random messages through every trellis.  Of the package it uses nothing.  Every constant, every layout
(which frame bit a code bit is) and every encoder is the per-word models'; what is new here is only that the decoders run over
thousands of words at once: the nearest codeword by one ``argmin`` over the book (the first minimum is the smallest data, so
the order (distance, data) is kept), the Hamming codes by their syndrome tables, BPTC(196,96) round by round over all frames,
and the two trellises step by step over all blocks, with the ties on the surviving path counted.  tests/test_coder_sweep_host.py
holds every batch form to its per-word model and checks the conditions on the sweeps; tests/test_gpu_coder_sweep.py holds the
kernels to them.  Everything is a pure function of a seed.

A record here is what the kernels read: u32 words, the first sent bit the MSB of word 0.  A sweep is a dict: ``words`` (the
records), the selector of the decoder (``duids``, ``kinds``, ``classes`` or ``masks``) and what was put in (the data, the
patterns, the flips), so a test can state an expectation without a model and can name the word that missed it."""
from __future__ import annotations

import functools
import importlib.util
import itertools
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


PM, DM, YM, NM = _load("p25_model"), _load("dmr_model"), _load("ysf_model"), _load("nxdn_model")
FAR = 1000
DENSITY = 0.15  # a trellis block takes 0 .. DENSITY * (its sent bits) flips, uniformly
SEED = 20

# ---- records ------------------------------------------------------------------------------------------------------------------


def bits_of_words(words) -> np.ndarray:
    """uint8[K][32 W]: the bits of uint32[K][W] records, the first sent bit first."""
    words = np.asarray(words, dtype=np.uint32)
    return np.unpackbits(np.ascontiguousarray(words.astype(">u4")).view(np.uint8).reshape(words.shape[0], -1), axis=1)


def words_of_bits(bits) -> np.ndarray:
    """uint32[K][W] of uint8[K][32 W]."""
    bits = np.asarray(bits, dtype=np.uint8)
    return np.ascontiguousarray(np.packbits(bits, axis=1)).view(">u4").astype(np.uint32)


def int_of_bits(bits) -> np.ndarray:
    """The integers of the bits along the last axis, the first bit on top (at most 64)."""
    bits = np.asarray(bits)
    n = bits.shape[-1]
    return (bits.astype(np.uint64) << np.arange(n - 1, -1, -1, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def bits_of_int(values, n: int) -> np.ndarray:
    """uint8[..., n]: the n low bits of the integers, the top one first."""
    values = np.asarray(values).astype(np.uint64)
    return ((values[..., None] >> np.arange(n - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)


def random_frames(rng, count: int, bits: int) -> np.ndarray:
    """uint8[count][bits]: seeded random frame bits, under which the swept words are laid: what a decoder must not read is noise."""
    return rng.integers(0, 2, (count, bits), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def patterns(n: int, low: int, high: int) -> np.ndarray:
    """uint8[P][n]: every error pattern of n bits whose weight is low .. high, in order of weight."""
    out = [np.zeros((0, n), dtype=np.uint8)]
    for w in range(low, high + 1):
        at = np.array(list(itertools.combinations(range(n), w)), dtype=np.int64).reshape(-1, w)
        one = np.zeros((at.shape[0], n), dtype=np.uint8)
        np.put_along_axis(one, at, 1, axis=1)
        out.append(one)
    out = np.concatenate(out)
    out.setflags(write=False)
    return out


def random_patterns(rng, n: int, weights) -> np.ndarray:
    """uint8[K][n]: row k a random pattern of weight weights[k]."""
    weights = np.asarray(weights)
    rank = rng.random((weights.size, n)).argsort(axis=1).argsort(axis=1)
    return (rank < weights[:, None]).astype(np.uint8)


def flips_of(pattern_row) -> list:
    return np.flatnonzero(np.asarray(pattern_row)).tolist()


# ---- the block codes, over many words -----------------------------------------------------------------------------------------


def nearest(words, book, chunk: int = 0) -> tuple:
    """(distance, data) int64[K] each: the nearest word of ``book`` (in order of its data) to every word, the smaller data on
    equal distance: ``argmin`` gives the first minimum."""
    words, book = np.asarray(words), np.asarray(book)
    chunk = chunk or max(1, (1 << 23) // book.size)
    dist, data = np.empty(words.size, dtype=np.int64), np.empty(words.size, dtype=np.int64)
    for a in range(0, words.size, chunk):
        d = np.bitwise_count(words[a : a + chunk, None] ^ book[None, :])
        at = d.argmin(axis=1)
        data[a : a + chunk] = at
        dist[a : a + chunk] = d[np.arange(at.size), at]
    return dist, data


def nid_bits(values, flip_parity: bool = False) -> np.ndarray:
    """uint8[K][64]: the 63 code bits and the parity bit of the 16-bit values."""
    cw = PM.bch_codewords()[np.asarray(values, dtype=np.int64)]
    parity = (np.bitwise_count(cw) & 1).astype(np.uint8) ^ np.uint8(1 if flip_parity else 0)
    return np.concatenate([bits_of_int(cw, 63), parity[:, None]], axis=1)


def nid_reference(bits64) -> np.ndarray:
    """int32[K][4] = status, distance, value, parity_ok of uint8[K][64]: the batch form of ``p25_model.nid_decode``."""
    word = int_of_bits(bits64)
    r = word >> np.uint64(1)
    dist, value = nearest(r, PM.bch_codewords())
    status = np.where(dist == 0, 0, np.where(dist <= 11, 1, 2))
    value = np.where(status == 2, (r >> np.uint64(47)).astype(np.int64), value)
    return np.stack([status, dist, value, 1 - (np.bitwise_count(word).astype(np.int64) & 1)], axis=1).astype(np.int32)


GOLAY24 = np.array(PM.GOLAY, dtype=np.uint32)
GOLAY24_YSF = np.asarray(YM.GOLAY, dtype=np.uint32)
GOLAY20 = np.array(DM.GOLAY, dtype=np.uint32)


def golay_reference(words, book=GOLAY24) -> tuple:
    """(distance, data, refused) of 24-bit (20-bit with the book of 256) words: the batch form of the models' ``golay_decode``;
    a refused word keeps the bits above its twelve check bits."""
    words = np.asarray(words, dtype=np.uint32)
    dist, data = nearest(words, book)
    refused = dist > 3
    return dist, np.where(refused, (words >> 12).astype(np.int64), data), refused


H10 = np.array(PM.HAMMING_ALL_COLUMNS, dtype=np.int64)
H10_AT = np.array([H10.tolist().index(s) if s in H10.tolist() else -1 for s in range(16)], dtype=np.int64)


def hamming10_reference(ten) -> tuple:
    """(six uint8[..., 6], flag): the batch form of ``p25_model.hamming_decode``."""
    ten = np.asarray(ten, dtype=np.uint8)
    syn = np.bitwise_xor.reduce(ten.astype(np.int64) * H10, axis=-1)
    at = H10_AT[syn]
    fixed = ten ^ (np.arange(10) == at[..., None]).astype(np.uint8)
    return fixed[..., :6], np.where(syn == 0, 0, np.where(at >= 0, 1, 2))


def _syndromes(bits, checks, first_parity: int) -> np.ndarray:
    """The syndromes as integers, check e the bit e, of words along the last axis: ``dmr_model._syndrome`` over many words."""
    bits = np.asarray(bits, dtype=np.int64)
    out = np.zeros(bits.shape[:-1], dtype=np.int64)
    for e, eq in enumerate(checks):
        out |= ((bits[..., list(eq)].sum(axis=-1) + bits[..., first_parity + e]) & 1) << e
    return out


def _positions(checks, length: int, first_parity: int) -> np.ndarray:
    """syndrome -> the bit it names, or -1."""
    out = np.full(1 << len(checks), -1, dtype=np.int64)
    out[_syndromes(np.eye(length, dtype=np.int64), checks, first_parity)] = np.arange(length)
    return out


H7_AT, H13_AT, H15_AT = _positions(DM.TACT_CHECKS, 7, 4), _positions(DM.COLUMN_CHECKS, 13, 9), _positions(DM.ROW_CHECKS, 15, 11)


def tact_reference(seven) -> tuple:
    """(status, nibble): the batch form of ``dmr_model.tact_decode``."""
    seven = np.asarray(seven, dtype=np.uint8)
    syn = _syndromes(seven, DM.TACT_CHECKS, 4)
    fixed = seven ^ ((np.arange(7) == H7_AT[syn][..., None]) & (syn != 0)[..., None]).astype(np.uint8)
    return (syn != 0).astype(np.int64), int_of_bits(fixed[..., :4]).astype(np.int64)


BPTC_ORDER = (DM.INTERLEAVE * np.arange(196)) % 196
BPTC_INFO = np.array(DM.INFO_INDEX, dtype=np.int64)


def bptc_reference(raw) -> tuple:
    """(status, flips, rounds, info uint8[K][96]) of uint8[K][196] as sent: the batch form of ``dmr_model.bptc_decode``, every round
    over all the frames that are still flipping."""
    raw = np.asarray(raw, dtype=np.uint8)
    k = raw.shape[0]
    m = raw[:, BPTC_ORDER][:, 1:].reshape(k, 13, 15).copy()  # m[:, r, c] is D[1 + 15 r + c]
    flips, rounds, active = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64), np.ones(k, dtype=bool)
    for _ in range(DM.ROUNDS):
        rounds += active
        at = H13_AT[_syndromes(m.transpose(0, 2, 1), DM.COLUMN_CHECKS, 9)]  # [K][15]
        do = (at >= 0) & active[:, None]
        f, c = np.nonzero(do)
        m[f, at[f, c], c] ^= 1
        now = do.sum(axis=1)
        syn = _syndromes(m[:, :9, :], DM.ROW_CHECKS, 11)  # [K][9]
        do = (syn != 0) & active[:, None]
        f, r = np.nonzero(do)
        m[f, r, H15_AT[syn[f, r]]] ^= 1
        now += do.sum(axis=1)
        flips += now
        active &= now > 0
    bad = (_syndromes(m.transpose(0, 2, 1), DM.COLUMN_CHECKS, 9) != 0).any(axis=1) | (_syndromes(m[:, :9, :], DM.ROW_CHECKS, 11) != 0).any(axis=1)
    status = np.where(bad, 2, np.where(flips > 0, 1, 0))
    return status, flips, rounds, m.reshape(k, 195)[:, BPTC_INFO - 1]


@functools.lru_cache(maxsize=1)
def _bptc_basis() -> np.ndarray:
    return np.array([DM.bptc_encode(row) for row in np.eye(96, dtype=np.int64).tolist()], dtype=np.uint8)


def bptc_encode_batch(info) -> np.ndarray:
    """uint8[K][196] as sent of uint8[K][96]: the code is linear, so a word is the sum of ``dmr_model.bptc_encode`` of its bits."""
    return ((np.asarray(info, dtype=np.int64) @ _bptc_basis().astype(np.int64)) & 1).astype(np.uint8)


# ---- the trellises, over many blocks ---------------------------------------------------------------------------------------------

P25_BRANCH = np.array([[(a << 2 | b) for a, b in (PM.TRELLIS_PAIRS[PM.TRELLIS_POINTS[i][j]] for j in range(4))] for i in range(4)], dtype=np.int64)
P25_COST = np.bitwise_count((np.arange(16)[:, None, None] ^ P25_BRANCH[None, :, :]).astype(np.uint8)).astype(np.int64)  # [rx][from][input]
P25_ORDER = np.array(PM.INTERLEAVE, dtype=np.int64)  # coded dibit n is sent dibit P25_ORDER[n]


def p25_trellis_encode_batch(dibits48) -> np.ndarray:
    """uint8[K][98] as sent of uint8[K][48]: ``p25_model.trellis_encode`` over many blocks."""
    d = np.concatenate([np.asarray(dibits48, dtype=np.int64), np.zeros((len(dibits48), 1), dtype=np.int64)], axis=1)
    state = np.concatenate([np.zeros((d.shape[0], 1), dtype=np.int64), d[:, :-1]], axis=1)
    pairs = np.array(PM.TRELLIS_PAIRS, dtype=np.uint8)[np.array(PM.TRELLIS_POINTS, dtype=np.int64)[state, d]]  # [K][49][2]
    sent = np.zeros((d.shape[0], 98), dtype=np.uint8)
    sent[:, P25_ORDER] = pairs.reshape(d.shape[0], 98)
    return sent


def p25_trellis_reference(sent98) -> tuple:
    """(dibits uint8[K][48], metric, ties on the surviving path) of uint8[K][98] as sent: the batch form of
    ``p25_model.trellis_decode``; on equal metric the smaller predecessor survives (``argmin`` gives the first minimum)."""
    coded = np.asarray(sent98, dtype=np.int64)[:, P25_ORDER]
    rx = coded[:, 0::2] << 2 | coded[:, 1::2]
    k = rx.shape[0]
    metric = np.full((k, 4), FAR, dtype=np.int64)
    metric[:, 0] = 0
    back, tied = np.empty((49, k, 4), dtype=np.int64), np.empty((49, k, 4), dtype=bool)
    for t in range(49):
        cost = metric[:, :, None] + P25_COST[rx[:, t]]  # [K][from][input]
        metric = cost.min(axis=1)
        back[t] = cost.argmin(axis=1)
        tied[t] = (cost == metric[:, None, :]).sum(axis=1) > 1
    rows, state = np.arange(k), np.zeros(k, dtype=np.int64)
    inputs, ties = np.empty((k, 49), dtype=np.uint8), np.zeros(k, dtype=np.int64)
    for t in range(48, -1, -1):
        inputs[:, t] = state
        ties += tied[t][rows, state]
        state = back[t][rows, state]
    return inputs[:, :48], metric[:, 0], ties


def conv_encode_batch(bits) -> np.ndarray:
    """uint8[K][2 n] of uint8[K][n] (the tail bits included): g1 = d ^ d3 ^ d4 at 2 t, g2 = d ^ d1 ^ d2 ^ d4 at 2 t + 1: the
    models' ``conv_encode`` over many blocks, without the four zeros it appends."""
    bits = np.asarray(bits, dtype=np.uint8)
    k, n = bits.shape
    pad = np.zeros((k, n + 4), dtype=np.uint8)
    pad[:, 4:] = bits
    d, d1, d2, d3, d4 = pad[:, 4:], pad[:, 3:-1], pad[:, 2:-2], pad[:, 1:-3], pad[:, :-4]
    out = np.empty((k, 2 * n), dtype=np.uint8)
    out[:, 0::2], out[:, 1::2] = d ^ d3 ^ d4, d ^ d1 ^ d2 ^ d4
    return out


_S = np.arange(16)
_PREV = np.stack([(_S & 7) << 1, (_S & 7) << 1 | 1])  # [2][16]: the two predecessors of a state, the smaller first
_G1 = (_S >> 3) ^ (_PREV >> 1 & 1) ^ (_PREV & 1)
_G2 = (_S >> 3) ^ (_PREV >> 3 & 1) ^ (_PREV >> 2 & 1) ^ (_PREV & 1)


def viterbi16_reference(coded, sent=None) -> tuple:
    """(bits uint8[K][steps] with the tail, metric, ties on the surviving path) of the coded bits uint8[K][2 steps]; ``sent``
    bool[2 steps]: which of them were sent (a punctured bit costs nothing on either branch; None: all).  The batch form of
    ``ysf_model.viterbi`` and ``nxdn_model.viterbi`` with the specification's tie rule: the smaller predecessor survives."""
    coded = np.asarray(coded, dtype=np.int64)
    k, steps = coded.shape[0], coded.shape[1] // 2
    sent = np.ones(2 * steps, dtype=bool) if sent is None else np.asarray(sent, dtype=bool)
    metric = np.full((k, 16), FAR, dtype=np.int64)
    metric[:, 0] = 0
    back, tied = np.empty((steps, k, 16), dtype=bool), np.empty((steps, k, 16), dtype=bool)
    for t in range(steps):
        cost = metric[:, _PREV]  # [K][2][16]
        if sent[2 * t]:
            cost = cost + (coded[:, 2 * t, None, None] != _G1)
        if sent[2 * t + 1]:
            cost = cost + (coded[:, 2 * t + 1, None, None] != _G2)
        back[t] = cost[:, 1] < cost[:, 0]
        tied[t] = cost[:, 1] == cost[:, 0]
        metric = np.where(back[t], cost[:, 1], cost[:, 0])
    rows, state = np.arange(k), np.zeros(k, dtype=np.int64)
    bits, ties = np.empty((k, steps), dtype=np.uint8), np.zeros(k, dtype=np.int64)
    for t in range(steps - 1, -1, -1):
        bits[:, t] = state >> 3
        ties += tied[t][rows, state]
        state = (state & 7) << 1 | back[t][rows, state]
    return bits, metric[:, 0], ties


# ---- where the codes lie in the records (the models' layouts, as index arrays) ------------------------------------------------------

P25_BITS, DMR_BITS, YSF_BITS, NXDN_BITS = 32 * PM.WORDS, 288, 32 * YM.WORDS, 32 * NM.WORDS
P25_NID_AT = np.array([PM.frame_bit_of(48 + j) for j in range(64)])
P25_GOLAY_AT = np.array([[PM.frame_bit_of(112 + 24 * w + k) for k in range(24)] for w in range(12)])
P25_HAMMING_AT = np.array([[PM.frame_bit_of(400 + 184 * (w // 4) + 10 * (w % 4) + k) for k in range(10)] for w in range(24)])
P25_TRELLIS_AT = np.array([[PM.frame_bit_of(112 + 196 * b + k) for k in range(196)] for b in range(3)])
DMR_TACT_AT = np.array(DM.TACT_BITS)
DMR_SLOT_AT = 24 + np.array(DM.SLOT_TYPE_BITS)
DMR_PAYLOAD_AT = 24 + np.array(DM.PAYLOAD_BITS)
YSF_FICH_AT = np.array([40 + 2 * YM.interleave_at(c >> 1, 5) + (c & 1) for c in range(200)])  # of coded bit c
YSF_STEPS = {1: 180, 2: 180, 3: 100}


@functools.lru_cache(maxsize=None)
def ysf_dch_at(cls: int, second: bool) -> np.ndarray:
    """The frame bit of every coded bit of a data channel."""
    return np.array([YM.coded_frame_bit(cls, second, c) for c in range(2 * YSF_STEPS[cls])])


@functools.lru_cache(maxsize=None)
def nxdn_at(kind: str, first: int) -> np.ndarray:
    """The frame bit of every coded bit of a block, -1 where it is punctured."""
    out, p = [], 0
    for j in range(2 * NM.BLOCKS[kind][0]):
        if NM.punctured(j, kind):
            out.append(-1)
        else:
            out.append(first + NM.channel_index(p, kind))
            p += 1
    return np.array(out)


# ---- the decoders of whole records: the batch forms of the models' decode_frame / decode_burst -------------------------------------


def p25_nid_reference(words) -> np.ndarray:
    """int32[K][4]: the batch form of ``p25_model.nid_all``."""
    return nid_reference(bits_of_words(words)[:, P25_NID_AT])


def p25_golay_records(value, dist, refused) -> tuple:
    """(info uint32[K][9], rec int32[K][8]) of a TDULC's twelve words (each [K][12])."""
    k = value.shape[0]
    bits = np.zeros((k, 288), dtype=np.uint8)
    bits[:, :144] = bits_of_int(value, 12).reshape(k, 144)
    fixed = (dist > 0) & ~refused
    rec = np.zeros((k, 8), dtype=np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = 2, fixed.sum(axis=1), refused.sum(axis=1), (dist * fixed).sum(axis=1)
    return words_of_bits(bits), rec


def p25_hamming_records(six, flag) -> tuple:
    """(info, rec) of an LDU1's 24 words (six [K][24][6], flag [K][24])."""
    k = six.shape[0]
    bits = np.zeros((k, 288), dtype=np.uint8)
    bits[:, :144] = six.reshape(k, 144)
    rec = np.zeros((k, 8), dtype=np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2] = 1, (flag == 1).sum(axis=1), (flag == 2).sum(axis=1)
    rec[:, 3] = rec[:, 1]
    return words_of_bits(bits), rec


def p25_trellis_records(dibits, metric) -> tuple:
    """(info, rec) of a TSBK frame's three blocks (dibits [K][3][48], metric [K][3])."""
    k = dibits.shape[0]
    bits = np.stack([dibits >> 1, dibits & 1], axis=3).reshape(k, 288).astype(np.uint8)
    rec = np.zeros((k, 8), dtype=np.int32)
    rec[:, 0], rec[:, 1:4] = 3, metric
    return words_of_bits(bits), rec


def p25_reference(words, duids) -> tuple:
    """(info uint32[K][9], rec int32[K][8]): the batch form of ``p25_model.decode_all``."""
    frame, duids = bits_of_words(words), np.asarray(duids, dtype=np.int64) & 15
    k = frame.shape[0]
    info, rec = np.zeros((k, 9), dtype=np.uint32), np.zeros((k, 8), dtype=np.int32)
    at = np.flatnonzero(duids == 0xF)
    if at.size:
        dist, value, refused = golay_reference(int_of_bits(frame[at][:, P25_GOLAY_AT]).reshape(-1).astype(np.uint32))
        info[at], rec[at] = p25_golay_records(value.reshape(-1, 12), dist.reshape(-1, 12), refused.reshape(-1, 12))
    at = np.flatnonzero(duids == 0x5)
    if at.size:
        info[at], rec[at] = p25_hamming_records(*hamming10_reference(frame[at][:, P25_HAMMING_AT]))
    at = np.flatnonzero(duids == 0x7)
    if at.size:
        two = frame[at][:, P25_TRELLIS_AT].reshape(-1, 98, 2)
        dibits, metric, _ = p25_trellis_reference(two[:, :, 0] << 1 | two[:, :, 1])
        info[at], rec[at] = p25_trellis_records(dibits.reshape(-1, 3, 48), metric.reshape(-1, 3))
    return info, rec


def dmr_reference(words, kinds) -> tuple:
    """(info uint32[K][3], rec int32[K][8]): the batch form of ``dmr_model.decode_all``."""
    frame, kinds = bits_of_words(words), np.asarray(kinds, dtype=np.int64) & 3
    k = frame.shape[0]
    info, rec = np.zeros((k, 96), dtype=np.uint8), np.tile(np.array([4, 0, 4, 0, 0, 4, 0, 0], dtype=np.int32), (k, 1))
    at = np.flatnonzero(kinds < 2)
    if at.size:
        rec[at, 0], rec[at, 1] = tact_reference(frame[at][:, DMR_TACT_AT])
    at = np.flatnonzero(kinds & 1)
    if at.size:
        dist, value, refused = golay_reference(int_of_bits(frame[at][:, DMR_SLOT_AT]).astype(np.uint32), GOLAY20)
        rec[at, 2], rec[at, 3], rec[at, 4] = np.where(dist == 0, 0, np.where(refused, 2, 1)), dist, value
        at = at[~refused]
        if at.size:
            rec[at, 5], rec[at, 6], rec[at, 7], info[at] = bptc_reference(frame[at][:, DMR_PAYLOAD_AT])
    return words_of_bits(info), rec


def ysf_fich_records(value, dist, refused, metric) -> tuple:
    """(fich uint32[K][2], rec int32[K][5]) of a FICH's four words (each [K][4]) behind a trellis of that metric."""
    k = value.shape[0]
    bits = np.zeros((k, 64), dtype=np.uint8)
    bits[:, :48] = bits_of_int(value, 12).reshape(k, 48)
    fixed = (dist > 0) & ~refused
    rec = np.zeros((k, 5), dtype=np.int32)
    rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4] = metric, fixed.sum(axis=1), refused.sum(axis=1), (dist * fixed).sum(axis=1)
    rec[:, 0] = np.where(rec[:, 3] > 0, 2, np.where((rec[:, 1] > 0) | (rec[:, 2] > 0), 1, 0))
    return words_of_bits(bits), rec


def ysf_fich_reference(words) -> tuple:
    """(fich, rec, ties, the 100 decoded bits): the batch form of ``ysf_model.fich_all``."""
    decoded, metric, ties = viterbi16_reference(bits_of_words(words)[:, YSF_FICH_AT])
    dist, value, refused = golay_reference(int_of_bits(decoded[:, :96].reshape(-1, 24)).astype(np.uint32), GOLAY24_YSF)
    return ysf_fich_records(value.reshape(-1, 4), dist.reshape(-1, 4), refused.reshape(-1, 4), metric) + (ties, decoded)


def ysf_reference(words, classes) -> tuple:
    """(info uint32[K][12], rec int32[K][4], ties [K][2]): the batch form of ``ysf_model.decode_all``."""
    frame, classes = bits_of_words(words), np.asarray(classes, dtype=np.int64)
    k = frame.shape[0]
    bits, rec, ties = np.zeros((k, 384), dtype=np.uint8), np.zeros((k, 4), dtype=np.int32), np.zeros((k, 2), dtype=np.int64)
    for cls in (1, 2, 3):
        at = np.flatnonzero(classes == cls)
        if not at.size:
            continue
        rec[at, 0] = cls
        for second in ((False, True) if cls == 1 else (False,)):
            decoded, metric, tie = viterbi16_reference(frame[at][:, ysf_dch_at(cls, second)])
            bits[at, 192 * second : 192 * second + decoded.shape[1]] = decoded
            rec[at, 1 + second], ties[at, int(second)] = metric, tie
    return words_of_bits(bits), rec, ties


def nxdn_reference(words, masks) -> tuple:
    """(info uint32[K][14], rec int32[K][4], ties [K][4] by record slot): the batch form of ``nxdn_model.decode_all``."""
    frame, masks = bits_of_words(words), np.asarray(masks, dtype=np.int64)
    masks = np.where((masks <= 7) | (masks == 8), masks, 0)
    k = frame.shape[0]
    bits, rec, ties = np.zeros((k, 32 * NM.INFO), dtype=np.uint8), np.zeros((k, 4), dtype=np.int32), np.zeros((k, 4), dtype=np.int64)
    rec[:, 0] = masks
    for bit, kind, first, word, _count, slot in NM.LAYOUT:
        at = np.flatnonzero(masks & bit)
        if not at.size:
            continue
        where = nxdn_at(kind, first)
        decoded, metric, tie = viterbi16_reference(frame[at][:, np.maximum(where, 0)], where >= 0)
        bits[at, 32 * word : 32 * word + decoded.shape[1]] = decoded
        rec[at, slot], ties[at, slot] = metric, tie
    return words_of_bits(bits), rec, ties


# ---- the sweeps: whole codebooks ---------------------------------------------------------------------------------------------------


def _frames_to_words(frame) -> np.ndarray:
    out = words_of_bits(frame)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=1)
def nid_codebook(seed: int = SEED) -> dict:
    """All 65 536 (NAC, DUID) values, clean, and the same with the parity bit flipped."""
    rng = np.random.default_rng(seed)
    values = np.arange(65536)
    frame = random_frames(rng, 65536, P25_BITS)
    frame[:, P25_NID_AT] = nid_bits(values)
    words = _frames_to_words(frame)
    frame[:, P25_NID_AT[63]] ^= 1
    return dict(values=values, words=words, words_parity=_frames_to_words(frame))


def _fill(values, multiple: int) -> np.ndarray:
    """``values`` with zeros behind them up to a multiple."""
    values = np.asarray(values)
    return np.concatenate([values, np.zeros((-values.size) % multiple, dtype=values.dtype)])


@functools.lru_cache(maxsize=1)
def p25_golay_codebook(seed: int = SEED) -> dict:
    """All 4096 data words, twelve to a TDULC: data d lies at the word position d mod 12."""
    data = _fill(np.arange(4096), 12).reshape(-1, 12)
    return _p25_golay_frames(np.random.default_rng(seed), data, np.zeros_like(data))


def _p25_golay_frames(rng, data, pattern) -> dict:
    """TDULC records whose word [f][w] is the codeword of data[f][w] with the 24-bit error pattern[f][w] on it."""
    sent = GOLAY24[data] ^ pattern.astype(np.uint32)
    frame = random_frames(rng, data.shape[0], P25_BITS)
    frame[:, P25_GOLAY_AT] = bits_of_int(sent, 24)
    return dict(data=data, pattern=pattern, sent=sent, words=_frames_to_words(frame), duids=np.full(data.shape[0], 0xF, dtype=np.uint8))


@functools.lru_cache(maxsize=1)
def ysf_fich_codebook(seed: int = SEED) -> dict:
    """All 4096 data words, four to a FICH: data d lies in the slot d mod 4."""
    data = np.arange(4096).reshape(-1, 4)
    return _ysf_golay_frames(np.random.default_rng(seed), data, np.zeros_like(data))


def _ysf_golay_frames(rng, data, pattern) -> dict:
    """Records whose FICH word [f][j] is the codeword of data[f][j] with pattern[f][j] on it *in front of* the convolutional
    coder: the trellis returns it with metric 0."""
    sent = GOLAY24_YSF[data] ^ pattern.astype(np.uint32)
    message = np.zeros((data.shape[0], 100), dtype=np.uint8)
    message[:, :96] = bits_of_int(sent, 24).reshape(-1, 96)
    frame = random_frames(rng, data.shape[0], YSF_BITS)
    frame[:, YSF_FICH_AT] = conv_encode_batch(message)
    return dict(data=data, pattern=pattern, sent=sent, words=_frames_to_words(frame))


def _dmr_frames(rng, count: int, kind: int, tact=None, slot=None, raw=None) -> np.ndarray:
    """uint8[count][288]: random bursts with the given TACT (uint8[count][7]), slot type (the 20 bits) and payload (the 196 bits)."""
    frame = random_frames(rng, count, DMR_BITS)
    if tact is not None:
        frame[:, DMR_TACT_AT] = tact
    if slot is not None:
        frame[:, DMR_SLOT_AT] = slot
    if raw is not None:
        frame[:, DMR_PAYLOAD_AT] = raw
    return frame


@functools.lru_cache(maxsize=1)
def dmr_slot_codebook(seed: int = SEED) -> dict:
    """All 256 slot-type bytes, clean, each over a clean payload of its own."""
    rng = np.random.default_rng(seed)
    data, info = np.arange(256), rng.integers(0, 2, (256, 96), dtype=np.uint8)
    frame = _dmr_frames(rng, 256, 1, slot=bits_of_int(GOLAY20[data], 20), raw=bptc_encode_batch(info))
    return dict(data=data, info=info, words=_frames_to_words(frame), kinds=np.ones(256, dtype=np.uint8))


@functools.lru_cache(maxsize=1)
def dmr_tact_codebook(seed: int = SEED) -> dict:
    """All 128 seven-bit TACT words on voice bursts of a base station (kind 0): every one is a codeword or one bit from one."""
    rng = np.random.default_rng(seed)
    seven = bits_of_int(np.arange(128), 7)
    return dict(seven=seven, words=_frames_to_words(_dmr_frames(rng, 128, 0, tact=seven)), kinds=np.zeros(128, dtype=np.uint8))


@functools.lru_cache(maxsize=1)
def p25_hamming_sweep(seed: int = SEED) -> dict:
    """All 1024 ten-bit words at each of the 24 positions of an LDU1: frame f holds the word (f + 43 p) mod 1024 at position p."""
    rng = np.random.default_rng(seed)
    ten = (np.arange(1024)[:, None] + 43 * np.arange(24)[None, :]) % 1024
    frame = random_frames(rng, 1024, P25_BITS)
    frame[:, P25_HAMMING_AT] = bits_of_int(ten, 10)
    return dict(ten=ten, words=_frames_to_words(frame), duids=np.full(1024, 0x5, dtype=np.uint8))


# ---- the sweeps: every pattern up to the guarantee, and one beyond ------------------------------------------------------------------


def _golay_words(rng, bits: int, data_bits: int, low_count: int, four_count: int) -> tuple:
    """(data, pattern): ``low_count`` random data words under every pattern of weight 1 .. 3, ``four_count`` under every one of weight 4."""
    low, four = int_of_bits(patterns(bits, 1, 3)).astype(np.int64), int_of_bits(patterns(bits, 4, 4)).astype(np.int64)
    picks = rng.choice(1 << data_bits, low_count + four_count, replace=False)
    data = np.concatenate([np.repeat(picks[:low_count], low.size), np.repeat(picks[low_count:], four.size)])
    return data, np.concatenate([np.tile(low, low_count), np.tile(four, four_count)])


@functools.lru_cache(maxsize=1)
def golay24_pattern_words(seed: int = SEED) -> tuple:
    """(data, pattern) int64[39844]: 8 data words under all 2324 patterns of weight 1 .. 3, 2 under all 10 626 of weight 4."""
    return _golay_words(np.random.default_rng(seed), 24, 12, 8, 2)


@functools.lru_cache(maxsize=1)
def p25_golay_patterns(seed: int = SEED) -> dict:
    data, pattern = golay24_pattern_words(seed)
    order = np.random.default_rng(seed + 1).permutation(_fill(data, 12).size)  # (a frame holds words of every weight, so rec sums mix)
    return _p25_golay_frames(np.random.default_rng(seed + 2), _fill(data, 12)[order].reshape(-1, 12), _fill(pattern, 12)[order].reshape(-1, 12))


@functools.lru_cache(maxsize=1)
def ysf_golay_patterns(seed: int = SEED) -> dict:
    data, pattern = golay24_pattern_words(seed)
    data, pattern = np.concatenate([data, data[:1]]), np.concatenate([pattern, pattern[:1]])  # 39 845 words: 9961 frames and one over
    order = np.random.default_rng(seed + 1).permutation(_fill(data, 4).size)
    return _ysf_golay_frames(np.random.default_rng(seed + 2), _fill(data, 4)[order].reshape(-1, 4), _fill(pattern, 4)[order].reshape(-1, 4))


@functools.lru_cache(maxsize=1)
def dmr_golay_patterns(seed: int = SEED) -> dict:
    """16 slot-type bytes under all 1350 patterns of weight 1 .. 3 and 2 under all 4845 of weight 4, over one clean payload."""
    rng = np.random.default_rng(seed)
    data, pattern = _golay_words(rng, 20, 8, 16, 2)
    info = rng.integers(0, 2, (1, 96), dtype=np.uint8)
    sent = GOLAY20[data] ^ pattern.astype(np.uint32)
    frame = _dmr_frames(rng, data.size, 1, slot=bits_of_int(sent, 20), raw=bptc_encode_batch(info))
    return dict(data=data, pattern=pattern, sent=sent, info=info[0], words=_frames_to_words(frame), kinds=np.ones(data.size, dtype=np.uint8))


def golay_expected(data, pattern, sent) -> tuple:
    """(distance, data, refused) by the code's algebra alone: the codewords lie 8 apart, so a word 1 .. 3 from one is restored, and
    a word 4 from one is 4 from the nearest and is refused with the bits above its check bits kept.  Weight 0 .. 4 only."""
    weight = np.bitwise_count(np.asarray(pattern).astype(np.uint32)).astype(np.int64)
    assert weight.max() <= 4
    return weight, np.where(weight == 4, (np.asarray(sent) >> 12).astype(np.int64), data), weight == 4


@functools.lru_cache(maxsize=1)
def nid_patterns(seed: int = SEED) -> dict:
    """For each weight 1 .. 11, 256 random (codeword, pattern) pairs, the codewords from the whole book; then 2048 random patterns
    of weight 12 .. 16.  The patterns lie on the 63 code bits; the parity bit is the codeword's.  A pattern drawn from all 63
    bits nearly never comes within 11 of another codeword (6 of 2048 did), so every other one of the 2048 is drawn from the bits
    of a random codeword of weight 23 .. weight + 11: it leaves the word at most 11 from the sent codeword plus that one."""
    rng = np.random.default_rng(seed)
    weight = np.concatenate([np.repeat(np.arange(1, 12), 256), rng.integers(12, 17, 2048)])
    values = rng.integers(0, 65536, weight.size)
    pattern = np.concatenate([random_patterns(rng, 63, weight), np.zeros((weight.size, 1), dtype=np.uint8)], axis=1)
    book = PM.bch_codewords()
    heavy = np.bitwise_count(book).astype(np.int64)
    for k in range(11 * 256, weight.size, 2):
        toward = rng.choice(np.flatnonzero((heavy >= 23) & (heavy <= weight[k] + 11)))
        pattern[k] = 0
        pattern[k, rng.choice(np.flatnonzero(bits_of_int(book[toward], 63)), weight[k], replace=False)] = 1
    bits = nid_bits(values) ^ pattern
    frame = random_frames(rng, weight.size, P25_BITS)
    frame[:, P25_NID_AT] = bits
    return dict(values=values, weight=weight, pattern=pattern, bits=bits, words=_frames_to_words(frame), guaranteed=weight <= 11)


@functools.lru_cache(maxsize=1)
def bptc_singles(seed: int = SEED) -> dict:
    """64 random messages, each with all 196 single flips of its payload, under a clean slot type."""
    rng = np.random.default_rng(seed)
    info = np.repeat(rng.integers(0, 2, (64, 96), dtype=np.uint8), 196, axis=0)
    flip = np.tile(np.arange(196), 64)
    raw = bptc_encode_batch(info)
    raw[np.arange(flip.size), flip] ^= 1
    frame = _dmr_frames(rng, flip.size, 1, slot=bits_of_int(GOLAY20[rng.integers(0, 256, flip.size)], 20), raw=raw)
    return dict(info=info, flip=flip, raw=raw, words=_frames_to_words(frame), kinds=np.ones(flip.size, dtype=np.uint8))


@functools.lru_cache(maxsize=1)
def bptc_random(seed: int = SEED) -> dict:
    """4000 random (message, pattern) pairs of weight 2 .. 12, under a clean slot type."""
    rng = np.random.default_rng(seed)
    info = rng.integers(0, 2, (4000, 96), dtype=np.uint8)
    weight = rng.integers(2, 13, 4000)
    pattern = random_patterns(rng, 196, weight)
    raw = bptc_encode_batch(info) ^ pattern
    frame = _dmr_frames(rng, 4000, 1, slot=bits_of_int(GOLAY20[rng.integers(0, 256, 4000)], 20), raw=raw)
    return dict(info=info, weight=weight, pattern=pattern, raw=raw, words=_frames_to_words(frame), kinds=np.ones(4000, dtype=np.uint8))


# ---- the sweeps: dense errors through every trellis ------------------------------------------------------------------------------------


def trellis_block(rng, count: int, message, sent) -> dict:
    """``count`` blocks of the K = 5 code: ``message`` uint8[count][steps] (the four tail zeros included), ``sent`` bool[2 steps]
    which coded bits are sent; the flips per block uniform in 0 .. DENSITY * (sent bits), on sent bits only.  ``coded`` is what
    arrives (a punctured bit reads 0)."""
    sent = np.asarray(sent, dtype=bool)
    flips = rng.integers(0, int(DENSITY * sent.sum()) + 1, count)
    pattern = np.zeros((count, sent.size), dtype=np.uint8)
    pattern[:, sent] = random_patterns(rng, int(sent.sum()), flips)
    coded = (conv_encode_batch(message) ^ pattern) * sent.astype(np.uint8)
    return dict(message=message, sent=sent, flips=flips, pattern=pattern, coded=coded, steps=sent.size // 2)


def _random_message(rng, count: int, steps: int) -> np.ndarray:
    out = rng.integers(0, 2, (count, steps), dtype=np.uint8)
    out[:, steps - 4 :] = 0
    return out


FRAMES = 1025  # blocks of a class in a trellis sweep: over 1024, and odd


@functools.lru_cache(maxsize=1)
def ysf_fich_trellis(seed: int = SEED, count: int = FRAMES) -> dict:
    """Records whose FICH is four codewords of random data, with dense flips behind the convolutional coder.  1025 frames: the last
    wave of four holds one."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 4096, (count, 4))
    message = np.zeros((count, 100), dtype=np.uint8)
    message[:, :96] = bits_of_int(GOLAY24_YSF[data], 24).reshape(count, 96)
    block = trellis_block(rng, count, message, np.ones(200, dtype=bool))
    frame = random_frames(rng, count, YSF_BITS)
    frame[:, YSF_FICH_AT] = block["coded"]
    return dict(data=data, words=_frames_to_words(frame), blocks={"fich": dict(block, rows=np.arange(count))})


@functools.lru_cache(maxsize=1)
def ysf_dch_trellis(seed: int = SEED, count: int = 3 * FRAMES + 2) -> dict:
    """Records of the classes 1, 2, 3 in turn (so every pair of classes shares a wave, and the last wave holds one frame), every
    data channel a random message with dense flips of its own."""
    rng = np.random.default_rng(seed)
    classes = (1 + np.arange(count) % 3).astype(np.uint8)
    frame = random_frames(rng, count, YSF_BITS)
    blocks = {}
    for cls, second in ((1, False), (1, True), (2, False), (3, False)):
        rows = np.flatnonzero(classes == cls)
        steps = YSF_STEPS[cls]
        block = trellis_block(rng, rows.size, _random_message(rng, rows.size, steps), np.ones(2 * steps, dtype=bool))
        frame[rows[:, None], ysf_dch_at(cls, second)[None, :]] = block["coded"]
        blocks[f"class{cls}-{'b' if second else 'a'}"] = dict(block, rows=rows, first_bit=192 * second, slot=1 + second)
    return dict(classes=classes, words=_frames_to_words(frame), blocks=blocks)


#: the block classes of the NXDN sweep: name -> (the mask of its frames, the kind, the first frame bit, the first info word, the record slot)
NXDN_CLASSES = {"sacch-alone": (1, "sacch", 36, 0, 1), "sacch-with": (7, "sacch", 36, 0, 1), "facch1-a-with": (7, "facch1", 96, 2, 2),
                "facch1-b-with": (7, "facch1", 240, 5, 3), "facch1-a-alone": (2, "facch1", 96, 2, 2), "facch1-b-alone": (4, "facch1", 240, 5, 3),
                "cac": (8, "cac", 36, 8, 1)}


@functools.lru_cache(maxsize=1)
def nxdn_trellis(seed: int = SEED, count: int = 5 * FRAMES) -> dict:
    """Records of the masks 1, 7, 2, 4, 8 in turn, every block a random message with dense flips of its own: the three blocks of a
    mask 7 share a wave."""
    rng = np.random.default_rng(seed)
    masks = np.array([1, 7, 2, 4, 8], dtype=np.uint8)[np.arange(count) % 5]
    frame = random_frames(rng, count, NXDN_BITS)
    blocks = {}
    for name, (mask, kind, first, word, slot) in NXDN_CLASSES.items():
        rows = np.flatnonzero(masks == mask)
        at = nxdn_at(kind, first)
        block = trellis_block(rng, rows.size, _random_message(rng, rows.size, at.size // 2), at >= 0)
        frame[rows[:, None], at[at >= 0][None, :]] = block["coded"][:, at >= 0]
        blocks[name] = dict(block, rows=rows, first_bit=32 * word, slot=slot)
    return dict(masks=masks, words=_frames_to_words(frame), blocks=blocks)


@functools.lru_cache(maxsize=1)
def p25_trellis(seed: int = SEED, count: int = FRAMES) -> dict:
    """TSBK records of three blocks, every block 48 random dibits with 0 .. 29 flips among its 196 bits."""
    rng = np.random.default_rng(seed)
    frame = random_frames(rng, count, P25_BITS)
    blocks = {}
    for b in range(3):
        dibits = rng.integers(0, 4, (count, 48), dtype=np.uint8)
        clean = p25_trellis_encode_batch(dibits)
        flips = rng.integers(0, int(DENSITY * 196) + 1, count)
        pattern = random_patterns(rng, 196, flips)
        bits = np.stack([clean >> 1, clean & 1], axis=2).reshape(count, 196) ^ pattern
        frame[:, P25_TRELLIS_AT[b]] = bits
        blocks[f"block-{b}"] = dict(message=dibits, flips=flips, pattern=pattern, bits=bits, rows=np.arange(count), steps=49)
    return dict(duids=np.full(count, 0x7, dtype=np.uint8), words=_frames_to_words(frame), blocks=blocks)


def p25_flip_steps(pattern) -> np.ndarray:
    """bool[K][49]: the trellis steps that a pattern over a block's 196 bits touches."""
    step_of_dibit = np.empty(98, dtype=np.int64)
    step_of_dibit[P25_ORDER] = np.arange(98) // 2
    out = np.zeros((pattern.shape[0], 49), dtype=bool)
    for bit in range(196):
        out[:, step_of_dibit[bit >> 1]] |= pattern[:, bit].astype(bool)
    return out


def conv_flip_steps(pattern) -> np.ndarray:
    """bool[K][steps]: the trellis steps that a pattern over a block's coded bits touches."""
    return (pattern[:, 0::2] | pattern[:, 1::2]).astype(bool)
