"""The checks that more than one protocol layer runs (``protocol_layer.crc_ccitt``, ``info_bytes``, ``gf_tables``), without a GPU:
the table form of the CRC against the bitwise form written out here, the fields against their definition."""
from __future__ import annotations

import random
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from iq_to_audio_amd import dmr, p25, ysf  # noqa: E402
from iq_to_audio_amd import protocol_layer as L  # noqa: E402


def bitwise_crc(data) -> int:
    """CRC-CCITT bit by bit: polynomial 0x1021 from 0, eight shifts per byte."""
    crc = 0
    for byte in data:
        crc ^= int(byte) << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def test_the_table_crc_equals_the_bitwise_crc():
    assert all(L.crc_ccitt([b]) == bitwise_crc([b]) for b in range(256))
    rng = random.Random(1021)
    for _ in range(1000):
        data = [rng.randrange(256) for _ in range(12)]
        assert L.crc_ccitt(data) == bitwise_crc(data), data
    assert L.crc_ccitt(b"123456789") == 0x31C3 and L.crc_ccitt(b"") == 0 and L.CRC_POLY == 0x1021
    assert dmr.crc_ccitt is p25.crc_ccitt is ysf.crc_ccitt is L.crc_ccitt


def test_info_bytes():
    assert L.info_bytes([0x01020304, 0xFFFEFDFC, 0x80000001]) == [1, 2, 3, 4, 0xFF, 0xFE, 0xFD, 0xFC, 0x80, 0, 0, 1] and L.info_bytes([]) == []
    assert dmr.info_bytes is p25.info_bytes is ysf.info_bytes is L.info_bytes


def slow_mul(a: int, b: int, poly: int, bits: int) -> int:
    """The product in GF(2^bits) modulo ``poly`` by shift and add."""
    out = 0
    while b:
        if b & 1:
            out ^= a
        a <<= 1
        if a >> bits:
            a ^= poly
        b >>= 1
    return out


def test_gf_tables():
    for poly, bits, module in ((0x11D, 8, dmr), (0x43, 6, p25)):
        size = (1 << bits) - 1
        exp, log, mul = L.gf_tables(poly, bits)
        assert (exp, log) == (module._EXP, module._LOG) and len(exp) == 2 * size and len(log) == size + 1
        assert sorted(exp[:size]) == list(range(1, size + 1)) and exp[size:] == exp[:size] and all(exp[log[x]] == x for x in range(1, size + 1))
        assert all(mul(a, b) == module.gf_mul(a, b) == slow_mul(a, b, poly, bits) for a in range(size + 1) for b in range(size + 1))
