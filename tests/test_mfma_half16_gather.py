"""The tap gather of the 16x16x64 tile body (csrc/channelize_ring.hip, ring_main_h16), restated in NumPy.

The half-step kernels (k_channelize_mfma_s16_ring_multi_half<KS>, KS = 1..8) take their tap operands out of the planner's
fragments, which are laid out for v_mfma_i32_32x32x32_i8 (lane l of a k step: tap row l & 31, values 16 (l >> 5) .. + 15).
For chunk c of 64 values, tap-row half bi and lane l the operand of v_mfma_i32_16x16x64_i8 is the 16 bytes of k step
2 c + (l >> 5), lane 16 bi + (l & 15) + 32 ((l >> 4) & 1); an odd last k step is a v_mfma_i32_16x16x32_i8 whose operand is
half a fragment: lane 16 bi + (l & 15) + 32 (l >> 5), bytes 8 ((l >> 4) & 1) .. + 7.  The instruction wants, in lane l,
tap row 16 bi + (l & 15), values 64 c + 16 (l >> 4) .. + 15 (or 32 (KS - 1) + 8 (l >> 4) .. + 7): for every (KS, row tile,
chunk, bi, piece, lane) the gathered bytes must be q1 / q2 of ``plan.tq`` at that row and those values.
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import mfma_dispatch as X


def _plan(d: int):
    from iq_to_audio_amd import dsp_plan as P

    L = 64 * d - d // 3 - 1
    rng = np.random.default_rng(d)
    g = (rng.uniform(-1.0, 1.0, L) + 1j * rng.uniform(-1.0, 1.0, L)) * P.INGEST_SCALE["s16"]
    plan = P.ChannelPlan(fmt="s16", ntaps=L, decimation=d, taps_window=None, conj_sum=0, rotate=0, rot_step=0, rot_base=0,
                         out_scale=1.0 + 0j, taps_natural=g)
    return P.plan_mfma(plan, acc32=True)


def _pieces(tq: np.ndarray):
    """T = 256 q1 + q2, both bytes signed."""
    q2 = ((tq + 128) & 255) - 128
    q1 = (tq - q2) >> 8
    assert np.array_equal(256 * q1 + q2, tq) and np.abs(q1).max() <= 128
    return q1.astype(np.int8), q2.astype(np.int8)


HALF_D = [d for _, ks, d in X.sweep_cases() if _ == "multi_half"] + [4, 100, 104, 116]


@pytest.mark.parametrize("d", sorted(set(HALF_D)))
def test_gathered_tap_operands_are_the_plans_taps(d):
    ks = -(-2 * d // 32)
    assert X.expected_kernel("multi", "s16", d, 0, ks, False, False) == f"k_channelize_mfma_s16_ring_multi_half<{ks}>"
    mp = _plan(d)
    grp = mp.groups[0]
    afrag = grp.afrag  # [ksteps, row tile 4, piece 2, lane 64, 16]
    assert afrag.shape == (ks, 4, 2, 64, 16)
    q = _pieces(grp.tq)  # [128, 32 ks] each
    assert np.any(q[1]), "full taps: the low byte is in use"
    assert not np.any(grp.tq[:, 2 * d:]), "the K padding holds zero taps"
    lane = np.arange(64)
    r16, g = lane & 15, lane >> 4
    j16, j8 = np.arange(16), np.arange(8)
    seen = np.zeros((2, 128, 32 * ks), dtype=np.int32)  # how often a tap byte reaches a matrix instruction
    for rt in range(4):
        for bi in range(2):
            row = 32 * rt + 16 * bi + r16  # per lane
            for pc in range(2):
                for c in range(ks // 2):
                    got = afrag[2 * c + (g >> 1), rt, pc, 16 * bi + r16 + 32 * (g & 1), :]  # [64, 16]
                    k = 64 * c + 16 * g[:, None] + j16[None, :]
                    assert np.array_equal(got, q[pc][row[:, None], k]), (d, rt, bi, pc, c)
                    np.add.at(seen[pc], (np.broadcast_to(row[:, None], k.shape), k), 1)
                if ks & 1:
                    frag = afrag[ks - 1, rt, pc, 16 * bi + r16 + 32 * (g >> 1), :]  # [64, 16]
                    got = np.where((g & 1)[:, None] == 0, frag[:, :8], frag[:, 8:])
                    k = 32 * (ks - 1) + 8 * g[:, None] + j8[None, :]
                    assert np.array_equal(got, q[pc][row[:, None], k]), (d, rt, bi, pc, "odd last step")
                    np.add.at(seen[pc], (np.broadcast_to(row[:, None], k.shape), k), 1)
    assert np.all(seen == 1), "every tap byte of every row reaches exactly one instruction"


def test_plane_pitch_is_conflict_free_for_the_operand_reads():
    """ds_read_b128 serves a wave in four groups of 16 lanes; the 16 lanes of a group must touch 16 different 16-byte bank
    quads of the 256-byte LDS row.  Lane l reads unit 4 c + (l >> 4) of row l & 15 at a pitch of 2 KS (odd KS) or 2 KS + 2
    (even KS) units; the pitch of the other byte-plane kernels (2 KS + 1) would be a 2-way conflict for this pattern."""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[l + 32 for l in grp] for grp in groups]

    def worst(pitch_units, c):
        w = 0
        for grp in groups:
            quads = [((l & 15) * pitch_units + 4 * c + (l >> 4)) % 16 for l in grp]
            w = max(w, max(quads.count(x) for x in quads))
        return w

    for ks in range(1, 9):
        pitch = 2 * ks if ks & 1 else 2 * ks + 2
        assert 16 * pitch >= 32 * ks  # a row's values fit
        for c in range(ks // 2):
            assert worst(pitch, c) == 1, (ks, c)
    assert worst(15, 0) == 2
