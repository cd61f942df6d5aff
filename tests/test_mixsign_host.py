"""``mixsign.probe_window``: the lengths of the mixer-sign probe, against the rule of the oracle's ``choose_mix_sign``
(``oracle/cpu_ref.py``; reference processing.py:636-656), worked out by hand at every shape where the rule branches:

    take    = min(n_in, max(int(0.05 fs), 4 L, 131072));  if take < L: take = min(n_in, 2 L)
    n_z     = ceil(take / max(D, 1))                      (``[::D]`` of ``take`` filtered samples)
    discard = min(L, n_z // 4);  if nothing were left: discard = 0
    keep    = n_z - discard

``n_in = 0`` is the callers' early return (``MixSignProbe``: sign +1 without a launch), not this function's.
"""
from __future__ import annotations

import pytest

from iq_to_audio_amd.mixsign import probe_window

# (n_in, L, fs, D) -> (snippet, n_z, discard, keep)
CASES = [
    # n_in < L: the whole warm-up (the second rule's min(n_in, 2 L) is n_in again)
    ((100, 401, 2.5e6, 1), (100, 100, 25, 75)),
    ((100, 401, 2.5e6, 208), (100, 1, 0, 1)),  # n_z = 1: n_z // 4 = 0
    # L <= n_in < 2 L
    ((600, 401, 2.5e6, 1), (600, 600, 150, 450)),
    ((600, 401, 2.5e6, 208), (600, 3, 0, 3)),  # n_z = 3: n_z // 4 = 0
    ((700, 401, 2.5e6, 208), (700, 4, 1, 3)),  # n_z = 4: n_z // 4 = 1
    ((600, 401, 2.5e6, 0), (600, 600, 150, 450)),  # a decimation below 1 is 1
    # n_in exactly 4 L
    ((1604, 401, 2.5e6, 26), (1604, 62, 15, 47)),
    # 4 L < n_in < 131072: still the whole warm-up
    ((100_000, 6401, 2.5e6, 26), (100_000, 3847, 961, 2886)),
    # n_in > 131072, 0.05 fs = 125 000 below it (2.5 MS/s): 131072 frames
    ((1_000_000, 6401, 2.5e6, 26), (131_072, 5042, 1260, 3782)),
    ((1_000_000, 401, 2.5e6, 1), (131_072, 131_072, 401, 130_671)),  # discard held by L, not by n_z // 4
    ((1_000_000, 40_000, 2.5e6, 26), (160_000, 6154, 1538, 4616)),  # 4 L above both
    # n_in > 131072, 0.05 fs = 1 000 000 above it (20 MS/s)
    ((2_400_000, 28_571, 20e6, 208), (1_000_000, 4808, 1202, 3606)),
    ((500_000, 28_571, 20e6, 208), (500_000, 2404, 601, 1803)),  # ... and a warm-up shorter than that
]


@pytest.mark.parametrize("args, want", CASES)
def test_probe_window_is_the_oracles_rule(args, want):
    got = probe_window(*args)
    assert got == want
    assert all(isinstance(v, int) for v in got)


def test_a_probe_is_never_emptied():
    """discard <= n_z // 4 < n_z for every n_z >= 1, so ``keep`` >= 1 whenever there is a warm-up (the rule for a probe
    that ``discard`` would empty never fires there).  That a channelizer turns ``snippet`` frames into exactly ``n_z``
    outputs is checked on the GPU (``test_gpu_mixsign.py``)."""
    for n_in in (1, 2, 3, 4, 5, 63, 64, 65, 207, 208, 209, 1000, 131_071, 131_072, 131_073, 300_001):
        for ntaps in (1, 2, 31, 401, 6401):
            for d in (1, 2, 26, 208):
                snippet, n_z, discard, keep = probe_window(n_in, ntaps, 2.5e6, d)
                assert 1 <= snippet <= n_in and n_z == -(-snippet // d) >= 1 and 0 <= discard < n_z and keep == n_z - discard >= 1
