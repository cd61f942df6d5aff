"""The capture stream of the byte-plane ring kernels at every phase against a 16-byte boundary.

The loader waves of the contiguous-slot int16 kernels (``ring_loader_split``) fetch the capture as it lies in memory, 16
bytes per lane from a stream that starts (pointer / 4 + 1 - consumed) mod 4 frames behind a 16-byte boundary -- a phase that
is uniform per launch and that real use meets at all four values.  These loads are the contiguous kernels' own (non-temporal
since round 7 in launches of a single lane; an aligned-unit form with the shift done in registers
was measured beside them and dropped), so every phase is pinned here in either kind of launch: one launch per case, compared with the exact integer model (``torch.equal``; the rotated
lane within the rotation's own bar, as everywhere).  The capture holds exactly what the launch may read.

Shapes: D = 8 (a tile is one 1 KiB piece, the second loader of a parity fetches nothing it writes), D = 104 (13 pieces,
the two loaders of a parity take 7 and 6), D = 100 (an even row pitch, padded in LDS), D = 208 (13 k steps: the uneven
split and the packed (row, unit) path) and D = 208 as a lane pair (four loaders on one tile, three rounds in flight).
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import mfma_dispatch as X
from test_gpu_mfma_exact import Lane, _check_abi_selects, _rot, check_lane, launch, make_plan, setup_capture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


FMT, OPB, N_OUT, M_FIRST = "s16", 256, 2 * 256 + 37, 64 + 1000

SHAPES = {  # name -> (entry, D)
    "d8-half1": ("multi", 8),
    "d104-half7": ("multi", 104),
    "d100-half7": ("multi", 100),
    "d208-multi13": ("multi", 208),
    "d208-pairs13": ("pairs", 208),
}


def _ks(d):
    return -(-2 * d // 32)


def _first_row_frame(d):
    return (M_FIRST - 64) * d + 1  # global frame of the first byte the launch needs (tap-row group 0)


def _lanes(d):
    """One plain lane; one rotated, conjugated and scaled by j."""
    rng = np.random.default_rng(7000 + d)
    step, base = _rot(rng)
    mp_a = make_plan(64 * d - d // 3 - 1, d, FMT, True, seed=d)
    mp_b = make_plan(64 * d - d // 3 - 6, d, FMT, True, seed=d + 100)
    return [Lane(mp_a, 0), Lane(mp_b, 0, rotate=1, conj=1, scale=1j, rot_step=step, rot_base=base)]


def _select(A, shape):
    entry, d = SHAPES[shape]
    name = X.expected_kernel(entry, FMT, d, 0, _ks(d), False, False)
    want = {"d8-half1": "k_channelize_mfma_s16_ring_multi_half<1>", "d104-half7": "k_channelize_mfma_s16_ring_multi_half<7>",
            "d100-half7": "k_channelize_mfma_s16_ring_multi_half<7>", "d208-multi13": "k_channelize_mfma_s16_ring_multi<13>",
            "d208-pairs13": "k_channelize_mfma_s16_ring_pairs<13>"}[shape]
    assert name == want
    _check_abi_selects(A, entry, FMT, d, 0, _ks(d), False, name)
    return entry, d


def _run(A, shape, consumed, x_of, what, one_lane=False):
    """One launch at ``consumed``; ``x_of(raw_full, n_frames)`` builds the device tensor handed over and returns it with
    the dwords its first frame lies behind a 16-byte boundary.  ``one_lane``: the rotated lane alone."""
    entry, d = _select(A, shape)
    raw, x_full, n_frames, consumed = setup_capture(FMT, d, 1, 0, _ks(d), 0, 0, M_FIRST, N_OUT, OPB, seed=d + consumed % 4, consumed=consumed)
    x, ptr_dwords = x_of(x_full, n_frames)
    lanes = _lanes(d)[1:] if one_lane else _lanes(d)
    launch(entry, FMT, d, 0, _ks(d), OPB, lanes, x, n_frames, consumed, M_FIRST, N_OUT)
    for i, ln in enumerate(lanes):
        check_lane(ln, 0, raw, d, consumed, M_FIRST, N_OUT, f"{shape} {what} lane {i}")
    return (ptr_dwords + 1 - consumed) % 4


def _whole(x_full, n_frames):
    assert x_full.data_ptr() % 16 == 0
    return x_full, 0


@pytest.mark.parametrize("phase", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_stream_phase_through_consumed(A, shape, phase):
    """consumed = 0, 1, 2, 3 (mod 4) with the capture at the start of its tensor: the stream at every phase."""
    d = SHAPES[shape][1]
    consumed = _first_row_frame(d) - 4 - phase  # 4..7 frames in front of the first row
    assert _run(A, shape, consumed, _whole, f"phase {phase}") == phase


@pytest.mark.parametrize("phase", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [s for s in SHAPES if SHAPES[s][0] == "multi"])
def test_stream_phase_of_a_single_lane(A, shape, phase):
    """One lane per launch: one workgroup streams each range, the launches whose loaders fetch with non-temporal loads."""
    d = SHAPES[shape][1]
    assert _run(A, shape, _first_row_frame(d) - 4 - phase, _whole, f"one lane, phase {phase}", one_lane=True) == phase


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("shape", ["d8-half1", "d104-half7"])
def test_stream_phase_through_the_pointer(A, shape, shift):
    """The capture handed over as a view that starts 1, 2 and 3 frames into its tensor."""
    import torch

    d = SHAPES[shape][1]
    consumed = _first_row_frame(d) - 4  # phase 0 at an aligned pointer

    def view(x_full, n_frames):
        junk = torch.randint(-32768, 32767, (2 * shift,), dtype=torch.int16, device=x_full.device)
        big = torch.cat([junk, x_full])
        assert big.data_ptr() % 16 == 0
        v = big[2 * shift:]
        assert v.data_ptr() == big.data_ptr() + 4 * shift
        return v, shift

    assert _run(A, shape, consumed, view, f"pointer + {shift} frames") == shift


@pytest.mark.parametrize("shape", list(SHAPES))
def test_first_byte_inside_the_first_unit_of_the_allocation(A, shape):
    """The tensor begins at the first byte of its allocation and the stream's first byte is its frame 1, inside the
    allocation's first 16 bytes."""
    d = SHAPES[shape][1]
    assert _run(A, shape, _first_row_frame(d) - 1, _whole, "first unit") == 1


@pytest.mark.parametrize("shape", list(SHAPES))
def test_readable_bound_ends_in_the_last_unit_of_the_tensor(A, shape):
    """The tensor ends with the last frame the launch may read, 8 bytes into a 16-byte unit."""
    d = SHAPES[shape][1]
    consumed = _first_row_frame(d) - 4 - 2  # phase 2

    def exact(x_full, n_frames):
        x = x_full[: 2 * n_frames].clone()
        assert x.data_ptr() % 16 == 0 and x.numel() == 2 * n_frames and (4 * n_frames) % 16 == 8
        return x, 0

    assert _run(A, shape, consumed, exact, "last unit") == 2
