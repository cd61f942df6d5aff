"""What ``MixSignProbe._probe_one``'s whole-snippet path relies on: a channelizer at the start of a capture turns the
``snippet`` frames of ``mixsign.probe_window`` into exactly ``n_z`` outputs (``process(..., last_block=True)``), so the
lengths need not be derived again from what comes back."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fs, d, fmt, n_in", [
    (2.5e6, 26, "s16", 100),        # shorter than the filter
    (2.5e6, 26, "s16", 5_000),      # the whole warm-up, float32 edge kernel only
    (2.5e6, 26, "u8", 131_073),     # 131072 frames: n_z = 5042
    (2.5e6, 26, "f32", 131_073),
    (20e6, 208, "s16", 700),        # n_z = 4
    (20e6, 208, "f32", 1_000_001),  # 0.05 fs frames: n_z = 4808
    (250e3, 1, "f32", 3_000),       # no decimation
])
def test_a_snippet_gives_n_z_outputs(fs, d, fmt, n_in):
    import iq_to_audio_amd as A
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.mixsign import probe_window

    A.native.lib()
    A.native.require_gpu()
    taps = A.design_channel_filter(fs, 12_500.0, d)
    snippet, n_z, _, _ = probe_window(n_in, len(taps), fs, d)
    rng = np.random.default_rng(3)
    if fmt == "f32":
        x = D.to_device((rng.normal(size=snippet) + 1j * rng.normal(size=snippet)).astype(np.complex64) * 0.1, "complex64")
    else:
        dt = {"s16": "int16", "u8": "uint8"}[fmt]
        x = D.to_device(rng.integers(0, 200, size=2 * snippet).astype(dt), dt)
    for sign in (1, -1):
        ch = A.Channelizer(taps, sample_rate=fs, freq_offset=25e3, mix_sign=sign, decimation=d, fmt=fmt)
        z = ch.process(x, last_block=True)
        assert int(z.numel()) == n_z
