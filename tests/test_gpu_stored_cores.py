"""The shared host cores on the MI355X: the per-block store of the side decoders (``decoders/common.py``: ``BlockStore``), the
carried history of their stream core (``StreamCore``) at block lengths around the history's, and the stored discriminator
stream of the protocol decoders (``protocol_layer.StoredTheta`` under ``FlexDecoder`` and ``DmrDecoder``), whose output does
not depend on how the stream was cut.  The decoders themselves are tested in their own files; every comparison is exact."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HIST = 8


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


def test_block_store_joins_once(A):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.decoders.common import BlockStore

    rng = np.random.default_rng(1)
    blocks = [rng.standard_normal(n).astype(np.float32) for n in (1, 0, 7, 0, 2048)]
    store = BlockStore(dict(x="float32", kept=None))
    empty = store.joined("x")
    assert empty.is_cuda and tuple(empty.shape) == (0,) and str(empty.dtype) == "torch.float32" and store.joined("kept") is None
    store.append("x", D.from_numpy(blocks[0]))
    assert store.joined("x").cpu().numpy().tobytes() == blocks[0].tobytes()  # (a single block is handed on as it is)
    for block in blocks[1:]:
        store.append("x", D.from_numpy(block))
    joined = store.joined("x")
    assert joined.cpu().numpy().tobytes() == np.concatenate(blocks).tobytes()
    assert store.joined("x") is joined and store.joined("kept") is None
    store.reset()
    again = store.joined("x")
    assert tuple(again.shape) == (0,) and str(again.dtype) == "torch.float32" and store.joined("kept") is None


def test_stream_core_carries_the_history(A):
    from iq_to_audio_amd import _dev as D
    from iq_to_audio_amd.decoders.common import StreamCore

    class Quantised(StreamCore):
        """Its history is carried over the block's quantised values; they are stored as well."""

        def _block(self, x, n):
            t = x.round().int()
            self.store.append("t", t)
            return t

    core = Quantised(None, HIST, dict(t="int32"))
    rng = np.random.default_rng(2)
    stream = np.zeros(0, dtype=np.int32)
    for n in (1, 0, HIST - 1, HIST, HIST + 1, 1):  # shorter than, as long as and longer than the history; a short one behind a long one
        block = rng.integers(-2000, 2000, n).astype(np.float32)
        core.process(D.from_numpy(block))
        stream = np.concatenate([stream, block.astype(np.int32)])
        want = np.concatenate([np.zeros(HIST, dtype=np.int32), stream])[-HIST:]
        if stream.size:
            assert core._hist.cpu().numpy().tolist() == want.tolist() and str(core._hist.dtype) == "torch.int32"
        else:
            assert core._hist is None
        assert core.pos == stream.size
    assert core.store.joined("t").cpu().numpy().tolist() == stream.tolist()
    core.reset()
    assert core._hist is None and core.pos == 0 and tuple(core.store.joined("t").shape) == (0,)
    plain = Quantised(None, 0, dict(t="int32"))  # no history: nothing is carried
    plain.process(D.from_numpy(np.ones(3, dtype=np.float32)))
    assert plain._hist is None and plain.pos == 3


def _same(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name,fs", [("FlexDecoder", 8 * 1600.0), ("DmrDecoder", 4 * 4800.0)])  # the lowest rates their plans accept
def test_stored_theta_does_not_depend_on_the_cut(A, name, fs):
    theta = np.zeros(4096, dtype=np.float32)
    whole = getattr(A, name)(fs)
    whole.process(theta)
    want = whole.stages()
    assert want and all(_same(want[key], again) for key, again in whole.stages().items())
    cut = getattr(A, name)(fs)
    for _ in range(2):  # and once more behind reset()
        for part in (theta[:1], theta[:0], theta[1:4095], theta[4095:]):
            cut.process(part)
        got = cut.stages()
        assert list(got) == list(want)
        for key in want:
            assert _same(got[key], want[key]), key
        assert cut.finish() == whole.finish() and cut.finish() is cut.finish()
        cut.reset()
        assert cut._stored == [] and cut._st is None and cut._result is None
