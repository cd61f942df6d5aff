"""Capture blocks from the memory-mapped file to the device (``_BlockStager``)."""
from __future__ import annotations

import threading

import numpy as np

from . import _dev as D


class _BlockStager:
    """Capture blocks: memory-mapped file -> one of two pinned host buffers (filled by a helper thread,
    overlapping the previous block's GPU work) -> device tensor by asynchronous H2D copy.
    Replaces the reference's ffmpeg decode pipe + ``IQReader.read_block`` (processing.py:238-266): the
    capture's own sample format goes to the GPU untouched."""

    #: pinned staging buffers that finished runs gave back, by (dtype, elements): pinning 50 MB costs ~15 ms and a run
    #: on a small capture (the reference's --benchmark: 50 MB) spent a third of its wall time on it
    _POOL: dict = {}
    _POOL_MAX_BYTES = 2 << 30
    _POOL_LOCK = threading.Lock()

    def __init__(self, frames: np.ndarray, dtype: str, max_frames: int):
        torch = D.torch_mod()
        self.frames = frames
        self.dtype = getattr(torch, dtype)
        self.numel = 2 * max_frames
        self.bufs = [None, None]  # pinned lazily: a capture of one block needs one
        self.events = [None, None]
        self.pending = None  # (thread, slot, lo, hi)
        self.slot = 0

    def _buf(self, slot: int):
        if self.bufs[slot] is None:
            torch = D.torch_mod()
            key = (str(self.dtype), self.numel)
            with self._POOL_LOCK:
                stack = self._POOL.get(key)
                self.bufs[slot] = stack.pop() if stack else None
            if self.bufs[slot] is None:
                self.bufs[slot] = torch.empty(self.numel, dtype=self.dtype, pin_memory=True)
        return self.bufs[slot]

    def close(self) -> None:
        """Give the pinned buffers back (every H2D copy out of them has completed)."""
        if self.pending is not None:
            self.pending[0].join()
            self.pending = None
        for ev in self.events:
            if ev is not None:
                ev.synchronize()
        key = (str(self.dtype), self.numel)
        with self._POOL_LOCK:
            held = sum(t.numel() * t.element_size() for st in self._POOL.values() for t in st)
            for i, b in enumerate(self.bufs):
                if b is not None and held + b.numel() * b.element_size() <= self._POOL_MAX_BYTES:
                    self._POOL.setdefault(key, []).append(b)
                    held += b.numel() * b.element_size()
                self.bufs[i] = None

    #: helper threads of one block copy (file mapping -> pinned buffer): a single memcpy moves ~2.7 GB/s on the GPU boxes'
    #: hosts, which made the FILE the bottleneck of a file -> WAV run (10 s @ 10 MS/s: 0.148 s, of which ~0.1 s this copy)
    copy_threads = 8

    def _fill(self, slot: int, lo: int, hi: int) -> None:
        dst = self._buf(slot).numpy()[: 2 * (hi - lo)]
        src = self.frames[2 * lo : 2 * hi]
        parts = min(int(self.copy_threads), max(1, dst.size // (1 << 22)))  # (NumPy copies release the GIL)
        if parts <= 1:
            np.copyto(dst, src)
            return
        cuts = [dst.size * i // parts for i in range(parts + 1)]
        workers = [threading.Thread(target=np.copyto, args=(dst[a:b], src[a:b]), name="iq-stager-copy", daemon=True)
                   for a, b in zip(cuts[1:-1], cuts[2:])]
        for w in workers:
            w.start()
        np.copyto(dst[: cuts[1]], src[: cuts[1]])
        for w in workers:
            w.join()

    def prefetch(self, lo: int, hi: int) -> None:
        slot = self.slot ^ 1
        if self.events[slot] is not None:
            self.events[slot].synchronize()  # the previous H2D out of this buffer must be done
        th = threading.Thread(target=self._fill, args=(slot, lo, hi), name="iq-stager", daemon=True)
        th.start()
        self.pending = (th, slot, lo, hi)

    def fetch(self, lo: int, hi: int):
        torch = D.torch_mod()
        if self.pending is not None and self.pending[2:] == (lo, hi):
            th, slot = self.pending[0], self.pending[1]
            th.join()
        else:
            if self.pending is not None:
                # a prefetch for other bounds is filling the very buffer this fetch is about to fill (both take slot ^ 1):
                # let the helper finish first.  (The pipeline's block loop always fetches what it prefetched; this is
                # for other callers of the class.)
                self.pending[0].join()
            slot = self.slot ^ 1
            if self.events[slot] is not None:
                self.events[slot].synchronize()
            self._fill(slot, lo, hi)
        self.pending = None
        self.slot = slot
        dev = torch.empty(2 * (hi - lo), dtype=self.dtype, device=D.device())
        dev.copy_(self._buf(slot)[: 2 * (hi - lo)], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[slot] = ev
        return dev
