"""What the decoders share: the DC blocker of the AM and SSB decoders, and the pieces every side decoder (``side.py``) repeats
-- merging the records of one frame, a search whose list may turn out too short, the carried history, the stage API."""
from __future__ import annotations

from ctypes import c_double, c_int64

import numpy as np

from .. import _dev as D
from .. import _native as N
from .base import n_elements, scan_workspace


class DCBlocker:
    """y[n] = x[n] - x[n-1] + r y[n-1] across calls (reference decoders/common.py:6-30), as a parallel affine scan in
    float64; the pair (x[last], y[last]) lives in a device double[2]."""

    def __init__(self, radius: float = 0.995):
        if not 0.0 < radius < 1.0:
            raise ValueError("radius must be between 0 and 1")
        self.radius = radius
        self._pair = None

    def carried(self) -> tuple[float, float]:
        """(x_prev, y_prev) as the next call will see them."""
        if self._pair is None:
            return 0.0, 0.0
        x_prev, y_prev = self._pair.cpu().numpy()
        return float(x_prev), float(y_prev)

    def process(self, samples):
        if n_elements(samples) == 0:
            return samples
        if self._pair is None:
            self._pair = D.zeros(2, "float64")
        x = D.to_device(samples, "float32")
        y = D.empty(x.numel(), "float32")
        N.call("iqa_dc_block", N.ptr(x), c_int64(x.numel()), c_double(self.radius), N.ptr(self._pair), N.ptr(y),
               N.ptr(scan_workspace(x.numel())), N.stream_ptr())
        return D.like_input(y, samples)


def group_records(start, lengths, data, reach: int, tie=None) -> list:
    """Merge the kept records that are one frame seen several times (at several sampling phases, gains or positions): walked
    in ascending ``start`` (ties by ``tie``, else in the order given), a record joins the latest group with the same bytes
    ``data[k, : lengths[k]]`` whose first start lies within ``reach`` of its own, and opens a group otherwise.  Returns
    ``[first start, bytes, hits, index of the first record]`` per group, ascending in the first start."""
    order = np.argsort(start, kind="stable") if tie is None else np.lexsort((tie, start))
    groups: list = []
    for k in order.tolist():
        raw, at = data[k, : int(lengths[k])].tobytes(), int(start[k])
        for grp in reversed(groups):
            if at - grp[0] > reach:  # (ascending starts: every earlier group is further back still)
                groups.append([at, raw, 1, k])
                break
            if grp[1] == raw:
                grp[2] += 1
                break
        else:
            groups.append([at, raw, 1, k])
    return groups


def search_with_room(searches, counts, capacity: int):
    """Run every ``search(capacity)`` (each queues one search launch whose list holds ``capacity`` entries and which counts
    what it wanted to keep in ``counts[i]``, device int64), read ``counts`` back ONCE behind all of them, and repeat each
    search whose list was too short with room for all it keeps: a truncated list is never used.  Returns (what the searches
    returned, ``counts`` on the host as ints)."""
    found = [search(capacity) for search in searches]
    host = [int(v) for v in counts.cpu().numpy()]
    for i, search in enumerate(searches):
        if host[i] > capacity:
            found[i] = search(host[i])
            assert int(counts[i].item()) == host[i]
    return found, host


def carried_history(hist, t, h: int, dtype: str = "int32"):
    """The last ``h`` values of the stream that ends with block ``t`` (``hist``: those before it, ``None`` = zeros): what the
    next block's kernel reads in front of its own samples.  ``None`` for a kernel without history (h = 0)."""
    if not h:
        return None
    n = int(t.numel())
    if n >= h:
        return t[n - h :].clone()
    prev = hist if hist is not None else D.zeros(h, dtype)
    return D.torch_mod().cat([prev[n:], t])


def unit_prev():
    """The discriminator state of a stream that has seen nothing: device complex64[1] = 1 + 0j."""
    return D.from_numpy(np.array([1 + 0j], dtype=np.complex64))


class SideStage:
    """The stage API of a side decoder: ``process(block)`` per block of the channel -- complex (the channelizer's output, run
    through ``iqa_quadrature`` with this decoder's own ``prev``, or through ``iqa_envelope``, as ``source`` says) or float32
    (that kernel's output, made elsewhere) -- and ``finish()`` once: the core's ``result`` over its cached ``finish()``.  The
    subclass names the plan, the core and ``stages()`` for the tests."""

    source = "theta"  # or "envelope"
    finish_args: dict = {}  # what ``_finished`` passes to the core's ``finish``

    def __init__(self, core, *, keep: bool, **context):
        self.plan, self.core, self.context = core.plan, core, context
        self._prev = unit_prev() if self.source == "theta" else None
        self._keep = keep
        self.inputs: list = []  # with keep: the kernel input of every block (device float32)
        self._fin = None

    def process(self, block) -> None:
        torch = D.torch_mod()
        if torch.is_complex(block) if D.is_tensor(block) else np.iscomplexobj(block):
            z = D.to_device(block, "complex64")
            n = int(z.numel())
            x = D.empty(n, "float32")
            if n and self.source == "theta":
                N.call("iqa_quadrature", N.ptr(z), c_int64(n), N.ptr(self._prev), N.ptr(x), N.stream_ptr())
            elif n:
                N.call("iqa_envelope", N.ptr(z), c_int64(n), N.ptr(x), N.stream_ptr())
        else:
            x = D.to_device(block, "float32")
            if self.source == "envelope":
                x = x.clone()  # (the core keeps the tensor: the caller's may change)
        if self._keep:
            self.inputs.append(x)
        self.core.process(x)
        self._fin = None

    def _finished(self) -> dict:
        if self._fin is None:
            self._fin = self.core.finish(**self.finish_args)
        return self._fin

    def _inputs_host(self):
        return D.torch_mod().cat(self.inputs).cpu().numpy() if self.inputs else None

    def finish(self):
        return self.core.result(self._finished(), **self.context)
