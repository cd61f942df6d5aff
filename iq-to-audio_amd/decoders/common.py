"""What the decoders share: the DC blocker of the AM and SSB decoders, and everything a side decoder (``side.py``) is written
against rather than copied from its neighbour.

Of a side decoder's core: ``BlockStore`` (named per-block device planes, joined once), ``StreamCore`` (plan, position, carried
history and the store: ``process`` and ``reset``; the subclass writes ``_block``), ``kept_records`` (one search whose list
may be too short, read back and sorted) and ``FrameCore`` (the tail of the decoders that read frames at several sampling
phases: count table, bits or symbols launch, frames launch, the ``finish`` dict).  Of its host side: ``parse_head`` (the
records of a parser as arrays), ``group_records`` (one frame seen several times), ``stage_records`` and ``phase_planes``
(what ``stages()`` shows of a ``FrameCore``).  ``search_with_room`` serves the decoders with several searches and the
finder; ``SideStage`` is the stage API."""
from __future__ import annotations

from ctypes import c_double, c_int32, c_int64

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


class BlockStore:
    """Named per-block device planes of one stream: ``append`` one tensor per name and block, ``joined(name)`` concatenates at
    most once and keeps the joined tensor.  ``dtypes``: name -> the dtype of the empty tensor that a stream which has seen
    nothing gives, or ``None`` for a plane that is then ``None`` (one stored only for the tests)."""

    def __init__(self, dtypes: dict):
        self.dtypes = dict(dtypes)
        self.reset()

    def reset(self) -> None:
        self._blocks = {name: [] for name in self.dtypes}

    def append(self, name, plane) -> None:
        self._blocks[name].append(plane)

    def joined(self, name):
        blocks = self._blocks[name]
        if len(blocks) > 1:
            blocks[:] = [D.torch_mod().cat(blocks)]
        if blocks:
            return blocks[0]
        return None if self.dtypes[name] is None else D.empty(0, self.dtypes[name])


class StreamCore:
    """Per-stream device state of a side decoder's core: the plan, the absolute position ``pos`` of the next block's first
    sample, the carried history (``_hist``: device ``hist_dtype[hist_len]``, ``None`` = zeros) and the ``store`` of its planes
    (``BlockStore``).  The subclass writes ``_block(x, n)``: the launches of one block of n > 0 samples, which appends to the
    store and returns the tensor whose last ``hist_len`` values the next block reads (``None`` where hist_len = 0)."""

    hist_dtype = "int32"

    def __init__(self, plan, hist_len: int = 0, planes: dict | None = None):
        self.plan, self.hist_len, self.store = plan, hist_len, BlockStore(planes or {})
        self._hist, self.pos = None, 0

    def process(self, x) -> None:
        """One block of the core's input (device float32[n]); an empty block changes nothing."""
        n = int(x.numel())
        if n:
            self._hist = carried_history(self._hist, self._block(x, n), self.hist_len, self.hist_dtype)
            self.pos += n

    def reset(self) -> None:
        """Back to a stream that has seen nothing: no history, position 0, no stored planes."""
        self._hist, self.pos = None, 0
        self.store.reset()


def kept_records(search, capacity: int, width: int, slot_bytes: int, sort_by) -> tuple:
    """The kept list of one ``search(room, counts)`` (it queues one launch that keeps up to ``room`` entries of ``width`` int64
    values and ``slot_bytes`` bytes each, counts what it wanted to keep in ``counts[0]`` and what it looked at in ``counts[1]``,
    and returns (list, slots)): (entries int64[kept, width], data uint8[kept, slot_bytes], kept, looked at) on the host, the
    rows sorted by the columns ``sort_by`` (the first the major one).  A list too short is never used (``search_with_room``)."""
    counts = D.zeros(2, "int64")
    ((lst, slots),), (kept, seen) = search_with_room([lambda room: search(room, counts)], counts, capacity)
    entries = lst[: width * kept].cpu().numpy().reshape(-1, width)
    data = slots[: slot_bytes * kept].cpu().numpy().reshape(-1, slot_bytes)
    order = np.lexsort([entries[:, c] for c in reversed(sort_by)])
    return entries[order], data[order], kept, seen


class FrameCore(StreamCore):
    """The cores that read one stored plane at several sampling phases and keep the frames whose check holds (AX.25, ACARS,
    AIS).  The subclass names the two entries, the slot width, the phases and the streams read (phases x gains), the record
    key (``key``), the keys of the plane and its length in ``finish()`` (``plane_keys``) and the plane's dtype, and hands
    ``__init__`` the window the kernels take (``reach``: the plan's L or W) and the plan's count of a phase's bits."""

    bits_entry = frames_entry = key = plane_dtype = None
    SLOT_BYTES = PHASES = STREAMS = 0
    plane_keys = ("bits", "nbits")

    def __init__(self, plan, reach: int, count, hist_len: int = 0, planes: dict | None = None):
        super().__init__(plan, hist_len, planes)
        self.reach, self._count = reach, count

    def counts_of(self, n: int) -> list:
        """What every phase reads of a stored plane of n samples."""
        return [self._count(p, n) for p in range(self.PHASES)]

    def frames_of(self, src, capacity: int) -> dict:
        """The tail of ``finish``: the stored plane ``src`` read at every phase and the kept frames of all of them, as
        dict(<key>, s, start, nbytes, data, candidates, <plane>, <its length>, count_of), the records as numpy arrays sorted
        by (<key>, s).  A list too short for the kept frames is never used: the search is repeated with room for all."""
        n, step, reach = int(src.numel()), c_double(self.plan.step), c_int32(self.reach)
        counts_of = self.counts_of(n)
        longest = max(counts_of)
        count_of = (c_int64 * self.PHASES)(*counts_of)
        plane = D.empty(self.STREAMS * longest, self.plane_dtype)
        N.call(self.bits_entry, N.ptr(src), c_int64(n), reach, step, c_int64(longest), N.ptr(plane), N.stream_ptr())

        def search(room: int, counts):
            lst, slots = D.empty(4 * room, "int64"), D.empty(self.SLOT_BYTES * room, "uint8")
            N.call(self.frames_entry, N.ptr(plane), c_int64(longest), count_of, reach, step, N.ptr(lst), N.ptr(slots), c_int64(room),
                   N.ptr(counts), N.stream_ptr())
            return lst, slots

        entries, data, _, closed = kept_records(search, capacity, 4, self.SLOT_BYTES, (0, 1))
        cols = {name: entries[:, c].copy() for c, name in enumerate((self.key, "s", "start", "nbytes"))}
        return dict(cols, data=data, candidates=closed, **{self.plane_keys[0]: plane, self.plane_keys[1]: longest}, count_of=counts_of)


def parse_head(result, records: dict, candidates: int, *names) -> tuple:
    """The head of a parser of kept records: (``result(candidates=, crc_ok=<the records>)``, then ``records[name]`` as int64[k]
    for every name, then ``records["data"]`` as uint8[k, slot width]; uint8[0, 0] without a record)."""
    cols = [np.asarray(records[name], dtype=np.int64).reshape(-1) for name in names]
    k = cols[0].size
    data = np.asarray(records["data"], dtype=np.uint8).reshape(k, -1) if k else np.zeros((0, 0), dtype=np.uint8)
    return (result(candidates=int(candidates), crc_ok=k), *cols, data)


def stage_records(fin: dict, key: str) -> list:
    """``records`` of ``stages()``: [(<key>, s, start instant, bytes)] of a ``FrameCore.finish()``, in its order."""
    return [(int(p), int(s), int(at), fin["data"][k, : int(nb)].tobytes())
            for k, (p, s, at, nb) in enumerate(zip(fin[key], fin["s"], fin["start"], fin["nbytes"]))]


def phase_planes(core: FrameCore, fin: dict) -> list:
    """The plane of ``core.finish()`` on the host, one array per stream read, each as long as its phase has bits or symbols."""
    plane, longest = (fin[k] for k in core.plane_keys)
    dtype = {"uint8": np.uint8, "int32": np.int32}[core.plane_dtype]
    plane = plane.cpu().numpy().reshape(core.STREAMS, -1) if longest else np.zeros((core.STREAMS, 0), dtype=dtype)
    return [plane[v, : fin["count_of"][v % core.PHASES]] for v in range(core.STREAMS)]


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
