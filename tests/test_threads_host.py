"""The package's process-wide state under several host threads, without a GPU.

INTEGRATION.md ("Threading contract") promises N pipelines from N host threads.  What the threads share is host-side
bookkeeping: the pinned upload pool and the side-stream table of ``_dev``, the probe read-back buffers of ``mixsign``, the
staging-buffer pool of ``_BlockStager``, the kernel and table caches, the library handle of ``_native`` and the library's
thread-local error string.  Each is driven here from real threads against a stand-in for ``torch`` (``FakeTorch``) whose
"device" is host memory and whose copies are ASYNCHRONOUS: a queued copy reads its pinned source when the test completes
the stream, not when it is queued, as a DMA engine does.  The interleavings are forced, not hoped for: the stand-in holds
threads at a barrier inside ``empty`` / ``Stream`` / ``CDLL``, so every run takes the same path.

The last two tests use the real library: it loads, and rejects bad arguments, without a GPU.
"""
from __future__ import annotations

import ctypes
import threading
from collections import OrderedDict
from ctypes import c_int32, c_int64, c_void_p

import numpy as np
import pytest

from iq_to_audio_amd import _dev as D
from iq_to_audio_amd import _native as N

WAIT = 30.0  # seconds a stuck thread is given before the test fails (never reached by a passing run)


# ---- a stand-in for torch ------------------------------------------------------------------------------------------------


class FakeTensor:
    def __init__(self, torch, arr, *, pinned=False, device=None, root=None):
        self.torch, self.arr, self.pinned, self.device = torch, arr, pinned, device
        self.root = self if root is None else root  # the allocation a view belongs to

    def _like(self, arr):
        return FakeTensor(self.torch, arr, pinned=self.pinned, device=self.device, root=self.root)

    is_cuda = property(lambda self: self.device is not None)
    dtype = property(lambda self: self.arr.dtype)
    shape = property(lambda self: self.arr.shape)

    def pin_memory(self):
        self.torch.hook("pin_memory")
        return FakeTensor(self.torch, self.arr.copy(), pinned=True)

    def __getitem__(self, key):
        return self._like(self.arr[key])

    def numpy(self):
        assert self.device is None, "numpy() of a device tensor"
        return self.arr

    def numel(self):
        return int(self.arr.size)

    def element_size(self):
        return int(self.arr.itemsize)

    def view(self, dtype):
        return self._like(self.arr.view(dtype))

    def reshape(self, *shape):
        return self._like(self.arr.reshape(*shape))

    def contiguous(self):
        return self

    def to(self, device):  # pageable memory -> device: the copy has been made when the call returns
        self.torch.note("copy_blocking")
        return FakeTensor(self.torch, self.arr.copy(), device=device)

    def copy_(self, src, non_blocking=False):
        self.torch.queue_copy(self, src)
        if not non_blocking:
            self.torch.cuda.current_stream().synchronize()
        return self

    def read(self):
        """What the device holds NOW (copies that have not completed have not arrived)."""
        return self.arr.copy()


class FakeTorch:
    """``torch`` as ``_dev``, ``staging``, ``mixsign`` and the caches use it.  One stream per host thread: a copy queued by
    a thread completes at that thread's ``synchronize`` (stream or event) or at the test's ``complete_all``."""

    def __init__(self):
        self.mu = threading.Lock()
        self.queues: dict = {}  # thread id -> copies queued and not complete: (dst, src)
        self.queued: dict = {}  # thread id -> copies ever queued
        self.done: dict = {}  # thread id -> copies complete
        self.log: list = []  # (what, thread name) in order
        self.hooks: dict = {}
        self.violations: list = []
        self.streams_made = 0
        for name in ("uint8", "int16", "int32", "int64", "float32", "float64", "complex64"):
            setattr(self, name, np.dtype(name))
        self.cuda = _FakeCuda(self)
        self._C = None

    def hook(self, name):
        fn = self.hooks.get(name)
        if fn is not None:
            fn()

    def note(self, what):
        with self.mu:
            self.log.append((what, threading.current_thread().name))

    def empty(self, n, dtype=None, device=None, pin_memory=False):
        if device is not None:
            self.hook("empty_device")
        return FakeTensor(self, np.zeros(int(n), dtype=dtype), pinned=bool(pin_memory), device=device)

    zeros = empty

    def from_numpy(self, arr):
        return FakeTensor(self, arr)

    def device(self, *a):
        return "dev0"

    # -- the asynchronous copy engine
    def queue_copy(self, dst, src):
        tid = threading.get_ident()
        with self.mu:
            for q in self.queues.values():
                for _, other in q:
                    if other.root is src.root:
                        self.violations.append("a pinned buffer is the source of two copies in flight")
            self.queues.setdefault(tid, []).append((dst, src))
            self.queued[tid] = self.queued.get(tid, 0) + 1
            self.log.append(("copy_queued", threading.current_thread().name))

    def _complete(self, tid, upto=None):
        q = self.queues.get(tid, [])
        while q and (upto is None or self.done.get(tid, 0) < upto):
            dst, src = q.pop(0)
            dst.arr[...] = src.arr  # the source is read NOW
            self.done[tid] = self.done.get(tid, 0) + 1

    def complete_all(self):
        with self.mu:
            for tid in list(self.queues):
                self._complete(tid)

    def in_flight(self, tensor) -> bool:
        """A queued copy INTO this tensor's allocation has not completed."""
        with self.mu:
            return any(dst.root is tensor.root for q in self.queues.values() for dst, _ in q)

    def sources_in_flight(self) -> list:
        with self.mu:
            return [src.root for q in self.queues.values() for _, src in q]


class _FakeCuda:
    def __init__(self, torch):
        outer = torch

        class Event:
            def __init__(self):
                self.tid, self.seq = None, 0

            def record(self):
                self.tid = threading.get_ident()
                with outer.mu:
                    self.seq = outer.queued.get(self.tid, 0)

            def query(self):
                outer.hook("query")
                with outer.mu:
                    return outer.done.get(self.tid, 0) >= self.seq

            def synchronize(self):
                with outer.mu:
                    outer._complete(self.tid, self.seq)
                    outer.log.append(("event_sync", threading.current_thread().name))

        class Stream:
            def __init__(self, device=None):
                with outer.mu:
                    outer.streams_made += 1
                outer.hook("Stream")
                self.device = device

            def synchronize(self):
                with outer.mu:
                    outer._complete(threading.get_ident())
                    outer.log.append(("stream_sync", threading.current_thread().name))

        self.Event, self.Stream = Event, Stream
        self._current = Stream.__new__(Stream)

    def current_device(self):
        return 0

    def current_stream(self):
        return self._current

    def is_current_stream_capturing(self):
        return False


@pytest.fixture
def fake(monkeypatch):
    torch = FakeTorch()
    monkeypatch.setattr(D, "torch_mod", lambda: torch)
    monkeypatch.setattr(D, "device", lambda index=None: "dev0")
    monkeypatch.setattr(D, "is_tensor", lambda x: isinstance(x, FakeTensor))
    monkeypatch.setattr(D, "_pin_pool", {})
    monkeypatch.setattr(D, "_SIDE_STREAMS", {})
    return torch


def run_threads(fns, timeout: float = WAIT) -> list:
    """Run ``fns`` in one thread each; their results in order.  A worker's exception or a join that times out fails."""
    out, errs = [None] * len(fns), []

    def body(i):
        try:
            out[i] = fns[i]()
        except BaseException as exc:  # noqa: BLE001
            errs.append((i, exc))

    ths = [threading.Thread(target=body, args=(i,), name=f"worker{i}", daemon=True) for i in range(len(fns))]
    for t in ths:
        t.start()
    for t in ths:
        t.join(timeout)
    assert not [t.name for t in ths if t.is_alive()], "a worker did not finish"
    if errs:
        raise errs[0][1]
    return out


class CountingLock:
    """A lock that counts the threads that have come to it (those that hold it, wait for it, or have passed it)."""

    def __init__(self):
        self._lock, self._mu, self.arrivals = threading.Lock(), threading.Condition(), 0

    def __enter__(self):
        with self._mu:
            self.arrivals += 1
            self._mu.notify_all()
        self._lock.acquire()
        return self

    def __exit__(self, *exc):
        self._lock.release()
        return False

    def wait_for(self, pred) -> None:
        with self._mu:
            assert self._mu.wait_for(pred, WAIT), "the other threads never arrived"

    def poke(self) -> None:
        with self._mu:
            self._mu.notify_all()


# ---- _dev._upload: the pinned upload pool --------------------------------------------------------------------------------


def _pattern(i: int, nbytes: int = 64) -> np.ndarray:
    return ((np.arange(nbytes) * 7 + 31 * (i + 1)) % 251).astype(np.uint8)


@pytest.mark.parametrize("n_threads", [2, 4])
def test_upload_pool_gives_every_concurrent_upload_its_own_slot(fake, n_threads):
    """One free slot in the pool, ``n_threads`` uploads of distinct arrays at once, every thread held (in the allocation
    of its device tensor) until all have chosen a slot and staged their bytes; the copies complete only afterwards.  Every
    device tensor holds its own bytes, no pinned buffer is the source of two copies in flight, a slot is not reused while
    its copy is in flight and is reused once its event has completed."""
    first = D._upload(fake, _pattern(99))
    fake.complete_all()
    assert np.array_equal(first.read(), _pattern(99)) and [len(v) for v in D._pin_pool.values()] == [1]
    (slots,) = D._pin_pool.values()

    gate = threading.Barrier(n_threads)
    fake.hooks["empty_device"] = lambda: gate.wait(WAIT)
    devs = run_threads([lambda i=i: D._upload(fake, _pattern(i)) for i in range(n_threads)])
    fake.hooks.clear()
    assert fake.violations == []
    held = fake.sources_in_flight()
    assert len(held) == n_threads and len({id(r) for r in held}) == n_threads
    assert len(slots) == n_threads  # the free slot and n - 1 new ones
    # nothing has completed: one more upload must not take any of the slots in flight
    extra = D._upload(fake, _pattern(50))
    assert fake.violations == [] and len(slots) == n_threads + 1
    fake.complete_all()
    for i, dev in enumerate(devs):
        assert np.array_equal(dev.read(), _pattern(i)), f"thread {i} received another upload's bytes"
    assert np.array_equal(extra.read(), _pattern(50))
    # every event has completed: the next uploads reuse the slots, one after the other
    for k in range(3):
        again = D._upload(fake, _pattern(60 + k))
        fake.complete_all()
        assert np.array_equal(again.read(), _pattern(60 + k))
    assert len(slots) == n_threads + 1 and fake.violations == []
    assert not any(s[2] for s in slots)  # no claim outlives its upload


def test_upload_pool_single_thread_reuses_one_slot_in_order(fake):
    """The single-threaded path is what it was: one slot per size class while every copy has completed before the next
    upload, a second slot only while the first is in flight; other size classes have pools of their own."""
    for k in range(4):
        dev = D._upload(fake, _pattern(k))
        fake.complete_all()
        assert np.array_equal(dev.read(), _pattern(k))
    assert {c: len(v) for c, v in D._pin_pool.items()} == {256: 1}
    a = D._upload(fake, _pattern(7))
    b = D._upload(fake, _pattern(8))  # a's copy is in flight
    big = D._upload(fake, _pattern(9, 1000).view(np.int16))
    assert {c: len(v) for c, v in D._pin_pool.items()} == {256: 2, 1024: 1}
    fake.complete_all()
    assert np.array_equal(a.read(), _pattern(7)) and np.array_equal(b.read(), _pattern(8))
    assert big.dtype == np.int16 and np.array_equal(big.read(), _pattern(9, 1000).view(np.int16))
    assert fake.violations == []


def test_upload_that_fails_does_not_leave_a_claimed_slot(fake):
    def boom():
        raise MemoryError("no device memory")

    fake.hooks["empty_device"] = boom
    with pytest.raises(MemoryError):
        D._upload(fake, _pattern(1))
    fake.hooks.clear()
    assert [len(v) for v in D._pin_pool.values()] == [0]
    dev = D._upload(fake, _pattern(2))
    fake.complete_all()
    assert np.array_equal(dev.read(), _pattern(2))


# ---- _dev.side_stream ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_threads", [2, 4])
def test_side_stream_first_requests_share_one_stream(fake, monkeypatch, n_threads):
    """Concurrent first requests for one (device, role): the stream's constructor does not return before every thread has
    either entered it too or come to the table's lock.  All get the same object, made once."""
    lock = CountingLock()
    monkeypatch.setattr(D, "_SIDE_STREAMS_LOCK", lock, raising=False)

    def held():
        lock.poke()
        lock.wait_for(lambda: lock.arrivals >= n_threads or fake.streams_made >= n_threads)

    fake.hooks["Stream"] = held
    start = threading.Barrier(n_threads)

    def request():
        start.wait(WAIT)
        return D.side_stream("tail")

    got = run_threads([request] * n_threads)
    assert all(s is got[0] for s in got) and fake.streams_made == 1
    fake.hooks.clear()
    assert D.side_stream("tail") is got[0] and D.side_stream("aux") is not got[0]
    assert D.side_stream("tail", 1) is not got[0] and fake.streams_made == 3


# ---- mixsign: the probes' pinned read-back buffers -----------------------------------------------------------------------


def test_pinned_scalars_have_one_owner_and_come_back(fake, monkeypatch):
    from iq_to_audio_amd import mixsign as M

    monkeypatch.setattr(M, "_PINNED_SCALARS", [])
    n, rounds = 4, 25
    mu, owned = threading.Lock(), {}
    phase = threading.Barrier(n)

    def worker(i):
        for r in range(rounds):
            buf = M._pinned_scalars(("owner", i, r))
            with mu:
                assert id(buf) not in owned, "a read-back buffer was handed to two probes"
                owned[id(buf)] = i
            phase.wait(WAIT)  # all n hold one now
            with mu:
                assert len(owned) == n
            phase.wait(WAIT)
            with mu:
                del owned[id(buf)]
            M._release_scalars(buf)
            phase.wait(WAIT)

    run_threads([lambda i=i: worker(i) for i in range(n)])
    assert len(M._PINNED_SCALARS) == n  # released buffers were handed out again, round after round
    assert all(t[1] is None for t in M._PINNED_SCALARS) and len({id(t[0]) for t in M._PINNED_SCALARS}) == n
    # reservations from two threads at once, while two buffers are taken
    taken = [M._pinned_scalars("a"), M._pinned_scalars("b")]
    run_threads([lambda: M.reserve_pinned_scalars(5)] * 2)
    free = [t for t in M._PINNED_SCALARS if t[1] is None]
    assert len(free) >= 5 and len(M._PINNED_SCALARS) == len({id(t[0]) for t in M._PINNED_SCALARS}) <= 2 + 5 + 5
    assert all(not any(t[0] is b for t in free) for b in taken)


# ---- _BlockStager: the pool of pinned staging buffers, and fetch against a pending prefetch --------------------------------


def test_block_stager_pool_under_threads(fake, monkeypatch):
    from iq_to_audio_amd.staging import _BlockStager

    max_frames, n, rounds = 512, 4, 6
    nbytes = 2 * max_frames * 2
    monkeypatch.setattr(_BlockStager, "_POOL", {})
    monkeypatch.setattr(_BlockStager, "_POOL_MAX_BYTES", 5 * nbytes)  # the cap bites: 8 buffers come back per round
    frames = np.arange(2 * max_frames, dtype=np.int16)
    phase = threading.Barrier(n)
    mu, held = threading.Lock(), {}

    def pool_bytes():
        with _BlockStager._POOL_LOCK:
            pooled = [t for st in _BlockStager._POOL.values() for t in st]
        assert len({id(t) for t in pooled}) == len(pooled), "a buffer is in the pool twice"
        return pooled, sum(t.numel() * t.element_size() for t in pooled)

    def worker(i):
        for _ in range(rounds):
            st = _BlockStager(frames, "int16", max_frames)
            bufs = [st._buf(0), st._buf(1)]
            assert st._buf(0) is bufs[0] and bufs[0] is not bufs[1]
            with mu:
                for b in bufs:
                    assert id(b) not in held, "one pinned buffer in two stagers"
                    held[id(b)] = i
            phase.wait(WAIT)  # every stager holds its two buffers
            pooled, size = pool_bytes()
            assert size <= _BlockStager._POOL_MAX_BYTES
            with mu:
                assert not any(id(t) in held for t in pooled), "a buffer in use is also in the pool"
            phase.wait(WAIT)
            with mu:
                for b in bufs:
                    del held[id(b)]
            st.close()
            assert st.bufs == [None, None]
            assert pool_bytes()[1] <= _BlockStager._POOL_MAX_BYTES
            phase.wait(WAIT)

    run_threads([lambda i=i: worker(i) for i in range(n)])
    pooled, size = pool_bytes()
    assert size == 5 * nbytes and len(pooled) == 5


def test_fetch_waits_for_a_pending_prefetch_of_other_bounds(fake):
    """``fetch(lo, hi)`` while the helper thread of ``prefetch(lo', hi')`` is still filling: both use buffer
    ``slot ^ 1``.  (Not reachable from ``MultiChannelPipeline._run_blocks``, which fetches exactly what it prefetched;
    ``fetch`` joins the helper all the same.)  The helper is held inside its copy until ``fetch`` either joins it or --
    the defect -- starts its own copy into the same buffer."""
    from iq_to_audio_amd.staging import _BlockStager

    frames = np.arange(2 * 4096, dtype=np.int16)
    st = _BlockStager(frames, "int16", 1024)
    active, overlaps = [0, 0], []
    gate, mu = threading.Event(), threading.Lock()
    real_fill = st._fill

    def fill(slot, lo, hi):
        with mu:
            if active[slot]:
                overlaps.append((slot, lo, hi))
                gate.set()  # (let the helper go: the overlap has been seen)
            active[slot] += 1
        if threading.current_thread().name == "iq-stager":
            assert gate.wait(WAIT)
        real_fill(slot, lo, hi)
        with mu:
            active[slot] -= 1

    st._fill = fill

    class JoinSpy:
        def __init__(self, th):
            self.th, self.joined = th, False

        def join(self):
            self.joined = True
            gate.set()
            self.th.join(WAIT)
            assert not self.th.is_alive()

    try:
        st.prefetch(0, 1024)
        spy = JoinSpy(st.pending[0])
        st.pending = (spy,) + st.pending[1:]
        dev = st.fetch(2048, 3072)
        assert spy.joined and overlaps == []
        assert st.pending is None
        fake.complete_all()
        assert np.array_equal(dev.read(), frames[2 * 2048 : 2 * 3072])
        # and the matching case: the prefetched block is the one fetched, filled once
        st.prefetch(3072, 4096)
        dev = st.fetch(3072, 4096)
        fake.complete_all()
        assert np.array_equal(dev.read(), frames[2 * 3072 : 2 * 4096]) and overlaps == []
    finally:
        gate.set()
        st.close()


# ---- the kernel cache and the resampler tables: usable under concurrent requests, published after their uploads ---------


class _LoggingDict(OrderedDict):
    """A cache that notes every insertion in the stand-in's log and checks the inserted object's uploads."""

    def __init__(self, torch, tensors_of):
        super().__init__()
        self.torch, self.tensors_of, self.bad = torch, tensors_of, []

    def __setitem__(self, key, value):
        for t in self.tensors_of(value):
            if self.torch.in_flight(t):
                self.bad.append(key)
        self.torch.note("cache_insert")
        super().__setitem__(key, value)


def _order_ok(log, thread: str) -> bool:
    """In ``thread``'s own events: every copy queued before an insertion is followed by a synchronisation before it."""
    pending = False
    for what, who in log:
        if who != thread:
            continue
        if what == "copy_queued":
            pending = True
        elif what in ("stream_sync", "event_sync"):
            pending = False
        elif what == "cache_insert" and pending:
            return False
    return True


def test_cached_kernel_is_published_after_its_uploads(fake, monkeypatch):
    """Identical concurrent requests: every caller gets a usable (plan, kernel); whatever reaches ``_KERNEL_CACHE`` -- where
    a thread on another stream can take it -- has no upload in flight (order per builder: copies queued, stream
    synchronised, inserted).  The same for the lazily planned matrix-core fragments, which ``_ensure_mfma`` publishes
    under the kernel's own lock."""
    import iq_to_audio_amd as pkg
    from iq_to_audio_amd import channelizer as C
    from iq_to_audio_amd import dsp_plan as P

    cache = _LoggingDict(fake, lambda v: [v[2].taps_dev])
    monkeypatch.setattr(C, "_KERNEL_CACHE", cache)
    fs = 2.5e6
    d, _ = P.choose_decimation(fs, 96_000.0)
    taps = pkg.design_channel_filter(fs, 12_500.0, d)
    n = 3
    start = threading.Barrier(n)
    # all builders queue their tap upload before any of them goes on: an insertion without a wait would be caught
    staged = threading.Barrier(n)
    fake.hooks["empty_device"] = lambda: staged.wait(WAIT)

    def request():
        start.wait(WAIT)
        return C._cached_kernel(taps, sample_rate=fs, freq_offset=25e3, mix_sign=1, decimation=d, fmt="s16", iq_order="iq")

    got = run_threads([request] * n)
    fake.hooks.clear()
    assert cache.bad == [] and len(cache) == 1
    assert all(_order_ok(fake.log, f"worker{i}") for i in range(n))
    assert sum(1 for what, _ in fake.log if what == "cache_insert") >= 1
    for plan, kernel in got:
        assert plan.decimation == d and not fake.in_flight(kernel.taps_dev)
        assert np.array_equal(kernel.taps_dev.read(), plan.taps_window.reshape(-1))
    # a later request is a hit: the published kernel, no upload, no wait
    before = len(fake.log)
    plan, kernel = request_hit = C._cached_kernel(taps, sample_rate=fs, freq_offset=25e3, mix_sign=1, decimation=d, fmt="s16",
                                                  iq_order="iq")
    assert kernel is next(iter(cache.values()))[2] and len(fake.log) == before and request_hit[0] is plan

    assert kernel._mfma_ok
    start2 = threading.Barrier(n)

    def plan_mfma():
        start2.wait(WAIT)
        mp = kernel._ensure_mfma()
        assert all(not fake.in_flight(t) for t in kernel.afrag_dev), "fragments published with their copy in flight"
        return mp

    mps = run_threads([plan_mfma] * n)
    assert all(m is mps[0] for m in mps)
    assert sum(1 for what, _ in fake.log[before:] if what == "copy_queued") == len(kernel.afrag_dev)  # planned once
    for g, t in zip(mps[0].groups, kernel.afrag_dev):
        assert np.array_equal(t.read(), g.afrag.reshape(-1).view(np.uint8))


def test_resampler_table_is_published_after_its_upload(fake, monkeypatch):
    from iq_to_audio_amd import channel_demod as CD

    tables = _LoggingDict(fake, lambda v: [v])
    monkeypatch.setattr(CD.Resampler48k, "_TABLES", tables)
    monkeypatch.setattr(D, "_PIN_LIMIT", 1 << 30)  # the table through the asynchronous path (it is a blocking copy above 1 MiB)
    n = 3
    start, staged = threading.Barrier(n), threading.Barrier(n)
    fake.hooks["empty_device"] = lambda: staged.wait(WAIT)

    def make():
        start.wait(WAIT)
        return CD.Resampler48k(2.5e6 / 26)

    got = run_threads([make] * n)
    fake.hooks.clear()
    assert tables.bad == [] and len(tables) == 1
    assert all(_order_ok(fake.log, f"worker{i}") for i in range(n))
    for rs in got:
        assert not fake.in_flight(rs.table_dev) and np.array_equal(rs.table_dev.read(), rs.plan.table.reshape(-1))
    assert CD.Resampler48k(2.5e6 / 26).table_dev is next(iter(tables.values()))


# ---- the real library: one handle, and a thread-local error string -------------------------------------------------------


@pytest.mark.parametrize("n_threads", [2, 6])
def test_native_lib_first_call_from_threads_loads_once(monkeypatch, n_threads):
    """``n_threads`` make the process's "first" call of ``_native.lib()`` at once.  The loader (``ctypes.CDLL``) does not
    return before every other thread has entered it too or come to the load lock: one load, one handle for all, every
    signature bound."""
    N.build()
    lock = CountingLock()
    monkeypatch.setattr(N, "_lib", None)
    monkeypatch.setattr(N, "_LIB_LOCK", lock, raising=False)
    real, loads = ctypes.CDLL, []

    def cdll(path, *a, **kw):
        loads.append(threading.current_thread().name)
        lock.poke()
        lock.wait_for(lambda: lock.arrivals >= n_threads or len(loads) >= n_threads)
        return real(path, *a, **kw)

    monkeypatch.setattr(ctypes, "CDLL", cdll)
    start = threading.Barrier(n_threads)

    def first_call():
        start.wait(WAIT)
        return N.lib()

    got = run_threads([first_call] * n_threads)
    assert len(loads) == 1 and all(h is got[0] for h in got) and N.lib() is got[0]
    for name, (res, args) in N._SIGNATURES.items():
        fn = getattr(got[0], name)
        assert fn.restype is res and list(fn.argtypes or []) == list(args), name
    assert got[0].iqa_abi_version() == N.ABI_VERSION


def test_last_error_is_per_thread():
    """Two threads, released together, alternate 100 rejections each: ``iqa_decimate`` with D = 0 in one,
    ``iqa_gate_power`` with sh = 99 in the other, in lock step (both have failed before either reads).  Each reads its
    own message; a thread that has made no failing call reads an empty string."""
    lib = N.lib()
    step = threading.Barrier(2)

    def decimate():
        return lib.iqa_decimate(c_void_p(0), c_int64(10), c_int64(0), c_int32(0), c_void_p(0), c_int64(1), c_void_p(0))

    def gate_power():
        return lib.iqa_gate_power(c_void_p(0), c_int64(10), c_int64(0), c_int32(99), c_void_p(0), c_void_p(0))

    def worker(fail, want):
        seen = set()
        step.wait(WAIT)
        for _ in range(100):
            assert fail() == N.IQA_EINVAL
            step.wait(WAIT)  # both have failed ...
            seen.add((lib.iqa_last_error() or b"").decode())
            step.wait(WAIT)  # ... and both have read
        assert seen == {want}, seen
        return seen

    run_threads([lambda: worker(decimate, "invalid argument: bad decimate sizes"),
                 lambda: worker(gate_power, "invalid argument: sh must be -30 .. 30")])
    assert run_threads([lambda: (lib.iqa_last_error() or b"").decode()]) == [""]
    # through the shim: the exception carries the calling thread's message
    def shim():
        with pytest.raises(ValueError, match="bad decimate sizes"):
            N.call("iqa_decimate", c_void_p(0), c_int64(10), c_int64(0), c_int32(0), c_void_p(0), c_int64(1), c_void_p(0))
        return True

    assert run_threads([shim, shim]) == [True, True]
