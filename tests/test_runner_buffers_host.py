"""Host-side halves of the resident runners' buffer contract (no GPU; tests/test_gpu_runner_buffers.py holds the rest):

* ``mixsign.level_window`` -- where ``queue_raw_level`` starts reading a warm-up block that does not begin on a 16-byte
  boundary (a capture behind a lead-in of a few frames).  ``iqa_raw_level`` itself refuses such a pointer and stays so.
* ``batch.GraphBook`` -- which captured graph ``submit_captured`` / ``submit_captured_batch`` replay, driven by a stand-in
  runner that keeps the real runner's order of events (slot rotation, runner-wide speculation for the ordinary runs,
  probes read at collect) and counts what a GPU would have had to do.
"""
from __future__ import annotations

import numpy as np
import pytest

from iq_to_audio_amd.batch import GraphBook
from iq_to_audio_amd.mixsign import LEVEL_VECTOR_BYTES, level_window

ITEM = {"s16": 2, "u8": 1, "f32": 4}
LENGTHS = (0, 1, 15, 16, 17, 33, 1000)  # values (not bytes); 0 .. 17 straddle one vector of every format


def library_refuses(address: int, n_values: int, value_bytes: int) -> bool:
    """The rule of iqa_raw_level (csrc/demod.hip): a pointer off the 16-byte grid is an error once there is a whole vector to read."""
    return n_values // (LEVEL_VECTOR_BYTES // value_bytes) > 0 and address % LEVEL_VECTOR_BYTES != 0


@pytest.mark.parametrize("fmt", sorted(ITEM))
@pytest.mark.parametrize("phase", range(16))
def test_level_window_every_byte_phase_and_short_lengths(fmt, phase):
    """Every byte phase 0..15 of the run's first value against a 16-byte boundary, run lengths around one vector: the
    window starts on the first boundary at or behind the run's start (never further than 15 bytes in), never leaves the
    run, keeps every value from there on, and is never one the library refuses.  A phase no tensor of that type can have
    (off the value's own size) is an error, not a guess."""
    size = ITEM[fmt]
    base = 0x7F00_0000_1000
    for n in LENGTHS:
        if phase % size:
            with pytest.raises(ValueError):
                level_window(base + phase, n, size)
            continue
        skip, count = level_window(base + phase, n, size)
        assert 0 <= skip and 0 <= count and skip + count == n, (n, skip, count)
        assert skip * size < LEVEL_VECTOR_BYTES
        assert skip * size == min((-phase) % 16, n * size), (n, skip)  # the FIRST boundary, or the run's end before it
        assert not library_refuses(base + phase + skip * size, count, size), (n, skip, count)
        if phase == 0:
            assert (skip, count) == (0, n)  # an aligned run is handed over as it stands: nothing changes for it
        # what the parent did (the run as it stands) is refused exactly where the issue says: a whole vector, off the grid
        assert library_refuses(base + phase, n, size) == (phase != 0 and n * size >= 16)


@pytest.mark.parametrize("fmt", sorted(ITEM))
def test_level_window_on_real_addresses(fmt):
    """The same on memory: views of one allocation at every value offset up to two vectors; the window's first value sits on
    a 16-byte boundary of the machine and the values behind it are the view's own."""
    dtype = {"s16": np.int16, "u8": np.uint8, "f32": np.float32}[fmt]
    size = ITEM[fmt]
    store = np.arange(4096, dtype=np.int64).astype(dtype)
    per_vec = 16 // size
    for off in range(2 * per_vec + 1):
        for n in (0, 1, per_vec - 1, per_vec, per_vec + 1, 777):
            view = store[off : off + n]
            skip, count = level_window(view.ctypes.data, view.size, size)
            win = view[skip : skip + count]
            assert win.size == count and skip + count == n
            if count >= per_vec:
                assert win.ctypes.data % 16 == 0 and win.ctypes.data - view.ctypes.data < 16
                assert np.array_equal(win, store[off + skip : off + n])
    with pytest.raises(ValueError):
        level_window(store.ctypes.data, 10, 3)


# ---- GraphBook on a stand-in runner ------------------------------------------------------------------------------------


class StandInRunner:
    """The bookkeeping of ResidentCaptureRunner's captured entries without a GPU: ``truth[buffer]`` is what a probe of the
    capture in that buffer says.  Ordinary runs start from the runner-wide speculation and are redone when the probe says
    otherwise; replays start from the speculation their graph was captured with."""

    SLOTS = 3

    def __init__(self, truth: dict, slots: int = 3):
        self.SLOTS, self.truth = slots, dict(truth)
        self.book = GraphBook()
        self.spec = (1, "fast")
        self.next = 0
        self.redone = self.replays_redone = self.ordinary = self.syncs = 0

    def _ordinary(self, buf):
        self.ordinary += 1
        self.next += 1
        if self.truth[buf] != self.spec:
            self.redone += 1
        self.spec = self.truth[buf]
        return self.spec

    def _capture(self, spec):
        self.syncs += 1  # (a device-wide synchronise comes with every capture)
        return dict(spec=tuple(spec), replays=0)

    def submit_captured(self, buf):
        index = self.next % self.SLOTS
        place = (buf, index)
        before = self.next
        entry = self.book.entry_for(place, lambda: [self._ordinary(buf)], self._capture)
        if self.next == before:
            self.next += 1
        entry["replays"] += 1
        return dict(place=(place, 0), ran=entry["spec"][0], buf=buf)

    def submit_captured_batch(self, bufs):
        place = ("batch",) + tuple(bufs)

        def run_ordinary():
            self.next = 0
            return [self._ordinary(b) for b in bufs]

        entry = self.book.entry_for(place, run_ordinary, self._capture)
        entry["replays"] += 1
        return [dict(place=(place, i), ran=entry["spec"][i], buf=b) for i, b in enumerate(bufs)]

    def collect(self, ticket):
        said = self.truth[ticket["buf"]]
        self.spec = said
        if said != ticket["ran"]:
            self.redone += 1
            self.replays_redone += 1
        self.book.probed(*ticket["place"], *said)
        return said

    def counters(self):
        return self.book.captures, self.redone, self.replays_redone, self.ordinary, self.syncs


PAIRS = [({"a": (1, "fast"), "b": (-1, "fast")}, 3), ({"a": (1, "fine"), "b": (1, "fast")}, 3), ({"a": (1, "fast"), "b": (-1, "fine")}, 8)]


@pytest.mark.parametrize("truth,slots", PAIRS, ids=["signs", "weak-strong", "both-8-slots"])
def test_alternating_buffers_settle_once_every_buffer_and_slot_has_been_met(truth, slots):
    """Two buffers in turn whose captures probe differently: after the rounds that bring every buffer into every slot it
    reaches, nothing is captured, synchronised, run the ordinary way or redone again, and no replay ever assumed the other
    buffer's speculation.  (Keyed on the runner-wide speculation, every call of this pattern missed its graph.)"""
    rn = StandInRunner(truth, slots)
    settled = None
    met = set()
    for rep in range(3 * slots):
        tickets = [rn.submit_captured(b) for b in ("a", "b")]
        for t in tickets:
            assert rn.collect(t) == truth[t["buf"]]
        new = {t["place"][0] for t in tickets} - met
        met |= new
        if new:
            settled = None
        elif settled is None:
            settled = rn.counters()
        else:
            assert rn.counters() == settled, (rep, rn.counters(), settled)
    assert settled is not None
    assert rn.book.captures == len(rn.book.graphs) == len(met) == rn.ordinary == rn.syncs
    assert rn.replays_redone == 0


def test_a_buffer_that_changes_sides_gets_a_second_graph_and_finds_the_first_again():
    rn = StandInRunner({"a": (1, "fast")}, slots=2)
    for _ in range(4):  # slots 0, 1, 0, 1
        rn.collect(rn.submit_captured("a"))
    assert rn.counters() == (2, 0, 0, 2, 2)
    rn.truth["a"] = (-1, "fast")  # new data in the same buffer, carrier on the other side
    rn.collect(rn.submit_captured("a"))  # slot 0: the +1 graph replays and is redone; the place now speculates -1
    assert (rn.book.captures, rn.replays_redone) == (2, 1)
    rn.collect(rn.submit_captured("a"))  # slot 1: the same
    rn.collect(rn.submit_captured("a"))  # slot 0: no -1 graph yet: ordinary run (right from the start), one capture
    rn.collect(rn.submit_captured("a"))  # slot 1
    assert (rn.book.captures, rn.replays_redone, rn.redone) == (4, 2, 2)
    before = rn.counters()
    for _ in range(4):
        rn.collect(rn.submit_captured("a"))
    assert rn.counters() == before
    rn.truth["a"] = (1, "fast")  # and back: one redone replay per slot, then the FIRST graphs again -- nothing captured
    for _ in range(6):
        rn.collect(rn.submit_captured("a"))
    assert (rn.book.captures, rn.replays_redone, rn.ordinary) == (4, 4, 4)


def test_batch_graph_holds_one_speculation_per_capture():
    """A batch graph is captured with each capture's own probed sign and precision, so the -1 buffer of a (+1, -1) batch is
    not redone at every replay, and a batch is never captured twice."""
    truth = {"a": (1, "fast"), "b": (-1, "fine"), "c": (1, "fast")}
    rn = StandInRunner(truth)
    for rep in range(4):
        for t in rn.submit_captured_batch(["a", "b", "c"]):
            assert rn.collect(t) == truth[t["buf"]]
        if rep == 0:
            first = rn.counters()
            assert rn.book.captures == 1 and rn.ordinary == 3 and rn.replays_redone == 0
            (entry,) = rn.book.graphs.values()
            assert entry["spec"] == ((1, "fast"), (-1, "fine"), (1, "fast"))
        assert rn.counters() == first
    # another order of the same buffers is another place; single captures of them are others again
    rn.submit_captured_batch(["b", "a"])
    rn.submit_captured("a")
    assert rn.book.captures == 3


def test_graph_book_probed_touches_only_its_part_and_known_places():
    book = GraphBook()
    book.probed(("nowhere", 0), 0, -1, "fine")  # a ticket of a place the book has never seen: nothing to remember
    assert book.spec == {} and book.lookup(("nowhere", 0)) is None
    made = []
    entry = book.entry_for("p", lambda: [(1, "fast"), (1, "fast")], lambda spec: made.append(spec) or {"spec": spec})
    assert entry == {"spec": ((1, "fast"), (1, "fast"))} and book.captures == 1
    book.probed("p", 1, -1, "fast")
    assert book.spec["p"] == ((1, "fast"), (-1, "fast")) and book.lookup("p") is None
    book.probed("p", 1, 1, "fast")
    assert book.lookup("p") is entry and made == [((1, "fast"), (1, "fast"))]
