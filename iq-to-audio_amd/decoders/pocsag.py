"""POCSAG paging beside narrowband FM: 512, 1200 and 2400 baud, all searched at once.

Per block ``iqa_pocsag_integrate`` quantises the discriminator output and appends the bit integrators of the three baud
rates to the run's stored planes; once per run ``iqa_pocsag_sync`` evaluates the sync correlator at every sample and baud
and keeps the local maxima, and ``iqa_pocsag_codewords`` reads, checks and corrects the 16 codewords behind every kept
sync.  Every batch carries its own sync word, so timing is re-acquired per batch by search: there is no loop.  Message
assembly is integer host logic on the codewords and runs on plain numpy arrays as well (``parse_batches``)."""
from __future__ import annotations

from ctypes import c_int32, c_int64, c_void_p
from dataclasses import asdict, dataclass, field

import numpy as np

from .. import _dev as D
from .. import _native as N
from .. import dsp_plan as P
from .common import SideStage, StreamCore, search_with_room

SYNC_WORD = 0x7CD215D8
IDLE_WORD = 0x7A89C197
BCH_POLY = 0x769  # x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1
NUMERIC = "0123456789*U -]["
FUNCTION_KIND = ("numeric", "alpha", "alpha", "alpha")  # by function code 0 .. 3
STATUS = ("ok", "corrected", "uncorrectable", "absent")


@dataclass
class PocsagMessage:
    time_s: float  # of the address codeword's first bit instant
    baud: int
    inverted: bool
    address: int
    function: int
    kind: str  # "numeric" for function 0, else "alpha"
    text: str
    payload_bits: int
    corrected: int  # codewords of the message (address included) with status 1
    batches: int  # batches the message touches
    payload: str = ""  # the raw payload bits, first transmitted bit first, as hex (zero-padded to whole digits)

    def line(self) -> str:
        return f'POCSAG{self.baud} addr={self.address} func={self.function} {self.kind} "{self.text}"'


@dataclass
class PocsagResult:
    messages: list = field(default_factory=list)  # PocsagMessage, in order of time
    syncs: dict = field(default_factory=dict)  # baud -> kept syncs
    codewords: dict = field(default_factory=dict)  # status name -> count
    bauds_skipped: list = field(default_factory=list)
    dc_hz: float | None = None  # median tuning error seen by the sync words
    orphans: int = 0  # message codewords without an open message

    def to_json(self) -> dict:
        out = asdict(self)
        out["syncs"] = {str(k): v for k, v in self.syncs.items()}
        return out


def _numeric(bits: list) -> str:
    out = []
    for i in range(0, len(bits) - 3, 4):
        b = bits[i : i + 4]
        out.append(NUMERIC[b[0] | (b[1] << 1) | (b[2] << 2) | (b[3] << 3)])  # each group LSB first
    return "".join(out)


def _alpha(bits: list) -> str:
    codes = []
    for i in range(0, len(bits) - 6, 7):
        codes.append(sum(bit << k for k, bit in enumerate(bits[i : i + 7])))
    while codes and codes[-1] in (0x00, 0x03, 0x04):  # NUL, ETX, EOT
        codes.pop()
    return "".join(chr(c) if 0x20 <= c <= 0x7E else "�" for c in codes)


def parse_batches(plan: P.PocsagPlan, batches: dict) -> PocsagResult | None:
    """``batches``: baud -> dict(n0=int64[k], sigma=int64[k], inverted=[k], words=uint32[k, 16], status=uint8[k, 16]) in
    any order -> the run's messages.  Integer logic only; ``None`` when no baud has a kept sync."""
    res = PocsagResult(bauds_skipped=list(plan.skipped), codewords={s: 0 for s in STATUS})
    dcs = []
    for pb in plan.bauds:
        got = batches.get(pb.baud)
        n0 = np.zeros(0, dtype=np.int64) if got is None else np.asarray(got["n0"], dtype=np.int64).reshape(-1)
        res.syncs[pb.baud] = int(n0.size)
        if not n0.size:
            continue
        order = np.argsort(n0, kind="stable")
        n0 = n0[order]
        sigma = np.asarray(got["sigma"], dtype=np.int64).reshape(-1)[order]
        inverted = np.asarray(got["inverted"]).reshape(-1)[order]
        words = np.asarray(got["words"]).astype(np.int64).reshape(-1, 16)[order]
        status = np.asarray(got["status"]).astype(np.int64).reshape(-1, 16)[order]
        for s in sigma.tolist():
            dcs.append(s * plan.fs / (32.0 * pb.L * 2.0 ** P.POCSAG_THETA_BITS * 2.0 * np.pi))
        span = int(pb.offsets[P.POCSAG_BATCH_BITS])
        msg = None  # the open message
        bits: list = []

        def close():
            nonlocal msg, bits
            if msg is not None:
                msg.payload_bits = len(bits)
                msg.text = _numeric(bits) if msg.function == 0 else _alpha(bits)
                pad = bits + [0] * (-len(bits) % 4)
                msg.payload = "".join(f"{pad[i] << 3 | pad[i + 1] << 2 | pad[i + 2] << 1 | pad[i + 3]:x}" for i in range(0, len(pad), 4))
                res.messages.append(msg)
            msg, bits = None, []

        for k in range(n0.size):
            if k and abs(int(n0[k]) - (int(n0[k - 1]) + span)) > pb.h:
                close()  # a missing continuation
            if msg is not None:
                msg.batches += 1
            for c in range(16):
                st, cw = int(status[k, c]), int(words[k, c])
                res.codewords[STATUS[st]] += 1
                if st >= 2 or cw == IDLE_WORD:
                    close()
                elif cw >> 31 == 0:
                    close()
                    fn = (cw >> 11) & 3
                    msg = PocsagMessage(time_s=(int(n0[k]) + int(pb.offsets[32 * (1 + c)])) / plan.fs, baud=pb.baud,
                                        inverted=bool(inverted[k]), address=((cw >> 13) & 0x3FFFF) << 3 | (c >> 1), function=fn,
                                        kind=FUNCTION_KIND[fn], text="", payload_bits=0, corrected=int(st == 1), batches=1)
                elif msg is None:
                    res.orphans += 1
                else:
                    msg.corrected += int(st == 1)
                    bits.extend((cw >> s) & 1 for s in range(30, 10, -1))
        close()
    if not dcs:
        return None
    res.messages.sort(key=lambda m: (m.time_s, m.baud))
    res.dc_hz = float(np.median(np.asarray(dcs, dtype=np.float64)))
    return res


class PocsagCore(StreamCore):
    """Per-stream device state (``StreamCore``): the carried quantised history, the absolute position, and the growing store
    of the integrator planes (one device tensor per block and baud, joined by ``finish``).  ``keep_t`` also stores t."""

    def __init__(self, plan: P.PocsagPlan, *, keep_t: bool = False):
        super().__init__(plan, plan.hist_len, {"t": None, **{pb.baud: "int32" for pb in plan.bauds}})
        self._windows = (c_int32 * 3)(*plan.lengths())
        self._active = [i for i, L in enumerate(plan.lengths()) if L]  # slots of P.POCSAG_BAUDS that run, in the order of plan.bauds
        self._offsets_dev = {pb.baud: D.from_numpy(np.ascontiguousarray(pb.offsets)) for pb in plan.bauds}
        self.keep_t = keep_t

    def _block(self, theta, n: int):
        """One block of the discriminator output (device float32[n], radians per sample)."""
        t = D.empty(n, "int32")
        outs = (c_void_p * 3)()
        for slot, pb in zip(self._active, self.plan.bauds):
            plane = D.empty(n, "int32")
            outs[slot] = plane.data_ptr()
            self.store.append(pb.baud, plane)
        N.call("iqa_pocsag_integrate", N.ptr(theta), c_int64(n), N.ptr(self._hist), c_int32(self.hist_len), self._windows, N.ptr(t),
               outs, N.stream_ptr())
        if self.keep_t:
            self.store.append("t", t)
        return t

    def joined(self) -> dict:
        return dict(t=self.store.joined("t"), S={pb.baud: self.store.joined(pb.baud) for pb in self.plan.bauds})

    def _search(self, pb, s, score, capacity: int, count):
        lst = D.empty(4 * capacity, "int64")
        offs = (c_int32 * 32)(*[int(v) for v in pb.offsets[:32]])
        N.call("iqa_pocsag_sync", N.ptr(s), c_int64(int(s.numel())), offs, c_int32(pb.h), N.ptr(score), N.ptr(lst), c_int64(capacity),
               N.ptr(count), N.stream_ptr())
        return lst

    def finish(self) -> dict:
        """The sync search and the codewords of the stored run: baud -> dict(n0, sigma, inverted, distance, words, raw,
        status) as numpy arrays sorted by n0.  The searches of all bauds are queued before the one read-back of their
        counts; the codeword kernel reads the device list as the search left it, and the rows are sorted on the host."""
        st = self.joined()
        bauds = self.plan.bauds
        counts = D.zeros(len(bauds), "int64")
        score = D.empty(max(max(int(st["S"][pb.baud].numel()) for pb in bauds), 1), "int64")  # (shared: stream order)
        searches = [lambda capacity, i=i, pb=pb: self._search(pb, st["S"][pb.baud], score, capacity, counts[i : i + 1])
                    for i, pb in enumerate(bauds)]
        lists, kept = search_with_room(searches, counts, 1024)
        words_dev = []
        for i, pb in enumerate(bauds):
            k, s = kept[i], st["S"][pb.baud]
            both, status = D.empty(32 * k, "int32"), D.empty(16 * k, "uint8")  # [corrected | raw]
            if k:
                N.call("iqa_pocsag_codewords", N.ptr(s), c_int64(int(s.numel())), N.ptr(lists[i]), c_int64(k),
                       N.ptr(self._offsets_dev[pb.baud]), N.ptr(both), N.ptr(both[16 * k :]), N.ptr(status), N.stream_ptr())
            words_dev.append((both, status))
        out = {}
        for i, pb in enumerate(bauds):
            k = kept[i]
            entries = lists[i][: 4 * k].cpu().numpy().reshape(-1, 4)
            order = np.argsort(entries[:, 0], kind="stable")
            entries = entries[order]
            both = words_dev[i][0].cpu().numpy().view(np.uint32).reshape(2, k, 16)
            status = words_dev[i][1].cpu().numpy().reshape(k, 16)
            out[pb.baud] = dict(n0=entries[:, 0].copy(), sigma=entries[:, 1].copy(), inverted=entries[:, 2].astype(bool),
                                distance=entries[:, 3].astype(np.int32), words=both[0][order], raw=both[1][order], status=status[order])
        return out

    def result(self, fin=None, **context) -> PocsagResult | None:
        """The run's ``PocsagResult`` (``None`` without a kept sync); ``fin``: a ``finish()`` made earlier."""
        return parse_batches(self.plan, self.finish() if fin is None else fin)


class PocsagDecoder(SideStage):
    """The stage API: ``process(block)`` per block of the channel (complex: the channelizer's output, run through
    ``iqa_quadrature`` with this decoder's own ``prev``; or float32: a discriminator output in radians per sample),
    ``finish()`` once (a ``PocsagResult``, or ``None`` without a kept sync), ``stages()`` for the tests."""

    def __init__(self, rate: float, *, keep_t: bool = True):
        super().__init__(PocsagCore(P.plan_pocsag(float(rate)), keep_t=keep_t), keep=keep_t)

    def stages(self) -> dict:
        """Host copies: ``theta`` and ``t`` (with keep_t), ``S`` (baud -> int32[n]) and ``batches`` (baud -> kept syncs
        sorted by n0 with their corrected words, raw words and status)."""
        fin = self._finished()
        st = self.core.joined()
        return dict(theta=self._inputs_host(), t=None if st["t"] is None else st["t"].cpu().numpy(),
                    S={b: s.cpu().numpy() for b, s in st["S"].items()}, batches=fin)
