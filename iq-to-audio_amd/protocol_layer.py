"""What the protocol layers behind section 25 share (``flex.py``, ``dmr.py``, ``p25.py``, ``ysf.py``, ``nxdn.py``; DESIGN.md, "Adding a
layer to the second pass"): the stored discriminator stream of one channel and its decoder (``join_theta``, ``StoredTheta``),
the shape of a device call on host rows (``device_rows``, ``slice_hits``) and the checks in front of one (``slice_frames``,
``word_rows``, ``frame_classes``), the keep rule across a protocol's patterns (``strongest_hits``, ``sync_hits``), the per-lane
loop of a layer's ``finish_*`` (``finish_lanes``), its result builder (``layer_result``), ``mostly_inverted``, its keys of
``stages()`` (``layer_stage_keys``), the declaration that ties these to one layer (``ProtocolLayer``: a module's ``LAYER``, with
``finish``, ``result_of`` and ``stage_keys``), the checks that more than one layer runs (``info_bytes``, ``crc_ccitt``,
``gf_tables``) and the mixins of the result classes (``JsonRecord``, ``ChannelLabel``, ``ChannelLines``).  A layer's module keeps
its plan, its own checks, its parser and its dataclasses.  Nothing here touches the GPU at import; ``identify.py``, which the
layers import, imports this module in turn."""
from __future__ import annotations

import ctypes
from ctypes import c_int32, c_int64
from dataclasses import asdict, dataclass
from typing import Callable

import numpy as np

from . import _dev as D
from . import _native as N
from . import dsp_plan as P


def join_theta(stored):
    """The stored blocks of one discriminator stream (device float32) as one device tensor: the single block, or the blocks
    joined, or an empty tensor.  Made anew by every call and kept by none: the stream can approach 2^30 samples."""
    if not stored:
        return D.empty(0, "float32")
    return stored[0] if len(stored) == 1 else D.torch_mod().cat(stored)


def checked_theta(stored):
    """``join_theta``, with ``ValueError`` for a stream longer than the sync search indexes (``IDENT_MAX_N``)."""
    theta = join_theta(stored)
    if int(theta.numel()) > P.IDENT_MAX_N:
        raise ValueError(f"a stored stream of {int(theta.numel())} samples is longer than 2^30")
    return theta


class StoredTheta:
    """A protocol decoder for one discriminator stream from Python: ``process(theta_block)`` per block (float32, radians per
    sample at ``fs_ch``), ``finish()`` once (the layer's result of one channel), ``stages()`` for the tests, ``reset()``.
    ``centre``: section 23's centre of the quantised stream.  The subclass names its plan function (``ValueError`` where
    ``fs_ch`` does not fit), the device planes that ``stages()`` moves to the host, and either what ``_decode`` runs (the
    ``patterns`` searched for on the plan's one integrated plane and the module's ``LAYER``, for its ``decode_stream``,
    ``channel_of`` and ``result``) or a ``_decode(theta)`` of its own: (the stages of the stream, its result)."""

    plan_of = None
    planes = ("v",)
    patterns = ()
    layer = None

    def __init__(self, fs_ch: float, centre: int = 0):
        self.plan = type(self).plan_of(fs_ch)
        self.centre = int(centre)
        self.reset()

    def reset(self) -> None:
        self._stored: list = []
        self._st = None
        self._result = None

    def process(self, theta_block) -> None:
        theta = D.to_device(theta_block, "float32").reshape(-1)
        if int(theta.numel()):
            self._stored.append(theta)
            self._st = self._result = None

    def finish(self):
        if self._result is None:
            self._st, self._result = self._decode(checked_theta(self._stored))
        return self._result

    def _decode(self, theta) -> tuple:
        from . import identify as I  # (identify imports this module)

        v = I.integrate(theta, self.plan.ident, self.centre)
        _, hits = I.search(v, self.plan.ident, self.patterns)
        st = self.layer.decode_stream(theta, self.plan, self.centre, hits, self.patterns, v)
        st["hits"] = hits
        return st, self.layer.result(channels=[self.layer.channel_of(st, self.plan.fs_ch, 0, 0.0, None)], sample_rate=self.plan.fs_ch)

    def stages(self) -> dict:
        """The stages of ``_decode`` with the planes on the host."""
        self.finish()
        st = dict(self._st)
        for name in self.planes:
            st[name] = None if st[name] is None else st[name].cpu().numpy()
        return st


class Out:
    """An output of ``device_rows``: ``cols`` values of the numpy type ``dtype`` to a row (uint32 travels as int32)."""

    def __init__(self, cols: int, dtype):
        self.cols, self.dtype = int(cols), np.dtype(dtype)


def device_rows(entry: str, k: int, empty: bool, *args) -> list:
    """Host rows in, one call of ``entry``, host arrays out.  ``args`` are the entry point's, in its order and less the stream: a
    ctypes value goes as it is, a device tensor as its pointer, a host array is uploaded, an ``Out`` is allocated for ``k`` rows
    and comes back as a host array [k][cols], in the order of the ``Out``s.  ``empty`` (nothing to read): the same call with
    every pointer NULL, which runs the entry point's checks and touches no device memory, and zeros come back."""
    passed = (c_int32, c_int64, ctypes.Array)
    if empty:
        N.call(entry, *(a if isinstance(a, passed) else N.ptr(None) for a in args), N.stream_ptr())
        return [np.zeros((k, a.cols), dtype=a.dtype) for a in args if isinstance(a, Out)]
    held = [D.empty(k * a.cols, "int32" if a.dtype == np.uint32 else a.dtype.name) if isinstance(a, Out)
            else D.from_numpy(a) if isinstance(a, np.ndarray) else a for a in args]
    N.call(entry, *(t if isinstance(t, passed) else N.ptr(t) for t in held), N.stream_ptr())
    return [t.cpu().numpy().view(a.dtype).reshape(k, a.cols) for a, t in zip(args, held) if isinstance(a, Out)]


def slice_hits(entry: str, plane, rows, offsets, words: int) -> tuple:
    """An ``iqa_*_slice`` on a device int32 plane for the checked ``rows`` (int64[K][..], a hit each) with the plan's ``offsets``:
    (bits uint32[K][words], levels int64[K][3]) on the host."""
    n, k = int(plane.numel()), rows.shape[0]
    return tuple(device_rows(entry, k, n == 0 or k == 0, plane, c_int64(n), rows, c_int64(k), (c_int32 * len(offsets))(*offsets),
                             Out(words, np.uint32), Out(3, np.int64)))


def slice_frames(entry: str, plane, rows, offsets, words: int) -> tuple:
    """``slice_hits`` for ``rows`` of (m, s) (int64[K][2]), with ``ValueError`` for a sign other than +-1 before anything is
    launched: the ``slice_frames`` of a layer whose hits carry no kind."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 2))
    if rows.size and not np.isin(rows[:, 1], (-1, 1)).all():
        raise ValueError(f"{entry}: a hit's sign must be +-1")
    return slice_hits(entry, plane, rows, offsets, words)


def word_rows(bits, words: int) -> np.ndarray:
    """``bits`` as contiguous uint32[K][words]: the sliced frames that a decode entry point takes."""
    return np.ascontiguousarray(np.asarray(bits, dtype=np.uint32).reshape(-1, words))


def frame_classes(entry: str, bits, classes, noun: str, top: int, span: str) -> np.ndarray:
    """The ``classes`` that pick the decoders of the frames ``bits`` (``word_rows``' form) as int64[K], checked before anything is
    launched: ``ValueError`` unless there is one ``noun`` to a frame and each is 0 .. ``top`` (``span`` in the message)."""
    classes = np.asarray(classes, dtype=np.int64).reshape(-1)
    if classes.shape[0] != bits.shape[0]:
        raise ValueError(f"{entry}: one {noun} to a frame")
    if classes.size and not ((classes >= 0) & (classes <= top)).all():
        raise ValueError(f"{entry}: a {noun} must be {span}")
    return classes


def sync_hits(hits, pats, protocol: str, half: int) -> np.ndarray:
    """int64[K][2], (m, s) in order of m: of the kept hits (int64[K][6] of section 25, ``pats`` the patterns searched for) every
    hit of the one pattern of ``protocol``, less those with another within +-``half`` that has a larger |C|, or the same |C| at a
    smaller m (section 29's keep rule): the ``frame_hits`` of a layer with one sync word."""
    cand = []
    for p, m, c, _e, _pre, _post in np.asarray(hits, dtype=np.int64).reshape(-1, P.IDENT_RECORD).tolist():
        if pats[p].protocol == protocol and c != 0:
            cand.append((m, -abs(c), 0, -1 if c < 0 else 1))
    rows = [(m, s) for m, _neg, _tie, s in strongest_hits(cand, half)]
    return np.array(rows, dtype=np.int64).reshape(-1, 2)


def mostly_inverted(rows) -> bool:
    """Whether most of the hits ``rows`` (m, s, ..) are negative: the channel's spectrum is inverted."""
    signs = rows[:, 1]
    return bool(2 * int((signs < 0).sum()) > signs.size)


def layer_stage_keys(prefix: str, x: dict, names, keep: bool) -> dict:
    """A layer's keys of ``ChannelDescriber.stages()`` from ``x``, its ``finish_*`` dict of one channel: ``<prefix>_rows`` (None
    where nothing was decoded) and, with ``keep``, ``<prefix>_plan`` and ``<prefix>_<name>`` for every one of ``names``."""
    d = {f"{prefix}_rows": x.get("rows")}
    if keep and "rows" in x:
        d.update({f"{prefix}_plan": x["plan"]}, **{f"{prefix}_{name}": x[name] for name in names})
    return d


def strongest_hits(cand, half: int) -> list:
    """Of ``cand`` (tuples that begin m, -|C|, tie) those, in order of m, with no other within +-``half`` that has a larger |C|, or
    the same |C| at a smaller m, or the same m at a smaller ``tie`` (the pattern's place in the table): section 25's keep rule
    across the patterns of one protocol."""
    cand = sorted(cand)
    kept = []
    for j, c in enumerate(cand):
        lo = hi = j
        while lo > 0 and c[0] - cand[lo - 1][0] <= half:
            lo -= 1
        while hi + 1 < len(cand) and cand[hi + 1][0] - c[0] <= half:
            hi += 1
        if not any((o[1], o[0], o[2]) < (c[1], c[0], c[2]) for o in cand[lo : hi + 1]):
            kept.append(c)
    return kept


def finish_lanes(lanes, found, rate: int, plan_of, word: str, decode) -> list:
    """The ``finish_*`` of a layer: per lane of the pass (``found``: its dict of ``identify.finish_identify``) the output of
    ``decode(theta, plan, centre, hits, v)`` with ``plan`` (``plan_of`` the lane's rate) and ``note``, or a dict of ``note``
    alone where nothing is decoded: the channel is not of the family ``rate`` ("no ``word`` channel"), its rate does not fit
    or nothing was searched.  It reuses section 25's hits and plane and runs no second search."""
    out = []
    for lane, d in zip(lanes, found):
        if d["rate"] != rate:
            out.append(dict(note=f"no {word} channel"))
            continue
        try:
            plan = plan_of(lane.plan.fs_ch)
        except ValueError:
            plan = None
        if plan is None or d["hits"] is None:
            out.append(dict(note="rate does not fit" if plan is None or d["plan"] is None else "not measured"))
            continue
        st = decode(join_theta(lane.stored), plan, lane.centre, d["hits"], d["v"])
        st.update(plan=plan, note="")
        out.append(st)
    return out


def layer_result(result, channel, channel_of, channels, lanes, decoded, sample_rate: float, center_freq: float | None = None):
    """The ``result`` of the pass (``FlexResult``, ``DmrResult``): ``channels`` the finder's, ``decoded`` the dicts of the layer's
    ``finish_*``; per channel ``channel_of`` its decoded stream, or a ``channel`` of the note alone."""
    chans = []
    for ch, lane, st in zip(channels, lanes, decoded):
        freq = None if center_freq is None else center_freq + ch.offset_hz
        if "rows" not in st:
            chans.append(channel(offset_hz=ch.offset_hz, freq_hz=freq, note=st["note"]))
        else:
            chans.append(channel_of(st, lane.plan.fs_ch, lane.keyed_from, ch.offset_hz, freq))
    return result(channels=chans, sample_rate=sample_rate, center_freq=center_freq)


@dataclass(frozen=True)
class ProtocolLayer:
    """A protocol layer of the second pass, declared once in its module as ``LAYER``; ``ChannelDescriber`` finds it by ``name``,
    the module's name and the keyword of its row in ``find_layers``."""

    name: str
    rates: tuple  # the families whose channels it decodes, whose integrated plane it reads from section 25's dicts (``v``)
    plan_of: Callable  # (fs_ch, rate) -> the layer's plan; ``ValueError`` where ``fs_ch`` does not fit
    word: str  # the note of a channel of another family is "no ``word`` channel"
    decode_stream: Callable  # (theta, plan, centre, hits, pats, v) -> the stages of one stream
    channel_of: Callable  # (stages, fs_ch, keyed_from, offset_hz, freq_hz) -> the channel dataclass
    channel: type
    result: type
    keys: tuple = ()  # the stages that ``stages()`` shows with ``keep_stages``, as ``<name>_<key>`` beside ``<name>_rows`` and ``<name>_plan``
    keys_of: Callable | None = None  # (the lane's dict of ``finish``, keep) -> its keys of ``stages()``, where ``keys`` will not do

    def finish(self, lanes, found) -> list:
        """Per lane of the pass (``found``: its dict of ``identify.finish_identify``) the output of ``decode_stream`` with ``plan`` and
        ``note``, or a dict of ``note`` alone where nothing is decoded: the channel is of none of ``rates``, its rate does not fit
        or nothing was searched.  ``finish_lanes`` once per symbol rate, merged by lane: a lane belongs to one family at the most."""
        from . import identify as I  # (identify imports this module)

        out = None
        for rate in self.rates:
            pats = I.patterns_for(rate)
            got = finish_lanes(lanes, found, rate, lambda fs_ch, rate=rate: self.plan_of(fs_ch, rate), self.word,
                               lambda theta, plan, centre, hits, v, pats=pats: self.decode_stream(theta, plan, centre, hits, pats, v))
            out = got if out is None else [b if d["rate"] == rate else a for a, b, d in zip(out, got, found)]
        return out

    def result_of(self, channels, lanes, decoded, sample_rate: float, center_freq: float | None = None):
        """The ``result`` of the pass: ``channels`` the finder's, ``decoded`` the dicts of ``finish``."""
        return layer_result(self.result, self.channel, self.channel_of, channels, lanes, decoded, sample_rate, center_freq)

    def stage_keys(self, describer, j: int, lane, keep: bool) -> dict:
        """This layer's keys of ``ChannelDescriber.stages()`` for channel ``j``."""
        x = describer.finish_layer(self.name)[j]
        return layer_stage_keys(self.name, x, self.keys, keep) if self.keys_of is None else self.keys_of(x, keep)


# ---- the checks that more than one layer runs (host, integers) --------------------------------------------------------------------


def info_bytes(words) -> list:
    """The bytes of 32-bit information words (the first bit the MSB of word 0)."""
    return [(int(w) >> s) & 0xFF for w in words for s in (24, 16, 8, 0)]


CRC_POLY = 0x1021


def _crc_table() -> tuple:
    table = []
    for byte in range(256):
        crc = byte << 8
        for _ in range(8):
            crc = ((crc << 1) ^ CRC_POLY) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
        table.append(crc)
    return tuple(table)


_CRC = _crc_table()


def crc_ccitt(data) -> int:
    """CRC-CCITT of the bytes ``data``: polynomial 0x1021 from 0, MSB first, not complemented."""
    crc = 0
    for byte in data:
        crc = ((crc << 8) & 0xFFFF) ^ _CRC[(crc >> 8) ^ int(byte)]
    return crc


def gf_tables(poly: int, bits: int) -> tuple:
    """(exp, log, gf_mul) of GF(2^``bits``) modulo ``poly``: alpha^i for i < 2 (2^bits - 1), so that a sum of two logarithms needs
    no reduction, the logarithms, and the product by them."""
    size = (1 << bits) - 1
    exp, log, x = [0] * (2 * size), [0] * (size + 1), 1
    for i in range(size):
        exp[i], log[x] = x, i
        x <<= 1
        if x >> bits:
            x ^= poly
    exp[size:] = exp[:size]
    exp, log = tuple(exp), tuple(log)

    def gf_mul(a: int, b: int) -> int:
        return 0 if a == 0 or b == 0 else exp[log[a] + log[b]]

    return exp, log, gf_mul


class JsonRecord:
    """``to_json`` / ``from_json`` of a result dataclass.  ``NESTED`` names the list fields that hold dataclasses (field ->
    class, itself a ``JsonRecord``); a mixin, not a dataclass: the fields and their order are the class's own."""

    NESTED = {}

    def to_json(self) -> dict:
        return asdict(self)

    @classmethod
    def from_json(cls, data: dict):
        data = dict(data)
        for name, item in cls.NESTED.items():
            data[name] = [item.from_json(x) for x in data.get(name, [])]
        return cls(**data)


class ChannelLabel:
    """``label()`` of a channel dataclass with ``freq_hz`` and ``offset_hz``: its frequency, or its offset where none is known."""

    def label(self) -> str:
        return f"{self.freq_hz:.0f} Hz" if self.freq_hz is not None else f"{self.offset_hz:+.0f} Hz"


class ChannelLines:
    """``lines()`` of a result whose ``channels`` have ``lines()`` of their own: all of them, in channel order."""

    def lines(self) -> list:
        return [line for ch in self.channels for line in ch.lines()]
