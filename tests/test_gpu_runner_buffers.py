"""The resident runners (batch.ResidentCaptureRunner, batch.ResidentBankRunner) held to what their API accepts: every
sample format and iq_order, a capture that is a slice of a larger buffer (``enclosing=``, ``lead_frames=``, the slack of
``padded_capture_frames``) and so does not start on a 16-byte boundary, ``resident=``, and the captured-graph entries --
through the Python glue between the runner and the kernels (halo -> consumed - lead, ``_interior``, ``_edges``,
``warm_block``, the probes, the guard's level read, graph places that carry the lead).  The kernels themselves are pinned at
consumed < 0 and at odd frame offsets by tests/test_gpu_mfma_exact.py.

Two shapes, the smallest that reach both slot forms of the ring kernels once ``_ChannelKernel.mfma_min_outputs`` is 4096:

  A: 2.5 MS/s, D = 26 (row-staged slots), 260 003 frames, chunk 131 072
  B: 10 MS/s, D = 104 (contiguous slots), 1 040 007 frames, chunk 524 288

Both give 10 001 outputs and one full reference chunk plus a ragged second (two chunk starts).  NFM, 12.5 kHz, the tone of
``oracle.cpu_ref.synth_capture_s16`` at 25 kHz.  The reference is ``oracle.cpu_ref.run_chain`` (complex128 filter), run once
per (shape, format): a capture handed to the GPU with another ``iq_order`` is re-ordered / negated so that it ingests to the
SAME complex stream.  A slip of one frame moves z by about 0.04, a thousand times the bars below; the tone's audio alone
would not see it.

Bars, the ones the project already holds per format: int16 z rms < 2e-5 and max < 1e-4 (test_gpu_parity.py, the padded
runner capture), uint8 z rms < 1.4e-5 and max < 1e-4 (both x sqrt(ntaps / 6401) where that exceeds 1: it does not here;
test_mfma_ring_kernel_uint8_captures), float32 |z - want| <= 3e-6 (test_channelizer_formats_orders_streaming); sign and sample
counts exact, peak to 1e-5, PCM16 within one LSB.  What is stated as equal is ``torch.equal``, and only between runs of the
same dispatch.  Measured figures are printed with a ``[runner-buffers]`` prefix.
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np
import pytest
import scan_model as SM

from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu

F_OFF, BW = 25e3, 12_500.0
SHAPES = {"A": dict(fs=2.5e6, d=26, n=260_003, chunk=131_072), "B": dict(fs=10e6, d=104, n=1_040_007, chunk=524_288)}
N_OUT = 10_001
NP_DTYPE = {"s16": np.int16, "u8": np.uint8, "f32": np.float32}
FRAME_BYTES = {"s16": 4, "u8": 2, "f32": 8}
RING = {"s16": "k_channelize_mfma_s16_ring", "u8": "k_channelize_mfma_u8_ring", "f32": "k_channelize_v1"}
ZERO = {"s16": 0, "u8": 128, "f32": 0.0}  # the value of a lead-in: what the filter's zero state ingests to
GUARD_VALUES = 256  # sentinel values on either side of an enclosing buffer (a multiple of 16 bytes in every format)
SENTINEL = {"s16": -21555, "u8": 0xA5, "f32": -7.25}


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()  # fail loudly if the HIP library is missing
    pkg.native.require_gpu()
    return pkg


def rms(a):
    a = np.asarray(a)
    return float(np.sqrt(np.mean(np.abs(a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)) ** 2)))


@contextlib.contextmanager
def short_captures_on_the_matrix_cores():
    from iq_to_audio_amd import processing as PR

    old = PR._ChannelKernel.mfma_min_outputs
    try:
        PR._ChannelKernel.mfma_min_outputs = 4096
        yield
    finally:
        PR._ChannelKernel.mfma_min_outputs = old


# ---- captures and their oracle chains (computed once per module run, never written to) -------------------------------


def _freeze(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


def _as_fmt(s16: np.ndarray, fmt: str) -> np.ndarray:
    """(n, 2) int16 -> the same capture in ``fmt``: uint8 as test_mfma_ring_kernel_uint8_captures makes it, float32 as
    s16 / 32768 plus a dither off the 2^-15 grid (so that nothing can take it for int16 values)."""
    if fmt == "s16":
        return s16
    if fmt == "u8":
        return ((s16.astype(np.int32) >> 8) + 128).astype(np.uint8)
    dither = np.random.default_rng(77).uniform(-2.0 ** -18, 2.0 ** -18, size=s16.shape)
    return (s16.astype(np.float64) / 32768.0 + dither).astype(np.float32)


@functools.lru_cache(maxsize=None)
def base_capture(shape: str, fmt: str, side: int = 1) -> np.ndarray:
    """(n, 2) I/Q in ``fmt``'s type, order 'iq'; ``side`` -1: the carrier at -F_OFF (the probe then says -1)."""
    sh = SHAPES[shape]
    s16 = O.synth_capture_s16(sh["fs"], sh["n"] / sh["fs"], side * F_OFF, seed=42 if side == 1 else 43)
    assert s16.shape == (sh["n"], 2)
    return _freeze(_as_fmt(s16, fmt))


@functools.lru_cache(maxsize=None)
def oracle_chain(shape: str, fmt: str, side: int = 1):
    sh = SHAPES[shape]
    want = O.run_chain(base_capture(shape, fmt, side), sample_rate=sh["fs"], freq_offset=F_OFF, bandwidth=BW, fmt=fmt, iq_order="iq",
                       chunk_size=sh["chunk"], tune_chunk=False)
    # the oracle's own expectations, before anything is compared with it
    assert want.mix_sign == side and want.decimation == sh["d"] and want.chunk == sh["chunk"]
    assert want.decimated.size == want.audio.size == N_OUT == -(-sh["n"] // sh["d"])
    assert len(want.rms_dbfs) == 2  # one full chunk and a ragged one
    assert 0.5 < rms(want.decimated) < 0.8  # the 0.7 tone sits in the channel: this sign, this side
    ref48 = O.float_to_pcm16(O.resample_48k(want.audio, want.fs_channel))
    for a in (want.decimated, want.audio, ref48):
        a.setflags(write=False)
    return want, ref48


def in_order(base: np.ndarray, fmt: str, order: str) -> np.ndarray:
    """The (n, 2) capture that ingests with ``order`` to what ``base`` ingests to with 'iq'."""
    i, q = base[:, 0], base[:, 1]
    if order.endswith("_inv"):
        if fmt == "u8":
            assert q.min() >= 1  # 256 - 0 has no uint8
            q = (256 - q.astype(np.int32)).astype(np.uint8)
        else:
            assert fmt != "s16" or q.min() > -32768
            q = -q
    cap = np.ascontiguousarray(np.column_stack((i, q) if order.startswith("iq") else (q, i)))
    assert cap.dtype == base.dtype
    assert np.array_equal(O.ingest_to_complex64(cap, fmt, order), O.ingest_to_complex64(base, fmt, "iq"))
    return cap


def make_runner(A, shape: str, fmt: str, order: str = "iq", **kw):
    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.batch import ResidentCaptureRunner

    sh = SHAPES[shape]
    d, fs_ch = P.choose_decimation(sh["fs"], 96_000.0)
    assert d == sh["d"]
    taps = A.design_channel_filter(sh["fs"], BW, d)
    return ResidentCaptureRunner(taps, sample_rate=sh["fs"], freq_offset=F_OFF, decimation=d, fs_channel=fs_ch, chunk=sh["chunk"],
                                 n_frames=sh["n"], demod_mode="nfm", fmt=fmt, iq_order=order, **kw), taps


def upload(values: np.ndarray, fmt: str):
    """Flat host values of a capture -> the device tensor a runner takes: interleaved int16 / uint8, complex64 for 'f32'."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(values).reshape(-1).copy()).cuda()
    return torch.view_as_complex(t.reshape(-1, 2)) if fmt == "f32" else t


class Enclosed:
    """``sentinel | zeros(lead) | capture | slack | sentinel`` in one allocation: ``buf`` the enclosing buffer (16-byte
    aligned), ``raw`` the capture's slice of it, ``outer`` everything."""

    def __init__(self, cap: np.ndarray, fmt: str, lead: int, slack: int, fill="12345", seed: int = 5):
        import torch

        n = cap.shape[0]
        g, dt = GUARD_VALUES, NP_DTYPE[fmt]
        host = np.full(2 * g + 2 * (lead + n + slack), SENTINEL[fmt], dtype=dt)
        host[g : g + 2 * lead] = ZERO[fmt]
        host[g + 2 * lead : g + 2 * (lead + n)] = cap.reshape(-1)
        tail = host[g + 2 * (lead + n) : g + 2 * (lead + n + slack)]
        info = np.iinfo(dt) if fmt != "f32" else np.finfo(dt)
        if fill == "12345":
            tail[:] = 12345 if fmt == "s16" else (0x39 if fmt == "u8" else 12345.0)
        elif fill == "random":
            rng = np.random.default_rng(seed)
            tail[:] = rng.integers(info.min, int(info.max) + 1, size=tail.size).astype(dt) if fmt != "f32" else rng.uniform(-1e30, 1e30, tail.size).astype(dt)
        elif fill == "extremes":
            tail[0::2], tail[1::2] = info.min, info.max  # (I at one end of the type's range, Q at the other)
        else:
            raise ValueError(fill)
        self.host, self.fmt, self.lead, self.n, self.slack = host, fmt, lead, n, slack
        self.outer = torch.from_numpy(host.copy()).cuda()
        flat = self.outer[g : self.outer.numel() - g]
        if fmt == "f32":
            self.buf = torch.view_as_complex(flat.reshape(-1, 2))
            self.raw = self.buf[lead : lead + n]
        else:
            self.buf = flat
            self.raw = flat[2 * lead : 2 * (lead + n)]
        # what the case claims about the addresses
        assert self.buf.data_ptr() % 16 == 0
        assert self.raw.data_ptr() - self.buf.data_ptr() == lead * FRAME_BYTES[fmt]
        assert self.raw.data_ptr() % 16 == (lead * FRAME_BYTES[fmt]) % 16
        assert self.raw.numel() == (n if fmt == "f32" else 2 * n)
        torch.cuda.synchronize()

    def submit_args(self):
        return dict(enclosing=self.buf, lead_frames=self.lead)

    def assert_untouched(self):
        """Nothing in the allocation was written: the sentinels in front of and behind the enclosing buffer, and the buffer."""
        import torch

        torch.cuda.synchronize()
        now = self.outer.cpu().numpy()
        g = GUARD_VALUES
        assert np.array_equal(now[:g].view(np.uint8), self.host[:g].view(np.uint8)), "bytes in front of the enclosing buffer"
        assert np.array_equal(now[-g:].view(np.uint8), self.host[-g:].view(np.uint8)), "bytes behind the enclosing buffer"
        assert np.array_equal(now.view(np.uint8), self.host.view(np.uint8)), "the enclosing buffer itself"


def slack_frames(shape: str, taps) -> int:
    from iq_to_audio_amd.batch import ResidentCaptureRunner

    lead, slack = ResidentCaptureRunner.padded_capture_frames(SHAPES[shape]["d"], len(taps))
    assert lead == 0 and slack > 0
    return slack


def snapshot(r) -> tuple:
    """The bits of a collected capture (the runner's buffers are reused): z, audio, PCM16."""
    import torch

    torch.cuda.synchronize()
    return r["z"].clone(), r["audio"].clone(), r["pcm_host"].clone()


def assert_same_bits(a: tuple, b: tuple, what: str) -> None:
    import torch

    for name, x, y in zip(("z", "audio", "pcm16"), a, b):
        x = torch.view_as_real(x) if x.is_complex() else x
        y = torch.view_as_real(y) if y.is_complex() else y
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name)
        bits = {8: torch.int64, 4: torch.int32, 2: torch.int16}[x.element_size()]
        assert torch.equal(x.contiguous().view(bits), y.contiguous().view(bits)), (what, name)


def check_against_oracle(r, runner, shape: str, fmt: str, side: int, tag: str, edges: bool = False) -> None:
    """z at the format's bars, sign, counts, peak, PCM16 <= 1 LSB; ``edges``: the first and last 200 outputs at the bars too."""
    want, ref48 = oracle_chain(shape, fmt, side)
    z = r["z"].cpu().numpy()
    audio = r["audio"].cpu().numpy()
    pcm = r["pcm_host"].numpy()
    assert z.shape == want.decimated.shape and audio.shape == want.audio.shape and pcm.shape == ref48.shape == (runner.n48,)
    err = z - want.decimated
    grow = max(1.0, float(np.sqrt(want.ntaps / 6401.0)))
    lsb = int(np.max(np.abs(pcm.astype(np.int32) - ref48.astype(np.int32))))
    print(f"[runner-buffers] {tag}: {r['kernel']} sign {r['sign']:+d} z rms {rms(err):.3e} max {np.abs(err).max():.3e} "
          f"first200 {np.abs(err[:200]).max():.3e} last200 {np.abs(err[-200:]).max():.3e} audio rms {rms(audio - want.audio):.3e} "
          f"peak diff {abs(r['demod'].peak - want.audio_peak):.2e} pcm16 {lsb} LSB")
    assert r["sign"] == want.mix_sign == side
    assert r["kernel"] == RING[fmt], r["kernel"]
    parts = [("all", err)] + ([("first 200", err[:200]), ("last 200", err[-200:])] if edges else [])
    for name, e in parts:
        if fmt == "s16":
            assert rms(e) < 2e-5 and np.abs(e).max() < 1e-4, (tag, name, rms(e), np.abs(e).max())
        elif fmt == "u8":
            assert rms(e) < 1.4e-5 * grow and np.abs(e).max() < 1e-4 * grow, (tag, name, rms(e), np.abs(e).max())
        else:
            assert np.abs(e).max() <= 3e-6, (tag, name, np.abs(e).max())
    assert abs(r["demod"].peak - want.audio_peak) < 1e-5
    assert len(r["demod"].chunk_rms_dbfs()) == len(want.rms_dbfs)
    assert lsb <= 1, (tag, lsb)


# ---- formats and orders, a plain aligned tensor ---------------------------------------------------------------------

PLAIN = ([("A", "s16", o, 1) for o in O.IQ_ORDERS] + [("B", "s16", "iq", 1)]
         + [(s, "u8", o, 1) for s in ("A", "B") for o in ("iq", "qi_inv")]
         + [("A", "f32", o, 1) for o in ("iq", "qi")]
         + [("A", "s16", "iq", -1)])


@pytest.mark.parametrize("shape,fmt,order,side", PLAIN, ids=[f"{s}-{f}-{o}{'' if sd == 1 else '-neg'}" for s, f, o, sd in PLAIN])
def test_formats_and_orders_through_submit(A, shape, fmt, order, side):
    """Every format the runner takes, the orders named for it, both slot forms, and a capture whose carrier sits at -F_OFF
    (speculated +1, probed -1, run again): one ``submit`` of a fresh aligned tensor against the oracle chain."""
    import torch

    want, _ = oracle_chain(shape, fmt, side)
    assert want.mix_sign == side and want.decimated.size == N_OUT
    cap = in_order(base_capture(shape, fmt, side), fmt, order)
    with short_captures_on_the_matrix_cores():
        runner, _ = make_runner(A, shape, fmt, order)
        assert (runner.n_dec, len(runner.starts)) == (N_OUT, 2)
        x = upload(cap, fmt)
        assert x.data_ptr() % 256 == 0
        torch.cuda.synchronize()
        r = runner.collect(runner.submit(x))
        check_against_oracle(r, runner, shape, fmt, side, f"plain {shape} {fmt} {order} side {side:+d}")
        assert runner.redone == dict(sign=int(side == -1), precision=0)


# ---- lead-in and alignment ---------------------------------------------------------------------------------------------

LEADS = [("A", "s16", ld) for ld in (1, 3, 4, 7)] + [("A", "u8", ld) for ld in (1, 3, 5, 8)] + [("A", "f32", 1)] + [("B", "s16", 3), ("B", "u8", 5)]


@pytest.mark.parametrize("resident", [False, True], ids=["queued", "resident"])
@pytest.mark.parametrize("guard", [None, 0.0], ids=["guard-on", "guard-off"])
@pytest.mark.parametrize("shape,fmt,lead", LEADS, ids=[f"{s}-{f}-lead{ld}" for s, f, ld in LEADS])
def test_capture_behind_a_lead_in(A, shape, fmt, lead, guard, resident):
    """The same capture inside ``zeros(lead) | capture | slack``: its first byte 4, 12, 0, 12 (int16), 2, 6, 10, 0 (uint8) or 8
    (float32) bytes off a 16-byte boundary.  With the guard on the probe reads the warm-up block's level from that address
    (``mixsign.queue_raw_level``; ``iqa_raw_level`` itself refuses it).  The same bars as for the plain tensor, the first
    and last 200 outputs too: with a halo the last ones come from the matrix cores."""
    with short_captures_on_the_matrix_cores():
        runner, taps = make_runner(A, shape, fmt, precision_guard=guard)
        enc = Enclosed(base_capture(shape, fmt), fmt, lead, slack_frames(shape, taps))
        assert enc.raw.data_ptr() % 16 == {"s16": 4 * lead % 16, "u8": 2 * lead % 16, "f32": 8 * lead % 16}[fmt]
        r = runner.collect(runner.submit(enc.raw, resident=resident, **enc.submit_args()))
        check_against_oracle(r, runner, shape, fmt, 1, f"lead {shape} {fmt} lead {lead} guard {'on' if guard is None else 'off'} "
                             f"{'resident' if resident else 'queued'}", edges=fmt != "f32")
        assert runner.redone == dict(sign=0, precision=0)
        enc.assert_untouched()


# ---- exact invariances -----------------------------------------------------------------------------------------------------

EXACT = [("A", "s16", 3), ("A", "u8", 5), ("A", "f32", 1), ("B", "s16", 1)]


@pytest.mark.parametrize("shape,fmt,lead", EXACT, ids=[f"{s}-{f}-lead{ld}" for s, f, ld in EXACT])
def test_slack_residency_and_repetition_change_no_bit(A, shape, fmt, lead):
    """One ticket geometry (same lead, same slack length -- the same dispatch): whatever the slack holds, a second run,
    ``resident=True`` and buffers that sit elsewhere give the same z, audio and PCM16 bits; no byte of the allocation is
    written.  (Lead 0 against lead L chooses another interior: that pair is held to the oracle bars above, not to equality.)"""
    with short_captures_on_the_matrix_cores():
        runner, taps = make_runner(A, shape, fmt)
        slack = slack_frames(shape, taps)
        cap = base_capture(shape, fmt)
        encs = {fill: Enclosed(cap, fmt, lead, slack, fill) for fill in ("12345", "random", "extremes")}
        first = snapshot(runner.collect(runner.submit(encs["12345"].raw, **encs["12345"].submit_args())))
        again = snapshot(runner.collect(runner.submit(encs["12345"].raw, **encs["12345"].submit_args())))
        assert_same_bits(first, again, "second run")
        for fill in ("random", "extremes"):
            got = snapshot(runner.collect(runner.submit(encs[fill].raw, **encs[fill].submit_args())))
            assert_same_bits(first, got, f"slack {fill}")
        res = runner.collect(runner.submit(encs["extremes"].raw, resident=True, **encs["extremes"].submit_args()))
        check_against_oracle(res, runner, shape, fmt, 1, f"exact {shape} {fmt} lead {lead} resident, slack at the extremes", edges=fmt != "f32")
        assert_same_bits(first, snapshot(res), "resident=True")
        for enc in encs.values():
            enc.assert_untouched()


GRAPH = [("A", "s16", 3), ("A", "u8", 5), ("B", "s16", 1)]


@pytest.mark.parametrize("shape,fmt,lead", GRAPH, ids=[f"{s}-{f}-lead{ld}" for s, f, ld in GRAPH])
def test_captured_entries_equal_submit_behind_a_lead_in(A, shape, fmt, lead):
    """``submit_captured(raw, enclosing=buf, lead_frames=lead)`` replayed three times, and ``submit_captured_batch`` of two
    such buffers (the same capture, other slack), equal ``submit`` of the same arguments bit for bit; nothing is captured
    twice and no replay is redone."""
    with short_captures_on_the_matrix_cores():
        runner, taps = make_runner(A, shape, fmt)
        slack = slack_frames(shape, taps)
        cap = base_capture(shape, fmt)
        one, two = Enclosed(cap, fmt, lead, slack, "12345"), Enclosed(cap, fmt, lead, slack, "random", seed=9)
        want = snapshot(runner.collect(runner.submit(one.raw, **one.submit_args())))
        for rep in range(3):
            r = runner.collect(runner.submit_captured(one.raw, **one.submit_args()))
            assert r["sign"] == 1 and r["kernel"] == RING[fmt]
            assert_same_bits(want, snapshot(r), f"replay {rep}")
        assert runner.graph_captures == 3 and runner.replays_redone == 0  # (one fixed buffer over three slots)
        for rep in range(2):
            tickets = runner.submit_captured_batch([(e.raw, e.buf, e.lead) for e in (one, two)])
            for k, t in enumerate(tickets):
                r = runner.collect(t)
                assert r["sign"] == 1
                assert_same_bits(want, snapshot(r), f"batch round {rep} capture {k}")
        assert runner.graph_captures == 4 and runner.replays_redone == 0 and runner.redone == dict(sign=0, precision=0)
        check_against_oracle(r, runner, shape, fmt, 1, f"graph {shape} {fmt} lead {lead} batch replay", edges=True)
        one.assert_untouched()
        two.assert_untouched()


# ---- ResidentBankRunner ------------------------------------------------------------------------------------------------

BANK_OFFSETS = (25e3, -150e3)


@functools.lru_cache(maxsize=None)
def bank_capture(fmt: str) -> np.ndarray:
    from iq_to_audio_amd.benchmark import synthetic_multi_iq_s16

    sh = SHAPES["A"]
    s16 = synthetic_multi_iq_s16(sh["fs"], sh["n"] / sh["fs"], [(off, 0.3, "nfm") for off in BANK_OFFSETS], seed=42)
    assert s16.shape == (sh["n"], 2)
    return _freeze(_as_fmt(s16, fmt))


@functools.lru_cache(maxsize=None)
def bank_oracle(fmt: str, offset: float):
    """The bank runner tunes its chunk as the pipeline does (131 072 -> 1 048 576 at 2.5 MS/s: the capture is one chunk)."""
    sh = SHAPES["A"]
    want = O.run_chain(bank_capture(fmt), sample_rate=sh["fs"], freq_offset=offset, bandwidth=BW, fmt=fmt, chunk_size=sh["chunk"], tune_chunk=True)
    assert want.mix_sign == 1 and want.decimation == sh["d"] and want.decimated.size == N_OUT and len(want.rms_dbfs) == 1
    assert 0.2 < rms(want.decimated) < 0.4  # each target holds its own 0.3 carrier
    ref48 = O.float_to_pcm16(O.resample_48k(want.audio, want.fs_channel))
    for a in (want.decimated, want.audio, ref48):
        a.setflags(write=False)
    return want, ref48


@pytest.mark.parametrize("fmt", ["s16", "u8"])
def test_bank_runner_behind_a_lead_in(A, fmt):
    """Two NFM targets, one on each side of DC, out of one capture at lead 3 (12 / 6 bytes off the boundary): inside a buffer
    that ends with the capture ("plain") and inside a padded one, each target against its own oracle chain at the bars above;
    the padded buffer's slack changes no bit."""
    from iq_to_audio_amd.batch import ResidentBankRunner

    sh, lead = SHAPES["A"], 3
    with short_captures_on_the_matrix_cores():
        bank = ResidentBankRunner([dict(freq_offset=off, bandwidth=BW) for off in BANK_OFFSETS], sample_rate=sh["fs"], n_frames=sh["n"],
                                  chunk_size=sh["chunk"], fmt=fmt)
        assert bank.d == sh["d"] and bank.n_dec == N_OUT
        slack = slack_frames("A", bank.targets[0]["taps"])
        cap = bank_capture(fmt)
        encs = dict(plain=Enclosed(cap, fmt, lead, 0), padded=Enclosed(cap, fmt, lead, slack, "12345"), other=Enclosed(cap, fmt, lead, slack, "extremes"))
        bits = {}
        for name, enc in encs.items():
            res = bank.collect(bank.submit(enc.raw, **enc.submit_args()))
            assert len(res) == 2
            bits[name] = [snapshot(r) for r in res]
            for off, r in zip(BANK_OFFSETS, res):
                want, ref48 = bank_oracle(fmt, off)
                z, audio, pcm = r["z"].cpu().numpy(), r["audio"].cpu().numpy(), r["pcm_host"].numpy()
                err = z - want.decimated
                lsb = int(np.max(np.abs(pcm.astype(np.int32) - ref48.astype(np.int32))))
                print(f"[runner-buffers] bank {fmt} lead {lead} {name} target {off:+.0f} Hz: sign {r['sign']:+d} z rms {rms(err):.3e} "
                      f"max {np.abs(err).max():.3e} last200 {np.abs(err[-200:]).max():.3e} audio rms {rms(audio - want.audio):.3e} pcm16 {lsb} LSB")
                assert z.shape == want.decimated.shape and pcm.shape == ref48.shape
                assert r["sign"] == want.mix_sign
                for e in (err, err[:200], err[-200:]):
                    if fmt == "s16":
                        assert rms(e) < 2e-5 and np.abs(e).max() < 1e-4, (name, off, rms(e), np.abs(e).max())
                    else:
                        assert rms(e) < 1.4e-5 and np.abs(e).max() < 1e-4, (name, off, rms(e), np.abs(e).max())
                assert abs(r["demod"].peak - want.audio_peak) < 1e-5
                assert lsb <= 1
            enc.assert_untouched()
        assert bank.redone == dict(sign=0, precision=0)
        for a, b in zip(bits["padded"], bits["other"]):
            assert_same_bits(a, b, "bank slack")


# ---- the precision guard on an unaligned capture ---------------------------------------------------------------------------


def test_guard_reads_the_level_of_an_unaligned_capture(A):
    """The weak channel beside a strong tone of test_precision_guard_in_the_batch_runners (shape B's length) at lead 1: the
    precision picked and the ``redone`` counters equal the lead 0 run's, and the level the probe reports is the documented
    eight-stretch mean square (tests/scan_model.py: raw_level_want, to 1e-12 as in test_gpu_scan_exact.py) of the warm-up
    block's values from its first 16-byte boundary on."""
    from test_gpu_configs import dynamic_range_capture

    from iq_to_audio_amd import dsp_plan as P
    from iq_to_audio_amd.batch import ResidentCaptureRunner
    from iq_to_audio_amd.mixsign import wideband_rms_from

    sh = SHAPES["B"]
    fs, n, chunk, d = sh["fs"], sh["n"], sh["chunk"], sh["d"]
    cap = dynamic_range_capture(n, fs)
    taps = A.design_channel_filter(fs, BW, d)
    slack = slack_frames("B", taps)
    seen = {}
    with short_captures_on_the_matrix_cores():
        for lead in (0, 1):
            runner = ResidentCaptureRunner(taps, sample_rate=fs, freq_offset=1.0e6, decimation=d, fs_channel=P.choose_decimation(fs, 96_000.0)[1],
                                           chunk=chunk, n_frames=n)
            enc = Enclosed(cap, "s16", lead, slack)
            assert enc.raw.data_ptr() % 16 == 4 * lead
            picked, levels = [], []
            for k in range(2):
                ticket = runner.submit(enc.raw, resident=bool(k), **enc.submit_args())
                r = runner.collect(ticket)
                picked.append((r["precision"], r["sign"]))
                levels.append(ticket["probe"].wideband_rms)
            warm = cap.reshape(-1)[: 2 * min(chunk, n)]
            skip = (-4 * lead % 16) // 2  # values in front of the slice's first 16-byte boundary
            want_rms = wideband_rms_from(SM.raw_level_want("s16", warm[skip:]), "s16")
            print(f"[runner-buffers] guard lead {lead}: picked {picked} redone {runner.redone} level {levels[0]!r} want {want_rms!r}")
            assert want_rms > 0.5  # the 0.95 tone
            for got in levels:
                assert abs(got ** 2 - want_rms ** 2) <= 1e-12 * want_rms ** 2, (lead, got, want_rms)
            seen[lead] = (picked, dict(runner.redone))
            enc.assert_untouched()
    assert seen[0] == ([("fine", 1), ("fine", 1)], dict(sign=0, precision=1))  # the first capture re-run at "fine", the second speculated there
    assert seen[1] == seen[0]
