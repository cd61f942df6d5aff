"""N pipelines from N host threads, and the C ABI from N threads on distinct streams and buffers (INTEGRATION.md,
"Threading contract"; the host-side bookkeeping is tested without a GPU in ``test_threads_host.py``).

Every comparison is BIT FOR BIT against the same work done serially in the same process: the kernels' arithmetic is pinned
elsewhere, what is asserted here is that threads change nothing.  The one exception is the per-chunk RMS, which comes
from float atomics whose order varies even between two serial runs: it is held to the bound ``test_gpu_scan_exact.py``
uses for the segment sums, 2^-21 relative (of the mean square: 10 log10(1 + 2^-21) dB).

Workers are daemon threads joined with a time limit; a worker's exception or a join that times out fails the test and
makes every later test of this module fail at once, without touching the GPU.  Nothing is retried.
"""
from __future__ import annotations

import math
import os
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

JOIN = 60.0  # seconds a group of workers is given (a passing test needs a few)
RMS_DB = 10.0 * math.log10(1.0 + 2.0 ** -21)
_BROKEN: list = []  # why a test of this module left a worker behind or saw one fail: later tests do not run


@pytest.fixture(scope="module")
def A():
    import iq_to_audio_amd as pkg

    pkg.native.lib()
    pkg.native.require_gpu()
    return pkg


@pytest.fixture(autouse=True)
def _module_still_sound():
    if _BROKEN:
        pytest.fail(f"an earlier test of this module failed in a worker thread ({_BROKEN[0]}): not touching the GPU again")


def run_threads(fns, timeout: float = JOIN, meanwhile=None) -> list:
    """``fns`` in one daemon thread each, released together; their results in order.  ``meanwhile`` runs in the calling
    thread once they have been started."""
    out, errs = [None] * len(fns), []
    gate = threading.Barrier(len(fns))

    def body(i):
        try:
            gate.wait(timeout)
            out[i] = fns[i]()
        except BaseException as exc:  # noqa: BLE001
            errs.append((i, exc))
            gate.abort()

    threads = [threading.Thread(target=body, args=(i,), name=f"worker{i}", daemon=True) for i in range(len(fns))]
    for t in threads:
        t.start()
    try:
        if meanwhile is not None:
            meanwhile()
    finally:
        for t in threads:
            t.join(timeout)
    stuck = [t.name for t in threads if t.is_alive()]
    if stuck:
        _BROKEN.append(f"{stuck} did not finish within {timeout:.0f} s")
        pytest.fail(_BROKEN[-1])
    if errs:
        _BROKEN.append(f"worker{errs[0][0]}: {errs[0][1]!r}")
        raise errs[0][1]
    return out


# ---- package level -------------------------------------------------------------------------------------------------------

FC = 400e6


def _signal(fs: float, secs: float, f_off: float, kind: str, seed: int) -> np.ndarray:
    """Complex baseband, |x| < 0.6: a carrier at ``f_off`` with NFM (1 kHz + 2.3 kHz), AM (700 Hz) or an upper side band
    of two tones, and noise 40 dB below it."""
    n = int(round(fs * secs))
    t = np.arange(n, dtype=np.float64) / fs
    rng = np.random.default_rng(seed)
    if kind == "nfm":
        msg = np.sin(2 * np.pi * 1000.0 * t) + 0.5 * np.sin(2 * np.pi * 2300.0 * t)
        x = 0.5 * np.exp(1j * (2 * np.pi * f_off * t + 3000.0 / fs * 2 * np.pi * np.cumsum(msg)))
    elif kind == "am":
        x = 0.3 * (1.0 + 0.8 * np.sin(2 * np.pi * 700.0 * t)) * np.exp(2j * np.pi * f_off * t)
    else:
        x = 0.25 * np.exp(2j * np.pi * (f_off + 900.0) * t) + 0.2 * np.exp(2j * np.pi * (f_off + 1700.0) * t)
    return x + 0.005 * (rng.normal(size=n) + 1j * rng.normal(size=n))


def _frames(x: np.ndarray, fmt: str) -> np.ndarray:
    iq = np.column_stack((x.real, x.imag))
    if fmt == "s16":
        return np.rint(iq * 32767.0).astype(np.int16).reshape(-1)
    if fmt == "u8":
        return (np.rint(iq * 127.0) + 128.0).astype(np.uint8).reshape(-1)
    return iq.astype(np.float32).reshape(-1)  # fractional values: the two-plane path


class Spec:
    """One pipeline configuration and its capture file; ``run(tag)`` makes a fresh pipeline writing ``<tag>.wav``."""

    SUFFIX = {"s16": ".cs16", "u8": ".cu8", "f32": ".cf32"}

    def __init__(self, A, tmp: Path, name: str, *, fmt, fs, f_off, mode, secs, agc=True, seed=1, side=None, frames=None,
                 chunk_size=1_048_576, fc=FC):
        self.A, self.tmp, self.name, self.mode, self.agc, self.fs, self.fc, self.f_off = A, tmp, name, mode, agc, fs, fc, f_off
        self.side, self.chunk_size = dict(side or {}), chunk_size
        self.path = tmp / f"{name}_{int(fc)}Hz{self.SUFFIX[fmt]}"
        if frames is None:
            frames = _frames(_signal(fs, secs, f_off, "usb" if mode == "usb" else mode, seed), fmt)
        self.path.write_bytes(np.ascontiguousarray(frames).tobytes())

    def config(self, tag: str, f_off=None):
        f = self.f_off if f_off is None else f_off
        return self.A.ProcessingConfig(in_path=self.path, target_freq=self.fc + f, demod_mode=self.mode, agc_enabled=self.agc,
                                       input_sample_rate=self.fs, chunk_size=self.chunk_size, output_path=self.tmp / f"{tag}.wav")

    def pipeline(self, tag: str):
        pipe = self.A.ProcessingPipeline(self.config(tag), **self.side)
        pipe.block_frames_target = 1_048_576  # (a): two device blocks through _BlockStager
        return pipe

    def run(self, tag: str) -> dict:
        pipe = self.pipeline(tag)
        res = pipe.run()
        return outcome(pipe, res, self.tmp / f"{tag}.wav")


def outcome(pipe, res, wav: Path) -> dict:
    side = {name: (None if getattr(pipe, name) is None else getattr(pipe, name).to_json()) for name in ("tones", "pocsag")}
    multi = getattr(pipe, "_multi", None)  # (float32 captures: blocks that ran as one / as two int16 planes)
    return dict(wav=wav.read_bytes(), result=res, rms=list(pipe.chunk_rms_dbfs), precision=pipe.channelizer_precision, side=side,
                planes=None if multi is None else (multi.integer_blocks, multi.split_blocks))


def same(got: dict, want: dict, what: str) -> None:
    assert len(got["wav"]) == len(want["wav"]) > 44, what  # the 48 kHz sample count
    assert got["wav"] == want["wav"], f"{what}: the WAV differs from the serial run's"
    assert got["result"] == want["result"], (what, got["result"], want["result"])  # counts, sign, peak: exactly
    # (not ``channelizer_kernel``: a diagnostic read from the cached kernel object, which pipelines of one configuration
    # share -- it names whichever thread's launch came last)
    assert (got["precision"], got["planes"]) == (want["precision"], want["planes"]), what
    assert len(got["rms"]) == len(want["rms"]) > 0, what
    worst = max(abs(a - b) for a, b in zip(got["rms"], want["rms"]))
    print(f"{what}: per-chunk rms differs by at most {worst:.3e} dB (bound {RMS_DB:.3e})")
    assert worst <= RMS_DB, (what, worst)
    assert got["side"] == want["side"], what


@pytest.fixture(scope="module")
def specs(A, tmp_path_factory):
    """(a), (b), (c), a second capture for (a), and each one's serial outcome -- computed once, shared read-only."""
    tmp = tmp_path_factory.mktemp("threads")
    s = {
        "a": Spec(A, tmp, "a", fmt="s16", fs=2.5e6, f_off=25e3, mode="nfm", secs=0.6, seed=1),
        "b": Spec(A, tmp, "b", fmt="u8", fs=2.4e6, f_off=-300e3, mode="am", secs=0.6, seed=2),
        "c": Spec(A, tmp, "c", fmt="f32", fs=2.5e6, f_off=25e3, mode="usb", secs=0.4, seed=3),
        "a2": Spec(A, tmp, "a2", fmt="s16", fs=2.5e6, f_off=25e3, mode="nfm", secs=0.6, seed=4),
    }
    serial = {k: v.run(f"serial_{k}") for k, v in s.items()}
    print({k: (v["precision"], v["planes"], len(v["wav"])) for k, v in serial.items()})
    assert serial["c"]["precision"] == "full" and serial["c"]["planes"] == (0, 1)  # SSB with AGC; fractions: two int16 planes
    assert serial["a"]["wav"] != serial["a2"]["wav"]
    return s, serial


def test_three_pipelines_three_threads_three_configurations(specs):
    s, serial = specs
    for rnd in range(4):
        got = run_threads([lambda k=k, rnd=rnd: s[k].run(f"r{rnd}_{k}") for k in "abc"])
        for k, g in zip("abc", got):
            same(g, serial[k], f"round {rnd} ({k})")


def test_two_threads_same_configuration_different_files(specs):
    """Both share the cached ``_ChannelKernel`` and the resampler table."""
    s, serial = specs
    for rnd in range(2):
        got = run_threads([lambda k=k, rnd=rnd: s[k].run(f"same{rnd}_{k}") for k in ("a", "a2")])
        for k, g in zip(("a", "a2"), got):
            same(g, serial[k], f"same configuration, round {rnd} ({k})")


def test_multi_channel_pipeline_beside_a_single_one(A, specs):
    s, serial = specs
    offs = (25e3, -200e3, 400e3)

    def multi(tag):
        cfgs = [s["a"].config(f"{tag}{i}", off) for i, off in enumerate(offs)]
        m = A.MultiChannelPipeline(cfgs)
        for o in m.owners:
            o.block_frames_target = 1_048_576
        res = m.run()
        return [outcome(o, r, c.output_path) for o, r, c in zip(m.owners, res, cfgs)]

    want = multi("mserial")
    got_multi, got_b = run_threads([lambda: multi("mthread"), lambda: s["b"].run("beside_multi_b")])
    for i, (g, w) in enumerate(zip(got_multi, want)):
        same(g, w, f"multi-channel target {i}")
    same(got_b, serial["b"], "(b) beside the multi-channel run")


def test_side_decoders_in_threads(A, tmp_path):
    """``tones=True`` beside ``pocsag=True``, on the captures of ``test_gpu_tones.py`` / ``test_gpu_pocsag.py``."""
    import test_gpu_pocsag as TP
    import test_gpu_tones as TT

    fs = 2.4e6
    tones = Spec(A, tmp_path, "voice", fmt="s16", fs=fs, f_off=300e3, mode="nfm", secs=0, side=dict(tones=True), chunk_size=65_536,
                 frames=TT._capture(fs, 2.6).reshape(-1), fc=455.5e6)
    pager = Spec(A, tmp_path, "pager", fmt="s16", fs=fs, f_off=300e3, mode="nfm", secs=0, side=dict(pocsag=True), chunk_size=65_536,
                 frames=TP._capture(fs, 2.2).reshape(-1), fc=150e6)
    want = [tones.run("serial_tones"), pager.run("serial_pager")]
    assert [e["tone_hz"] for e in want[0]["side"]["tones"]["ctcss"]] == [TT.TONE] and want[0]["side"]["pocsag"] is None
    assert len(want[1]["side"]["pocsag"]["messages"]) == 2 and want[1]["side"]["tones"] is None
    got = run_threads([lambda: tones.run("thread_tones"), lambda: pager.run("thread_pager")])
    same(got[0], want[0], "tones beside pocsag")
    same(got[1], want[1], "pocsag beside tones")


def test_cancel_from_the_main_thread_while_another_pipeline_runs(A, specs):
    """The cancelled pipeline is held in its first block's status callback until the main thread has called ``cancel()``:
    it raises ``ProcessingCancelled`` at its next check and leaves no output; the other one's WAV is its serial run's."""
    from iq_to_audio_amd.progress import NullProgressSink

    s, serial = specs
    pipe = s["a"].pipeline("cancelled")
    out = s["a"].tmp / "cancelled.wav"
    out.write_bytes(b"stale")
    running, cancelled = threading.Event(), threading.Event()

    class Sink(NullProgressSink):
        def status(self, message):
            if message.startswith("channel") and not running.is_set():
                running.set()
                assert cancelled.wait(JOIN)

    def victim():
        with pytest.raises(A.ProcessingCancelled):
            pipe.run(Sink())
        return "cancelled"

    def other():
        return s["b"].run("beside_cancel_b")

    def cancel_it():  # in the main thread, while both run
        try:
            assert running.wait(JOIN)
            pipe.cancel()
        finally:
            cancelled.set()

    got = run_threads([victim, other], meanwhile=cancel_it)
    assert got[0] == "cancelled" and not out.exists()
    same(got[1], serial["b"], "(b) beside a cancelled run")


# ---- library level -------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def W():
    import threads_work

    return threads_work


@pytest.mark.parametrize("ks", [13, 9])
def test_two_pair_launches_in_flight(A, W, ks):
    """Two lane-pair launches with pacing on, in flight at once: (1) queued on two streams from one thread, (2) from two
    threads on a stream each, released together round by round.  Every lane of both launches equals the exact integer
    model.  Each launch takes ``slice_words`` of the RG_PACE_WORDS pacing words, round-robin: the 16 launches of each part
    wrap the offset once or more, whatever it was.  (Pacing gives up after RG_PACE_SPINS: a shared slice would show as
    wrong traffic, not as a hang; the outputs are exact either way.)"""
    import test_gpu_mfma_exact as E
    import torch
    from oracle import mfma_dispatch as X

    job = W.PairJob(ks)
    E._check_abi_selects(A, "pairs", "s16", job.d, 0, ks, False, X.expected_kernel("pairs", "s16", job.d, 0, ks, False, False))
    rounds = 8
    assert rounds * 2 * job.slice_words > W.RG_PACE_WORDS, job.slice_words
    torch.cuda.synchronize()  # the capture and the tap fragments are in place
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for rnd in range(rounds):
        tables = [job.lanes(), job.lanes()]
        for st, lanes in zip(streams, tables):
            with torch.cuda.stream(st):
                job.launch(lanes)
        for st in streams:
            st.synchronize()
        for i, lanes in enumerate(tables):
            job.check(lanes, f"ks {ks}, two streams, round {rnd}, launch {i}")

    step = threading.Barrier(2)

    def worker(who):
        done = []
        with torch.cuda.stream(streams[who]):
            for _ in range(rounds):
                lanes = job.lanes()
                step.wait(JOIN)
                job.launch(lanes)
                streams[who].synchronize()
                done.append(lanes)
        return done

    try:
        got = run_threads([lambda: worker(0), lambda: worker(1)])
    finally:
        step.abort()
    for who, tables in enumerate(got):
        for rnd, lanes in enumerate(tables):
            job.check(lanes, f"ks {ks}, two threads, round {rnd}, thread {who}")


def test_psd_frames_from_two_threads(A):
    """``iqa_psd_frames`` at nfft 4096 (radix) in one thread and 3000 (Bluestein) in the other, five frame counts each, twice
    over and in lock step: ten (nfft, batch) plans compete for the eight places of the plan LRU, so plans are made, hit
    and evicted while the other thread launches.  Every result is bit-identical to the single-threaded call."""
    import test_gpu_spectrum_shapes as SP
    import torch

    rng = np.random.default_rng(5)
    counts = (1, 2, 3, 4, 5)
    raw = {nfft: np.rint(rng.normal(scale=3000.0, size=2 * (nfft + 6 * 512))).astype(np.int16) for nfft in (4096, 3000)}
    window = {nfft: np.hanning(nfft) for nfft in raw}

    def call(nfft, n_frames):
        out = SP.psd_frames(raw[nfft], "s16", "iq", 0, 512, n_frames, nfft, nfft, window[nfft], 1.0 / nfft, want32=False)
        return out["f64"].view(np.uint64).copy()

    want = {(nfft, k): call(nfft, k) for nfft in raw for k in counts}
    assert all(np.isfinite(w.view(np.float64)).all() for w in want.values())
    step = threading.Barrier(2)

    def worker(nfft):
        got = []
        with torch.cuda.stream(torch.cuda.Stream()):
            for _ in range(2):
                for k in counts:
                    step.wait(JOIN)
                    got.append(((nfft, k), call(nfft, k)))
        return got

    try:
        results = run_threads([lambda: worker(4096), lambda: worker(3000)])
    finally:
        step.abort()
    for got in results:
        assert len(got) == 10
        for key, g in got:
            np.testing.assert_array_equal(g, want[key], err_msg=f"nfft {key[0]}, {key[1]} frames")


def test_first_use_from_two_threads_in_a_fresh_process(A, W):
    """The serial run here is checked against the models and digested; ``threads_first_use_child.py`` makes the same
    launches as a fresh process's first ones, from two threads at once, and prints its digest."""
    import torch

    outs = []
    for who in range(2):
        jobs = W.first_use_jobs(who)
        pair = W.PairJob(13)
        lanes = pair.lanes()
        for job in jobs:
            job.launch()
        pair.launch(lanes)
        torch.cuda.synchronize()
        for job in jobs:
            job.check()
        pair.check(lanes, "serial pairs")
        outs += [a for job in jobs for a in job.outputs()] + [ln.out.cpu().numpy() for ln in lanes]
    want = W.digest(outs)
    child = subprocess.run([sys.executable, str(ROOT / "tests" / "threads_first_use_child.py")], capture_output=True, text=True,
                           timeout=240, env=dict(os.environ), cwd=str(ROOT))
    assert child.returncode == 0, (child.stdout[-2000:], child.stderr[-2000:])
    lines = [ln.split() for ln in child.stdout.splitlines() if ln.startswith("digest ")]
    assert lines == [["digest", want]], (child.stdout[-2000:], want)
