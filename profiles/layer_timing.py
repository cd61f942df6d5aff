"""What the timing scripts of the protocol layers share (flex_timing.py, dmr_timing.py, p25_timing.py, ysf_timing.py,
nxdn_timing.py): the device-resident capture of profiles/find_timing.py (60 s at 10 MS/s int16) with the layer's channel
written into it on the device (``add_channel``), the finder once, then the finder's channels through ``ChannelDescriber`` in the
blocks ``find_channels`` uses, with ``identify`` alone (the yardstick) and with the layer beside it, alternating in one process.
By device events behind one warm-up each: the whole second pass with its results (median of REPEATS), then the layer's entry
points on their own, on its lane's plane (``entry_ms``: median of REPEATS each).  ``run`` prints the one JSON line; a script
keeps its model and symbol table, its centre frequency, its summary of a channel and its entry points."""
from __future__ import annotations

import importlib.util
import json
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from iq_to_audio_amd import describe as DS  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd import find as FD  # noqa: E402


def load(name, folder):
    spec = importlib.util.spec_from_file_location(name, ROOT / folder / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


FT = load("find_timing", "profiles")
REPEATS = FT.REPEATS
OFFSET, AMP = -3.6e6, 0.01  # the added channel's place and amplitude (at 0.05 the sidelobes of rectangular symbols read as a wide FM channel)


def add_channel(capture, table, steps: int, dev: float) -> None:
    """Adds an FSK channel to the device capture in place, a second at a time: the level ``table`` in a loop at ``steps`` entries
    a second, a level of 1 ``dev`` Hz off the carrier, the phase carried from second to second."""
    levels = torch.tensor(table, dtype=torch.float64, device="cuda")
    fs, n = FT.FS, int(capture.numel()) // 2
    phase = 0.0
    for a in range(0, n, int(fs)):
        b = min(n, a + int(fs))
        k = torch.arange(a, b, dtype=torch.int64, device="cuda")
        step = torch.div(k * steps, int(fs), rounding_mode="floor") % len(table)
        turns = torch.cumsum(levels[step] * (dev / fs), 0) + phase
        phase = float(turns[-1]) % 1.0
        angle = 2.0 * math.pi * ((turns + (k.to(torch.float64) * (OFFSET / fs))) % 1.0)
        z = torch.stack([torch.cos(angle), torch.sin(angle)], dim=1) * (AMP * 32768.0)
        capture[2 * a : 2 * b] += torch.round(z).to(torch.int16).reshape(-1)


def second_pass(capture, plan, fin, channels, fc: float, layer: str, on: bool):
    """One whole second pass -> (device ms by events, wall ms, the describer)."""
    describer = DS.ChannelDescriber(plan, fin, channels, "s16", "iq", keying=True, identify=True, **{layer: on})
    n = plan.n_samples
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e[0].record()
    for a in range(0, n, FD.BLOCK_FRAMES):
        describer.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    describer.keying_result(fc)
    describer.protocol_result(fc)
    if on:
        describer.layer_result(layer, fc)
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), (time.perf_counter() - t0) * 1e3, describer


def timed(fn) -> float:
    """Device ms of one call of ``fn`` by events."""
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    e[0].record()
    fn()
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1])


def entry_ms(fn) -> dict:
    """An entry point on its own: one warm-up, then the median of REPEATS."""
    fn()
    return FT.med([timed(fn) for _ in range(REPEATS)])


def run(layer: str, fc: float, what: str, add, sent_key: str, summary, first_lines: int, entry_points) -> None:
    """The whole measurement of ``layer``, one JSON line.  ``add(capture)`` writes the channel (``what`` in the capture's text) and
    returns what it sent (``sent_key``); ``summary(ch)`` is the dict of one channel of the result; ``entry_points(st, head)`` times
    the entry points on ``st``, the lane's dict of ``finish_layer``, into ``head`` (offset_hz, fs_ch, sps) and returns it."""
    torch.cuda.set_device(0)
    capture = FT.make_capture()
    sent = add(capture)
    n = int(capture.numel()) // 2
    plan = P.plan_find(FT.FS, n)
    out = {"capture": f"{FT.SECS:.0f} s @ {FT.FS / 1e6:.0f} MS/s cs16, device-resident, with {what} at {OFFSET:+.0f} Hz",
           "device": torch.cuda.get_device_name(0), "repeats": REPEATS, sent_key: sent}
    finder = FD.ChannelFinder(plan, "s16")
    for a in range(0, n, FD.BLOCK_FRAMES):
        finder.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    fin, found = finder.finish(), finder.result(fc)
    runs = {False: [], True: []}
    for on in (False, True):
        second_pass(capture, plan, fin, found.channels, fc, layer, on)  # warm-up: tap fragments, code objects, pools
    last = None
    for _ in range(REPEATS):  # alternating
        for on in (False, True):
            r = second_pass(capture, plan, fin, found.channels, fc, layer, on)
            runs[on].append(r)
            last = r[2] if on else last
    for on, tag in ((False, "identify"), (True, layer)):
        out[f"{tag}_device_ms"], out[f"{tag}_wall_ms"] = FT.med([r[0] for r in runs[on]]), FT.med([r[1] for r in runs[on]])
    out["keying"] = [line.strip() for line in last.keying_result(fc).lines()]
    out["protocols"] = [line.strip() for line in last.protocol_result(fc).lines()]
    result = last.layer_result(layer, fc)
    out["channels"] = [summary(ch) for ch in result.channels]
    out["first_lines"] = result.lines()[:first_lines]
    out["entry_points"] = [entry_points(st, dict(offset_hz=ch.offset_hz, fs_ch=lane.plan.fs_ch, sps=st["plan"].sps))
                           for ch, lane, st in zip(found.channels, last.lanes(), last.finish_layer(layer)) if "rows" in st and len(st["rows"])]
    print(json.dumps(out))
