"""Cost of the YSF frame decoding (--find-ysf) on the device-resident capture of profiles/find_timing.py
(60 s at 10 MS/s int16, the capture and the method of profiles/p25_timing.py) with a YSF channel in place of the P25 one: the
test script of tests/ysf_model.py (a transmission of 13 frames: header, V/D mode 2, V/D mode 1, data FR, voice FR, terminator)
in a loop, at -3.6 MHz, written into the capture on the device.  The finder runs once; its channels then go through
``ChannelDescriber`` in the blocks ``find_channels`` uses, with ``identify`` alone (the yardstick) and with ``ysf`` beside it,
alternating in one process.  By device events behind one warm-up each: the whole second pass with its results (median of
REPEATS).  Then the three entry points on their own, on the YSF lane's plane: median of REPEATS each.  Prints one JSON line (kept
as profiles/ysf_timing.json).  Kernel resources: ``make -C iq-to-audio_amd/csrc asm F=ysf``."""
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
from iq_to_audio_amd import ysf as X  # noqa: E402


def _load(name, folder):
    spec = importlib.util.spec_from_file_location(name, ROOT / folder / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


FT = _load("find_timing", "profiles")
YM = _load("ysf_model", "tests")

REPEATS = FT.REPEATS
FC = 433.0e6
YSF_OFFSET, YSF_AMP = -3.6e6, 0.01  # (the place and the amplitude of profiles/dmr_timing.py's added channel)


def add_ysf(capture) -> int:
    """Adds the YSF channel to the device capture in place, a second at a time: the script's symbols in a loop, every symbol one
    entry of a level table.  Returns the frames sent."""
    table = YM.station(YM.SCRIPT)
    assert len(table) == 480 * len(YM.SCRIPT)
    levels = torch.tensor(table, dtype=torch.float64, device="cuda")
    fs, n = FT.FS, int(capture.numel()) // 2
    phase = 0.0
    for a in range(0, n, int(fs)):
        b = min(n, a + int(fs))
        k = torch.arange(a, b, dtype=torch.int64, device="cuda")
        symbol = torch.div(k * 4800, int(fs), rounding_mode="floor") % len(table)
        turns = torch.cumsum(levels[symbol] * (YM.DEV / fs), 0) + phase
        phase = float(turns[-1]) % 1.0
        angle = 2.0 * math.pi * ((turns + (k.to(torch.float64) * (YSF_OFFSET / fs))) % 1.0)
        z = torch.stack([torch.cos(angle), torch.sin(angle)], dim=1) * (YSF_AMP * 32768.0)
        capture[2 * a : 2 * b] += torch.round(z).to(torch.int16).reshape(-1)
    return int(n * 4800 // (int(fs) * 480))


def second_pass(capture, plan, fin, channels, ysf: bool):
    """One whole second pass -> (device ms by events, wall ms, the describer)."""
    describer = DS.ChannelDescriber(plan, fin, channels, "s16", "iq", keying=True, identify=True, ysf=ysf)
    n = plan.n_samples
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e[0].record()
    for a in range(0, n, FD.BLOCK_FRAMES):
        describer.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    describer.keying_result(FC)
    describer.protocol_result(FC)
    if ysf:
        describer.ysf_result(FC)
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


def main():
    torch.cuda.set_device(0)
    capture = FT.make_capture()
    sent = add_ysf(capture)
    n = int(capture.numel()) // 2
    plan = P.plan_find(FT.FS, n)
    out = dict(capture=f"{FT.SECS:.0f} s @ {FT.FS / 1e6:.0f} MS/s cs16, device-resident, with a YSF channel at {YSF_OFFSET:+.0f} Hz",
               device=torch.cuda.get_device_name(0), repeats=REPEATS, frames_sent=sent)
    finder = FD.ChannelFinder(plan, "s16")
    for a in range(0, n, FD.BLOCK_FRAMES):
        finder.process(capture[2 * a : 2 * min(n, a + FD.BLOCK_FRAMES)])
    fin, found = finder.finish(), finder.result(FC)
    runs = {False: [], True: []}
    for ysf in (False, True):
        second_pass(capture, plan, fin, found.channels, ysf)  # warm-up: tap fragments, code objects, pools
    last = None
    for _ in range(REPEATS):  # alternating
        for ysf in (False, True):
            r = second_pass(capture, plan, fin, found.channels, ysf)
            runs[ysf].append(r)
            last = r[2] if ysf else last
    for ysf, tag in ((False, "identify"), (True, "ysf")):
        out[f"{tag}_device_ms"], out[f"{tag}_wall_ms"] = FT.med([r[0] for r in runs[ysf]]), FT.med([r[1] for r in runs[ysf]])
    out["keying"] = [line.strip() for line in last.keying_result(FC).lines()]
    out["protocols"] = [line.strip() for line in last.protocol_result(FC).lines()]
    result = last.ysf_result(FC)
    out["channels"] = [dict(offset_hz=ch.offset_hz, note=ch.note, frames=ch.frames, no_level=ch.no_level, cut=ch.cut, fich_failed=ch.fich_failed,
                            golay_refused=ch.golay_refused, dch_failed=ch.dch_failed, fixed=ch.fixed, inverted=ch.inverted,
                            transmissions=len(ch.transmissions), terminated=sum(t.terminated for t in ch.transmissions),
                            conflicts=sum(t.conflicts for t in ch.transmissions)) for ch in result.channels]
    out["first_lines"] = result.lines()[:3]
    entries = []
    for ch, lane, st in zip(found.channels, last.lanes(), last.finish_ysf()):
        if "rows" not in st or not len(st["rows"]):
            continue
        yplan, rows = st["plan"], st["rows"]
        entry = dict(offset_hz=ch.offset_hz, fs_ch=lane.plan.fs_ch, sps=yplan.sps, samples=int(st["v"].numel()), frames=len(rows))
        X.slice_frames(st["v"], rows, yplan)  # warm-up
        entry["slice_ms"] = FT.med([timed(lambda: X.slice_frames(st["v"], rows, yplan)) for _ in range(REPEATS)])
        X.decode_fich(st["bits"])  # warm-up
        entry["fich_ms"] = FT.med([timed(lambda: X.decode_fich(st["bits"])) for _ in range(REPEATS)])
        X.decode_frames(st["bits"], st["classes"])  # warm-up
        entry["decode_ms"] = FT.med([timed(lambda: X.decode_frames(st["bits"], st["classes"])) for _ in range(REPEATS)])
        entries.append(entry)
    out["entry_points"] = entries
    print(json.dumps(out))


if __name__ == "__main__":
    main()
