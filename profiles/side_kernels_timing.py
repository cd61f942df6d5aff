"""Per-call device times of the side decoders' entry points whose kernels are built from csrc/sideband.h (DESIGN.md section
20): iqa_pocsag_integrate, iqa_afsk_correlate / _bits / _frames, iqa_ais_filter / _symbols / _frames and iqa_acars_max /
_detect / _bits / _frames, at the shapes of profiles/pocsag_timing.py, ax25_timing.py, ais_timing.py and acars_timing.py: a
channel of 10e6 / 104 = 96 153.8 Hz in blocks of 64 Mi / 104 = 645 277 samples, BLOCKS of them per run (POCSAG 188 / 80 / 40,
AFSK L = 80, AIS W = 29, ACARS W = 53 and L = 40).  The input is seeded noise (a discriminator output uniform in +-1 rad per
sample, an envelope uniform in 0 .. 1): the filters do not care what they filter, and on noise the frame kernels test every
position's opener and walk the chance hits (one position in 256 for AFSK) until they abort.  The decoders' own cores make the
calls; device events sit around every call, as profiles/ais_timing.py's CallTimes puts them.  Prints one JSON line:
per entry point the per-call milliseconds of each of REPEATS runs behind one warm-up run.

Two builds are compared by running this file alternately with IQA_LIB naming the one library and the other
(profiles/side_kernels_shared.json)."""
from __future__ import annotations

import json
import sys
from collections import defaultdict
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from iq_to_audio_amd import _native as N  # noqa: E402
from iq_to_audio_amd import dsp_plan as P  # noqa: E402
from iq_to_audio_amd.decoders.acars import AcarsCore  # noqa: E402
from iq_to_audio_amd.decoders.ais import AisCore  # noqa: E402
from iq_to_audio_amd.decoders.ax25 import AfskCore  # noqa: E402
from iq_to_audio_amd.decoders.pocsag import PocsagCore  # noqa: E402

FS_CH = 10e6 / 104
BLOCK = 64 * 1024 * 1024 // 104
BLOCKS = 8
REPEATS = 5
PREFIXES = ("iqa_pocsag_integrate", "iqa_afsk_", "iqa_ais_", "iqa_acars_")


def one_run(cores, theta, envelope) -> dict:
    events, real = [], N.call

    def timed(name, *args):
        if not name.startswith(PREFIXES):
            return real(name, *args)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        try:
            return real(name, *args)
        finally:
            e[1].record()
            events.append((name, e))

    N.call = timed
    try:
        for name, core in cores.items():
            core.reset()
            for block in (envelope if name == "acars" else theta):
                core.process(block)
            if name != "pocsag":  # (its finish runs no kernel of the shared header)
                core.finish()
    finally:
        N.call = real
    torch.cuda.synchronize()
    ms, count = defaultdict(float), defaultdict(int)
    for name, e in events:
        ms[name] += e[0].elapsed_time(e[1])
        count[name] += 1
    return {name: ms[name] / count[name] for name in sorted(ms)}


def main():
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(11)
    theta = [torch.rand(BLOCK, generator=g, device="cuda", dtype=torch.float32) * 2.0 - 1.0 for _ in range(BLOCKS)]
    envelope = [torch.rand(BLOCK, generator=g, device="cuda", dtype=torch.float32) for _ in range(BLOCKS)]
    cores = dict(pocsag=PocsagCore(P.plan_pocsag(FS_CH)), afsk=AfskCore(P.plan_afsk(FS_CH)), ais=AisCore(P.plan_ais(FS_CH)),
                 acars=AcarsCore(P.plan_acars(FS_CH)))
    one_run(cores, theta, envelope)  # warm-up: code objects, allocator
    runs = [one_run(cores, theta, envelope) for _ in range(REPEATS)]
    out = dict(library=str(N.LIB_PATH), device=torch.cuda.get_device_name(0), channel_rate=FS_CH, block=BLOCK, blocks=BLOCKS,
               per_call_ms={name: [round(r[name], 5) for r in runs] for name in runs[0]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
