"""Child process of ``test_gpu_threads.py::test_first_use_from_two_threads_in_a_fresh_process``.

In a process that has launched nothing yet, two threads (a stream each) meet at a barrier and then make, at the same
moment, the process's FIRST launch of each kernel that raises its dynamic-LDS limit (the contiguous-slot ring kernel at
D = 104, the per-lane kernel), ``iqa_rds_baseband`` at its largest LDS image, and the first lane-pair launch, which
allocates the pacing buffer.  Prints ``digest <hex>`` of everything the launches wrote (thread 0's, then thread 1's);
the parent compares it with the digest of the same jobs run serially and checked against their models there.
Exit status 0 only if both threads finished; nothing is retried."""
from __future__ import annotations

import sys
import threading
from pathlib import Path

HERE = Path(__file__).resolve().parent
for p in (str(HERE), str(HERE.parent)):
    if p not in sys.path:
        sys.path.insert(0, p)

WAIT = 60.0


def main() -> int:
    import threads_work as W
    import torch

    from iq_to_audio_amd import _native as N

    N.lib()
    N.require_gpu()
    gate, prepare = threading.Barrier(2), threading.Lock()
    out, errs = [None, None], []

    def worker(who: int):
        try:
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                with prepare:  # (uploads and models: the test helpers' memo tables are not made for threads)
                    jobs = W.first_use_jobs(who)
                    pair = W.PairJob(13)
                    lanes = pair.lanes()
                stream.synchronize()
                for job in jobs:
                    gate.wait(WAIT)
                    job.launch()
                gate.wait(WAIT)
                pair.launch(lanes)
                stream.synchronize()
                out[who] = [a for job in jobs for a in job.outputs()] + [ln.out.cpu().numpy() for ln in lanes]
        except BaseException as exc:  # noqa: BLE001
            errs.append(repr(exc))
            gate.abort()

    threads = [threading.Thread(target=worker, args=(i,), daemon=True) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(2 * WAIT)
    if errs or any(t.is_alive() for t in threads) or any(o is None for o in out):
        print("failed", errs, [t.is_alive() for t in threads], flush=True)
        return 1
    print("digest", W.digest(out[0] + out[1]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
