#!/usr/bin/env python
"""num_jitters at the size of a gallery enrolment: n = 256 faces, J = 10 and 100 jitters each, one MI355X.  Per J, from the library's
profiling families (HIP events around the kernels): the milliseconds of jitter_k ("jitter"), of the embedder's forward it feeds ("conv"),
and of the same chips sampled by transform_k launched over n * J jobs on the chips in HBM ("jitter_xf", the debug switch
pvf_debug_jitter_chips_transform; its mirrored jitters stay unmirrored: the same reads, arithmetic and bytes written).  Three runs after
a warm-up that grows the buffers; the two jitter kernels alternate.
    python tools/bench_jitter.py [out.json]
"""
import json
import os
import sys
import tempfile
import time
import numpy as np
import torch  # noqa: F401  first, as in bench.py: the process then runs on the HIP runtime torch ships

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
from pyannote_video_amd import models  # noqa: E402
from pyannote_video_amd.runtime import Context  # noqa: E402

N = 256
CHIP_BYTES = 150 * 150 * 3


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    _, ep = models.ensure_synthetic_models(tempfile.mkdtemp(), small=True)
    ctx = Context(device=0, detector=None, embedding=ep)
    rng = np.random.default_rng(20261019)
    chips = rng.integers(0, 256, (N, 150, 150, 3), dtype=np.uint8)
    res = {"what": "jitter_k against transform_k over n*J jobs, and the forward the jittered chips feed; one MI355X, three runs each",
           "n": N, "chip_bytes": CHIP_BYTES}
    for J in (10, 100):
        ctx.embed_chips(chips, num_jitters=J)                                 # warm-up: module load, buffers
        ctx.jitter_chips(chips, J, via_transform=True, copy_out=False)
        runs = {"jitter_ms": [], "forward_ms": [], "transform_ms": [], "call_wall_ms": []}
        for rep in range(3):
            ctx.prof_reset(); ctx.prof_enable(True)
            t0 = time.perf_counter()
            ctx.embed_chips(chips, num_jitters=J)
            wall = (time.perf_counter() - t0) * 1e3
            ctx.prof_enable(False)
            runs["jitter_ms"].append(round(ctx.prof_get("jitter")[0], 4))
            runs["forward_ms"].append(round(ctx.prof_get("conv")[0], 4))
            runs["call_wall_ms"].append(round(wall, 3))
            launches = ctx.prof_get("jitter")[1]
            ctx.prof_reset(); ctx.prof_enable(True)
            ctx.jitter_chips(chips, J, via_transform=True, copy_out=False)
            ctx.prof_enable(False)
            runs["transform_ms"].append(round(ctx.prof_get("jitter_xf")[0], 4))
        jm, fm, tm = (float(np.median(runs[k])) for k in ("jitter_ms", "forward_ms", "transform_ms"))
        written = N * J * CHIP_BYTES
        runs.update(J=J, chips=N * J, rounds=int(launches), bytes_written=written,
                    jitter_write_GBps=round(written / (jm * 1e-3) / 1e9, 1), transform_write_GBps=round(written / (tm * 1e-3) / 1e9, 1),
                    jitter_us_per_chip=round(jm * 1e3 / (N * J), 4), forward_us_per_chip=round(fm * 1e3 / (N * J), 4),
                    jitter_share_of_kernels=round(jm / (jm + fm), 4), transform_over_jitter=round(tm / jm, 3),
                    jitter_k_not_slower_than_transform_k=bool(jm <= tm))
        res["J%d" % J] = runs
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
