#!/usr/bin/env python
"""Identification at the c5 scale (tools/c5_cluster.py's rows): N = 100 000 query rows in T = 10 000 groups against a gallery of
M = 10 000 rows in K = 1 000 identities, one MI355X.  Times pvf_identify (cross_tiles_k + identify_pick_k) and, in the same process, the
route a user had before it: pvf_pair_mean_dist over the concatenated table, of whose (T + K)^2 matrix the T x K corner is read.  Three
alternating runs each; wall time of the call (uploads and the copy of the result included: the call a user makes) and the HIP-event
time of the kernels alone.  The rectangular kernel computes N M pair distances, the concatenation (N + M)^2 / 2.
    python tools/bench_identify.py [out.json]
"""
import json
import os
import sys
import time
import numpy as np
import torch  # noqa: F401  first, as in bench.py: the process then runs on the HIP runtime torch ships

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
from pyannote_video_amd.runtime import Context  # noqa: E402

F64_MFMA_PEAK_TFLOPS = 78.6     # MI355X fp64 matrix = fp64 vector peak
T, ROWS, K, GROWS = 10000, 10, 1000, 10


def make(seed=20261018):
    """queries around 1 500 centres of which the first 1 000 are enrolled: within-identity distances 0.3-0.5, between ~0.8"""
    rng = np.random.default_rng(seed)
    cent = rng.normal(size=(K * 3 // 2, 128)); cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    ident = rng.integers(0, len(cent), T)

    def rows(c, n):
        x = cent[np.repeat(c, n)] + 0.05 * rng.normal(size=(len(c) * n, 128))
        return np.round(0.55 * x / np.linalg.norm(x, axis=1, keepdims=True), 5)
    return rows(ident, ROWS), (np.arange(T + 1) * ROWS).astype(np.int32), rows(np.arange(K), GROWS), (np.arange(K + 1) * GROWS).astype(np.int32), ident


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = Context(device=0, detector=None)
    X, rs, G, gs, ident = make()
    N, M = len(X), len(G)
    XG, rsg = np.concatenate([X, G]), np.concatenate([rs, gs[1:] + N]).astype(np.int32)
    ctx.identify(X[:rs[64]], rs[:65], G[:gs[8]], gs[:9], 0.6)             # warm-up (module load)
    ctx.pair_mean_dist(XG[:rs[64]], rs[:65])
    runs = {"identify": [], "concat": []}
    for rep in range(4):                                                  # the first pair grows the buffers: not counted
        for name in ("identify", "concat"):
            ctx.prof_reset(); ctx.prof_enable(True)
            t0 = time.perf_counter()
            if name == "identify":
                best, bd, second, sd = ctx.identify(X, rs, G, gs, 0.6)
            else:
                corner = ctx.pair_mean_dist(XG, rsg)[:T, T:]
            wall = (time.perf_counter() - t0) * 1e3
            ctx.prof_enable(False)
            if rep:
                runs[name].append((wall, ctx.prof_get("identify" if name == "identify" else "pdist")[0]))
    D = ctx.gallery_mean_dist(X, rs, G, gs)
    truth = np.where(ident < K, ident, -1)
    res = {"what": "pvf_identify against pvf_pair_mean_dist on the concatenated table, one MI355X, three alternating runs each",
           "N": N, "T": T, "M": M, "K": K, "threshold": 0.6,
           "pair_distances_identify": N * M, "pair_distances_concat": (N + M) * (N + M - 1) // 2,
           "names_equal_generator_truth": bool(np.array_equal(best, truth)), "matched_groups": int((best >= 0).sum()),
           "max_abs_diff_to_concat_corner": float(np.abs(D - corner).max())}
    for name, flop in (("identify", 2.0 * 128 * N * M), ("concat", 2.0 * 128 * (N + M) * (N + M - 1) / 2.0)):
        wall, kern = [r[0] for r in runs[name]], [r[1] for r in runs[name]]
        res[name] = {"wall_ms": [round(v, 3) for v in wall], "kernel_ms": [round(v, 3) for v in kern],
                     "kernel_fp64_tflops": [round(flop / (v * 1e-3) / 1e12, 2) for v in kern],
                     "kernel_frac_of_fp64_mfma_peak": round(flop / (min(kern) * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS, 3)}
    for key in ("wall_ms", "kernel_ms"):
        a, b = res["identify"][key], res["concat"][key]
        spread = max(max(a) - min(a), max(b) - min(b))
        res["faster_by_more_than_the_spread_" + key] = bool(min(b) - max(a) > spread)
        res["speedup_median_" + key] = round(float(np.median(b) / np.median(a)), 2)
    res["k10_fp64_tflops_r06_c5_cluster_same_N"] = 37.3
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()
    return 0 if res["faster_by_more_than_the_spread_wall_ms"] and res["faster_by_more_than_the_spread_kernel_ms"] else 1


if __name__ == "__main__":
    sys.exit(main())
