#!/usr/bin/env python
"""Search at Q = 256 queries, k = 100, against N synthetic 5-decimal rows, one MI355X.  Times pvf_search (search_quant_k +
search_tiles_k + search_merge_k) and, in the same process on the same inputs, the only route a user had before it:
Context.gallery_mean_dist on singleton groups -- a Q x N float64 matrix copied to the host -- plus np.argpartition and a sort there.
Three alternating runs each after one uncounted pair that grows the buffers; wall time of the call a user makes (uploads, copies and,
for the route, the host selection included) and the HIP-event time of the kernels alone; median, lowest and highest.  Both do the same
2 * 128 * Q * N flop on the f64 matrix cores.  The lists are compared wherever the route's distances, recovered as rint((D * 1e5)^2),
do not tie among a query's first k + 1; the share of queries compared is reported, not a pass mark.
    python tools/bench_search.py [out.json] [N] [--large N2]       (N2: one more pvf_search run through the chunked path, e.g. 10000000)
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

F64_MFMA_PEAK_TFLOPS = 78.6     # MI355X fp64 matrix
Q, K_HITS = 256, 100


def make(n, seed=20261020):
    """unit-sphere descriptors scaled to 0.55 around n / 50 centres, as the 5-decimal text gives them back"""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((max(n // 50, 1), 128)).astype(np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    x = cent[rng.integers(0, len(cent), n)] + 0.05 * rng.standard_normal((n, 128), dtype=np.float32)
    x *= 0.55 / np.linalg.norm(x, axis=1, keepdims=True)
    return np.round(x.astype(np.float64), 5)


def route(ctx, Qr, X, k):
    """the parent commit's route: all distances to the host, the k smallest there by (D, index)"""
    D = ctx.gallery_mean_dist(Qr, np.arange(len(Qr) + 1, dtype=np.int32), X, np.arange(len(X) + 1, dtype=np.int32))
    part = np.argpartition(D, k, axis=1)[:, :k + 1]
    d = np.take_along_axis(D, part, 1)
    order = np.lexsort((part, d), axis=1)
    return np.take_along_axis(part, order, 1), np.take_along_axis(d, order, 1)


def stats(v):
    return {"median": round(float(np.median(v)), 3), "lowest": round(float(min(v)), 3), "highest": round(float(max(v)), 3)}


def main():
    argv = sys.argv[1:]
    large = 0
    if "--large" in argv:
        i = argv.index("--large")
        large = int(argv[i + 1])
        del argv[i:i + 2]
    out = argv[0] if argv else None
    N = int(argv[1]) if len(argv) > 1 else 200000
    ctx = Context(device=0, detector=None)
    X = make(N)
    Qr = X[np.random.default_rng(1).choice(N, Q, replace=False)].copy()
    ctx.search(Qr[:16], X[:1000], 10)                                     # warm-up (module load)
    route(ctx, Qr[:16], X[:1000], 10)
    runs = {"search": [], "route": []}
    for rep in range(4):                                                  # the first pair grows the buffers: not counted
        for name in ("search", "route"):
            ctx.prof_reset(); ctx.prof_enable(True)
            t0 = time.perf_counter()
            if name == "search":
                idx, d2, count = ctx.search(Qr, X, K_HITS)
            else:
                r_idx, r_d = route(ctx, Qr, X, K_HITS)
            wall = (time.perf_counter() - t0) * 1e3
            ctx.prof_enable(False)
            if rep:
                runs[name].append((wall, ctx.prof_get("search" if name == "search" else "identify")[0]))
    # agreement, where the route does not tie
    r_d2 = np.rint((r_d * 1e5) ** 2).astype(np.int64)
    clear = (np.diff(r_d2, axis=1) > 0).all(1)
    same = [bool(np.array_equal(idx[q], r_idx[q, :K_HITS]) and np.array_equal(d2[q], r_d2[q, :K_HITS])) for q in np.flatnonzero(clear)]
    flop = 2.0 * 128 * Q * N
    res = {"what": "pvf_search against gallery_mean_dist on singleton groups + argpartition on the host, one MI355X, three alternating runs each",
           "Q": Q, "N": N, "k": K_HITS, "plan": ctx.search_plan(Q, N, K_HITS), "flop": flop,
           "queries_compared_share": round(float(clear.mean()), 4), "queries_compared": int(clear.sum()),
           "compared_queries_with_identical_hits": int(sum(same)), "every_query_finds_itself_first": bool((d2[:, 0] == 0).all())}
    for name in ("search", "route"):
        wall, kern = [r[0] for r in runs[name]], [r[1] for r in runs[name]]
        res[name] = {"wall_ms": stats(wall), "kernel_ms": stats(kern), "wall_ms_runs": [round(v, 3) for v in wall],
                     "kernel_ms_runs": [round(v, 3) for v in kern],
                     "kernel_fp64_tflops_median": round(flop / (float(np.median(kern)) * 1e-3) / 1e12, 2),
                     "kernel_frac_of_fp64_mfma_peak": round(flop / (min(kern) * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS, 3)}
    for key in ("wall_ms", "kernel_ms"):
        res["ratio_route_over_search_median_" + key] = round(res["route"][key]["median"] / res["search"][key]["median"], 2)
        res["search_not_slower_" + key] = bool(res["search"][key]["median"] <= res["route"][key]["median"])
    if large:
        try:
            reps = -(-large // N)
            XL = np.tile(X, (reps, 1))[:large]
            ctx.prof_reset(); ctx.prof_enable(True)
            t0 = time.perf_counter()
            li, ld, lc = ctx.search(Qr, XL, K_HITS)
            wall = (time.perf_counter() - t0) * 1e3
            ctx.prof_enable(False)
            kern = ctx.prof_get("search")[0]
            # the table is X repeated: every distance of the small run comes back once per copy
            first = ld[:, ::reps] if large % N == 0 and K_HITS % reps == 0 else None
            res["large"] = {"N": large, "plan": ctx.search_plan(Q, large, K_HITS), "wall_ms": round(wall, 1), "kernel_ms": round(kern, 3),
                            "kernel_fp64_tflops": round(2.0 * 128 * Q * large / (kern * 1e-3) / 1e12, 2),
                            "host_table_gb": round(XL.nbytes / 1e9, 2),
                            "distances_of_the_first_copies_equal_the_small_run": None if first is None else bool(np.array_equal(first, d2[:, :K_HITS // reps]))}
        except MemoryError as e:
            res["large"] = {"N": large, "error": "host memory: %s" % e}
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
