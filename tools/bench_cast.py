#!/usr/bin/env python
"""The cast of N nodes at k = 64, one MI355X.  Times pvf_cast stage by stage (HIP events of the families cast_quant, cast_lists,
cast_links, cast_cc) and as the whole call a user makes (wall time, upload included), and, in the same process on the same nodes, the
only route a user had before it for the lists: the same self-join through Context.search in query batches of 4096 rows, every batch
uploading the table again and copying its lists to the host.  Alternating runs after one uncounted pair that grows the buffers; median,
lowest and highest.  The lists of the two are compared with np.array_equal.
    N = 10 000      the track means of the rows tools/c5_cluster.py clusters (the data of tests/golden/c5_cluster_T10000.npz)
    N = 100 000     blobs of N / 50 identities -- the size the bar is set at
    --large N2      one more pvf_cast call (no route) on N2 blob nodes, e.g. 1000000
    python tools/bench_cast.py [out.json] [--runs 3] [--large N2]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from pyannote_video_amd import cast as face_cast  # noqa: E402
from pyannote_video_amd.runtime import Context  # noqa: E402
from bench_search import make as blobs  # noqa: E402
import c5_cluster  # noqa: E402

F64_MFMA_PEAK_TFLOPS = 78.6     # MI355X fp64 matrix
K, MAX_D2, NUM, DEN, ROUTE_BATCH = 64, 60000 ** 2, 2000, 1000, 4096
STAGES = ("cast_quant", "cast_lists", "cast_links", "cast_cc")


def track_means():
    g = np.load(os.path.join(ROOT, "tests", "golden", "c5_cluster_T10000.npz"))
    T, rows = int(g["T"]), int(g["rows_per_track"])
    x, _, _ = c5_cluster.make(T, rows, seed=int(g["seed"]))
    q = face_cast.quantise(x).reshape(T, rows, 128)
    return np.array([face_cast.track_mean(t) for t in q], np.int64) / 1e5


def route(ctx, X, k, max_d2):
    """the parent commit's route to the lists: pvf_search batch by batch, each row in a group of its own"""
    N = len(X)
    own = np.arange(N, dtype=np.int32)
    parts = [ctx.search(X[q0:q0 + ROUTE_BATCH], X, k, max_d2=max_d2, query_group=own[q0:q0 + ROUTE_BATCH], row_group=own) for q0 in range(0, N, ROUTE_BATCH)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def stats(v):
    return {"median": round(float(np.median(v)), 3), "lowest": round(float(min(v)), 3), "highest": round(float(max(v)), 3)}


def one_cast(ctx, X):
    ctx.prof_reset(); ctx.prof_enable(True)
    t0 = time.perf_counter()
    labels, comps = ctx.cast(X, K, MAX_D2, NUM, DEN)
    wall = (time.perf_counter() - t0) * 1e3
    ctx.prof_enable(False)
    return dict({s: ctx.prof_get(s)[0] for s in STAGES}, wall=wall, launches_cc=ctx.prof_get("cast_cc")[1]), labels, comps


def measure(ctx, X, runs, with_route=True):
    N = len(X)
    cast_runs, route_runs = [], []
    for rep in range(runs + 1):                                           # the first pair grows the buffers: not counted
        r, labels, comps = one_cast(ctx, X)
        if rep:
            cast_runs.append(r)
        if with_route:
            ctx.prof_reset(); ctx.prof_enable(True)
            t0 = time.perf_counter()
            lists = route(ctx, X, K, MAX_D2)
            wall = (time.perf_counter() - t0) * 1e3
            ctx.prof_enable(False)
            if rep:
                route_runs.append({"wall": wall, "kernel": ctx.prof_get("search")[0]})
    flop = 2.0 * 128 * N * N
    res = {"N": N, "k": K, "plan": ctx.cast_plan(N, K), "components": int(comps), "flop_lists": flop}
    for s in STAGES + ("wall",):
        res[s + "_ms"] = stats([r[s] for r in cast_runs])
    res["cc_launches"] = int(cast_runs[-1]["launches_cc"])
    lists_ms = res["cast_lists_ms"]["median"]
    res["lists_fp64_tflops_median"] = round(flop / (lists_ms * 1e-3) / 1e12, 2)
    res["lists_frac_of_fp64_mfma_peak"] = round(flop / (res["cast_lists_ms"]["lowest"] * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS, 3)
    if with_route:
        idx, d2, count = ctx.cast_lists(X, K, MAX_D2)
        res["lists_equal_the_route"] = bool(np.array_equal(idx, lists[0]) and np.array_equal(d2, lists[1]) and np.array_equal(count, lists[2]))
        traffic = (float(count[idx[idx >= 0]].sum()) + float(count.sum())) * 4.0      # every L_b a wave reads, and its own L_a
        res["links_list_bytes"] = traffic
        res["links_list_gb_per_s_median"] = round(traffic / (res["cast_links_ms"]["median"] * 1e-3) / 1e9, 1)
        res["route"] = {"batch": ROUTE_BATCH, "wall_ms": stats([r["wall"] for r in route_runs]), "kernel_ms": stats([r["kernel"] for r in route_runs])}
        lists_wall = res["wall_ms"]["median"]
        res["ratio_route_wall_over_whole_cast_wall"] = round(res["route"]["wall_ms"]["median"] / lists_wall, 2)
        res["ratio_route_kernel_over_cast_lists_kernel"] = round(res["route"]["kernel_ms"]["median"] / lists_ms, 2)
        res["cast_not_slower_than_the_route"] = bool(lists_wall <= res["route"]["wall_ms"]["median"])
    return res


def main():
    argv = sys.argv[1:]
    large, runs = 0, 3
    for flag in ("--large", "--runs"):
        if flag in argv:
            i = argv.index(flag)
            if flag == "--large":
                large = int(argv[i + 1])
            else:
                runs = int(argv[i + 1])
            del argv[i:i + 2]
    out = argv[0] if argv else None
    ctx = Context(device=0, detector=None)
    ctx.cast(blobs(1000), 8)                                              # warm-up (module load)
    ctx.search(blobs(16), blobs(1000), 8)
    res = {"what": "pvf_cast (k = 64, cut 0.6, threshold 2.0) stage by stage against the same self-join through Context.search in batches of "
                   "4096 queries with the lists copied to the host; one MI355X, alternating runs in one process",
           "runs": runs, "track_means_10000": measure(ctx, track_means(), runs), "blobs_100000": measure(ctx, blobs(100000), runs)}
    if large:
        res["large"] = measure(ctx, blobs(large), 1, with_route=False)
    print(json.dumps(res))
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
