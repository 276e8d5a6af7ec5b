#!/usr/bin/env python
"""BASELINE.json configs[4], clustering-only stressor: X f64 [N, 128] drawn around K = 500 identity centres so
that within-identity distances sit at 0.3-0.5 and between-identity ones near 0.8 (they bracket the reference's 0.6 threshold,
clustering.py:138), T = 10 000 tracks with 1 (N = 1e4) or 10 (N = 1e5) rows each.  Times K10 (pair_tiles_k on the f64 matrix cores)
and K11 (hac_persist_k) with the library's HIP events and checks the result against the generator's ground truth.
    python tools/c5_cluster.py [out.json]
The 10 000 x 10 case is run a second time with the do-not-cooccur constraint (clustering.py:142-143; FaceClustering(constraint='cooccur')):
extents drawn so that about one pair in a hundred is forbidden; the agglomeration's time with it (the stamping kernel included and also
on its own, beside a plain fill of the same T x T matrix) stands next to the time without.
"""
import json
import os
import sys
import time
import numpy as np
import torch  # noqa: F401  first, as in bench.py: the process then runs on the HIP runtime torch ships (used for the plain fill below)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
from pyannote_video_amd.runtime import Context  # noqa: E402

F64_MFMA_PEAK_TFLOPS = 78.6     # MI355X fp64 matrix = fp64 vector peak


def make(T, rows, K=500, seed=20260925):
    rng = np.random.default_rng(seed)
    cent = rng.normal(size=(K, 128)); cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    ident = rng.integers(0, K, T)
    x = cent[np.repeat(ident, rows)] + 0.05 * rng.normal(size=(T * rows, 128))
    x = np.round(0.55 * x / np.linalg.norm(x, axis=1, keepdims=True), 5)
    return x, (np.arange(T + 1) * rows).astype(np.int32), ident


def extents(T, span=300.0, seed=20261018):
    """(start, end) per track: 0.5-2.5 s long, starts uniform over `span` seconds -- two tracks intersect with probability ~ 2 * 1.5 / span"""
    rng = np.random.default_rng(seed)
    start = np.round(rng.uniform(0.0, span, T), 3)
    return np.stack([start, start + np.round(rng.uniform(0.5, 2.5, T), 3)], axis=1)


def constrained(ctx, X, rs, free_labels, reps=3):
    """the same agglomeration with the constraint: HIP-event times of the `hac` family (stamping included) and of the stamping kernel
    alone (one launch between two HIP events per call), the latter beside torch's fill of a matrix of the same size timed the same way"""
    T = len(rs) - 1
    ext = extents(T)
    hac, stamp = [], []
    for _ in range(reps):
        ctx.prof_reset(); ctx.prof_enable(True)
        labels, log, n_blocked = ctx.cluster_tracks_cooccur(X, rs, 0.6, extent=ext)
        ctx.prof_enable(False)
        hac.append(ctx.prof_get("hac")[0]); stamp.append(ctx.prof_get("cooccur_stamp")[0])
    s, e = ext[:, 0], ext[:, 1]
    viol = viol_free = 0
    for i0 in range(0, T, 1000):                          # co-occurring pairs that share a label, with and without the constraint
        co = (np.minimum(e[i0:i0 + 1000, None], e[None, :]) - np.maximum(s[i0:i0 + 1000, None], s[None, :])) > 1e-6
        co &= np.arange(i0, min(i0 + 1000, T))[:, None] < np.arange(T)[None, :]
        viol += int((co & (labels[i0:i0 + 1000, None] == labels[None, :])).sum())
        viol_free += int((co & (free_labels[i0:i0 + 1000, None] == free_labels[None, :])).sum())
    # the plain fill, timed the way the stamp is: one launch between two events per repetition, after two warm-up fills
    m = torch.empty(T * T, dtype=torch.float64, device="cuda")
    fill = []
    for rep in range(2 + reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(); m.fill_(float("inf")); ev[1].record(); torch.cuda.synchronize()
        if rep >= 2:
            fill.append(ev[0].elapsed_time(ev[1]))
    return {"forbidden_pairs": int(n_blocked), "forbidden_fraction": round(n_blocked / (T * (T - 1) / 2.0), 5), "hac_ms_constrained": [round(v, 3) for v in hac],
            "stamp_ms": [round(v, 4) for v in stamp], "plain_fill_ms_same_matrix": [round(v, 4) for v in fill],
            "merges": int(len(log)), "clusters": int(len(set(labels.tolist()))), "nan_in_log": bool(np.isnan(log).any()),
            "cooccurring_pairs_sharing_a_label": viol, "cooccurring_pairs_sharing_a_label_without_constraint": viol_free}


def main():  # noqa: C901
    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = Context(device=0, detector=None)
    res = []
    for T, rows in ((10000, 1), (10000, 10), (2000, 50), (720, 250)):      # the last: one GPU's share of configs[2] (22 500 frames, 250-row tracks)
        X, rs, ident = make(T, rows)
        N = len(X)
        ctx.cluster_tracks(X[:rs[64]], rs[:65], 0.6)                  # warm-up (module load, buffers)
        ctx.prof_reset(); ctx.prof_enable(True)
        t0 = time.perf_counter()
        labels, log = ctx.cluster_tracks(X, rs, 0.6)
        wall = time.perf_counter() - t0
        ctx.prof_enable(False)
        pd_ms, _ = ctx.prof_get("pdist")
        hac_ms, _ = ctx.prof_get("hac")
        pure = all(ident[labels[t]] == ident[t] for t in range(T))
        one = len(set(labels.tolist())) == len(set(ident.tolist()))
        # the algorithm's work: the N (N - 1) / 2 row pairs the reference's pdist computes (clustering.py:101), one 128-D dot product each
        # (Gram form).  Round 3 reported 2 * 128 * N^2 -- both triangles, which that kernel really swept; the upper-triangle kernel
        # does not, so its rate is quoted on the pairs that exist.
        flop = 2.0 * 128 * N * (N - 1) / 2.0
        # the in-memory path on the same rows: float32 descriptors, table rounded + gathered on the device
        E = X.astype(np.float32)
        ctx.prof_reset(); ctx.prof_enable(True)
        t1 = time.perf_counter()
        lf, logf = ctx.cluster_tracks_f32(E, None, rs, 0.6)
        wall_f32 = time.perf_counter() - t1
        ctx.prof_enable(False)
        # the full-size case against the CPU oracle's frozen result (tests/golden/c5_cluster_T10000.npz, made by tests/golden/make_c5_cluster.py)
        fixture = None
        fx = os.path.join(ROOT, "tests", "golden", "c5_cluster_T10000.npz")
        if (T, rows) == (10000, 10) and os.path.exists(fx):
            g = np.load(fx)
            same_pairs = len(log) == len(g["merge_pairs"]) and np.array_equal(np.asarray(log)[:, :2].astype(np.int32), g["merge_pairs"])
            fixture = {"labels_equal_oracle": bool(np.array_equal(labels, g["labels"])), "merges_equal_oracle_in_order": bool(same_pairs),
                       "merge_distance_max_abs_diff": float(np.abs(np.asarray(log)[:, 2] - g["merge_dist"]).max()) if len(log) == len(g["merge_dist"]) else None,
                       "f32_path_labels_equal_oracle": bool(np.array_equal(lf, g["labels"]))}
        res.append({"T": T, "rows_per_track": rows, "N": N, "oracle_fixture": fixture, "pdist_ms": round(pd_ms, 3), "hac_ms": round(hac_ms, 3), "wall_s": round(wall, 3), "wall_s_f32_in_memory_path": round(wall_f32, 3), "f32_path_same_labels": bool(np.array_equal(lf, labels)),
                    "pdist_fp64_tflops": round(flop / (pd_ms * 1e-3) / 1e12, 2), "pdist_frac_of_fp64_mfma_peak": round(flop / (pd_ms * 1e-3) / 1e12 / F64_MFMA_PEAK_TFLOPS, 3),
                    "merges": int(len(log)), "merges_per_s": round(len(log) / max(hac_ms * 1e-3, 1e-9)),
                    "hac_D_bytes": int(T) * int(T) * 8, "clusters": int(len(set(labels.tolist()))), "identities": int(len(set(ident.tolist()))),
                    "clusters_pure": bool(pure), "one_cluster_per_identity": bool(one)})
        if (T, rows) == (10000, 10):
            res[-1]["do_not_cooccur"] = constrained(ctx, X, rs, labels)
        print(json.dumps(res[-1]))
        sys.stdout.flush()
    if out:
        with open(out, "w") as f:
            json.dump({"what": "configs[4] clustering stressor on one MI355X: pair_tiles_k (v_mfma_f64_16x16x4_f64) + hac_persist_k", "results": res}, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
