"""Blend bench (csrc/blend.hip; BLEND.md), on an MI355X, in one process.

pvf_frame_blend on 64 frames resident in HBM, 1080p and 2160p, thumbnails 64 x 36, with 32 planes of history.  After one uncounted pass,
three alternating windows of (a) frame_blend calls -- the two new kernels timed by the library's own device events (family "blend"),
frame_thumbs_k of the same calls by its own (family "thumbs"), and the calls' wall time -- and (b) the route a user had before:
Context.frame_thumbs to the host, then the rows through numpy (tests/blend_ref.py, the restatement), wall time.  Median with lowest and
highest.  Two bars: the call is not slower than the route before, and the two new kernels together take no longer than frame_thumbs_k
in the same calls.  The rows of both routes must be equal.

Writes profiles/blend_n64.json and prints it.

    python tools/bench_blend.py [--frames 64] [--width 64] [--calls 100]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
sys.path.insert(0, ROOT)


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 5), "lowest": round(s[0], 5), "highest": round(s[-1], 5)}


def bench(ctx, torch, a):
    from tests import blend_ref
    n, configs = a.frames, {}
    for name, (h, w) in (("1080p", (1080, 1920)), ("2160p", (2160, 3840))):
        tw, th = blend_ref.tile_size(a.width, w, h)
        P = tw * th
        src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        dev = [ctx.wrap_torch(src[i]) for i in range(n)]
        handles = ctx.frame_handles(dev)
        hist = np.random.default_rng(1).integers(0, 256, (32, P), dtype=np.uint8)

        def library(calls):
            """-> (ms of the two kernels, ms of frame_thumbs_k, wall ms) per call, and the rows"""
            ctx.prof_enable(True)
            ctx.prof_reset()
            t0 = time.perf_counter()
            for _ in range(calls):
                rows, _ = ctx.frame_blend(handles, tw, th, hist=hist)
            wall = (time.perf_counter() - t0) * 1e3 / calls
            ctx.sync()
            blend_ms, scopes = ctx.prof_get("blend")
            thumbs_ms, launches = ctx.prof_get("thumbs")
            ctx.prof_enable(False)
            assert scopes == calls and launches == calls, (scopes, launches, calls)
            return blend_ms / calls, thumbs_ms / calls, wall, rows

        def before(calls):
            """frame_thumbs to the host, then luma and rows in numpy -> wall ms per call, and the rows"""
            t0 = time.perf_counter()
            for _ in range(calls):
                thumbs = ctx.frame_thumbs(handles, tw, th)
                luma = np.stack([blend_ref.luma_of(t) for t in thumbs])
                rows = blend_ref.rows_of(np.concatenate([hist, luma]), first=len(hist), size_word=tw | th << 16)
            return (time.perf_counter() - t0) * 1e3 / calls, rows
        library(3); before(1)                                       # the uncounted pass
        k, t, wl, wb = [], [], [], []
        for _ in range(3):
            b_ms, t_ms, wall, rows = library(a.calls)
            before_ms, rows_before = before(max(2, a.calls // 5))
            assert np.array_equal(rows, rows_before), "the two routes disagree"
            k.append(b_ms); t.append(t_ms); wl.append(wall); wb.append(before_ms)
        km, tm, wlm, wbm = (stats(v)["median"] for v in (k, t, wl, wb))
        configs[name] = {
            "thumbnail": [tw, th], "source_bytes": n * h * w * 3, "bytes_touched_by_the_new_kernels": n * P * 3 + n * P * (1 + 4 * 3 + 2),
            "calls_per_window": a.calls, "blend_kernels_ms_per_call": stats(k), "frame_thumbs_k_ms_per_call": stats(t),
            "call_wall_ms": stats(wl), "route_before_wall_ms": stats(wb), "new_kernels_over_frame_thumbs_k": round(km / tm, 4),
            "new_kernels_no_longer_than_frame_thumbs_k": bool(km <= tm), "call_over_route_before": round(wlm / wbm, 4),
            "call_not_slower_than_route_before": bool(wlm <= wbm), "rows_equal": True,
        }
        del dev, handles, src
        ctx.unstage_all()
        torch.cuda.empty_cache()
    return {"bench": "blend: blend_luma_k + blend_measure_k behind frame_thumbs_k on %d resident frames, 32 planes of history" % n, "frames": n,
            "configurations": configs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--calls", type=int, default=100, help="frame_blend calls per timed window")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0)
    res = bench(ctx, torch, a)
    with open(os.path.join(a.out_dir, "blend_n64.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
