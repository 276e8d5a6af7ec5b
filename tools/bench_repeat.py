"""Repeat bench (csrc/repeat.hip; REPEAT.md), on an MI355X, in one process.

Prints: pvf_frame_prints on 64 frames resident in HBM, 1080p and 2160p, output in device memory.  After one uncounted pair, three
alternating windows of (a) frame_prints calls, the two kernels timed by the library's own device events (family "prints"), and (b) as
many device-to-device copies of the same frames, each between two device events; and, for the design decision, (c) frame_thumbs_k at
9 x 9 on the same frames (family "thumbs"), which a two-kernel variant would have called for the grid.  The bar is section 21's: the
kernel is not slower than the copy of its own input.  Median with lowest and highest.

Runs: pvf_print_runs on random prints with 20 planted runs, NA = NB = 40 000 (two films) and a self-join at NA = 10^6 (a season): the
kernel time from the library's device events (family "runs"), the call's wall time, the same tables compared through numpy on the host
in this process (in full at the first shape, a stated sample of rows at the second; the runs must agree exactly where both were
computed), and the share of the vector-issue bound: --valu vector instructions per cell (counted in the compiler's output of the inner
loop) x cells / (256 CUs x 4 SIMDs x 64 lanes / 2 cycles an instruction x the clock).

Writes profiles/repeat_prints.json and profiles/repeat_runs.json and prints both.

    python tools/bench_repeat.py [--frames 64] [--window 0.1] [--valu 13] [--nops 4] [--clock 2.4e9] [--skip-season]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
HBM_STREAM = 6.29e12            # bytes per second (section 21)
TAU, MIN_LEN, PLANT_BITS, N_PLANTS = 10, 8, 6, 20


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 5), "lowest": round(s[0], 5), "highest": round(s[-1], 5)}


def bench_prints(ctx, torch, a):
    n, configs = a.frames, {}
    for name, (h, w) in (("1080p", (1080, 1920)), ("2160p", (2160, 3840))):
        src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        out = torch.empty(n * 4, dtype=torch.int64, device="cuda")
        grid = torch.empty(n * 9 * 9 * 3, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        dev = [ctx.wrap_torch(src[i]) for i in range(n)]
        handles = ctx.frame_handles(dev)
        source_bytes = n * h * w * 3

        def family_ms(call, family, calls, launches_per_call=1):
            ctx.prof_enable(True)
            ctx.prof_reset()
            for _ in range(calls):
                call()
            ctx.sync()
            ms, launches = ctx.prof_get(family)
            ctx.prof_enable(False)
            assert launches == calls * launches_per_call, (family, launches, calls)
            return ms / calls

        def copy_ms(calls):
            total = 0.0
            for _ in range(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(src)
                e1.record()
                e1.synchronize()
                total += e0.elapsed_time(e1)
            return total / calls
        prints = lambda: ctx.frame_prints(handles, out_ptr=out.data_ptr())                  # noqa: E731
        thumbs = lambda: ctx.frame_thumbs(handles, 9, 9, out_ptr=grid.data_ptr())           # noqa: E731
        calls = max(5, int(a.window * 1e3 / max(family_ms(prints, "prints", 5), 1e-3)))
        family_ms(prints, "prints", calls); copy_ms(calls); family_ms(thumbs, "thumbs", 3)  # the uncounted pair
        k, c, t = [], [], []
        for _ in range(3):
            k.append(family_ms(prints, "prints", calls))
            c.append(copy_ms(calls))
            t.append(family_ms(thumbs, "thumbs", max(3, calls // 4)))
        km, cm = stats(k)["median"], stats(c)["median"]
        configs[name] = {
            "source_bytes": source_bytes, "calls_per_window": calls, "prints_ms_per_call": stats(k), "copy_ms_per_call": stats(c),
            "frame_thumbs_9x9_ms_per_call": stats(t), "prints_us_per_frame": round(km * 1e3 / n, 3),
            "source_bytes_per_second": round(source_bytes / (km * 1e-3), 0), "prints_over_copy": round(km / cm, 4),
            "prints_not_slower_than_copy": bool(km <= cm), "prints_over_frame_thumbs_9x9": round(km / stats(t)["median"], 4),
            "share_of_hbm_stream_rate": round(source_bytes / (km * 1e-3) / HBM_STREAM, 4),
        }
        del dev, handles, src, dst
        ctx.unstage_all()
        torch.cuda.empty_cache()
    return {"bench": "prints: frame_print_k + print_finish_k on %d resident frames, output in device memory" % n, "frames": n,
            "hbm_stream_bytes_per_second": HBM_STREAM, "configurations": configs}


def tables(NA, NB, self_mode, seed):
    """random prints with N_PLANTS planted copies of PLANT_BITS flipped bits a row -> (A, B or None, the planted runs)"""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 1 << 64, (NA, 2), dtype=np.uint64)
    B = A if self_mode else rng.integers(0, 1 << 64, (NB, 2), dtype=np.uint64)
    plants = []
    slot_a, slot_b = NA // (2 * N_PLANTS), NB // (2 * N_PLANTS)
    for k in range(N_PLANTS):
        n = 25 + 37 * k                                                        # 25 .. 728 frames
        i = k * slot_a + int(rng.integers(0, max(slot_a - n, 1)))               # sources in the first half, copies in the second
        j = (NB // 2 if self_mode else 0) + k * slot_b + int(rng.integers(0, max(slot_b - n, 1)))
        rows = A[i:i + n].copy()
        for r in range(n):
            for b in rng.choice(128, PLANT_BITS, replace=False):
                rows[r, b // 64] ^= np.uint64(1 << (int(b) % 64))
        B[j:j + n] = rows
        plants.append((i, j, n))
    return A, (None if self_mode else B), sorted(plants, key=lambda r: (r[1] - r[0], r[0]))


def host_matches(A, B, rows, lo_gap=None):
    """the matching cells (i, j) of the given rows of A against all of B through numpy, 32 M cells at a time: j >= i + lo_gap in self mode"""
    hits, chunk = [], max(1, (32 << 20) // len(B))
    for c0 in range(0, len(rows), chunk):
        r = rows[c0:c0 + chunk]
        d = np.bitwise_count(A[r, None, 0] ^ B[None, :, 0]).astype(np.uint8)
        d += np.bitwise_count(A[r, None, 1] ^ B[None, :, 1])
        ii, jj = np.nonzero(d <= TAU)
        ii = r[ii]
        if lo_gap is not None:
            keep = jj >= ii + lo_gap
            ii, jj = ii[keep], jj[keep]
        hits.append(np.stack([ii, jj], 1))
    return np.concatenate(hits) if hits else np.zeros((0, 2), np.int64)


def runs_of_cells(cells):
    """maximal runs (i, j, len) of a set of cells, ordered by (j - i, i)"""
    if not len(cells):
        return []
    d = cells[:, 1] - cells[:, 0]
    order = np.lexsort((cells[:, 0], d))
    i, d = cells[order, 0], d[order]
    new = np.ones(len(i), bool)
    new[1:] = (d[1:] != d[:-1]) | (i[1:] != i[:-1] + 1)
    starts = np.nonzero(new)[0]
    ends = np.append(starts[1:], len(i))
    return [(int(i[s]), int(i[s] + d[s]), int(e - s)) for s, e in zip(starts, ends)]


def bench_runs(ctx, a):
    issue_rate = 256 * 4 * 64 / 2.0 * a.clock                                   # lane-instructions per second
    shapes = {}
    todo = [("two_films", 40000, 40000, False)] + ([] if a.skip_season else [("season_self_join", 1000000, 1000000, True)])
    for name, NA, NB, self_mode in todo:
        A, B, plants = tables(NA, NB, self_mode, 7)
        ua = np.ones(NA, np.uint8)
        ub = None if self_mode else np.ones(NB, np.uint8)
        call = lambda: ctx.print_runs(A, ua, B, ub, tau=TAU, min_len=MIN_LEN, min_gap=1)     # noqa: E731
        found = call()                                                          # warm-up; the result
        k, wall = [], []
        for _ in range(3):
            ctx.prof_enable(True)
            ctx.prof_reset()
            t0 = time.perf_counter()
            again = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms, launches = ctx.prof_get("runs")
            ctx.prof_enable(False)
            assert launches == 1 and np.array_equal(again, found)
            k.append(ms)
        cells = NA * (NA - 1) // 2 if self_mode else NA * NB
        # the host route: every row at the first shape, a sample at the second (the planted rows' first 16 each, and 704 random rows)
        t0 = time.perf_counter()
        if self_mode:
            rng = np.random.default_rng(11)
            rows = np.unique(np.concatenate([np.arange(i, i + 16) for i, _, _ in plants] + [rng.integers(0, NA, 704)]))
            hit = host_matches(A, A, rows, lo_gap=1)
            sampled = set(rows.tolist())
            got = set((i + t, j + t) for i, j, n in found.tolist() for t in range(n) if i + t in sampled)
            host_cells = len(rows) * NA
            agree = got == set(map(tuple, hit.tolist()))
        else:
            rows = np.arange(NA)
            hit = host_matches(A, B, rows)
            host_runs = [r for r in runs_of_cells(hit) if r[2] >= MIN_LEN]
            host_cells = cells
            agree = host_runs == [tuple(r) for r in found.tolist()]
        host_s = time.perf_counter() - t0
        km = stats(k)["median"]
        shapes[name] = {
            "NA": NA, "NB": NB, "self_mode": self_mode, "tau": TAU, "min_len": MIN_LEN, "planted": len(plants), "runs_found": int(len(found)),
            "runs_are_the_planted_ones": bool([tuple(r) for r in found.tolist()] == plants), "cells": cells,
            "kernel_ms": stats(k), "call_wall_ms": stats(wall), "cells_per_second": round(cells / (km * 1e-3), 0),
            "host_numpy": {"rows": int(len(rows)), "cells": int(host_cells), "seconds": round(host_s, 3),
                           "cells_per_second": round(host_cells / host_s, 0), "agrees_exactly": bool(agree)},
            "vector_issue_bound": {"valu_per_cell": a.valu, "s_nop_per_cell": a.nops, "clock_hz": a.clock,
                                   "lane_instructions_per_second": issue_rate, "bound_ms": round(cells * a.valu / issue_rate * 1e3, 4),
                                   "share_reached": round(cells * a.valu / issue_rate * 1e3 / km, 4)},
        }
    return {"bench": "runs: print_runs_k, random prints with %d planted runs of %d flipped bits" % (N_PLANTS, PLANT_BITS), "shapes": shapes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--window", type=float, default=0.1, help="seconds of kernel time per timed window of the prints")
    ap.add_argument("--valu", type=int, default=13, help="vector instructions per cell in print_runs_k's inner loop (from the compiler's output)")
    ap.add_argument("--nops", type=int, default=4, help="s_nop per cell beside them")
    ap.add_argument("--clock", type=float, default=2.4e9)
    ap.add_argument("--skip-season", action="store_true")
    ap.add_argument("--skip-prints", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0)
    if not a.skip_prints:
        res = bench_prints(ctx, torch, a)
        with open(os.path.join(a.out_dir, "repeat_prints.json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
    res = bench_runs(ctx, a)
    with open(os.path.join(a.out_dir, "repeat_runs.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
