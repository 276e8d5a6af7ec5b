"""Text bench (csrc/text.hip; CAPTION.md), on an MI355X, in one process.

pvf_frame_text on 64 frames resident in HBM, 1080p and 2160p, default parameters.  After an uncounted pass, five alternations of
  (a) frame_text calls: text_cells_k by the library's own device events (family "text"), text_head_k by its own (family "text_head"),
      and the calls' wall time, rows to the host included;
  (b) as many device-to-device copies of the same 64 frames' bytes, each between two device events: the yardstick `storyboard` and
      `fingerprint` use.  The copy reads and writes every byte, a read-once kernel moves half of that, so the bar is that text_cells_k
      is not slower than the copy of its own input.
Once per size, the route a user had before: the frames to the host and tests/text_ref.py's numpy on them, wall time; the rows of both
routes must be equal.  Median with lowest and highest of the five, and the ratios.

Writes profiles/text_n64.json and prints it.

    python tools/bench_text.py [--frames 64] [--rounds 5] [--calls 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
sys.path.insert(0, ROOT)
HBM_STREAM = 6.29e12                       # bytes a second a streaming read reaches on this chip (tools/bw_probe.py)


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 5), "lowest": round(s[0], 5), "highest": round(s[-1], 5)}


def bench(ctx, torch, a):
    from tests import text_ref
    n, configs = a.frames, {}
    for name, (h, w) in (("1080p", (1080, 1920)), ("2160p", (2160, 3840))):
        # blocks of 4 x 4 that drift a pixel a frame over a still lower third with bars: strokes, moved pixels and persistent strokes
        g = torch.Generator(device="cuda").manual_seed(h)
        coarse = torch.randint(0, 256, (h // 4, (w + n) // 4 + 1, 3), dtype=torch.uint8, device="cuda", generator=g)
        wide = coarse.repeat_interleave(4, 0).repeat_interleave(4, 1)
        src = torch.stack([wide[:, i:i + w] for i in range(n)]).contiguous()
        bars = (((torch.arange(w, device="cuda") >> 1) & 1) * 200 + 20).to(torch.uint8)
        src[:, 2 * h // 3:, :, :] = bars[None, None, :, None]
        dst = torch.empty_like(src)
        torch.cuda.synchronize()
        dev = [ctx.wrap_torch(src[i]) for i in range(n)]
        handles = ctx.frame_handles(dev)
        source_bytes = n * h * w * 3

        def library(calls):
            ctx.prof_enable(True)
            ctx.prof_reset()
            t0 = time.perf_counter()
            for _ in range(calls):
                rows, _ = ctx.frame_text(handles, size=(w, h))
            wall = (time.perf_counter() - t0) * 1e3 / calls
            ctx.sync()
            cells_ms, launches = ctx.prof_get("text")
            head_ms, _ = ctx.prof_get("text_head")
            ctx.prof_enable(False)
            assert launches == calls, (launches, calls)
            return cells_ms / calls, head_ms / calls, wall, rows

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
        library(3); copy_ms(3)                                       # the uncounted pass
        k, hd, wl, c = [], [], [], []
        for _ in range(a.rounds):
            cells_ms, head_ms, wall, rows = library(a.calls)
            k.append(cells_ms); hd.append(head_ms); wl.append(wall)
            c.append(copy_ms(a.calls))
        t0 = time.perf_counter()
        host = [src[i].cpu().numpy() for i in range(n)]
        fetch_ms = (time.perf_counter() - t0) * 1e3
        rows_before, _ = text_ref.rows_of(host)
        before_ms = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(rows, rows_before), "the two routes disagree"
        km, cm, wm = stats(k)["median"], stats(c)["median"], stats(wl)["median"]
        configs[name] = {
            "source_bytes": source_bytes, "row_bytes_per_frame": int(rows.shape[1]) * 4, "calls_per_round": a.calls,
            "set_bits_per_frame": round(float(rows[1:, 5].mean()), 1), "stroke_pixels_per_frame": round(float(rows[:, 2].mean()), 1),
            "text_cells_k_ms_per_call": stats(k), "text_head_k_ms_per_call": stats(hd), "call_wall_ms": stats(wl),
            "device_to_device_copy_ms": stats(c), "route_before_wall_ms_once": round(before_ms, 1), "of_which_frames_to_the_host_ms": round(fetch_ms, 1),
            "text_cells_k_us_per_frame": round(km * 1e3 / n, 3), "source_bytes_per_second": round(source_bytes / (km * 1e-3), 0),
            "share_of_hbm_stream_rate": round(source_bytes / (km * 1e-3) / HBM_STREAM, 4),
            "text_cells_k_over_copy": round(km / cm, 4), "text_cells_k_not_slower_than_copy": bool(km <= cm),
            "call_over_route_before": round(wm / before_ms, 6), "rows_equal": True,
        }
        del dev, handles, src, dst, wide, coarse
        ctx.unstage_all()
        torch.cuda.empty_cache()
    return {"bench": "text: text_cells_k on %d resident frames against the device-to-device copy of the same frames" % n, "frames": n,
            "rounds": a.rounds, "hbm_stream_bytes_per_second": HBM_STREAM, "configurations": configs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the call window and the copy window")
    ap.add_argument("--calls", type=int, default=20, help="calls per window")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0)
    res = bench(ctx, torch, a)
    with open(os.path.join(a.out_dir, "text_n64.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
