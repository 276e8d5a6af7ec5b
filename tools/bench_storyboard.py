"""Storyboard bench (csrc/board.hip; STORYBOARD.md), on an MI355X, in one process.

frame_thumbs_k on 64 frames resident in HBM, 1080p and 2160p, to 160 x 90 and to 320 x 180, output in device memory (no host copy in
the window).  Everything is warmed up first; then, alternating in the same run, (a) `calls` frame_thumbs calls, the kernel timed by the
library's own device events around each launch (family "thumbs") and summed -- enough calls for a window of tenths of a second -- and
(b) as many device-to-device copies of the same 64 frames' bytes, each between two device events.  The bar: the copy moves twice the
bytes the kernel does (it writes what it reads), so the kernel is not slower than the copy of its own input.  Per configuration: us per
frame, source bytes over kernel time, the ratio to the in-run copy, the share of the 6.29 TB/s a streaming read reaches on this chip.

Then the verb end to end on synthetic:1920x1080x1000 with its own shots: wall seconds, and the split between the library calls
(frame_thumbs, thumb_sheet) and everything else (making and staging the frames).

Writes one JSON object to --out (default profiles/storyboard_n64.json) and prints it.

    python tools/bench_storyboard.py [--frames 64] [--window 0.2] [--rounds 5] [--skip-verb]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
HBM_STREAM = 6.29e12            # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of kernel time per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="alternations of kernel window and copy window")
    ap.add_argument("--skip-verb", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "storyboard_n64.json"))
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    from pyannote_video_amd import cli
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0)
    n = a.frames
    med = lambda v: sorted(v)[len(v) // 2]          # noqa: E731
    configs = {}
    for name, (h, w) in (("1080p", (1080, 1920)), ("2160p", (2160, 3840))):
        src = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        torch.cuda.synchronize()
        dev = [ctx.wrap_torch(src[i]) for i in range(n)]
        handles = ctx.frame_handles(dev)
        source_bytes = n * h * w * 3
        for tw, th in ((160, 90), (320, 180)):
            out = torch.empty(n * th * tw * 3, dtype=torch.uint8, device="cuda")
            call = lambda: ctx.frame_thumbs(handles, tw, th, out_ptr=out.data_ptr())          # noqa: E731

            def kernel_ms(calls):
                ctx.prof_enable(True)
                ctx.prof_reset()
                for _ in range(calls):
                    call()
                ctx.sync()
                ms, launches = ctx.prof_get("thumbs")
                ctx.prof_enable(False)
                assert launches == calls, (launches, calls)
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
            for _ in range(3):                      # warm-up of both
                call()
            copy_ms(3)
            calls = max(10, int(a.window * 1e3 / max(kernel_ms(10), 1e-3)))
            k, c = [], []
            for _ in range(a.rounds):
                k.append(kernel_ms(calls))
                c.append(copy_ms(calls))
            km, cm = med(k), med(c)
            configs["%s_to_%dx%d" % (name, tw, th)] = {
                "source_bytes": source_bytes, "output_bytes": n * th * tw * 3, "calls_per_window": calls,
                "kernel_ms_per_call": [round(v, 5) for v in k], "copy_ms_per_call": [round(v, 5) for v in c],
                "kernel_us_per_frame": round(km * 1e3 / n, 3), "source_bytes_per_second": round(source_bytes / (km * 1e-3), 0),
                "kernel_over_copy": round(km / cm, 4), "kernel_not_slower_than_copy": bool(km <= cm),
                "share_of_hbm_stream_rate": round(source_bytes / (km * 1e-3) / HBM_STREAM, 4),
            }
        del dev, handles, src, dst
        ctx.unstage_all()
        torch.cuda.empty_cache()
    result = {"bench": "storyboard: frame_thumbs_k on %d resident frames, output in device memory" % n, "frames": n, "rounds": a.rounds,
              "hbm_stream_bytes_per_second": HBM_STREAM, "configurations": configs}
    if not a.skip_verb:
        spec, fps = "synthetic:1920x1080x1000", 25.0
        video = cli.open_video(spec, fps)
        spent = {"frame_thumbs": 0.0, "thumb_sheet": 0.0}

        class Timed(object):
            """the context, with the two library calls of the verb timed by the host clock (both end in a device synchronise)"""

            def __getattr__(self, name):
                f = getattr(ctx, name)
                if name not in spent:
                    return f

                def timed(*args, **kw):
                    t0 = time.perf_counter()
                    r = f(*args, **kw)
                    spent[name] += time.perf_counter() - t0
                    return r
                return timed
        d = tempfile.mkdtemp()
        sp = os.path.join(d, "shot.json")
        with open(sp, "w") as f:
            json.dump([[s0, s1] for s0, s1 in video.shots()], f)
        runs = []
        for _ in range(2):                          # the second run is the warm one
            for k in spent:
                spent[k] = 0.0
            t0 = time.perf_counter()
            res = cli.storyboard(video, sp, os.path.join(d, "board.ppm"), per=8, ctx=Timed())
            wall = time.perf_counter() - t0
            runs.append({"wall_seconds": round(wall, 4), "library_seconds": dict((k, round(v, 5)) for k, v in spent.items()),
                         "reading_and_host_seconds": round(wall - sum(spent.values()), 4), "result": res})
        result["verb_end_to_end"] = {"video": spec, "per": 8, "runs": runs}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
