"""Clothes bench (csrc/clothes.hip; CLOTHES.md), on an MI355X, in one process.

pvf_frame_hist on 4096 torso windows -- faces of 150 .. 500 pixels, the tube bench's boxes, 64 a frame, clothes.torso's defaults, clipped
by the frame -- of 64 frames resident in HBM, 1080p and 2160p, with noise and with one colour everywhere (every lane of a wave adds to
one bin: the LDS-contention worst case), 64 groups, 2 bands, the result left on the device.  After an uncounted pass, five alternations of
  (a) frame_hist calls: box_hist_k by the library's own device events (family "hist"), the zeroing by its own (family "hist_zero"), and
      the calls' wall time, piece list made and uploaded included;
  (b) crop_k at S = 96 on the same windows (family "tube"; it reads the same source pixels), pictures left on the device;
  (c) as many device-to-device copies of as many bytes as the clipped windows hold, each between two device events.  The copy reads and
      writes every byte, a read-once kernel moves half of that, so the bar is that box_hist_k is not slower than the copy of its input.
Once per size, on noise, the route a user had before: the frames to the host and tests/clothes_ref.py's numpy on them, wall time; the
results of both routes must be equal.  Median with lowest and highest of the five, and the ratios.

Writes profiles/clothes_n4096.json and prints it.

    python tools/bench_clothes.py [--windows 4096] [--frames 64] [--rounds 5] [--calls 10]"""
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
GROUPS, BANDS, CROP_S = 64, 2, 96
MID = (90, 140, 200)


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 5), "lowest": round(s[0], 5), "highest": round(s[-1], 5)}


def bench(ctx, torch, a):
    from pyannote_video_amd import clothes
    from tests import clothes_ref
    n, nf, configs = a.windows, a.frames, {}
    for name, (h, w) in (("1080p", (1080, 1920)), ("2160p", (2160, 3840))):
        rng = np.random.RandomState(20261019)
        side = rng.randint(150, 501, n)
        left, top = rng.randint(0, w - side + 1), rng.randint(0, h - side + 1)
        wins = np.array([clothes.torso((l, t, l + s, t + s)) for l, t, s in zip(left, top, side)], np.int32)
        clip = np.stack([np.maximum(wins[:, 0], 0), np.maximum(wins[:, 1], 0), np.minimum(wins[:, 2], w), np.minimum(wins[:, 3], h)], 1).astype(np.int64)
        pixels = np.maximum(clip[:, 2] - clip[:, 0], 0) * np.maximum(clip[:, 3] - clip[:, 1], 0)
        window_bytes = int(3 * pixels.sum())
        # the same windows as squares for crop_k: (X0, Y0, L) in sixteenths of a pixel, L the window's width (its height is the same: 2 x the face)
        crops = np.stack([16 * wins[:, 0], 16 * wins[:, 1], 16 * (wins[:, 2] - wins[:, 0])], 1).astype(np.int32)
        group = (np.arange(n) % GROUPS).astype(np.int32)
        out = torch.zeros((GROUPS, BANDS, 256), dtype=torch.int32, device="cuda")
        pictures = torch.empty(n * CROP_S * CROP_S * 3, dtype=torch.uint8, device="cuda")
        copy_src = torch.empty(window_bytes, dtype=torch.uint8, device="cuda")
        copy_dst = torch.empty_like(copy_src)
        for content in ("noise", "constant"):
            if content == "noise":
                g = torch.Generator(device="cuda").manual_seed(h)
                src = torch.randint(0, 256, (nf, h, w, 3), dtype=torch.uint8, device="cuda", generator=g)
            else:
                src = torch.tensor(MID, dtype=torch.uint8, device="cuda").expand(nf, h, w, 3).contiguous()
            torch.cuda.synchronize()
            dev = [ctx.wrap_torch(src[i]) for i in range(nf)]
            handles = ctx.frame_handles([dev[(i * nf) // n] for i in range(n)])

            def library(calls):
                ctx.prof_enable(True)
                ctx.prof_reset()
                t0 = time.perf_counter()
                for _ in range(calls):
                    ctx.frame_hist(handles, wins, group, GROUPS, bands=BANDS, out_ptr=out.data_ptr())
                wall = (time.perf_counter() - t0) * 1e3 / calls
                ctx.sync()
                hist_ms, launches = ctx.prof_get("hist")
                zero_ms, _ = ctx.prof_get("hist_zero")
                ctx.prof_enable(False)
                return hist_ms / calls, zero_ms / calls, wall, launches // calls

            def crop_ms(calls):
                ctx.prof_enable(True)
                ctx.prof_reset()
                for _ in range(calls):
                    ctx.frame_crops(handles, crops, CROP_S, out_ptr=pictures.data_ptr())
                ctx.sync()
                ms = ctx.prof_get("tube")[0] / calls
                ctx.prof_enable(False)
                return ms

            def copy_ms(calls):
                total = 0.0
                for _ in range(calls):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    copy_dst.copy_(copy_src)
                    e1.record()
                    e1.synchronize()
                    total += e0.elapsed_time(e1)
                return total / calls
            library(2); crop_ms(2); copy_ms(2)                           # the uncounted pass
            k, z, wl, cr, cp = [], [], [], [], []
            for _ in range(a.rounds):
                hist_ms, zero_ms, wall, launches = library(a.calls)
                k.append(hist_ms); z.append(zero_ms); wl.append(wall)
                cr.append(crop_ms(a.calls))
                cp.append(copy_ms(a.calls))
            got = out.cpu().numpy().view(np.uint32)
            assert int(got.sum()) == int(pixels.sum()), "the counts do not add up to the clipped windows"
            km, cm, rm, wm = stats(k)["median"], stats(cp)["median"], stats(cr)["median"], stats(wl)["median"]
            res = {
                "windows": n, "frames": nf, "groups": GROUPS, "bands": BANDS, "clipped_window_bytes": window_bytes, "calls_per_round": a.calls,
                "kernel_launches_per_call": int(launches),
                "box_hist_k_ms_per_call": stats(k), "hist_zero_k_ms_per_call": stats(z), "call_wall_ms": stats(wl),
                "crop_k_s96_ms_per_call": stats(cr), "device_to_device_copy_ms": stats(cp),
                "window_bytes_per_second": round(window_bytes / (km * 1e-3), 0), "share_of_hbm_stream_rate": round(window_bytes / (km * 1e-3) / HBM_STREAM, 4),
                "box_hist_k_over_copy": round(km / cm, 4), "box_hist_k_not_slower_than_copy": bool(km <= cm),
                "box_hist_k_over_crop_k": round(km / rm, 4), "box_hist_k_not_slower_than_crop_k": bool(km <= rm),
            }
            if content == "noise":
                t0 = time.perf_counter()
                host = [src[i].cpu().numpy() for i in range(nf)]
                fetch_ms = (time.perf_counter() - t0) * 1e3
                known = dict((id(f), clothes_ref.bins_of(f).astype(np.uint8)) for f in host)
                before = clothes_ref.hist_of([host[(i * nf) // n] for i in range(n)], wins, group, GROUPS, BANDS, known=known)
                before_ms = (time.perf_counter() - t0) * 1e3
                assert np.array_equal(got, before), "the two routes disagree"
                res.update({"route_before_wall_ms_once": round(before_ms, 1), "of_which_frames_to_the_host_ms": round(fetch_ms, 1),
                            "call_over_route_before": round(wm / before_ms, 6), "results_equal": True})
                del host, known, before
            configs["%s_%s" % (name, content)] = res
            print("%s %s: box_hist_k %.4f ms, copy %.4f ms, crop_k %.4f ms" % (name, content, km, cm, rm), file=sys.stderr, flush=True)
            del dev, handles, src
            ctx.unstage_all()
            torch.cuda.empty_cache()
    return {"bench": "clothes: box_hist_k on %d torso windows of %d resident frames against crop_k on the same windows and the device-to-device "
                     "copy of as many bytes" % (n, nf), "rounds": a.rounds, "hbm_stream_bytes_per_second": HBM_STREAM, "configurations": configs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the call window, the crop window and the copy window")
    ap.add_argument("--calls", type=int, default=10, help="calls per window")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0)
    res = bench(ctx, torch, a)
    with open(os.path.join(a.out_dir, "clothes_n%d.json" % a.windows), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
