"""Tube bench (csrc/tube.hip; TUBE.md), on 1080p frames resident in HBM, in one process: pvf_frame_crops at n
crops (default 4096), 8 per frame, L / 16 drawn from 150 .. 500, at S = 224 and S = 96 in both layouts.  Per configuration: ms per
call by the host clock (output in host memory: the call ends when the last round's copy has arrived), the kernel alone from the
library's own event timing (family "tube"), the algorithmic bytes (window bytes in plus picture bytes out) and the share of the 8 TB/s
HBM peak the kernel time makes of them.  Two yardsticks from code older than the verb, timed in the same process: (a) the "chip"
family of pvf_face_chips for as many faces on the same frames, (b) the device-to-host copy of the call's own output alone.
Writes one JSON object to --out (default profiles/tube_n4096.json) and prints it.

--align: the aligned leg on the same windows, made oriented windows (tube.quantise_oriented) with rolls spread
over +-30 degrees and once more at 0 degrees: pvf_frame_warps' kernel beside pvf_frame_crops' on the same windows, the copy of the same
pictures to the host and the chip step of as many faces, all in this run.  Writes profiles/tube_align_n4096.json.

    python tools/bench_tube.py [--crops 4096] [--frames 64] [--repeats 5] [--align]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_tube.py --kernel-only 10

--kernel-only N: nothing but N frame_crops calls into device memory (S = 224, RGB), for a kernel trace of its own."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12               # bytes per second
PER_FRAME = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=64, help="distinct frames in HBM; crops use them in turn, 8 to a frame")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="calls per timed window")
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N")
    ap.add_argument("--align", action="store_true", help="the aligned leg: warp_k beside crop_k, the copy and the chip step")
    ap.add_argument("--out", default=None, help="default: profiles/tube_n4096.json, with --align profiles/tube_align_n4096.json")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "tube_align_n4096.json" if a.align else "tube_n4096.json")
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from bench_faces import H, W, face_points
    from pyannote_video_amd import synth
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0)
    video = synth.SyntheticVideo(width=W, height=H, n_frames=a.frames, n_shots=4, faces=8, seed=20260925, frame_rate=25.0)
    frames_t = video.frames_torch(torch.device("cuda", 0))
    torch.cuda.synchronize()
    dev = [ctx.wrap_torch(frames_t[i]) for i in range(a.frames)]
    n = a.crops
    handles = ctx.frame_handles([dev[(i // PER_FRAME) % a.frames] for i in range(n)])
    rng = np.random.RandomState(20261019)
    side = rng.randint(150, 501, n)
    win = np.stack([rng.randint(0, 16 * (W - side) + 1), rng.randint(0, 16 * (H - side) + 1), 16 * side + rng.randint(0, 16, n)], 1).astype(np.int32)
    window_bytes = int((3 * (side + 1).astype(np.int64) ** 2).sum())

    if a.kernel_only:
        buf = torch.empty(n * 224 * 224 * 3, dtype=torch.uint8, device="cuda")
        for _ in range(a.kernel_only):
            ctx.frame_crops(handles, win, 224, out_ptr=buf.data_ptr())
        print(json.dumps({"bench": "frame_crops kernel alone", "calls": a.kernel_only, "crops": n}))
        return

    def window(call):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.rounds):
            call()
        ctx.sync()
        return (time.perf_counter() - t0) / a.rounds * 1e3

    def family(call, name):
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(a.rounds):
            call()
        ctx.sync()
        v = round(ctx.prof_get(name)[0] / a.rounds, 5)
        ctx.prof_enable(False)
        return v

    med = lambda v: sorted(v)[len(v) // 2]
    # (a) the existing per-face resampling step: the chips of as many faces on the same frames
    pts = face_points(n)
    # (through pvf_face_quality, which runs pvf_face_chips' chip step -- the family "chip" -- without needing an embedder's file)
    chips = lambda: ctx.face_quality(handles, pts)
    chips()
    chip_ms = sorted(family(chips, "chip") for _ in range(a.repeats))
    configs = {}
    if a.align:
        import math
        from pyannote_video_amd import tube
        rolls = rng.uniform(-30.0, 30.0, n)

        def oriented(S, degrees):
            return np.array([tube.quantise_oriented((x + L / 2.0) / 16.0, (y + L / 2.0) / 16.0, L / 16.0, math.cos(math.radians(d)),
                                                    math.sin(math.radians(d)), S) for (x, y, L), d in zip(win.tolist(), degrees)], np.int32)
        for S in (224, 96):
            for layout in ("rgb", "yuv420"):
                out_bytes = n * (S * S * 3 if layout == "rgb" else S * S + 2 * ((S + 1) // 2) ** 2)
                dbuf = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
                legs = {"rolls_within_30_degrees": oriented(S, rolls), "roll_0": oriented(S, np.zeros(n))}
                calls = dict((k, (lambda w: (lambda: ctx.frame_warps(handles, w, S, layout, out_ptr=dbuf.data_ptr())))(w)) for k, w in legs.items())
                calls["crop_k_same_windows"] = lambda: ctx.frame_crops(handles, win, S, layout, out_ptr=dbuf.data_ptr())
                host = lambda: ctx.frame_warps(handles, legs["rolls_within_30_degrees"], S, layout)
                for c in list(calls.values()) + [host]:
                    c()                                             # warm-up
                kern = dict((k, sorted(family(c, "tube") for _ in range(a.repeats))) for k, c in calls.items())
                ms_host = [round(window(host), 4) for _ in range(a.repeats)]

                def copy():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    dbuf.cpu()
                    return (time.perf_counter() - t0) * 1e3
                copy()
                copy_ms = sorted(round(copy(), 4) for _ in range(a.repeats))
                k = med(kern["rolls_within_30_degrees"])
                configs["S%d_%s" % (S, layout)] = {
                    "picture_bytes_out": out_bytes, "window_bytes_in": window_bytes,
                    "sub_samples_per_axis": dict((str(int(v)), int((legs["rolls_within_30_degrees"][:, 4] == v).sum()))
                                                 for v in np.unique(legs["rolls_within_30_degrees"][:, 4])),
                    "kernel_ms_per_call_to_device": kern, "ms_per_call_host_clock_to_host": ms_host,
                    "copy_of_the_output_to_host_ms": copy_ms,
                    "warp_over_crop": round(k / med(kern["crop_k_same_windows"]), 4), "warp_over_copy": round(k / med(copy_ms), 4),
                    "warp_over_chip": round(k / med(chip_ms), 4), "warp_below_copy": bool(k < med(copy_ms)),
                }
    for S in (() if a.align else (224, 96)):
        for layout in ("rgb", "yuv420"):
            out_bytes = n * (S * S * 3 if layout == "rgb" else S * S + 2 * ((S + 1) // 2) ** 2)
            dbuf = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
            host = lambda: ctx.frame_crops(handles, win, S, layout)
            on_dev = lambda: ctx.frame_crops(handles, win, S, layout, out_ptr=dbuf.data_ptr())
            host(); on_dev()                                    # warm-up
            ms_host = [round(window(host), 4) for _ in range(a.repeats)]
            ms_dev = [round(window(on_dev), 4) for _ in range(a.repeats)]
            kern = sorted(family(on_dev, "tube") for _ in range(a.repeats))
            kern_host = sorted(family(host, "tube") for _ in range(a.repeats))
            # (b) the device-to-host copy of the call's own output alone, into pageable host memory as the call's is
            dview = dbuf.cpu

            def copy():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = dview()
                return (time.perf_counter() - t0) * 1e3, got
            copy()
            copy_ms = sorted(round(copy()[0], 4) for _ in range(a.repeats))
            k = med(kern)
            configs["S%d_%s" % (S, layout)] = {
                "picture_bytes_out": out_bytes, "window_bytes_in": window_bytes,
                "ms_per_call_host_clock": {"to_host": ms_host, "to_device": ms_dev},
                "kernel_ms_per_call": {"to_device": kern, "to_host": kern_host},
                "share_of_hbm_peak": round((window_bytes + out_bytes) / (k * 1e-3) / HBM_PEAK, 4),
                "copy_of_the_output_to_host_ms": copy_ms,
                "kernel_over_copy": round(k / med(copy_ms), 4), "kernel_over_chip": round(k / (med(chip_ms) * 1.0), 4),
                "kernel_below_copy": bool(k < med(copy_ms)), "kernel_not_slower_than_chip": bool(k <= med(chip_ms)),
            }
    line = {
        "bench": ("tube --align: %d oriented windows" if a.align else "tube: %d crops") % n + " of 1080p frames, %d per frame, L / 16 in 150 .. 500" % PER_FRAME, "crops": n, "frames": a.frames,
        "repeats": a.repeats, "calls_per_window": a.rounds, "hbm_peak_bytes_per_second": HBM_PEAK,
        "chip_family_ms_for_as_many_faces": chip_ms, "configurations": configs,
    }
    text = json.dumps(line, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(line))
    for f in dev:
        f.release()
    ctx.close()


if __name__ == "__main__":
    main()
