"""Tube bench (csrc/tube.hip; TUBE.md), on 1080p frames resident in HBM, in one process: pvf_frame_crops at n
crops (default 4096), 8 per frame, L / 16 drawn from 150 .. 500, at S = 224 and S = 96 in both layouts.  Per configuration: ms per
call by the host clock (output in host memory: the call ends when the last round's copy has arrived), the kernel alone from the
library's own event timing (family "tube"), the algorithmic bytes (window bytes in plus picture bytes out) and the share of the 8 TB/s
HBM peak the kernel time makes of them.  Two yardsticks from code older than the verb, timed in the same process: (a) the "chip"
family of pvf_face_chips for as many faces on the same frames, (b) the device-to-host copy of the call's own output alone.
Writes one JSON object to --out (default profiles/tube_n4096.json) and prints it.

    python tools/bench_tube.py [--crops 4096] [--frames 64] [--repeats 5]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tube_n4096.json"))
    a = ap.parse_args()
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
    for S in (224, 96):
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
        "bench": "tube: %d crops of 1080p frames, %d per frame, L / 16 in 150 .. 500" % (n, PER_FRAME), "crops": n, "frames": a.frames,
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
