"""Redaction bench: 1080p frames resident in HBM redacted at source size into planar YUV 4:2:0 (csrc/render.hip: redact_means_k in
front of render_k's REDACT instantiation), in one process:
  (a) the batch form (pvf_render_batch into device memory), frames/s at 3 and at 40 faces per frame in each of the three modes
      (a face = one elliptical redaction of a padded box, 8 cells along its longer side, as build_redaction_plan makes them);
  (b) the two kernels alone, ms per frame from the library's own event timing (families "redact_means" and "render"), beside the
      algorithmic bytes per frame computed from the shapes and the share of HBM bandwidth they come to:
        means:  3 bytes per pixel of every redaction's box inside the frame (identity resize: each source byte once) + 4 per cell written
        render: 3 bytes per source pixel + 1.5 bytes per output pixel + 32 per primitive + 4 per cell read
      `fill` has no table: its means figures are absent.
Timed windows hold --rounds passes over the resident frames.  One JSON line.

    python tools/bench_redact.py [--frames 64] [--repeats 3]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_redact.py --kernel-only 20 [--faces 40] [--mode mosaic]

--kernel-only N: nothing but N passes of batch calls in one mode, for a kernel trace of its own."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
HBM_ACHIEVABLE_TBPS = 6.3       # what a float4 copy reaches on an MI355X (of 8 TB/s nominal)
W, H = 1920, 1080
MODES = ("mosaic", "smooth", "fill")


def face_lists(n_frames, faces, mode, seed=1):
    """per-frame lists of the shape build_redaction_plan makes: one padded elliptical redaction per face"""
    import numpy as np
    from pyannote_video_amd import render
    rng = np.random.RandomState(seed)
    flags = render.REDACT_MODES[mode] | render.REDACT_ELLIPSE
    out = []
    for _ in range(n_frames):
        prims = []
        for _ in range(faces):
            s = int(rng.randint(80, 300))
            l, t = int(rng.randint(0, W - s)), int(rng.randint(0, H - s))
            box = render.redaction_box((l, t, l + s, t + s * 5 // 4), 25)
            prims.append((render.PRIM_REDACT,) + box + ((0, 0, 0), render.redaction_cell(box, 8), flags))
        out.append(prims)
    return out


def algorithmic_bytes(lists):
    """(means, render) bytes per frame, averaged over the lists"""
    from pyannote_video_amd import render
    means = rend = 0
    for prims in lists:
        rend += W * H * 3 + W * H * 3 // 2 + 32 * len(prims)
        for p in prims:
            cells = render.redaction_cells(p)
            if cells:
                w = max(0, min(p[3], W - 1) - max(p[1], 0) + 1)
                h = max(0, min(p[4], H - 1) - max(p[2], 0) + 1)
                means += 3 * w * h + 4 * cells
                rend += 4 * cells
    return means / len(lists), rend / len(lists)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=10, help="passes over the resident frames per timed window")
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N")
    ap.add_argument("--faces", type=int, default=40, help="faces per frame of a --kernel-only run")
    ap.add_argument("--mode", choices=MODES, default="mosaic", help="mode of a --kernel-only run")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    from pyannote_video_amd import synth, render
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0)
    n = a.frames
    video = synth.SyntheticVideo(width=W, height=H, n_frames=n, n_shots=4, faces=8, seed=20260925, frame_rate=25.0)
    frames_t = video.frames_torch(torch.device("cuda", 0))
    torch.cuda.synchronize()
    dev = [ctx.wrap_torch(frames_t[i]) for i in range(n)]
    fb = W * H + 2 * ((W + 1) // 2) * ((H + 1) // 2)
    out = torch.zeros((a.batch, fb), dtype=torch.uint8, device="cuda")
    cases = [(a.faces, a.mode)] if a.kernel_only else [(f, m) for f in (3, 40) for m in MODES]
    lists = {c: face_lists(n, *c) for c in cases}
    packed = {c: [render.pack_primitives(lists[c][i:i + a.batch]) for i in range(0, n, a.batch)] for c in cases}

    def render_all(case):
        for j, i in enumerate(range(0, n, a.batch)):
            ctx.render(dev[i:i + a.batch], packed[case][j], W, H, out_ptr=out.data_ptr())

    if a.kernel_only:
        for _ in range(a.kernel_only):
            render_all(cases[0])
        mb, rb = algorithmic_bytes(lists[cases[0]])
        print(json.dumps({"bench": "redact kernels alone", "passes": a.kernel_only, "frames_per_pass": n, "frames_per_call": a.batch, "faces": a.faces,
                          "mode": a.mode, "algorithmic_bytes_per_frame": {"redact_means_k": round(mb), "render_k": round(rb)}}))
        return

    def timed(case):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.rounds):
            render_all(case)
        ctx.sync()
        return (time.perf_counter() - t0) / a.rounds

    line = {"bench": "redact, 1080p at source size -> YUV 4:2:0", "frames": n, "batch": a.batch, "repeats": a.repeats, "rounds": a.rounds,
            "hbm_achievable_TBps": HBM_ACHIEVABLE_TBPS, "cases": {}}
    for case in cases:
        render_all(case)                                 # warm-up
        fps = [round(n / timed(case), 1) for _ in range(a.repeats)]
        ctx.prof_enable(True)
        ctx.prof_reset()
        render_all(case)
        ctx.sync()
        ms_means = ctx.prof_get("redact_means")[0] / n if case[1] != "fill" else None
        ms_render = ctx.prof_get("render")[0] / n
        ctx.prof_enable(False)
        mb, rb = algorithmic_bytes(lists[case])
        share = lambda b, ms: round(b / (ms * 1e-3) / (HBM_ACHIEVABLE_TBPS * 1e12), 4) if ms else None
        line["cases"]["%d_faces_%s" % case] = {
            "frames_per_s": fps, "kernel_ms_per_frame": {"redact_means_k": ms_means and round(ms_means, 5), "render_k": round(ms_render, 5)},
            "algorithmic_bytes_per_frame": {"redact_means_k": round(mb), "render_k": round(rb)},
            "share_of_hbm_bandwidth": {"redact_means_k": share(mb, ms_means), "render_k": share(rb, ms_render)}}
    print(json.dumps(line))
    for f in dev:
        f.release()
    ctx.close()


if __name__ == "__main__":
    main()
