"""Faces bench (csrc/faces.hip; FACES.md), on 1080p frames resident in HBM, in one process:
  (a) pvf_face_quality at n faces (default 4096, one round): ms per call by the host clock (the call ends in a stream synchronise), and
      from the library's own event timing the two steps it is made of -- the chip extraction (family "chip": pyramid levels and the
      affine sampling, what pvf_face_chips runs before its copy to the host) and chip_quality_k (family "chip_quality") -- on the same
      faces in the same calls;
  (b) chip_quality_k alone against its algorithmic bytes, 67 500 read + 40 written per chip, as a share of HBM bandwidth (achievable and
      nominal).  n = 4096 chips are 276 MB, written by the chip step just before: part of them may still lie in the 256 MiB Infinity
      Cache, so the figure is an upper bound on what HBM itself delivered;
  (c) a contact sheet of 24 groups x 4 faces at tile 150 (pvf_face_sheet: chips, sheet_tiles_k, sheet_prims_k, the copy of the sheet to
      the host): ms per call, and the kernels' share from the families "chip" and "sheet".
Writes one JSON object to --out (default profiles/faces_n4096.json) and prints it.

    python tools/bench_faces.py [--faces 4096] [--frames 64] [--repeats 5]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_faces.py --kernel-only 10

--kernel-only N: nothing but N face_quality calls, for a kernel trace of its own."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
HBM_ACHIEVABLE_TBPS = 6.3       # what a float4 copy reaches on an MI355X (of 8 TB/s nominal)
HBM_NOMINAL_TBPS = 8.0
W, H = 1920, 1080
CHIP_BYTES = 150 * 150 * 3


def face_points(n, seed=3):
    """int32 [n, 68, 2]: dlib's mean face shape, 60 .. 400 pixels wide, turned by up to 25 degrees, centred anywhere in the frame (a face
    near an edge gives a chip that is partly black, as in a film)"""
    import numpy as np
    from pyannote_video_amd import models
    rng = np.random.RandomState(seed)
    mean = np.stack([np.asarray(models.DLIB_MEAN_FACE_X), np.asarray(models.DLIB_MEAN_FACE_Y)], 1)
    jaw = np.stack([0.5 + 0.55 * np.cos(np.linspace(math.pi, 0, 17)), 0.5 + 0.55 * np.sin(np.linspace(math.pi, 0, 17))], 1)
    unit = np.concatenate([jaw, mean]) - 0.5
    out = np.empty((n, 68, 2), np.int32)
    for i in range(n):
        face = rng.uniform(60, 400)
        a = math.radians(rng.uniform(-25, 25))
        cx, cy = rng.uniform(0, W), rng.uniform(0, H)
        x = cx + face * (math.cos(a) * unit[:, 0] - math.sin(a) * unit[:, 1])
        y = cy + face * (math.sin(a) * unit[:, 0] + math.cos(a) * unit[:, 1])
        out[i] = np.rint(np.stack([x, y], 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=10, help="calls per timed window")
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "faces_n4096.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from pyannote_video_amd import faces, synth
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0)
    video = synth.SyntheticVideo(width=W, height=H, n_frames=a.frames, n_shots=4, faces=8, seed=20260925, frame_rate=25.0)
    frames_t = video.frames_torch(torch.device("cuda", 0))
    torch.cuda.synchronize()
    dev = [ctx.wrap_torch(frames_t[i]) for i in range(a.frames)]
    n = a.faces
    pts = face_points(n)
    handles = ctx.frame_handles([dev[i % a.frames] for i in range(n)])

    if a.kernel_only:
        for _ in range(a.kernel_only):
            ctx.face_quality(handles, pts)
        print(json.dumps({"bench": "face_quality kernels alone", "calls": a.kernel_only, "faces": n}))
        return

    def window(call):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.rounds):
            call()
        ctx.sync()
        return (time.perf_counter() - t0) / a.rounds * 1e3

    def families(call, names):
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(a.rounds):
            call()
        ctx.sync()
        out = {k: round(ctx.prof_get(k)[0] / a.rounds, 5) for k in names}
        ctx.prof_enable(False)
        return out

    quality = lambda: ctx.face_quality(handles, pts)
    sums = quality()                                        # warm-up
    black = float((sums[:, 3] > 0.25 * 22500).mean())
    q_ms = [round(window(quality), 4) for _ in range(a.repeats)]
    q_fam = [families(quality, ("chip", "chip_quality")) for _ in range(a.repeats)]
    kq = sorted(f["chip_quality"] for f in q_fam)
    kc = sorted(f["chip"] for f in q_fam)
    bytes_q = n * (CHIP_BYTES + 40)
    tbps = bytes_q / (kq[len(kq) // 2] * 1e-3) / 1e12

    groups = [("#%d" % g, g, 4) for g in range(24)]
    SW, SH, corners, prims = faces.layout(groups, 4, 150, 1)
    xy = [c for g in corners for c in g]
    sheet = lambda: ctx.face_sheet(handles[:96], pts[:96], xy, 150, SW, SH, faces.BACKGROUND, prims)
    sheet()
    s_ms = [round(window(sheet), 4) for _ in range(a.repeats)]
    s_fam = [families(sheet, ("chip", "sheet")) for _ in range(a.repeats)]

    line = {
        "bench": "faces: quality of %d faces on 1080p frames, and a 24 x 4 sheet" % n, "faces": n, "frames": a.frames, "repeats": a.repeats,
        "calls_per_window": a.rounds, "share_of_faces_with_more_than_a_quarter_black": round(black, 4),
        "face_quality": {
            "ms_per_call_host_clock": q_ms, "bytes_back_per_face": 40,
            "kernel_ms_per_call": {"chip_step": kc, "chip_quality_k": kq},
            "chip_quality_share_of_chip_step_plus_itself": round(kq[len(kq) // 2] / (kq[len(kq) // 2] + kc[len(kc) // 2]), 4)},
        "chip_quality_k": {
            "algorithmic_bytes_per_call": bytes_q, "median_ms": kq[len(kq) // 2], "TB_per_s": round(tbps, 4),
            "share_of_hbm_achievable_%.1f" % HBM_ACHIEVABLE_TBPS: round(tbps / HBM_ACHIEVABLE_TBPS, 4),
            "share_of_hbm_nominal_%.1f" % HBM_NOMINAL_TBPS: round(tbps / HBM_NOMINAL_TBPS, 4),
            "note": "the chips were written by the chip step just before; 276 MB against a 256 MiB Infinity Cache: an upper bound on HBM's own rate"},
        "sheet_24x4_tile150": {"width": SW, "height": SH, "ms_per_call_host_clock": s_ms,
                               "kernel_ms_per_call": {"chip_step": sorted(f["chip"] for f in s_fam), "sheet_kernels": sorted(f["sheet"] for f in s_fam)},
                               "sheet_bytes_to_host": SW * SH * 3},
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
