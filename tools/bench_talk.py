"""Talk bench (csrc/talk.hip; TALK.md), on 1080p frames resident in HBM, in one process: pvf_face_motion at n
faces (default 4096, one round), every face but the first of its chain of 16 linked to the face before it.  ms per call by the host
clock (the call ends in a stream synchronise), and from the library's own event timing the two steps it is made of -- the chip
extraction (family "chip": pyramid levels and the affine sampling) and mouth_patch_k + patch_motion_k (family "talk") -- on the same
faces in the same calls, and their ratio.
Writes one JSON object to --out (default profiles/talk_n4096.json) and prints it.

    python tools/bench_talk.py [--faces 4096] [--frames 64] [--repeats 5]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_talk.py --kernel-only 10

--kernel-only N: nothing but N face_motion calls, for a kernel trace of its own."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CHAIN = 16                      # faces of a chain: the first has no predecessor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=10, help="calls per timed window")
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "talk_n4096.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from bench_faces import H, W, face_points
    from pyannote_video_amd import synth, talk
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0)
    video = synth.SyntheticVideo(width=W, height=H, n_frames=a.frames, n_shots=4, faces=8, seed=20260925, frame_rate=25.0)
    frames_t = video.frames_torch(torch.device("cuda", 0))
    torch.cuda.synchronize()
    dev = [ctx.wrap_torch(frames_t[i]) for i in range(a.frames)]
    n = a.faces
    pts = face_points(n)
    handles = ctx.frame_handles([dev[i % a.frames] for i in range(n)])
    prev = np.array([-1 if i % CHAIN == 0 else i - 1 for i in range(n)], np.int32)
    motion = lambda: ctx.face_motion(handles, pts, prev)

    if a.kernel_only:
        for _ in range(a.kernel_only):
            motion()
        print(json.dumps({"bench": "face_motion kernels alone", "calls": a.kernel_only, "faces": n}))
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

    rows = motion()                                         # warm-up
    dark = float((rows[:, 7] > talk.MAX_DARK * talk.BOTH_PIXELS).mean())
    ms = [round(window(motion), 4) for _ in range(a.repeats)]
    fam = [families(motion, ("chip", "talk")) for _ in range(a.repeats)]
    kc, kt = sorted(f["chip"] for f in fam), sorted(f["talk"] for f in fam)
    scale = 4096.0 / n
    line = {
        "bench": "talk: motion of %d faces on 1080p frames, chains of %d" % (n, CHAIN), "faces": n, "linked": int((prev >= 0).sum()),
        "frames": a.frames, "repeats": a.repeats, "calls_per_window": a.rounds, "share_of_faces_too_dark_to_be_valid": round(dark, 4),
        "face_motion": {"ms_per_call_host_clock": ms, "bytes_back_per_face": 32, "kernel_ms_per_call": {"chip": kc, "talk": kt}},
        "ms_per_4096_faces": {"chip": round(kc[len(kc) // 2] * scale, 5), "talk": round(kt[len(kt) // 2] * scale, 5)},
        "talk_over_chip": round(kt[len(kt) // 2] / kc[len(kc) // 2], 4),
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
