"""Demo-render bench: 1080p frames resident in HBM rendered to 711 x 400 planar YUV 4:2:0 (csrc/render.hip), in one process:
  (a) render only, batch form (pvf_render_batch into device memory), frames/s at 3 and at 40 faces per frame
      (a face = rectangle + '#id' + label + nose line; every frame also carries its timestamp);
  (b) the kernel alone, ms per frame from the library's own event timing (family "render"), and the fraction of HBM bandwidth its
      algorithmic bytes come to: the source bytes the resize touches plus 1.5 bytes per output pixel;
  (c) the path a user had before, timed in the same run: Context.resize, then a device-to-host copy of the RGB frame
      (no drawing, no colour conversion, 3 bytes per output pixel over PCIe);
  (d) the egress ring fed from resident frames (render, copy to pinned host memory, nothing written), frames/s;
  (e) the `demo` verb end to end on `synthetic:1920x1080x<frames>`, written to a temporary file, beside the rate at which that source
      alone yields frames (the synthetic renderer stands in for a decoder and runs on the host);
  (f) the verb on the same number of frames served from host memory (the --frames pictures in turn: a decoder that costs nothing), so
      that what is timed is the verb -- pinned ingest, render, egress, file write -- and not the source.
Timed windows of (a), (c), (d) hold --rounds passes over the resident frames.  One JSON line.

    python tools/bench_demo.py [--frames 128] [--repeats 3] [--e2e-frames 1000]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_demo.py --kernel-only 20

--kernel-only N: nothing but N batch calls at 40 faces, for a kernel trace of its own."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
HBM_ACHIEVABLE_TBPS = 6.3       # what a float4 copy reaches on an MI355X (of 8 TB/s nominal)
W, H, OW, OH = 1920, 1080, 711, 400


def face_lists(n_frames, faces, seed=1):
    """per-frame primitive lists of the shape build_plan makes: timestamp, then rectangle, '#id', label and nose line per face"""
    import numpy as np
    from pyannote_video_amd import render
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n_frames):
        prims = [(render.PRIM_TEXT, 10, OH - 10, render.TEXT_COLOUR, 2, b"%.3f" % (k / 25.0))]
        for ident in range(faces):
            s = int(rng.randint(30, 110))
            l, t = int(rng.randint(0, OW - s)), int(rng.randint(0, OH - s))
            colour = render.PALETTE[ident % 26]
            prims += [(render.PRIM_RECT, l, t, l + s, t + s, colour), (render.PRIM_TEXT, l, t + s + 15, render.TEXT_COLOUR, 2, b"#%d" % ident),
                      (render.PRIM_TEXT, l, t - 7, render.TEXT_COLOUR, 2, b"%d" % (ident % 7)),
                      (render.PRIM_LINE, l + s // 2, t + s // 3, l + s // 2 + 2, t + 2 * s // 3, colour)]
        out.append(prims)
    return out


def touched_source_bytes():
    """bytes of the source frame the bilinear taps of a 1920 x 1080 -> 711 x 400 resize read (each once)"""
    import numpy as np
    def taps(n_in, n_out):
        f = ((np.arange(n_out) + 0.5) * (float(n_in) / n_out) - 0.5).astype(np.float32)
        s = np.clip(np.floor(f).astype(np.int64), 0, n_in - 1)
        return len(set(s.tolist()) | set(np.minimum(s + 1, n_in - 1).tolist()))
    return taps(W, OW) * taps(H, OH) * 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=40, help="passes over the resident frames per timed window of (a); (c) and (d) take a quarter")
    ap.add_argument("--e2e-frames", type=int, default=1000)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from pyannote_video_amd import synth, render, cli
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0)
    n = a.frames
    video = synth.SyntheticVideo(width=W, height=H, n_frames=n, n_shots=4, faces=8, seed=20260925, frame_rate=25.0)
    frames_t = video.frames_torch(torch.device("cuda", 0))
    torch.cuda.synchronize()
    dev = [ctx.wrap_torch(frames_t[i]) for i in range(n)]
    fb = OW * OH + 2 * ((OW + 1) // 2) * ((OH + 1) // 2)
    out = torch.zeros((a.batch, fb), dtype=torch.uint8, device="cuda")
    packed = {faces: [render.pack_primitives(face_lists(n, faces)[i:i + a.batch]) for i in range(0, n, a.batch)] for faces in (3, 40)}

    def render_all(faces):
        for j, i in enumerate(range(0, n, a.batch)):
            ctx.render(dev[i:i + a.batch], packed[faces][j], OW, OH, out_ptr=out.data_ptr())

    if a.kernel_only:
        for _ in range(a.kernel_only):
            render_all(40)
        print(json.dumps({"bench": "render_k alone", "calls": a.kernel_only * len(packed[40]), "frames_per_call": a.batch, "faces": 40,
                          "algorithmic_bytes_per_frame": touched_source_bytes() + fb}))
        return
    with open("/proc/self/maps") as maps:          # the HIP runtime this process already runs on
        hip = C.CDLL(sorted(set(line.split()[-1] for line in maps if "libamdhip64" in line))[0])
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    host_rgb = torch.zeros((OH, OW, 3), dtype=torch.uint8).pin_memory()

    def resize_and_copy():
        from pyannote_video_amd._lib import check
        for f in dev:
            g = ctx.resize(f, OW, OH)
            p = C.c_void_p(0)
            check(ctx._l.pvf_frame_device_ptr(ctx._h, g.handle, C.byref(p)))
            ctx.sync()
            assert hip.hipMemcpy(host_rgb.data_ptr(), p.value, OW * OH * 3, 2) == 0
            g.release()

    ring = ctx.egress_ring(OW, OH, depth=16)
    lists3 = face_lists(n, 3)

    def ring_all():
        pending = []
        for f, prims in zip(dev, lists3):
            if len(pending) == 16:
                s = pending.pop(0)
                ring.wait(s)
                ring.release(s)
            pending.append(ring.submit(f, prims))
        for s in pending:
            ring.wait(s)
            ring.release(s)

    def timed(fn, *args, rounds=1):
        """seconds per pass"""
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(rounds):
            fn(*args)
        ctx.sync()
        return (time.perf_counter() - t0) / rounds

    for fn, args in ((render_all, (3,)), (render_all, (40,)), (resize_and_copy, ()), (ring_all, ())):          # warm-up
        fn(*args)
    t = {"render_3": [], "render_40": [], "resize_copy": [], "ring_3": []}
    kernel_ms = {}
    for _ in range(a.repeats):
        t["render_3"].append(timed(render_all, 3, rounds=a.rounds))
        t["render_40"].append(timed(render_all, 40, rounds=a.rounds))
        t["resize_copy"].append(timed(resize_and_copy, rounds=max(1, a.rounds // 4)))
        t["ring_3"].append(timed(ring_all, rounds=max(1, a.rounds // 4)))
    for faces in (3, 40):
        ctx.prof_enable(True)
        ctx.prof_reset()
        render_all(faces)
        ctx.sync()
        ms, launches = ctx.prof_get("render")
        ctx.prof_enable(False)
        kernel_ms[faces] = ms / n
    algo = touched_source_bytes() + fb
    line = {"bench": "demo render, 1080p -> 711x400 YUV 4:2:0", "frames": n, "batch": a.batch, "repeats": a.repeats, "rounds": a.rounds,
            "a_render_only_frames_per_s": {"3_faces": [round(n / x, 1) for x in t["render_3"]], "40_faces": [round(n / x, 1) for x in t["render_40"]]},
            "b_kernel_ms_per_frame": {"3_faces": round(kernel_ms[3], 5), "40_faces": round(kernel_ms[40], 5)},
            "b_algorithmic_bytes_per_frame": algo,
            "b_fraction_of_%.1f_TBps" % HBM_ACHIEVABLE_TBPS: {k: round(algo / (v * 1e-3) / (HBM_ACHIEVABLE_TBPS * 1e12), 4) for k, v in
                                                               (("3_faces", kernel_ms[3]), ("40_faces", kernel_ms[40]))},
            "c_resize_then_rgb_copy_frames_per_s": [round(n / x, 1) for x in t["resize_copy"]],
            "d_egress_ring_3_faces_frames_per_s": [round(n / x, 1) for x in t["ring_3"]],
            "bytes_over_pcie_per_frame": {"fused": fb, "resize_then_rgb_copy": OW * OH * 3}}
    ring.close()
    if a.e2e_frames > 0:
        m = a.e2e_frames
        spec = "synthetic:%dx%dx%d" % (W, H, m)
        tmp = tempfile.mkdtemp()
        track = os.path.join(tmp, "track.txt")
        rng = np.random.RandomState(2)
        with open(track, "w") as f:                     # three faces on every frame (the verb does not care where they come from)
            for k in range(m):
                for ident in range(3):
                    l, tp = rng.uniform(0.0, 0.7, 2)
                    f.write("%.3f %d %.3f %.3f %.3f %.3f detection\n" % (k / 25.0, ident, l, tp, l + 0.2, tp + 0.25))
        t0 = time.perf_counter()
        k = 0
        for _ in cli.open_video("synthetic:%dx%dx%d" % (W, H, min(m, 50)), 25.0):
            k += 1
        source_rate = k / (time.perf_counter() - t0)
        t0 = time.perf_counter()
        res = cli.demo(cli.open_video(spec, 25.0), track, os.path.join(tmp, "demo.y4m"), ctx=ctx)
        dt = time.perf_counter() - t0
        line["e_demo_verb"] = {"video": spec, "output_frames": res["frames"], "frames_per_s": round(res["frames"] / dt, 1),
                               "source_alone_frames_per_s": round(source_rate, 1), "output_bytes": os.path.getsize(os.path.join(tmp, "demo.y4m"))}
        os.remove(os.path.join(tmp, "demo.y4m"))

        class HostClip(object):
            """m frames, the n resident pictures in turn, already decoded in host memory"""
            frame_rate, size = 25.0, (W, H)

            def __init__(self):
                self.pictures = [frames_t[i].cpu().numpy() for i in range(n)]

            def __len__(self):
                return m

            def __iter__(self):
                for k in range(m):
                    yield k / 25.0, self.pictures[k % n]
        clip = HostClip()
        t0 = time.perf_counter()
        res = cli.demo(clip, track, os.path.join(tmp, "demo.y4m"), ctx=ctx)
        dt = time.perf_counter() - t0
        line["f_demo_verb_frames_in_host_memory"] = {"output_frames": res["frames"], "frames_per_s": round(res["frames"] / dt, 1)}
        os.remove(os.path.join(tmp, "demo.y4m"))
    print(json.dumps(line))
    for f in dev:
        f.release()
    ctx.close()


if __name__ == "__main__":
    main()
