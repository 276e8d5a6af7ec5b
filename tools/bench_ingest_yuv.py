"""Ingest bench: the bench clip (BASELINE.json configs[1]: 1000 frames of 1080p) waiting in pinned host slots once as RGB and once as
YUV 4:2:0, modelled on bench.py's host_ingest_pass.  For each form, alternating in one process, `--repeats` times:
  (a) uploads alone  -- every slot submitted, then the ring's copy stream drained: GB/s over PCIe and frames/s (the YUV ring's figure
      includes its conversion kernel, which runs on the same stream behind each copy);
  (b) the full step  -- pipe.run fed from the ring, frames/s.
Both rings deliver the same pictures: the clip is taken to 4:2:0 once and the RGB ring holds its conversion back to RGB (the project's
integer formula, evaluated with torch), so the steps must return the same tracks -- `same_result` in the line.  One JSON line.

    python tools/bench_ingest_yuv.py [--frames 1000] [--repeats 3]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_ingest_yuv.py --kernel-only 200

--kernel-only N: nothing but N conversions of planes resident in HBM (1080p and 4K, planar and NV12), for a kernel trace of its own;
the line it prints holds the bytes each launch has to move (4.5 per pixel for 4:2:0) to put beside the trace's kernel times."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
HBM_ACHIEVABLE_TBPS = 6.3       # what a float4 copy reaches on an MI355X (of 8 TB/s nominal)


def rgb_to_yuv420_torch(rgb):
    """input maker (BT.601 limited range in float, chroma averaged over 2x2): uint8 [H, W, 3] on the device -> y, u, v uint8"""
    import torch
    r, g, b = (rgb[..., k].float() for k in range(3))
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    pool = lambda p: torch.nn.functional.avg_pool2d(p[None, None], 2)[0, 0]
    q8 = lambda p: p.round().clamp(0, 255).to(torch.uint8)
    return q8(y), q8(pool(u)), q8(pool(v))


def yuv420_to_rgb_torch(y, u, v):
    """the project's conversion (BT.601, limited range) in int32 on the device: what the kernel writes, byte for byte"""
    import torch
    from pyannote_video_amd.y4m import coefficients
    ymul, yoff, crv, cgu, cgv, cbu = coefficients("601", False)
    h, w = y.shape
    c = ymul * y.int() + yoff
    up = lambda p: p.int().repeat_interleave(2, 0).repeat_interleave(2, 1)[:h, :w] - 128
    uu, vv = up(u), up(v)
    return torch.stack([((c + crv * vv) >> 16).clamp(0, 255), ((c - cgu * uu - cgv * vv) >> 16).clamp(0, 255),
                        ((c + cbu * uu) >> 16).clamp(0, 255)], dim=-1).to(torch.uint8)


def kernel_only(ctx, n):
    import torch
    out = {}
    for name, (w, h) in (("1080p", (1920, 1080)), ("2160p", (3840, 2160))):
        g = torch.Generator(device="cuda").manual_seed(1)
        y = torch.randint(0, 256, (h, w), dtype=torch.uint8, device="cuda", generator=g)
        u = torch.randint(0, 256, (h // 2, w // 2), dtype=torch.uint8, device="cuda", generator=g)
        v = torch.randint(0, 256, (h // 2, w // 2), dtype=torch.uint8, device="cuda", generator=g)
        uv = torch.stack([u, v], dim=-1).contiguous()
        torch.cuda.synchronize()
        for kind, args in (("planar", (y, u, v)), ("nv12", (y, uv))):
            t0 = time.perf_counter()
            for _ in range(n):
                ctx.frame_from_yuv_torch(*args).release()
            ctx.sync()
            dt = time.perf_counter() - t0
            out["%s_%s" % (name, kind)] = {"launches": n, "bytes_per_launch": int(h * w * 4.5),
                                           "us_at_%.1f_TBps" % HBM_ACHIEVABLE_TBPS: round(h * w * 4.5 / (HBM_ACHIEVABLE_TBPS * 1e12) * 1e6, 2),
                                           "host_us_per_call_including_the_wait": round(1e6 * dt / n, 1)}
    print(json.dumps({"bench": "yuv_to_rgb_k alone (planes in HBM, pvf_frame_from_yuv)", "cases": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N")
    a = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from pyannote_video_amd import synth, models, pipeline
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0)
    if a.kernel_only:
        return kernel_only(ctx, a.kernel_only)
    n, w, h = a.frames, 1920, 1080
    lp, ep = models.ensure_synthetic_models(os.path.join(tempfile.gettempdir(), "pvface_models_rank0"), small=False)
    video = synth.SyntheticVideo(width=w, height=h, n_frames=n, n_shots=4, faces=8, seed=20260925, frame_rate=25.0)
    frames_t = video.frames_torch(torch.device("cuda", 0))
    times = [video.timestamp(i) for i in range(n)]
    shots = video.shots()
    pipe = pipeline.FacePipeline(ctx, lp, ep, detect_batch_size=128)
    rings = {"rgb": ctx.ingest_ring(h, w, depth=n), "yuv420": ctx.ingest_ring_yuv(h, w, depth=n)}      # the whole clip "decoded" into pinned slots, once
    for i in range(n):
        y, u, v = rgb_to_yuv420_torch(frames_t[i])
        for dst, src in zip(rings["yuv420"].slot(), (y, u, v)):
            np.copyto(dst, src.cpu().numpy())
        np.copyto(rings["rgb"].slot(), yuv420_to_rgb_torch(y, u, v).cpu().numpy())
    del frames_t
    torch.cuda.empty_cache()
    bytes_per_frame = {"rgb": h * w * 3, "yuv420": h * w * 3 // 2}

    def submit_all(ring):
        out = []
        for _ in range(n):
            ring.slot()                                    # slot i again (its bytes are still there); waits for its previous upload
            out.append(ring.submit())
        return out

    def uploads_alone(ring):
        ctx.sync()
        t0 = time.perf_counter()
        dev = submit_all(ring)
        ring.wait()
        dt = time.perf_counter() - t0
        for f in dev:
            f.release()
        return dt

    def full_step(ring):
        ctx.sync()
        t0 = time.perf_counter()
        dev = submit_all(ring)
        res = pipe.run(dev, times, video.frame_rate, shots, cluster=True)
        ctx.sync()
        dt = time.perf_counter() - t0
        for f in dev:
            f.release()
        return dt, res

    results = {}
    for kind, ring in rings.items():                       # warm-up: every shape the timed windows use
        uploads_alone(ring)
        results[kind] = full_step(ring)[1]
    same = (results["rgb"]["tracks"] == results["yuv420"]["tracks"] and results["rgb"]["labels"] == results["yuv420"]["labels"]
            and np.array_equal(results["rgb"]["embeddings"], results["yuv420"]["embeddings"]))
    t_copy = {k: [] for k in rings}
    t_step = {k: [] for k in rings}
    for _ in range(a.repeats):
        for kind, ring in rings.items():
            t_copy[kind].append(uploads_alone(ring))
        for kind, ring in rings.items():
            t_step[kind].append(full_step(ring)[0])
    line = {"bench": "ingest ring, RGB against YUV 4:2:0", "frames": n, "size": [w, h], "repeats": a.repeats, "same_result": bool(same),
            "tracks": len(results["rgb"]["tracks"])}
    for kind in rings:
        line[kind] = {"bytes_per_frame_over_pcie": bytes_per_frame[kind],
                      "uploads_alone_GBps": [round(n * bytes_per_frame[kind] / t / 1e9, 2) for t in t_copy[kind]],
                      "uploads_alone_frames_per_s": [round(n / t, 1) for t in t_copy[kind]],
                      "full_step_frames_per_s": [round(n / t, 1) for t in t_step[kind]]}
    best = lambda kind, d: n / min(d[kind])
    line["yuv_over_rgb"] = {"uploads_alone_frames_per_s": round(best("yuv420", t_copy) / best("rgb", t_copy), 3),
                            "full_step_frames_per_s": round(best("yuv420", t_step) / best("rgb", t_step), 3)}
    print(json.dumps(line))
    for ring in rings.values():
        ring.close()
    ctx.close()


if __name__ == "__main__":
    main()
