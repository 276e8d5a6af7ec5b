#!/usr/bin/env python
"""Shot threading benchmark: a synthetic clip of --shots shots cut from --setups recurring camera set-ups (textured scenes, small camera
jitter), threaded at --lookahead as `thread` does it.  Stage by stage, in ms: frames (build + upload of the two frames per shot),
extract (ORB on all of them, csrc/orb.hip), match (every pair within the lookahead, one launch), host (graph, labels, smoothing); then
the CPU restatement (tests/orb_ref.py, numpy, --cpu-workers processes) on a sample of the same frames and pairs, scaled to the whole
input.  Prints one JSON line.
    python tools/bench_thread.py [--shots 1000] [--lookahead 24] [--width 640 --height 360] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scenes(n, h, w, seed=0):
    out = []
    for k in range(n):
        rng = np.random.default_rng(seed * 1000 + k)
        small = rng.random((h // 16 + 2, w // 16 + 2, 3)) * 120 + 60
        img = np.repeat(np.repeat(small, 16, 0), 16, 1)[:h, :w].copy()
        for _ in range(60):
            rh, rw = rng.integers(8, h // 4), rng.integers(8, w // 4)
            y, x = rng.integers(0, h - rh), rng.integers(0, w - rw)
            img[y:y + rh, x:x + rw] = rng.integers(0, 256, 3)
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def _cpu_orb(frame):
    import orb_ref
    return orb_ref.orb_frame(frame)[1]


def _cpu_match(args):
    import orb_ref
    a, b = args
    return orb_ref.match_count(a, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shots", type=int, default=1000)
    ap.add_argument("--setups", type=int, default=40)
    ap.add_argument("--lookahead", type=int, default=24)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--cpu-workers", type=int, default=16)
    ap.add_argument("--cpu-frames", type=int, default=64, help="frames the CPU restatement extracts (scaled to all)")
    ap.add_argument("--cpu-pairs", type=int, default=256, help="pairs the CPU restatement matches (scaled to all)")
    a = ap.parse_args()
    from pyannote_video_amd import structure
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0)
    pad = 4
    sc = scenes(a.setups, a.height + 2 * pad, a.width + 2 * pad)
    rng = np.random.default_rng(1)
    setup_of = rng.integers(0, a.setups, a.shots)
    jit = rng.integers(-pad, pad + 1, (2 * a.shots, 2))
    ow, oh = 200, int(a.width * 200 / a.height)
    pairs = structure.lookahead_pairs(a.shots, a.lookahead)
    set_pairs = np.array([(2 * i + 1, 2 * k) for i, k in pairs], np.int32)      # (last frame of shot i, first frame of shot k)
    times = {"frames": [], "extract": [], "match": [], "host": []}
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        frames = [sc[setup_of[j // 2]][pad + jit[j, 0]:pad + jit[j, 0] + a.height, pad + jit[j, 1]:pad + jit[j, 1] + a.width]
                  for j in range(2 * a.shots)]
        staged = [ctx.upload(np.ascontiguousarray(f)) for f in frames]
        ctx.sync()
        t1 = time.perf_counter()
        counts, _, _ = ctx.orb_extract(staged, ow, oh)
        t2 = time.perf_counter()
        got = ctx.orb_match_counts(set_pairs)
        t3 = time.perf_counter()
        segs = [structure.Segment(i, i + 1) for i in range(a.shots)]
        threads = structure.thread_labels(segs, [p for p, c in zip(pairs, got) if c > 20])
        structure.thread_scenes(threads)
        t4 = time.perf_counter()
        for k, v in zip(times, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            times[k].append(v * 1e3)
        del staged
    med = {k: round(float(np.median(v)), 2) for k, v in times.items()}
    # CPU restatement on a sample, scaled to the whole input
    from multiprocessing import Pool
    sample = list(range(0, 2 * a.shots, max(1, 2 * a.shots // a.cpu_frames)))[:a.cpu_frames]
    with Pool(a.cpu_workers) as pool:
        c0 = time.perf_counter()
        descs = pool.map(_cpu_orb, [np.ascontiguousarray(frames[j]) for j in sample])
        c1 = time.perf_counter()
        pidx = rng.integers(0, len(descs), (a.cpu_pairs, 2))
        pool.map(_cpu_match, [(descs[i], descs[j]) for i, j in pidx])
        c2 = time.perf_counter()
    cpu_extract = (c1 - c0) * 1e3 * (2 * a.shots) / len(sample)
    cpu_match = (c2 - c1) * 1e3 * len(pairs) / a.cpu_pairs
    gpu = med["extract"] + med["match"]
    per1000 = 1000.0 / a.shots
    print(json.dumps({
        "metric": "thread_ms_per_1000_shots", "shots": a.shots, "lookahead": a.lookahead, "pairs": len(pairs), "frames": 2 * a.shots,
        "frame_size": [a.width, a.height], "small_image": [ow, oh], "mean_keypoints": round(float(counts.mean()), 1),
        "edges": int((got > 20).sum()), "stage_ms": med, "gpu_extract_match_ms_per_1000_shots": round(gpu * per1000, 2),
        "cpu_restatement": {"workers": a.cpu_workers, "frames_sampled": len(sample), "pairs_sampled": a.cpu_pairs,
                            "extract_ms_scaled": round(cpu_extract, 1), "match_ms_scaled": round(cpu_match, 1),
                            "extract_match_ms_per_1000_shots": round((cpu_extract + cpu_match) * per1000, 1)},
        "speedup_vs_cpu_restatement": round((cpu_extract + cpu_match) / gpu, 1) if gpu > 0 else None}))
    ctx.close()


if __name__ == "__main__":
    main()
