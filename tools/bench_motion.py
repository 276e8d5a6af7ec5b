"""Motion bench (csrc/motion.hip; MOTION.md), on an MI355X, in one process.

pvf_shot_motion on 256 frames of 1080p resident in HBM (a smooth picture that drifts 3 pixels a frame), small images of 96 x 54 and of
128 x 128.  After one uncounted pass, five repeats in which the two routes take
turns:
  (a) shot_motion calls: wall time, and the library's own device events -- family "motion" is motion_fit_k alone, family "shot" is
      everything the call puts on the stream (shot_convert_k, shot_pair_k, motion_fit_k, the copies of 80 bytes a pair and of the
      differences), so motion_fit_k's share is taken against the rest of that family;
  (b) the route a user had: shot_dfd with the flows brought to the host (about 41 KB a pair at 96 x 54), wall time;
  (c) the fit of those flows in numpy (tests/motion_ref.py, the restatement), wall time, once per repeat.
The rows of (a) and of (b) + (c) must be equal.  No bar is fixed in advance; the design intent -- (a) is not slower than (b) -- is judged
against the spread of (b)'s five repeats and written down either way.

--before-only measures (b) and (c) alone and needs nothing of this pull request but tests/motion_ref.py: with --package-dir it runs on
another build of the package (the commit before), and its JSON is merged into the main run's with --before-json.

Writes profiles/motion_n256.json and prints it.

    python tools/bench_motion.py [--frames 256] [--calls 5] [--before-json FILE]
    python tools/bench_motion.py --before-only --package-dir DIR --out FILE"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPEATS = 5
SIZES = ((96, 54), (128, 128))


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 4), "lowest": round(s[0], 4), "highest": round(s[-1], 4)}


def resident_frames(ctx, torch, n, h=1080, w=1920):
    ys, xs = np.mgrid[0:h, 0:w + 3 * n].astype(np.float32)
    g = (130.0 + 40.0 * np.sin(0.011 * xs + 0.005 * ys) + 30.0 * np.sin(0.007 * xs - 0.013 * ys + 1.0) + 20.0 * np.sin(0.0031 * xs + 0.019 * ys + 2.0)
         + 10.0 * np.sin(0.023 * xs - 0.021 * ys))
    wide = torch.from_numpy(np.clip(g, 0, 255).astype(np.uint8)).cuda()
    src = torch.stack([wide[:, 3 * i:3 * i + w] for i in range(n)])[..., None].expand(n, h, w, 3).contiguous()
    torch.cuda.synchronize()
    dev = [ctx.wrap_torch(src[i]) for i in range(n)]
    return src, dev, ctx.frame_handles(dev)


def timed(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn()
    return (time.perf_counter() - t0) * 1e3 / calls, out


def before_once(ctx, handles, tw, th, tables, calls, motion_ref):
    """-> (wall ms of shot_dfd with the flows to the host per call, wall ms of the numpy fit of one call's flows, the rows)"""
    ms, (dfd, flow) = timed(lambda: ctx.shot_dfd(handles, tw, th, tables, want_flow=True), calls)
    t0 = time.perf_counter()
    rows = motion_ref.rows_of(flow, dfd)
    return ms, (time.perf_counter() - t0) * 1e3, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--calls", type=int, default=5, help="calls per repeat")
    ap.add_argument("--before-only", action="store_true")
    ap.add_argument("--package-dir", default=os.path.join(ROOT, "pyannote-video_amd"))
    ap.add_argument("--before-json", default=None, help="what a --before-only run on the commit before wrote")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_n256.json"))
    a = ap.parse_args()
    sys.path.insert(0, a.package_dir)
    sys.path.insert(0, ROOT)
    import torch
    torch.cuda.set_device(0)
    from pyannote_video_amd import structure
    from pyannote_video_amd.runtime import Context
    from tests import motion_ref
    ctx = Context(device=0)
    tables = structure.shot_tables()
    n = a.frames
    src, dev, handles = resident_frames(ctx, torch, n)
    configs = {}
    for tw, th in SIZES:
        name = "%dx%d" % (tw, th)
        ctx.shot_dfd(handles, tw, th, tables, want_flow=True)       # the uncounted pass
        if not a.before_only:
            ctx.shot_motion(handles, tw, th, tables)
        call, fit, wall, share, fit_ms, rest_ms = [], [], [], [], [], []
        for _ in range(REPEATS):                                    # the two routes take turns
            ms, np_ms, rows_before = before_once(ctx, handles, tw, th, tables, a.calls, motion_ref)
            call.append(ms); fit.append(np_ms)
            if a.before_only:
                continue
            ctx.prof_enable(True)
            ctx.prof_reset()
            ms, (rows, dfd) = timed(lambda: ctx.shot_motion(handles, tw, th, tables), a.calls)
            ctx.sync()
            m_ms, m_n = ctx.prof_get("motion")
            s_ms, s_n = ctx.prof_get("shot")
            ctx.prof_enable(False)
            assert m_n == s_n == a.calls, (m_n, s_n)
            assert np.array_equal(rows, rows_before), "the two routes disagree"
            wall.append(ms); fit_ms.append(m_ms / a.calls); rest_ms.append((s_ms - m_ms) / a.calls); share.append(m_ms / (s_ms - m_ms))
        c = {"pairs": n - 1, "flow_bytes_per_pair": tw * th * 8, "row_bytes_per_pair": 80, "calls_per_repeat": a.calls,
             "shot_dfd_with_flow_out_wall_ms": stats(call), "numpy_fit_wall_ms": stats(fit)}
        if not a.before_only:
            c.update({"shot_motion_wall_ms": stats(wall), "motion_fit_k_ms_per_call": stats(fit_ms), "rest_of_the_shot_family_ms_per_call": stats(rest_ms),
                      "motion_fit_k_over_the_rest": stats(share), "rows_equal": True})
        configs[name] = c
    res = {"bench": "motion: pvf_shot_motion on %d resident frames of 1080p against pvf_shot_dfd with flow_out and a numpy fit" % n, "frames": n,
           "repeats": REPEATS, "configurations": configs}
    if a.before_json:
        res["commit_before"] = json.load(open(a.before_json))["configurations"]
    if not a.before_only:
        for name, c in configs.items():
            ref = res.get("commit_before", configs)[name]["shot_dfd_with_flow_out_wall_ms"]
            c["route_before_measured_on"] = "the commit before" if a.before_json else "this tree"
            c["shot_motion_over_shot_dfd_with_flow_out"] = round(c["shot_motion_wall_ms"]["median"] / ref["median"], 4)
            c["not_slower_than_shot_dfd_with_flow_out"] = bool(c["shot_motion_wall_ms"]["median"] <= ref["highest"])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    del dev, handles, src
    ctx.close()


if __name__ == "__main__":
    main()
