"""GPU: the DSST tracker (csrc/dsst.hip: the fused start / update kernels through the chip path of csrc/chip.hip, and scale_fhog_k<true>,
which samples the frame itself) against oracle.Tracker on the geometry table of tests/chip_cases.py -- row pitches of every remainder
modulo 4, frames smaller than the tracker's chips, boxes inside, across, as large as, larger and far larger than the frame, frames that
reach the kernels by every route (upload, a wrapped tensor, views 1, 2 and 3 bytes into a buffer of 0xAA, the ingest ring), one call over
frames of different sizes, and the pipeline on a 854 x 480 clip.  tests/test_chip_cases.py proves on the oracle alone that the table holds
what it claims.  Filter states compare as bytes, positions as values, confidences with NaN == NaN (tests/test_gpu_tracker_edges.py).
No tolerances.  Reference: pyannote/video/tracking.py:203,231,250-251."""
import numpy as np
import pytest
import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships

import chip_cases as cc
from test_gpu_tracker_edges import _against_oracle, _diff, _same_psr, _state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables():
    from pyannote_video_amd import models
    return models.dsst_tables()


@pytest.mark.parametrize("g", cc.GEOMETRY, ids=lambda g: g.name)
def test_start_and_two_updates_equal_the_oracle(ctx, oracle, tables, g):
    """all boxes of the geometry in one *_many call; state, confidence and position after the start and after each update"""
    bad = _against_oracle(ctx, oracle, tables, [cc.tracker_case(g, c) for c in cc.tracker_content(g)])
    assert not bad, bad[:20]


@pytest.mark.parametrize("g", cc.GEOMETRY, ids=lambda g: g.name)
def test_deferred_update_and_commit_equal_the_immediate_update(ctx, g):
    """both arg-max kernels on the odd geometries: update_many(defer=True) returns what the immediate update returns and leaves every
    filter untouched; commit_many then gives the immediate update's state"""
    bad = []
    for c in cc.tracker_content(g):
        case = cc.tracker_case(g, c)
        n = len(case.boxes)
        now, later = ctx.tracker_create_many(n), ctx.tracker_create_many(n)
        try:
            for t in (now, later):
                ctx.tracker_start_many(t, [case.frames[0]] * n, case.boxes)
            for i, f in enumerate(case.frames[1:]):
                p0, b0 = ctx.tracker_update_many(now, [f] * n)
                before = [_state(ctx, t) for t in later]
                p1, b1 = ctx.tracker_update_many(later, [f] * n, defer=True)
                bad += [(case.name, i, k, "the deferred update wrote the filters", d) for k, (t, s) in enumerate(zip(later, before))
                        for d in [_diff(_state(ctx, t), s)] if d]
                if not _same_psr(p0, p1) or not np.array_equal(b0, b1):
                    bad.append((case.name, i, "deferred", p0.tolist(), p1.tolist()))
                ctx.tracker_commit_many(later, [f] * n)
                if [ctx.tracker_position(t) for t in now] != [ctx.tracker_position(t) for t in later]:
                    bad.append((case.name, i, "position after the commit"))
                bad += [(case.name, i, k, "state after the commit", d) for k, (a, b) in enumerate(zip(now, later))
                        for d in [_diff(_state(ctx, b), _state(ctx, a))] if d]
        finally:
            ctx.tracker_destroy_many(now + later)
    assert not bad, bad[:20]


MIXED_BOXES = ("inside", "corner_bottom_right", "whole_frame", "larger_than_frame", "far_larger_than_frame", "last_pixels")


def test_one_call_over_frames_of_different_sizes_equals_one_call_per_tracker(ctx, oracle, tables):
    frames, boxes, tags = [], [], []
    for name in cc.MIXED_SIZES:
        g = cc.by_name(name)
        for bname in MIXED_BOXES:
            frames.append(cc.frames(g, "blobs"))
            boxes.append(dict(cc.boxes(g))[bname])
            tags.append("%s_%s" % (name, bname))
    n = len(boxes)
    batch, single = ctx.tracker_create_many(n), ctx.tracker_create_many(n)
    ref = [oracle.Tracker(tables) for _ in range(n)]
    bad = []
    try:
        ctx.tracker_start_many(batch, [f[0] for f in frames], boxes)
        for t, f, b, r in zip(single, frames, boxes, ref):
            ctx.tracker_start_many([t], [f[0]], [b])
            r.start_track(f[0], b)
        for i, defer in ((1, True), (2, False)):                    # a deferred update with its commit, then an immediate one
            pb, bb = ctx.tracker_update_many(batch, [f[i] for f in frames], defer=defer)
            one = [ctx.tracker_update_many([t], [f[i]], defer=defer) for t, f in zip(single, frames)]
            want = [r.update(f[i]) for r, f in zip(ref, frames)]
            if defer:
                ctx.tracker_commit_many(batch, [f[i] for f in frames])
                for t, f in zip(single, frames):
                    ctx.tracker_commit_many([t], [f[i]])
            for k in range(n):
                if not _same_psr(pb[k], one[k][0][0]) or not _same_psr(pb[k], want[k]):
                    bad.append((tags[k], i, "psr", float(pb[k]), float(one[k][0][0]), want[k]))
                if tuple(bb[k]) != tuple(one[k][1][0]) or tuple(bb[k]) != ref[k].get_position():
                    bad.append((tags[k], i, "position", tuple(bb[k]), ref[k].get_position()))
                d = _diff(_state(ctx, batch[k]), _state(ctx, single[k]))
                if d:
                    bad.append((tags[k], i, "state", d))
    finally:
        ctx.tracker_destroy_many(batch + single)
    assert not bad, bad[:20]


@pytest.mark.parametrize("name", cc.ROUTES)
def test_trackers_on_frames_by_every_route(ctx, oracle, tables, name):
    """a byte read from beside the frame changes a value: the views lie in a buffer of 0xAA"""
    g = cc.by_name(name)
    h, w, nb = g.h, g.w, g.h * g.w * 3
    case = cc.tracker_case(g, "tail")
    n = len(case.boxes)
    f0, f1 = case.frames[0], case.frames[1]
    ref = [oracle.Tracker(tables) for _ in range(n)]
    for r, b in zip(ref, case.boxes):
        r.start_track(f0, b)
    started = [dict(zip(("A", "B", "As", "Bs"), r.debug_state() + r.debug_scale_state())) for r in ref]
    psr = [r.update(f1) for r in ref]
    updated = [dict(zip(("A", "B", "As", "Bs"), r.debug_state() + r.debug_scale_state())) for r in ref]
    bad = []

    def check(d0, d1, how):
        trk = ctx.tracker_create_many(n)
        try:
            ctx.tracker_start_many(trk, [d0] * n, case.boxes)
            for k in range(n):
                d = _diff(_state(ctx, trk[k]), started[k])
                if d:
                    bad.append((name, how, k, "start", d))
            p, b = ctx.tracker_update_many(trk, [d1] * n)
            for k in range(n):
                if not _same_psr(p[k], psr[k]) or tuple(b[k]) != ref[k].get_position():
                    bad.append((name, how, k, "update", float(p[k]), psr[k], tuple(b[k]), ref[k].get_position()))
                d = _diff(_state(ctx, trk[k]), updated[k])
                if d:
                    bad.append((name, how, k, "state after the update", d))
        finally:
            ctx.tracker_destroy_many(trk)

    held = [ctx.upload(f0), ctx.upload(f1)]
    check(held[0], held[1], "upload")
    for fr in held:
        fr.release()
    t0, t1 = torch.from_numpy(f0.copy()).cuda(), torch.from_numpy(f1.copy()).cuda()      # allocations of exactly the frame
    held = [ctx.wrap_torch(t0), ctx.wrap_torch(t1)]
    check(held[0], held[1], "wrap")
    for fr in held:
        fr.release()
    for off in (1, 2, 3):                                            # 1, 2 and 3 bytes into larger byte buffers
        held, bufs = [], []
        for f in (f0, f1):
            buf = torch.full((nb + 8,), 0xAA, dtype=torch.uint8, device="cuda")
            view = buf[off:off + nb].view(h, w, 3)
            view.copy_(torch.from_numpy(f.copy()))
            assert view.data_ptr() % 4 == off and view.is_contiguous()
            bufs.append(buf)
            held.append(ctx.wrap_torch(view))
        torch.cuda.synchronize()
        check(held[0], held[1], "offset%d" % off)
        for fr in held:
            fr.release()
        assert all(bool((buf[:off] == 0xAA).all()) and bool((buf[off + nb:] == 0xAA).all()) for buf in bufs)
    ring = ctx.ingest_ring(h, w, depth=4)
    try:
        held = [ring.push(f0), ring.push(f1)]
        ring.wait()
        check(held[0], held[1], "ring")
        for fr in held:
            fr.release()
    finally:
        ring.close()
    assert not bad, bad[:20]


@pytest.mark.parametrize("every_frames", [0, 3])
def test_pipeline_on_a_480p_clip_matches_the_oracle_flow(ctx, oracle, model_paths, tables, every_frames):
    """854 x 480, the usual 480p size: a 2562-byte pitch.  Six frames, two faces, through FacePipeline.run against the reference's
    sequential flow (tests/test_gpu_e2e.py does this at 640 x 360); with detection on every third frame the trackers carry the faces"""
    from pyannote_video_amd import formats, models, pipeline, synth
    from oracle import ref_flow
    v = synth.SyntheticVideo(width=854, height=480, n_frames=6, n_shots=1, faces=2, min_face=70, max_face=140, seed=3)
    frames_np = [v.frame(i) for i in range(v.n_frames)]
    times = [v.timestamp(i) for i in range(v.n_frames)]
    every = every_frames / v.frame_rate
    pipe = pipeline.FacePipeline(ctx, model_paths[0], model_paths[1], detect_every=every, detect_batch_size=4)
    res = pipe.run([ctx.upload(f) for f in frames_np], times, v.frame_rate, v.shots(), cluster=not every_frames)
    det = oracle.Detector(models.load_container(models.DEFAULT_DETECTOR))
    ref_tracks = ref_flow.track_video(frames_np, times, v.shots(), det, lambda: oracle.Tracker(tables), v.frame_rate, detect_every=every,
                                      min_conf=10., ratio=0.5, max_gap=1.0)
    assert len(ref_tracks) >= v.faces and all(len(tr) == v.n_frames for tr in ref_tracks[:v.faces])
    assert res["tracks"] == ref_tracks
    if every_frames:
        assert any("forward" in st or "backward" in st for tr in ref_tracks for _, _, st in tr)
        return
    sp = oracle.ShapePredictor(models.load_container(model_paths[0]))
    emb = oracle.Embedder(models.load_container(model_paths[1]))
    lines = ref_flow.track_text(ref_tracks)
    assert lines == [l.rstrip("\n") for i, tr in enumerate(res["tracks"]) for l in formats.track_lines(i, tr)]
    got_pts = []
    lm, em = ref_flow.extract(lines, frames_np, times, lambda f, b: got_pts.append(sp(f, b)) or got_pts[-1], emb)
    assert len(got_pts) == len(res["landmarks"]) > 0
    assert np.array_equal(np.stack(got_pts), res["landmarks"])
    ref_e = np.array([[float(x) for x in line.split()[2:]] for line in em]).reshape(-1, 128)
    assert np.linalg.norm(ref_e - res["embeddings"], axis=1).max() <= 1e-4 + 128 ** 0.5 * 5e-6   # text rounding of the reference side
    assert [int(l.split()[1]) for l in em] == res["face_id"].tolist()
    assert ref_flow.cluster(em, 0.6) == res["labels"]
