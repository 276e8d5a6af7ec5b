"""GPU: the DSST tracker (csrc/dsst.hip) and the chip extraction under it (csrc/chip.hip) against oracle.Tracker on the edge-case table of
tests/tracker_cases.py -- boxes that cross, touch, leave or dwarf the frame, faces that slide out of the picture or change size, blank
frames (all-zero response: confidence 0/0 = NaN, arg-max ties, peak at (0, 0), scale index 0), 160 black frames and the return to picture.
tests/test_tracker_edge_cases.py proves on the oracle alone that the table contains those conditions.  Everything is compared bit for
bit; confidences compare as values with NaN == NaN (the sign and payload of a 0/0 differ between x86 and the GPU).  No tolerances.
Reference: pyannote/video/tracking.py:203,231,250-251."""
import numpy as np
import pytest

import tracker_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables():
    from pyannote_video_amd import models
    return models.dsst_tables()


def _same_psr(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def _state(ctx, h, with_F=False):
    F, A, B = ctx.tracker_state(h)
    As, Bs = ctx.tracker_scale_state(h)
    return dict(A=A, B=B, As=As, Bs=Bs, **({"F": F} if with_F else {}))


def _ref_state(r, with_F=False):
    A, B = r.debug_state()
    As, Bs = r.debug_scale_state()
    return dict(A=A, B=B, As=As, Bs=Bs, **({"F": r.debug_F()} if with_F else {}))


def _diff(got, want):
    return [k for k in want if not np.array_equal(got[k], want[k])]


def _against_oracle(ctx, oracle, tables, cases):
    """start_many + the case's updates, library and oracle in lock step; -> list of what differed (empty = equal)"""
    bad = []
    for case in cases:
        n = len(case.boxes)
        ref = [oracle.Tracker(tables) for _ in range(n)]
        trk = ctx.tracker_create_many(n)
        ctx.tracker_start_many(trk, [case.frames[0]] * n, case.boxes)
        for r, b in zip(ref, case.boxes):
            r.start_track(case.frames[0], b)
        for k in range(n):
            d = _diff(_state(ctx, trk[k]), _ref_state(ref[k]))
            if d or ctx.tracker_position(trk[k]) != ref[k].get_position():
                bad.append((case.name, k, "start", d))
        last = len(case.frames) - 1
        for i in range(1, last + 1):
            f = case.frames[i]
            psr, pos = ctx.tracker_update_many(trk, [f] * n)
            for k, r in enumerate(ref):
                p = r.update(f)
                if not _same_psr(psr[k], p):
                    bad.append((case.name, k, i, "psr", float(psr[k]), p))
                if tuple(pos[k]) != r.get_position() or ctx.tracker_position(trk[k]) != r.get_position():
                    bad.append((case.name, k, i, "position", tuple(pos[k]), r.get_position()))
                if i in (1, last) or i % 40 == 0:
                    with_F = n == 1                          # (the plane spectra of a call are those of its first tracker)
                    d = _diff(_state(ctx, trk[k], with_F), _ref_state(r, with_F))
                    if d:
                        bad.append((case.name, k, i, "state", d))
        ctx.tracker_destroy_many(trk)
    return bad


def test_every_case_equals_the_oracle(ctx, oracle, small_video, tables):
    bad = _against_oracle(ctx, oracle, tables, tc.small_cases(small_video))
    assert not bad, bad[:20]


def test_full_size_subset_equals_the_oracle(ctx_full, oracle, tables):
    bad = _against_oracle(ctx_full, oracle, tables, tc.full_cases())
    assert not bad, bad[:20]


def test_deferred_update_and_commit_equal_the_immediate_update(ctx, small_video):
    """update_fused_k's 512-thread arg-max against peak_k's 256-thread one, all-tie maps (black frames, off-frame boxes) included"""
    bad = []
    for case in tc.small_cases(small_video):
        n = len(case.boxes)
        now, later = ctx.tracker_create_many(n), ctx.tracker_create_many(n)
        for t in (now, later):
            ctx.tracker_start_many(t, [case.frames[0]] * n, case.boxes)
        for i, f in enumerate(case.frames[1:]):
            p0, b0 = ctx.tracker_update_many(now, [f] * n)
            before = _state(ctx, later[0]) if i == 0 else None
            p1, b1 = ctx.tracker_update_many(later, [f] * n, defer=True)
            if before is not None and _diff(_state(ctx, later[0]), before):
                bad.append((case.name, i, "the deferred update wrote the filters"))
            if not _same_psr(p0, p1) or not np.array_equal(b0, b1):
                bad.append((case.name, i, "deferred", p0.tolist(), p1.tolist()))
            ctx.tracker_commit_many(later, [f] * n)
            if [ctx.tracker_position(t) for t in now] != [ctx.tracker_position(t) for t in later]:
                bad.append((case.name, i, "position after the commit"))
        for a, b in zip(now, later):
            d = _diff(_state(ctx, b), _state(ctx, a))
            if d:
                bad.append((case.name, "state after the commits", d))
        ctx.tracker_destroy_many(now + later)
    assert not bad, bad[:20]


CLONE_CASES = ("box_cross_left", "box_outside_near", "box_outside_far", "box_strip_7px", "box_levels_3", "box_inverted", "picture_then_black",
               "start_on_black", "reenter_a", "reenter_c", "shift_right_30")


def test_clones_before_and_after_one_side_writes(ctx, small_video):
    cases = {c.name: c for c in tc.small_cases(small_video)}
    for name in CLONE_CASES:
        case = cases[name]
        n = len(case.boxes)
        f0, f1, f2 = case.frames[0], case.frames[1], case.frames[2]
        alone = ctx.tracker_create_many(n)                       # never cloned: what each side must equal
        src = ctx.tracker_create_many(n)
        for t in (alone, src):
            ctx.tracker_start_many(t, [f0] * n, case.boxes)
        twin = ctx.tracker_clone_many(src)
        s0 = [_state(ctx, t) for t in src]
        assert all(not _diff(_state(ctx, t), s) for t, s in zip(twin, s0)), name
        assert [ctx.tracker_position(t) for t in twin] == [ctx.tracker_position(t) for t in src]
        # both sides read the shared filters in one deferred call
        pa, ba = ctx.tracker_update_many(alone, [f1] * n)
        pd, bd = ctx.tracker_update_many(src + twin, [f1] * (2 * n), defer=True)
        assert _same_psr(pd[:n], pa) and _same_psr(pd[n:], pa), name
        assert np.array_equal(bd[:n], ba) and np.array_equal(bd[n:], ba), name
        # one side writes: the other keeps what it had
        ctx.tracker_commit_many(src, [f1] * n)
        assert all(not _diff(_state(ctx, t), s) for t, s in zip(twin, s0)), name
        assert all(not _diff(_state(ctx, t), _state(ctx, a)) for t, a in zip(src, alone)), name
        ctx.tracker_commit_many(twin, [f1] * n)
        assert all(not _diff(_state(ctx, t), _state(ctx, a)) for t, a in zip(twin, alone)), name
        pa, ba = ctx.tracker_update_many(alone, [f2] * n)
        for side in (src, twin):
            p, b = ctx.tracker_update_many(side, [f2] * n)
            assert _same_psr(p, pa) and np.array_equal(b, ba), name
            assert all(not _diff(_state(ctx, t), _state(ctx, a)) for t, a in zip(side, alone)), name
        ctx.tracker_destroy_many(alone + src + twin)


MIXED = ("box_outside_far", "box_levels_3", "box_cross_left", "box_strip_7px", "box_levels_4", "box_px1", "box_outside_near", "box_levels_2",
         "box_strip_collapses_later", "box_whole_frame", "box_levels_1", "box_inverted", "box_outside_negative", "box_larger_than_frame")


def test_one_mixed_batch_equals_one_call_per_tracker(ctx, small_video):
    """empty chips, level-0 chips and chips of three and four pyramid levels in ONE call (the padding of chip_extract_batch's level
    tables to the deepest pyramid of the batch) against the same trackers one per call"""
    cases = {c.name: c for c in tc.small_cases(small_video)}
    boxes = [cases[name].boxes[0] for name in MIXED]
    frames = cases[MIXED[0]].frames
    plans = [tc.chip_levels(tc.tracker_rect(b), *tc.SMALL) for b in boxes]
    assert any(p["empty"] for p in plans) and any(p["levels"] == 0 and not p["empty"] for p in plans)
    assert any(p["levels"] >= 3 and not p["collapsed"] for p in plans) and any(p["collapsed"] for p in plans)
    n = len(boxes)
    batch, single = ctx.tracker_create_many(n), ctx.tracker_create_many(n)
    ctx.tracker_start_many(batch, [frames[0]] * n, boxes)
    for t, b in zip(single, boxes):
        ctx.tracker_start_many([t], [frames[0]], [b])
    for a, b in zip(batch, single):
        assert not _diff(_state(ctx, a), _state(ctx, b))
    for f, defer in ((frames[1], True), (frames[2], False)):    # a deferred update with its commit, then an immediate one
        pb, bb = ctx.tracker_update_many(batch, [f] * n, defer=defer)
        one = [ctx.tracker_update_many([t], [f], defer=defer) for t in single]
        assert _same_psr(pb, [p[0] for p, _ in one])
        assert np.array_equal(bb, np.stack([b[0] for _, b in one]))
        if defer:
            ctx.tracker_commit_many(batch, [f] * n)
            for t in single:
                ctx.tracker_commit_many([t], [f])
        for a, b in zip(batch, single):
            assert not _diff(_state(ctx, a), _state(ctx, b))
    ctx.tracker_destroy_many(batch + single)


def test_bad_start_boxes_are_refused_and_nothing_changes(ctx, oracle, small_video, tables):
    from pyannote_video_amd import _lib
    f0, f1, f2 = small_video.frame(0), small_video.frame(1), small_video.frame(2)
    good = tc.face_boxes(small_video, 0)[0]
    other = (200.0, 100.0, 320.0, 220.0)
    ref = oracle.Tracker(tables)
    ref.start_track(f0, good)
    started, fresh = ctx.tracker_create_many(2)
    ctx.tracker_start_many([started], [f0], [good])
    psr, _ = ctx.tracker_update_many([started], [f1])
    assert psr[0] == ref.update(f1)
    pos, state = ctx.tracker_position(started), _state(ctx, started)
    for box in tc.REFUSED_BOXES:
        for trks, boxes in (([started], [box]), ([started, fresh], [other, box]), ([fresh, started], [box, other])):
            with pytest.raises(_lib.PvfError):
                ctx.tracker_start_many(trks, [f0] * len(trks), boxes)
            assert ctx.tracker_position(started) == pos == ref.get_position()
            assert not _diff(_state(ctx, started), state)
            with pytest.raises(_lib.PvfError):                   # the other tracker of a refused call was not started
                ctx.tracker_update_many([fresh], [f1])
    # the context and both trackers keep working: an ordinary update, start and update equal the oracle
    psr, box = ctx.tracker_update_many([started], [f2])
    assert psr[0] == ref.update(f2) and tuple(box[0]) == ref.get_position()
    assert not _diff(_state(ctx, started), _ref_state(ref))
    ref2 = oracle.Tracker(tables)
    ref2.start_track(f0, other)
    ctx.tracker_start_many([fresh], [f0], [other])
    psr, box = ctx.tracker_update_many([fresh], [f1])
    assert psr[0] == ref2.update(f1) and tuple(box[0]) == ref2.get_position()
    assert not _diff(_state(ctx, fresh), _ref_state(ref2))
    ctx.tracker_destroy_many([started, fresh])


@pytest.mark.parametrize("every_frames", [0, 3])
def test_pipeline_on_a_clip_whose_faces_leave_and_that_fades_to_black(ctx, oracle, small_video, model_paths, tables, every_frames):
    """FacePipeline.run against the reference's sequential flow on a clip in which the faces slide out through the right edge, five
    black frames follow and the picture returns: trackers run partly off the frame, and through the black frames on NaN confidences
    (tracking.py:204 keeps them), in both passes"""
    import math
    from pyannote_video_amd import models, pipeline
    from oracle import ref_flow
    frames = tc.sliding_clip(small_video)
    n, rate = len(frames), small_video.frame_rate
    times = [i / rate for i in range(n)]
    shots = [(0.0, n / rate)]
    every = every_frames / rate
    det = oracle.Detector(models.load_container(models.DEFAULT_DETECTOR))
    found = {}

    def detect(f):
        if id(f) not in found:
            found[id(f)] = det(f, 1)
        return found[id(f)]
    log = []
    ref_tracks = ref_flow.track_video(frames, times, shots, detect, tc.recording_tracker(oracle, tables, log), rate, detect_every=every,
                                      min_conf=10., ratio=0.5, max_gap=1.0)
    w, h = tc.SMALL
    assert any(math.isnan(c) for c, _ in log)
    assert any(not c < 10. and p[0] < w - 1 < p[2] for c, p in log)              # a tracker that lives on, partly beyond the right edge
    assert any("forward" in st or "backward" in st for tr in ref_tracks for _, _, st in tr)
    pipe = pipeline.FacePipeline(ctx, model_paths[0], model_paths[1], detect_every=every, detect_batch_size=4)
    res = pipe.run([ctx.upload(f) for f in frames], times, rate, shots, cluster=False)
    assert res["tracks"] == ref_tracks
