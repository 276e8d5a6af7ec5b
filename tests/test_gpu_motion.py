"""GPU: the `motion` verb's kernel (csrc/motion.hip) against MOTION.md as tests/motion_ref.py restates it, with np.array_equal: the rows of
the caller's own flows over the sizes, contents and pair counts of tests/motion_cases.py (whose reach tests/test_motion_ref.py proves on
the CPU), the rows of resident frames against the restatement on the oracle's flows with pvf_shot_dfd unchanged beside them, every
refusal, and the two verbs in processes of their own."""
import json
import os
import subprocess
import sys

import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships
import numpy as np
import pytest

import shot_cases as sc
from tests import motion_cases as mc, motion_ref as mr
from tests.test_gpu_faces import bare_ctx      # noqa: F401 -- fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want, what=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "%d differ, first at %s: %s against %s" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


@pytest.fixture(scope="module")
def tables():
    from pyannote_video_amd import structure
    return structure.shot_tables()


# ---- pvf_flow_motion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", mc.SIZES, ids=lambda v: str(v))
def test_rows_of_every_content(bare_ctx, w, h):
    flows = np.stack([mc.reference(c, w, h)[0] for c in mc.CONTENTS])
    want = np.stack([mc.reference(c, w, h)[1] for c in mc.CONTENTS])
    got = bare_ctx.flow_motion(flows)                               # every content in one call
    for k, c in enumerate(mc.CONTENTS):
        _same(got[k], want[k], (c, w, h))
    _same(bare_ctx.flow_motion(flows[:1]), want[:1], "one pair")
    _same(bare_ctx.flow_motion(flows[3:5]), want[3:5], "two pairs")
    _same(bare_ctx.flow_motion(flows[::-1]), want[::-1], "another order")
    assert not got[:, 7].any() and not got[:, 8].any() and (got[:, 9] == (w | h << 16)).all()


def test_three_hundred_pairs_in_one_call(bare_ctx):
    w, h = 13, 17
    kinds = ("noise", "nonfinite", "ties")
    flows = np.stack([mc.flow_of(kinds[k % 3], w, h, seed=k) for k in range(300)])      # more than a round of 256, every pair different
    want = mr.rows_of(flows)
    assert len(set(r.tobytes() for r in want)) == 300
    _same(bare_ctx.flow_motion(flows), want, "300 pairs")
    _same(bare_ctx.flow_motion(flows[:257]), want[:257], "a round and one pair")
    assert bare_ctx.flow_motion(flows[:0]).shape == (0, 10)


def test_the_call_again_after_other_work(bare_ctx, tables):
    w, h = 96, 54
    flows = np.stack([mc.reference(c, w, h)[0] for c in ("noise", "planted37", "clip")])
    want = np.stack([mc.reference(c, w, h)[1] for c in ("noise", "planted37", "clip")])
    _same(bare_ctx.flow_motion(flows), want, "before")
    frames = [bare_ctx.upload(f) for f in mc.camera_clip(still=2, pan=2, zoom=0).frames]
    bare_ctx.frame_blend(frames, 64, 36)                            # the same scratch buffer, carved another way
    bare_ctx.shot_dfd(frames, 96, 54, tables, want_flow=True)
    bare_ctx.shot_motion(frames, 96, 54, tables)
    for f in frames:
        f.release()
    big = mc.reference("worst_pp", 128, 128)
    _same(bare_ctx.flow_motion(big[0][None]), big[1][None], "a larger one")
    _same(bare_ctx.flow_motion(flows), want, "after")


# ---- pvf_shot_motion ------------------------------------------------------------------------------------------------------------------
# geometries of tests/shot_cases.py whose small image lies within the caps: no coarser level (12 x 12, 50 x 88 with the whole content set,
# frames reduced by a non-integer factor) and one (64 x 64 with the whole content set, 65 x 65, frames enlarged onto 65 x 67)
SHOT_CASES = ("content_12x12", "content_50x88", "convert_down_noninteger", "content_64x64", "content_65x65", "convert_up_both_levels")


@pytest.mark.parametrize("name", SHOT_CASES)
def test_rows_of_resident_frames(ctx, oracle, tables, name):
    c = sc.case(name)
    assert oracle.farneback_levels(c.oh, c.ow) == (0 if name in SHOT_CASES[:3] else 1)
    ref = sc.oracle_results(c, oracle, tables)
    want = mr.rows_of(ref["flow"], ref["dfd"])                      # the restatement on the oracle's flows
    frames = c.frames()[:64]                                        # the table's pairs are the frames (2 i, 2 i + 1)
    p = len(frames) // 2
    before = ctx.shot_dfd(frames, c.ow, c.oh, tables, want_gray=True, want_flow=True)
    rows, dfd = ctx.shot_motion(frames, c.ow, c.oh, tables)
    after = ctx.shot_dfd(frames, c.ow, c.oh, tables, want_gray=True, want_flow=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    assert rows.shape == (len(frames) - 1, 10) and dfd.tobytes() == before[0].tobytes()
    _same(rows[0::2], want[:p], name)
    _same(rows[:, 7], dfd.view(np.int64), "word 7")
    _same(rows, mr.rows_of(before[2], before[0]), "the pairs in between, on the library's own flow")
    assert dfd[0::2].tolist() == ref["dfd"][:p].tolist()
    only_rows, none = ctx.shot_motion(frames, c.ow, c.oh, tables, want_dfd=False)
    assert none is None
    _same(only_rows, rows, "without dfd")
    _same(ctx.shot_motion(frames[:2], c.ow, c.oh, tables)[0], rows[:1], "two frames")
    for n in (0, 1):
        r, d = ctx.shot_motion(frames[:n], c.ow, c.oh, tables)
        assert r.shape == (0, 10) and d.shape == (0,)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(bare_ctx, tables):
    from pyannote_video_amd import _lib
    c, l, P_ = bare_ctx, bare_ctx._l, _lib.ptr
    flows = np.stack([mc.reference("noise", 13, 17)[0]] * 2)
    want = np.stack([mc.reference("noise", 13, 17)[1]] * 2)
    SENTINEL = 0x5A5A5A5A5A5A5A5A
    out = np.full((2, 10), SENTINEL, np.int64)

    def fit(flow=flows, n=2, h=17, w=13, r=out):
        return l.pvf_flow_motion(c._h, P_(flow), n, h, w, P_(r))
    for kw, message in ((dict(n=-1), "negative count"), (dict(w=11), "a side outside"), (dict(h=11), "a side outside"), (dict(w=257), "a side outside"),
                        (dict(h=257, w=12), "a side outside"), (dict(w=0), "a side outside"), (dict(h=-17), "a side outside"),
                        (dict(h=129, w=128), "PVF_MOTION_MAX_PIXELS"), (dict(h=256, w=65), "PVF_MOTION_MAX_PIXELS"),
                        (dict(flow=None), "null flow or rows"), (dict(r=None), "null flow or rows")):
        assert fit(**kw) != 0, message
        assert message in l.pvf_last_error().decode(), (message, l.pvf_last_error().decode())
        assert (out == SENTINEL).all()                              # refused before any work
        assert fit() == 0 and np.array_equal(out, want)             # the context goes on
        out[:] = SENTINEL
    assert l.pvf_flow_motion(c._h, None, 0, 17, 13, None) == 0      # nothing to fit is legal
    with pytest.raises(ValueError, match="float32"):
        c.flow_motion(np.zeros((2, 12, 12), np.float32))
    # resident frames
    f = mc.camera_clip(still=1, pan=1, zoom=0).frames
    a, b, other, gone = c.upload(f[0]), c.upload(f[1]), c.upload(np.ascontiguousarray(f[0][:-1])), c.upload(f[0])
    gone_handle = gone.handle
    gone.release()
    hs = np.array([a.handle, b.handle], np.uint64)
    ref_rows, ref_dfd = c.shot_motion([a, b], 24, 14, tables)
    rows, dfd = np.full((1, 10), SENTINEL, np.int64), np.full(1, -7.0)

    def call(frames=hs, n=2, w=24, h=14, t=tables, r=rows, d=dfd):
        return l.pvf_shot_motion(c._h, P_(frames), n, w, h, P_(t), P_(r), P_(d))
    for kw, message in ((dict(n=-1), "negative count"), (dict(w=11), "a side outside"), (dict(h=11), "a side outside"), (dict(w=257), "a side outside"),
                        (dict(w=128, h=129), "PVF_MOTION_MAX_PIXELS"), (dict(frames=None), "null frames, tables or rows"),
                        (dict(t=None), "null frames, tables or rows"), (dict(r=None), "null frames, tables or rows"),
                        (dict(frames=np.array([a.handle, 987654321], np.uint64)), "unknown frame handle"),
                        (dict(frames=np.array([gone_handle, a.handle], np.uint64)), "unknown frame handle"),
                        (dict(frames=np.array([a.handle, other.handle], np.uint64)), "frames of different sizes")):
        assert call(**kw) != 0, message
        assert message in l.pvf_last_error().decode(), (message, l.pvf_last_error().decode())
        assert (rows == SENTINEL).all() and dfd[0] == -7.0
        assert call() == 0 and np.array_equal(rows, ref_rows) and dfd.tobytes() == ref_dfd.tobytes()
        rows[:] = SENTINEL
        dfd[:] = -7.0
    assert call(d=None) == 0 and np.array_equal(rows, ref_rows) and dfd[0] == -7.0      # dfd is optional
    assert l.pvf_shot_motion(c._h, None, 0, 24, 14, None, None, None) == 0 and call(n=1, r=None, d=None) == 0
    for d in (a, b, other):
        d.release()
    with pytest.raises(ValueError, match="22 floats"):
        c.shot_motion([], 24, 14, tables[:21])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_the_verbs_in_processes_of_their_own(tmp_path):
    from tests import yuv_ref
    from tests.test_motion_ref import check_labels
    clip = mc.camera_clip()
    tw, th = mr.tile_size(mc.CLIP_WIDTH, mc.CLIP_W, mc.CLIP_H)
    video, rows_a, rows_b, out_a, out_b, y4m = (str(tmp_path / n) for n in ("clip.npy", "a.npy", "b.npy", "a.json", "b.json", "clip.y4m"))
    np.save(video, np.stack(clip.frames))
    planes = [yuv_ref.from_rgb(f, "420") for f in clip.frames]
    yuv_ref.write_y4m(y4m, planes, rate="25:1")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pyannote-video_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for args, stdin in ((["motion", "--batch", "7", video, rows_a], None), (["camera", rows_a, out_a], None),
                        (["motion", "-", rows_b], y4m), (["camera", rows_b, out_b], None)):
        with open(stdin or os.devnull, "rb") as fi:
            run = subprocess.run([sys.executable, "-m", "pyannote_video_amd", "--fps", str(mc.FPS)] + args, stdin=fi, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, env=env, timeout=600)
        assert run.returncode == 0, (args, run.stderr.decode()[-2000:])
    want = mc.oracle_rows(clip.frames, tw, th)
    _same(np.load(rows_a), want)
    found = json.load(open(out_a))
    assert found == mr.camera_report(want)
    check_labels(found, clip.parts)
    rgb = [yuv_ref.to_rgb(*p) for p in planes]
    want = mc.oracle_rows(rgb, tw, th)
    _same(np.load(rows_b), want)
    found = json.load(open(out_b))
    assert found == mr.camera_report(want)
    check_labels(found, clip.parts)
