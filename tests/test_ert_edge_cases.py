"""CPU: the landmark edge-case table (tests/ert_cases.py) does what it claims, on the oracle (oracle/pvo_ert.c) and its numpy restatement
(tests/ert_ref.py) alone -- no GPU, no library call.  tests/test_gpu_ert_edges.py then holds csrc/ert.hip: ert_k to the oracle on the same
table; what is shown here is that such a comparison, float shape bit for bit and integer points, would see a kernel that is subtly wrong.

  * the restatement equals the oracle on EVERY row (12 models x 305 faces: the vectors of the restatement run over the 136 coordinates and
    over independent trees, so no row is too large to loop over), floats bit for bit and integers;
  * the table reaches every seam of the kernel, counted from the restatement's own trace;
  * ten planted defects each change the float shape or the integer points on a row that the test names;
  * collapsed landmarks (a zero-area box) give NaN chip details, a black chip and a finite descriptor in the oracle, and the library's
    chip_plan, compiled for the host under UBSan, answers NaN details with the empty job (tests/csrc/chip_plan_check.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ert_cases as ec
import ert_ref as er

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def table(small_video):
    return ec.frames(small_video), ec.faces(small_video)


@pytest.fixture(scope="module")
def runs(table, oracle):
    """{model name: (Trace, [(points, shape)] of the restatement, [(points, shape)] of the oracle)}, computed once per model"""
    frames, faces = table
    cache = {}

    def get(name):
        if name not in cache:
            t = ec.tensors(name)
            sp = oracle.ShapePredictor(t)
            trace = er.Trace()
            mine = [er.landmarks(t, frames[f], b, trace=trace) for f, _, b in faces]
            theirs = [sp.shape_f32(frames[f], b) for f, _, b in faces]
            cache[name] = (trace, mine, theirs)
        return cache[name]
    return get


@pytest.mark.parametrize("model", ec.MODELS, ids=repr)
def test_restatement_equals_the_oracle_on_every_row(table, runs, oracle, model):
    _, faces = table
    _, mine, theirs = runs(model.name)
    assert len(faces) >= 300
    bad = [(f, c) for (f, c, _), (p, s), (wp, ws) in zip(faces, mine, theirs) if not (np.array_equal(p, wp) and er.same_bits(s, ws))]
    assert not bad, bad[:10]
    # pvo_landmarks is pvo_landmarks_f32 without the floats
    sp = oracle.ShapePredictor(ec.tensors(model.name))
    frames = table[0]
    for (f, c, b), (wp, _) in list(zip(faces, theirs))[::7]:
        assert np.array_equal(sp(frames[f], b), wp), (f, c)


def test_the_model_rows_cover_the_kernels_geometry():
    """ert_k: the leaf sum takes trees twenty at a time, then one by one; 256 lanes stride over trees and pixels; LDS is carved at
    (n_pix + 3) & ~3; load_shape accepts depth 1 .. 6 (the table has the shallowest, the usual and the deepest) and up to 1024 pixels"""
    trees = {m.n_trees for m in ec.MODELS}
    pix = {m.n_pix for m in ec.MODELS}
    assert {t % 20 for t in trees} >= {0, 1, 19}
    assert any(t < 20 for t in trees) and any(t > 256 for t in trees) and any(t > 256 and t % 20 for t in trees)
    assert any(p < 256 for p in pix) and any(p > 256 for p in pix) and 1024 in pix and 1 in pix
    assert {p % 4 for p in pix} >= {0, 1, 3}
    assert {m.depth for m in ec.MODELS} == {1, 4, 6}
    assert {m.n_cascades for m in ec.MODELS} >= {1, 3}
    assert sum(not m.integer_thresholds for m in ec.MODELS) == 1
    assert any(m.leaf_sigma >= 100 * 2e-4 for m in ec.MODELS)
    for m in ec.MODELS:
        assert m.leaf_mib() <= 32 and (m.n_cascades <= 2 or not (m.n_trees > 256 and m.depth == 6)), m


@pytest.mark.parametrize("model", ec.MODELS, ids=repr)
def test_every_seam_is_reached(runs, model):
    """each count comes from the restatement's trace of the rows themselves; all of them are required above zero"""
    tr, mine, _ = runs(model.name)
    print(model, "splits", tr.splits, "ties", tr.ties, "off-frame", tr.off, "on-frame", tr.inside, "last row / column", tr.last_row, tr.last_col,
          "final coordinates on .5", tr.half, "saturated high / low", tr.sat_hi, tr.sat_lo, "max |u|, |v|", tr.max_uv, "deepest leaf", tr.max_leaf)
    if model.integer_thresholds:
        assert tr.ties > 0                                     # diff == thresh: what tells > from >=
    for side in ("left", "right", "top", "bottom"):
        assert tr.off[side] > 0, side
    assert tr.inside > 0 and tr.last_row > 0 and tr.last_col > 0
    assert tr.half > 0                                         # floor(x + 0.5) with x on the boundary (the box of side 2^24)
    assert tr.sat_hi > 0 and tr.sat_lo > 0
    assert tr.max_leaf == (1 << model.depth) - 1               # the walk reaches the last leaf: every level went right at least once
    # (long)floor(u * (right - left) + left + 0.5) is defined: |u| < 2^20 and |right - left| < 2^32 keep it far inside 2^63
    assert tr.max_uv < float(1 << 20)


def test_the_wandering_model_leaves_the_box(runs):
    assert runs("c3_t40_p120_d4_wander")[0].max_uv > 1.6 > runs("c3_t40_p120_d4")[0].max_uv


def test_zero_area_boxes_give_68_identical_points(table, runs):
    _, faces = table
    seen = 0
    for name in ("c3_t40_p120_d4", "c3_t40_p120_d4_wander", "c2_t300_p257_d6"):
        _, _, theirs = runs(name)
        for (f, c, b), (p, s) in zip(faces, theirs):
            if c in ec.ZERO_AREA:
                assert b[0] == b[2] and b[1] == b[3]
                assert (p == np.array([b[0], b[1]])).all(), (name, f, c)
                seen += 1
            elif c == "zero_width":
                assert (p[:, 0] == b[0]).all() and len(set(p[:, 1].tolist())) > 1
            elif c == "zero_height":
                assert (p[:, 1] == b[1]).all() and len(set(p[:, 0].tolist())) > 1
    assert seen >= 3 * 20


def test_saturation_decides_at_the_int32_extremes(table, runs):
    _, faces = table
    _, _, theirs = runs("c3_t40_p120_d4")
    hi = lo = 0
    for (f, c, b), (p, s) in zip(faces, theirs):
        if c in ec.SATURATING:
            hi += int((p == ec.I32_MAX).sum()); lo += int((p == ec.I32_MIN).sum())
            X = s[:, 0].astype(np.float64) * (float(b[2]) - float(b[0])) + float(b[0])
            assert ((p[:, 0] == ec.I32_MAX) == (np.floor(X + 0.5) >= ec.I32_MAX)).all(), (f, c)       # never the wrapped value
            assert ((p[:, 0] == ec.I32_MIN) == (np.floor(X + 0.5) <= ec.I32_MIN)).all(), (f, c)
    assert hi > 0 and lo > 0


# the row on which each planted defect is seen: (model, frame, box class, what differs)
DEFECT_ROWS = {
    "ge": ("c3_t40_p120_d4", "video0", "inside", "shape"),
    "half_even": ("c3_t40_p120_d4", "video0", "dwarfing_2p24", "points"),
    "clamp_pixel": ("c3_t40_p120_d4", "video0", "cross_left", "shape"),
    "rounded_gray": ("c3_t40_p120_d4", "truncating", "inside", "shape"),
    "pairwise": ("c3_t40_p120_d4", "video0", "dwarfing", "points"),
    "reversed": ("c3_t40_p120_d4", "video0", "dwarfing", "points"),
    "drop_tail": ("c3_t21_p257_d4", "video0", "inside", "shape"),
    "fit_f32": ("c3_t40_p120_d4", "strip_2x1000000", "strip_dwarfing", "shape"),
    "prev_anchor": ("c3_t40_p120_d4", "video0", "inside", "shape"),
    "unsaturated": ("c3_t40_p120_d4", "video0", "i32_right", "points"),
}


@pytest.mark.parametrize("defect", sorted(er.DEFECTS))
def test_the_comparison_sees_a_planted_defect(table, defect):
    frames, faces = table
    model, fname, cls, what = DEFECT_ROWS[defect]
    t = ec.tensors(model)
    box = next(b for f, c, b in faces if f == fname and c == cls)
    p, s = er.landmarks(t, frames[fname], box)
    dp, ds = er.landmarks(t, frames[fname], box, defect=defect)
    print(defect, "(%s) on %s %s/%s: shape differs %s (max %g), points differ %s" % (er.DEFECTS[defect], model, fname, cls, not er.same_bits(s, ds),
                                                                                      np.abs(s.astype(np.float64) - ds).max(), not np.array_equal(p, dp)))
    if what == "shape":
        assert not er.same_bits(s, ds)
    else:
        assert not np.array_equal(p, dp)


def test_order_defects_show_in_the_floats_of_an_ordinary_box_only(table):
    """why the float shape is compared at all: on a box inside the frame a pairwise or reversed leaf sum leaves every integer point where it
    was and changes the float shape by an ulp"""
    frames, faces = table
    t = ec.tensors("c3_t40_p120_d4")
    box = next(b for f, c, b in faces if f == "video0" and c == "inside")
    p, s = er.landmarks(t, frames["video0"], box)
    for defect in ("pairwise", "reversed"):
        dp, ds = er.landmarks(t, frames["video0"], box, defect=defect)
        assert np.array_equal(p, dp) and not er.same_bits(s, ds)
        assert np.abs(s.astype(np.float64) - ds).max() < 1e-6


def test_drop_tail_is_invisible_without_a_tail(table):
    """40 trees = two groups of twenty: the suite's only geometry before this table never entered the tail loop"""
    frames, faces = table
    t = ec.tensors("c3_t40_p120_d4")
    for f, c, b in faces[:30]:
        p, s = er.landmarks(t, frames[f], b)
        dp, ds = er.landmarks(t, frames[f], b, defect="drop_tail")
        assert np.array_equal(p, dp) and er.same_bits(s, ds)


# ---- collapsed landmarks -> chip ------------------------------------------------------------------------------------------------------------
def test_collapsed_landmarks_give_nan_details_a_black_chip_and_a_finite_descriptor(oracle, model_paths, small_video):
    from pyannote_video_amd import models
    emb = oracle.Embedder(models.load_container(model_paths[1]))
    f = small_video.frame(0)
    pts = np.tile(np.array([[100, 100]], np.int32), (68, 1))
    rect, cs, sn = emb.chip_details(pts)
    assert rect == (100.0, 100.0, 100.0, 100.0) and np.isnan(cs) and np.isnan(sn)
    chip = emb.chip(f, pts)
    assert chip.shape == (150, 150, 3) and not chip.any()
    d = emb.forward(chip)
    assert np.isfinite(d).all() and np.array_equal(d, emb.forward(np.zeros((150, 150, 3), np.uint8)))


def test_chip_plan_answers_nan_details_with_the_empty_job(tmp_path):
    """csrc/chip_plan.h compiled for the host with a main of its own, under UBSan with float-cast-overflow: NaN or infinite details give the
    empty job (before: (int)floor(NaN), and a chip that was black only because transform_k's guard is a negated comparison); every other
    plan, from boxes of 1e-300 to 1e300 pixels on frames from 1 x 1 to 2 x 1000000, is empty or inside [0, w) x [0, h)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "chip_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                           "-I", os.path.join(HERE, "..", "pyannote-video_amd", "csrc"), "-o", exe, os.path.join(HERE, "csrc", "chip_plan_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-800:], out.stderr[-800:])
    assert " 0 failures" in out.stdout
