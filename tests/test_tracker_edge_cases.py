"""CPU: the tracker's edge-case table (tests/tracker_cases.py) does what it claims -- on the oracle alone.  tests/test_gpu_tracker_edges.py
runs the library over the SAME table, so what is proven here is what is tested there: a NaN confidence, a correlation peak on the
map's border, a clipped PSR window, scale peaks at both ends of the 32 scales, the refused sub-pixel step, blank frames, boxes beside and
beyond the frame.  Conditions, not tolerances.  Reference: pyannote/video/tracking.py:203 (confidence = tracker.update(frame)),
:204-206 (`if confidence < self.track_min_confidence`), :250-251 (start_track).

The `det == 0` return of the sub-pixel step is not in the table: it needs an interior arg-max whose 3 x 3 neighbourhood has an exactly
singular quadratic fit, and every flat map (the only exact cancellation blank frames give) has its arg-max at index 0, on the border,
where the step is skipped.  Scans of several hundred off-frame starts, noise frames and tiny boxes never met it; the other early return
(`dx * k2 + dy * k3 < 0`) is met by case reenter_c."""
import math

import numpy as np
import pytest

import tracker_cases as tc
from test_host_logic import ModelScriptTracker
from test_shotgraph import _both


@pytest.fixture(scope="module")
def tables():
    from pyannote_video_amd import models
    return models.dsst_tables()


@pytest.fixture(scope="module")
def small_runs(oracle, small_video, tables):
    return [(c, tc.run_oracle(c, oracle, tables)) for c in tc.small_cases(small_video)]


@pytest.fixture(scope="module")
def full_runs(oracle, tables):
    return [(c, tc.run_oracle(c, oracle, tables)) for c in tc.full_cases()]


def test_box_table_covers_every_class():
    for boxes, (w, h), required in ((tc.small_boxes(), tc.SMALL, tc.REQUIRED_BOX_CLASSES), (tc.full_boxes(), tc.FULL, tc.REQUIRED_BOX_CLASSES_FULL)):
        seen = set()
        for _, box in boxes:
            seen |= tc.box_class(box, w, h)
        assert not (required - seen), sorted(required - seen)
    # the pyramid classes hold for the rectangles they were written for (the 1.4x rectangle of the named box)
    named = dict(tc.small_boxes())
    for name, levels in (("levels_1", 1), ("levels_2", 2), ("levels_3", 3), ("levels_4", 4), ("cross_left", 0)):
        assert tc.chip_levels(tc.tracker_rect(named[name]), *tc.SMALL)["levels"] == levels, name
    p = tc.chip_levels(tc.tracker_rect(named["strip_7px"]), *tc.SMALL)
    assert p["levels"] == 1 and p["sw"] == 7 and p["collapsed"] and not p["empty"]
    p = tc.chip_levels(tc.tracker_rect(named["strip_collapses_later"]), *tc.SMALL)
    assert p["levels"] == 3 and p["sw"] > 8 and p["collapsed"]
    assert tc.chip_levels(tc.tracker_rect(named["outside_far"]), *tc.SMALL)["empty"]


def test_chip_levels_restatement_equals_the_oracles_chip(oracle, small_video):
    """the restated plan predicts what the oracle's chip does: black exactly when the plan is empty or its pyramid runs out"""
    f = small_video.frame(0)
    for name, box in tc.small_boxes():
        rect = tc.tracker_rect(box)
        plan = tc.chip_levels(rect, *tc.SMALL)
        chip = oracle.extract_chip(f, rect, 1.0, 0.0, tc.CHIP, tc.CHIP)
        if plan["empty"] or plan["collapsed"]:
            assert not chip.any(), name
        else:
            assert chip.any(), name


def _updates(runs):
    for case, recs in runs:
        for k, rec in enumerate(recs):
            for i, last in enumerate(rec["last"]):
                yield case, k, i, rec["psr"][i], rec["pos"][i], last


def test_table_meets_every_condition_on_the_oracle(small_runs):
    seen = set()
    for case, k, i, psr, pos, last in _updates(small_runs):
        px, py = last["ipx"], last["ipy"]
        on_border = px < 1 or py < 1 or px > 62 or py > 62
        assert on_border == (last["how"] == "border")
        if math.isnan(psr):
            seen.add("nan_psr")
        if on_border:
            seen.add("peak_on_border")
            if not math.isnan(psr):
                seen.add("peak_on_border_with_a_number")
        rx, ry = int(math.floor(last["ppx"] + 0.5)), int(math.floor(last["ppy"] + 0.5))
        if rx - 4 < 0 or ry - 4 < 0 or rx + 3 > 63 or ry + 3 > 63:
            seen.add("psr_window_clipped")
            if not math.isnan(psr):
                seen.add("psr_window_clipped_with_a_number")
        if last["bk"] == 0:
            seen.add("bk_0")
        if last["bk"] == 31:
            seen.add("bk_31")
            if not math.isnan(psr):
                seen.add("bk_31_with_a_number")
        if 0 < last["bk"] < 31 and last["spos"] != last["bk"]:
            seen.add("bk_inside_interpolated")
        if last["how"] == "taken":
            seen.add("step_taken")
        if last["how"] == "against":
            seen.add("step_against_the_gradient")
        w, h = case.size
        if (pos[0] < 0 or pos[1] < 0 or pos[2] > w - 1 or pos[3] > h - 1) and not math.isnan(psr) and psr > 10:
            seen.add("confident_partly_off_frame")
    want = {"nan_psr", "peak_on_border", "peak_on_border_with_a_number", "psr_window_clipped", "psr_window_clipped_with_a_number", "bk_0", "bk_31",
            "bk_31_with_a_number", "bk_inside_interpolated", "step_taken", "step_against_the_gradient", "confident_partly_off_frame"}
    assert not (want - seen), sorted(want - seen)


@pytest.mark.parametrize("which", ["small", "full"])
def test_every_state_stays_finite(which, request):
    runs = request.getfixturevalue(which + "_runs")
    for case, recs in runs:
        for k, rec in enumerate(recs):
            assert np.isfinite(rec["pos"]).all(), (case, k)
            for name in ("A", "B", "As", "Bs"):
                assert np.isfinite(rec[name]).all(), (case, k, name)
            assert not np.isinf(rec["psr"]).any(), (case, k)


def test_full_size_subset_meets_its_conditions(full_runs):
    seen = set()
    for case, k, i, psr, pos, last in _updates(full_runs):
        if math.isnan(psr):
            seen.add("nan_psr")
        if last["how"] == "border":
            seen.add("peak_on_border")
        if last["how"] == "taken" and psr > 10:
            seen.add("tracked")
    assert seen == {"nan_psr", "peak_on_border", "tracked"}


def test_black_run_shrinks_the_box_to_nothing_and_back(small_runs):
    (case, recs), = [r for r in small_runs if r[0].name == "fade_black_run"]
    rec = recs[0]
    assert len(rec["psr"]) == tc.BLACK_RUN + 2
    assert np.isnan(rec["psr"][:tc.BLACK_RUN]).all()
    assert all(l["ipx"] == 0 and l["ipy"] == 0 and l["bk"] == 0 for l in rec["last"][:tc.BLACK_RUN])
    w0 = case.boxes[0][2] - case.boxes[0][0]
    assert rec["pos"][0][2] - rec["pos"][0][0] == pytest.approx(w0 * 1.02 ** -16, rel=1e-6)      # 0.73 per black frame
    width = rec["pos"][tc.BLACK_RUN - 1][2] - rec["pos"][tc.BLACK_RUN - 1][0]
    assert 0 <= width < 1e-9
    assert np.isfinite(rec["pos"]).all()


# ---- a NaN confidence keeps the tracker (tracking.py:204: `if confidence < self.track_min_confidence` is False for NaN)
def _special(value):
    class T(ModelScriptTracker):
        def update(self, frame):
            conf = ModelScriptTracker.update(self, frame)
            return value if frame.i % 3 == 1 else conf

    class R(T):
        def get_position(self):
            return self.box
    return T, R


def _same_edges(a, b):
    assert len(a) == len(b)
    for (u1, v1, c1), (u2, v2, c2) in zip(a, b):
        assert u1 == u2 and v1 == v2 and (c1 == c2 or (math.isnan(c1) and math.isnan(c2)))


@pytest.mark.parametrize("seed", range(4))
def test_nan_confidence_keeps_the_tracker_in_both_state_machines(seed):
    from oracle import ref_flow
    kw = dict(n=50, faces=3, p_miss=0.5, p_false=0.1, ratio=0.5, gap=1.0)
    out = {}
    for name, value in (("nan", float("nan")), ("kept", 12.0), ("killed", 3.0)):
        T, R = _special(value)
        cache, dets, (nat, py) = _both(700 + seed, tracker=T, **kw)
        for lane in (0, 1):
            _same_edges(nat[0][lane], py[0][lane])              # every add_edge call of both passes, library form == Python form
        assert nat[1] == py[1] and nat[3] == py[3]
        assert nat[1] == ref_flow.track_shot(cache, dets, R, 10., 0.5, 1.0)         # ... == the reference's flow
        out[name] = (nat[1], [c for lane in nat[0] for _, _, c in lane])
    assert any(math.isnan(c) for c in out["nan"][1])                                # NaN confidences did reach the comparison
    assert out["nan"][0] == out["kept"][0]                                          # and are kept, like a confidence above the threshold
    assert out["nan"][0] != out["killed"][0]                                        # (a low one on the same frames changes the tracks)


def test_oracle_refuses_the_boxes_the_library_refuses(oracle, small_video, tables):
    f = small_video.frame(0)
    t = oracle.Tracker(tables)
    t.start_track(f, (100.0, 100.0, 180.0, 180.0))
    t.update(small_video.frame(1))
    before = (t.get_position(), t.debug_state()[1].copy())
    for box in tc.REFUSED_BOXES:
        with pytest.raises(ValueError):
            t.start_track(f, box)
    assert t.get_position() == before[0] and np.array_equal(t.debug_state()[1], before[1])
    t.start_track(f, (180.0, 180.0, 100.0, 100.0))                                  # inverted corners stay accepted
    assert math.isfinite(t.update(small_video.frame(1))) and np.isfinite(t.get_position()).all()
