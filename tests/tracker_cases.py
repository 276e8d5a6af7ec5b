"""The tracker's edge-case table, shared by tests/test_tracker_edge_cases.py (CPU: the table does what it claims, on the oracle alone)
and tests/test_gpu_tracker_edges.py (GPU: the library equals the oracle on every case).  Deterministic builders only: boxes that cross,
touch, leave or dwarf the frame, and frame sequences in which the faces of the small clip slide out of the picture, change size, or
give way to blank frames.  Reference: pyannote/video/tracking.py:203,231,250-251 (dlib.correlation_tracker start_track / update /
get_position); dlib's chip pyramid rule is restated in chip_levels() below and never asks the library."""
import math

import numpy as np

SMALL = (640, 360)
FULL = (1920, 1080)
CHIP = 64                 # the translation chip is 64 x 64 of the box scaled by 1.4 about its centre
BLACK_RUN = 160


class Case(object):
    """start one tracker per box on frames[0], then update on frames[1:] in order"""

    def __init__(self, name, frames, boxes, size=SMALL):
        self.name, self.frames, self.boxes, self.size = name, frames, [tuple(float(v) for v in b) for b in boxes], size

    def __repr__(self):
        return self.name


# ---- dlib's extract_image_chip plan for an unrotated rectangle, restated (image_transforms/interpolation.h: chip_details,
# extract_image_chips; pyramid_down<2>::rect_down is p / 2 - (1.25, 0.75), its image loses (n - 3) / 2 and vanishes at n <= 8)
def _down(r):
    return (r[0] / 2.0 - 1.25, r[1] / 2.0 - 0.75, r[2] / 2.0 - 1.25, r[3] / 2.0 - 0.75)


def _area(r):
    return 0.0 if (r[0] > r[2] or r[1] > r[3]) else (r[2] - r[0]) * (r[3] - r[1])


def tracker_rect(box, scale=1.4):
    cx, cy = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2
    w, h = (box[2] - box[0]) * scale, (box[3] - box[1]) * scale
    return (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2)


def chip_levels(rect, w, h, rows=CHIP, cols=CHIP):
    """-> dict(empty, levels, sw, sh, collapsed): the source strip that is cropped from the frame, the number of pyramid_down<2> steps
    applied to it, and whether one of them runs out of pixels (then the chip is black)"""
    size = float(rows * cols)
    grow, r = 2.0, _down(rect)
    while _area(r) > size:
        r = _down(r)
        grow = grow * 2 + 2
    l, t = min(rect[0], rect[2]) - grow, min(rect[1], rect[3]) - grow
    rr, b = max(rect[0], rect[2]) + grow, max(rect[1], rect[3]) + grow
    l, t, rr, b = max(l, 0.0), max(t, 0.0), min(rr, w - 1.0), min(b, h - 1.0)
    out = dict(empty=True, levels=0, sw=0, sh=0, collapsed=False)
    if l > rr or t > b:
        return out
    x0, y0, x1, y1 = (int(math.floor(v + 0.5)) for v in (l, t, rr, b))
    sw, sh = x1 - x0 + 1, y1 - y0 + 1
    if sw <= 0 or sh <= 0:
        return out
    levels, r = 0, (rect[0] - x0, rect[1] - y0, rect[2] - x0, rect[3] - y0)
    while _area(_down(r)) > size:
        r = _down(r)
        levels += 1
    ph, pw, collapsed = sh, sw, False
    for _ in range(levels):
        ph, pw = (0, 0) if (ph <= 8 or pw <= 8) else ((ph - 3) // 2, (pw - 3) // 2)
        collapsed = collapsed or ph == 0 or pw == 0
    return dict(empty=False, levels=levels, sw=sw, sh=sh, collapsed=collapsed)


def _rot(cx, cy, x, y, cs, sn):
    dx, dy = x - cx, y - cy
    return cs * dx - sn * dy + cx, sn * dx + cs * dy + cy


def chip_plan(rect, w, h, rows=CHIP, cols=CHIP, cs=1.0, sn=0.0):
    """chip_levels() for a rectangle turned by (cs, sn) about its centre, with what the kernels are handed: -> dict(empty, levels, sw, sh,
    collapsed, x0, y0: the strip's first column and row in the frame, dims: [(width, height)] of the strip and of every pyramid level
    built from it (a collapsed level is (0, 0)), m, b: the affine chip (column, row) -> sampled image, None for an empty plan).  Details
    that are not finite make the empty plan.  The operations and their order are those of the library's host plan and the oracle's."""
    out = dict(empty=True, levels=0, sw=0, sh=0, collapsed=False, x0=0, y0=0, dims=[], m=None, b=None)
    if not all(math.isfinite(v) for v in tuple(rect) + (cs, sn)):
        return out
    size = float(rows * cols)
    grow, r = 2.0, _down(rect)
    while _area(r) > size:
        r = _down(r)
        grow = grow * 2 + 2
    cx, cy = (rect[0] + rect[2]) / 2, (rect[1] + rect[3]) / 2
    pts = [_rot(cx, cy, x, y, cs, sn) for x, y in ((rect[0], rect[1]), (rect[2], rect[1]), (rect[0], rect[3]), (rect[2], rect[3]))]
    l, t = min(p[0] for p in pts) - grow, min(p[1] for p in pts) - grow
    rr, b = max(p[0] for p in pts) + grow, max(p[1] for p in pts) + grow
    l, t, rr, b = max(l, 0.0), max(t, 0.0), min(rr, w - 1.0), min(b, h - 1.0)
    if l > rr or t > b:
        return out
    x0, y0, x1, y1 = (int(math.floor(v + 0.5)) for v in (l, t, rr, b))
    sw, sh = x1 - x0 + 1, y1 - y0 + 1
    if sw <= 0 or sh <= 0:
        return out
    levels, r = 0, (rect[0] - x0, rect[1] - y0, rect[2] - x0, rect[3] - y0)
    while _area(_down(r)) > size:
        r = _down(r)
        levels += 1
    dims, collapsed = [(sw, sh)], False
    for _ in range(levels):
        pw, ph = dims[-1]
        dims.append((0, 0) if (ph <= 8 or pw <= 8) else ((pw - 3) // 2, (ph - 3) // 2))
        collapsed = collapsed or dims[-1] == (0, 0)
    lcx, lcy = (r[0] + r[2]) / 2, (r[1] + r[3]) / 2
    tl, tr, bl = _rot(lcx, lcy, r[0], r[1], cs, sn), _rot(lcx, lcy, r[2], r[1], cs, sn), _rot(lcx, lcy, r[0], r[3], cs, sn)
    m = ((tr[0] - tl[0]) / float(cols - 1), (bl[0] - tl[0]) / float(rows - 1), (tr[1] - tl[1]) / float(cols - 1), (bl[1] - tl[1]) / float(rows - 1))
    return dict(empty=False, levels=levels, sw=sw, sh=sh, collapsed=collapsed, x0=x0, y0=y0, dims=dims, m=m, b=tl)


def box_class(box, w, h):
    """the classes the table must cover, for one start box"""
    out = set()
    l, t, r, b = box
    plan = chip_levels(tracker_rect(box), w, h)
    inverted = l > r or t > b
    if inverted:
        out.add("inverted")
    lo_x, hi_x, lo_y, hi_y = min(l, r), max(l, r), min(t, b), max(t, b)
    outside = hi_x < 0 or hi_y < 0 or lo_x > w - 1 or lo_y > h - 1
    if outside:
        out.add("outside_far" if max(abs(v) for v in box) >= 1e6 else "outside_near")
    else:
        sides = [s for s, c in (("left", lo_x < 0), ("right", hi_x > w - 1), ("top", lo_y < 0), ("bottom", hi_y > h - 1)) if c]
        if len(sides) == 1:
            out.add("cross_" + sides[0])
        if len(sides) == 2 and ("left" in sides or "right" in sides) and ("top" in sides or "bottom" in sides):
            out.add("corner_" + "_".join(sides))
        if len(sides) == 4:
            out.add("larger_than_frame")
    if r == w - 1:
        out.add("touch_last_column")
    if b == h - 1:
        out.add("touch_last_row")
    if (l, t, r, b) == (0, 0, w - 1, h - 1):
        out.add("whole_frame")
    ew, eh = abs(r - l), abs(b - t)
    if ew <= 1 and eh <= 1:
        out.add("px1")
    elif ew <= 3 and eh <= 3:
        out.add("px3")
    if any(v != math.floor(v) for v in box):
        out.add("fractional")
    if min(ew, eh) > 0 and max(ew, eh) / min(ew, eh) >= 50:
        out.add("aspect_wide" if ew > eh else "aspect_tall")
    if plan["empty"]:
        out.add("plan_empty")
    else:
        out.add("levels_%d" % min(plan["levels"], 4))
        if plan["levels"] >= 1 and plan["collapsed"]:
            out.add("pyramid_collapses")
            if min(plan["sw"], plan["sh"]) <= 8:
                out.add("strip_le_8")
    return out


REQUIRED_BOX_CLASSES = {"cross_left", "cross_right", "cross_top", "cross_bottom", "corner_left_top", "corner_right_top", "corner_left_bottom",
                        "corner_right_bottom", "touch_last_column", "touch_last_row", "outside_near", "outside_far", "px1", "px3", "fractional",
                        "whole_frame", "larger_than_frame", "aspect_wide", "aspect_tall", "inverted", "plan_empty", "levels_0", "levels_1",
                        "levels_2", "levels_3", "levels_4", "pyramid_collapses", "strip_le_8"}
REQUIRED_BOX_CLASSES_FULL = {"cross_left", "corner_right_bottom", "touch_last_column", "touch_last_row", "outside_near", "outside_far",
                             "whole_frame", "larger_than_frame", "levels_0", "levels_2", "levels_4", "pyramid_collapses", "inverted"}


def small_boxes(w=SMALL[0], h=SMALL[1]):
    return [
        ("cross_left", (-30, 100, 50, 180)), ("cross_right", (w - 50, 100, w + 30, 180)),
        ("cross_top", (300, -30, 380, 50)), ("cross_bottom", (300, h - 50, 380, h + 30)),
        ("corner_tl", (-20, -20, 60, 60)), ("corner_tr", (w - 60, -20, w + 20, 60)),
        ("corner_bl", (-20, h - 60, 60, h + 20)), ("corner_br", (w - 60, h - 60, w + 20, h + 20)),
        ("touch_last_column", (w - 80, 100, w - 1, 180)), ("touch_last_row", (300, h - 80, 380, h - 1)),
        ("outside_rect_inside", (w + 10, 100, w + 90, 180)),          # the box is outside, its 1.4x rectangle still reaches the frame
        ("outside_near", (w + 60, 100, w + 140, 180)), ("outside_negative", (-200, -200, -120, -120)),
        ("outside_far", (1e6, 1e6, 1e6 + 80, 1e6 + 80)),
        ("px1", (320, 180, 321, 181)), ("px3", (320, 180, 323, 183)), ("fractional", (100.37, 60.81, 171.93, 140.26)),
        ("whole_frame", (0, 0, w - 1, h - 1)), ("larger_than_frame", (-200, -150, w + 200, h + 150)),
        ("aspect_wide", (170, 178, 470, 182)), ("aspect_tall", (318, 30, 322, 330)),
        ("inverted", (380, 180, 300, 100)), ("inverted_x", (380, 100, 300, 180)),
        ("levels_1", (200, 100, 320, 220)), ("levels_2", (150, 50, 400, 300)), ("levels_3", (120, -20, 520, 380)),
        ("levels_4", (-60, -200, 700, 560)),
        ("mostly_outside", (-590, 30, 10, 330)),                      # a 600-px box with 10 px inside the frame
        ("strip_7px", (-167.6, 100, -27.6, 240)),                     # 1.4x rectangle ends at x = 0.4; one level; source strip 7 px wide
        ("strip_collapses_later", (-719.6, 30, -119.6, 330)),         # three levels; the 31-px strip runs out at the third
    ]


def full_boxes(w=FULL[0], h=FULL[1]):
    return [
        ("cross_left", (-90, 300, 150, 540)), ("corner_br", (w - 180, h - 180, w + 60, h + 60)),
        ("touch_last_column", (w - 240, 300, w - 1, 540)), ("touch_last_row", (900, h - 240, 1140, h - 1)),
        ("outside_near", (w + 200, 300, w + 440, 540)), ("outside_far", (1e6, 1e6, 1e6 + 240, 1e6 + 240)),
        ("whole_frame", (0, 0, w - 1, h - 1)), ("larger_than_frame", (-600, -450, w + 600, h + 450)),
        ("levels_0", (800, 400, 880, 480)), ("levels_2", (600, 200, 900, 500)), ("inverted", (1140, 540, 900, 300)),
        ("strip_collapses", (-2159.6, 90, -359.6, 990)),
    ]


# ---- frames
def shifted(frame, dx, dy=0):
    """the picture moved by (dx, dy) pixels, zero fill"""
    h, w = frame.shape[:2]
    out = np.zeros_like(frame)
    xs0, xs1 = max(0, -dx), min(w, w - dx)
    ys0, ys1 = max(0, -dy), min(h, h - dy)
    if xs1 > xs0 and ys1 > ys0:
        out[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx] = frame[ys0:ys1, xs0:xs1]
    return out


def rescaled(frame, factor, cx, cy):
    """nearest-neighbour magnification by `factor` about (cx, cy), zero fill"""
    h, w = frame.shape[:2]
    ys = np.floor(cy + (np.arange(h) - cy) / factor + 0.5).astype(np.int64)
    xs = np.floor(cx + (np.arange(w) - cx) / factor + 0.5).astype(np.int64)
    oky, okx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    out = frame[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)].copy()
    out[~oky] = 0
    out[:, ~okx] = 0
    return np.ascontiguousarray(out)


def uniform(value, w, h):
    return np.full((h, w, 3), value, np.uint8)


def noise_frame(w, h, seed=1234):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def face_boxes(video, i=0):
    return [tuple(float(v) for v in b[1:]) for b in video.face_boxes(i)]


_CACHE = {}


def small_cases(video):
    """video: the suite's small clip (conftest small_video: 640 x 360, two shots of 6 frames, 3 faces)"""
    key = ("small", id(video))
    if key in _CACHE:
        return _CACHE[key]
    w, h = SMALL
    pics = [video.frame(i) for i in range(6)]                        # one shot
    faces = face_boxes(video, 0)
    black, grey, white = uniform(0, w, h), uniform(128, w, h), uniform(255, w, h)
    cases = [Case("box_" + name, pics[:3], [box]) for name, box in small_boxes()]
    for px in (5, 15, 30):
        cases.append(Case("shift_right_%d" % px, [shifted(pics[i], px * i) for i in range(6)], faces))
    cases.append(Case("shift_down_left_15", [shifted(pics[i], -15 * i, 15 * i) for i in range(6)], faces))
    f0 = faces[0]
    fcx, fcy = (f0[0] + f0[2]) / 2, (f0[1] + f0[3]) / 2
    for pct in (10, -10, 25, -25, 40, -40):
        s = 1 + pct / 100.0
        cases.append(Case("rescale_%+d" % pct, [pics[0]] + [rescaled(pics[i], s ** i, fcx, fcy) for i in range(1, 5)], [f0]))
    for name, blank in (("black", black), ("grey128", grey), ("white255", white)):
        cases.append(Case("picture_then_" + name, [pics[0], blank, blank, blank], faces[:2]))
        cases.append(Case("start_on_" + name, [blank, blank, pics[1], pics[2]], faces[:1]))
    cases.append(Case("fade_black_run", [pics[0]] + [black] * BLACK_RUN + [pics[1], pics[2]], faces[:1]))
    # a tracker started beside the frame learns nothing, jumps half a chip per update and re-enters the picture with a scale filter
    # trained towards index 0: the family in which the scale peak lands on index 31 and the sub-pixel step is refused
    for name, box in (("a", (680, 140, 760, 220)), ("b", (680, 200, 760, 280)), ("c", (712, 100, 832, 220)), ("d", (696, 260, 816, 380))):
        cases.append(Case("reenter_" + name, pics[:4], [box]))
    cases.append(Case("noise_frame", [pics[0], pics[1], noise_frame(w, h), pics[2], pics[3]], faces[:2]))
    _CACHE[key] = cases
    return cases


def full_video():
    if "full_video" not in _CACHE:
        from pyannote_video_amd import synth
        _CACHE["full_video"] = synth.SyntheticVideo(width=FULL[0], height=FULL[1], n_frames=3, n_shots=1, faces=3, min_face=150, max_face=320, seed=7)
    return _CACHE["full_video"]


def full_cases():
    """the 1920 x 1080 subset"""
    if "full" in _CACHE:
        return _CACHE["full"]
    w, h = FULL
    v = full_video()
    pics = [v.frame(i) for i in range(3)]
    faces = face_boxes(v, 0)
    black = uniform(0, w, h)
    cases = [Case("full_box_" + name, pics, [box], FULL) for name, box in full_boxes()]
    cases.append(Case("full_shift_right_40", [shifted(pics[i], 40 * i) for i in range(3)], faces, FULL))
    cases.append(Case("full_picture_then_black", [pics[0], black, black, pics[1]], faces[:2], FULL))
    _CACHE["full"] = cases
    return cases


# the boxes pvf_tracker_start_many and oracle.Tracker.start_track refuse: a non-finite coordinate, or a width or height of exactly zero
REFUSED_BOXES = [(float("nan"), 100.0, 180.0, 180.0), (100.0, float("inf"), 180.0, 180.0), (100.0, 100.0, float("-inf"), 180.0),
                 (100.0, 100.0, 180.0, float("nan")), (100.0, 100.0, 100.0, 180.0), (100.0, 100.0, 180.0, 100.0), (50.5, 60.5, 50.5, 60.5),
                 (0.0, 0.0, 0.0, 0.0)]


def run_oracle(case, oracle, tables, states=True):
    """the oracle's tracker over one case -> per box dict(psr [n], pos [n][4], last [n] debug_last() records, A, B, As, Bs after the run)"""
    out = []
    for box in case.boxes:
        t = oracle.Tracker(tables)
        t.start_track(case.frames[0], box)
        psr, pos, last = [], [], []
        for f in case.frames[1:]:
            psr.append(t.update(f)); pos.append(t.get_position()); last.append(t.debug_last())
        rec = dict(psr=np.array(psr, np.float64), pos=np.array(pos, np.float64).reshape(-1, 4), last=last)
        if states:
            rec["A"], rec["B"] = t.debug_state()
            rec["As"], rec["Bs"] = t.debug_scale_state()
        out.append(rec)
    return out


def sliding_clip(video, px=15, slide=14, black=5, after=4):
    """one shot built from the small clip's first shot: the picture slides out through the right edge by `px` pixels per frame (zero
    fill; the source frames go back and forth so that the faces' own motion stays continuous), then black frames, then picture again"""
    pics = [video.frame(i) for i in range(6)]
    order = [0, 1, 2, 3, 4, 5, 4, 3, 2, 1]
    w, h = SMALL
    frames = [shifted(pics[order[i % len(order)]], px * i) for i in range(slide)]
    frames += [uniform(0, w, h) for _ in range(black)]
    frames += [pics[order[i % len(order)]].copy() for i in range(after)]
    return frames


def recording_tracker(oracle, tables, log):
    """oracle.Tracker that appends (confidence, position) of every update to `log`"""
    class T(oracle.Tracker):
        def __init__(self):
            oracle.Tracker.__init__(self, tables)

        def update(self, rgb):
            c = oracle.Tracker.update(self, rgb)
            log.append((c, self.get_position()))
            return c
    return T
