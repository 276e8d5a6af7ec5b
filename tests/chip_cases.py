"""The geometry table of the chip kernels (csrc/chip.hip: pyr_down2_k, transform_k) and of the tracker kernels that sample the frame
themselves (csrc/dsst.hip: scale_fhog_k<true>, the fused start / update kernels through the chip path), shared by tests/test_chip_cases.py
(CPU: the table reaches what it claims, on the restated plan of tracker_cases.chip_plan and on the oracle alone) and by
tests/test_gpu_chip_geometry.py / tests/test_gpu_tracker_geometry.py (GPU: the library equals the oracle on every case).  Those kernels read
RGB frames with unaligned dword loads at byte (y * w + x) * 3; the table holds row pitches of every remainder modulo 4, frames smaller than a
chip, pyramid levels on the seams of pyr_down2_k's 32 x 8 tiles, chips on the seam of transform_k's 64-column blocks, sample grids that
land exactly on integers, exact quarter turns and jobs that are empty, collapsed or not finite.  Deterministic builders only; nothing here
imports a GPU context or the oracle.  Reference: pyannote/video/tracking.py:203,231,250-251 (dlib.correlation_tracker),
pyannote/video/face/face.py:73-76 (compute_face_descriptor: dlib's 150 x 150 chip of the 68 landmarks)."""
import math

import numpy as np

import tracker_cases as tc

PD_TW, PD_TH = 32, 8      # chip.hip: pyr_down2_k's tile of output pixels
XF_BLOCK = 64             # chip.hip: transform_k, chip columns per block
FACE = 150                # the embedder's chip


class Geo(object):
    def __init__(self, w, h, why):
        self.w, self.h, self.why = w, h, why
        self.name = "%dx%d" % (w, h)

    def __repr__(self):
        return self.name

    @property
    def pitch_phase(self):
        return (3 * self.w) % 4

    @property
    def tiny(self):
        return min(self.w, self.h) <= 9


GEOMETRY = [
    Geo(854, 480, "480p: a 2562-byte pitch, 2 modulo 4"),
    Geo(853, 479, "pitch 3 modulo 4, odd x odd"),
    Geo(641, 361, "pitch 3 modulo 4; frame bytes 3 modulo 4"),
    Geo(97, 81, "pitch 3 modulo 4; a frame hardly larger than the tracker's chip"),
    Geo(68, 20, "pitch 0 modulo 4: the control; level 1 of the whole frame is 32 x 8, exactly one tile"),
    Geo(1, 1, "one pixel: every bilinear sample needs a right and a lower neighbour, so every chip is black"),
    Geo(2, 2, "one sample position has both neighbours"),
    Geo(7, 5, "below pyramid_down's limit in both dimensions: a first level collapses"),
    Geo(8, 8, "at the limit: a side of 8 still collapses"),
    Geo(9, 9, "one above the limit: level 1 is 3 x 3, a second level collapses"),
    Geo(8, 200, "collapses by its width alone"),
    Geo(200, 9, "level 1 is 98 x 3; pitch 0 modulo 4"),
    Geo(4099, 9, "very wide and thin: level 1 is 2048 x 3, 64 tile columns of one partial tile row; pitch 1 modulo 4"),
    Geo(65, 17, "level 1 of the whole frame is 31 x 7: one short of a tile both ways"),
    Geo(67, 19, "level 1 is 32 x 8 from odd sides; pitch 1 modulo 4"),
    Geo(69, 21, "level 1 is 33 x 9: a second tile column and a second tile row of one pixel each"),
    Geo(131, 35, "level 1 is 64 x 16: two by two full tiles; level 2 is 30 x 6; pitch 1 modulo 4"),
    Geo(133, 37, "level 1 is 65 x 17: a third tile column and row of one pixel; level 2 is 31 x 7"),
    Geo(70, 24, "level 1 is 33 x 10 from even sides: a partial last tile row of even height"),
    Geo(77, 29, "level 1 is 37 x 13"),
]


def by_name(name):
    return [g for g in GEOMETRY if g.name == name][0]


STUDY = ("854x480", "853x479", "641x361", "97x81")          # the sizes that carry the full list of chip requests
ROUTES = ("854x480", "853x479", "641x361", "97x81", "67x19", "7x5")   # frames by every route: the odd pitches and a tiny one
MIXED_SIZES = ("854x480", "7x5", "97x81", "9x9", "4099x9", "2x2")     # one call over frames of different sizes


# ---- content -------------------------------------------------------------------------------------------------------------------------
def blob_picture(w, h, seed=5):
    """blobs of 8 x 8 pixels under a little noise (the picture of test_gpu_tracker_transform.py), cut to w x h"""
    rng = np.random.default_rng(seed)
    H, W = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    coarse = rng.integers(0, 256, (H // 8, W // 8, 3)).astype(np.int64)
    img = np.kron(coarse, np.ones((8, 8, 1), np.int64)) + rng.integers(-12, 13, (H, W, 3))
    return np.ascontiguousarray(np.clip(img, 0, 255).astype(np.uint8)[:h, :w])


def tail_picture(w, h, seed=0):
    """dark noise with the last row and the last column at 255 (detector_cases' noise_tail)"""
    f = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8) >> 1
    f[-1, :, :] = 255
    f[:, -1, :] = 255
    return f


CONTENT = ("blobs", "noise", "tail", "black")
_FRAMES = {}


def step(geo):
    """how far the picture moves per update"""
    return (min(3, geo.w // 4), min(2, geo.h // 4))


def frames(geo, content):
    """-> [start frame, first update, second update]: the picture and two shifted copies of it (zero fill)"""
    key = (geo.name, content)
    if key not in _FRAMES:
        k = GEOMETRY.index(geo)
        if content == "blobs":
            f = blob_picture(geo.w, geo.h, 5 + k)
        elif content == "noise":
            f = tc.noise_frame(geo.w, geo.h, 100 + k)
        elif content == "tail":
            f = tail_picture(geo.w, geo.h, 200 + k)
        else:
            f = np.zeros((geo.h, geo.w, 3), np.uint8)
        dx, dy = step(geo)
        _FRAMES[key] = [f, tc.shifted(f, dx, dy), tc.shifted(f, 2 * dx, 2 * dy)]
        for a in _FRAMES[key]:
            a.setflags(write=False)
    return _FRAMES[key]


def frame(geo, content):
    return frames(geo, content)[0]


# ---- chip requests -------------------------------------------------------------------------------------------------------------------
class Req(object):
    def __init__(self, name, rect, rows, cols, cs=1.0, sn=0.0):
        self.name, self.rect, self.rows, self.cols, self.cs, self.sn = name, tuple(float(v) for v in rect), int(rows), int(cols), float(cs), float(sn)

    def __repr__(self):
        return self.name

    def plan(self, geo):
        return tc.chip_plan(self.rect, geo.w, geo.h, self.rows, self.cols, self.cs, self.sn)


def _fit(rect, levels, cap=FACE):
    """(rows, cols) of about the rectangle's size after `levels` halvings, at most `cap` a side: the chip then takes at least that
    many levels and samples nearly every pixel of the last"""
    cw, ch = (rect[2] - rect[0]) / 2.0 ** levels, (rect[3] - rect[1]) / 2.0 ** levels
    return max(2, min(int(ch) - 1, cap)), max(2, min(int(cw) - 1, cap))


def _turn(degrees):
    a = math.radians(degrees)
    return math.cos(a), math.sin(a)


def requests(geo):
    w, h = geo.w, geo.h
    s = float(min(w, h))
    whole = (-2.0, -2.0, w + 1.0, h + 1.0)                     # dwarfs the frame: the cropped strip is the whole frame
    out = []
    if min(w, h) > 8:                                          # one level is really taken (more where the chip's side is capped)
        for lv in (1, 2):
            rows, cols = _fit(whole, lv, FACE if geo.name in STUDY else 1100)
            out.append(Req("whole_frame_%d" % lv, whole, rows, cols))
    else:
        rows, cols = _fit(whole, 0, 64)
        out.append(Req("whole_frame_0", whole, rows, cols))
        out.append(Req("whole_frame_collapses", whole, 2, 2))
    if geo.tiny:
        out.append(Req("first_pixel", (0.1, 0.1, 0.9, 0.9), 5, 5))   # the sample position a 2 x 2 frame has
    if min(w, h) >= 2:                                         # the last sample lies half a pixel inside the last column and row
        out.append(Req("tail_corner", (w - 9.5, h - 9.5, w - 1.5, h - 1.5), 9, 9))
    cs, sn = _turn(30)
    out.append(Req("inside_fractional", (0.21 * w + 0.37, 0.18 * h + 0.81, 0.21 * w + 0.37 + 0.45 * s, 0.18 * h + 0.81 + 0.45 * s), 64, 64))
    out.append(Req("corner_turned_30", (w - 1 - 0.3 * s, h - 1 - 0.3 * s, w - 1 + 0.3 * s, h - 1 + 0.3 * s), 23, 65, cs, sn))
    if geo.name not in STUDY:
        return out
    # level counts 0, 1, 2, >= 3 of the embedder's chip; its block seam (150 = 2 * 64 + 22)
    cx, cy = 0.5 * w, 0.5 * h
    for name, side in (("levels_0", 0.5 * s), ("levels_1", 400.0), ("levels_2", 800.0), ("levels_3", 1900.0), ("levels_4", 3700.0)):
        out.append(Req(name, (cx - side / 2, cy - side / 2, cx + side / 2, cy + side / 2), FACE, FACE))
    out.append(Req("collapsed", (cx - 4e5, cy - 4e5, cx + 4e5, cy + 4e5), FACE, FACE))
    out.append(Req("empty_outside", (w + 400.0, h + 300.0, w + 500.0, h + 400.0), FACE, FACE))
    out.append(Req("empty_negative", (-900.0, -700.0, -800.0, -600.0), 64, 64))
    out.append(Req("not_finite", (30.0, 30.0, 30.0, 30.0), FACE, FACE, float("nan"), float("nan")))    # what 68 identical landmarks give
    # the seam of transform_k's 64-column blocks, on a fractional rectangle turned a little
    cs, sn = _turn(-7)
    for cols, rows in ((2, 2), (63, 9), (64, 9), (65, 9), (150, 5), (64, 23), (23, 64)):
        out.append(Req("cols_%d_rows_%d" % (cols, rows), (0.3 * w + 0.25, 0.3 * h + 0.6, 0.3 * w + 0.25 + 0.4 * s, 0.3 * h + 0.6 + 0.3 * s), rows, cols, cs, sn))
    # sample grids on integers: a rectangle cols - 1 wide and rows - 1 high at integer corners
    for name, x0, y0, rows, cols in (("grid_flush_left_top", 0, 0, 23, 64), ("grid_flush_right_bottom", w - 64, h - 23, 23, 64),
                                     ("grid_flush_right", w - 65, 3, 9, 65), ("grid_flush_bottom", 5, h - 9, 9, 63),
                                     ("grid_inside", 11, 7, 23, 64)):
        out.append(Req(name, (x0, y0, x0 + cols - 1, y0 + rows - 1), rows, cols))
    for name, x0, y0 in (("grid_half_outside_left_top", -0.5, -0.5), ("grid_half_outside_right_bottom", w - 64 + 0.5, h - 23 + 0.5)):
        out.append(Req(name, (x0, y0, x0 + 63, y0 + 22), 23, 64))
    # exact quarter and half turns, and the same angles from the maths library (cos(pi / 2) = 6e-17)
    q = (0.25 * w, 0.2 * h, 0.25 * w + 0.5 * s, 0.2 * h + 0.4 * s)
    for name, cs, sn in (("turn_quarter", 0.0, 1.0), ("turn_minus_quarter", 0.0, -1.0), ("turn_half", -1.0, 0.0)):
        out.append(Req(name, q, 33, 65, cs, sn))
    for name, a in (("turn_quarter_libm", math.pi / 2), ("turn_minus_quarter_libm", -math.pi / 2), ("turn_half_libm", math.pi)):
        out.append(Req(name, q, 33, 65, math.cos(a), math.sin(a)))
    gq = (9.0, 6.0, 9.0 + 63, 6.0 + 63)                          # ... on an integer grid: every sample of the quarter turn is a pixel
    out.append(Req("grid_turn_quarter", gq, 64, 64, 0.0, 1.0))
    out.append(Req("grid_turn_quarter_libm", gq, 64, 64, math.cos(math.pi / 2), math.sin(math.pi / 2)))
    return out


def all_requests():
    return [(g, r) for g in GEOMETRY for r in requests(g)]


PYRAMID_TAIL = ("97x81", "65x17", "67x19", "69x21", "77x29")     # odd x odd: the last pixel of level 1 holds the frame's last pixel


def tail_requests(geo):
    """the requests whose chip changes with the frame's bottom-right pixel: a sample half a pixel inside it, and, where both sides are
    odd, the one-level chip of the whole frame (test_chip_cases.py holds the oracle to that)"""
    names = (["tail_corner"] if min(geo.w, geo.h) >= 2 else []) + (["whole_frame_1"] if geo.name in PYRAMID_TAIL else [])
    return [r for r in requests(geo) if r.name in names]


# ---- what the kernels are handed, from the plan ------------------------------------------------------------------------------------------
def pyr_sources(plan, w):
    """per pyramid level built: (row pitch in pixels, x0, y0, output width, output height) of pyr_down2_k's job"""
    out = []
    for l in range(plan["levels"]):
        dw, dh = plan["dims"][l + 1]
        if dw <= 0 or dh <= 0:
            break
        out.append((w, plan["x0"], plan["y0"], dw, dh) if l == 0 else (plan["dims"][l][0], 0, 0, dw, dh))
    return out


def pyr_phases(plan, w):
    """the first byte of pyr_down2_k's 15-byte reads, modulo 4, over every horizontal sum of every level"""
    seen = set()
    for pitch, x0, y0, dw, dh in pyr_sources(plan, w):
        r = np.arange(2 * dh + 3, dtype=np.int64)[:, None]
        c = np.arange(dw, dtype=np.int64)[None, :]
        seen |= set(np.unique((((y0 + r) * pitch + x0 + 2 * c) * 3) % 4).tolist())
    return seen


def sample_grid(req, plan):
    """(px, py) float64 [rows, cols] of transform_k's samples in the image it reads, (pitch, x0, y0, sw, sh) of that image"""
    m, b = plan["m"], plan["b"]
    c = np.arange(req.cols, dtype=np.float64)[None, :]
    r = np.arange(req.rows, dtype=np.float64)[:, None]
    return m[0] * c + m[1] * r + b[0], m[2] * c + m[3] * r + b[1]


def transform_source(plan, w):
    if plan["levels"] == 0:
        return w, plan["x0"], plan["y0"], plan["sw"], plan["sh"]
    dw, dh = plan["dims"][-1]
    return dw, 0, 0, dw, dh


def transform_phases(req, plan, w):
    """the first byte of transform_k's 6-byte reads, modulo 4, over the samples that are read"""
    if plan["empty"] or plan["collapsed"]:
        return set()
    pitch, x0, y0, sw, sh = transform_source(plan, w)
    px, py = sample_grid(req, plan)
    fx, fy = np.floor(px), np.floor(py)
    ok = (fx >= 0) & (fy >= 0) & (fx + 1 < sw) & (fy + 1 < sh)
    at = ((y0 + fy[ok].astype(np.int64)) * pitch + x0 + fx[ok].astype(np.int64)) * 3
    return set(np.unique(at % 4).tolist())


# ---- face landmarks -------------------------------------------------------------------------------------------------------------------------
def face_sets(geo):
    """(name, (cx, cy, face, degrees)) for test_gpu_chip_edges.landmarks; None: 68 identical points"""
    w, h = geo.w, geo.h
    s = float(min(w, h))
    out = [("inside", (0.5 * w, 0.5 * h, max(0.6 * s, 2.0), 0)), ("corner_20", (w - 1 - 0.2 * s, h - 1 - 0.2 * s, max(0.8 * s, 2.0), 20)),
           ("larger_than_frame", (0.4 * w, 0.6 * h, 1.5 * max(w, h), -15))]
    if geo.name in STUDY:
        out += [("levels_0", (0.3 * w, 0.4 * h, 60.0, 5)), ("levels_1", (0.5 * w, 0.5 * h, 300.0, 0)), ("levels_2", (0.5 * w, 0.5 * h, 620.0, -10)),
                ("levels_3", (0.5 * w, 0.5 * h, 1500.0, 0)), ("empty", (w + 3000.0, h + 3000.0, 80.0, 0)), ("collapsed", (0.5 * w, 0.5 * h, 4e5, 0)),
                ("not_finite", None), ("off_left_45", (2.0, 0.5 * h, 0.5 * s, 45))]
    return out


COMPOSITION = ("levels_0", "levels_1", "levels_2", "levels_3", "empty", "collapsed", "not_finite", "inside", "corner_20")


def face_points(mean51, geo):
    """-> names, int32 [n, 68, 2]"""
    from test_gpu_chip_edges import landmarks
    names, pts = [], []
    for name, a in face_sets(geo):
        names.append(name)
        pts.append(np.full((68, 2), 30, np.int32) if a is None else landmarks(mean51, *a))
    return names, np.stack(pts)


# ---- tracker boxes --------------------------------------------------------------------------------------------------------------------------
def boxes(geo):
    """start boxes scaled to the frame; never one of zero width or height (the library and the oracle refuse those)"""
    w, h = float(geo.w), float(geo.h)
    s = min(w, h)
    a = max(2.0, math.floor(0.4 * s))                                       # the box's side
    cx, cy = math.floor(0.45 * w), math.floor(0.5 * h)
    r, b = w - 1, h - 1
    return [("inside", (cx - a / 2, cy - a / 2, cx + a / 2, cy + a / 2)),
            ("cross_left", (-a / 4, cy - a / 2, 3 * a / 4, cy + a / 2)), ("cross_right", (r - 3 * a / 4, cy - a / 2, r + a / 4, cy + a / 2)),
            ("cross_top", (cx - a / 2, -a / 4, cx + a / 2, 3 * a / 4)), ("cross_bottom", (cx - a / 2, b - 3 * a / 4, cx + a / 2, b + a / 4)),
            ("corner_bottom_right", (r - a / 2, b - a / 2, r + a / 2, b + a / 2)),
            ("whole_frame", (0.0, 0.0, max(r, 1.0), max(b, 1.0))),
            ("larger_than_frame", (-0.25 * w - 1, -0.25 * h - 1, r + 0.25 * w + 1, b + 0.25 * h + 1)),
            ("far_larger_than_frame", (-1000 * w, -1000 * h, 1001 * w, 1001 * h)),
            ("fractional", (0.37 * w + 0.37, 0.31 * h + 0.81, 0.37 * w + 0.37 + 0.62 * a + 0.26, 0.31 * h + 0.81 + 0.55 * a + 0.45)),
            ("last_pixels", (r - 4.5, b - 4.5, r + 0.5, b + 0.5))]          # five pixels a side at the bottom right: no pyramid level dilutes the last pixel


TRACKER_CONTENT = {"854x480": ("blobs", "tail", "noise"), "853x479": ("blobs", "tail"), "641x361": ("blobs", "tail", "black"), "97x81": ("blobs", "tail", "noise"),
                   "67x19": ("blobs", "tail", "black"), "7x5": ("blobs", "tail")}


def tracker_content(geo):
    return TRACKER_CONTENT.get(geo.name, ("blobs", "tail"))


def tracker_case(geo, content):
    return tc.Case("%s_%s" % (geo.name, content), frames(geo, content), [b for _, b in boxes(geo)], (geo.w, geo.h))
