"""The detector's edge-case table, shared by tests/test_detector_edge_cases.py (CPU: the table reaches what it claims, on the oracle and
on plan_dims() alone) and tests/test_gpu_detector_edges.py (GPU: pyramid bytes, feature bits, raw candidates and boxes equal the oracle's on
every case).  Frame geometries chosen for the seams of the kernels' fixed-width pieces, frame byte lengths and row pitches that are not
multiples of 4, and content the synthetic renderer never makes.  Nothing here imports a GPU context or the oracle.
Reference: pyannote/video/face/face.py:54,66 (dlib.get_frontal_face_detector()(rgb, 1))."""
import numpy as np

# ---- the piece sizes of the detector's kernels (pyannote-video_amd/csrc) ---------------------------------------------------------------
FHOG_STRIP = 61         # detect.hip: FUSED_OUT -- feature columns a 64-lane strip of fhog_split_ml_k yields
SCORE_STRIP = 96        # detect.hip: ml_plan, d.score_bx = (out_c + 95) / 96 -- output columns of a score_roll_k strip
SCR_GROUP = 48          # screen.hip: a 16-base group of the screening pass covers 48 output columns
SCR_SG = 4              # detect_ml.h: SCR_SG groups per screening strip
SCREEN_STRIP = SCR_GROUP * SCR_SG
RESIZE_WAVE = 64        # detect.hip: resize_rows_k, a wave's segment of output columns ...
RESIZE_BLOCK = 256      # ... and a block's
RESIZE_ROWS = 16        # detect.hip: launch_resize_rows, RS output rows per strip ...
RESIZE_ROWS_WAVE = 32   # ... and NSTRIP = 2 strips per wave
FEAT_PAD_COLS = 52      # detect_ml.h: zero columns behind every stored feature row (the screening pass reads into them)
WINDOW = 80             # the scanner's window in pixels: a level below it has no window to score
FILTER = 10             # filter rows and columns in cells
FIRST = 5               # feature-map row and column of the first scanned window (its centre cell)
ORACLE_CAP = 65536      # oracle.Detector._run: candidates its buffer holds; a count equal to it means truncation
COMPLETE_MAX = 60000    # cases with at most this many (window, filter) pairs are compared window by window
ALL_PASS = -100.0       # adjust_threshold under which every window of every tested content passes (test_detector_edge_cases.py proves it)


def plan_dims(w, h, upsample, levels):
    """the level schedule restated: -> (ups, lv); ups = [(w, h)] of every upsampling stage's output, lv = [(w, h, hog_nc, hog_nr)] per
    pyramid level.  `levels` comes from the oracle (Detector.levels of the upsampled size)."""
    ups = []
    for _ in range(upsample):
        w, h = 2 * w + 2, 2 * h + 1
        ups.append((w, h))
    lv = []
    for l in range(levels):
        lv.append((w, h, int(w / 8.0 + 0.5) - 2, int(h / 8.0 + 0.5) - 2))
        w, h = 5 * w // 6, 5 * h // 6
    return ups, lv


def upsampled(w, h, upsample):
    for _ in range(upsample):
        w, h = 2 * w + 2, 2 * h + 1
    return w, h


def scored(lv):
    """the levels that carry a feature map (and so at least one window)"""
    return [(l, d) for l, d in enumerate(lv) if d[2] > 0 and d[3] > 0]


def pairs(lv, n_filters=5):
    """raw candidates when every window of every filter passes"""
    return n_filters * sum(d[2] * d[3] for _, d in scored(lv))


def resize_outputs(w, h, upsample, levels):
    """(ow, oh) of every image resize_rows_k writes: the upsampling stages and the levels 1 .. (level 0 without upsampling is a copy)"""
    ups, lv = plan_dims(w, h, upsample, levels)
    return ups + [(d[0], d[1]) for d in lv[1:]]


class Geo(object):
    def __init__(self, w, h, up, levels, why):
        self.w, self.h, self.up, self.levels, self.why = w, h, up, levels, why      # levels: as the oracle counts them (the CPU test holds it to that)
        self.name = "%dx%d_up%d" % (w, h, up)

    def __repr__(self):
        return self.name

    @property
    def lv(self):
        return plan_dims(self.w, self.h, self.up, self.levels)[1]

    @property
    def pairs(self):
        return pairs(self.lv)

    @property
    def complete(self):
        return self.pairs <= COMPLETE_MAX

    @property
    def degenerate(self):
        return not scored(self.lv)

    @property
    def odd(self):
        """a pitch or a frame length that is not a multiple of 4"""
        return (self.w * 3) % 4 != 0 or (self.w * self.h * 3) % 4 != 0


GEOMETRY = [
    Geo(251, 60, 1, 4, "level 0 is 61 x 13 cells: exactly one full FHOG strip"),
    Geo(255, 100, 1, 7, "62 columns: a second FHOG strip of ONE column; ow = 512 = 2 * 256"),
    Geo(500, 61, 1, 4, "123 columns: a third FHOG strip of one column; frame bytes % 4 = 0, w even"),
    Geo(385, 97, 1, 7, "95 columns: one short of a 96 scoring strip; odd x odd frame"),
    Geo(769, 50, 1, 3, "191 columns: one short of a 192 screening strip"),
    Geo(1543, 41, 1, 2, "384 columns = 2 * 192 = 4 * 96 exactly; >= 12 resize blocks per row"),
    Geo(2049, 41, 0, 1, "no upsampling, w = 8 * 256 + 1, three feature rows"),
    Geo(257, 255, 0, 8, "256-pixel block + 1; frame bytes % 4 = 1"),
    Geo(256, 256, 0, 8, "256-pixel block; frame bytes % 4 = 0"),
    Geo(127, 127, 1, 8, "ow = 256 exactly"),
    Geo(641, 361, 1, 14, "frame bytes % 4 = 3; odd pitch"),
    Geo(643, 363, 1, 14, "frame bytes % 4 = 3; odd pitch, 8 pixels wider at level 0 than 641 x 361"),
    Geo(642, 361, 1, 14, "frame bytes % 4 = 2; even pitch, odd height"),
    Geo(457, 257, 1, 12, "frame bytes % 4 = 3; odd pitch"),
    Geo(641, 361, 0, 10, "level 0 is a copy of an odd-pitch frame"),
    Geo(161, 121, 2, 12, "two upsampling stages (the up_tmp path)"),
    Geo(1000, 90, 1, 6, "extreme aspect: wide"),
    Geo(90, 1000, 1, 6, "extreme aspect: tall"),
    Geo(97, 55, 1, 4, "just above the window after upsampling"),
    Geo(41, 39, 1, 2, "upsampled to 84 x 79: below the window in one dimension"),
    Geo(79, 79, 0, 2, "one pixel below the 80-pixel window"),
    Geo(80, 80, 0, 2, "at the 80-pixel window"),
    Geo(40, 40, 0, 1, "one level, nine windows"),
    Geo(7, 5, 0, 1, "no feature map: one level, nothing to score"),
    Geo(1, 1, 1, 1, "one pixel, upsampled to 4 x 3: no feature map"),
    # ---- seams the issue's table leaves to this one
    Geo(390, 45, 1, 3, "96 columns: exactly one scoring strip = two screening groups"),
    Geo(393, 45, 1, 3, "97 columns: a second scoring strip of one column; 48 * 2 + 1"),
    Geo(773, 45, 1, 3, "192 columns: exactly one screening strip"),
    Geo(777, 45, 1, 3, "193 columns: a second screening strip of one column; a third scoring strip of one"),
    Geo(1164, 95, 0, 3, "144 columns = 48 * 3 exactly, no upsampling"),
    Geo(391, 99, 0, 3, "47 columns: one short of a screening group; no upsampling, odd pitch"),
    Geo(404, 132, 0, 5, "49 columns: a screening group + 1"),
    Geo(612, 98, 0, 3, "level 1 (not 0) is 510 wide: 62 columns, a second FHOG strip of one column on a later level"),
    Geo(309, 117, 0, 4, "level 1 is 257 x 97: ow = 256 + 1, oh = 32 * 3 + 1"),
    Geo(231, 98, 0, 3, "level 1 is 192 x 81: ow = 64 * 3, oh = 16 * 5 + 1"),
    Geo(495, 61, 1, 4, "122 columns: exactly two FHOG strips"),
    Geo(155, 97, 0, 3, "level 1 is 129 x 80: ow = 64 * 2 + 1"),
]


def by_name(name):
    return [g for g in GEOMETRY if g.name == name][0]


# ---- seams: (name, predicate over the plan) -- test_detector_edge_cases.py shows every one is hit by a level of a case ------------------
def _cols(g):
    return [d[2] for _, d in scored(g.lv)]


def _outs(g):
    return resize_outputs(g.w, g.h, g.up, g.levels)


SEAMS = [("fhog %d columns" % n, (lambda g, n=n: n in _cols(g))) for n in (FHOG_STRIP, FHOG_STRIP + 1, 2 * FHOG_STRIP, 2 * FHOG_STRIP + 1)]
SEAMS += [("score / screen %d columns" % n, (lambda g, n=n: n in _cols(g)))
          for n in (SCORE_STRIP - 1, SCORE_STRIP, SCORE_STRIP + 1, SCREEN_STRIP - 1, SCREEN_STRIP, SCREEN_STRIP + 1, 2 * SCREEN_STRIP)]
SEAMS += [("screen group 48k - 1", lambda g: any(n % SCR_GROUP == SCR_GROUP - 1 for n in _cols(g))),
          ("screen group 48k", lambda g: any(n % SCR_GROUP == 0 for n in _cols(g))),
          ("screen group 48k + 1", lambda g: any(n % SCR_GROUP == 1 and n > 1 for n in _cols(g))),
          ("resize ow = 64k", lambda g: any(ow % RESIZE_WAVE == 0 for ow, _ in _outs(g))),
          ("resize ow = 64k + 1", lambda g: any(ow % RESIZE_WAVE == 1 and ow > 1 for ow, _ in _outs(g))),
          ("resize ow = 256k", lambda g: any(ow % RESIZE_BLOCK == 0 for ow, _ in _outs(g))),
          ("resize ow = 256k + 1", lambda g: any(ow % RESIZE_BLOCK == 1 and ow > 1 for ow, _ in _outs(g))),
          ("resize oh = 16k + 1", lambda g: any(oh % RESIZE_ROWS == 1 and oh > 1 for _, oh in _outs(g))),
          ("resize oh = 32k + 1", lambda g: any(oh % RESIZE_ROWS_WAVE == 1 and oh > 1 for _, oh in _outs(g))),
          ("a FHOG-strip seam on a level other than 0", lambda g: any(l > 0 and d[2] % FHOG_STRIP in (0, 1) and d[2] > 1 for l, d in scored(g.lv))),
          ("a level of at most three feature rows", lambda g: any(d[3] <= 3 for _, d in scored(g.lv))),
          ("a level without a feature map", lambda g: len(scored(g.lv)) < len(g.lv)),
          ("no level with a feature map", lambda g: g.degenerate),
          ("two upsampling stages", lambda g: g.up == 2)]


# ---- content -----------------------------------------------------------------------------------------------------------------------------
def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _renderer(h, w, seed):
    if min(h, w) < 32:                      # (the renderer's face grid needs room: below about 20 pixels it fails)
        return _noise(h, w, seed)
    from pyannote_video_amd import synth
    v = synth.SyntheticVideo(width=w, height=h, n_frames=2, n_shots=1, faces=2 if w >= 2 * h else 1, min_face=40, max_face=110, seed=seed)
    return v.frame(0)


def _const(v):
    return lambda h, w, seed: np.full((h, w, 3), v, np.uint8)


def _checker(period, channels=(0, 1, 2)):
    def make(h, w, seed):
        y, x = np.mgrid[0:h, 0:w]
        board = ((((y // period) + (x // period)) & 1) * 255).astype(np.uint8)
        out = np.zeros((h, w, 3), np.uint8)
        for c in channels:
            out[:, :, c] = board
        return out
    return make


def _grey_noise(h, w, seed):
    g = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))


def _ramp_x(h, w, seed):
    r = np.rint(np.arange(w) * 255.0 / max(w - 1, 1)).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(r[None, :, None], (h, w, 3)))


def _ramp_y(h, w, seed):
    r = np.rint(np.arange(h) * 255.0 / max(h - 1, 1)).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(r[:, None, None], (h, w, 3)))


def _noise_tail(h, w, seed):
    """dark noise whose last row, last column and bottom-right pixel are 255: a tail byte of the frame that reads as zero shows"""
    f = _noise(h, w, seed) >> 1
    f[-1, :, :] = 255
    f[:, -1, :] = 255
    return f


CONTENT = [("renderer", _renderer), ("noise", _noise), ("black", _const(0)), ("white", _const(255)), ("grey", _const(128)),
           ("checker1", _checker(1)), ("checker2", _checker(2)), ("checker1_r", _checker(1, (0,))), ("checker1_g", _checker(1, (1,))),
           ("checker1_b", _checker(1, (2,))), ("grey_noise", _grey_noise), ("ramp_x", _ramp_x), ("ramp_y", _ramp_y),
           ("noise_tail", _noise_tail)]
_CONTENT = dict(CONTENT)
CONSTANT = ("black", "white", "grey")
SATURATED = ("checker1", "checker2")
CONTENT_SIZES = ("255x100_up1", "385x97_up1", "641x361_up0")       # every CONTENT generator runs at these (all complete)


def frame(name, h, w, seed=0):
    """(name, h, w, seed) -> uint8 RGB [h, w, 3], contiguous"""
    f = np.ascontiguousarray(_CONTENT[name](h, w, seed), np.uint8)
    assert f.shape == (h, w, 3)
    return f


def case_frame(geo, content, seed=0):
    return frame(content, geo.h, geo.w, seed + 1000 * GEOMETRY.index(geo))


# ---- thresholds --------------------------------------------------------------------------------------------------------------------------
# (case, content) -> adjust_threshold for the cases too large to compare window by window: found by bisection on the oracle (tools: the
# loop of test_detector_with_hundreds_of_candidates_at_the_threshold) so that between 2 000 and 60 000 windows pass, every level holds
# candidates and each level's first and last scanned row and column are among them.  test_detector_edge_cases.py re-checks all of that.
ADJUST = {
    ("641x361_up1", "renderer"): -0.81640625, ("641x361_up1", "noise"): -0.845703125,
    ("643x363_up1", "renderer"): -0.81640625, ("643x363_up1", "noise"): -0.84375,
    ("642x361_up1", "renderer"): -0.818359375, ("642x361_up1", "noise"): -0.845703125,
    ("457x257_up1", "renderer"): -0.85546875, ("457x257_up1", "noise"): -0.8828125,
    ("161x121_up2", "renderer"): -0.861328125, ("161x121_up2", "noise"): -0.89453125,
    ("1000x90_up1", "renderer"): -0.841796875, ("1000x90_up1", "noise"): -0.86328125,
    ("90x1000_up1", "renderer"): -0.892578125, ("90x1000_up1", "noise"): -0.91015625,
}
# frames at unaligned device addresses: five noise frames (seeds 0 .. 4) each.  Stacked in one tensor, frame i starts i * h * w * 3 bytes in:
# three or four different remainders modulo 4 for the STACKED_ODD sizes (byte lengths % 4 = 3, 3, 1); 255 x 100 is 76 500 bytes, its
# stacked frames stay aligned (odd pitch at an aligned base) and it meets the other remainders through the offset slices
ADDRESS_SIZES = ("641x361_up1", "385x97_up1", "255x100_up1", "1543x41_up1")
STACKED_ODD = ("641x361_up1", "385x97_up1", "1543x41_up1")
ADDRESS_SEEDS = (0, 1, 2, 3, 4)


def thresholds(geo, content):
    """adjust_threshold values a (case, content) is compared at: the shipped one and the all-pass or the bisected one"""
    if geo.complete:
        return (0.0, ALL_PASS)
    return (0.0, ADJUST[(geo.name, content)])


# ---- what the GPU test sends through detect_raw: (case, content, seed, adjust_threshold) -- the CPU test holds every one below ORACLE_CAP --
BATCH_SIZE = "385x97_up1"                                            # seven distinct frames of one odd size, mixed content in one call
BATCH_FRAMES = (("noise", 0), ("black", 0), ("renderer", 0), ("noise", 1), ("checker2", 0), ("renderer", 1), ("white", 0))
TINY_BATCH_SIZE = "40x40_up0"
CHUNK_SIZES = ("40x40_up0", "255x100_up1")                           # PVF_FHOG_CHUNK / PVF_SCORE_SEG: the smallest case and a two-strip one
AFTER_OTHER_WORK = ("385x97_up1", "641x361_up0")                     # run after tracker work and after each other on one context


def geometry_runs():
    return [(g, c, 0, a) for g in GEOMETRY for c in ("renderer", "noise") for a in thresholds(g, c)]


def content_runs():
    return [(by_name(n), c, 0, ALL_PASS) for n in CONTENT_SIZES for c, _ in CONTENT]


def address_runs():
    return [(by_name(n), "noise", s, thresholds(by_name(n), "noise")[1]) for n in ADDRESS_SIZES for s in ADDRESS_SEEDS]


def batch_runs():
    return [(by_name(BATCH_SIZE), c, s, a) for c, s in BATCH_FRAMES for a in (0.0, ALL_PASS)] + \
           [(by_name(TINY_BATCH_SIZE), c, s, ALL_PASS) for c, s in BATCH_FRAMES]


def all_runs():
    seen, out = set(), []
    for g, c, s, a in geometry_runs() + content_runs() + address_runs() + batch_runs():
        if (g.name, c, s, a) not in seen:
            seen.add((g.name, c, s, a))
            out.append((g, c, s, a))
    return out
