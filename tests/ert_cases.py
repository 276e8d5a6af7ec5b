"""The landmark kernel's edge-case table, shared by tests/test_ert_edge_cases.py (CPU: the table reaches every seam it claims, on the
oracle and the numpy restatement tests/ert_ref.py alone) and tests/test_gpu_ert_edges.py (GPU: csrc/ert.hip: ert_k equals the oracle on
every model x frame x box, float shape bit for bit).  Deterministic builders only.  Reference: pyannote/video/face/face.py:58,69-70
(dlib.shape_predictor(path)(rgb, rect)).

Models are models.make_shape_predictor(...) with the split thresholds ROUNDED TO INTEGERS (pixel differences are integers: only then
does diff == thresh occur, the case that tells `>` from `>=`), but for one row that keeps them as drawn."""
import functools

import numpy as np

from pyannote_video_amd import models

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


class Model(object):
    def __init__(self, name, n_cascades, n_trees, n_pix, depth, leaf_sigma=2e-4, integer_thresholds=True, seed=20260925):
        self.name, self.n_cascades, self.n_trees, self.n_pix, self.depth = name, n_cascades, n_trees, n_pix, depth
        self.leaf_sigma, self.integer_thresholds, self.seed = leaf_sigma, integer_thresholds, seed

    def __repr__(self):
        return self.name

    def leaf_mib(self):
        return self.n_cascades * self.n_trees * (1 << self.depth) * 136 * 4 / 2.0 ** 20


# ert_k: 256 lanes walk trees and gather pixels with a stride of 256, the leaf sum takes trees twenty at a time and the rest one by one,
# LDS is carved at (n_pix + 3) & ~3, load_shape accepts depth 1 .. 6 and 1 .. 1024 pixels.  About a dozen rows, not the product.
MODELS = [
    Model("c3_t40_p120_d4", 3, 40, 120, 4),                            # the suite's small model, integer thresholds
    Model("c3_t40_p120_d4_float_thresholds", 3, 40, 120, 4, integer_thresholds=False),
    Model("c1_t1_p3_d1", 1, 1, 3, 1, seed=20260926),                   # one tree, one split: the tail loop alone
    Model("c3_t19_p1_d6", 3, 19, 1, 6),                                # no full group of twenty; one pixel: every diff is 0
    Model("c3_t20_p255_d1", 3, 20, 255, 1),                            # exactly one group, no tail
    Model("c3_t21_p257_d4", 3, 21, 257, 4),                            # tail of one; pixel 256 is a lane's second
    Model("c3_t59_p3_d4", 3, 59, 3, 4),                                # tail of nineteen
    Model("c1_t257_p1024_d4", 1, 257, 1024, 4),                        # tree 256 is a lane's second; the most pixels
    Model("c2_t257_p120_d6", 2, 257, 120, 6),
    Model("c2_t300_p257_d6", 2, 300, 257, 6),                          # 20 MiB of leaves: at most two cascades at depth 6
    Model("c3_t300_p1024_d1", 3, 300, 1024, 1),
    Model("c3_t40_p120_d4_wander", 3, 40, 120, 4, leaf_sigma=2e-2),    # leaves 100 x larger: the shape wanders off the box and the frame
]
INTEGER_MODELS = [m for m in MODELS if m.integer_thresholds]


def model_by_name(name):
    return next(m for m in MODELS if m.name == name)


@functools.lru_cache(maxsize=None)
def tensors(name):
    """the model file's tensors, as models.save_container writes and models.load_container / oracle.ShapePredictor read them"""
    m = model_by_name(name)
    t = models.make_shape_predictor(seed=m.seed, n_cascades=m.n_cascades, n_trees=m.n_trees, n_pix=m.n_pix, depth=m.depth,
                                    leaf_sigma=m.leaf_sigma)
    if m.integer_thresholds:
        t["sp.split_thresh"] = np.rint(t["sp.split_thresh"]).astype(np.float32)
    for v in t.values():
        v.setflags(write=False)
    return t


# ---- frames -------------------------------------------------------------------------------------------------------------------------------
def _noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _truncating(h, w):
    """r + g + b = 2 (mod 3) on a random half of the pixels -- there (r + g + b) / 3 truncates by 2/3 and a rounded gray is one more --
    and = 0 (mod 3) on the others, where both agree: a split compares two pixels, and an error common to both would cancel"""
    rng = np.random.default_rng(3)
    f = rng.integers(0, 253, (h, w, 3), dtype=np.uint8)
    want = np.where(rng.integers(0, 2, (h, w)) == 1, 2, 0)
    f[:, :, 0] += ((want - f.astype(np.int64).sum(axis=2)) % 3).astype(np.uint8)      # at most 252 + 2
    assert (f.astype(np.int64).sum(axis=2) % 3 == want).all() and (want == 2).sum() > h * w // 4
    return f


def frames(small_video):
    """{name: uint8 [h, w, 3]}; the names say what each is for"""
    out = {
        "video0": small_video.frame(0),
        "video7": small_video.frame(7),
        "1x1": _noise(1, 1, 11),
        "2x3": _noise(2, 3, 12),
        "5x1": _noise(5, 1, 13),
        "odd_bytes_37x23": _noise(37, 23, 14),                 # 37 * 23 * 3 = 2553 bytes = 1 (mod 4)
        "zeros": np.zeros((48, 64, 3), np.uint8),
        "all255": np.full((48, 64, 3), 255, np.uint8),
        "noise": _noise(90, 120, 15),
        "truncating": _truncating(90, 120),
        # 6 MB of noise two rows high: the only frame on which samples of a box a million pixels wide still land (STRIP_BOXES)
        "strip_2x1000000": _noise(2, 1000000, 16),
    }
    assert out["odd_bytes_37x23"].size % 4 != 0
    return out


# ---- boxes --------------------------------------------------------------------------------------------------------------------------------
def boxes(h, w):
    """[(class, (left, top, right, bottom))] for a frame of h x w: every class of the issue, sized from the frame"""
    s = max(4, min(h, w) // 2)                                  # a box about half the frame
    cx, cy = w // 2, h // 2
    out = [
        ("inside", (cx - s // 2, cy - s // 2, cx + s // 2, cy + s // 2)),
        ("inside_odd", (cx - s // 3, cy - s // 2, cx + s // 2 + 1, cy + s // 3)),
        ("whole_frame", (0, 0, w - 1, h - 1)),
        ("cross_left", (-s // 2, cy - s // 2, s // 2, cy + s // 2)),
        ("cross_right", (w - s // 2, cy - s // 2, w + s // 2, cy + s // 2)),
        ("cross_top", (cx - s // 2, -s // 2, cx + s // 2, s // 2)),
        ("cross_bottom", (cx - s // 2, h - s // 2, cx + s // 2, h + s // 2)),
        ("corner_tl", (-s // 2, -s // 2, s // 2, s // 2)),
        ("corner_tr", (w - s // 2, -s // 2, w + s // 2, s // 2)),
        ("corner_bl", (-s // 2, h - s // 2, s // 2, h + s // 2)),
        ("corner_br", (w - s // 2, h - s // 2, w + s // 2, h + s // 2)),
        ("outside_left", (-3 * s, cy - s // 2, -2 * s, cy + s // 2)),
        ("outside_right", (w + 2 * s, cy - s // 2, w + 3 * s, cy + s // 2)),
        ("outside_top", (cx - s // 2, -3 * s, cx + s // 2, -2 * s)),
        ("outside_bottom", (cx - s // 2, h + 2 * s, cx + s // 2, h + 3 * s)),
        ("zero_width", (cx, cy - s // 2, cx, cy + s // 2)),
        ("zero_height", (cx - s // 2, cy, cx + s // 2, cy)),
        ("zero_area", (cx, cy, cx, cy)),
        ("zero_area_off_frame", (-7, h + 5, -7, h + 5)),
        ("inverted_x", (cx + s // 2, cy - s // 2, cx - s // 2, cy + s // 2)),
        ("inverted_y", (cx - s // 2, cy + s // 2, cx + s // 2, cy - s // 2)),
        ("inverted_both", (cx + s // 2, cy + s // 2, cx - s // 2, cy - s // 2)),
        ("one_pixel", (cx, cy, cx + 1, cy + 1)),
        ("dwarfing", (-1000000, -1000000, 1000000, 1000000)),   # one ulp of the shape is about 0.1 pixel: order defects reach the integers
        ("dwarfing_2p24", (0, 0, 1 << 24, 1 << 24)),            # u * 2^24 is a multiple of 1/2 for u in [1/4, 1/2): final coordinates ON .5
        ("i32_right", (I32_MAX - 199, 0, I32_MAX, 100)),        # points right of u = 1 saturate at INT32_MAX
        ("i32_left", (I32_MIN, 0, I32_MIN + 200, 100)),         # points left of u = 0 saturate at INT32_MIN
        ("i32_bottom", (0, I32_MAX - 199, 100, I32_MAX)),
        ("i32_top", (0, I32_MIN, 100, I32_MIN + 200)),
        ("i32_whole", (I32_MIN, I32_MIN, I32_MAX, I32_MAX)),    # both directions at once; right - left = 2^32 - 1 needs the double
    ]
    for _, b in out:
        assert all(I32_MIN <= v <= I32_MAX for v in b)
    return out


# One ulp of a sample's u is 6e-8 of the box: it moves a sample to another pixel only on boxes of millions of pixels, and such a box puts
# samples ON a frame only if the frame is that wide too.  Two pixels high, so that v * 2 stays on it.  These are the rows on which the
# precision of the similarity fit (an ulp or two of M) is visible at all.
STRIP_BOXES = [
    ("strip_dwarfing", (-1000000, 0, 2000000, 2)),
    ("strip_dwarfing_wide", (-2000000, 0, 3000000, 2)),
    ("strip_dwarfing_widest", (-4500000, 0, 5500000, 2)),
    ("strip_whole", (0, 0, 999999, 1)),
    ("strip_zero_area", (500000, 1, 500000, 1)),
]


def boxes_of(name, h, w):
    return STRIP_BOXES if name.startswith("strip") else boxes(h, w)


BOX_CLASSES = [c for c, _ in boxes(100, 100)] + [c for c, _ in STRIP_BOXES]
ZERO_AREA = ("zero_area", "zero_area_off_frame", "strip_zero_area")
SATURATING = ("i32_right", "i32_left", "i32_bottom", "i32_top", "i32_whole")


def faces(small_video):
    """[(frame name, box class, box)] : every frame x every box -- what one batched call of the GPU test runs for each model"""
    out = []
    for name, f in frames(small_video).items():
        for cls, b in boxes_of(name, f.shape[0], f.shape[1]):
            out.append((name, cls, b))
    return out
