"""oracle/pvo_ert.c restated in numpy (dlib.shape_predictor(path)(rgb, rect), reference pyannote/video/face/face.py:58,69-70): what
tests/test_ert_edge_cases.py holds against the oracle, reads its trace from and plants defects in.

Every float32 value is made by one float32 operation at a time, in the oracle's order: the similarity fit sums over the parts
sequentially in float64, a coordinate's leaf sum is a float32 chain over the trees 0 .. T - 1 (the vectors below run over the 136
coordinates, never over the trees), the sample coordinates are floor(x + 0.5) of a float64, gray is (r + g + b) / 3 truncated, a sample
off the frame reads 0, the final points are floor(x + 0.5) saturated to the int32 range.

landmarks(..., defect=NAME) computes something subtly different instead; DEFECTS names what each one changes."""
import numpy as np

F32 = np.float32
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

DEFECTS = {
    "ge": "a split goes left on diff >= thresh instead of diff > thresh",
    "half_even": "coordinates are rounded half to even instead of floor(x + 0.5)",
    "clamp_pixel": "a sample off the frame reads the nearest frame pixel instead of 0",
    "rounded_gray": "gray is (r + g + b) / 3 rounded instead of truncated",
    "pairwise": "the leaves of a cascade are summed pairwise before they are added to the shape",
    "reversed": "the leaves are added in the order T - 1 .. 0",
    "drop_tail": "the trees after the last full group of twenty are not added",
    "fit_f32": "the similarity fit keeps its sums in float32",
    "prev_anchor": "cascade k > 0 samples around the anchors of cascade k - 1",
    "unsaturated": "the final conversion wraps out-of-range values to INT32_MIN (x86) instead of saturating",
}


class Trace(object):
    """what one or more landmarks() calls met"""

    def __init__(self):
        self.splits = self.ties = 0
        self.off = {"left": 0, "right": 0, "top": 0, "bottom": 0}
        self.inside = self.last_row = self.last_col = 0
        self.half = 0                 # final coordinates with floor(x + 0.5) on the boundary: x - floor(x) == 0.5 exactly
        self.sat_hi = self.sat_lo = 0
        self.max_uv = 0.0             # largest |u|, |v| of a sample in normalised coordinates
        self.max_leaf = 0             # deepest leaf index taken


def _fit(initial, cur, f32):
    """similarity_linear(initial -> cur): the four float32 of M"""
    n = len(initial) // 2
    t = F32 if f32 else float
    fr = [t(v) for v in initial]
    to = [t(v) for v in cur]
    mfx = mfy = mtx = mty = t(0)
    for i in range(n):
        mfx = mfx + fr[2 * i]; mfy = mfy + fr[2 * i + 1]; mtx = mtx + to[2 * i]; mty = mty + to[2 * i + 1]
    nn = t(n)
    mfx = mfx / nn; mfy = mfy / nn; mtx = mtx / nn; mty = mty / nn
    a = b = s = t(0)
    for i in range(n):
        fx, fy = fr[2 * i] - mfx, fr[2 * i + 1] - mfy
        tx, ty = to[2 * i] - mtx, to[2 * i + 1] - mty
        a = a + (fx * tx + fy * ty)
        b = b + (fx * ty - fy * tx)
        s = s + (fx * fx + fy * fy)
    with np.errstate(all="ignore"):
        ca, cb = a / s, b / s
    return F32(ca), F32(-cb), F32(cb), F32(ca)


def _round(x, half_even):
    return np.rint(x) if half_even else np.floor(x + 0.5)


def _pairwise(rows):
    rows = list(rows)
    while len(rows) > 1:
        nxt = [rows[i] + rows[i + 1] for i in range(0, len(rows) - 1, 2)]
        if len(rows) % 2:
            nxt.append(rows[-1])
        rows = nxt
    return rows[0]


def landmarks(model, rgb, rect, defect=None, trace=None):
    """-> (int32 [68, 2] points, float32 [68, 2] shape after the last cascade)"""
    assert defect is None or defect in DEFECTS, defect
    C, T, P, NP, depth = (int(v) for v in model["sp.meta"])
    n_split = (1 << depth) - 1
    h, w = rgb.shape[:2]
    with np.errstate(over="ignore"):
        gray_sum = rgb.astype(np.int64).sum(axis=2)
    gray = ((gray_sum + 1) // 3 if defect == "rounded_gray" else gray_sum // 3).astype(F32)      # (s + 1) // 3 = s / 3 rounded, for integers
    initial = np.ascontiguousarray(model["sp.initial_shape"], F32).reshape(-1)
    anchors = model["sp.anchor_idx"].reshape(C, NP)
    deltas = np.ascontiguousarray(model["sp.deltas"], F32).reshape(C, NP, 2)
    idx1 = model["sp.split_idx1"].reshape(C, T, n_split)
    idx2 = model["sp.split_idx2"].reshape(C, T, n_split)
    thresh = np.ascontiguousarray(model["sp.split_thresh"], F32).reshape(C, T, n_split)
    leaves = np.ascontiguousarray(model["sp.leaves"], F32).reshape(C, T, 1 << depth, 2 * P)
    sx, sy = float(rect[2]) - float(rect[0]), float(rect[3]) - float(rect[1])
    ox, oy = float(rect[0]), float(rect[1])
    cur = initial.copy()
    trees = np.arange(T)
    for it in range(C):
        M = _fit(initial, cur, defect == "fit_f32")
        an = anchors[it - 1 if (defect == "prev_anchor" and it > 0) else it]
        dx, dy = deltas[it, :, 0], deltas[it, :, 1]
        u = (M[0] * dx + M[1] * dy) + cur[2 * an]                      # float32 arrays: one rounding per operation, as the scalars
        v = (M[2] * dx + M[3] * dy) + cur[2 * an + 1]
        assert u.dtype == F32 and v.dtype == F32
        X = u.astype(np.float64) * sx + ox
        Y = v.astype(np.float64) * sy + oy
        px, py = _round(X, defect == "half_even"), _round(Y, defect == "half_even")      # float64, integral: compared as such
        inside = (px >= 0) & (py >= 0) & (px < w) & (py < h)
        pix = np.zeros(NP, F32)
        if defect == "clamp_pixel":
            pix[:] = gray[np.clip(py, 0, h - 1).astype(np.int64), np.clip(px, 0, w - 1).astype(np.int64)]
        else:
            pix[inside] = gray[py[inside].astype(np.int64), px[inside].astype(np.int64)]
        if trace is not None:
            trace.max_uv = max(trace.max_uv, float(np.abs(u).max()), float(np.abs(v).max()))
            trace.inside += int(inside.sum())
            trace.off["left"] += int((px < 0).sum()); trace.off["right"] += int((px >= w).sum())
            trace.off["top"] += int((py < 0).sum()); trace.off["bottom"] += int((py >= h).sum())
            trace.last_row += int((inside & (py == h - 1)).sum()); trace.last_col += int((inside & (px == w - 1)).sum())
        node = np.zeros(T, np.int64)
        for _ in range(depth):                                          # the trees of a cascade decide independently of each other
            diff = pix[idx1[it, trees, node]] - pix[idx2[it, trees, node]]
            th = thresh[it, trees, node]
            left = (diff >= th) if defect == "ge" else (diff > th)
            if trace is not None:
                trace.splits += T
                trace.ties += int((diff == th).sum())
            node = np.where(left, 2 * node + 1, 2 * node + 2)
        leaf = node - n_split
        if trace is not None:
            trace.max_leaf = max(trace.max_leaf, int(leaf.max()))
        rows = leaves[it, trees, leaf]                                  # [T, 136]
        if defect == "drop_tail":
            rows = rows[:T - T % 20]
        if defect == "reversed":
            rows = rows[::-1]
        if defect == "pairwise":
            if len(rows):
                cur = cur + _pairwise(rows)
        else:
            for r in rows:                                              # the chain over trees, all 136 coordinates at a time
                cur = cur + r
        assert cur.dtype == F32
    shape = cur.reshape(P, 2).copy()
    with np.errstate(invalid="ignore"):
        X = shape[:, 0].astype(np.float64) * sx + ox
        Y = shape[:, 1].astype(np.float64) * sy + oy
        R = np.stack([_round(X, defect == "half_even"), _round(Y, defect == "half_even")], axis=1)
        raw = np.stack([X, Y], axis=1)
        if trace is not None:
            trace.half += int((raw - np.floor(raw) == 0.5).sum())
            trace.sat_hi += int((R > I32_MAX).sum()); trace.sat_lo += int((R < I32_MIN).sum())
        if defect == "unsaturated":
            out = np.where((R > I32_MAX) | (R < I32_MIN) | np.isnan(R), float(I32_MIN), R)
        else:
            out = np.fmin(np.fmax(R, float(I32_MIN)), float(I32_MAX))   # fmax / fmin drop a NaN: INT32_MIN
    return out.astype(np.int64).astype(np.int32), shape


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))
