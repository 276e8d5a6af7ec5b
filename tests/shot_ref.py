"""Plain numpy restatements of the three parts of the shot detector that can be restated exactly, written from
pyannote/video/structure/shot.py and the comments of oracle/pvo_shot.c; they never call the oracle.  tests/test_shot_edge_cases.py holds
them equal to the oracle bit for bit, so that the oracle's integer conversion, its pyramid plan and its displaced lookup each have a second,
independent statement.  The Farneback arithmetic itself has none: it stays pinned to the oracle (PARITY UNPINNED against OpenCV)."""
import math

import numpy as np


# ---- shot.py:71-73: cv2.cvtColor(rgb, COLOR_RGB2GRAY), then cv2.resize(gray, (ow, oh)) (8-bit INTER_LINEAR)
def resize_coeffs(n_in, n_out):
    """per output index: the first source index and the two 11-bit weights (the source coordinate is a float32, its fraction too;
    both ends clamp with weight 2048 on one pixel)"""
    scale = float(n_in) / float(n_out)
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    low, high = s < 0, s >= n_in - 1
    f[low | high] = 0
    s[low] = 0
    s[high] = n_in - 1
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)      # (ties to even, like nearbyintf)
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, c0, c1


def convert(rgb, ow, oh):
    """uint8 [oh, ow]: 14-bit gray, two 11-bit blends, `>> 4`, `>> 16` per row term, `+ 2 >> 2`; all in int64"""
    rgb = np.asarray(rgb).astype(np.int64)
    ih, iw = rgb.shape[:2]
    gray = (rgb[..., 0] * 4899 + rgb[..., 1] * 9617 + rgb[..., 2] * 1868 + 8192) >> 14
    sy, b0, b1 = resize_coeffs(ih, oh)
    sx, a0, a1 = resize_coeffs(iw, ow)
    sy1, sx1 = np.minimum(sy + 1, ih - 1), np.minimum(sx + 1, iw - 1)
    S0 = gray[sy][:, sx] * a0 + gray[sy][:, sx1] * a1
    S1 = gray[sy1][:, sx] * a0 + gray[sy1][:, sx1] * a1
    out = (((b0[:, None] * (S0 >> 4)) >> 16) + ((b1[:, None] * (S1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


# ---- the pyramid of cv2.calcOpticalFlowFarneback(prev, cur, None, 0.5, 3, 15, 3, 5, 1.1, 0)
def cv_round(v):
    """cvRound: to nearest, ties to even (Python's round on a float does exactly that)"""
    return int(round(float(v)))


def levels(h, w):
    """coarser levels: halve while both sides stay at 32 pixels or more, three times at most"""
    k, scale = 0, 1.0
    while k < 3:
        scale *= 0.5
        if w * scale < 32 or h * scale < 32:
            break
        k += 1
    return k


def gauss_taps(n, sigma):
    """getGaussianKernel(n, sigma, CV_32F): exp in double, kept as float32, normalised by the double sum of the float32 values"""
    s2 = -0.5 / (sigma * sigma)
    t = []
    for i in range(n):
        x = i - (n - 1) * 0.5
        t.append(np.float32(math.exp(s2 * x * x)))          # (in this order: s2 is not a dyadic number for sigma = 1.5 and 3.5)
    total = 0.0
    for v in t:
        total += float(v)
    total = 1.0 / total
    return np.array([np.float32(float(v) * total) for v in t], np.float32)


def level_plan(h, w):
    """[(level height, level width, smoothing size, float32 taps)] for k = 0 .. levels; level 0 has the fixed 3 x 3 kernel and no taps"""
    out = []
    for k in range(levels(h, w) + 1):
        scale = 0.5 ** k
        sigma = (1.0 / scale - 1) * 0.5
        size = max(cv_round(sigma * 5) | 1, 3)
        out.append((cv_round(h * scale), cv_round(w * scale), size, gauss_taps(size, sigma) if k else np.zeros(0, np.float32)))
    return out


# ---- shot.py:89-99: reconstruct[y, x] = current[int(clamp(y + dy)), int(clamp(x + dx))] with `dy, dx = flow[y, x]`
def displaced_lookup(flow):
    """(row, column) the reference reads for every pixel: float32 sums (NumPy >= 2 keeps `int + float32` in float32), the four clamps,
    truncation"""
    h, w = flow.shape[:2]
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    fx = x + flow[..., 1].astype(np.float32)
    fy = y + flow[..., 0].astype(np.float32)
    assert fx.dtype == np.float32 and fy.dtype == np.float32
    fx = np.where(fx > np.float32(w - 1), np.float32(w - 1), fx)
    fx = np.where(fx < 0, np.float32(0), fx)
    fy = np.where(fy > np.float32(h - 1), np.float32(h - 1), fy)
    fy = np.where(fy < 0, np.float32(0), fy)
    return fy.astype(np.int64), fx.astype(np.int64)


def dfd_from_flow(prev, cur, flow):
    """mean |previous - current displaced by the flow|: an integer sum divided once"""
    ry, rx = displaced_lookup(flow)
    d = np.abs(prev.astype(np.int64) - cur.astype(np.int64)[ry, rx])
    return float(int(d.sum())) / float(prev.size)
