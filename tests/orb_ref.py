"""Test infrastructure: a numpy restatement of the ORB extraction and of the Hamming ratio-test matcher (csrc/orb.hip), written
independently of the kernels.  The behaviours recalled from OpenCV 3.4 that it states (and that ORB.md lists with what would flip each
one) are those of `cv2.ORB_create()` with its defaults, run by the reference's shot threading (structure/thread.py:139-150).

Integer arithmetic everywhere except the Harris response (float32, in OpenCV's order), the centroid angle (fastAtan2 in float32) and
the rotation of the sampling pattern (float32 with cos / sin computed in double and rounded) -- the kernels do the same operations in
the same order without contraction, so the two agree bit for bit.
"""
import math

import numpy as np

NFEATURES, SCALE_FACTOR, NLEVELS, EDGE, FAST_T, PATCH = 500, 1.2, 8, 31, 20, 31
HALF = PATCH // 2
HARRIS_BLOCK, HARRIS_K = 7, np.float32(0.04)
# FAST-9/16 circle (x, y), in order around the circle
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
          (-2, 2), (-1, 3)]
f32 = np.float32


def level_quota(nfeatures=NFEATURES, scale_factor=SCALE_FACTOR, nlevels=NLEVELS):
    """features per pyramid level: a geometric series in float32, cvRound for all levels but the last, which takes the rest"""
    factor = f32(1.0 / scale_factor)
    want = f32(nfeatures) * (f32(1) - factor) / (f32(1) - f32(float(factor) ** nlevels))
    out, total = [], 0
    for _ in range(nlevels - 1):
        q = int(np.rint(want))
        out.append(q)
        total += q
        want = f32(want * factor)
    out.append(max(nfeatures - total, 0))
    return out


def level_sizes(w, h, scale_factor=SCALE_FACTOR, nlevels=NLEVELS):
    """(width, height) of every level: cvRound(side * (1 / 1.2^k)) in float32"""
    out = []
    for k in range(nlevels):
        s = f32(1) / f32(scale_factor ** k)
        out.append((int(np.rint(f32(w) * s)), int(np.rint(f32(h) * s))))
    return out


def umax():
    """half-widths of the radius-15 disc of the intensity centroid, made symmetric as OpenCV does"""
    u = [0] * (HALF + 2)
    vmax = int(math.floor(HALF * float(np.sqrt(f32(2))) / 2 + 1))
    vmin = int(math.ceil(HALF * float(np.sqrt(f32(2))) / 2))
    for v in range(vmax + 1):
        u[v] = int(np.rint(math.sqrt(HALF * HALF - v * v)))
    v0 = 0
    for v in range(HALF, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return u[:HALF + 1]


def gaussian7():
    """GaussianBlur(7 x 7, sigma 2) on 8-bit images: the bit-exact kernel in 8 fraction bits (error diffusion over the taps, the centre
    takes the rest of 256)"""
    n, sigma = 7, 2.0
    vals = [math.exp((x * x) * (-0.125 / (sigma * sigma))) for x in range(1 - n, 0, 2)]
    s = 1.0 / (2 * sum(vals) + 1.0)
    k, err, total = [0] * n, 0.0, 0
    for i, v in enumerate(vals):
        adj = v * s * 256 + err
        r = int(np.rint(adj))
        err = adj - r
        k[i] = k[n - 1 - i] = r
        total += r
    k[n // 2] = 256 - 2 * total
    return k


def make_pattern(npoints=512):
    """OpenCV's makeRandomPattern: RNG(0x34985739), x then y uniform in [-15, 16) for each point (256 point pairs)"""
    state = 0x34985739
    out = []
    for _ in range(2 * npoints):
        state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & 0xFFFFFFFFFFFFFFFF
        out.append(int((state & 0xFFFFFFFF) % (PATCH)) - HALF)
    return np.array(out, np.int32).reshape(npoints, 2)


def _lin_table(inn, out):
    """cv2.resize INTER_LINEAR, 8 bit: source index and 11-bit coefficients (float fraction, cvRound)"""
    scale = inn / out
    idx = np.zeros(out, np.int64)
    c = np.zeros((out, 2), np.int64)
    for d in range(out):
        f = f32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = f32(f - f32(s))
        if s < 0:
            f, s = f32(0), 0
        if s >= inn - 1:
            f, s = f32(0), inn - 1
        idx[d] = s
        c[d] = (int(np.int16(np.rint(f32(f32(1) - f) * f32(2048)))), int(np.int16(np.rint(f * f32(2048)))))
    return idx, c


def resize_linear_rgb(img, ow, oh):
    """cv2.resize(rgb, (ow, oh)) -- the arithmetic of oracle.cv_resize"""
    ih, iw = img.shape[:2]
    xi, xc = _lin_table(iw, ow)
    yi, yc = _lin_table(ih, oh)
    a = img.astype(np.int64)
    x1 = np.minimum(xi + 1, iw - 1)
    y1 = np.minimum(yi + 1, ih - 1)
    S0 = a[yi][:, xi] * xc[None, :, 0, None] + a[yi][:, x1] * xc[None, :, 1, None]
    S1 = a[y1][:, xi] * xc[None, :, 0, None] + a[y1][:, x1] * xc[None, :, 1, None]
    out = (((yc[:, 0, None, None] * (S0 >> 4)) >> 16) + ((yc[:, 1, None, None] * (S1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def gray(rgb):
    """cv2.cvtColor(rgb, COLOR_RGB2GRAY), 8 bit"""
    a = rgb.astype(np.int64)
    return ((a[..., 0] * 4899 + a[..., 1] * 9617 + a[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def _exact_table(inn, out):
    """INTER_LINEAR_EXACT: double source position, coefficients in 8 fraction bits (c1 = cvRound(frac * 256), c0 = 256 - c1);
    positions left of the first pixel or right of the last one take that pixel alone"""
    scale = inn / out
    idx = np.zeros(out, np.int64)
    c = np.zeros((out, 2), np.int64)
    for d in range(out):
        fx = (d + 0.5) * scale - 0.5
        s = int(math.floor(fx))
        if s < 0:
            idx[d], c[d] = 0, (256, 0)
        elif s >= inn - 1:
            idx[d], c[d] = inn - 1, (256, 0)
        else:
            c1 = int(np.rint((fx - s) * 256))
            idx[d], c[d] = s, (256 - c1, c1)
    return idx, c


def resize_exact(img, ow, oh):
    ih, iw = img.shape
    xi, xc = _exact_table(iw, ow)
    yi, yc = _exact_table(ih, oh)
    a = img.astype(np.int64)
    x1 = np.minimum(xi + 1, iw - 1)
    y1 = np.minimum(yi + 1, ih - 1)
    H0 = a[yi][:, xi] * xc[None, :, 0] + a[yi][:, x1] * xc[None, :, 1]
    H1 = a[y1][:, xi] * xc[None, :, 0] + a[y1][:, x1] * xc[None, :, 1]
    return ((H0 * yc[:, 0, None] + H1 * yc[:, 1, None] + 32768) >> 16).astype(np.uint8)


def pyramid(g, nlevels=NLEVELS):
    """level 0 = the gray image; level k = INTER_LINEAR_EXACT resize of level k - 1 to level_sizes()[k]"""
    h, w = g.shape
    out = [g]
    for k, (lw, lh) in enumerate(level_sizes(w, h, nlevels=nlevels)[1:], 1):
        out.append(resize_exact(out[-1], lw, lh))
    return out


def _r101(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def blur(img):
    """GaussianBlur(img, (7, 7), 2, 2, BORDER_REFLECT_101) on 8 bits: rows into 8 fraction bits, then columns, round half up"""
    k = np.array(gaussian7(), np.int64)
    h, w = img.shape
    a = img.astype(np.int64)
    xs = np.arange(w)
    H = sum(k[j] * a[:, _r101(xs + j - 3, w)] for j in range(7))
    ys = np.arange(h)
    V = sum(k[i] * H[_r101(ys + i - 3, h)] for i in range(7))
    return ((V + 32768) >> 16).astype(np.uint8)


def fast_scores(img, lo=3):
    """FAST-9/16 (threshold 20) score map: 0 where the pixel is not a corner, else the largest threshold for which it still is one,
    minus 1 (OpenCV's cornerScore<16>).  Computed for pixels lo <= x < w - lo, lo <= y < h - lo (lo >= 3)."""
    h, w = img.shape
    a = img.astype(np.int32)
    S = np.zeros((h, w), np.int32)
    if h - 2 * lo <= 0 or w - 2 * lo <= 0:
        return S
    v = a[lo:h - lo, lo:w - lo]
    d = np.stack([v - a[lo + dy:h - lo + dy, lo + dx:w - lo + dx] for dx, dy in CIRCLE])      # [16, ...]: centre minus circle
    dd = np.concatenate([d, d[:8]])
    arc_min = np.stack([dd[s:s + 9].min(0) for s in range(16)])     # darker circle
    arc_max = np.stack([dd[s:s + 9].max(0) for s in range(16)])     # brighter circle
    best = np.maximum(arc_min.max(0), (-arc_max).max(0))
    corner = best > FAST_T
    S[lo:h - lo, lo:w - lo] = np.where(corner, best - 1, 0)
    return S


def nms_candidates(S, w, h):
    """3 x 3 non-maximum suppression (strictly above all eight neighbours) and runByImageBorder(31): (y, x) in raster order"""
    if w <= 2 * EDGE or h <= 2 * EDGE:
        return np.zeros((0, 2), np.int64)
    P = np.pad(S, 1)
    c = P[1:-1, 1:-1]
    keep = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                keep &= c > P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    m = np.zeros_like(keep)
    m[EDGE:h - EDGE, EDGE:w - EDGE] = True
    return np.argwhere(keep & m)


def retain_best(resp, n):
    """KeyPointsFilter::retainBest: when there are more than n, keep every point whose response is >= the n-th largest (ties kept)"""
    resp = np.asarray(resp)
    if len(resp) <= n:
        return np.ones(len(resp), bool)
    if n == 0:
        return np.zeros(len(resp), bool)
    thr = np.sort(resp)[::-1][n - 1]
    return resp >= thr


def harris(img, ys, xs):
    """HarrisResponses(block 7, k = 0.04): integer Sobel sums, the response in float32 in OpenCV's order"""
    a = img.astype(np.int64)
    A = np.zeros(len(ys), np.int64); B = np.zeros(len(ys), np.int64); Cc = np.zeros(len(ys), np.int64)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            y, x = ys + dy, xs + dx
            ix = (a[y, x + 1] - a[y, x - 1]) * 2 + (a[y - 1, x + 1] - a[y - 1, x - 1]) + (a[y + 1, x + 1] - a[y + 1, x - 1])
            iy = (a[y + 1, x] - a[y - 1, x]) * 2 + (a[y + 1, x - 1] - a[y - 1, x - 1]) + (a[y + 1, x + 1] - a[y - 1, x + 1])
            A += ix * ix; B += iy * iy; Cc += ix * iy
    scale = f32(1) / (f32(4 * HARRIS_BLOCK) * f32(255))
    ssss = f32(f32(f32(scale * scale) * scale) * scale)
    fa, fb, fc = A.astype(np.float32), B.astype(np.float32), Cc.astype(np.float32)
    s = fa + fb
    return (((fa * fb) - (fc * fc)) - ((HARRIS_K * s) * s)) * ssss


_P1, _P3, _P5, _P7 = (f32(f32(c) * f32(180 / math.pi)) for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281,
                                                                    -0.04432655554792128))
_EPS = f32(2.220446049250313e-16)


def fast_atan2(y, x):
    """cv::fastAtan2 in float32 (degrees, [0, 360))"""
    y, x = f32(y), f32(x)
    ax, ay = abs(x), abs(y)
    if ax >= ay:
        c = ay / (ax + _EPS); c2 = c * c
        a = (((_P7 * c2 + _P5) * c2 + _P3) * c2 + _P1) * c
    else:
        c = ax / (ay + _EPS); c2 = c * c
        a = f32(90) - (((_P7 * c2 + _P5) * c2 + _P3) * c2 + _P1) * c
    if x < 0:
        a = f32(180) - a
    if y < 0:
        a = f32(360) - a
    return f32(a)


_UMAX = umax()


def ic_angle(img, y, x):
    a = img.astype(np.int64)
    m10 = int((np.arange(-HALF, HALF + 1) * a[y, x - HALF:x + HALF + 1]).sum())
    m01 = 0
    for v in range(1, HALF + 1):
        d = _UMAX[v]
        u = np.arange(-d, d + 1)
        p, m = a[y + v, x - d:x + d + 1], a[y - v, x - d:x + d + 1]
        m01 += v * int((p - m).sum())
        m10 += int((u * (p + m)).sum())
    return fast_atan2(f32(m01), f32(m10))


_PATTERN = make_pattern()
_DEG2RAD = f32(math.pi / f32(180))


def descriptor(bl, y, x, angle):
    """rotated BRIEF on the blurred level image: 256 comparisons of rotated pattern points (cvRound), 32 bytes"""
    ang = f32(angle * _DEG2RAD)
    ca, sa = f32(math.cos(float(ang))), f32(math.sin(float(ang)))
    px = _PATTERN[:, 0].astype(np.float32)
    py = _PATTERN[:, 1].astype(np.float32)
    rx = np.rint(px * ca - py * sa).astype(np.int64)
    ry = np.rint(px * sa + py * ca).astype(np.int64)
    vals = bl[y + ry, x + rx].astype(np.int32)
    bits = (vals[0::2] < vals[1::2]).astype(np.uint8)             # 256 bits, bit k of byte i = pair 8 i + k
    return np.packbits(bits.reshape(32, 8), axis=1, bitorder="little").reshape(32)


def orb_gray(g):
    """ORB on one gray image (cv2.ORB_create() defaults).  Returns (keypoints [K, 6] float64 rows of
    (x, y, level, fast score, harris response, angle) in level / y / x order, coordinates in level pixels; descriptors uint8 [K, 32])"""
    quota = level_quota()
    kps, descs = [], []
    for lv, img in enumerate(pyramid(g)):
        h, w = img.shape
        if w <= 2 * EDGE or h <= 2 * EDGE:
            continue
        S = fast_scores(img, lo=EDGE - 1)
        yx = nms_candidates(S, w, h)
        score = S[yx[:, 0], yx[:, 1]]
        yx, score = yx[retain_best(score, 2 * quota[lv])], score[retain_best(score, 2 * quota[lv])]
        resp = harris(img, yx[:, 0], yx[:, 1])
        keep = retain_best(resp, quota[lv])
        yx, score, resp = yx[keep], score[keep], resp[keep]
        if not len(yx):
            continue
        bl = blur(img)
        for (y, x), s, r in zip(yx, score, resp):
            ang = ic_angle(img, y, x)
            kps.append((x, y, lv, s, float(r), float(ang)))
            descs.append(descriptor(bl, y, x, ang))
    return np.array(kps, np.float64).reshape(-1, 6), np.array(descs, np.uint8).reshape(-1, 32)


def thread_size(frame_w, frame_h, height=200):
    """(width, height) of the small image: (height, int(w * height / h)) handed to cv2.resize as dsize (thread.py:104)"""
    return int(height), int(frame_w * height / frame_h)


def orb_frame(rgb, height=200):
    """structure/thread.py:139-150: resize the RGB frame, convert to gray, ORB"""
    ow, oh = thread_size(rgb.shape[1], rgb.shape[0], height)
    return orb_gray(gray(resize_linear_rgb(rgb, ow, oh)))


# ---- matching
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    """[na, nb] Hamming distances between 32-byte descriptors"""
    return _POP[np.bitwise_xor(a[:, None, :], b[None, :, :])].sum(-1)


def match_count(a, b):
    """thread.py:152-170 with an exact 2-NN: 0 when either side has fewer than 2 rows, else the rows of `a` whose best and second-best
    distances in `b` pass d1 < 0.7 d2 (for integers: 10 d1 < 7 d2)"""
    if a is None or b is None or len(a) < 2 or len(b) < 2:
        return 0
    d = np.sort(hamming(a, b), axis=1)
    return int(np.count_nonzero(10 * d[:, 0] < 7 * d[:, 1]))
