"""The flows, frames and clips that tests/test_motion_ref.py (CPU: the restatement against hand cases, the overflow proof, planted defects,
the camera rules) and tests/test_gpu_motion.py (GPU: csrc/motion.hip against the restatement) share.  Deterministic builders only."""
import collections

import numpy as np

# (w, h): fewer pixels than the block has lanes; odd sides and an odd pixel count; the `blend` thumbnail's size; the verb's own 96 x 54; the
# three shapes at the cap of 16384 pixels, which hold the largest |X|, |Y| and sums
SIZES = ((12, 12), (13, 17), (64, 36), (96, 54), (128, 128), (256, 64), (64, 256))
CAP_SIZES = ((128, 128), (256, 64), (64, 256))
Q_MAX = 1 << 20                                  # |u|, |v| at most, in 1/64 pixel

WORST = ("worst_sums", "worst_pp", "worst_qq", "worst_left_half", "worst_top_half", "worst_checker")
CONTENTS = ("translation", "zoom", "roll", "planted18", "planted37", "nonfinite", "clip", "one_valid", "two_valid", "three_valid", "none_valid",
            "noise", "halves", "ties", "tau_edge") + WORST


def grid(w, h):
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    return 2 * x - (w - 1), 2 * y - (h - 1)


def from_units(u, v):
    """the float32 flow whose quantised components are u, v (|u|, |v| <= 2^20: a multiple of 1/64 is exact in float32)"""
    return np.stack([np.asarray(u, np.float64) / 64.0, np.asarray(v, np.float64) / 64.0], axis=2).astype(np.float32)


def similarity(w, h, tx, ty, a, b):
    """the exact flow of the model with integer parameters in 1/64 pixel: u = tx + a X - b Y, v = ty + b X + a Y"""
    X, Y = grid(w, h)
    return tx + a * X - b * Y, ty + b * X + a * Y


BACKGROUND = (96, -32, 1, 0)                     # a pan of 1.5 pixels right and half a pixel up, and a zoom


def rect_of(w, h, share):
    """(x0, y0, rw, rh) of the planted foreground: 18.5 % and 37 % of 96 x 54 are 40 x 24 and 60 x 32; off centre"""
    rw, rh = {18: (5 * w // 12, 4 * h // 9), 37: (5 * w // 8, 16 * h // 27)}[share]
    return w // 12, h // 9, max(rw, 1), max(rh, 1)


def planted(w, h, share):
    """the background's model everywhere but in a rectangle, which moves 3 pixels to the right of it: (flow, background pixel count)"""
    u, v = similarity(w, h, *BACKGROUND)
    x0, y0, rw, rh = rect_of(w, h, share)
    u = u.copy()
    u[y0:y0 + rh, x0:x0 + rw] += 192
    return from_units(u, v), w * h - rw * rh


def flow_of(content, w, h, seed=0):
    """float32 [h, w, 2]"""
    X, Y = grid(w, h)
    rng = np.random.default_rng(1000 * seed + 7 * w + h)
    zero = np.zeros((h, w), np.int64)
    if content == "translation":
        return from_units(zero + 96, zero - 40)
    if content == "zoom":
        return from_units(3 * X, 3 * Y)
    if content == "roll":
        return from_units(-2 * Y, 2 * X)
    if content in ("planted18", "planted37"):
        return planted(w, h, int(content[-2:]))[0]
    if content == "noise":                       # a model, noise of 0.02 pixel, and a tenth of the pixels anywhere within 8 pixels
        u, v = similarity(w, h, -50, 20, -1, 2)
        f = from_units(u, v) + rng.normal(0.0, 0.02, (h, w, 2)).astype(np.float32)
        wild = rng.random((h, w)) < 0.1
        f[wild] = rng.uniform(-8.0, 8.0, (int(wild.sum()), 2)).astype(np.float32)
        return f
    if content == "nonfinite":
        f = flow_of("noise", w, h, seed + 1)
        bad = rng.integers(0, 12, (h, w))
        f[bad == 0, 0] = np.nan
        f[bad == 1, 1] = np.inf
        f[bad == 2, 0] = -np.inf
        f[bad == 3] = np.nan
        return f
    if content == "clip":                        # the +-3e6 flows of tests/shot_cases.py's rank-one pairs: far beyond 2^20 / 64
        s = np.where((X + Y) % 4 < 2, 1.0, -1.0)
        return np.stack([3e6 * s, -3e6 * np.where(X > 0, 1.0, -1.0)], axis=2).astype(np.float32)
    if content in ("one_valid", "two_valid", "three_valid", "none_valid"):
        f = np.full((h, w, 2), np.nan, np.float32)
        spots = {"none_valid": [], "one_valid": [(h // 3, w // 2)], "two_valid": [(1, 2), (h - 2, w - 1)],
                 "three_valid": [(0, 0), (h - 1, 3), (h // 2, w - 1)]}[content]
        for k, (y, x) in enumerate(spots):
            f[y, x] = (1.25 + k, -0.5 * k)
        return f
    if content == "halves":                      # two motions of equal size: trimming has no majority to find
        return from_units(np.where(X < 0, 64, -64), zero + 3)
    if content == "tau_edge":
        # columns in six classes by |X|, u = 0, 0, 0, 17, 17, 64 sixty-fourths: at 12 x 12 the first fit leaves the columns of 17 with a
        # residual of exactly floor(sum / n) = 2 m + 1, so a tau without the floor keeps them and the right one drops them
        return from_units(np.array([0, 0, 0, 17, 17, 64])[(np.abs(X) // 2) % 6], zero)
    if content == "ties":                        # every component on a rounding tie of the quantiser: k + 1/2 sixty-fourths
        k = rng.integers(-300, 300, (h, w, 2))
        return ((k + 0.5) / 64.0).astype(np.float32)
    # ---- the largest sums there are: every component +-2^20, the signs chosen for one sum each
    top = zero + Q_MAX
    sx, sy = np.where(X > 0, 1, -1), np.where(Y > 0, 1, -1)
    if content == "worst_sums":                  # Su, Sv, and the translation's numerator
        return from_units(top, top)
    if content == "worst_pp":                    # sum (X u + Y v)
        return from_units(top * sx, top * sy)
    if content == "worst_qq":                    # sum (X v - Y u)
        return from_units(-top * sy, top * sx)
    if content in ("worst_left_half", "worst_top_half"):      # SX Su (SY Sv): one half of the image alone is valid
        f = from_units(top, -top)
        f[(X > 0) if content == "worst_left_half" else (Y > 0)] = np.nan
        return f
    if content == "worst_checker":               # the largest residuals: neighbours at opposite ends
        c = np.where(((X + Y) // 2) % 2 == 0, 1, -1)
        return from_units(top * c, -top * c)
    raise KeyError(content)


_CACHE = {}


def reference(content, w, h):
    """(flow, the restatement's row), computed once per process and shared read-only"""
    from tests import motion_ref
    key = (content, w, h)
    if key not in _CACHE:
        f = flow_of(content, w, h)
        r = motion_ref.row_of(f)
        f.setflags(write=False)
        r.setflags(write=False)
        _CACHE[key] = (f, r)
    return _CACHE[key]


# ---- clips -----------------------------------------------------------------------------------------------------------------------------
FPS = 25.0
CLIP_W, CLIP_H, CLIP_WIDTH = 192, 108, 96        # reduced 2 : 1 to 96 x 54
Clip = collections.namedtuple("Clip", "frames parts")          # parts: (kind, first frame, last frame)


def picture(xs, ys):
    """a smooth picture sampled at any real coordinates, 30 .. 230"""
    return (130.0 + 40.0 * np.sin(0.110 * xs + 0.050 * ys) + 30.0 * np.sin(0.070 * xs - 0.130 * ys + 1.0)
            + 20.0 * np.sin(0.031 * xs + 0.190 * ys + 2.0) + 10.0 * np.sin(0.230 * xs - 0.210 * ys))


def camera_clip(still=20, pan=24, zoom=24, sigma=1.0, seed=3):
    """a still, a pan (the content moves 2 source pixels a frame to the left: the camera pans right), a zoom in of 1 % a frame; noise of
    `sigma` on every frame"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:CLIP_H, 0:CLIP_W].astype(np.float64)
    cx, cy = (CLIP_W - 1) / 2.0, (CLIP_H - 1) / 2.0
    views = [(0.0, 1.0)] * still                 # (offset in x, scale about the centre)
    views += [(2.0 * k, 1.0) for k in range(1, pan + 1)]
    views += [(2.0 * pan, 1.01 ** k) for k in range(1, zoom + 1)]
    frames = []
    for off, s in views:
        g = picture(cx + (xs - cx) / s + off + 300.0, cy + (ys - cy) / s + 200.0)
        g = np.clip(np.rint(g + rng.normal(0.0, sigma, g.shape)), 0, 255).astype(np.uint8)
        frames.append(np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)))
    parts = [("static", 0, still - 1), ("pan-right", still, still + pan - 1), ("zoom-in", still + pan, still + pan + zoom - 1)]
    return Clip(frames, parts)


def soft_pan_clip(seed=5, sigma=3.0):
    """BLEND.md's first planted clip, as far as `transition --motion` needs it: a still, a dissolve of 15 mixed frames, a still, a cut, a pan
    of 1 pixel a frame over blobs 10 pixels wide (which `transition` alone reports as a dissolve), a still.  160 x 90 at 25 frames a second,
    noise of sigma 3: the pictures of tests/blend_cases.py"""
    from tests import blend_cases as bc
    rng = np.random.default_rng(seed)
    h, w = bc.CLIP_H, bc.CLIP_W
    A, B = bc._texture(rng, h, w), bc._texture(rng, h, w)
    wide = bc._texture(rng, h, w + 40)
    pure, parts = [], []

    def part(kind, imgs):
        parts.append((kind, len(pure), len(pure) + len(imgs) - 1))
        pure.extend(imgs)
    part("still", [A] * 14)
    part("dissolve", [A + (B - A) * (k / 16.0) for k in range(1, 16)])
    part("still", [B] * 14)
    part("pan", [wide[:, k:k + w] for k in range(30)])
    part("still", [wide[:, 29:29 + w]] * 14)
    frames = [np.clip(np.rint(f + rng.normal(0.0, sigma, f.shape)), 0, 255).astype(np.uint8) for f in pure]
    return Clip(frames, parts)


def oracle_rows(frames, tw, th, fps=FPS):
    """what `motion` writes for these frames, from the oracle's small images and flows and the restatement's rows; once per process"""
    from oracle import oracle
    from tests import motion_ref, shot_cases
    key = ("rows", id(frames), tw, th)
    if key not in _CACHE:
        tables = oracle.shot_tables()
        gray = [oracle.shot_convert(f, tw, th) for f in frames]
        pairs = range(len(frames) - 1)
        flows = shot_cases.threaded(lambda i: oracle.farneback(gray[i], gray[i + 1], tables), pairs)
        dfd = np.array([oracle.shot_dfd_from_flow(gray[i], gray[i + 1], flows[i]) for i in pairs], np.float64)
        _CACHE[key] = (motion_ref.video_rows(np.stack(flows), dfd, tw, th, fps), frames)      # (the frames are kept: their id is the key)
    return _CACHE[key][0]
