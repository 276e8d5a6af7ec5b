"""The planes, frames and the planted clip that tests/test_blend_ref.py (CPU: the restatement against hand cases and planted defects) and
tests/test_gpu_blend.py (GPU: the kernels against the restatement) share."""
import collections

import numpy as np

# pvf_blend_measure: the head and tail of the 32-bit loads (1 .. 5), one wave's reach of 64 dwords (255 .. 257), a lane's second dword,
# odd P (planes start at odd addresses), the verb's own 64 x 36, and the cap
PIXELS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2304, 16383, 16384)
COUNTS = (1, 2, 4, 5, 32, 33, 70)
CONTENTS = ("zeros", "jump16", "jump2", "alternate", "random", "ramp")
N_MOST = max(COUNTS)


def planes(content, N, P, seed=0):
    """uint8 [N, P]"""
    t = np.arange(N, dtype=np.int64)[:, None]
    p = np.arange(P, dtype=np.int64)[None, :]
    if content == "zeros":
        y = np.zeros((N, P), np.int64)
    elif content == "jump16":                    # 16 planes of 0, 16 of 255, ...: at t = 32 the lag 32 sees 0, 255, 0 -- R = 510 P, the largest
        y = 255 * ((t // 16) % 2) + 0 * p
    elif content == "jump2":                     # the same for the lag 4 at t = 4, 8, ...
        y = 255 * ((t // 2) % 2) + 0 * p
    elif content == "alternate":                 # a checkerboard of the extremes that flips with every frame
        y = 255 * ((t + p) % 2)
    elif content == "random":
        y = np.random.default_rng(1000 * seed + P).integers(0, 256, (N, P))
    elif content == "ramp":                      # Y_t = c + k t exactly: R = 0, E_L = k L summed over the pixels
        y = (p % 40) + (1 + p % 3) * t
        assert y.max() <= 255
    else:
        raise KeyError(content)
    return y.astype(np.uint8)


def firsts(N):
    """first at 0, at N, and either side of every lag"""
    return sorted(set(f for L in (1, 4, 8, 16, 32) for f in (L - 1, L, L + 1) if 0 <= f <= N) | {0, N})


# pvf_frame_blend: (w, h, tw, th); 3 w takes every residue mod 4, 1 x 1 and 1080p are the ends, P is odd, even and a multiple of 4
FRAME_SIZES = ((1, 1, 1, 1), (5, 3, 5, 3), (6, 5, 3, 2), (7, 4, 7, 3), (8, 9, 4, 5), (33, 21, 16, 9), (160, 90, 32, 18), (1920, 1080, 64, 36))
HISTORIES = (0, 1, 3, 4, 5, 31, 32)


def frames_of(w, h, n, seed=0):
    """n frames that drift: noise over a gradient that moves, so that every lag sees something of its own"""
    rng = np.random.default_rng(77 + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for t in range(n):
        base = (xx * 3 + yy * 5 + 4 * t) % 256
        f = np.stack([base, (base * 2 + t) % 256, 255 - base], axis=2) + rng.integers(-20, 21, (h, w, 3))
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


# ---- the planted clip ---------------------------------------------------------------------------------------------------------------
CLIP_W, CLIP_H, CLIP_WIDTH, CLIP_FPS = 160, 90, 32, 25.0        # reduced 5 : 1 to 32 x 18
Plant = collections.namedtuple("Plant", "kind first last")       # the last pure frame before the ramp, the first pure frame after it
Clip = collections.namedtuple("Clip", "frames plants quiet")     # quiet: (what, first, last) stretches in which nothing may be reported


def _texture(rng, h, w, cell=10):
    """a picture of soft blobs, 40 .. 215: coarse enough to survive the reduction"""
    coarse = rng.integers(40, 216, (h // cell + 2, w // cell + 2, 3)).astype(np.float64)
    big = np.kron(coarse, np.ones((cell, cell, 1)))
    k = np.ones(cell) / cell
    for axis in (0, 1):
        big = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), axis, big)
    return big[cell // 2:cell // 2 + h, cell // 2:cell // 2 + w]


def planted_clip(seed=5, sigma=3.0):
    """still, dissolve (15 mixed frames), still, cut, slow pan (1 pixel a frame), fade-out (11), black, fade-in (5), still, one flash
    frame, still; noise of `sigma` on every frame"""
    rng = np.random.default_rng(seed)
    h, w = CLIP_H, CLIP_W
    A, B, D = (_texture(rng, h, w) for _ in range(3))
    # the pan's picture is fine-grained and hard-edged: under the reduction a pixel's value then walks at random as columns enter and
    # leave it, which is what a pan over detail does; a pan over soft blobs is a linear change over 4 frames and is found as a dissolve
    wide = np.kron(rng.integers(40, 216, (h // 2, (w + 40) // 2, 3)).astype(np.float64), np.ones((2, 2, 1)))
    black = np.zeros((h, w, 3))
    pure, plants, quiet = [], [], []

    def hold(img, n, what=None):
        if what:
            quiet.append((what, len(pure), len(pure) + n - 1))
        pure.extend([img] * n)

    def ramp(a, b, mixed, kind):
        plants.append(Plant(kind, len(pure) - 1, len(pure) + mixed))
        for k in range(1, mixed + 1):
            pure.append(a + (b - a) * (k / float(mixed + 1)))
    hold(A, 14, "still")
    ramp(A, B, 15, "dissolve")
    hold(B, 14, "still")
    quiet.append(("cut", len(pure) - 1, len(pure)))
    start = len(pure)
    for k in range(30):
        pure.append(wide[:, k:k + w])
    quiet.append(("pan", start, len(pure) - 1))
    last = pure[-1]
    hold(last, 6)
    ramp(last, black, 11, "fade-out")
    hold(black, 9)
    ramp(black, D, 5, "fade-in")
    hold(D, 36, "still")                         # longer than the widest window: no window holds the fade-in and the flash
    quiet.append(("flash", len(pure) - 1, len(pure) + 1))
    pure.append(np.full((h, w, 3), 255.0))
    hold(D, 8, "still")
    frames = [np.clip(np.rint(f + rng.normal(0.0, sigma, f.shape)), 0, 255).astype(np.uint8) for f in pure]
    return Clip(frames, plants, quiet)
