"""The geometries, contents, parameters and planted clips that tests/test_text_ref.py (CPU: the restatement against worked values and
planted defects, and that this table reaches every seam and equality) and tests/test_gpu_text.py (GPU: the kernel against the
restatement) share."""
import numpy as np

STRIP_CELLS = 16                         # TX_STRIP_CELLS of csrc/text.hip: the cells of one workgroup, 256 columns
S = STRIP_CELLS

# w x h
GEOMETRIES = ((1, 1), (2, 1), (1, 2),                                          # the smallest frames
              (5, 3), (7, 9), (21, 16),                                        # 3 w = 15, 21, 63: rows start at every byte alignment
              (15, 15), (16, 16), (17, 17), (31, 16), (33, 32), (16, 257),     # cell seams
              (511, 16), (512, 16), (513, 16), (1030, 20),                     # cw = 32, 32, 33 and 65: the mask-word seam
              (S * 16 - 1, 17), (S * 16, 17), (S * 16 + 1, 17))                # either side of the strip
CONTENTS = ("constant", "noise", "repeat", "step", "alternate", "ramp", "saturated", "edge_eq", "still_eq", "on_eq")
PARAMS = ((1, 0, 1), (48, 8, 24), (255, 254, 256))                             # (edge, still, on)
N_FRAMES = 5


def grey(y):
    return np.repeat(np.asarray(y)[..., None], 3, axis=2).astype(np.uint8)


def _row_with(strokes, base, w):
    """a row of luma, 0 or 255, with exactly `strokes` stroke pixels (gx = 255) in the cell that starts at column `base` (a multiple
    of 16, base >= 16, base + 16 <= w - 1), whatever the edge; it touches columns base - 1 .. base + 16 only"""
    y = np.zeros(w, np.int64)
    if strokes >= 15:
        x = np.arange(base - 1, base + 17)
        y[x] = 255 * ((x >> 1) & 1)
        if strokes == 15:
            y[base + 16] = 255                   # takes the stroke at base + 15 away
    elif strokes == 3:
        y[base - 1] = y[base + 2] = 255
    elif strokes == 2:
        y[base + 2] = 255
    elif strokes == 1:
        y[base - 1] = 255
    return y


def cell_with(target, base, w):
    """16 rows of luma with `target` stroke pixels in the cell at column `base`"""
    rows, left = [], target
    for _ in range(16):
        take = next(k for k in (16, 15, 3, 2, 1, 0) if k <= left)
        rows.append(_row_with(take, base, w))
        left -= take
    assert left == 0, target
    return np.stack(rows)


def frames_of(content, w, h, params=(48, 8, 24), n=N_FRAMES, seed=0):
    """n frames uint8 [h][w][3]"""
    edge, still, on = params
    rng = np.random.default_rng(1000 * w + h + 7 * seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "constant":
        return [grey(np.full((h, w), 100))] * n
    if content == "noise":
        return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    if content == "repeat":
        return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8)] * n
    if content == "step":
        return [grey(255 * (xx >= min(16, w // 2)))] * n
    if content == "alternate":
        return [grey(255 * (xx & 1))] * n
    if content == "ramp":                        # Y = 3 x, cut at 255
        return [grey(np.minimum(3 * xx, 255))] * n
    if content == "saturated":                   # blocks of the eight corner colours; every other frame shifted by a column
        a = 255 * rng.integers(0, 2, (h // 3 + 1, w // 2 + 2, 3))
        big = np.kron(a, np.ones((3, 2, 1), np.int64))
        return [big[:h, (t & 1):(t & 1) + w].astype(np.uint8) for t in range(n)]
    if content == "edge_eq":                     # columns 0, 0, e, e, ...: gx = e inside; e = edge on even rows, edge - 1 on odd rows
        e = np.where(yy & 1, edge - 1, edge)
        return [grey(e * ((xx >> 1) & 1))] * n
    if content == "still_eq":                    # frames A, B, A, ...: B = A + still on even columns, A + still + 1 on odd columns
        top = 255 - (still + 1)
        a = top * rng.integers(0, 2, (h, w))
        b = a + np.where(xx & 1, still + 1, still)
        return [grey(b if t & 1 else a) for t in range(n)]
    if content == "on_eq":                       # one frame repeated: S = on in cell (0, 1) and on - 1 in cell (0, 3), where they exist
        y = np.zeros((h, w), np.int64)
        if h >= 16:
            for base, target in ((16, on), (48, on - 1)):
                if base + 16 <= w - 1:
                    y[:16] += cell_with(target, base, w)
        return [grey(y)] * n
    raise KeyError(content)


def cases():
    """(w, h, content, params) of the whole table"""
    return [(w, h, c, p) for w, h in GEOMETRIES for c in CONTENTS for p in PARAMS]


# ---- the planted clips ----------------------------------------------------------------------------------------------------------------
CLIP_W, CLIP_H, CLIP_FPS, CLIP_N = 320, 180, 25.0, 100
STRAP = (64, 128, 224, 160)              # left, top, right, bottom
STRAP_FRAMES = (30, 79)                  # first and last frame with the strap


def planted_clip(moving=True, strap=True, seed=3):
    """CLIP_N frames: a background of 6-pixel blocks of random grey that moves 2 pixels a frame (or stands still), noise of sigma 1, and
    on the frames STRAP_FRAMES a dark strap with bright bars, 2 pixels on and 2 off"""
    rng = np.random.default_rng(seed)
    h, w = CLIP_H, CLIP_W
    wide = np.kron(rng.integers(30, 226, (h // 6 + 1, (w + 2 * CLIP_N) // 6 + 2)), np.ones((6, 6), np.int64)).astype(np.float64)
    l, t, r, b = STRAP
    bars = np.where((np.arange(r - l) >> 1) & 1, 230.0, 25.0)[None, :] * np.ones((b - t, 1))
    frames = []
    for i in range(CLIP_N):
        x = 2 * i if moving else 0
        f = wide[:h, x:x + w].copy()
        if strap and STRAP_FRAMES[0] <= i <= STRAP_FRAMES[1]:
            f[t:b, l:r] = bars
        frames.append(grey(np.clip(np.rint(f + rng.normal(0.0, 1.0, f.shape)), 0, 255)))
    return frames
