"""FACES.md restated in numpy, independent of the package: the five quality sums of a face chip, frontalness, score, eligibility and the
choice of a group's faces, a chip resampled to a tile, the sheet of tiles and primitives, the layout of the panels and the bytes of a
PPM.  Primitives are drawn by demo_ref.  Everything on the pixel side is integer arithmetic, so the GPU is held to it bit for bit.
The keyword switches of `quality`, `tile` and `sheet` plant the defects test_faces_ref.py shows the comparison can see."""
import math

import numpy as np

from tests import demo_ref

N = 148 * 148
PIXELS = 150 * 150
GAP = 6
BACKGROUND = (24, 24, 24)


def luma(chip, rounding=True):
    c = np.asarray(chip).astype(np.int64).reshape(150, 150, 3)
    return (77 * c[:, :, 0] + 150 * c[:, :, 1] + 29 * c[:, :, 2] + (128 if rounding else 0)) >> 8


def quality(chip, border=False, bits32=False, rounding=True, dark_strict=False):
    """(S1, S2, SY, ND, NB) as Python ints.  Defects: border -- the Laplacian over all 150 x 150 pixels, the plane continued by its edge
    values; bits32 -- S2 kept to 32 bits; rounding off -- Y without the + 128; dark_strict -- ND counts Y < 16"""
    Y = luma(chip, rounding)
    if border:
        P = np.pad(Y, 1, mode="edge")
        L = 4 * P[1:-1, 1:-1] - P[:-2, 1:-1] - P[2:, 1:-1] - P[1:-1, :-2] - P[1:-1, 2:]
    else:
        L = 4 * Y[1:-1, 1:-1] - Y[:-2, 1:-1] - Y[2:, 1:-1] - Y[1:-1, :-2] - Y[1:-1, 2:]
    S2 = int((L * L).sum())
    if bits32:
        S2 &= 0xFFFFFFFF
    return int(L.sum()), S2, int(Y.sum()), int((Y < 16).sum() if dark_strict else (Y <= 16).sum()), int((Y >= 239).sum())


def qualities(chips, **kw):
    return np.array([quality(c, **kw) for c in chips], np.int64).reshape(-1, 5)


def sharpness(q):
    return N * int(q[1]) - int(q[0]) ** 2


def symmetry(pts):
    p = [(int(x), int(y)) for x, y in np.asarray(pts).reshape(68, 2)]
    dl = (p[30][0] - p[2][0]) ** 2 + (p[30][1] - p[2][1]) ** 2
    dr = (p[30][0] - p[14][0]) ** 2 + (p[30][1] - p[14][1]) ** 2
    return 0.0 if max(dl, dr) == 0 else math.sqrt(min(dl, dr) / max(dl, dr))


def score(q, sym):
    return float(sharpness(q)) / float(N * N) * sym


def eligible(q, box_height, frame_height, max_dark=0.25, max_bright=0.25, min_size=0.0):
    return int(q[3]) <= max_dark * PIXELS and int(q[4]) <= max_bright * PIXELS and box_height >= min_size * frame_height


def choose(faces, K, spread=1.0):
    """faces: [(score, t, track, eligible)] -> indices shown, in order"""
    order = sorted(range(len(faces)), key=lambda i: (0 if faces[i][3] else 1, -faces[i][0], faces[i][1], faces[i][2]))
    taken, skipped = [], []
    for i in order:
        if len(taken) == K:
            break
        near = [j for j in taken if faces[j][2] == faces[i][2] and abs(faces[j][1] - faces[i][1]) <= spread]
        (skipped if near else taken).append(i)
    while len(taken) < K and skipped:
        taken.append(skipped.pop(0))
    return taken


def _axis(S, clamp=True):
    u = (2 * np.arange(S, dtype=np.int64) + 1) * 150 - S
    if clamp:
        u = np.clip(u, 0, 149 * 2 * S)
    i0 = np.sign(u) * (np.abs(u) // (2 * S))          # C's division; the same as // where u >= 0, which the clamp guarantees
    f = u - i0 * 2 * S
    return i0, np.minimum(i0 + 1, 149), f


def tile(chip, S, clamp=True):
    """uint8 [S, S, 3].  Defect: clamp off -- u is not clamped: below 0 for S > 150, where C's division and remainder give index 0 and a
    negative weight (above, 299 S - 150 < 300 S keeps the index at 149 with or without the clamp)"""
    c = np.asarray(chip).astype(np.int64).reshape(150, 150, 3)
    x0, x1, fx = _axis(S, clamp)
    y0, y1, fy = x0[:, None], x1[:, None], fx[:, None]
    x0, x1, fx = x0[None, :], x1[None, :], fx[None, :]
    D = 2 * S
    out = np.empty((S, S, 3), np.int64)
    for k in range(3):
        p = c[:, :, k]
        out[:, :, k] = ((D - fx) * (D - fy) * p[y0, x0] + fx * (D - fy) * p[y0, x1] + (D - fx) * fy * p[y1, x0] + fx * fy * p[y1, x1] +
                        2 * S * S) // (4 * S * S)
    return out.astype(np.uint8)


def sheet(chips, xy, S, W, H, background=(0, 0, 0), prims=(), first_wins=False):
    """uint8 [H, W, 3].  Defect: first_wins -- an earlier tile lies over a later one"""
    img = np.empty((H, W, 3), np.uint8)
    img[:, :] = background
    order = list(range(len(chips)))
    for i in (reversed(order) if first_wins else order):
        x, y = int(xy[i][0]), int(xy[i][1])
        xa, xb, ya, yb = max(x, 0), min(x + S, W), max(y, 0), min(y + S, H)
        if xa >= xb or ya >= yb:
            continue
        img[ya:yb, xa:xb] = tile(chips[i], S)[ya - y:yb - y, xa - x:xb - x]
    return demo_ref.draw(img, list(prims))


def layout(groups, K, S, columns):
    """groups: [(label, colour index, shown)] -> (W, H, [[(x, y)]], prims in demo_ref's form)"""
    s = max(1, S // 48)
    pw, ph = GAP + K * (S + GAP), 3 * GAP + 7 * s + S
    corners, prims = [], []
    for p, (label, colour, shown) in enumerate(groups):
        x, y = (p % columns) * pw, (p // columns) * ph
        rgb = tuple(demo_ref.PALETTE[colour % len(demo_ref.PALETTE)])
        data = str(label).encode("utf-8")[:min(demo_ref.MAX_RUN, (pw - 2 * GAP) // (6 * s))]
        prims.append((demo_ref.TEXT, x + GAP, y + GAP + 7 * s - 1, rgb, s, data))
        mine = []
        for k in range(min(shown, K)):
            tx, ty = x + GAP + k * (S + GAP), y + 2 * GAP + 7 * s
            mine.append((tx, ty))
            prims.append((demo_ref.RECT, tx - 1, ty - 1, tx + S, ty + S, rgb))
        corners.append(mine)
    rows = -(-len(groups) // columns)
    return min(columns, len(groups)) * pw, rows * ph, corners, prims


def ppm(img):
    h, w = img.shape[:2]
    return ("P6\n%d %d\n255\n" % (w, h)).encode("ascii") + np.ascontiguousarray(img, np.uint8).tobytes()


# ---- contents the tests share -----------------------------------------------------------------------------------------------------
def grey(Y):
    """a chip whose luma plane is Y (uint8 [150, 150]): R = G = B = Y gives (256 Y + 128) >> 8 = Y"""
    return np.repeat(np.asarray(Y, np.uint8)[:, :, None], 3, axis=2)


def named_chips():
    """{name: chip}: the contents ISSUE and FACES.md name, with what they are known to give in test_faces_ref.py"""
    r, c = np.mgrid[0:150, 0:150]
    rng = np.random.default_rng(20261019)
    out = {
        "black": grey(np.zeros((150, 150))),
        "white": grey(np.full((150, 150), 255)),
        "ramp": grey(np.tile(np.arange(150) * 255 // 149, (150, 1))),        # 0 .. 255 over a row: steps of 1 and 2
        "checker": grey(255 * ((r + c) & 1)),
        "dot": grey(np.where((r == 0) & (c == 5), 255, 0)),
        "noise": rng.integers(0, 256, (150, 150, 3)).astype(np.uint8),
        "stripes_v": grey(255 * (c & 1)),
        "stripes_h": grey(255 * (r & 1)),
        "frame": grey(np.where((r == 0) | (r == 149) | (c == 0) | (c == 149), 255, 0)),
    }
    # colour edges of equal luma: (200, 0, 0) and (0, 103, 0) both give Y = 60; the Laplacian must not see the edge
    edge = np.zeros((150, 150, 3), np.uint8)
    edge[:, :75] = (200, 0, 0)
    edge[:, 75:] = (0, 103, 0)
    out["equal_luma_edge"] = edge
    for y in (16, 17, 238, 239):
        out["y%d" % y] = grey(np.full((150, 150), y))
    # a luma exactly at and one beside each rounding step: 77 R + 150 G + 29 B + 128 = 256 k and 256 k - 1
    out["round_at"] = np.tile(np.array([0, 0, 128 // 29 + 1], np.uint8), (150, 150, 1))        # 29 * 5 + 128 = 273 -> 1
    out["round_below"] = np.tile(np.array([0, 0, 4], np.uint8), (150, 150, 1))                   # 29 * 4 + 128 = 244 -> 0
    return out
