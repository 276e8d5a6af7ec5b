"""The case table of the `clothes` kernel, shared by tests/test_clothes_ref.py (which proves on the CPU what it reaches) and
tests/test_gpu_clothes.py (which runs it): frame sizes, windows, contents and groupings -- the smallest shapes at which box_hist_k
(csrc/clothes.hip) can go wrong.  A piece of the kernel is at most PIECE_ROWS x PIECE_COLS pixels."""
import numpy as np

from tests import clothes_ref as cr

PIECE_COLS, PIECE_ROWS = 256, 16
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
SIZES = (1, 15, 16, 17, 255, 256, 257)   # widths and heights of windows: the piece sizes and their neighbours are among them
BANDS = (1, 2, 3, 4)

# row byte lengths 3 w in every class mod 16 (w = 1, 2, 5, 21, 67, 85 and 256, 257 give 3, 6, 15, 15, 9, 15, 0, 3 ...) and mod 4
GEOMETRIES = [(w, h) for w in (1, 2, 5, 21, 67, 85, 256, 257) for h in (1, 2, 3, 17)]
LARGE = ((1920, 1080), (3840, 2160))
CONTENTS = ("black", "white", "mid", "halves", "noise", "every", "seams")
MID, LEFT, RIGHT = (90, 140, 200), (200, 40, 40), (30, 60, 220)

# colours on every class boundary: Y at 63 / 64, 127 / 128, 191 / 192 (greys), c1 and c2 at -65, -64, -49, -48, 47, 48, 63, 64, and
# odd negative 2 B - R - G, where the floor and the truncation differ
EDGES = (-65, -64, -49, -48, 47, 48, 63, 64)
SEAMS = ([(v, v, v) for v in (63, 64, 127, 128, 191, 192)] + [(128 + k, 128, 128 + (k >> 1)) for k in EDGES] + [(100, 100, 100 + k) for k in EDGES]
         + [(101, 100, 50), (1, 0, 0), (200, 201, 100), (255, 254, 0)])


def frame_of(content, w, h):
    """uint8 [h][w][3]"""
    if content in ("black", "white", "mid"):
        f = np.zeros((h, w, 3), np.uint8)
        f[:] = {"black": (0, 0, 0), "white": (255, 255, 255), "mid": MID}[content]
        return f
    if content == "halves":
        f = np.zeros((h, w, 3), np.uint8)
        f[:, :w // 2], f[:, w // 2:] = LEFT, RIGHT
        return f
    if content == "noise":
        return np.random.default_rng(1000 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    palette = cr.every_colour()[1] if content == "every" else np.array(SEAMS, np.uint8)
    return palette[np.arange(w * h) % len(palette)].reshape(h, w, 3)


def windows_for(w, h):
    """int32 [n][4]: windows inside, across every edge and corner, containing the frame, outside on every side, empty, inverted, of one
    pixel, at the int32 extremes, of the sizes SIZES, of heights around the band counts, and clipped at the top"""
    a, b = w // 2, h // 2
    wins = [(w // 4, h // 4, w // 4 + max(1, a), h // 4 + max(1, b)),                                       # inside
            (-3, h // 3, a + 1, h // 3 + max(1, b)), (a, h // 3, w + 4, h // 3 + max(1, b)),                # across the left and right edge
            (w // 3, -2, w // 3 + max(1, a), b + 1), (w // 3, b, w // 3 + max(1, a), h + 5),                # the top and the bottom edge
            (-2, -2, a + 1, b + 1), (a, -2, w + 3, b + 1), (-2, b, a + 1, h + 3), (a, b, w + 3, h + 3),     # the corners
            (-5, -7, w + 3, h + 9), (0, 0, w, h),                                                           # containing the frame; the frame
            (-10, 0, 0, h), (w, 0, w + 5, h), (0, -4, w, 0), (0, h, w, h + 3), (-10, -10, -1, -1),          # outside on each side
            (1, 1, 1, 5), (0, 0, w, 0), (3, 0, 1, h), (0, 5, w, 2),                                         # empty and inverted
            (0, 0, 1, 1), (w - 1, h - 1, w, h),                                                             # one pixel
            (I32_MIN, 0, w, h), (0, I32_MIN, w, h), (0, 0, I32_MAX, h), (0, 0, w, I32_MAX), (I32_MIN, I32_MIN, I32_MAX, I32_MAX),
            (I32_MAX, I32_MAX, I32_MIN, I32_MIN), (I32_MIN, I32_MIN, I32_MIN + 5, I32_MAX), (I32_MAX - 1, 0, I32_MAX, h), (a, I32_MIN, a + 1, I32_MIN + 9),
            (0, -5, w, 4), (0, -9, w, 9), (a, -40, w, 3)]                                                   # clipped at the top
    wins += [(x, 0, x + s, h) for s in SIZES for x in (0, 1)]                                               # widths
    wins += [(0, y, w, y + s) for s in SIZES for y in (0, 1)]                                               # heights (those above the frame's are clipped)
    wins += [(0, 0, w, k) for k in (2, 3, 4, 5)] + [(0, h - 2, w, h + 1)]                                   # heights below, at and above the band counts
    return np.array(wins, np.int64).astype(np.int32)


def large_windows(w, h):
    """windows of a full-size frame: a torso, the frame and more, the corners, a row of the whole width, and SIZES squared at odd offsets"""
    wins = [(600, 300, 1200, 900), (-1, -1, w + 1, h + 1), (-100, -100, 300, 300), (w - 301, h - 299, w + 50, h + 50), (0, 500, w, 501), (777, 0, 778, h),
            (I32_MIN, 1000, I32_MAX, 1003)]
    wins += [(101 + 3 * i, 51 + 5 * j, 101 + 3 * i + s, 51 + 5 * j + t) for i, s in enumerate(SIZES) for j, t in enumerate(SIZES)]
    return np.array(wins, np.int64).astype(np.int32)


def groupings(n):
    """[(name, int32 [n] groups, G)]"""
    i = np.arange(n, dtype=np.int32)
    return [("identity", i, n), ("one", np.zeros(n, np.int32), 1), ("interleaved", i % 3, 3), ("holes", 2 * i + 1, 2 * n + 2),
            ("reversed", n - 1 - i, n)]


# ---- the planted clip of `clothes` and `link`: two people in coloured clothes, each track cut in two, and a third in grey ----------------
CLIP_W, CLIP_H, CLIP_FPS, CLIP_FRAMES = 192, 144, 25.0, 40
PEOPLE = {"red": ((200, 40, 40), (60, 40, 150)), "green": ((40, 160, 60), (230, 200, 40)), "grey": ((120, 120, 120), (90, 90, 90))}
# track: (person, first frame, last frame, the face box (l, t, r, b))
CLIP_TRACKS = {0: ("red", 0, 14, (20, 10, 44, 34)), 1: ("green", 0, 14, (120, 12, 144, 36)), 2: ("red", 20, 39, (100, 14, 124, 38)),
               3: ("green", 20, 39, (30, 8, 54, 32)), 4: ("grey", 16, 18, (80, 10, 104, 34))}
CLIP_LINKS = [(0, 2), (1, 3)]


def planted_clip():
    """(frames uint8 [n][h][w][3], tracking lines [(T, track, box normalised float32, status)]): under every face a shirt of the person's
    upper colour over trousers of the lower one, on a noisy background, shifting a pixel now and then"""
    rng = np.random.default_rng(7)
    frames = rng.integers(100, 140, (CLIP_FRAMES, CLIP_H, CLIP_W, 3)).astype(np.uint8)
    lines = []
    for track, (person, first, last, (l, t, r, b)) in sorted(CLIP_TRACKS.items()):
        upper, lower = PEOPLE[person]
        for fi in range(first, last + 1):
            dx = (fi // 5) % 2
            frames[fi, t:b, l + dx:r + dx] = (220, 180, 150)
            frames[fi, b:b + 40, l + dx - 14:r + dx + 14] = np.clip(np.array(upper) + rng.integers(-6, 7, (40, r - l + 28, 3)), 0, 255)
            frames[fi, b + 40:b + 80, l + dx - 14:r + dx + 14] = np.clip(np.array(lower) + rng.integers(-6, 7, (40, r - l + 28, 3)), 0, 255)
            box = tuple(np.float32("%.3f" % v) for v in ((l + dx) / CLIP_W, t / CLIP_H, (r + dx) / CLIP_W, b / CLIP_H))
            lines.append((fi / CLIP_FPS, track, box, "detection"))
    lines.sort(key=lambda r: r[0])
    return frames, lines
