"""The host side of the `faces` verb (FACES.md): which faces of a track, cluster or name are its best, and where they go on the
contact sheet.  The pixels -- the quality sums of a chip, the resampled tiles, the drawing -- are the library's (csrc/faces.hip);
what is here is a handful of integers and floats per face."""
import math

import numpy as np

from . import render

CHIP = 150
CHIP_PIXELS = CHIP * CHIP                  # 22 500: what ND and NB count over
INTERIOR = (CHIP - 2) * (CHIP - 2)         # N = 21 904: the pixels that have a Laplacian
MIN_TILE, MAX_TILE = 48, 600               # PVF_SHEET_MIN_TILE / _MAX_TILE
MAX_SIDE, MAX_PIXELS, MAX_TILES = 16384, 1 << 26, 65536
GAP = 6                                    # between tiles, and around a panel: two outlines of 2 pixels and 2 of background
BACKGROUND = (24, 24, 24)


def symmetry(pts):
    """frontalness from the 68 integer points: sqrt(min / max) of the squared distances of the nose tip (30) to the jaw at the height of
    the nose (2 and 14); 1.0 for a frontal face, towards 0 in profile, 0.0 when both distances are 0"""
    p = np.asarray(pts).reshape(68, 2)
    dl = (int(p[30][0]) - int(p[2][0])) ** 2 + (int(p[30][1]) - int(p[2][1])) ** 2
    dr = (int(p[30][0]) - int(p[14][0])) ** 2 + (int(p[30][1]) - int(p[14][1])) ** 2
    lo, hi = min(dl, dr), max(dl, dr)
    return 0.0 if hi == 0 else math.sqrt(float(lo) / float(hi))


def sharpness(q):
    """V = N S2 - S1^2 of a chip's sums (S1, S2, SY, ND, NB): N^2 times the variance of its Laplacian, an integer >= 0"""
    return INTERIOR * int(q[1]) - int(q[0]) ** 2


def score(q, sym):
    return float(sharpness(q)) / float(INTERIOR * INTERIOR) * sym


def eligible(q, box_height, frame_height, max_dark=0.25, max_bright=0.25, min_size=0.0):
    """not mostly black (a chip is black where it leaves the frame), not blown out, not too small"""
    return bool(int(q[3]) <= max_dark * CHIP_PIXELS and int(q[4]) <= max_bright * CHIP_PIXELS and box_height >= min_size * frame_height)


def choose(faces, K, spread=1.0):
    """indices of the (at most) K faces shown for a group.  faces: [(score, t, track, eligible)].  Rank: eligible first, then score
    descending, time ascending, track ascending.  The ranked list is walked greedily; a face is passed over when a chosen face of its
    track lies within `spread` seconds; what is missing after that comes from the passed-over faces, in rank order."""
    rank = sorted(range(len(faces)), key=lambda i: (not faces[i][3], -faces[i][0], faces[i][1], faces[i][2]))
    chosen, passed = [], []
    for i in rank:
        if len(chosen) >= K:
            break
        _, t, track, _ = faces[i]
        if any(faces[j][2] == track and abs(faces[j][1] - t) <= spread for j in chosen):
            passed.append(i)
        else:
            chosen.append(i)
    return chosen + passed[:max(K - len(chosen), 0)]


def text_scale(S):
    return max(1, int(S) // 48)


def panel_size(K, S):
    """(width, height) of a panel: a label line over a row of K tiles"""
    return GAP + K * (S + GAP), 3 * GAP + 7 * text_scale(S) + S


def default_columns(n_groups):
    return 1 if n_groups <= 24 else -(-n_groups // 24)


def layout(groups, K, S, columns):
    """groups: [(label, colour index, number of faces shown)], in sheet order.  -> (W, H, [[(x, y)] per group], primitives): panel p sits
    at column p % columns, row p // columns of a grid of panel_size cells; its label's glyph boxes start GAP in and GAP down, its tile k
    at (x + GAP + k (S + GAP), y + 2 GAP + 7 scale), each with an outline two pixels wide around it, not on it.  A group with fewer
    than K faces leaves background."""
    K, S, columns = int(K), int(S), int(columns)
    if K < 1 or columns < 1 or not groups:
        raise ValueError("a sheet has at least one group, one face a group and one column")
    s = text_scale(S)
    pw, ph = panel_size(K, S)
    rows = -(-len(groups) // columns)
    corners, prims = [], []
    for p, (label, colour, shown) in enumerate(groups):
        x, y = (p % columns) * pw, (p // columns) * ph
        rgb = render.PALETTE[colour % len(render.PALETTE)]
        text = (label if isinstance(label, bytes) else str(label).encode("utf-8"))[:min(render.MAX_TEXT_RUN, (pw - 2 * GAP) // (6 * s))]
        prims.append((render.PRIM_TEXT, x + GAP, y + GAP + 7 * s - 1, rgb, s, text))
        mine = []
        for k in range(min(int(shown), K)):
            tx, ty = x + GAP + k * (S + GAP), y + 2 * GAP + 7 * s
            mine.append((tx, ty))
            prims.append((render.PRIM_RECT, tx - 1, ty - 1, tx + S, ty + S, rgb))
        corners.append(mine)
    return min(columns, len(groups)) * pw, rows * ph, corners, prims


def check_sheet(W, H, n_tiles, n_prims):
    """the library's caps, refused here with the options that shrink a sheet"""
    if W > MAX_SIDE or H > MAX_SIDE or W * H > MAX_PIXELS or n_tiles > MAX_TILES or n_prims > render.MAX_PRIMS:
        raise ValueError("a sheet of %d x %d pixels with %d faces and %d labels and outlines is beyond what one picture holds (sides up to %d, "
                         "%d pixels, %d drawn items): choose a smaller --tile, fewer faces with --per, fewer groups with --only, or more "
                         "--columns" % (W, H, n_tiles, n_prims, MAX_SIDE, MAX_PIXELS, render.MAX_PRIMS))


def ppm_bytes(rgb):
    """a binary PPM (P6): `P6\\n<width> <height>\\n255\\n`, then the bytes row by row"""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("a picture is uint8 [height, width, 3]")
    return b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]) + rgb.tobytes()


def quality_line(T, track, q, sym, sc, ok):
    return "%.3f %d %d %d %d %d %d %.5f %.5f %d\n" % (T, track, int(q[0]), int(q[1]), int(q[2]), int(q[3]), int(q[4]), sym, sc, 1 if ok else 0)


def landmark_faces(track_rows, landmark_rows, frame_times, width, height):
    """every row of a landmark file as a face: [(T, track, frame index, box, int32 [68, 2] points)] in the file's order.  Rows are paired
    with frames by getFaceGenerator's rules (pipeline.faces_per_frame, as `extract` paired them when it wrote the file); points are
    np.round(x * width) on float32 (render.landmark_groups), and every row is used: the last group, which the reference's landmark
    generator never emits, is a face like any other here."""
    from .pipeline import faces_per_frame
    where = {}
    for fi, T, g in faces_per_frame(track_rows, frame_times, width, height):
        for ident, box in g:
            where[(int(round(T * 1000.0)), int(ident))] = (fi, box)
    out = []
    for T, ident, pts in landmark_rows:
        if len(pts) != 68:
            raise ValueError("landmarks: 68 points a face expected, found %d" % len(pts))
        key = (int(round(T * 1000.0)), int(ident))
        if key not in where:
            raise KeyError("landmarks: no face of track %d at %.3f in the tracking file" % (ident, T))
        p = np.array(pts, np.float32)
        p[:, 0] = np.round(p[:, 0] * width)
        p[:, 1] = np.round(p[:, 1] * height)
        out.append((T, int(ident), where[key][0], where[key][1], p.astype(np.int32)))
    return out


def group_faces(faces, labels=None, only=None, t_from=0.0, t_until=None):
    """[(name, colour index, [face index])] in sheet order: a group per track (`#id`), or per name with labels ({track: name}; a track
    without one stays a group of its own).  Groups come in the order of their smallest track number, which is also their colour index (a
    track's colour is `demo`'s).  only: names to keep (`#7` or `7` for a track); faces outside [t_from, t_until) take no part."""
    by_name = {}
    for i, (T, track) in enumerate((f[0], f[1]) for f in faces):
        if T < t_from or (t_until is not None and not T < t_until):
            continue
        name = (labels or {}).get(track) or "#%d" % track
        by_name.setdefault(name, [track, []])
        by_name[name][0] = min(by_name[name][0], track)
        by_name[name][1].append(i)
    groups = sorted(((name, first, idx) for name, (first, idx) in by_name.items()), key=lambda g: (g[1], g[0]))
    if only is not None:
        groups = [g for g in groups if g[0] in only or g[0].lstrip("#") in only]
    return groups
