"""TUBE.md "Oriented window" restated in numpy: an oriented window (CX, CY, BX, BY, K) of a frame as an S x S picture, by a plain loop over
the K x K sub-samples in int64, its YUV 4:2:0 form, which of the kernel's two load paths a tile takes, the host rules of `tube --align`
and the table of named cases the GPU tests run.  The kernel (warp_k in csrc/tube.hip) is compared with `warp` / `warps` bit for bit;
tube.py with the host rules.  The keyword arguments plant the defects that test_warp_ref.py shows the comparison to see; none is used
anywhere else."""
import math

import numpy as np

from tests import tube_ref as tr

MAX_K, MAX_STEP = 16, 1 << 20            # PVF_WARP_MAX_K, PVF_WARP_MAX_STEP
MAX_COORD, MAX_SIZE, MAX_CROPS = tr.MAX_COORD, tr.MAX_SIZE, tr.MAX_CROPS
# the seams of warp_k: output pixels of a tile along each axis, LDS bytes of a staged box
W_SIDE, W_TILE = 16, 24576
ONE = 65536                              # a step of one source pixel


# ---- window -> picture ----------------------------------------------------------------------------------------------------------------
def quotient(v, d):
    """v // d the way the kernel takes it: v < 2^16, d <= 256, M = 2^24 // d + 1"""
    return (int(v) * ((1 << 24) // int(d) + 1)) >> 24


def positions(window, S, a, b, perp_sign=False, no_half=False, k_off=False):
    """PX [S][S], PY [S][S] of sub-sample (a, b) of every output pixel, int64, in 1 / 131072 pixel"""
    CX, CY, BX, BY, K = (int(v) for v in window)
    j = np.arange(S, dtype=np.int64)
    m = (2 * (j * (K + 1 if k_off else K) + a) + 1 - S * K)[None, :]
    n = (2 * (j * K + b) + 1 - S * K)[:, None]
    half = 0 if no_half else 65536
    if perp_sign:
        return 8192 * CX + m * BX + n * BY - half, 8192 * CY + m * BY - n * BX - half
    return 8192 * CX + m * BX - n * BY - half, 8192 * CY + m * BY + n * BX - half


def warp(frame, window, S, perp_sign=False, no_half=False, truncate=False, clamp=False, round_fx=False, rounding=True, k_off=False,
         swap_channels=False):
    """uint8 [S][S][3]: the oriented window of uint8 [h][w][3]"""
    frame = np.asarray(frame)
    h, w = frame.shape[:2]
    K, S = int(window[4]), int(S)
    f = frame.astype(np.int64)
    if swap_channels:
        f = f[:, :, [1, 0, 2]]
    total = np.zeros((S, S, 3), np.int64)

    def taps(x, y):
        if clamp:
            return f[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return f[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)] * inside[:, :, None]

    for b in range(K):
        for a in range(K):
            PX, PY = positions(window, S, a, b, perp_sign, no_half, k_off)
            if truncate:
                x0, y0 = np.sign(PX) * (np.abs(PX) >> 17), np.sign(PY) * (np.abs(PY) >> 17)
            else:
                x0, y0 = PX >> 17, PY >> 17
            if round_fx:
                fx, fy = np.minimum(((PX & 131071) + 256) >> 9, 255), np.minimum(((PY & 131071) + 256) >> 9, 255)
            else:
                fx, fy = (PX & 131071) >> 9, (PY & 131071) >> 9
            fx, fy = fx[:, :, None], fy[:, :, None]
            total += (256 - fx) * (256 - fy) * taps(x0, y0) + fx * (256 - fy) * taps(x0 + 1, y0) + (256 - fx) * fy * taps(x0, y0 + 1) + \
                fx * fy * taps(x0 + 1, y0 + 1)
    den = 65536 * K * K
    assert total.max() + den // 2 < 2 ** 32
    out = (total + (den // 2 if rounding else 0)) // den
    return out.astype(np.uint8)


def warps(frames, windows, S, layout="rgb", matrix="601", full_range=False, **defects):
    """what Context.frame_warps returns"""
    out = []
    for f, win in zip(frames, windows):
        rgb = warp(f, win, S, **defects)
        out.append(rgb if layout == "rgb" else tr.to_yuv(rgb, matrix, full_range))
    if not out:
        return np.zeros((0, S, S, 3) if layout == "rgb" else (0, S * S + 2 * ((S + 1) // 2) ** 2), np.uint8)
    return np.stack(out)


def tile_paths(h, w, window, S):
    """which way each tile of warp_k gets its source pixels: "lds" (the box of the tile's taps, clipped to the frame, is staged),
    "direct" (the box is larger than W_TILE bytes) or "empty" (no tap inside the frame), in tile order.  The box is restated from the
    first and last sub-samples of every pixel of the tile, not from the tile's four corners alone."""
    K = int(window[4])
    grids = [positions(window, S, a, b) for b in (0, K - 1) for a in (0, K - 1)]
    out = []
    for i0 in range(0, S, W_SIDE):
        for j0 in range(0, S, W_SIDE):
            xs = np.concatenate([g[0][i0:i0 + W_SIDE, j0:j0 + W_SIDE].reshape(-1) for g in grids]) >> 17
            ys = np.concatenate([g[1][i0:i0 + W_SIDE, j0:j0 + W_SIDE].reshape(-1) for g in grids]) >> 17
            bx0, bx1, by0, by1 = max(int(xs.min()), 0), min(int(xs.max()) + 1, w - 1), max(int(ys.min()), 0), min(int(ys.max()) + 1, h - 1)
            if bx0 > bx1 or by0 > by1:
                out.append("empty")
            else:
                pitch = (3 + 3 * (bx1 - bx0 + 1) + 15) & ~15
                out.append("lds" if (by1 - by0 + 1) * pitch <= W_TILE else "direct")
    return out


def identity(x, y, S):
    """the axis-aligned window whose picture is frame[y:y + S, x:x + S]: its centre lies 8 S sixteenths right of and below pixel (x, y)'s corner"""
    return (16 * x + 8 * S, 16 * y + 8 * S, ONE, 0, 1)


def direction(degrees, step=ONE):
    r = math.radians(degrees)
    return int(math.floor(step * math.cos(r) + 0.5)), int(math.floor(step * math.sin(r) + 0.5))


def window_cases(h, w, S):
    """{name: (CX, CY, BX, BY, K)}: the named windows of the issue on an h x w frame at picture size S"""
    cx, cy = 8 * w, 8 * h                                          # the frame's centre
    zoom = min(max(ONE * min(h, w) // (2 * S), 1), MAX_STEP)       # half the frame's smaller side across the picture
    c = {
        "east": (cx + 3, cy + 5, zoom, 0, 1), "south": (cx, cy, 0, zoom, 1), "west": (cx - 7, cy, -zoom, 0, 1), "north": (cx, cy + 9, 0, -zoom, 1),
        "east_off": (cx, cy, zoom, 1, 1), "east_off2": (cx, cy, zoom, -1, 2), "south_off": (cx, cy, 1, zoom, 1), "south_off2": (cx, cy, -1, zoom, 3),
        "west_off": (cx, cy, -zoom, 1, 2), "west_off2": (cx, cy, -zoom, -1, 1), "north_off": (cx, cy, 1, -zoom, 1), "north_off2": (cx, cy, -1, -zoom, 2),
        "diagonal": (cx, cy, zoom, zoom, 1), "diagonal_k2": (cx + 1, cy - 1, zoom // 2 + 1, zoom // 2 + 1, 2),
        "any_1": (cx + 11, cy - 4) + direction(17.0, zoom) + (1,), "any_2": (cx - 5, cy + 2) + direction(-63.0, zoom // 2 + 1) + (2,),
        "any_3": (cx, cy) + direction(141.0, zoom // 3 + 1) + (3,), "any_16": (cx, cy) + direction(-108.0, zoom // 16 + 1) + (16,),
        "k16_east": (cx, cy, zoom // 16 + 1, 0, 16), "k3_south": (cx, cy, 0, zoom // 3 + 1, 3),
        "still": (cx + 5, cy + 3, 0, 0, 1), "still_k16": (16 * 3 + 1, 16 * 2 + 15, 0, 0, 16),
        "enlarge": (cx, cy) + direction(30.0, ONE // 5) + (1,),
        "cross_left": (0, cy) + direction(10.0, zoom) + (1,), "cross_right": (16 * w, cy) + direction(-20.0, zoom) + (2,),
        "cross_top": (cx, 0) + direction(100.0, zoom) + (1,), "cross_bottom": (cx, 16 * h) + direction(200.0, zoom) + (3,),
        "corner_tl": (3, -5) + direction(45.0, zoom) + (1,), "corner_tr": (16 * w - 1, 7) + direction(-45.0, zoom) + (2,),
        "corner_bl": (-9, 16 * h + 2) + direction(135.0, zoom) + (1,), "corner_br": (16 * w + 4, 16 * h - 3) + direction(15.0, zoom) + (1,),
        "dwarf": (cx, cy) + direction(33.0, min(4 * ONE * max(h, w) // S + 1, MAX_STEP)) + (1,),
        "outside_left": (-16 * 40 * S - 16 * w, cy, ONE, 0, 1), "outside_right": (16 * 40 * S + 32 * w, cy, 0, ONE, 2),
        "outside_top": (cx, -16 * 40 * S - 16 * h) + direction(45.0, ONE) + (1,), "outside_bottom": (cx, 16 * 40 * S + 32 * h) + direction(-30.0, ONE) + (3,),
        "cap_far": (MAX_COORD, -MAX_COORD, MAX_STEP, -MAX_STEP, 16), "cap_far2": (-MAX_COORD, MAX_COORD, -MAX_STEP, MAX_STEP, 1),
        "cap_far3": (MAX_COORD, MAX_COORD, 0, 0, 16), "cap_step": (cx, cy, MAX_STEP, MAX_STEP, 16), "cap_step2": (cx, cy, -MAX_STEP, 0, 1),
    }
    return c


BLACK = ("outside_left", "outside_right", "outside_top", "outside_bottom", "cap_far", "cap_far2", "cap_far3")


# ---- host rules ------------------------------------------------------------------------------------------------------------------------
def unit(dx, dy):
    length = math.hypot(dx, dy)
    return (dx / length, dy / length) if length > 0.0 else (1.0, 0.0)


def eye_direction(pts):
    if pts is None:
        return 1.0, 0.0
    p = np.asarray(pts).reshape(68, 2)
    e0 = [sum(int(v) for v in p[36:42, k]) / 6.0 for k in (0, 1)]
    e1 = [sum(int(v) for v in p[42:48, k]) / 6.0 for k in (0, 1)]
    return unit(e1[0] - e0[0], e1[1] - e0[1])


def quantise_oriented(cx, cy, side, c, s, S):
    CX = min(max(int(math.floor(16.0 * float(cx) + 0.5)), -MAX_COORD), MAX_COORD)
    CY = min(max(int(math.floor(16.0 * float(cy) + 0.5)), -MAX_COORD), MAX_COORD)
    lim = float(2 * MAX_K * MAX_STEP)
    ax = min(max(float(side) / float(S) * 65536.0 * float(c), -lim), lim)
    ay = min(max(float(side) / float(S) * 65536.0 * float(s), -lim), lim)
    AX, AY = int(math.floor(ax + 0.5)), int(math.floor(ay + 0.5))
    K = ([k for k in range(1, MAX_K) if (65536 * k) ** 2 >= AX * AX + AY * AY] + [MAX_K])[0]
    BX = min(max(int(math.floor(ax / K + 0.5)), -MAX_STEP), MAX_STEP)
    BY = min(max(int(math.floor(ay / K + 0.5)), -MAX_STEP), MAX_STEP)
    return CX, CY, BX, BY, K


def plan(faces, size, region="face", scale=None, smooth_window=0.5, labels=None, only=None, segments=None, min_length=0.0, t_from=0.0,
         t_until=None, ext="npy"):
    """tube_ref.plan with oriented windows: [(file name, track, [(face index, T, (CX, CY, BX, BY, K))])]"""
    scale = (1.6 if region == "face" else 0.5) if scale is None else scale
    tracks = {}
    for i, f in enumerate(faces):
        tracks.setdefault(int(f[1]), []).append(i)
    out = []
    for track in sorted(tracks):
        name = (labels or {}).get(track) or "#%d" % track
        if only is not None and not (name in only or name.lstrip("#") in only):
            continue
        idx = sorted(tracks[track], key=lambda i: (tr.ms(faces[i][0]), i))
        raw = [tr.face_region(faces[i][3], scale) if region == "face" else tr.mouth_region(faces[i][3], faces[i][4], scale) for i in idx]
        times = [faces[i][0] for i in idx]
        sm = [tr.smooth(times, [r[k] for r in raw], smooth_window) for k in range(3)]
        dirs = [eye_direction(faces[i][4]) for i in idx]
        if tr.ms(smooth_window) > 0:
            dirs = [unit(x, y) for x, y in zip(tr.smooth(times, [d[0] for d in dirs], smooth_window), tr.smooth(times, [d[1] for d in dirs], smooth_window))]
        rows = [(i, faces[i][0], quantise_oriented(sm[0][k], sm[1][k], sm[2][k], dirs[k][0], dirs[k][1], size)) for k, i in enumerate(idx)]
        rows = [r for r in rows if r[1] >= t_from and (t_until is None or r[1] < t_until)]
        if segments is None:
            parts = [("track_%05d.%s" % (track, ext), rows)]
        else:
            parts = [("track_%05d_%03d.%s" % (track, k, ext), [r for r in rows if tr.ms(s) <= tr.ms(r[1]) <= tr.ms(e)])
                     for k, (s, e) in enumerate((s, e) for t, s, e in segments if t == track)]
        for fname, part in parts:
            if part and tr.ms(part[-1][1]) - tr.ms(part[0][1]) >= tr.ms(min_length):
                out.append((fname, track, part))
    return out


def index_line(fname, k, T, track, win):
    return "%s %d %.3f %d %d %d %d %d %d\n" % ((fname, k, T, track) + tuple(win))


def tube_files(frames, faces, S, fmt="npy", matrix="601", full_range=False, rate="25:1", **kw):
    """{file name: bytes} and the index lines of `tube --align`, by a plain loop: a warp per picture"""
    files, index = {}, []
    for fname, track, rows in plan(faces, S, ext=fmt, **kw):
        pics = [warps([frames[faces[i][2]]], [win], S, "rgb" if fmt == "npy" else "yuv420", matrix, full_range)[0] for i, _, win in rows]
        files[fname] = tr.file_bytes(pics, S, fmt, rate, full_range)
        index += [index_line(fname, k, T, track, win) for k, (i, T, win) in enumerate(rows)]
    return files, index
