"""TUBE.md restated in numpy: a window of a frame as an S x S picture in both regimes, its YUV 4:2:0 form, the host rules of tube.py and
the table of named cases the GPU tests run.  The kernel (csrc/tube.hip) is compared with `crop` / `crops` bit for bit; tube.py with the
host rules.  The keyword arguments plant the defects that test_tube_ref.py shows the comparison to see; none is used anywhere else."""
import io
import math

import numpy as np

import demo_ref

MIN_SIZE, MAX_SIZE = 1, 1024             # PVF_CROP_MIN_SIZE, PVF_CROP_MAX_SIZE
MIN_SIDE, MAX_SIDE = 16, 1 << 18         # PVF_CROP_MIN_SIDE, PVF_CROP_MAX_SIDE
MAX_COORD = 1 << 30                      # PVF_CROP_MAX_COORD
MAX_CROPS = 65536                        # PVF_CROP_MAX_CROPS
# the seams of csrc/tube.hip: output columns of a block, output rows of a block, source pixels of a staged row piece
C_COLS, C_BAND, C_TILE_PX = 128, 16, 2720


# ---- window -> picture ----------------------------------------------------------------------------------------------------------------
def reduce_weights(P0, L, S, n, last_off=0, clamp=False):
    """area average along one axis: [(source index, weight)] per output sample, in units of 1 / (16 S) pixel; every list sums to L.
    Indices outside 0 .. n - 1 are left out (black) unless clamp."""
    P0, L, S = int(P0), int(L), int(S)
    U, out = 16 * S, []
    for j in range(S):
        lo = S * P0 + j * L
        hi = lo + L
        taps = []
        for p in range(lo // U, (hi - 1) // U + 1):
            w = min(hi, U * (p + 1)) - max(lo, U * p)
            if p == (hi - 1) // U and p != lo // U:
                w += last_off
            taps.append((p, w))
        out.append(taps)
    return _inside(out, n, clamp)


def enlarge_weights(P0, L, S, n, clamp=False, truncate=False):
    """bilinear along one axis at the sample centres, in units of 1 / (32 S) pixel; every list sums to 32 S"""
    P0, L, S = int(P0), int(L), int(S)
    V, out = 32 * S, []
    for j in range(S):
        u = 2 * S * P0 + (2 * j + 1) * L - 16 * S
        x0 = int(u / V) if truncate else u // V
        fx = u - V * x0
        out.append([(x0, V - fx), (x0 + 1, fx)])
    return _inside(out, n, clamp)


def _inside(taps, n, clamp):
    if clamp:
        return [[(min(max(p, 0), n - 1), w) for p, w in t] for t in taps]
    return [[(p, w) for p, w in t if 0 <= p < n] for t in taps]


def _matrix(taps, n):
    """[S][hi - lo] float64 weights (exact: integers below 2^19) and the first source index they touch"""
    used = [p for t in taps for p, _ in t]
    if not used:
        return np.zeros((len(taps), 0)), 0
    lo, hi = min(used), max(used) + 1
    W = np.zeros((len(taps), hi - lo), np.float64)
    for j, t in enumerate(taps):
        for p, w in t:
            W[j, p - lo] += w
    return W, lo


def crop(frame, window, S, rounding=True, last_off=0, clamp=False, swap=False, truncate=False, wrap32=False):
    """uint8 [S][S][3]: the window (X0, Y0, L) of uint8 [h][w][3].  The sums run in float64, where they are exact: every partial sum
    is an integer below L^2 * 255 < 2^44."""
    frame = np.asarray(frame)
    h, w = frame.shape[:2]
    X0, Y0, L = (int(v) for v in window)
    S = int(S)
    enlarging = (L > 16 * S) if swap else (L < 16 * S)
    if enlarging:
        tx, ty, den = enlarge_weights(X0, L, S, w, clamp, truncate), enlarge_weights(Y0, L, S, h, clamp, truncate), 1024 * S * S
    else:
        tx, ty, den = reduce_weights(X0, L, S, w, last_off, clamp), reduce_weights(Y0, L, S, h, 0, clamp), L * L
    Wx, x0 = _matrix(tx, w)
    Wy, y0 = _matrix(ty, h)
    out = np.zeros((S, S, 3), np.uint8)
    if Wx.shape[1] == 0 or Wy.shape[1] == 0:
        return out
    sub = frame[y0:y0 + Wy.shape[1], x0:x0 + Wx.shape[1]].astype(np.float64)
    for c in range(3):
        total = (Wy @ sub[:, :, c] @ Wx.T).astype(np.int64)
        if wrap32:
            total &= 0xffffffff
        out[:, :, c] = (total + (den // 2 if rounding else 0)) // den
    return out


def to_yuv(rgb, matrix="601", full_range=False, wrong_chroma=False):
    """Y, U, V of an S x S RGB picture, tight: DEMO.md's conversion"""
    y, u, v = demo_ref.to_yuv420(rgb, matrix, full_range)
    if wrong_chroma:                     # the 2 x 2 blocks taken one pixel to the right
        _, u, v = demo_ref.to_yuv420(np.roll(rgb, -1, axis=1), matrix, full_range)
    return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])


def crops(frames, windows, S, layout="rgb", matrix="601", full_range=False, neighbour=False, **defects):
    """what Context.frame_crops returns"""
    wrong_chroma = defects.pop("wrong_chroma", False)
    out = []
    for i, win in enumerate(windows):
        f = frames[(i + 1) % len(frames)] if neighbour else frames[i]
        rgb = crop(f, win, S, **defects)
        out.append(rgb if layout == "rgb" else to_yuv(rgb, matrix, full_range, wrong_chroma))
    if not out:
        return np.zeros((0, S, S, 3) if layout == "rgb" else (0, S * S + 2 * ((S + 1) // 2) ** 2), np.uint8)
    return np.stack(out)


def picture(h, w, seed):
    """a frame without flat areas or symmetry: noise over two gradients"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(3 * x + y) % 256, (x + 5 * y + 60) % 256, (7 * x + 2 * y + 120) % 256], axis=2)
    return ((base + rng.randint(0, 96, (h, w, 3))) % 256).astype(np.uint8)


def window_cases(h, w, S):
    """{name: (X0, Y0, L)}: the named windows of the issue on an h x w frame at picture size S"""
    n = 16 * S
    side = 16 * min(h, w)
    c = {
        "identity": (0, 0, n),
        "seam_below": (37, 21, max(n - 1, MIN_SIDE)), "seam": (37, 21, n), "seam_above": (37, 21, n + 1),
        "one_pixel": (16 * (w // 2), 16 * (h // 2), 16),
        "one_pixel_phase": (16 * (w // 2) + 5, 16 * (h // 2) + 11, 16),
        "cross_left": (-side // 3, 16 * 3, side // 2), "cross_right": (16 * w - side // 3, 16 * 2, side // 2),
        "cross_top": (16 * 5, -side // 3, side // 2), "cross_bottom": (16 * 4, 16 * h - side // 3, side // 2),
        "corner_tl": (-side // 4 - 3, -side // 4 - 7, side // 2), "corner_tr": (16 * w - side // 4 + 3, -side // 4, side // 2),
        "corner_bl": (-side // 4, 16 * h - side // 4 + 5, side // 2), "corner_br": (16 * w - side // 4 - 9, 16 * h - side // 4 - 1, side // 2),
        "last_pixel": (16 * w - side // 2, 16 * h - side // 2, side // 2),
        "last_pixel_only": (16 * (w - 1), 16 * (h - 1), 16),
        # (a pixel away: an enlarging window's first samples reach half a pixel beyond its edge)
        "outside_left": (-2 * side, 0, side), "outside_right": (16 * w + 16, 0, side),
        "outside_top": (0, -side - 17, side), "outside_bottom": (0, 16 * h + 21, side),
        "dwarf": (-16 * 2 * w + 8, -16 * 2 * h - 8, 4 * 16 * max(h, w)),
        "cap_far": (MAX_COORD, -MAX_COORD, MAX_SIDE), "cap_far2": (-MAX_COORD, MAX_COORD, 16),
        "cap_over": (-MAX_SIDE // 2 + 16 * w // 2, -MAX_SIDE // 2 + 16 * h // 2, MAX_SIDE),
        "enlarge": (16 * 3 + 7, 16 * 2 + 3, max(16, (n * 2) // 5)),
        "reduce": (9, 4, min(side - 16, (n * 7) // 3) if side - 16 >= n else n),
    }
    for k in range(4):                   # left edges at every residue of the byte offset mod 4
        c["residue_%d" % k] = (16 * (k + 1) + 3, 16 * 1, side // 2)
    return c


def phase_windows(S):
    """all 16 x 16 sub-pixel phases at L = 16 S"""
    return [(16 + fx, 16 + fy, 16 * S) for fy in range(16) for fx in range(16)]


# ---- host rules ------------------------------------------------------------------------------------------------------------------------
def ms(t):
    return int(round(float(t) * 1000.0))


def face_region(box, scale=1.6):
    l, t, r, b = (int(v) for v in box)
    return (l + r) / 2.0, (t + b) / 2.0, float(scale) * float(max(r - l, b - t))


def mouth_region(box, pts, scale=0.5):
    p = np.asarray(pts).reshape(68, 2)
    sx = sum(int(v) for v in p[48:68, 0])
    sy = sum(int(v) for v in p[48:68, 1])
    l, t, r, b = (int(v) for v in box)
    return sx / 20.0, sy / 20.0, float(scale) * float(max(r - l, b - t))


def smooth(times, values, window):
    t, w = [ms(x) for x in times], ms(window)
    out = []
    for i in range(len(t)):
        total, n = 0.0, 0
        for j in range(len(t)):
            if 2 * abs(t[j] - t[i]) <= w:
                total += values[j]
                n += 1
        out.append(total / n)
    return out


def quantise(cx, cy, side):
    L = min(max(int(math.floor(float(side) * 16.0 + 0.5)), MIN_SIDE), MAX_SIDE)
    X0 = int(math.floor(float(cx) * 16.0 - L / 2.0 + 0.5))
    Y0 = int(math.floor(float(cy) * 16.0 - L / 2.0 + 0.5))
    return min(max(X0, -MAX_COORD), MAX_COORD), min(max(Y0, -MAX_COORD), MAX_COORD), L


def plan(faces, region="face", scale=None, smooth_window=0.5, labels=None, only=None, segments=None, min_length=0.0, t_from=0.0, t_until=None,
         ext="npy"):
    """faces: [(T, track, frame index, box, points or None)] -> [(file name, track, [(face index, T, (X0, Y0, L))])] by track, then span"""
    scale = (1.6 if region == "face" else 0.5) if scale is None else scale
    tracks = {}
    for i, f in enumerate(faces):
        tracks.setdefault(int(f[1]), []).append(i)
    out = []
    for track in sorted(tracks):
        name = (labels or {}).get(track) or "#%d" % track
        if only is not None and not (name in only or name.lstrip("#") in only):
            continue
        idx = sorted(tracks[track], key=lambda i: (ms(faces[i][0]), i))
        raw = [face_region(faces[i][3], scale) if region == "face" else mouth_region(faces[i][3], faces[i][4], scale) for i in idx]
        times = [faces[i][0] for i in idx]
        sm = [smooth(times, [r[k] for r in raw], smooth_window) for k in range(3)]
        rows = [(i, faces[i][0], quantise(sm[0][k], sm[1][k], sm[2][k])) for k, i in enumerate(idx)]
        rows = [r for r in rows if r[1] >= t_from and (t_until is None or r[1] < t_until)]
        if segments is None:
            parts = [("track_%05d.%s" % (track, ext), rows)]
        else:
            parts = [("track_%05d_%03d.%s" % (track, k, ext), [r for r in rows if ms(s) <= ms(r[1]) <= ms(e)])
                     for k, (s, e) in enumerate((s, e) for tr, s, e in segments if tr == track)]
        for fname, part in parts:
            if part and ms(part[-1][1]) - ms(part[0][1]) >= ms(min_length):
                out.append((fname, track, part))
    return out


def file_bytes(pictures, S, fmt, rate="25:1", full_range=False):
    """the bytes of one tube file: pictures is uint8 [n][S][S][3] (npy) or [n][frame bytes] (y4m)"""
    if fmt == "npy":
        f = io.BytesIO()
        np.save(f, np.ascontiguousarray(pictures, np.uint8).reshape(-1, S, S, 3))
        return f.getvalue()
    head = "YUV4MPEG2 W%d H%d F%s C420%s\n" % (S, S, rate, " XCOLORRANGE=FULL" if full_range else "")
    return head.encode("ascii") + b"".join(b"FRAME\n" + np.asarray(p, np.uint8).tobytes() for p in pictures)


def tube_files(frames, faces, S, fmt="npy", matrix="601", full_range=False, rate="25:1", **kw):
    """{file name: bytes} and the index lines, by a plain loop: a crop per picture"""
    files, index = {}, []
    for fname, track, rows in plan(faces, ext=fmt, **kw):
        pics = [crops([frames[faces[i][2]]], [win], S, "rgb" if fmt == "npy" else "yuv420", matrix, full_range)[0] for i, _, win in rows]
        files[fname] = file_bytes(pics, S, fmt, rate, full_range)
        for k, (i, T, win) in enumerate(rows):
            index.append("%s %d %.3f %d %d %d %d\n" % ((fname, k, T, track) + tuple(win)))
    return files, index
