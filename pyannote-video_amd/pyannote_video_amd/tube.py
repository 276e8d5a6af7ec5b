"""The host side of the `tube` verb (TUBE.md): from the boxes of a track (and, for mouth tubes, the 68 points of its faces) to one square
window per picture, in sixteenths of a source pixel, and from the pictures the library returns (csrc/tube.hip) to one file per tube.
The pixels are the library's; what is here is three floats per face, in float64 with one operation order, and the files."""
import collections
import math

import numpy as np

from .talk import ms

MIN_SIZE, MAX_SIZE = 1, 1024             # PVF_CROP_MIN_SIZE, PVF_CROP_MAX_SIZE
MIN_SIDE, MAX_SIDE = 16, 1 << 18         # PVF_CROP_MIN_SIDE, PVF_CROP_MAX_SIDE
MAX_COORD = 1 << 30                      # PVF_CROP_MAX_COORD
MAX_CROPS = 65536                        # PVF_CROP_MAX_CROPS
MAX_K, MAX_STEP = 16, 1 << 20            # PVF_WARP_MAX_K, PVF_WARP_MAX_STEP
SCALE = {"face": 1.6, "mouth": 0.5}
MAX_OPEN = 64                            # tube files open at a time (FilePool)


def face_region(box, scale=SCALE["face"]):
    """(centre x, centre y, side) in pixels: the centre of the track box, `scale` times the larger of its width and height"""
    l, t, r, b = (int(v) for v in box)
    return (l + r) / 2.0, (t + b) / 2.0, float(scale) * float(max(r - l, b - t))


def mouth_region(box, pts, scale=SCALE["mouth"]):
    """the mean of landmark points 48 .. 67 (integer sums, one division by 20.0 each); `scale` times the face region's side at scale 1"""
    p = np.asarray(pts).reshape(68, 2)
    sx = sum(int(v) for v in p[48:68, 0])
    sy = sum(int(v) for v in p[48:68, 1])
    l, t, r, b = (int(v) for v in box)
    return sx / 20.0, sy / 20.0, float(scale) * float(max(r - l, b - t))


def smooth(times, values, window):
    """one track in time order: the mean of `values` over the rows with 2 |ms(t') - ms(t)| <= ms(window), summed in time order"""
    t, w = [ms(x) for x in times], ms(window)
    out, lo = [], 0
    for i in range(len(t)):
        while 2 * (t[i] - t[lo]) > w:
            lo += 1
        total, n, j = 0.0, 0, lo
        while j < len(t) and 2 * (t[j] - t[i]) <= w:
            total += values[j]
            n += 1
            j += 1
        out.append(total / n)
    return out


def quantise(cx, cy, side):
    """three floats -> (X0, Y0, L): L = floor(16 side + 0.5) clipped to MIN_SIDE .. MAX_SIDE, then X0 = floor(16 cx - L / 2 + 0.5)
    (the product, the difference, the sum, in that order) and Y0 likewise, clipped to +-MAX_COORD"""
    L = min(max(int(math.floor(float(side) * 16.0 + 0.5)), MIN_SIDE), MAX_SIDE)
    X0 = int(math.floor(float(cx) * 16.0 - L / 2.0 + 0.5))
    Y0 = int(math.floor(float(cy) * 16.0 - L / 2.0 + 0.5))
    return min(max(X0, -MAX_COORD), MAX_COORD), min(max(Y0, -MAX_COORD), MAX_COORD), L


def eye_direction(pts):
    """the unit vector from the mean of points 36 .. 41 to the mean of points 42 .. 47 (integer sums, each divided by 6.0): the row
    direction of an aligned window.  (1.0, 0.0) for coincident eyes or a face without points."""
    if pts is None:
        return 1.0, 0.0
    p = np.asarray(pts).reshape(68, 2)
    e0x, e0y = sum(int(v) for v in p[36:42, 0]) / 6.0, sum(int(v) for v in p[36:42, 1]) / 6.0
    e1x, e1y = sum(int(v) for v in p[42:48, 0]) / 6.0, sum(int(v) for v in p[42:48, 1]) / 6.0
    return unit(e1x - e0x, e1y - e0y)


def unit(dx, dy):
    """(dx, dy) / hypot(dx, dy); (1.0, 0.0) for a vector of length 0"""
    length = math.hypot(dx, dy)
    return (dx / length, dy / length) if length > 0.0 else (1.0, 0.0)


def quantise_oriented(cx, cy, side, c, s, S):
    """centre, side and unit row direction -> (CX, CY, BX, BY, K) for pictures of side S (TUBE.md "Oriented window"):
    CX = floor(16 cx + 0.5); A = (side / S) 65536 (c, s); K the smallest of 1 .. MAX_K with (65536 K)^2 >= AX^2 + AY^2 on the components
    rounded half up to integers (MAX_K if none); B = floor(A / K + 0.5), clipped to +-MAX_STEP"""
    CX = min(max(int(math.floor(16.0 * float(cx) + 0.5)), -MAX_COORD), MAX_COORD)
    CY = min(max(int(math.floor(16.0 * float(cy) + 0.5)), -MAX_COORD), MAX_COORD)
    lim = float(MAX_K * MAX_STEP * 2)                            # (a step beyond it is clipped to the cap whatever K is)
    ax = min(max(float(side) / float(S) * 65536.0 * float(c), -lim), lim)
    ay = min(max(float(side) / float(S) * 65536.0 * float(s), -lim), lim)
    AX, AY = int(math.floor(ax + 0.5)), int(math.floor(ay + 0.5))
    K = MAX_K
    for k in range(1, MAX_K):
        if (65536 * k) ** 2 >= AX * AX + AY * AY:
            K = k
            break
    BX = min(max(int(math.floor(ax / K + 0.5)), -MAX_STEP), MAX_STEP)
    BY = min(max(int(math.floor(ay / K + 0.5)), -MAX_STEP), MAX_STEP)
    return CX, CY, BX, BY, K


def read_segments(path):
    """`track start end ...` lines, what `talk --segments` writes -> [(track, start, end)] in file order"""
    out = []
    with open(path) as f:
        for number, line in enumerate(f, 1):
            p = line.split()
            if not p:
                continue
            if len(p) < 3:
                raise ValueError("%s:%d: expected `track start end`, found %r" % (path, number, line.rstrip("\n")))
            out.append((int(p[0]), float(p[1]), float(p[2])))
    return out


def plan(faces, region="face", scale=None, smooth_window=0.5, labels=None, only=None, segments=None, min_length=0.0, t_from=0.0, t_until=None,
         ext="npy", align=False, size=None):
    """faces: [(T, track, frame index, box, points or None)] in any order -> [(file name, track, [(face index, T, (X0, Y0, L))])] by
    track, then span; with align, for pictures of side `size`, the windows are (CX, CY, BX, BY, K) along the smoothed eye line.
    A track's windows are smoothed over all its rows, whatever is selected afterwards: --from / --until, a span (ms(start) <= ms(T) <= ms(end)) and --min-length (ms(last T) - ms(first T) >= ms(min_length)) only choose among them."""
    if region not in SCALE:
        raise ValueError("tube: the region is face or mouth")
    scale = SCALE[region] if scale is None else float(scale)
    tracks = {}
    for i, f in enumerate(faces):
        tracks.setdefault(int(f[1]), []).append(i)
    out = []
    for track in sorted(tracks):
        name = (labels or {}).get(track) or "#%d" % track
        if only is not None and not (name in only or name.lstrip("#") in only):
            continue
        idx = sorted(tracks[track], key=lambda i: (ms(faces[i][0]), i))
        if region == "face":
            raw = [face_region(faces[i][3], scale) for i in idx]
        else:
            raw = [mouth_region(faces[i][3], faces[i][4], scale) for i in idx]
        times = [faces[i][0] for i in idx]
        sm = [smooth(times, [r[k] for r in raw], smooth_window) for k in range(3)]
        if align:
            # the direction is smoothed as a vector, component by component, and made a unit vector again: a track that passes +-180
            # degrees stays there; with --smooth 0 it is the raw direction
            dirs = [eye_direction(faces[i][4]) for i in idx]
            if ms(smooth_window) > 0:
                dirs = [unit(x, y) for x, y in zip(smooth(times, [d[0] for d in dirs], smooth_window), smooth(times, [d[1] for d in dirs], smooth_window))]
            rows = [(i, faces[i][0], quantise_oriented(sm[0][k], sm[1][k], sm[2][k], dirs[k][0], dirs[k][1], size)) for k, i in enumerate(idx)]
        else:
            rows = [(i, faces[i][0], quantise(sm[0][k], sm[1][k], sm[2][k])) for k, i in enumerate(idx)]
        rows = [r for r in rows if r[1] >= t_from and (t_until is None or r[1] < t_until)]
        if segments is None:
            parts = [("track_%05d.%s" % (track, ext), rows)]
        else:
            spans = [(s, e) for tr, s, e in segments if tr == track]
            parts = [("track_%05d_%03d.%s" % (track, k, ext), [r for r in rows if ms(s) <= ms(r[1]) <= ms(e)]) for k, (s, e) in enumerate(spans)]
        for fname, part in parts:
            if part and ms(part[-1][1]) - ms(part[0][1]) >= ms(min_length):
                out.append((fname, track, part))
    return out


def index_line(fname, k, T, track, window):
    """`file picture T track X0 Y0 L`, or with an oriented window `file picture T track CX CY BX BY K`"""
    return "%s %d %.3f %d" % (fname, k, T, track) + "".join(" %d" % int(v) for v in window) + "\n"


class FilePool(object):
    """Files that are written piece by piece, with at most `max_open` of them open: a film has thousands of tracks, and the pictures
    of the tracks on screen arrive interleaved.  A file is opened for writing the first time it is written to and for appending ever
    after; when one more would be open than allowed, the one written to longest ago is closed."""

    def __init__(self, max_open=MAX_OPEN):
        self.max_open = max(1, int(max_open))
        self._open = collections.OrderedDict()      # path -> file object, least recently written first
        self._seen = set()
        self.peak = 0

    def write(self, path, data):
        f = self._open.pop(path, None)
        if f is None:
            while len(self._open) >= self.max_open:
                self._open.popitem(last=False)[1].close()
            f = open(path, "ab" if path in self._seen else "wb")
            self._seen.add(path)
        self._open[path] = f
        self.peak = max(self.peak, len(self._open))
        f.write(data)

    def done(self, path):
        f = self._open.pop(path, None)
        if f is not None:
            f.close()

    def close(self):
        while self._open:
            self._open.popitem()[1].close()


class PooledFile(object):
    """what render.Y4mWriter and numpy's header writer take for a file: writes go through the pool"""

    def __init__(self, pool, path):
        self.pool, self.path = pool, path

    def write(self, data):
        self.pool.write(self.path, bytes(data))

    def flush(self):
        pass

    def close(self):
        self.pool.done(self.path)


class NpyWriter(object):
    """a uint8 [n][S][S][3] .npy file whose length is known before its first picture: the header goes out first"""

    def __init__(self, target, n, S):
        self._f, self.left, self.picture_bytes = target, int(n), int(S) * int(S) * 3
        np.lib.format.write_array_header_1_0(target, {"descr": "|u1", "fortran_order": False, "shape": (int(n), int(S), int(S), 3)})

    def write(self, picture):
        m = memoryview(np.ascontiguousarray(picture, np.uint8)).cast("B")
        if len(m) != self.picture_bytes or self.left < 1:
            raise ValueError("an unexpected picture for a .npy tube")
        self._f.write(m)
        self.left -= 1

    def close(self):
        self._f.close()
