"""The host rules of the `motion` and `camera` verbs (MOTION.md): a motion file's words, how a batch hands its last frame to the next call,
how the rows become pans, tilts, zooms and static stretches, and which frames of a file lie inside a camera move (`transition --motion`).
Nothing here touches the device but `Pairs.measure`, which calls runtime.Context.shot_motion."""
import numpy as np

from .storyboard import tile_size        # noqa: F401 -- th follows from --width as a storyboard thumbnail's does
from .talk import half_up, ms

WORDS = 10
MIN_SIDE, MAX_SIDE, MAX_PIXELS = 12, 256, 16384          # PVF_MOTION_MIN_SIDE, _MAX_SIDE, _MAX_PIXELS
MOVES = ("pan-left", "pan-right", "tilt-up", "tilt-down", "zoom-in", "zoom-out")
KINDS = MOVES + ("static",)
LOW32 = 0xFFFFFFFF


def div_half_up(a, b):
    """floor(a / b + 1 / 2) of integers, b > 0"""
    return (2 * int(a) + int(b)) // (2 * int(b))


def stamp(rows, first, frame_rate):
    """fills the caller's word of the rows of frames first, first + 1, ...: ms(T) | index << 32, T = index / frame_rate"""
    for k in range(len(rows)):
        i = first + k
        rows[k, 8] = ms(i / float(frame_rate)) | i << 32
    return rows


class Pairs(object):
    """the rows of a video, batch by batch: the last frame of a batch stays resident as the first frame of the next call, so every
    consecutive pair is measured once and the rows do not depend on how the frames are cut into calls"""

    def __init__(self, ctx, tw, th, tables=None):
        if not (MIN_SIDE <= tw <= MAX_SIDE and MIN_SIDE <= th <= MAX_SIDE) or tw * th > MAX_PIXELS:
            raise ValueError("motion: a small image of %d x %d pixels; sides of %d .. %d and at most %d pixels are measured (--width)"
                             % (tw, th, MIN_SIDE, MAX_SIDE, MAX_PIXELS))
        from . import structure
        self.ctx, self.tw, self.th = ctx, int(tw), int(th)
        self.tables = structure.shot_tables() if tables is None else tables
        self.held = None                         # the frame in front of the next batch

    def measure(self, frames):
        """-> (rows int64 [len(frames), 10], the frames the caller may release now: the one held from before and all but the last of
        these).  The first frame of the video gets a row without valid pixels."""
        if not frames:
            return np.zeros((0, WORDS), np.int64), []
        chain = ([self.held] if self.held is not None else []) + list(frames)
        rows, _ = self.ctx.shot_motion(chain, self.tw, self.th, self.tables)
        if self.held is None:
            head = np.zeros((1, WORDS), np.int64)
            head[0, 9] = self.tw | self.th << 16
            rows = np.concatenate([head, rows])
        self.held = chain[-1]
        return rows, chain[:-1]


def load(path, who="camera"):
    """a motion file: int64 [n][10]"""
    try:
        r = np.load(path, allow_pickle=False)
    except Exception as e:                   # noqa: BLE001 -- whatever numpy raises for a file that is no array
        raise ValueError("%s: %s is not a motion file (%s)" % (who, path, e))
    if r.dtype != np.int64 or r.ndim != 2 or r.shape[1] != WORDS:
        raise ValueError("%s: %s is not a motion file: int64 [n][10] is expected, %s %s found" % (who, path, r.dtype, list(r.shape)))
    return np.ascontiguousarray(r)


def fields(row):
    r = [int(v) for v in row]
    return {"n_valid": r[0] & LOW32, "n_in": r[0] >> 32, "tx": r[1], "ty": r[2], "a": r[3], "b": r[4], "m": r[5], "ms": r[8] & LOW32,
            "index": r[8] >> 32, "w": r[9] & 0xFFFF, "h": r[9] >> 16}


def per_frame(f):
    """(pan, tilt, zoom, roll) of a row in thousandths per frame: of the frame's width, of its height, of its scale, of a radian"""
    if f["w"] == 0 or f["h"] == 0:
        return 0, 0, 0, 0
    return (div_half_up(1000 * f["tx"], f["w"] << 22), div_half_up(1000 * f["ty"], f["h"] << 22), div_half_up(1000 * f["a"], 1 << 21),
            div_half_up(1000 * f["b"], 1 << 21))


def label_rows(rows, pan=5.0, zoom=3.0, window=0.5, min_inliers=50, shots=None):
    """-> (label or None per row, the labelled quantity's rate per second in thousandths, the shot of every row)"""
    pan10, zoom10 = half_up(10.0 * pan), half_up(10.0 * zoom)
    if pan10 < 1 or zoom10 < 1:
        raise ValueError("camera: --pan and --zoom are above 0")
    if not 0 <= int(min_inliers) <= 100 or window < 0:
        raise ValueError("camera: --min-inliers is 0 .. 100, --window is not negative")
    f = [fields(r) for r in rows]
    n = len(f)
    t = [x["ms"] for x in f]
    if shots is None:
        shot = [0] * n
    else:
        edges = [(ms(a), ms(b)) for a, b in shots]
        shot = [next((k for k, (a, b) in enumerate(edges) if a <= t[i] < b), -1) for i in range(n)]
    reliable = [False] * n
    for i in range(1, n):
        reliable[i] = (f[i]["n_valid"] > 0 and 100 * f[i]["n_in"] >= int(min_inliers) * f[i]["n_valid"] and shot[i] >= 0
                       and shot[i] == shot[i - 1])
    rates = [per_frame(x) for x in f]
    width = ms(window)
    thresholds = (pan10, pan10, zoom10)
    labels, values = [None] * n, [0] * n
    lo = 0
    for i in range(n):
        if not reliable[i]:
            continue
        while 2 * (t[i] - t[lo]) > width:
            lo += 1
        sums, span, j = [0, 0, 0], 0, lo
        while j < n and 2 * (t[j] - t[i]) <= width:
            if reliable[j] and shot[j] == shot[i]:
                span += t[j] - t[j - 1]
                for q in range(3):
                    sums[q] += rates[j][q]
            j += 1
        per_second = [div_half_up(1000 * s, span) if span > 0 else 0 for s in sums]
        best = 0
        for q in (1, 2):
            if abs(per_second[q]) * thresholds[best] > abs(per_second[best]) * thresholds[q]:
                best = q
        if abs(per_second[best]) >= thresholds[best]:
            labels[i] = MOVES[2 * best + (0 if per_second[best] > 0 else 1)]
            values[i] = per_second[best]
        else:
            labels[i] = "static"
    return labels, values, shot, t


def analyse(rows, pan=5.0, zoom=3.0, window=0.5, min_inliers=50, min_duration=0.5, max_gap=0.2, shots=None):
    """-> [(kind, s, e, rate)] in row indices by (s, e, kind)"""
    if min_duration < 0 or max_gap < 0:
        raise ValueError("camera: --min-duration and --max-gap are not negative")
    labels, values, shot, t = label_rows(rows, pan=pan, zoom=zoom, window=window, min_inliers=min_inliers, shots=shots)
    bridge, least = ms(max_gap), ms(min_duration)
    found = []
    for kind in KINDS:
        at = [i for i in range(len(labels)) if labels[i] == kind]
        spans = []
        for i in at:
            if spans and shot[spans[-1][1]] == shot[i] and (i == spans[-1][1] + 1 or t[i] - t[spans[-1][1]] <= bridge):
                spans[-1][1] = i
            else:
                spans.append([i, i])
        for s, e in spans:
            if t[e] - t[s] < least:
                continue
            mine = [values[i] for i in range(s, e + 1) if labels[i] == kind]
            found.append((kind, s, e, div_half_up(sum(mine), len(mine))))
    found.sort(key=lambda r: (r[1], r[2], KINDS.index(r[0])))
    return found


def report(rows, found):
    """the list the verb writes"""
    return [{"kind": kind, "start": round((int(rows[s, 8]) & LOW32) / 1000.0, 3), "end": round((int(rows[e, 8]) & LOW32) / 1000.0, 3),
             "first": int(rows[s, 8]) >> 32, "last": int(rows[e, 8]) >> 32, "rate": rate} for kind, s, e, rate in found]


def moving_frames(rows):
    """the frame indices inside a pan, tilt or zoom span of the file, under the default rules"""
    inside = set()
    for kind, s, e, _ in analyse(rows):
        if kind in MOVES:
            inside.update(range(int(rows[s, 8]) >> 32, (int(rows[e, 8]) >> 32) + 1))
    return inside
