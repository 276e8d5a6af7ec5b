"""The host rules of the `blend` and `transition` verbs (BLEND.md): a blend file's words, how the history of luma planes is carried from
one library call to the next, how the rows become fades, dissolves and blank stretches, and how those refine the shots of `shot`.
Nothing here touches the device but `Carry.measure`, which calls runtime.Context.frame_blend."""
import numpy as np

from .storyboard import tile_size        # noqa: F401 -- th follows from --width as a storyboard thumbnail's does
from .talk import half_up, ms

LAGS = (4, 8, 16, 32)                    # PVF_BLEND_LAGS
ABSENT = 0xFFFFFFFF                      # a sum whose earlier frame does not exist
MAX_PIXELS = 16384                       # PVF_BLEND_MAX_PIXELS
HISTORY = 32                             # PVF_BLEND_MAX_HISTORY
WORDS = 16
KINDS = ("dissolve", "fade-out", "fade-in", "blank", "camera")       # camera: with `transition --motion` only


def stamp(rows, first, frame_rate):
    """fills the caller's words of the rows of frames first, first + 1, ...: ms(T) and the frame index, T = index / frame_rate"""
    for k in range(len(rows)):
        i = first + k
        rows[k, 12] = ms(i / float(frame_rate))
        rows[k, 13] = i
    return rows


class Carry(object):
    """the rows of a video, batch by batch: keeps the last 32 luma planes of what it has measured as the history of the next call, so
    the rows do not depend on how the frames are cut into calls"""

    def __init__(self, ctx, tw, th):
        if tw < 1 or th < 1 or tw * th > MAX_PIXELS:
            raise ValueError("blend: a thumbnail of %d x %d pixels; lower --width (at most %d pixels)" % (tw, th, MAX_PIXELS))
        self.ctx, self.tw, self.th = ctx, int(tw), int(th)
        self.hist = np.zeros((0, self.tw * self.th), np.uint8)

    def measure(self, frames):
        """-> (rows uint32 [len(frames), 16], the frames the caller may release now: all of them, the planes are what is carried)"""
        rows, luma = self.ctx.frame_blend(frames, self.tw, self.th, hist=self.hist)
        self.hist = np.concatenate([self.hist, luma])[-HISTORY:]
        return rows, list(frames)


def load(path):
    """a blend file: uint32 [n][16]"""
    try:
        r = np.load(path, allow_pickle=False)
    except Exception as e:                   # noqa: BLE001 -- whatever numpy raises for a file that is no array
        raise ValueError("transition: %s is not a blend file (%s)" % (path, e))
    if r.dtype != np.uint32 or r.ndim != 2 or r.shape[1] != WORDS:
        raise ValueError("transition: %s is not a blend file: uint32 [n][16] is expected, %s %s found" % (path, r.dtype, list(r.shape)))
    return np.ascontiguousarray(r)


def halves(rows, move16, lin256):
    """int [n]: half[c] = the smallest L / 2 among the passing (t, L) with c = t - L / 2, else 0"""
    n = len(rows)
    half = [0] * n
    for t in range(n):
        P = int(rows[t, 0])
        for k, L in enumerate(LAGS):
            E, R = int(rows[t, 4 + 2 * k]), int(rows[t, 5 + 2 * k])
            if E == ABSENT or R == ABSENT or t - L < 0:
                continue
            if 16 * E >= move16 * P and 256 * R <= lin256 * E:
                c = t - L // 2
                if half[c] == 0 or L // 2 < half[c]:
                    half[c] = L // 2
    return half


def spans_of(half):
    """runs of consecutive centres -> [(s, e)] by s, merged where they overlap or touch (the next starts at most one frame behind the end)"""
    n, raw, c = len(half), [], 0
    while c < n:
        if half[c] == 0:
            c += 1
            continue
        s, e = c - half[c], c + half[c]
        while c + 1 < n and half[c + 1] > 0:
            c += 1
            s, e = min(s, c - half[c]), max(e, c + half[c])
        raw.append((max(s, 0), min(e, n - 1)))
        c += 1
    out = []
    for s, e in sorted(raw):
        if out and s <= out[-1][1] + 1:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        else:
            out.append((s, e))
    return out


def flat_frames(rows, flat16):
    """bool [n]: 256 (P S2 - S1^2) <= flat16^2 P^2"""
    return [256 * (int(r[0]) * int(r[2]) - int(r[1]) ** 2) <= flat16 * flat16 * int(r[0]) ** 2 for r in rows]


def flat_runs(flat):
    """maximal runs [(a, b)] of flat frames"""
    out, t, n = [], 0, len(flat)
    while t < n:
        if not flat[t]:
            t += 1
            continue
        a = t
        while t + 1 < n and flat[t + 1]:
            t += 1
        out.append((a, t))
        t += 1
    return out


def analyse(rows, move=4.0, linear=0.25, flat=2.0, min_duration=0.12, moving=None):
    """-> ([(kind, s, e)] in row indices by (s, e, kind), the cut rows of --refined).  moving: the frame indices (word 13) that lie inside a
    pan, tilt or zoom (motion.moving_frames): a span with more than half of its frames among them is a `camera` span and cuts nothing."""
    move16, lin256, flat16 = half_up(16.0 * move), half_up(256.0 * linear), half_up(16.0 * flat)
    if move16 < 1 or lin256 < 0 or flat16 < 0:
        raise ValueError("transition: --move is above 0, --linear and --flat are not negative")
    t_ms = [int(v) for v in rows[:, 12]]
    long_enough = ms(min_duration)
    is_flat = flat_frames(rows, flat16)
    runs = flat_runs(is_flat)
    found, cuts = [], set()

    def run_of(t):
        return [r for r in runs if r[0] <= t <= r[1]][0]
    for s, e in spans_of(halves(rows, move16, lin256)):
        if t_ms[e] - t_ms[s] < long_enough:
            continue
        kind = "fade-out" if is_flat[e] and not is_flat[s] else "fade-in" if is_flat[s] and not is_flat[e] else "dissolve"
        if moving is not None and 2 * sum(1 for r in range(s, e + 1) if int(rows[r, 13]) in moving) > e - s + 1:
            kind = "camera"
        found.append((kind, s, e))
        if kind == "camera":
            continue
        if kind == "dissolve":
            cuts.add((s + e) // 2)
        else:
            a, b = run_of(e if kind == "fade-out" else s)
            cuts.add((a + b) // 2)
    for a, b in runs:
        if t_ms[b] - t_ms[a] >= long_enough:
            found.append(("blank", a, b))
    found.sort(key=lambda f: (f[1], f[2], KINDS.index(f[0])))
    return found, sorted(cuts)


def report(rows, found):
    """the list the verb writes"""
    return [{"kind": kind, "start": round(int(rows[s, 12]) / 1000.0, 3), "end": round(int(rows[e, 12]) / 1000.0, 3),
             "first": int(rows[s, 13]), "last": int(rows[e, 13])} for kind, s, e in found]


def refine(shots, cut_times):
    """shots [(start, end)] seconds, cut at every time that lies strictly inside one: the pieces tile what the shots covered"""
    out = []
    for a, b in shots:
        edges = [a] + [t for t in sorted(set(cut_times)) if a < t < b] + [b]
        out.extend(zip(edges[:-1], edges[1:]))
    return out
