"""BLEND.md restated in numpy and plain Python, independently of pyannote_video_amd/blend.py and csrc/blend.hip: the blend record of a
frame (the thumbnail through tests/storyboard_ref.py, the luma, the sums, the row), the transition rules and the refinement of the
shots.  The GPU tests hold the kernels to this with np.array_equal; tests/test_blend_ref.py holds this to hand-computed cases and shows
that the comparison sees planted defects."""
import numpy as np

from tests import storyboard_ref

LAGS = (4, 8, 16, 32)
ABSENT = 0xFFFFFFFF
MAX_PIXELS = 16384
HISTORY = 32
DEFECTS = ("mid_off_by_one", "lag_swapped", "e_r_exchanged", "luma_floor", "tail_dropped", "history_reversed", "no_sentinel", "s2_wraps")


# ---- the row ------------------------------------------------------------------------------------------------------------------------
def tile_size(width, w, h):
    """th keeps the frame's aspect, rounded half up, at least 1 (STORYBOARD.md): 1920 x 1080 at 64 gives 64 x 36"""
    return int(width), max(1, (2 * int(width) * int(h) + int(w)) // (2 * int(w)))


def luma_of(g, defect=None):
    """uint8 [P] of a thumbnail uint8 [th, tw, 3]"""
    g = np.asarray(g).astype(np.int64).reshape(-1, 3)
    return ((77 * g[:, 0] + 150 * g[:, 1] + 29 * g[:, 2] + (0 if defect == "luma_floor" else 128)) >> 8).astype(np.uint8)


def plane(frame, tw, th, defect=None):
    return luma_of(storyboard_ref.thumb(frame, tw, th), defect)


def sums(y, defect=None):
    """(S1, S2) of a plane as Python ints, whatever its length"""
    y = np.asarray(y).reshape(-1).astype(np.int64)               # (255^2 P stays far below 2^63)
    if defect == "tail_dropped":
        y = y[:len(y) - len(y) % 4]
    s1, s2 = int(y.sum()), int((y * y).sum())
    return s1, (s2 & 0xFFFFFFFF if defect == "s2_wraps" else s2)


def sad(a, b, defect=None):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if defect == "tail_dropped":
        a, b = a[:len(a) - len(a) % 4], b[:len(b) - len(b) % 4]
    return int(np.abs(a - b).sum())


def rows_of(planes, first=0, size_word=0, defect=None):
    """uint32 [N - first, 16]: the rows of planes first .. N - 1 of uint8 [N, P], the planes in front of them as history; the words of
    the caller are 0"""
    planes = np.asarray(planes, np.uint8)
    N, P = planes.shape
    assert 1 <= P <= MAX_PIXELS, "beyond the cap a row cannot hold S2 (sums() shows it)"
    Y = planes.astype(np.int64)
    out = np.zeros((N - first, 16), np.uint32)
    lags = {4: 8, 8: 4}.get if defect == "lag_swapped" else (lambda L, _=None: None)
    for t in range(first, N):
        r = out[t - first]
        r[0] = P
        r[1], r[2] = sums(planes[t], defect)
        absent = 0 if defect == "no_sentinel" else ABSENT
        r[3] = sad(Y[t], Y[t - 1], defect) if t >= 1 else absent
        for k, slot in enumerate(LAGS):
            L = lags(slot) or slot
            if t - L < 0:
                E = R = absent
            else:
                mid = t - L // 2 - (1 if defect == "mid_off_by_one" else 0)
                E, R = sad(Y[t], Y[t - L], defect), sad(2 * Y[mid], Y[t - L] + Y[t], defect)
            if defect == "e_r_exchanged":
                E, R = R, E
            r[4 + 2 * k], r[5 + 2 * k] = E, R
        r[14] = size_word
    return out


def frame_rows(frames, tw, th, hist=None, defect=None):
    """(rows uint32 [n, 16], luma uint8 [n, P]) of frames uint8 [h, w, 3] with hist uint8 [nh, P] in front, oldest first"""
    P = tw * th
    hist = np.zeros((0, P), np.uint8) if hist is None else np.asarray(hist, np.uint8).reshape(-1, P)
    if defect == "history_reversed":
        hist = hist[::-1]
    luma = np.stack([plane(f, tw, th, defect) for f in frames]).reshape(-1, P) if len(frames) else np.zeros((0, P), np.uint8)
    return rows_of(np.concatenate([hist, luma]), first=len(hist), size_word=tw | th << 16, defect=defect), luma


def ms(t):
    return int(round(float(t) * 1000.0))


def stamp(rows, times, first=0):
    rows = np.array(rows, np.uint32)
    for k, t in enumerate(times):
        rows[k, 12], rows[k, 13] = ms(t), first + k
    return rows


def video_rows(frames, tw, th, fps, first=0):
    """what the `blend` verb writes for frames first, first + 1, ... of a video: one call, no history, stamped"""
    rows, _ = frame_rows(frames, tw, th)
    return stamp(rows, [(first + k) / float(fps) for k in range(len(rows))], first)


# ---- the transition rules -----------------------------------------------------------------------------------------------------------
def scaled(x, unit):
    return int(np.floor(unit * float(x) + 0.5))


def passes(rows, t, k, move16, lin256):
    L = LAGS[k]
    P, E, R = int(rows[t, 0]), int(rows[t, 4 + 2 * k]), int(rows[t, 5 + 2 * k])
    return t - L >= 0 and E != ABSENT and R != ABSENT and 16 * E >= move16 * P and 256 * R <= lin256 * E


def centre_halves(rows, move16, lin256):
    half = np.zeros(len(rows), np.int64)
    for k in reversed(range(len(LAGS))):         # the widest first, so that the narrowest is written last
        for t in range(len(rows)):
            if passes(rows, t, k, move16, lin256):
                half[t - LAGS[k] // 2] = LAGS[k] // 2
    return half


def spans(half):
    """the spans of the runs of marked centres, merged while one starts at most one frame behind the end of the one before"""
    n = len(half)
    marked = np.concatenate(([0], (np.asarray(half) > 0).astype(np.int8), [0]))
    step = np.diff(marked)
    raw = []
    for a, b in zip(np.nonzero(step == 1)[0], np.nonzero(step == -1)[0]):          # centres [a, b)
        c = np.arange(a, b)
        raw.append((max(int((c - half[a:b]).min()), 0), min(int((c + half[a:b]).max()), n - 1)))
    raw.sort()
    merged = []
    for s, e in raw:
        if merged and s <= merged[-1][1] + 1:
            merged[-1][1] = max(merged[-1][1], e)
        else:
            merged.append([s, e])
    return [tuple(m) for m in merged]


def is_flat(row, flat16):
    P, S1, S2 = int(row[0]), int(row[1]), int(row[2])
    return 256 * (P * S2 - S1 * S1) <= flat16 * flat16 * P * P


def transitions(rows, move=4.0, linear=0.25, flat=2.0, min_duration=0.12):
    """-> ([(kind, s, e)] in row indices, the rows at which --refined cuts)"""
    move16, lin256, flat16 = scaled(move, 16), scaled(linear, 256), scaled(flat, 16)
    t_ms = [int(r[12]) for r in rows]
    least = ms(min_duration)
    flat_at = [is_flat(r, flat16) for r in rows]
    edge = np.diff(np.concatenate(([0], np.array(flat_at, np.int8), [0])))
    blanks = [(int(a), int(b) - 1) for a, b in zip(np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0])]
    out, cuts = [], set()
    for s, e in spans(centre_halves(rows, move16, lin256)):
        if t_ms[e] - t_ms[s] < least:
            continue
        if flat_at[e] and not flat_at[s]:
            kind, at = "fade-out", e
        elif flat_at[s] and not flat_at[e]:
            kind, at = "fade-in", s
        else:
            kind, at = "dissolve", None
        out.append((kind, s, e))
        if at is None:
            cuts.add((s + e) // 2)
        else:
            a, b = [r for r in blanks if r[0] <= at <= r[1]][0]
            cuts.add((a + b) // 2)
    out += [("blank", a, b) for a, b in blanks if t_ms[b] - t_ms[a] >= least]
    order = ("dissolve", "fade-out", "fade-in", "blank")
    return sorted(out, key=lambda f: (f[1], f[2], order.index(f[0]))), sorted(cuts)


def report(rows, **kw):
    """the list the `transition` verb writes"""
    found, _ = transitions(rows, **kw)
    return [{"kind": k, "start": round(int(rows[s, 12]) / 1000.0, 3), "end": round(int(rows[e, 12]) / 1000.0, 3), "first": int(rows[s, 13]),
             "last": int(rows[e, 13])} for k, s, e in found]


def refined(rows, shots, **kw):
    """shots [(start, end)] -> the pieces [(start, end)]: every shot cut at the cut frames' times that lie strictly inside it"""
    _, cuts = transitions(rows, **kw)
    times = sorted(set(int(rows[c, 12]) / 1000.0 for c in cuts))
    out = []
    for a, b in shots:
        at = a
        for t in times:
            if a < t < b:
                out.append((at, t))
                at = t
        out.append((at, b))
    return out
