"""The host rules of the `clothes` and `link` verbs (CLOTHES.md): the torso window under a face box, which faces are skipped, how the
windows of a film go through runtime.Context.frame_hist in batches, the file, and how `link` scores pairs of tracks, finds the mutual
best matches and merges a label file along them.  Everything is integer arithmetic but the one float-to-int rule, `half_up`.  Nothing
here touches the device but `measure`."""
import numpy as np

from .talk import half_up, ms             # half_up: the float-to-int rule of both verbs (CLOTHES.md)

BINS = 256                               # PVF_HIST_BINS
MAX_BANDS = 4                            # PVF_HIST_MAX_BANDS
MAX_WINDOWS = 65536                      # PVF_HIST_MAX_WINDOWS: windows of one library call
HEAD = 6                                 # track, first ms, last ms, faces used, faces skipped, bands
ONE = 65536                              # the unit of scores and thresholds


def torso(box, widen=0.5, drop=0.25, height=2.0):
    """the window (x0, y0, x1, y1) under the face box (l, t, r, b), integer pixels: `widen` face widths more on either side, from `drop`
    face heights below the box, `height` face heights tall"""
    l, t, r, b = (int(v) for v in box)
    w, h = r - l, b - t
    dx = half_up(float(widen) * w)
    y0 = b + half_up(float(drop) * h)
    return l - dx, y0, r + dx, y0 + half_up(float(height) * h)


def clipped(win, W, H):
    x0, y0, x1, y1 = win
    return max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)


def meets(win, box):
    """the half-open rectangles share a pixel"""
    return max(win[0], box[0]) < min(win[2], box[2]) and max(win[1], box[1]) < min(win[3], box[3])


def windows_of(faces, W, H, widen=0.5, drop=0.25, height=2.0, min_size=0.0, keep_overlapped=False):
    """faces: [(track, (l, t, r, b))] of one frame -> [window or None] in their order; None: the face is skipped -- its box is lower
    than min_size * H, its clipped window is empty, or (unless keep_overlapped) its window meets the face box of another track"""
    out = []
    for track, box in faces:
        win = torso(box, widen, drop, height)
        cx0, cy0, cx1, cy1 = clipped(win, W, H)
        skip = (int(box[3]) - int(box[1])) < float(min_size) * H or cx1 <= cx0 or cy1 <= cy0
        if not skip and not keep_overlapped:
            skip = any(other != track and meets(win, b) for other, b in faces)
        out.append(None if skip else win)
    return out


def measure(ctx, frames, windows, tracks, bands, table, row_of):
    """one library call: the histograms of `windows` of `frames`, grouped by track, added into the int64 table"""
    present = sorted(set(tracks))
    index = dict((t, g) for g, t in enumerate(present))
    got = ctx.frame_hist(frames, np.array(windows, np.int32).reshape(-1, 4), np.array([index[t] for t in tracks], np.int32), len(present), bands=bands)
    for g, t in enumerate(present):
        table[row_of[t], HEAD:] += got[g].reshape(-1).astype(np.int64)


def load(path, who="link"):
    """a clothes file: int64 [T][6 + 256 bands], one band count, ascending tracks"""
    try:
        t = np.load(path, allow_pickle=False)
    except Exception as e:                   # noqa: BLE001 -- whatever numpy raises for a file that is no array
        raise ValueError("%s: %s is not a clothes file (%s)" % (who, path, e))
    return check(t, who, path)


def check(t, who="link", path="the table"):
    if t.dtype != np.int64 or t.ndim != 2 or t.shape[1] < HEAD + BINS or (t.shape[1] - HEAD) % BINS or (t.shape[1] - HEAD) // BINS > MAX_BANDS:
        raise ValueError("%s: %s is not a clothes file: int64 [T][6 + 256 bands] is expected, %s %s found" % (who, path, t.dtype, list(t.shape)))
    bands = (t.shape[1] - HEAD) // BINS
    if len(t) and ((t[:, 5] != bands).any() or (np.diff(t[:, 0]) <= 0).any() or (t[:, HEAD:] < 0).any()):
        raise ValueError("%s: %s holds rows of another band count, tracks out of order or negative counts" % (who, path))
    return np.ascontiguousarray(t)


def fraction(x, name):
    v = half_up(float(x) * ONE)
    if not 0 <= v <= ONE:
        raise ValueError("link: --%s is 0 .. 1" % name)
    return v


def usable(table, min_faces=3, min_pixels=20000):
    """bool [T]: faces used >= min_faces, every band non-empty, total pixels >= min_pixels"""
    bands = (table.shape[1] - HEAD) // BINS
    N = table[:, HEAD:].reshape(len(table), bands, BINS).sum(axis=2)
    return (table[:, 3] >= int(min_faces)) & (N > 0).all(axis=1) & (N.sum(axis=1) >= int(min_pixels))


def scores(table, ok):
    """int64 [T][T]: the histogram intersection of every pair of usable tracks in 0 .. 65536, -1 elsewhere and on the diagonal"""
    T = len(table)
    bands = (table.shape[1] - HEAD) // BINS
    S = np.full((T, T), -1, np.int64)
    idx = np.nonzero(ok)[0]
    if len(idx) == 0:
        return S
    h = table[idx, HEAD:].reshape(len(idx), bands, BINS)
    p = (h * ONE) // h.sum(axis=2, keepdims=True)          # (a count is below 2^47 or the file is no film's: the product fits)
    for k, a in enumerate(idx):
        S[a, idx] = np.minimum(p[k][None], p).sum(axis=(1, 2)) // bands
    S[np.arange(T), np.arange(T)] = -1
    return S


def gap_ms(a, c):
    """the time between two rows' extents in ms, or None where they intersect"""
    if a[1] <= c[2] and c[1] <= a[2]:
        return None
    return int(c[1] - a[2]) if c[1] > a[2] else int(a[1] - c[2])


def links(table, min_score=0.75, margin=0.05, max_gap=120.0, min_faces=3, min_pixels=20000):
    """-> [(a, b, score)] track numbers with a < b, sorted: the pairs that are each other's best candidate by at least the margin"""
    least, by, far = fraction(min_score, "min-score"), fraction(margin, "margin"), ms(max_gap)
    if far < 0 or int(min_faces) < 0 or int(min_pixels) < 0:
        raise ValueError("link: --max-gap, --min-faces and --min-pixels are not negative")
    ok = usable(table, min_faces, min_pixels)
    S = scores(table, ok)
    T = len(table)
    best = {}
    for a in range(T):
        if not ok[a]:
            continue
        cand = []
        for c in range(T):
            if c != a and ok[c]:
                g = gap_ms(table[a], table[c])
                if g is not None and g <= far:
                    cand.append((-int(S[a, c]), int(table[c, 0]), c))
        if not cand:
            continue
        cand.sort()
        lead = ONE if len(cand) == 1 else cand[1][0] - cand[0][0]
        if lead >= by:
            best[a] = cand[0][2]
    found = []
    for a, c in sorted(best.items()):
        if a < c and best.get(c) == a and int(S[a, c]) >= least:
            found.append((int(table[a, 0]), int(table[c, 0]), int(S[a, c])))
    return found


def merge_labels(labels, found, table):
    """{track: name} with clusters merged along the links, best first; a union is skipped when a track of one side is on screen with a
    track of the other; the merged cluster keeps the name of the side with more tracks (tie: the side with the smallest track)"""
    extent = dict((int(r[0]), (int(r[1]), int(r[2]))) for r in table if r[1] >= 0)
    name = dict((int(t), str(n)) for t, n in labels.items())
    members = {}
    for t, n in name.items():
        members.setdefault(n, set()).add(t)

    def together(u, v):
        return u in extent and v in extent and extent[u][0] <= extent[v][1] and extent[v][0] <= extent[u][1]
    for a, b, s in sorted(found, key=lambda f: (-f[2], f[0], f[1])):
        if a not in name or b not in name or name[a] == name[b]:
            continue
        A, B = members[name[a]], members[name[b]]
        if any(together(u, v) for u in A for v in B):
            continue
        keep, gone = (name[a], name[b]) if (len(A), -min(A)) > (len(B), -min(B)) else (name[b], name[a])
        for t in members.pop(gone):
            name[t] = keep
            members[keep].add(t)
    return name
