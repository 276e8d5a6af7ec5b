"""CLOTHES.md restated in numpy and plain Python, for clarity and not for speed: the bin of a pixel, the histogram of windows per group and
band, the torso window and the skip rules, the file `clothes` writes, and every rule of `link`.  The kernels (csrc/clothes.hip) and the
package (pyannote_video_amd/clothes.py) are held to this bit for bit.  `defect` plants one named mistake, so that the tests can show that
the comparison on the case table would see it."""
import math

import numpy as np

BINS, HEAD, ONE = 256, 6, 65536
DEFECTS = ("edge", "band_clipped", "logical_shift", "no_clamp", "swapped_group", "dropped_chunk", "pad_counted", "wrap32", "no_round",
           "truncate", "lead_counted")


def luma(rgb, defect=None):
    rgb = np.asarray(rgb).astype(np.int64)
    return (77 * rgb[..., 0] + 150 * rgb[..., 1] + 29 * rgb[..., 2] + (0 if defect == "no_round" else 128)) >> 8


def chroma(rgb, defect=None):
    """(c1, c2) = (R - G, floor((2 B - R - G) / 2)); numpy's >> on signed integers is the arithmetic shift"""
    rgb = np.asarray(rgb).astype(np.int64)
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    d = 2 * B - R - G
    if defect == "logical_shift":            # the bits of a negative int32 shifted as unsigned
        c2 = (d & 0xFFFFFFFF) >> 1
    elif defect == "truncate":               # towards zero
        c2 = np.sign(d) * (np.abs(d) // 2)
    else:
        c2 = d >> 1
    return R - G, c2


def q(c, defect=None):
    v = (np.asarray(c) + 64) >> 4
    return v if defect == "no_clamp" else np.minimum(np.maximum(v, 0), 7)


def bins_of(rgb, defect=None):
    """the bin of every pixel of uint8 [..., 3]"""
    c1, c2 = chroma(rgb, defect)
    return ((luma(rgb, defect) >> 6) * 64 + q(c1, defect) * 8 + q(c2, defect)) & 255      # (& 255 changes nothing without a defect)


_every = {}


def every_colour():
    """(reachable bins ascending, one (R, G, B) that reaches each): all 2^24 colours through the rule"""
    if not _every:
        first = {}
        gb = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), axis=-1).reshape(-1, 2)
        for R in range(256):
            rgb = np.concatenate([np.full((len(gb), 1), R), gb], axis=1)
            b, at = np.unique(bins_of(rgb), return_index=True)
            for k, i in zip(b.tolist(), at.tolist()):
                first.setdefault(k, tuple(int(v) for v in rgb[i]))
        _every["bins"] = np.array(sorted(first), np.int64)
        _every["colours"] = np.array([first[k] for k in sorted(first)], np.uint8)
    return _every["bins"], _every["colours"]


def wrap32(v):
    return (int(v) + (1 << 31)) % (1 << 32) - (1 << 31)


def clip_of(win, w, h, defect=None):
    """(cx0, cy0, cx1, cy1) of the window inside a w x h frame, in Python ints, or None where nothing is left"""
    x0, y0, x1, y1 = (int(v) for v in win)
    if defect == "wrap32" and (wrap32(x1 - x0) <= 0 or wrap32(y1 - y0) <= 0):
        return None
    if defect == "edge":
        x1 += 1
    if x1 <= x0 or y1 <= y0:
        return None
    c = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
    return c if c[2] > c[0] and c[3] > c[1] else None


def window_hist(bins, win, B, defect=None):
    """int64 [B][256]: the window's pixels inside the frame whose bins are `bins` [h][w], per band"""
    h, w = bins.shape
    out = np.zeros((B, BINS), np.int64)
    c = clip_of(win, w, h, defect)
    if c is None:
        return out
    cx0, cy0, cx1, cy1 = c
    y0, H = int(win[1]), int(win[3]) - int(win[1])
    if defect == "band_clipped":
        y0, H = cy0, cy1 - cy0
    for y in range(cy0, cy1):
        band = ((y - y0) * B) // H
        n = cx1 - cx0
        if defect == "dropped_chunk":        # the pixels that reach into the row's last, partial 16-byte chunk
            a, e = 3 * (y * w + cx0), 3 * (y * w + cx1)
            n = max(0, e // 16 * 16 - a) // 3 if e % 16 else n
        if defect == "lead_counted":         # counting from the row's first 16-byte chunk: the bytes in front of the row's first pixel
            at = max(0, y * w + cx0 - (3 * (y * w + cx0) % 16) // 3)
            out[band] += np.bincount(bins.reshape(-1)[at:at + n], minlength=BINS)
            continue
        out[band] += np.bincount(bins[y, cx0:cx0 + n], minlength=BINS)
    if defect == "pad_counted" and int(win[3]) - int(win[1]) <= 1 << 16:        # black outside the frame (where a loop can walk the rows)
        x0, x1, y1 = int(win[0]), int(win[2]), int(win[3])
        for y in range(int(win[1]), y1):
            inside = (cx1 - cx0) if cy0 <= y < cy1 else 0
            out[((y - int(win[1])) * B) // H, int(bins_of(np.zeros(3, np.uint8)))] += (x1 - x0) - inside
    return out


def hist_of(frames, windows, group, G, B, defect=None, known=None):
    """uint32 [G][B][256] of pvf_frame_hist: frames[i] is the uint8 [h][w][3] frame of window i.  known: {id(frame): bins}, kept by a
    caller that asks about the same frames again"""
    known = {} if known is None else known
    out = np.zeros((G, B, BINS), np.int64)
    for f, win, g in zip(frames, windows, group):
        if id(f) not in known:
            known[id(f)] = bins_of(f, defect)
        g = int(g)
        if defect == "swapped_group" and (g ^ 1) < G:
            g ^= 1
        out[g] += window_hist(known[id(f)], win, B, defect)
    assert defect is not None or out.max(initial=0) < 1 << 32
    return out.astype(np.uint32)


# ---- the verb `clothes` --------------------------------------------------------------------------------------------------------------
def half_up(x):
    return int(math.floor(float(x) + 0.5))


def ms(t):
    return int(round(float(t) * 1000.0))


def torso(box, widen=0.5, drop=0.25, height=2.0):
    l, t, r, b = (int(v) for v in box)
    w, h = r - l, b - t
    x0, x1 = l - half_up(widen * w), r + half_up(widen * w)
    y0 = b + half_up(drop * h)
    return x0, y0, x1, y0 + half_up(height * h)


def counted(faces, W, H, widen=0.5, drop=0.25, height=2.0, min_size=0.0, keep_overlapped=False):
    """[(track, box)] of one frame -> [window or None]"""
    out = []
    for track, box in faces:
        win = torso(box, widen, drop, height)
        ok = clip_of(win, W, H) is not None and not (int(box[3]) - int(box[1])) < min_size * H
        if ok and not keep_overlapped:
            for other, (l, t, r, b) in faces:
                if other != track and max(win[0], l) < min(win[2], r) and max(win[1], t) < min(win[3], b):
                    ok = False
        out.append(win if ok else None)
    return out


def table_of(frames, per_frame, tracks, bands=2, **kw):
    """the file of `clothes` by a plain loop, a face at a time.  frames: {frame index: rgb}; per_frame: [(frame index, T, [(track, box)])]
    of the selected range; tracks: every track of the tracking file"""
    tracks = sorted(tracks)
    table = np.zeros((len(tracks), HEAD + BINS * bands), np.int64)
    table[:, 0], table[:, 1], table[:, 2], table[:, 5] = tracks, -1, -1, bands
    frames = dict((fi, np.asarray(frames[fi])) for fi, _, _ in per_frame)              # held: `known` goes by the identity of a frame
    known = {}
    for fi, T, faces in per_frame:
        h, w = frames[fi].shape[:2]
        for (track, box), win in zip(faces, counted(faces, w, h, **kw)):
            r = table[tracks.index(track)]
            r[1] = ms(T) if r[1] < 0 else min(r[1], ms(T))
            r[2] = max(r[2], ms(T))
            if win is None:
                r[4] += 1
                continue
            r[3] += 1
            r[HEAD:] += hist_of([frames[fi]], [win], [0], 1, bands, known=known).reshape(-1)
    return table


# ---- the verb `link` -----------------------------------------------------------------------------------------------------------------
def threshold(x):
    return half_up(float(x) * ONE)


def is_usable(row, min_faces=3, min_pixels=20000):
    bands = int(row[5])
    N = [sum(int(v) for v in row[HEAD + BINS * b:HEAD + BINS * (b + 1)]) for b in range(bands)]
    return int(row[3]) >= min_faces and all(n > 0 for n in N) and sum(N) >= min_pixels


def score(ra, rc):
    """the histogram intersection of two usable rows, 0 .. 65536, in Python ints"""
    bands, total = int(ra[5]), 0
    for b in range(bands):
        ha = [int(v) for v in ra[HEAD + BINS * b:HEAD + BINS * (b + 1)]]
        hc = [int(v) for v in rc[HEAD + BINS * b:HEAD + BINS * (b + 1)]]
        Na, Nc = sum(ha), sum(hc)
        total += sum(min(x * ONE // Na, y * ONE // Nc) for x, y in zip(ha, hc))
    return total // bands


def apart(ra, rc):
    """ms between the extents [first, last] of two rows, or None where they intersect"""
    if int(ra[1]) <= int(rc[2]) and int(rc[1]) <= int(ra[2]):
        return None
    return int(rc[1]) - int(ra[2]) if int(rc[1]) > int(ra[2]) else int(ra[1]) - int(rc[2])


def links_of(table, min_score=0.75, margin=0.05, max_gap=120.0, min_faces=3, min_pixels=20000):
    """[(a, b, score)], a < b, sorted"""
    rows = [r for r in table if is_usable(r, min_faces, min_pixels)]

    def choice(ra):
        """(the best candidate's track, its score) where it leads the second best by the margin, else None"""
        cand = [(score(ra, rc), int(rc[0])) for rc in rows if int(rc[0]) != int(ra[0]) and apart(ra, rc) is not None and apart(ra, rc) <= ms(max_gap)]
        if not cand:
            return None
        cand.sort(key=lambda c: (-c[0], c[1]))
        lead = ONE if len(cand) == 1 else cand[0][0] - cand[1][0]
        return (cand[0][1], cand[0][0]) if lead >= threshold(margin) else None
    best = dict((int(r[0]), choice(r)) for r in rows)
    found = []
    for a in sorted(best):
        if best[a] is not None:
            c, s = best[a]
            if a < c and best[c] is not None and best[c][0] == a and s >= threshold(min_score):
                found.append((a, c, s))
    return found


def merged_labels(labels, found, table):
    extent = dict((int(r[0]), (int(r[1]), int(r[2]))) for r in table if int(r[1]) >= 0)
    name = dict(labels)
    for a, b, s in sorted(found, key=lambda f: (-f[2], f[0], f[1])):
        if a not in name or b not in name or name[a] == name[b]:
            continue
        A = sorted(t for t in name if name[t] == name[a])
        B = sorted(t for t in name if name[t] == name[b])
        if any(u in extent and v in extent and extent[u][0] <= extent[v][1] and extent[v][0] <= extent[u][1] for u in A for v in B):
            continue
        if len(A) > len(B) or (len(A) == len(B) and A[0] < B[0]):
            keep, gone = name[a], B
        else:
            keep, gone = name[b], A
        for t in gone:
            name[t] = keep
    return name
