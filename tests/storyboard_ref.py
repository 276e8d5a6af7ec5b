"""STORYBOARD.md restated in numpy and plain Python, independently of pyannote_video_amd/storyboard.py and csrc/board.hip: the
thumbnail (weights built literally from the interval definition, int64 sums), the sheet, and every host rule of the verb.  The GPU
tests hold the kernels to this bit for bit; tests/test_storyboard_ref.py holds this to hand-computed cases and shows that the
comparison sees planted defects."""
import numpy as np

from tests import demo_ref

GAP = 6
BACKGROUND = (24, 24, 24)
NEUTRAL = (200, 200, 200)


# ---- the thumbnail ------------------------------------------------------------------------------------------------------------------
def weights(n_src, n_out):
    """int64 [n_out, n_src]: in units of 1 / n_out source sample, source j is [j n_out, (j + 1) n_out), output X is [X n_src,
    (X + 1) n_src); the entry is the length of their intersection.  Every row sums to n_src."""
    j = np.arange(n_src, dtype=np.int64)[None, :]
    X = np.arange(n_out, dtype=np.int64)[:, None]
    lo = np.maximum(j * n_out, X * n_src)
    hi = np.minimum((j + 1) * n_out, (X + 1) * n_src)
    return np.maximum(hi - lo, 0)


DEFECTS = ("truncate", "shift_column", "swap_axes", "wrap32", "drop_last_row", "drop_row_tail", "swap_channels")


def thumb(frame, tw, th, defect=None):
    """uint8 [th, tw, 3] of uint8 [h, w, 3]: (sum_i sum_j wy wx byte + (w h) // 2) // (w h).  Zero weights are skipped, nothing else.
    defect: one of DEFECTS, what a kernel could get wrong (the tests plant them to show that the comparison sees them)."""
    frame = np.asarray(frame, np.uint8)
    h, w = frame.shape[:2]
    if defect == "swap_axes":                    # the frame's memory read as [w][h]
        frame = np.ascontiguousarray(frame).reshape(w, h, 3).transpose(1, 0, 2)
    wx, wy = weights(w, tw), weights(h, th)
    if defect == "shift_column":
        wx = np.roll(wx, 1, axis=1)
    if defect == "drop_row_tail":
        wx = wx.copy(); wx[:, -1] = 0
    if defect == "drop_last_row":
        wy = wy.copy(); wy[:, -1] = 0
    rows = np.zeros((h, tw, 3), np.int64)
    for X in range(tw):
        nz = np.nonzero(wx[X])[0]
        rows[:, X, :] = np.tensordot(frame[:, nz, :].astype(np.int64), wx[X, nz], axes=([1], [0]))
    total = np.zeros((th, tw, 3), np.int64)
    for Y in range(th):
        nz = np.nonzero(wy[Y])[0]
        total[Y] = np.tensordot(wy[Y, nz], rows[nz], axes=([0], [0]))
    den = w * h
    if defect == "wrap32":
        total = total & 0xFFFFFFFF
    out = ((total + (0 if defect == "truncate" else den // 2)) // den).astype(np.uint8)
    return out[:, :, ::-1].copy() if defect == "swap_channels" else out


def thumbs(frames, tw, th, defect=None):
    return np.stack([thumb(f, tw, th, defect) for f in frames]).reshape(-1, th, tw, 3)


def mismatch(got, want):
    """None when the two pictures (or batches) are the same bytes, else where they first differ: what every GPU comparison goes through"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape %s %s against %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return None
    at = tuple(int(v) for v in bad[0])
    return "%d of %d bytes differ, first at %s: %d against %d" % (len(bad), got.size, at, got[at], want[at])


# ---- the sheet ----------------------------------------------------------------------------------------------------------------------
def sheet(tiles, xy, W, H, background=(0, 0, 0), prims=(), first_wins=False):
    """uint8 [H, W, 3]: background, the tiles uint8 [n, th, tw, 3] copied in list order (clipped), the primitives over them.
    Defect: first_wins -- an earlier tile lies over a later one"""
    img = np.empty((H, W, 3), np.uint8)
    img[:, :] = background
    order = list(range(len(tiles)))
    for i in (reversed(order) if first_wins else order):
        th, tw = tiles[i].shape[:2]
        x, y = int(xy[i][0]), int(xy[i][1])
        xa, xb, ya, yb = max(x, 0), min(x + tw, W), max(y, 0), min(y + th, H)
        if xa >= xb or ya >= yb:
            continue
        img[ya:yb, xa:xb] = tiles[i][ya - y:yb - y, xa - x:xb - x]
    return demo_ref.draw(img, list(prims))


# ---- the host rules -----------------------------------------------------------------------------------------------------------------
def idx(fps, t):
    return int(fps * t + 1e-5)


def picks(start, end, fps, n_frames, K):
    a = idx(fps, start)
    if a >= n_frames:
        return None
    b = min(max(a, idx(fps, end) - 1), n_frames - 1)
    m = b - a + 1
    out = []
    for k in range(K):
        f = a + ((2 * k + 1) * m) // (2 * K)
        if f not in out:
            out.append(f)
    return out


def tile_size(width, w, h):
    return width, max(1, (2 * width * h + w) // (2 * w))


def caption(number, start, label=None):
    tenths = int(round(start * 10.0))
    s = "%d %d:%02d.%d" % (number, tenths // 600, tenths % 600 // 10, tenths % 10)
    return s if label is None else s + " " + label


def ranks(labels):
    seen = []
    for l in labels:
        if l is not None and l not in seen:
            seen.append(l)
    return {l: r for r, l in enumerate(seen)}


def layout(cells, K, tw, th, columns, by="time"):
    """cells: [(number, start, label, shown)] in time order -> (W, H, corners per cell, prims in demo_ref's form, sheet order)"""
    s = max(1, tw // 80)
    cw, ch = GAP + K * (tw + GAP), 3 * GAP + 7 * s + th
    rk = ranks([c[2] for c in cells])
    order = list(range(len(cells)))
    if by == "thread":
        order.sort(key=lambda i: (rk.get(cells[i][2], len(rk)), cells[i][1], i))
    corners, prims = [None] * len(cells), []
    col = row = widest = 0
    for p, i in enumerate(order):
        new_thread = by == "thread" and p > 0 and rk.get(cells[i][2], len(rk)) != rk.get(cells[order[p - 1]][2], len(rk))
        if p > 0 and (new_thread or col == columns):
            col, row = 0, row + 1
        number, start, label, shown = cells[i]
        x, y = col * cw, row * ch
        rgb = tuple(demo_ref.PALETTE[rk[label] % len(demo_ref.PALETTE)]) if label is not None else NEUTRAL
        data = caption(number, start, label).encode("utf-8")[:min(demo_ref.MAX_RUN, (cw - 2 * GAP) // (6 * s))]
        prims.append((demo_ref.TEXT, x + GAP, y + GAP + 7 * s - 1, rgb, s, data))
        tx, ty = x + GAP, y + 2 * GAP + 7 * s
        n = min(shown, K)
        corners[i] = [(tx + k * (tw + GAP), ty) for k in range(n)]
        if n:
            prims.append((demo_ref.RECT, tx - 1, ty - 1, tx + (n - 1) * (tw + GAP) + tw, ty + th, rgb))
        col += 1
        widest = max(widest, col)
    return widest * cw, (row + 1) * ch, corners, prims, order


def labels_of(shots, tracks):
    """shots: [(start, end)]; tracks: [(start, end, label)] in (start, end) order -> the label of the first track that holds a shot's middle"""
    out = []
    for a, b in shots:
        mid = (a + b) / 2.0
        out.append(next((l for ta, tb, l in tracks if ta <= mid < tb), None))
    return out


def board(frame_of, shots, labels, fps, n_frames, w, h, per=1, width=160, columns=None, by="time", t_from=0.0, t_until=None):
    """the verb by a plain loop: (sheet, index text).  frame_of(i) -> uint8 [h, w, 3]; shots: [(start, end)]"""
    tw, th = tile_size(width, w, h)
    chosen = []
    for number, ((a, b), label) in enumerate(zip(shots, labels)):
        if a < t_from or (t_until is not None and not a < t_until):
            continue
        fr = picks(a, b, fps, n_frames, per)
        if fr is not None:
            chosen.append((number, a, label, fr))
    cols = columns if columns else max(1, 1920 // (GAP + per * (tw + GAP)))
    W, H, corners, prims, order = layout([(c[0], c[1], c[2], len(c[3])) for c in chosen], per, tw, th, cols, by)
    tiles, xy, lines = [], [], []
    for ci in order:
        number, _, label, fr = chosen[ci]
        for k, f in enumerate(fr):
            tiles.append(thumb(frame_of(f), tw, th))
            xy.append(corners[ci][k])
            lines.append("%d %d %d %.3f %d %d %s\n" % (number, k, f, f / fps, xy[-1][0], xy[-1][1], "-" if label is None else label))
    return sheet(tiles, xy, W, H, BACKGROUND, prims), "".join(lines)
