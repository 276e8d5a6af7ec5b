"""REDACT.md restated in numpy, independent of the package: the cell means of a redaction, its three modes and two shapes composed
over the resized picture, which tracks the verb hides on which frame, and the bytes of the stream `redact` writes.  Resize, the
other primitives and the colour conversion are demo_ref's.  Everything is integer arithmetic, so the GPU is held to it bit for bit."""
import numpy as np

from tests import demo_ref

REDACT = 3
ELLIPSE = 1
MOSAIC, SMOOTH, FILL = 0, 2, 4
MAX_SIDE, MAX_COORD, MAX_CELL, MAX_CELLS = 16384, 1 << 20, 2048, 4096


def _ceil(a, b):
    return -(-a // b)


def has_table(p):
    """a (REDACT, l, t, r, b, colour, cell, flags) primitive with cells to average: not inverted, not a fill"""
    return p[0] == REDACT and p[3] - p[1] + 1 >= 1 and p[4] - p[2] + 1 >= 1 and (p[7] & 6) != FILL


def _means(resized, p):
    """(means uint8 [ny, nx, 3], n int64 [ny, nx]) of one redaction over the resized source picture; n = 0 cells read 0"""
    _, l, t, r, b, _, cell, _ = p
    oh, ow = resized.shape[:2]
    nx, ny = _ceil(r - l + 1, cell), _ceil(b - t + 1, cell)
    means, count = np.zeros((ny, nx, 3), np.uint8), np.zeros((ny, nx), np.int64)
    for j in range(ny):
        ya, yb = max(t + j * cell, 0), min(t + (j + 1) * cell - 1, b, oh - 1)
        if ya > yb:
            continue
        for i in range(nx):
            xa, xb = max(l + i * cell, 0), min(l + (i + 1) * cell - 1, r, ow - 1)
            if xa > xb:
                continue
            n = (xb - xa + 1) * (yb - ya + 1)
            S = resized[ya:yb + 1, xa:xb + 1].astype(np.int64).sum(axis=(0, 1))
            means[j, i] = (S + n // 2) // n
            count[j, i] = n
    return means, count


def cell_means(src, ow, oh, prims):
    """uint8 [cells, 3]: the tables of the list's mosaic and smooth redactions in list order, cells row-major"""
    resized = demo_ref.resize(src, ow, oh)
    out = [_means(resized, p)[0].reshape(-1, 3) for p in prims if has_table(p)]
    return np.concatenate(out) if out else np.zeros((0, 3), np.uint8)


def covered(p, ow, oh):
    """(xa, ya, mask bool [h, w]) of the redaction's pixels inside an ow x oh frame, the mask over region n frame; None if that is empty"""
    _, l, t, r, b, _, _, flags = p
    W, H = r - l + 1, b - t + 1
    if W < 1 or H < 1:
        return None
    xa, xb, ya, yb = max(l, 0), min(r, ow - 1), max(t, 0), min(b, oh - 1)
    if xa > xb or ya > yb:
        return None
    ys, xs = np.mgrid[ya:yb + 1, xa:xb + 1].astype(np.int64)
    if flags & ELLIPSE:                                  # every term below 2^59 (REDACT.md "Limits")
        mask = (2 * xs - (l + r)) ** 2 * (H * H) + (2 * ys - (t + b)) ** 2 * (W * W) <= W * W * H * H
    else:
        mask = np.ones(xs.shape, bool)
    return xa, ya, mask


def draw_redaction(img, resized, p):
    """one redaction onto img, made from `resized` (the source picture before anything was drawn)"""
    oh, ow = img.shape[:2]
    c = covered(p, ow, oh)
    if c is None:
        return
    xa, ya, mask = c
    _, l, t, r, b, colour, cell, flags = p
    h, w = mask.shape
    view = img[ya:ya + h, xa:xa + w]
    mode = flags & 6
    if mode == FILL:
        view[mask] = colour
        return
    means, count = _means(resized, p)
    ys, xs = np.mgrid[ya:ya + h, xa:xa + w].astype(np.int64)
    if mode == MOSAIC:
        view[mask] = means[(ys - t) // cell, (xs - l) // cell][mask]
        return
    # smooth: bilinear between nominal cell centres, neighbours clamped to the index rectangle of cells with n > 0
    jj, ii = np.nonzero(count)
    ilo, ihi, jlo, jhi = ii.min(), ii.max(), jj.min(), jj.max()
    assert (count[jlo:jhi + 1, ilo:ihi + 1] > 0).all()
    ux, uy = 2 * (xs - l) + 1, 2 * (ys - t) + 1
    i0, j0 = (ux - cell) // (2 * cell), (uy - cell) // (2 * cell)
    fx, fy = ux - cell - 2 * cell * i0, uy - cell - 2 * cell * j0
    ia, ib = np.clip(i0, ilo, ihi), np.clip(i0 + 1, ilo, ihi)
    ja, jb = np.clip(j0, jlo, jhi), np.clip(j0 + 1, jlo, jhi)
    m = means.astype(np.int64)
    wx0, wy0 = 2 * cell - fx, 2 * cell - fy
    num = ((wy0 * wx0)[..., None] * m[ja, ia] + (wy0 * fx)[..., None] * m[ja, ib] + (fy * wx0)[..., None] * m[jb, ia] +
           (fy * fx)[..., None] * m[jb, ib] + 2 * cell * cell)
    view[mask] = (num // (4 * cell * cell)).astype(np.uint8)[mask]


def render_rgb(src, ow, oh, prims):
    """the drawn picture: primitives in list order, a redaction always made from the resized source"""
    resized = demo_ref.resize(src, ow, oh)
    img = resized.copy()
    for p in prims:
        if p[0] == REDACT:
            draw_redaction(img, resized, p)
        else:
            demo_ref.draw(img, [p])
    return img


def render(src, ow, oh, prims, matrix="601", full_range=False):
    return b"".join(p.tobytes() for p in demo_ref.to_yuv420(render_rgb(src, ow, oh, prims), matrix, full_range))


# ---- what is hidden when --------------------------------------------------------------------------------------------------------------
def _faces(track_rows, sent, width, height):
    """{index into sent: [(identifier, box)]}: the pacing of demo_ref's generator (one group of equal times per frame at most, in order,
    a group waiting until the time sent has reached its own), but with the LAST group given out too"""
    groups = []
    for row in track_rows:
        T, ident, box = row[0], row[1], row[2]
        item = (ident, tuple(int(float(c) * s) for c, s in zip(box, (width, height, width, height))))
        if groups and groups[-1][0] == T:
            groups[-1][1].append(item)
        else:
            groups.append((T, [item]))
    out, gi = {}, 0
    for k, t in enumerate(sent):
        if gi == len(groups):
            break
        if groups[gi][0] > t:
            continue
        out[k] = groups[gi][1]
        gi += 1
    return out


def pad_box(box, pad):
    l, t, r, b = box
    dx, dy = ((r - l) * pad + 50) // 100, ((b - t) * pad + 50) // 100
    return l - dx, t - dy, r + dx, b + dy


def cell_side(box, cells):
    W, H = max(1, box[2] - box[0] + 1), max(1, box[3] - box[1] + 1)
    cell = min(MAX_CELL, max(1, _ceil(max(W, H), cells)))
    while _ceil(W, cell) * _ceil(H, cell) > MAX_CELLS:
        cell += 1
    return cell


def selected(ident, labels, only, keep):
    if only is not None:
        return labels.get(ident) in only
    if keep is not None:
        return labels.get(ident) not in keep
    return True


def plan(track_rows, fps, n_frames, width, height, labels=None, only=None, keep=None, pad=25, cells=8, shape="ellipse", mode="mosaic",
         colour=(0, 0, 0), t_from=0.0, t_until=None, shift=0.0, draw=False):
    """[(source index, t, primitives)] of the `redact` verb"""
    if only is not None and keep is not None:
        raise ValueError("both")
    if (only is not None or keep is not None) and labels is None:
        raise ValueError("no labels")
    fps = float(fps)
    until = n_frames / fps if t_until is None else t_until
    times, index, k = [], [], 0
    while True:
        t = t_from + k / fps
        i = int(fps * t + 0.00001)
        if not t < until or not 0 <= i < n_frames:
            break
        times.append(t)
        index.append(i)
        k += 1
    faces = _faces(track_rows, [t - shift for t in times], width, height)
    flags = {"mosaic": MOSAIC, "smooth": SMOOTH, "fill": FILL}[mode] | (ELLIPSE if shape == "ellipse" else 0)
    drawn = demo_ref.plan(track_rows, fps, n_frames, width, height, None, labels, t_from, t_until, shift) if draw else None
    out = []
    for k, t in enumerate(times):
        prims = []
        for ident, box in faces.get(k, ()):
            if selected(ident, labels or {}, only, keep):
                padded = pad_box(box, pad)
                prims.append((REDACT,) + padded + (tuple(colour), cell_side(padded, cells), flags))
        if draw:
            prims += drawn[k][2]
        out.append((index[k], t, prims))
    return out


def redact_bytes(frames, fps, rate_tag, track_rows, height=0, matrix="601", full_range=False, **options):
    """the whole output stream of `redact` for RGB frames [(h, w, 3) uint8]; options: those of plan()"""
    vh, vw = frames[0].shape[:2]
    width, height = (vw, vh) if not height else (int(height / vh * vw), height)
    head = "YUV4MPEG2 W%d H%d F%s C420" % (width, height, rate_tag) + (" XCOLORRANGE=FULL" if full_range else "")
    out = [head.encode() + b"\n"]
    for i, _, prims in plan(track_rows, fps, len(frames), width, height, **options):
        out.append(b"FRAME\n" + render(frames[i], width, height, prims, matrix, full_range))
    return b"".join(out)
