"""DEMO.md restated in numpy, independent of the package: resize, primitives, font, palette, colour conversion, the pacing of faces
and landmarks, and the bytes of the Y4M stream the `demo` verb writes.  Everything is integer arithmetic (Python ints where a
product may pass 64 bits), so the GPU is held to it bit for bit."""
import numpy as np

RECT, LINE, TEXT = 0, 1, 2
MAX_RUN = 64
RED = (255, 0, 0)

# 95 glyphs, ASCII 32 .. 126; 7 rows from the top, 5 bits a row, bit 4 leftmost (DEMO.md "Text")
FONT = [
    (0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00), (0x04, 0x04, 0x04, 0x04, 0x04, 0x00, 0x04), (0x0A, 0x0A, 0x0A, 0x00, 0x00, 0x00, 0x00),
    (0x0A, 0x0A, 0x1F, 0x0A, 0x1F, 0x0A, 0x0A), (0x04, 0x0F, 0x14, 0x0E, 0x05, 0x1E, 0x04), (0x18, 0x19, 0x02, 0x04, 0x08, 0x13, 0x03),
    (0x0C, 0x12, 0x14, 0x08, 0x15, 0x12, 0x0D), (0x04, 0x04, 0x08, 0x00, 0x00, 0x00, 0x00), (0x02, 0x04, 0x08, 0x08, 0x08, 0x04, 0x02),
    (0x08, 0x04, 0x02, 0x02, 0x02, 0x04, 0x08), (0x00, 0x04, 0x15, 0x0E, 0x15, 0x04, 0x00), (0x00, 0x04, 0x04, 0x1F, 0x04, 0x04, 0x00),
    (0x00, 0x00, 0x00, 0x00, 0x0C, 0x04, 0x08), (0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00), (0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C),
    (0x00, 0x01, 0x02, 0x04, 0x08, 0x10, 0x00), (0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E), (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E),
    (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F), (0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E), (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02),
    (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E), (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E), (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08),
    (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E), (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C), (0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x0C, 0x00),
    (0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x04, 0x08), (0x02, 0x04, 0x08, 0x10, 0x08, 0x04, 0x02), (0x00, 0x00, 0x1F, 0x00, 0x1F, 0x00, 0x00),
    (0x08, 0x04, 0x02, 0x01, 0x02, 0x04, 0x08), (0x0E, 0x11, 0x01, 0x02, 0x04, 0x00, 0x04), (0x0E, 0x11, 0x01, 0x0D, 0x15, 0x15, 0x0E),
    (0x0E, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11), (0x1E, 0x11, 0x11, 0x1E, 0x11, 0x11, 0x1E), (0x0E, 0x11, 0x10, 0x10, 0x10, 0x11, 0x0E),
    (0x1C, 0x12, 0x11, 0x11, 0x11, 0x12, 0x1C), (0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x1F), (0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x10),
    (0x0E, 0x11, 0x10, 0x17, 0x11, 0x11, 0x0F), (0x11, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11), (0x0E, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E),
    (0x07, 0x02, 0x02, 0x02, 0x02, 0x12, 0x0C), (0x11, 0x12, 0x14, 0x18, 0x14, 0x12, 0x11), (0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x1F),
    (0x11, 0x1B, 0x15, 0x15, 0x11, 0x11, 0x11), (0x11, 0x11, 0x19, 0x15, 0x13, 0x11, 0x11), (0x0E, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E),
    (0x1E, 0x11, 0x11, 0x1E, 0x10, 0x10, 0x10), (0x0E, 0x11, 0x11, 0x11, 0x15, 0x12, 0x0D), (0x1E, 0x11, 0x11, 0x1E, 0x14, 0x12, 0x11),
    (0x0F, 0x10, 0x10, 0x0E, 0x01, 0x01, 0x1E), (0x1F, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04), (0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E),
    (0x11, 0x11, 0x11, 0x11, 0x11, 0x0A, 0x04), (0x11, 0x11, 0x11, 0x15, 0x15, 0x15, 0x0A), (0x11, 0x11, 0x0A, 0x04, 0x0A, 0x11, 0x11),
    (0x11, 0x11, 0x11, 0x0A, 0x04, 0x04, 0x04), (0x1F, 0x01, 0x02, 0x04, 0x08, 0x10, 0x1F), (0x0E, 0x08, 0x08, 0x08, 0x08, 0x08, 0x0E),
    (0x00, 0x10, 0x08, 0x04, 0x02, 0x01, 0x00), (0x0E, 0x02, 0x02, 0x02, 0x02, 0x02, 0x0E), (0x04, 0x0A, 0x11, 0x00, 0x00, 0x00, 0x00),
    (0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x1F), (0x08, 0x04, 0x02, 0x00, 0x00, 0x00, 0x00), (0x00, 0x00, 0x0E, 0x01, 0x0F, 0x11, 0x0F),
    (0x10, 0x10, 0x16, 0x19, 0x11, 0x11, 0x1E), (0x00, 0x00, 0x0E, 0x10, 0x10, 0x11, 0x0E), (0x01, 0x01, 0x0D, 0x13, 0x11, 0x11, 0x0F),
    (0x00, 0x00, 0x0E, 0x11, 0x1F, 0x10, 0x0E), (0x06, 0x09, 0x08, 0x1C, 0x08, 0x08, 0x08), (0x00, 0x0F, 0x11, 0x11, 0x0F, 0x01, 0x0E),
    (0x10, 0x10, 0x16, 0x19, 0x11, 0x11, 0x11), (0x04, 0x00, 0x0C, 0x04, 0x04, 0x04, 0x0E), (0x02, 0x00, 0x06, 0x02, 0x02, 0x12, 0x0C),
    (0x10, 0x10, 0x12, 0x14, 0x18, 0x14, 0x12), (0x0C, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E), (0x00, 0x00, 0x1A, 0x15, 0x15, 0x11, 0x11),
    (0x00, 0x00, 0x16, 0x19, 0x11, 0x11, 0x11), (0x00, 0x00, 0x0E, 0x11, 0x11, 0x11, 0x0E), (0x00, 0x00, 0x1E, 0x11, 0x1E, 0x10, 0x10),
    (0x00, 0x00, 0x0D, 0x13, 0x0F, 0x01, 0x01), (0x00, 0x00, 0x16, 0x19, 0x10, 0x10, 0x10), (0x00, 0x00, 0x0E, 0x10, 0x0E, 0x01, 0x1E),
    (0x08, 0x08, 0x1C, 0x08, 0x08, 0x09, 0x06), (0x00, 0x00, 0x11, 0x11, 0x11, 0x13, 0x0D), (0x00, 0x00, 0x11, 0x11, 0x11, 0x0A, 0x04),
    (0x00, 0x00, 0x11, 0x11, 0x15, 0x15, 0x0A), (0x00, 0x00, 0x11, 0x0A, 0x04, 0x0A, 0x11), (0x00, 0x00, 0x11, 0x11, 0x0F, 0x01, 0x0E),
    (0x00, 0x00, 0x1F, 0x02, 0x04, 0x08, 0x1F), (0x02, 0x04, 0x04, 0x08, 0x04, 0x04, 0x02), (0x04, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04),
    (0x08, 0x04, 0x04, 0x02, 0x04, 0x04, 0x08), (0x00, 0x00, 0x08, 0x15, 0x02, 0x00, 0x00),
]

# (yoff, Y row, U row, V row) by (matrix, full_range)
TABLES = {
    ("601", False): (16, (16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681)),
    ("601", True): (0, (19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329)),
    ("709", False): (16, (11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639)),
    ("709", True): (0, (13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005)),
}
LUMA = {"601": (0.299, 0.114), "709": (0.2126, 0.0722)}      # (Kr, Kb)


def derive_table(matrix, full_range):
    """the rule the tables are built by (DEMO.md): round(c * 65536), a chroma row's rounding residual taken off its green coefficient"""
    kr, kb = LUMA[matrix]
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    r = lambda v: int(round(v * 65536))
    y = (r(kr * ys), r(kg * ys), r(kb * ys))
    u = [r(-kr / (2 * (1 - kb)) * cs), r(-kg / (2 * (1 - kb)) * cs), r(0.5 * cs)]
    v = [r(0.5 * cs), r(-kg / (2 * (1 - kr)) * cs), r(-kb / (2 * (1 - kr)) * cs)]
    u[1] -= sum(u)
    v[1] -= sum(v)
    return (0 if full_range else 16, y, tuple(u), tuple(v))


def hsv_to_rgb(h, s, v):
    sector, f = h // 60, h % 60
    p = v * (255 - s) // 255
    q = v * (255 * 60 - s * f) // (255 * 60)
    t = v * (255 * 60 - s * (60 - f)) // (255 * 60)
    return [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)][sector]


PALETTE = [hsv_to_rgb((i * 137) % 360, 255, 255 - 51 * (i % 3)) for i in range(26)]


# ---- resize: OpenCV's 8-bit INTER_LINEAR ------------------------------------------------------------------------------------------
def _table(n_in, n_out):
    scale = float(n_in) / n_out
    f = ((np.arange(n_out) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    lo, hi = s < 0, s >= n_in - 1
    f[lo | hi] = 0
    s[lo] = 0
    s[hi] = n_in - 1
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, n_in - 1), c0, c1


def resize(img, ow, oh):
    ih, iw = img.shape[:2]
    x0, x1, a0, a1 = _table(iw, ow)
    y0, y1, b0, b1 = _table(ih, oh)
    src = img.astype(np.int64)
    S0 = src[y0][:, x0] * a0[None, :, None] + src[y0][:, x1] * a1[None, :, None]
    S1 = src[y1][:, x0] * a0[None, :, None] + src[y1][:, x1] * a1[None, :, None]
    out = (((b0[:, None, None] * (S0 >> 4)) >> 16) + ((b1[:, None, None] * (S1 >> 4)) >> 16) + 2) >> 2
    return (out & 255).astype(np.uint8)


# ---- primitives -------------------------------------------------------------------------------------------------------------------
def rect_pixels(l, t, r, b, w, h):
    """set of (x, y) inside the frame"""
    out = set()
    for y in range(max(t - 1, 0), min(b + 1, h - 1) + 1):
        for x in range(max(l - 1, 0), min(r + 1, w - 1) + 1):
            if not (l + 1 <= x <= r - 1 and t + 1 <= y <= b - 1):
                out.add((x, y))
    return out


def draw_rect(img, l, t, r, b, colour):
    h, w = img.shape[:2]
    xa, xb, ya, yb = max(l - 1, 0), min(r + 1, w - 1), max(t - 1, 0), min(b + 1, h - 1)
    if xa > xb or ya > yb:
        return
    ys, xs = np.mgrid[ya:yb + 1, xa:xb + 1]
    inner = (xs >= l + 1) & (xs <= r - 1) & (ys >= t + 1) & (ys <= b - 1)
    img[ya:yb + 1, xa:xb + 1][~inner] = colour


def line_pixels(x1, y1, x2, y2, w=None, h=None, ties_down=False):
    """the line's pixels in step order, those outside a w x h frame left out (w None: all of them -- short lines only).
    ties_down: an exact half step rounds down (what drawing from the other end amounts to)"""
    dx, dy = x2 - x1, y2 - y1
    xmajor = abs(dx) >= abs(dy)
    D, d = (abs(dx), abs(dy)) if xmajor else (abs(dy), abs(dx))
    M1, m1 = (x1, y1) if xmajor else (y1, x1)
    sM = 1 if (dx if xmajor else dy) >= 0 else -1
    sm = 1 if (dy if xmajor else dx) >= 0 else -1
    k0, k1 = 0, D
    if w is not None:                                 # the steps whose major coordinate lies in the frame
        lim = w if xmajor else h
        a, b = (0 - M1) * sM, (lim - 1 - M1) * sM
        k0, k1 = max(k0, min(a, b)), min(k1, max(a, b))
    out = []
    for k in range(k0, k1 + 1):                       # Python ints: 2 k d passes 64 bits for far endpoints
        step = 0 if D == 0 else ((2 * k * d + D - (1 if ties_down else 0)) // (2 * D))
        M, m = M1 + sM * k, m1 + sm * step
        x, y = (M, m) if xmajor else (m, M)
        if w is None or (0 <= x < w and 0 <= y < h):
            out.append((x, y))
    return out


def draw_line(img, x1, y1, x2, y2, colour):
    h, w = img.shape[:2]
    for x, y in line_pixels(x1, y1, x2, y2, w, h):
        img[y, x] = colour


def draw_text(img, x, y, colour, scale, data):
    h, w = img.shape[:2]
    s = scale
    for i, ch in enumerate(bytes(data)):
        g = FONT[ch - 32] if 32 <= ch <= 126 else FONT[ord('?') - 32]
        gx = x + 6 * i * s
        if gx >= w or gx + 5 * s <= 0:
            continue
        for r in range(7):
            ya, yb = y - (7 - r) * s + 1, y - (6 - r) * s
            if yb < 0 or ya >= h:
                continue
            for c in range(5):
                if (g[r] >> (4 - c)) & 1:
                    xa = gx + c * s
                    if xa + s > 0 and xa < w:
                        img[max(ya, 0):max(yb + 1, 0), max(xa, 0):max(xa + s, 0)] = colour


def draw(img, prims):
    """in list order, later over earlier.  (RECT, l, t, r, b, colour) (LINE, x1, y1, x2, y2, colour) (TEXT, x, y, colour, scale, bytes)"""
    for p in prims:
        if p[0] == RECT:
            draw_rect(img, p[1], p[2], p[3], p[4], p[5])
        elif p[0] == LINE:
            draw_line(img, p[1], p[2], p[3], p[4], p[5])
        else:
            draw_text(img, p[1], p[2], p[3], p[4], p[5][:MAX_RUN])
    return img


# ---- colour -----------------------------------------------------------------------------------------------------------------------
def to_yuv420(rgb, matrix="601", full_range=False):
    """(Y [h, w], U, V [ceil(h / 2), ceil(w / 2)]) uint8"""
    yoff, yc, uc, vc = TABLES[(str(matrix), bool(full_range))]
    p = rgb.astype(np.int64)
    Y = (yc[0] * p[..., 0] + yc[1] * p[..., 1] + yc[2] * p[..., 2] + (yoff << 16) + 32768) >> 16
    h, w = Y.shape
    q = np.pad(p, ((0, h & 1), (0, w & 1), (0, 0)), mode="edge")
    S = q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2]
    U = (uc[0] * S[..., 0] + uc[1] * S[..., 1] + uc[2] * S[..., 2] + (128 << 18) + (1 << 17)) >> 18
    V = (vc[0] * S[..., 0] + vc[1] * S[..., 1] + vc[2] * S[..., 2] + (128 << 18) + (1 << 17)) >> 18
    return tuple(np.clip(a, 0, 255).astype(np.uint8) for a in (Y, U, V))


def unclamped_yuv(rgb, matrix, full_range):
    """the three values before the clamp, for one colour repeated over a block (int)"""
    yoff, yc, uc, vc = TABLES[(str(matrix), bool(full_range))]
    r, g, b = (int(v) for v in rgb)
    return ((yc[0] * r + yc[1] * g + yc[2] * b + (yoff << 16) + 32768) >> 16,
            (4 * (uc[0] * r + uc[1] * g + uc[2] * b) + (128 << 18) + (1 << 17)) >> 18,
            (4 * (vc[0] * r + vc[1] * g + vc[2] * b) + (128 << 18) + (1 << 17)) >> 18)


def render_rgb(src, ow, oh, prims):
    return draw(resize(src, ow, oh), prims)


def render(src, ow, oh, prims, matrix="601", full_range=False):
    """the frame's bytes: Y, U, V tight"""
    return b"".join(p.tobytes() for p in to_yuv420(render_rgb(src, ow, oh, prims), matrix, full_range))


# ---- what is drawn when -----------------------------------------------------------------------------------------------------------
def _generator(groups):
    """the pacing both of the reference's generators share (pyannote-face.py:133-175, :195-236), transcribed: it is sent a time and
    answers with a group at most; a group waits until the time has reached its own; the last group is never given out, because a group
    is complete only when the row after it has been read"""
    t = yield
    current, held = None, []
    for T, item in groups:
        if current is None or T == current:
            held.append(item)
            current = T
            continue
        while True:
            if current > t:
                t = yield []
                continue
            t = yield held
            held, current = [item], T
            break
    while True:
        t = yield []


def read_track_file(path):
    """[(T, identifier, (l, t, r, b) float32)] in the order of the reference's sorted table (numpy's default argsort on the times)"""
    rows = []
    for line in open(path):
        p = line.split()
        if p:
            rows.append((float(p[0]), int(p[1]), tuple(np.float32(v) for v in p[2:6])))
    order = np.argsort(np.array([r[0] for r in rows], np.float64), kind="quicksort")
    return [rows[i] for i in order]


def read_landmark_file(path):
    rows = []
    for line in open(path):
        p = line.split()
        if p:
            rows.append((float(p[0]), int(float(p[1])), np.array([float(v) for v in p[2:]]).astype(np.float32).reshape(-1, 2)))
    return rows


def read_label_file(path):
    return {int(p[0]): p[1] for p in (line.split() for line in open(path)) if p}


def plan(track_rows, fps, n_frames, width, height, landmark_rows=None, labels=None, t_from=0.0, t_until=None, shift=0.0):
    """[(source index, t, primitives)] (DEMO.md "What is drawn", "Timing")"""
    fps = float(fps)
    until = n_frames / fps if t_until is None else t_until
    faces = _generator([(T, (ident, tuple(int(float(c) * s) for c, s in zip(box, (width, height, width, height)))))
                        for T, ident, box in track_rows])
    next(faces)
    marks = None
    if landmark_rows is not None:
        items = []
        for T, ident, pts in landmark_rows:
            p = np.array(pts, np.float32)
            p[:, 0] = np.round(p[:, 0] * width)
            p[:, 1] = np.round(p[:, 1] * height)
            items.append((T, (ident, p)))
        marks = _generator(items)
        next(marks)
    labels = labels or {}
    scale = max(1, (height + 100) // 200)
    out, k = [], 0
    while True:
        t = t_from + k / fps
        i = int(fps * t + 0.00001)
        if not t < until or not 0 <= i < n_frames:
            break
        prims = [(TEXT, 10, height - 10, RED, scale, ('%.3f' % t).encode())]
        shown = faces.send(t - shift)
        noses = {}
        if marks is not None:
            for ident, p in marks.send(t - shift):
                noses.setdefault(ident, p)
        for ident, (l, tp, r, b) in shown:
            colour = PALETTE[ident % 26]
            prims.append((RECT, l, tp, r, b, colour))
            prims.append((TEXT, l, b + 15, RED, scale, ('#%d' % ident).encode()))
            if labels.get(ident):
                prims.append((TEXT, l, tp - 7, RED, scale, labels[ident].encode("utf-8")[:MAX_RUN]))
            if ident in noses and len(noses[ident]) > 33:
                p = noses[ident]
                prims.append((LINE, int(p[27, 0]), int(p[27, 1]), int(p[33, 0]), int(p[33, 1]), colour))
        out.append((i, t, prims))
        k += 1
    return out


def demo_bytes(frames, fps, rate_tag, track_rows, height, landmark_rows=None, labels=None, matrix="601", full_range=False,
               t_from=0.0, t_until=None, shift=0.0):
    """the whole output stream of `demo` for RGB frames [(h, w, 3) uint8]"""
    vh, vw = frames[0].shape[:2]
    width = int(height / vh * vw)
    head = "YUV4MPEG2 W%d H%d F%s C420" % (width, height, rate_tag) + (" XCOLORRANGE=FULL" if full_range else "")
    out = [head.encode() + b"\n"]
    for i, _, prims in plan(track_rows, fps, len(frames), width, height, landmark_rows, labels, t_from, t_until, shift):
        out.append(b"FRAME\n" + render(frames[i], width, height, prims, matrix, full_range))
    return b"".join(out)
