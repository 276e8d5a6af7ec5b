"""The host side of the `demo` verb (reference scripts/pyannote-face.py:317-413): what is drawn on which output frame, and the
YUV4MPEG2 stream the annotated frames leave in.  The pixels are made on the GPU (csrc/render.hip); DEMO.md states the semantics,
tests/demo_ref.py restates them in numpy.  Nothing in this module needs a GPU.  The `redact` verb (REDACT.md, tests/redact_ref.py)
plans with build_redaction_plan() and leaves through the same kernel and stream.

    FONT, glyph()        the project's 5 x 7 bitmap font, ASCII 32 .. 126
    PALETTE              26 track colours (golden-angle hue steps through an integer HSV -> RGB)
    YUV_TABLES           the 16.16 RGB -> YUV coefficients per (matrix, full_range)
    build_plan()         track rows, landmark rows, labels, times and shift -> per-frame primitive lists
    build_redaction_plan()   track rows, labels and a selection -> per-frame lists of redaction primitives
    pack_primitives()    those lists -> the CSR arrays pvf_render_batch / pvf_egress_submit take
    Y4mWriter            `YUV4MPEG2 W H F C420` to a path or to stdout
"""
import sys
from fractions import Fraction
import numpy as np

PRIM_RECT, PRIM_LINE, PRIM_TEXT, PRIM_REDACT = 0, 1, 2, 3
REDACT_ELLIPSE = 1                                    # flags bit 0 (PVF_REDACT_ELLIPSE): the ellipse inscribed in the box
REDACT_MOSAIC, REDACT_SMOOTH, REDACT_FILL = 0, 2, 4   # flags bits 1-2 (PVF_REDACT_*): the mode
REDACT_MODES = {"mosaic": REDACT_MOSAIC, "smooth": REDACT_SMOOTH, "fill": REDACT_FILL}
REDACT_MAX_SIDE = 16384   # PVF_REDACT_MAX_SIDE
REDACT_MAX_COORD = 1 << 20
REDACT_MAX_CELL = 2048
REDACT_MAX_CELLS = 4096   # per redaction
REDACT_MAX_TABLE = 1 << 22   # cells of all the redactions of one call
MAX_PRIMS = 4096          # per frame (PVF_RENDER_MAX_PRIMS)
MAX_TEXT_RUN = 64         # bytes per text primitive (PVF_RENDER_MAX_RUN): longer labels are cut
MAX_TEXT_BYTES = 1 << 20  # per call (PVF_RENDER_MAX_TEXT)
TEXT_COLOUR = (255, 0, 0)

# One glyph = 7 rows, top first; a row = 5 bits, bit 4 the leftmost column.  Typed in for this project from memory of the common
# 5 x 7 dot-matrix letter shapes (the style of character LCD modules); it is not copied from a file and not OpenCV's Hershey font.
_GLYPHS = {
    ' ': (0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00), '!': (0x04, 0x04, 0x04, 0x04, 0x04, 0x00, 0x04),
    '"': (0x0A, 0x0A, 0x0A, 0x00, 0x00, 0x00, 0x00), '#': (0x0A, 0x0A, 0x1F, 0x0A, 0x1F, 0x0A, 0x0A),
    '$': (0x04, 0x0F, 0x14, 0x0E, 0x05, 0x1E, 0x04), '%': (0x18, 0x19, 0x02, 0x04, 0x08, 0x13, 0x03),
    '&': (0x0C, 0x12, 0x14, 0x08, 0x15, 0x12, 0x0D), "'": (0x04, 0x04, 0x08, 0x00, 0x00, 0x00, 0x00),
    '(': (0x02, 0x04, 0x08, 0x08, 0x08, 0x04, 0x02), ')': (0x08, 0x04, 0x02, 0x02, 0x02, 0x04, 0x08),
    '*': (0x00, 0x04, 0x15, 0x0E, 0x15, 0x04, 0x00), '+': (0x00, 0x04, 0x04, 0x1F, 0x04, 0x04, 0x00),
    ',': (0x00, 0x00, 0x00, 0x00, 0x0C, 0x04, 0x08), '-': (0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00),
    '.': (0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C), '/': (0x00, 0x01, 0x02, 0x04, 0x08, 0x10, 0x00),
    '0': (0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E), '1': (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E),
    '2': (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F), '3': (0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E),
    '4': (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02), '5': (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),
    '6': (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E), '7': (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08),
    '8': (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E), '9': (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C),
    ':': (0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x0C, 0x00), ';': (0x00, 0x0C, 0x0C, 0x00, 0x0C, 0x04, 0x08),
    '<': (0x02, 0x04, 0x08, 0x10, 0x08, 0x04, 0x02), '=': (0x00, 0x00, 0x1F, 0x00, 0x1F, 0x00, 0x00),
    '>': (0x08, 0x04, 0x02, 0x01, 0x02, 0x04, 0x08), '?': (0x0E, 0x11, 0x01, 0x02, 0x04, 0x00, 0x04),
    '@': (0x0E, 0x11, 0x01, 0x0D, 0x15, 0x15, 0x0E), 'A': (0x0E, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11),
    'B': (0x1E, 0x11, 0x11, 0x1E, 0x11, 0x11, 0x1E), 'C': (0x0E, 0x11, 0x10, 0x10, 0x10, 0x11, 0x0E),
    'D': (0x1C, 0x12, 0x11, 0x11, 0x11, 0x12, 0x1C), 'E': (0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x1F),
    'F': (0x1F, 0x10, 0x10, 0x1E, 0x10, 0x10, 0x10), 'G': (0x0E, 0x11, 0x10, 0x17, 0x11, 0x11, 0x0F),
    'H': (0x11, 0x11, 0x11, 0x1F, 0x11, 0x11, 0x11), 'I': (0x0E, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E),
    'J': (0x07, 0x02, 0x02, 0x02, 0x02, 0x12, 0x0C), 'K': (0x11, 0x12, 0x14, 0x18, 0x14, 0x12, 0x11),
    'L': (0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x1F), 'M': (0x11, 0x1B, 0x15, 0x15, 0x11, 0x11, 0x11),
    'N': (0x11, 0x11, 0x19, 0x15, 0x13, 0x11, 0x11), 'O': (0x0E, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E),
    'P': (0x1E, 0x11, 0x11, 0x1E, 0x10, 0x10, 0x10), 'Q': (0x0E, 0x11, 0x11, 0x11, 0x15, 0x12, 0x0D),
    'R': (0x1E, 0x11, 0x11, 0x1E, 0x14, 0x12, 0x11), 'S': (0x0F, 0x10, 0x10, 0x0E, 0x01, 0x01, 0x1E),
    'T': (0x1F, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04), 'U': (0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0E),
    'V': (0x11, 0x11, 0x11, 0x11, 0x11, 0x0A, 0x04), 'W': (0x11, 0x11, 0x11, 0x15, 0x15, 0x15, 0x0A),
    'X': (0x11, 0x11, 0x0A, 0x04, 0x0A, 0x11, 0x11), 'Y': (0x11, 0x11, 0x11, 0x0A, 0x04, 0x04, 0x04),
    'Z': (0x1F, 0x01, 0x02, 0x04, 0x08, 0x10, 0x1F), '[': (0x0E, 0x08, 0x08, 0x08, 0x08, 0x08, 0x0E),
    '\\': (0x00, 0x10, 0x08, 0x04, 0x02, 0x01, 0x00), ']': (0x0E, 0x02, 0x02, 0x02, 0x02, 0x02, 0x0E),
    '^': (0x04, 0x0A, 0x11, 0x00, 0x00, 0x00, 0x00), '_': (0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x1F),
    '`': (0x08, 0x04, 0x02, 0x00, 0x00, 0x00, 0x00), 'a': (0x00, 0x00, 0x0E, 0x01, 0x0F, 0x11, 0x0F),
    'b': (0x10, 0x10, 0x16, 0x19, 0x11, 0x11, 0x1E), 'c': (0x00, 0x00, 0x0E, 0x10, 0x10, 0x11, 0x0E),
    'd': (0x01, 0x01, 0x0D, 0x13, 0x11, 0x11, 0x0F), 'e': (0x00, 0x00, 0x0E, 0x11, 0x1F, 0x10, 0x0E),
    'f': (0x06, 0x09, 0x08, 0x1C, 0x08, 0x08, 0x08), 'g': (0x00, 0x0F, 0x11, 0x11, 0x0F, 0x01, 0x0E),
    'h': (0x10, 0x10, 0x16, 0x19, 0x11, 0x11, 0x11), 'i': (0x04, 0x00, 0x0C, 0x04, 0x04, 0x04, 0x0E),
    'j': (0x02, 0x00, 0x06, 0x02, 0x02, 0x12, 0x0C), 'k': (0x10, 0x10, 0x12, 0x14, 0x18, 0x14, 0x12),
    'l': (0x0C, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0E), 'm': (0x00, 0x00, 0x1A, 0x15, 0x15, 0x11, 0x11),
    'n': (0x00, 0x00, 0x16, 0x19, 0x11, 0x11, 0x11), 'o': (0x00, 0x00, 0x0E, 0x11, 0x11, 0x11, 0x0E),
    'p': (0x00, 0x00, 0x1E, 0x11, 0x1E, 0x10, 0x10), 'q': (0x00, 0x00, 0x0D, 0x13, 0x0F, 0x01, 0x01),
    'r': (0x00, 0x00, 0x16, 0x19, 0x10, 0x10, 0x10), 's': (0x00, 0x00, 0x0E, 0x10, 0x0E, 0x01, 0x1E),
    't': (0x08, 0x08, 0x1C, 0x08, 0x08, 0x09, 0x06), 'u': (0x00, 0x00, 0x11, 0x11, 0x11, 0x13, 0x0D),
    'v': (0x00, 0x00, 0x11, 0x11, 0x11, 0x0A, 0x04), 'w': (0x00, 0x00, 0x11, 0x11, 0x15, 0x15, 0x0A),
    'x': (0x00, 0x00, 0x11, 0x0A, 0x04, 0x0A, 0x11), 'y': (0x00, 0x00, 0x11, 0x11, 0x0F, 0x01, 0x0E),
    'z': (0x00, 0x00, 0x1F, 0x02, 0x04, 0x08, 0x1F), '{': (0x02, 0x04, 0x04, 0x08, 0x04, 0x04, 0x02),
    '|': (0x04, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04), '}': (0x08, 0x04, 0x04, 0x02, 0x04, 0x04, 0x08),
    '~': (0x00, 0x00, 0x08, 0x15, 0x02, 0x00, 0x00),
}
FONT = tuple(_GLYPHS[chr(c)] for c in range(32, 127))       # FONT[byte - 32][row]


def glyph(byte):
    """the 7 rows of a byte's glyph; bytes outside 32 .. 126 draw `?`"""
    return FONT[byte - 32] if 32 <= byte <= 126 else FONT[ord('?') - 32]


def hsv_to_rgb(h, s, v):
    """integer HSV -> RGB: h in degrees 0 .. 359, s and v 0 .. 255; `//` floors (DEMO.md, "Palette")"""
    sector, f = h // 60, h % 60
    p = v * (255 - s) // 255
    q = v * (255 * 60 - s * f) // (255 * 60)
    t = v * (255 * 60 - s * (60 - f)) // (255 * 60)
    return ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))[sector]


PALETTE = tuple(hsv_to_rgb((i * 137) % 360, 255, 255 - 51 * (i % 3)) for i in range(26))

# (yoff, (yr, yg, yb), (ur, ug, ub), (vr, vg, vb)) per (matrix, full_range): round(c * 65536), and the rounding residual of a chroma row
# taken off its green coefficient so that the row sums to zero (DEMO.md, "Colour conversion")
YUV_TABLES = {
    ("601", False): (16, (16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681)),
    ("601", True): (0, (19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329)),
    ("709", False): (16, (11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639)),
    ("709", True): (0, (13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005)),
}


def text_scale(height):
    return max(1, (int(height) + 100) // 200)


def demo_size(video_width, video_height, height):
    """(width, height) of the output frames (pyannote-face.py:330-333)"""
    return int(height / video_height * video_width), int(height)


def _text(x, y, colour, scale, s):
    b = s if isinstance(s, bytes) else str(s).encode("utf-8")
    return (PRIM_TEXT, int(x), int(y), tuple(colour), int(scale), b[:MAX_TEXT_RUN])


def _paced(groups, times):
    """{index into times: group} by the pacing of the reference's generators (pyannote-face.py:159-172, :220-233): one group per
    time at most, in order, a group waiting until the time has reached its own"""
    out, gi = {}, 0
    for k, t in enumerate(times):
        if gi >= len(groups):
            break
        if groups[gi][0] > t:
            continue
        out[k] = groups[gi]
        gi += 1
    return out


def landmark_groups(rows, width, height):
    """getLandmarkGenerator's groups (pyannote-face.py:184-236): consecutive rows of one time, in FILE order, the last group never
    emitted; points are np.round(x * width) on float32.  rows: formats.read_landmarks"""
    groups = []
    for T, ident, pts in rows:
        p = np.array(pts, np.float32)
        p[:, 0] = np.round(p[:, 0] * width)
        p[:, 1] = np.round(p[:, 1] * height)
        if groups and groups[-1][0] == T:
            groups[-1][1].append((ident, p))
        else:
            groups.append((T, [(ident, p)]))
    return groups[:-1]


def plan_times(frame_rate, n_frames, t_from=0.0, t_until=None):
    """(times, source frame indices) of the output frames: frame k has t = t_from + k / frame_rate while t < t_until (default: the
    video's duration) and shows source frame int(frame_rate * t + 1e-5) (video.py:466-486); the output ends where the video does"""
    frame_rate = float(frame_rate)
    if t_until is None:
        t_until = n_frames / frame_rate
    times, index = [], []
    k = 0
    while True:
        t = t_from + k / frame_rate
        i = int(frame_rate * t + 0.00001)
        if not t < t_until or i >= n_frames or i < 0:
            break
        times.append(t)
        index.append(i)
        k += 1
    return times, index


def build_plan(track_rows, frame_rate, n_frames, width, height, landmark_rows=None, labels=None, t_from=0.0, t_until=None, shift=0.0):
    """[(source frame index, t, [primitive])] for every output frame: frame k has t = t_from + k / frame_rate while t < t_until (default:
    the video's duration, n_frames / frame_rate) and shows source frame int(frame_rate * t + 1e-5) (video.py:466-486); the output ends
    where the video does.  Faces are what getFaceGenerator yields for t - shift (pipeline.faces_per_frame), landmarks what
    getLandmarkGenerator yields, paired with the faces BY IDENTIFIER (DEMO.md, "Departures").  Primitives:
        (PRIM_RECT, l, t, r, b, colour)   (PRIM_LINE, x1, y1, x2, y2, colour)   (PRIM_TEXT, x, y, colour, scale, bytes)"""
    from .pipeline import faces_per_frame
    times, index = plan_times(frame_rate, n_frames, t_from, t_until)
    sent = [t - shift for t in times]
    faces = {k: g for k, _, g in faces_per_frame(track_rows, sent, width, height)}
    marks = _paced(landmark_groups(landmark_rows, width, height), sent) if landmark_rows is not None else None
    labels = labels or {}
    scale = text_scale(height)
    plan = []
    for k, t in enumerate(times):
        prims = [_text(10, height - 10, TEXT_COLOUR, scale, '%.3f' % t)]
        by_id = {}
        if marks is not None and k in marks:
            for ident, p in marks[k][1]:
                by_id.setdefault(ident, p)
        for ident, (left, top, right, bottom) in faces.get(k, ()):
            colour = PALETTE[ident % len(PALETTE)]
            prims.append((PRIM_RECT, left, top, right, bottom, colour))
            prims.append(_text(left, bottom + 15, TEXT_COLOUR, scale, '#%d' % ident))
            label = labels.get(ident, '')
            if label:
                prims.append(_text(left, top - 7, TEXT_COLOUR, scale, label))
            p = by_id.get(ident)
            if p is not None and len(p) > 33:
                prims.append((PRIM_LINE, int(p[27, 0]), int(p[27, 1]), int(p[33, 0]), int(p[33, 1]), colour))
        plan.append((index[k], t, prims))
    return plan


def redaction_box(box, pad=25):
    """the box a face's redaction covers: ((r - l) * pad + 50) // 100 more on the left and on the right, `pad` an integer per cent, and
    the same rule with b - t above and below (REDACT.md "The verb")"""
    l, t, r, b = (int(v) for v in box)
    dx, dy = ((r - l) * pad + 50) // 100, ((b - t) * pad + 50) // 100
    return l - dx, t - dy, r + dx, b + dy


def redaction_cell(box, cells=8):
    """the cell side for `cells` cells along the longer side of the (padded) box: max(1, ceil(max(W, H) / cells)), at most
    REDACT_MAX_CELL, raised as far as REDACT_MAX_CELLS asks"""
    W, H = max(1, box[2] - box[0] + 1), max(1, box[3] - box[1] + 1)
    cell = min(REDACT_MAX_CELL, max(1, -(-max(W, H) // int(cells))))
    while (-(-W // cell)) * (-(-H // cell)) > REDACT_MAX_CELLS:
        cell += 1
    return cell


def redaction_cells(p):
    """cells in the table of a (PRIM_REDACT, ...) primitive: 0 for an inverted box and for a fill"""
    W, H = p[3] - p[1] + 1, p[4] - p[2] + 1
    if W < 1 or H < 1 or (p[7] & 6) == REDACT_FILL:
        return 0
    return (-(-W // p[6])) * (-(-H // p[6]))


def _check_redaction(p):
    """the limits of REDACT.md, as the library checks them (render_launch)"""
    _, l, t, r, b, colour, cell, flags = p
    for v in (l, t, r, b):
        if not -REDACT_MAX_COORD <= int(v) <= REDACT_MAX_COORD:
            raise ValueError("redaction coordinate %r beyond +-%d" % (v, REDACT_MAX_COORD))
    if int(flags) & ~7 or (int(flags) & 6) == 6:
        raise ValueError("unknown redaction flags %r" % (flags,))
    if not 1 <= int(cell) <= REDACT_MAX_CELL:
        raise ValueError("redaction cell %r outside 1 .. %d" % (cell, REDACT_MAX_CELL))
    W, H = int(r) - int(l) + 1, int(b) - int(t) + 1
    if W < 1 or H < 1:
        return
    if W > REDACT_MAX_SIDE or H > REDACT_MAX_SIDE:
        raise ValueError("a redaction of %d x %d pixels (a side is at most %d)" % (W, H, REDACT_MAX_SIDE))
    n = (-(-W // int(cell))) * (-(-H // int(cell)))
    if n > REDACT_MAX_CELLS:
        raise ValueError("a redaction of %d cells (at most %d)" % (n, REDACT_MAX_CELLS))


def build_redaction_plan(track_rows, frame_rate, n_frames, width, height, labels=None, only=None, keep=None, pad=25, cells=8,
                         shape="ellipse", mode="mosaic", colour=(0, 0, 0), t_from=0.0, t_until=None, shift=0.0):
    """[(source frame index, t, [primitive])] as build_plan gives them, the primitives being the redactions of the chosen tracks:
        (PRIM_REDACT, l, t, r, b, colour, cell, flags)
    Faces are pipeline.faces_per_frame(..., drop_last=False): the LAST time's faces are there too (the reference's generator never emits
    them, and `demo` follows it; here that would leave a face visible).  Neither `only` nor `keep`: every track; only={names}: the tracks
    whose label is in the set; keep={names}: every track whose label is NOT in the set, tracks without a label included (the safe side).
    Both, or either without `labels`, is a ValueError.  The box is padded by redaction_box, the cell chosen by redaction_cell."""
    from .pipeline import faces_per_frame
    if only is not None and keep is not None:
        raise ValueError("only and keep exclude each other")
    if (only is not None or keep is not None) and labels is None:
        raise ValueError("only / keep select by label: they need labels")
    if shape not in ("ellipse", "box"):
        raise ValueError("shape is 'ellipse' or 'box', not %r" % (shape,))
    if mode not in REDACT_MODES:
        raise ValueError("mode is one of %s, not %r" % (", ".join(sorted(REDACT_MODES)), mode))
    flags = REDACT_MODES[mode] | (REDACT_ELLIPSE if shape == "ellipse" else 0)
    colour = tuple(int(v) for v in colour)
    only = None if only is None else set(only)
    keep = None if keep is None else set(keep)

    def chosen(ident):
        if only is not None:
            return ident in labels and labels[ident] in only
        if keep is not None:
            return not (ident in labels and labels[ident] in keep)
        return True
    times, index = plan_times(frame_rate, n_frames, t_from, t_until)
    faces = {k: g for k, _, g in faces_per_frame(track_rows, [t - shift for t in times], width, height, drop_last=False)}
    plan = []
    for k, t in enumerate(times):
        prims = []
        for ident, box in faces.get(k, ()):
            if chosen(ident):
                padded = redaction_box(box, pad)
                prims.append((PRIM_REDACT,) + padded + (colour, redaction_cell(padded, cells), flags))
        plan.append((index[k], t, prims))
    return plan


def pack_primitives(lists):
    """per-frame primitive lists -> (start int32 [n + 1], prims int32 [N, 8], text uint8 [T]): the CSR form of the C ABI.  A row is
    (type, a, b, c, d, colour = r | g << 8 | b << 16, scale, 0); text: a, b = x, y; c, d = offset into the pool and length; a
    redaction (PRIM_REDACT, l, t, r, b, colour, cell, flags): colour | flags << 24, scale = cell."""
    start, rows, pool = [0], [], bytearray()
    table = 0
    for prims in lists:
        if len(prims) > MAX_PRIMS:
            raise ValueError("%d primitives on one frame (at most %d)" % (len(prims), MAX_PRIMS))
        for p in prims:
            if p[0] == PRIM_TEXT:
                _, x, y, colour, scale, b = p
                if len(b) > MAX_TEXT_RUN:
                    raise ValueError("a text run of %d bytes (at most %d)" % (len(b), MAX_TEXT_RUN))
                a = (x, y, len(pool), len(b))
                pool += b
            elif p[0] == PRIM_REDACT:
                _check_redaction(p)
                table += redaction_cells(p)
                if table > REDACT_MAX_TABLE:
                    raise ValueError("more than %d redaction cells in one call" % REDACT_MAX_TABLE)
                colour, scale, a = (p[5][0], p[5][1], p[5][2] | int(p[7]) << 8), int(p[6]), p[1:5]      # the flags land in the top byte
            else:
                colour, scale, a = p[5], 0, p[1:5]
            for v in a:
                if not -(1 << 31) <= int(v) < (1 << 31):
                    raise ValueError("coordinate %r does not fit int32" % (v,))
            rows.append((p[0], int(a[0]), int(a[1]), int(a[2]), int(a[3]), colour[0] | colour[1] << 8 | colour[2] << 16, scale, 0))
        start.append(len(rows))
    prims = np.array(rows, np.int64).astype(np.int32).reshape(-1, 8)
    return np.array(start, np.int32), np.ascontiguousarray(prims), np.frombuffer(bytes(pool), np.uint8).copy()


def read_labels(path):
    """`identifier label` lines (what `cluster` writes; pyannote-face.py:391-397) -> {identifier: label}"""
    labels = {}
    with open(path) as f:
        for number, line in enumerate(f, 1):
            p = line.strip().split()
            if not p:
                continue
            if len(p) != 2:
                raise ValueError("%s:%d: expected `identifier label`, found %r" % (path, number, line.rstrip("\n")))
            labels[int(p[0])] = p[1]
    return labels


def rate_tag(video, fps):
    """the F tag: a Y4M source's own, else a rational of the frame rate"""
    tag = getattr(video, "rate_tag", None)
    if tag:
        return tag
    fr = Fraction(float(fps)).limit_denominator(1001)
    return "%d:%d" % (fr.numerator, fr.denominator)


class Y4mWriter(object):
    """`YUV4MPEG2 W<w> H<h> F<num>:<den> C420` (+ ` XCOLORRANGE=FULL`), then `FRAME\\n` + Y, U, V per frame.  target: a path, or `-` for
    stdout (`... demo film.y4m track.txt - | ffmpeg -i - out.mp4`)."""

    def __init__(self, target, width, height, rate="25:1", full_range=False):
        self.width, self.height = int(width), int(height)
        self.frame_bytes = self.width * self.height + 2 * ((self.width + 1) // 2) * ((self.height + 1) // 2)
        if hasattr(target, "write"):             # an object to write to (tube.PooledFile): closed with the writer
            self._own, self._f = True, target
        else:
            self._own = target != "-"
            self._f = open(target, "wb") if self._own else sys.stdout.buffer
        self.frames = 0
        head = "YUV4MPEG2 W%d H%d F%s C420" % (self.width, self.height, rate)
        if full_range:
            head += " XCOLORRANGE=FULL"
        self._f.write(head.encode("ascii") + b"\n")

    def write(self, planes):
        """planes: the frame_bytes of one frame (Y, U, V, tight), any buffer"""
        m = memoryview(planes).cast("B")
        if len(m) != self.frame_bytes:
            raise ValueError("a %dx%d frame has %d bytes, not %d" % (self.width, self.height, self.frame_bytes, len(m)))
        self._f.write(b"FRAME\n")
        self._f.write(m)
        self.frames += 1

    def close(self):
        if self._f is not None:
            self._f.flush()
            if self._own:
                self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
