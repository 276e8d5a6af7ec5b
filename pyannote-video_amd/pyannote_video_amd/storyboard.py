"""The host side of the `storyboard` verb (STORYBOARD.md): which frames of a shot are shown, how large a thumbnail is and where it
goes on the sheet.  The pixels -- the area average of a whole frame, the copied tiles, the drawing -- are the library's
(csrc/board.hip); what is here is a handful of integers per shot."""
import warnings

from . import render
from .faces import MAX_SIDE, MAX_PIXELS, MAX_TILES

MAX_THUMB = 1024                           # PVF_THUMB_MAX_SIDE
MAX_PER = 8
GAP = 6                                    # between tiles, and around a cell: an outline of 2 pixels and background
BACKGROUND = (24, 24, 24)
NEUTRAL = (200, 200, 200)                  # caption and outline of a cell without --thread
SHEET_WIDTH = 1920                         # what the default --columns fills


def frame_index(fps, t):
    """the frame at time t: int(fps t + 1e-5), the rule of structure.Thread._frame_index"""
    return int(float(fps) * float(t) + 0.00001)


def shot_frames(start, end, fps, n_frames, K):
    """the frames shown for the shot [start, end): a = idx(start), b = max(a, idx(end) - 1) clipped to the film, m = b - a + 1 frames;
    the K picks a + ((2 k + 1) m) // (2 K) are the centres of K equal parts, duplicates dropped.  None: the shot starts past the film."""
    a = frame_index(fps, start)
    if a >= n_frames or a < 0:
        return None
    b = min(max(a, frame_index(fps, end) - 1), n_frames - 1)
    m = b - a + 1
    picks = []
    for k in range(int(K)):
        f = a + ((2 * k + 1) * m) // (2 * int(K))
        if f not in picks:
            picks.append(f)
    return picks


def tile_size(width, w, h):
    """(tw, th): tw = --width, th the frame's aspect rounded half up, at least 1"""
    tw = int(width)
    return tw, max(1, (2 * tw * int(h) + int(w)) // (2 * int(w)))


def text_scale(tw):
    return max(1, int(tw) // 80)


def cell_size(K, tw, th):
    """(width, height) of a cell: a caption line over a row of K tiles"""
    return GAP + int(K) * (int(tw) + GAP), 3 * GAP + 7 * text_scale(tw) + int(th)


def default_columns(K, tw):
    return max(1, SHEET_WIDTH // cell_size(K, tw, 1)[0])


def caption(number, start, label=None):
    """`<shot number> <m:ss.s>`, and the thread label when there is one; the time is the shot's start rounded to tenths"""
    tenths = int(round(float(start) * 10.0))
    text = "%d %d:%02d.%d" % (number, tenths // 600, (tenths % 600) // 10, tenths % 10)
    return text if label is None else text + " " + str(label)


def thread_ranks(labels):
    """{label: rank}: the order of first appearance in `labels` (one per shot, in time order; None is no label)"""
    ranks = {}
    for l in labels:
        if l is not None and l not in ranks:
            ranks[l] = len(ranks)
    return ranks


def shot_labels(shots, annotation):
    """the label of every shot: that of the annotation's first track (in its order) whose segment holds the shot's middle -- `thread`
    merges touching shots of one thread into one segment -- else None"""
    if annotation is None:
        return [None] * len(shots)
    tracks = [(segment.start, segment.end, label) for segment, _, label in annotation.itertracks(yield_label=True)]
    out = []
    for s in shots:
        mid = (float(s.start) + float(s.end)) / 2.0
        out.append(next((l for a, b, l in tracks if a <= mid < b), None))
    return out


def sheet_order(cells, by):
    """cells: [(number, start, label)] in time order -> [(cell index, starts a new row)] in sheet order.  `time`: as they come.
    `thread`: by (rank of the label's first appearance, time), shots without a label last; every thread starts a new row."""
    if by == "time":
        return [(i, False) for i in range(len(cells))]
    if by != "thread":
        raise ValueError("--by is time or thread")
    ranks = thread_ranks([c[2] for c in cells])
    key = lambda i: (ranks.get(cells[i][2], len(ranks)), cells[i][1], i)          # noqa: E731
    order = sorted(range(len(cells)), key=key)
    return [(i, p > 0 and key(i)[0] != key(order[p - 1])[0]) for p, i in enumerate(order)]


def layout(cells, K, tw, th, columns, by="time"):
    """cells: [(number, start, label, tiles shown)] in time order.  -> (W, H, [[(x, y)] per cell, in time order], primitives, [cell
    index in sheet order]).  Cells are cell_size wide and high and fill rows of `columns` from the left in sheet order (sheet_order; a
    thread's first cell starts a new row).  In the cell at (x, y) the caption's glyph boxes start GAP in and GAP down at text_scale(tw),
    tile k sits at (x + GAP + k (tw + GAP), y + 2 GAP + 7 scale), and one outline two pixels wide runs around the row of tiles shown,
    not on it.  Caption and outline take render.PALETTE[rank % 26] of the cell's label, NEUTRAL without one."""
    K, tw, th, columns = int(K), int(tw), int(th), int(columns)
    if K < 1 or columns < 1 or not cells:
        raise ValueError("a storyboard has at least one shot, one frame a shot and one column")
    s = text_scale(tw)
    cw, ch = cell_size(K, tw, th)
    ranks = thread_ranks([c[2] for c in cells])
    order = sheet_order([c[:3] for c in cells], by)
    corners, prims = [None] * len(cells), []
    col, row, widest = 0, 0, 0
    for p, (i, new_row) in enumerate(order):
        if p and (new_row or col == columns):
            col, row = 0, row + 1
        number, start, label, shown = cells[i]
        x, y = col * cw, row * ch
        rgb = render.PALETTE[ranks[label] % len(render.PALETTE)] if label is not None else NEUTRAL
        text = caption(number, start, label).encode("utf-8")[:min(render.MAX_TEXT_RUN, (cw - 2 * GAP) // (6 * s))]
        prims.append((render.PRIM_TEXT, x + GAP, y + GAP + 7 * s - 1, rgb, s, text))
        n = min(int(shown), K)
        tx, ty = x + GAP, y + 2 * GAP + 7 * s
        corners[i] = [(tx + k * (tw + GAP), ty) for k in range(n)]
        if n:
            prims.append((render.PRIM_RECT, tx - 1, ty - 1, tx + (n - 1) * (tw + GAP) + tw, ty + th, rgb))
        col += 1
        widest = max(widest, col)
    return widest * cw, (row + 1) * ch, corners, prims, [i for i, _ in order]


def check_sheet(W, H, n_tiles, n_prims):
    """the library's caps, refused here with the options that shrink a storyboard"""
    for what, value, cap in (("PVF_SHEET_MAX_SIDE", max(W, H), MAX_SIDE), ("PVF_SHEET_MAX_PIXELS", W * H, MAX_PIXELS),
                             ("PVF_SHEET_MAX_TILES", n_tiles, MAX_TILES), ("PVF_RENDER_MAX_PRIMS", n_prims, render.MAX_PRIMS)):
        if value > cap:
            raise ValueError("a storyboard of %d x %d pixels with %d frames and %d captions and outlines is beyond what one picture holds "
                             "(%s: %d, at most %d): lower --width, or narrow --from / --until" % (W, H, n_tiles, n_prims, what, value, cap))


def index_line(number, k, frame, fps, xy, label):
    return "%d %d %d %.3f %d %d %s\n" % (number, k, frame, frame / float(fps), xy[0], xy[1], "-" if label is None else label)


def plan(shots, labels, fps, n_frames, per, t_from=0.0, t_until=None):
    """[(number, start, label, [frames])] for the shots whose start lies in [t_from, t_until), numbered by their place in the shot file
    (from 0); a shot that starts past the film is skipped with a warning"""
    out = []
    for number, (s, label) in enumerate(zip(shots, labels)):
        if s.start < t_from or (t_until is not None and not s.start < t_until):
            continue
        frames = shot_frames(s.start, s.end, fps, n_frames, per)
        if frames is None:
            warnings.warn("shot %d starts at t = %.3f, past the end of the video" % (number, s.start))
            continue
        out.append((number, float(s.start), label, frames))
    return out


def build(ctx, video, shots, labels=None, per=1, width=160, columns=None, by="time", t_from=0.0, t_until=None, batch=64, ahead=None):
    """the sheet of the shots: (uint8 [H, W, 3], index lines, {"width", "height", "shots", "tiles"}).  One FrameFeed over the wanted
    frames; every `batch` frames one frame_thumbs call, after which the frames are released -- only thumbnails are kept -- then one
    thumb_sheet call."""
    import numpy as np
    from .feed import FrameFeed
    per, width, batch = int(per), int(width), max(1, int(batch))
    if not 1 <= per <= MAX_PER:
        raise ValueError("storyboard: --per is 1 .. %d" % MAX_PER)
    if not 1 <= width <= MAX_THUMB:
        raise ValueError("storyboard: --width is 1 .. %d" % MAX_THUMB)
    fps, n_frames = float(video.frame_rate), len(video)
    w, h = video.frame_size
    tw, th = tile_size(width, w, h)
    if th > MAX_THUMB:
        raise ValueError("storyboard: a thumbnail of %d x %d pixels; lower --width (sides up to %d)" % (tw, th, MAX_THUMB))
    chosen = plan(shots, labels if labels is not None else [None] * len(shots), fps, n_frames, per, t_from, t_until)
    if not chosen:
        raise ValueError("storyboard: no shot to show (an empty shot file, or --from / --until leave none)")
    cols = int(columns) if columns else default_columns(per, tw)
    W, H, corners, prims, order = layout([(c[0], c[1], c[2], len(c[3])) for c in chosen], per, tw, th, cols, by)
    tiles = [(ci, k) for ci in order for k in range(len(chosen[ci][3]))]          # in sheet order: a later cell lies over an earlier
    check_sheet(W, H, len(tiles), len(prims))
    wanted = sorted(set(f for c in chosen for f in c[3]))
    thumb_of = {}
    with FrameFeed(ctx, video, set(wanted), ahead=ahead if ahead is not None else batch + 32, ring_depth=max(2, min(len(wanted), 16)),
                   seek=True, name="pvface-storyboard-reader") as feed:
        for part in feed.batches(batch):
            frames = [dev for _, dev in part]
            thumb_of.update(zip((fi for fi, _ in part), ctx.frame_thumbs(frames, tw, th)))
            feed.release_all(frames)
    thumbs = np.stack([thumb_of[chosen[ci][3][k]] for ci, k in tiles]).reshape(-1, th, tw, 3)
    sheet = ctx.thumb_sheet(thumbs, [corners[ci][k] for ci, k in tiles], W, H, BACKGROUND, prims)
    lines = [index_line(chosen[ci][0], k, chosen[ci][3][k], fps, corners[ci][k], chosen[ci][2]) for ci, k in tiles]
    return sheet, lines, {"width": W, "height": H, "shots": len(chosen), "tiles": len(tiles)}
