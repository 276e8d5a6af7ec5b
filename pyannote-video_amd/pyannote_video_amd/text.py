"""The host rules of the `text` and `caption` verbs (CAPTION.md): a text file's words, which frames of a video are measured, how a batch
hands its last frame to the next call, and how the masks become captions -- cells held over a window, gaps between words closed,
components over time and space, four drop rules, and the tracks on screen with a caption.  Everything is integer arithmetic.  Nothing here
touches the device but `Carry.measure`, which calls runtime.Context.frame_text."""
import numpy as np

from .feed import EveryKth               # noqa: F401 -- which frames of a video are measured: every k-th from the first
from .talk import half_up, ms

CELL = 16                                # PVF_TEXT_CELL
HEAD = 8                                 # PVF_TEXT_HEAD_WORDS
MAX_SIDE = 8192                          # PVF_TEXT_MAX_SIDE
MAX_FRAMES = 4096                        # PVF_TEXT_MAX_FRAMES: frames of one library call
HAS_PREV = 1 << 31


def geometry(w, h):
    """-> (cw, ch, wpr): cells across, cells down, mask words per cell row"""
    cw, ch = (int(w) + CELL - 1) // CELL, (int(h) + CELL - 1) // CELL
    return cw, ch, (cw + 31) // 32


def row_words(w, h):
    cw, ch, wpr = geometry(w, h)
    return HEAD + ch * wpr


def every(step, frame_rate):
    """k of `--step`: every k-th frame is measured, k = max(1, floor(step * rate + 1 / 2))"""
    return max(1, half_up(float(step) * float(frame_rate)))


def stamp(rows, first, frame_rate, k=1):
    """fills the caller's words of the rows of frames first, first + k, ...: ms(T) and the frame index, T = index / frame_rate"""
    for j in range(len(rows)):
        i = first + j * k
        rows[j, 6] = ms(i / float(frame_rate))
        rows[j, 7] = i
    return rows


class Carry(object):
    """the rows of a video, batch by batch: the last frame of a batch stays resident as `prev` of the next call, so the rows do not
    depend on how the frames are cut into calls"""

    def __init__(self, ctx, edge=48, still=8, on=24):
        if not (1 <= int(edge) <= 255 and 0 <= int(still) <= 254 and 1 <= int(on) <= 256):
            raise ValueError("text: --edge is 1 .. 255, --still 0 .. 254, --on 1 .. 256")
        self.ctx, self.edge, self.still, self.on = ctx, int(edge), int(still), int(on)
        self.held = None                         # the frame in front of the next batch

    def measure(self, frames):
        """-> (rows uint32 [len(frames), 8 + ch wpr], the frames the caller may release now: the one held from before and all but the
        last of these)"""
        if not frames:
            return None, []
        rows, _ = self.ctx.frame_text(frames, prev=self.held, edge=self.edge, still=self.still, on=self.on)
        done = ([self.held] if self.held is not None else []) + list(frames[:-1])
        self.held = frames[-1]
        return rows, done


def load(path, who="caption"):
    """a text file: uint32 [n][8 + ch wpr], consistent with its word 0"""
    try:
        r = np.load(path, allow_pickle=False)
    except Exception as e:                   # noqa: BLE001 -- whatever numpy raises for a file that is no array
        raise ValueError("%s: %s is not a text file (%s)" % (who, path, e))
    return check(r, who, path)


def check(r, who="caption", path="the table"):
    if r.dtype != np.uint32 or r.ndim != 2 or r.shape[1] < HEAD:
        raise ValueError("%s: %s is not a text file: uint32 [n][8 + ch wpr] is expected, %s %s found" % (who, path, r.dtype, list(r.shape)))
    r = np.ascontiguousarray(r)
    if len(r) == 0:
        return r
    w, h = int(r[0, 0]) & 0xFFFF, int(r[0, 0]) >> 16
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE) or r.shape[1] != row_words(w, h):
        raise ValueError("%s: %s is not a text file: rows of %d words do not belong to frames of %d x %d" % (who, path, r.shape[1], w, h))
    if (r[:, 0] != r[0, 0]).any() or ((r[:, 1] & ~np.uint32(HAS_PREV)) != (r[0, 1] & ~np.uint32(HAS_PREV))).any():
        raise ValueError("%s: %s holds rows of different frame sizes or parameters" % (who, path))
    if (np.diff(r[:, 6].astype(np.int64)) < 0).any():
        raise ValueError("%s: the rows of %s are not in the order of time" % (who, path))
    return r


def bits_of(rows):
    """bool [n][ch][cw]: the mask of every row"""
    w, h = int(rows[0, 0]) & 0xFFFF, int(rows[0, 0]) >> 16
    cw, ch, wpr = geometry(w, h)
    words = rows[:, HEAD:].reshape(len(rows), ch, wpr)
    b = (words[:, :, :, None] >> np.arange(32, dtype=np.uint32)[None, None, None, :]) & np.uint32(1)
    return b.reshape(len(rows), ch, wpr * 32)[:, :, :cw].astype(bool)


def close_gaps(held, gap):
    """bool [ch][cw]: a run of at most `gap` unheld cells between two held cells of a cell row is held too"""
    if gap <= 0 or not held.any():
        return held
    ch, cw = held.shape
    idx = np.arange(cw)[None, :]
    left = np.maximum.accumulate(np.where(held, idx, -1), axis=1)                     # the last held cell at or before c, or -1
    right = np.minimum.accumulate(np.where(held, idx, cw + gap + 1)[:, ::-1], axis=1)[:, ::-1]    # the next one, or far away
    return held | ((left >= 0) & (right < cw) & (right - left - 1 <= gap))


def runs_of(held):
    """[(r, c0, c1)] the maximal runs of held cells of every cell row, by (r, c0)"""
    ch, cw = held.shape
    p = np.zeros((ch, cw + 2), np.int8)
    p[:, 1:-1] = held
    d = np.diff(p, axis=1)
    rs, starts = np.nonzero(d == 1)
    _, ends = np.nonzero(d == -1)
    return [(int(r), int(a), int(b) - 1) for r, a, b in zip(rs, starts, ends)]


class _Sets(object):
    def __init__(self):
        self.parent = []

    def add(self):
        self.parent.append(len(self.parent))
        return len(self.parent) - 1

    def find(self, a):
        while self.parent[a] != a:
            self.parent[a] = self.parent[self.parent[a]]
            a = self.parent[a]
        return a

    def join(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)


def held_cells(rows, window=1.0, hold=0.5, gap=1, band=(0.0, 1.0)):
    """yields (t, bool [ch][cw]) for every row: rules 2, 3 and 4"""
    hold100 = half_up(100.0 * hold)
    a1000, b1000 = half_up(1000.0 * band[0]), half_up(1000.0 * band[1])
    if not 0 <= hold100 <= 100:
        raise ValueError("caption: --hold is 0 .. 1")
    if not 0 <= a1000 < b1000 <= 1000:
        raise ValueError("caption: --rows A,B with 0 <= A < B <= 1")
    if window < 0 or int(gap) < 0:
        raise ValueError("caption: --window and --gap are not negative")
    n = len(rows)
    if n == 0:
        return
    h = int(rows[0, 0]) >> 16
    bits = bits_of(rows)
    ch, cw = bits.shape[1:]
    centre = 1000 * (CELL * np.arange(ch) + CELL // 2)
    keep = ((a1000 * h <= centre) & (centre < b1000 * h))[:, None]
    usable = [bool(int(rows[t, 1]) & HAS_PREV) for t in range(n)]
    t_ms = [int(v) for v in rows[:, 6]]
    width = ms(window)
    total, count, lo, hi = np.zeros((ch, cw), np.int32), 0, 0, 0                      # the usable rows lo .. hi - 1 are in the window
    for t in range(n):
        if not usable[t]:
            yield t, np.zeros((ch, cw), bool)
            continue
        while hi < n and 2 * (t_ms[hi] - t_ms[t]) <= width:
            if usable[hi]:
                total += bits[hi]
                count += 1
            hi += 1
        while 2 * (t_ms[t] - t_ms[lo]) > width:
            if usable[lo]:
                total -= bits[lo]
                count -= 1
            lo += 1
        yield t, close_gaps((100 * total >= hold100 * count) & keep, int(gap))


def analyse(rows, window=1.0, hold=0.5, gap=1, min_duration=1.0, min_width=3, max_height=0.25, fill=0.5, band=(0.0, 1.0)):
    """-> [(s, e, r0, r1, c0, c1, K)] in row and cell indices: the components that pass rule 6, by (s, e, r0, c0)"""
    fill100, mh1000 = half_up(100.0 * fill), half_up(1000.0 * max_height)
    if not 0 <= fill100 <= 100:
        raise ValueError("caption: --fill is 0 .. 1")
    if min_duration < 0 or int(min_width) < 0 or max_height < 0:
        raise ValueError("caption: --min-duration, --min-width and --max-height are not negative")
    list(held_cells(rows[:0], window=window, hold=hold, gap=gap, band=band))         # the checks of rules 2 to 4, whatever the file holds
    if len(rows) == 0:
        return []
    h = int(rows[0, 0]) >> 16
    t_ms = [int(v) for v in rows[:, 6]]
    sets, box = _Sets(), []                      # per run: [s, e, r0, r1, c0, c1, K], summed into the root at the end
    before = {}                                  # the runs of the row before, by cell row: [(c0, c1, id)]
    for t, held in held_cells(rows, window=window, hold=hold, gap=gap, band=band):
        now = {}
        for r, c0, c1 in runs_of(held):
            k = sets.add()
            box.append([t, t, r, r, c0, c1, c1 - c0 + 1])
            # the cell row above in this row of the file, and the same cell row in the row before: cells that share a column
            for p0, p1, pk in now.get(r - 1, []) + before.get(r, []):
                if p0 <= c1 and c0 <= p1:
                    sets.join(k, pk)
            now.setdefault(r, []).append((c0, c1, k))
        before = now
    merged = {}
    for k, b in enumerate(box):
        m = merged.setdefault(sets.find(k), list(b[:6]) + [0])
        m[0], m[1], m[2], m[3], m[4], m[5] = min(m[0], b[0]), max(m[1], b[1]), min(m[2], b[2]), max(m[3], b[3]), min(m[4], b[4]), max(m[5], b[5])
        m[6] += b[6]
    least = ms(min_duration)
    found = []
    for s, e, r0, r1, c0, c1, K in merged.values():
        bw, bh = c1 - c0 + 1, r1 - r0 + 1
        if t_ms[e] - t_ms[s] < least or bw < int(min_width) or 1000 * CELL * bh > mh1000 * h or 100 * K < fill100 * bw * bh * (e - s + 1):
            continue
        found.append((s, e, r0, r1, c0, c1, K))
    found.sort(key=lambda f: (int(rows[f[0], 7]), int(rows[f[1], 7]), f[2], f[4]))
    return found


def present_tracks(tracks, a_ms, b_ms):
    """the identifiers of the tracks whose lines with ms(T) in [a_ms, b_ms] span at least half of b_ms - a_ms.  tracks: what
    formats.read_tracks returns"""
    seen = {}
    for line in tracks:
        T, identifier = ms(line[0]), int(line[1])
        if a_ms <= T <= b_ms:
            lo, hi = seen.get(identifier, (T, T))
            seen[identifier] = (min(lo, T), max(hi, T))
    return sorted(i for i, (lo, hi) in seen.items() if 2 * (hi - lo) >= b_ms - a_ms)


def report(rows, found, tracks=None):
    """the list the verb writes"""
    if len(rows) == 0:
        return []
    w, h = int(rows[0, 0]) & 0xFFFF, int(rows[0, 0]) >> 16
    out = []
    for s, e, r0, r1, c0, c1, K in found:
        d = {"start": round(int(rows[s, 6]) / 1000.0, 3), "end": round(int(rows[e, 6]) / 1000.0, 3), "first": int(rows[s, 7]), "last": int(rows[e, 7]),
             "left": CELL * c0, "top": CELL * r0, "right": min(w, CELL * (c1 + 1)), "bottom": min(h, CELL * (r1 + 1)), "cells": int(K)}
        if tracks is not None:
            d["tracks"] = present_tracks(tracks, int(rows[s, 6]), int(rows[e, 6]))
            d["alone"] = len(d["tracks"]) == 1
        out.append(d)
    return out
