"""CAPTION.md restated in numpy and plain loops: the text record of a frame (what csrc/text.hip computes; held to this with np.array_equal)
and the host rules of `caption` (what pyannote_video_amd/text.py computes).  Nothing here imports the package's text module.

`defect` plants one wrong reading of the definition into the record, for tests/test_text_ref.py to show that the comparison sees it."""
import numpy as np

CELL, HEAD = 16, 8
DEFECTS = ("forward", "wrap", "edge_gt", "still_lt", "no_prev_stroke", "cell15", "bit_reversed", "tail_bits", "two_back", "no_round")


def ms(t):
    return int(round(float(t) * 1000.0))


def half_up(x):
    return int(np.floor(float(x) + 0.5))


def geometry(w, h):
    cw, ch = -(-w // CELL), -(-h // CELL)
    return cw, ch, -(-cw // 32)


def luma(rgb, defect=None):
    p = np.asarray(rgb).astype(np.int64)
    return (77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + (0 if defect == "no_round" else 128)) >> 8


def gx_of(Y, defect=None):
    """the central horizontal difference, neighbours clamped at the frame's sides"""
    w = Y.shape[1]
    x = np.arange(w)
    if defect == "forward":
        return np.abs(Y[:, np.minimum(x + 1, w - 1)] - Y)
    if defect == "wrap":
        return np.abs(Y[:, (x + 1) % w] - Y[:, (x - 1) % w])
    return np.abs(Y[:, np.minimum(x + 1, w - 1)] - Y[:, np.maximum(x - 1, 0)])


def strokes_of(Y, edge, defect=None):
    g = gx_of(Y, defect)
    return g > edge if defect == "edge_gt" else g >= edge


def cell_sums(flag, defect=None):
    """[ch][cw]: how many pixels of every cell have the flag"""
    h, w = flag.shape
    cw, ch, _ = geometry(w, h)
    if defect != "cell15":
        p = np.zeros((ch * CELL, cw * CELL), np.int64)
        p[:h, :w] = flag
        return p.reshape(ch, CELL, cw, CELL).sum(axis=(1, 3))
    out = np.zeros((ch, cw), np.int64)
    np.add.at(out, (np.minimum(np.arange(h) // 15, ch - 1)[:, None], np.minimum(np.arange(w) // 15, cw - 1)[None, :]), flag.astype(np.int64))
    return out


def record(Y, Yp, edge, still, on, defect=None):
    """-> (row uint32 [8 + ch wpr], counts uint16 [ch][cw][4]) of a frame's luma Y and its predecessor's Yp (or None)"""
    h, w = Y.shape
    cw, ch, wpr = geometry(w, h)
    st = strokes_of(Y, edge, defect)
    NP, E = cell_sums(np.ones_like(st), defect), cell_sums(st, defect)
    if Yp is None:
        S, M = np.zeros_like(E), np.zeros_like(E)
    else:
        d = np.abs(Y - Yp)
        quiet = d < still if defect == "still_lt" else d <= still
        before = np.ones_like(st) if defect == "no_prev_stroke" else strokes_of(Yp, edge, defect)
        S, M = cell_sums(st & before & quiet, defect), cell_sums(d > still, defect)
    row = np.zeros(HEAD + ch * wpr, np.uint32)
    row[0] = w | h << 16
    row[1] = edge | still << 8 | on << 16 | (0 if Yp is None else 1) << 31
    bit = S >= on
    row[2], row[3], row[4], row[5] = E.sum(), S.sum(), M.sum(), bit.sum()
    for r in range(ch):
        for c in range(cw):
            if bit[r, c]:
                row[HEAD + r * wpr + (c >> 5)] |= np.uint32(1) << np.uint32(31 - (c & 31) if defect == "bit_reversed" else c & 31)
        if defect == "tail_bits":
            for c in range(cw, 32 * wpr):
                row[HEAD + r * wpr + (c >> 5)] |= np.uint32(1) << np.uint32(c & 31)
    return row, np.stack([E, S, M, NP], axis=2).astype(np.uint16)


def rows_of(frames, prev=None, edge=48, still=8, on=24, defect=None):
    """frames: a list of uint8 [h][w][3]; prev: the frame in front of frames[0] or None -> (rows uint32 [n][8 + ch wpr], counts uint16
    [n][ch][cw][4])"""
    chain = ([] if prev is None else [luma(prev, defect)]) + [luma(f, defect) for f in frames]
    lag = 2 if defect == "two_back" else 1
    first = len(chain) - len(frames)
    rows, counts = [], []
    for i in range(first, len(chain)):
        r, c = record(chain[i], chain[i - lag] if i - lag >= 0 else None, edge, still, on, defect)
        rows.append(r)
        counts.append(c)
    return np.stack(rows), np.stack(counts)


def video_rows(frames, fps, step=0.0, edge=48, still=8, on=24, first=0, end=None):
    """what `text` writes for a video: every k-th frame of [first, end) against the measured frame before it, stamped"""
    k = max(1, half_up(step * fps))
    idx = list(range(first, len(frames) if end is None else min(end, len(frames)), k))
    rows, _ = rows_of([frames[i] for i in idx], None, edge, still, on)
    for j, i in enumerate(idx):
        rows[j, 6], rows[j, 7] = ms(i / float(fps)), i
    return rows


# ---- the host rules -----------------------------------------------------------------------------------------------------------------------
def bits_of(rows):
    w, h = int(rows[0, 0]) & 0xFFFF, int(rows[0, 0]) >> 16
    cw, ch, wpr = geometry(w, h)
    out = np.zeros((len(rows), ch, cw), bool)
    for t in range(len(rows)):
        for r in range(ch):
            for c in range(cw):
                out[t, r, c] = (int(rows[t, HEAD + r * wpr + (c >> 5)]) >> (c & 31)) & 1
    return out


def held_of(rows, window=1.0, hold=0.5, gap=1, band=(0.0, 1.0)):
    """bool [n][ch][cw]: rules 2, 3 and 4"""
    n = len(rows)
    h = int(rows[0, 0]) >> 16
    bits = bits_of(rows)
    _, ch, cw = bits.shape
    hold100, a1000, b1000 = half_up(100 * hold), half_up(1000 * band[0]), half_up(1000 * band[1])
    usable = [(int(rows[t, 1]) >> 31) & 1 == 1 for t in range(n)]
    t_ms = [int(rows[t, 6]) for t in range(n)]
    held = np.zeros((n, ch, cw), bool)
    for t in range(n):
        if not usable[t]:
            continue
        win = [j for j in range(n) if usable[j] and 2 * abs(t_ms[j] - t_ms[t]) <= ms(window)]
        votes = sum(bits[j].astype(np.int64) for j in win)
        held[t] = 100 * votes >= hold100 * len(win)
        for r in range(ch):
            if not (a1000 * h <= 1000 * (CELL * r + 8) < b1000 * h):
                held[t, r] = False
                continue
            on = [c for c in range(cw) if held[t, r, c]]
            for a, b in zip(on[:-1], on[1:]):
                if b - a - 1 <= gap:
                    held[t, r, a:b] = True
    return held


def components(held):
    """[(s, e, r0, r1, c0, c1, K)] of the held cells: neighbours are (t, r, c +- 1), (t, r +- 1, c) and (t +- 1, r, c)"""
    seen = np.zeros_like(held)
    out = []
    n, ch, cw = held.shape
    for start in zip(*np.nonzero(held)):
        if seen[start]:
            continue
        seen[start] = True
        stack, cells = [start], []
        while stack:
            t, r, c = stack.pop()
            cells.append((t, r, c))
            for q in ((t, r, c - 1), (t, r, c + 1), (t, r - 1, c), (t, r + 1, c), (t - 1, r, c), (t + 1, r, c)):
                if 0 <= q[0] < n and 0 <= q[1] < ch and 0 <= q[2] < cw and held[q] and not seen[q]:
                    seen[q] = True
                    stack.append(q)
        ts, rs, cs = zip(*cells)
        out.append(tuple(int(v) for v in (min(ts), max(ts), min(rs), max(rs), min(cs), max(cs), len(cells))))
    return out


def captions(rows, window=1.0, hold=0.5, gap=1, min_duration=1.0, min_width=3, max_height=0.25, fill=0.5, band=(0.0, 1.0), tracks=None):
    """the list `caption` writes"""
    if len(rows) == 0:
        return []
    w, h = int(rows[0, 0]) & 0xFFFF, int(rows[0, 0]) >> 16
    fill100, mh1000 = half_up(100 * fill), half_up(1000 * max_height)
    out = []
    for s, e, r0, r1, c0, c1, K in components(held_of(rows, window, hold, gap, band)):
        bw, bh, a, b = c1 - c0 + 1, r1 - r0 + 1, int(rows[s, 6]), int(rows[e, 6])
        if b - a < ms(min_duration) or bw < min_width or 1000 * CELL * bh > mh1000 * h or 100 * K < fill100 * bw * bh * (e - s + 1):
            continue
        d = {"start": round(a / 1000.0, 3), "end": round(b / 1000.0, 3), "first": int(rows[s, 7]), "last": int(rows[e, 7]), "left": CELL * c0,
             "top": CELL * r0, "right": min(w, CELL * (c1 + 1)), "bottom": min(h, CELL * (r1 + 1)), "cells": K}
        if tracks is not None:
            ids = sorted(set(int(line[1]) for line in tracks))
            d["tracks"] = []
            for i in ids:
                times = [ms(line[0]) for line in tracks if int(line[1]) == i and a <= ms(line[0]) <= b]
                if times and 2 * (max(times) - min(times)) >= b - a:
                    d["tracks"].append(i)
            d["alone"] = len(d["tracks"]) == 1
        out.append(d)
    out.sort(key=lambda d: (d["first"], d["last"], d["top"], d["left"]))
    return out
