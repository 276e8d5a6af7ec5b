"""TALK.md restated in numpy: the eight integers of a face chip against its predecessor, and the host rules on top of them.  The
kernels (csrc/talk.hip) are compared with `motion` bit for bit; talk.py with the host rules.  The keyword arguments plant the defects
that test_talk_ref.py shows the comparison to see; none of them is used anywhere else."""
import math

import numpy as np

ROWS, COLS, COL0 = 40, 64, 42
MOUTH0, CONTROL0 = 94, 52
MARGIN = 3
PIXELS = ROWS * COLS
ZERO = 24
MAX_FACES = 32768
DEFAULTS = dict(window=0.4, on=3.0, off=1.5, min_duration=0.3, max_pause=0.3, max_dark=0.25)


def luma(chip, rounding=True):
    c = np.asarray(chip).astype(np.int64).reshape(150, 150, 3)
    return (77 * c[:, :, 0] + 150 * c[:, :, 1] + 29 * c[:, :, 2] + (128 if rounding else 0)) >> 8


def grey(y):
    """the chip whose luma is y (R = G = B = Y gives Y)"""
    return np.repeat(np.asarray(y, np.uint8).reshape(150, 150, 1), 3, axis=2)


def displaced(cur, prv, r0, c0=COL0, margin=MARGIN, wrong_face=False, squared=False):
    """D(dy, dx) of one window as a [7][7] array (2^30 where a defect's smaller range leaves a shift out)"""
    D = np.full((2 * MARGIN + 1, 2 * MARGIN + 1), 1 << 30, np.int64)
    for dy in range(-margin, margin + 1):
        for dx in range(-margin, margin + 1):
            if wrong_face:
                a, b = cur[r0 + dy:r0 + dy + ROWS, c0 + dx:c0 + dx + COLS], prv[r0:r0 + ROWS, c0:c0 + COLS]
            else:
                a, b = cur[r0:r0 + ROWS, c0:c0 + COLS], prv[r0 + dy:r0 + dy + ROWS, c0 + dx:c0 + dx + COLS]
            d = np.abs(a - b)
            D[dy + MARGIN, dx + MARGIN] = int((d * d).sum() if squared else d.sum())
    return D


def pick(D, plain_row_major=False):
    """(D0, Dmin, k): k = 24 when the zero shift is a minimum, else the first minimum in row-major order"""
    flat = [int(v) for v in D.reshape(-1)]
    dmin = min(flat)
    k = flat.index(dmin)
    if flat[ZERO] == dmin and not plain_row_major:
        k = ZERO
    return flat[ZERO], dmin, k


def motion(chips, prev, row_off=0, col_off=0, margin=MARGIN, wrong_face=False, squared=False, rounding=True, plain_row_major=False,
           nz_mouth_only=False):
    """int32 [n][8] = DM0, DMmin, kM, DC0, DCmin, kC, SM, NZ"""
    Y = {}

    def y(i):                                # (chips may be a long list of a few distinct arrays: a luma per array, not per face)
        key = id(chips[i])
        if key not in Y:
            Y[key] = luma(chips[i], rounding)
        return Y[key]
    out = np.full((len(chips), 8), -1, np.int32)
    memo = {}
    for i in range(len(chips)):
        cur = y(i)
        m0, c0, x0 = MOUTH0 + row_off, CONTROL0 + row_off, COL0 + col_off
        mouth, ctrl = cur[m0:m0 + ROWS, x0:x0 + COLS], cur[c0:c0 + ROWS, x0:x0 + COLS]
        out[i, 6] = int(mouth.sum())
        out[i, 7] = int((mouth <= 16).sum()) + (0 if nz_mouth_only else int((ctrl <= 16).sum()))
        p = int(prev[i])
        if p < 0:
            continue
        key = (id(chips[i]), id(chips[p]))
        if key not in memo:
            kw = dict(c0=x0, margin=margin, wrong_face=wrong_face, squared=squared)
            memo[key] = pick(displaced(cur, y(p), m0, **kw), plain_row_major) + pick(displaced(cur, y(p), c0, **kw), plain_row_major)
        out[i, :6] = memo[key]
    return out


# ---- host rules (talk.py), written as plainly as they are stated -------------------------------------------------------------------
def ms(t):
    return int(round(float(t) * 1000.0))


def openness(pts):
    p = np.asarray(pts, np.int64).reshape(68, 2)
    gap, width = int(((p[66] - p[62]) ** 2).sum()), int(((p[54] - p[48]) ** 2).sum())
    return math.sqrt(gap / width) if width else 0.0


def activity(row, linked, max_dark=0.25):
    valid = bool(linked) and int(row[7]) <= max_dark * 5120
    return (max(0, int(row[1]) - int(row[4])) / 2560.0, True) if valid else (0.0, False)


def link(faces):
    out = []
    for f, k in faces:
        hits = [j for j, (g, l) in enumerate(faces) if g == f - 1 and l == k]
        out.append(hits[0] if hits else -1)
    return out


def smooth(times, a, valid, window=0.4):
    out = []
    for t in times:
        near = [a[j] for j, u in enumerate(times) if valid[j] and 2 * abs(ms(u) - ms(t)) <= ms(window)]
        total = 0.0
        for v in near:
            total += v
        out.append(total / len(near) if near else 0.0)
    return out


def decide(s, on=3.0, off=1.5):
    out = []
    for v in s:
        out.append(True if v >= on else False if v < off else (out[-1] if out else False))
    return out


def spans(times, state, s, min_duration=0.3, max_pause=0.3):
    runs = []
    for i, on in enumerate(state):
        if on and i > 0 and state[i - 1]:
            runs[-1][1] = i
        elif on:
            runs.append([i, i])
    merged = []
    for r in runs:
        if merged and ms(times[r[0]]) - ms(times[merged[-1][1]]) <= ms(max_pause):
            merged[-1][1] = r[1]
        else:
            merged.append(list(r))
    out = []
    for i, j in merged:
        if ms(times[j]) - ms(times[i]) >= ms(min_duration):
            total = 0.0
            for v in s[i:j + 1]:
                total += v
            out.append((i, j, total / (j - i + 1)))
    return out


# ---- contents the tests share ------------------------------------------------------------------------------------------------------
def smooth_chip(oy=0, ox=0):
    """smooth, non-periodic content: a sum of two chirps, so that a displaced copy matches at one shift only.  The chip is the
    150 x 150 cut at (oy, ox) of one unbounded picture: smooth_chip(oy + dy, ox + dx)(r, c) = smooth_chip(oy, ox)(r + dy, c + dx)."""
    r, c = np.mgrid[0:150, 0:150].astype(np.float64)
    r, c = r + oy, c + ox
    y = 128 + 60 * np.sin(0.0009 * (r + 70) ** 2 + 0.05 * c) + 60 * np.cos(0.0007 * (c + 45) ** 2 - 0.031 * r)
    return grey(np.clip(np.round(y), 0, 255))


def shifted(chip, dy, dx, fill=0):
    """out(r, c) = chip(r + dy, c + dx): against `chip` as the predecessor the minimum lies at shift (dy, dx)"""
    out = np.full_like(chip, fill)
    h = 150
    out[max(0, -dy):h - max(0, dy), max(0, -dx):h - max(0, dx)] = chip[max(0, dy):h - max(0, -dy), max(0, dx):h - max(0, -dx)]
    return out


def shift_chain():
    """50 chips: the smooth chip, then 49 faces, face 1 + k a copy of ITS predecessor displaced by shift k; prev = i - 1.  (The
    displacements add up to at most 42 rows and 6 columns on the way and to nothing at the end.)"""
    chips, oy, ox = [smooth_chip()], 0, 0
    for k in range(49):
        oy, ox = oy + k // 7 - 3, ox + k % 7 - 3
        chips.append(smooth_chip(oy, ox))
    return chips, [-1] + list(range(49))


def named_cases():
    """{name: (chips, prev)}: what test_gpu_talk.py runs the library on and test_talk_ref.py plants the defects on"""
    rng = np.random.default_rng(1207)
    rnd = [rng.integers(0, 256, (150, 150, 3), dtype=np.uint8) for _ in range(5)]
    black, white = grey(np.zeros((150, 150))), grey(np.full((150, 150), 255))
    stripes = grey(255 * (np.arange(150) % 2)[None, :].repeat(150, 0))              # a one-pixel shift turns it into its negative
    base = smooth_chip()
    dark_nose = base.copy()
    dark_nose[60:70, 50:60] = 0                                                     # dark pixels in the control window only
    cases = {
        "one": (rnd[:1], [-1]),
        "two": (rnd[:2], [-1, 0]),
        "none_linked": (rnd, [-1] * 5),
        "chain": (rnd, [-1, 0, 1, 2, 3]),
        "shared": (rnd, [-1, 0, 0, 2, 2]),
        "far_back": (rnd + rnd[::-1], [-1, -1, -1, -1, -1, 0, 0, 5, 1, 0]),
        "shifts": shift_chain(),
        "moved": ([base, shifted(base, -2, 1)], [-1, 0]),                           # cur[2:, :149] = prev[:148, 1:]
        "extremes": ([black, white, black, stripes, shifted(stripes, 0, 1, fill=255), white], [-1, 0, 1, -1, 3, 4]),
        "constant": ([grey(np.full((150, 150), v)) for v in (90, 90, 93)], [-1, 0, 1]),
        "dark": ([grey(np.full((150, 150), v)) for v in (16, 17)] + [base, dark_nose], [-1, 0, -1, 2]),
        "rounding": ([np.full((150, 150, 3), (1, 0, 0), np.uint8), np.full((150, 150, 3), (2, 0, 0), np.uint8)], [-1, 0]),
    }
    return cases
