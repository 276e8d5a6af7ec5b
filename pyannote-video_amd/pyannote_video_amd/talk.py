"""The host side of the `talk` verb (TALK.md): from the eight integers the library returns per face (csrc/talk.hip) and the 68 points
of a face to lip activity, its smoothed course along a track, and the spans in which a track is taken to be talking.  The pixels are
the library's; what is here is a handful of integers and floats per face."""
import math

import numpy as np

WINDOW_ROWS, WINDOW_COLS = 40, 64
WINDOW_PIXELS = WINDOW_ROWS * WINDOW_COLS  # 2560: what an activity is divided by
BOTH_PIXELS = 2 * WINDOW_PIXELS            # 5120: what NZ counts over
MOUTH_ROW0, CONTROL_ROW0, COL0 = 94, 52, 42
MARGIN = 3                                 # shifts of -3 .. 3 rows and columns
ZERO_SHIFT = (2 * MARGIN + 1) * MARGIN + MARGIN        # 24 = (0 + 3) * 7 + (0 + 3)
MAX_FACES = 32768                          # PVF_MOTION_MAX_FACES
COLUMNS = ("DM0", "DMmin", "kM", "DC0", "DCmin", "kC", "SM", "NZ")
WINDOW, ON, OFF, MIN_DURATION, MAX_PAUSE, MAX_DARK = 0.4, 3.0, 1.5, 0.3, 0.3, 0.25      # untuned (TALK.md, Departures)


def ms(t):
    """a time in whole milliseconds: every comparison of times below is made on these"""
    return int(round(float(t) * 1000.0))


def half_up(x):
    """the float-to-int rule of the verbs' options: floor(x + 1/2), x the float64 product or fraction as Python computes it"""
    return int(math.floor(float(x) + 0.5))


def openness(pts):
    """sqrt(gap^2 / width^2) from the 68 integer points: the inner lips' middle points (62 over 66) against the mouth corners (48, 54);
    0.0 when the corners coincide"""
    p = np.asarray(pts).reshape(68, 2)
    gap = (int(p[66][0]) - int(p[62][0])) ** 2 + (int(p[66][1]) - int(p[62][1])) ** 2
    width = (int(p[54][0]) - int(p[48][0])) ** 2 + (int(p[54][1]) - int(p[48][1])) ** 2
    return 0.0 if width == 0 else math.sqrt(float(gap) / float(width))


def activity(row, linked, max_dark=MAX_DARK):
    """(a, valid) of a face's eight integers: a = max(0, DMmin - DCmin) / 2560 in grey levels per pixel, what the mouth window
    changed beyond what the control window above it did, each after the best of 49 shifts; 0.0 for a face that is not linked to a
    predecessor or whose windows are too dark (a chip is black where it leaves the frame)"""
    valid = bool(linked and int(row[7]) <= max_dark * BOTH_PIXELS)
    return (max(0, int(row[1]) - int(row[4])) / float(WINDOW_PIXELS) if valid else 0.0), valid


def link(faces):
    """faces: [(frame index, track)] -> for each the index of the face of the same track on the frame before, or -1"""
    at = dict(((int(f), int(k)), i) for i, (f, k) in enumerate(faces))
    return [at.get((int(f) - 1, int(k)), -1) for f, k in faces]


def smooth(times, a, valid, window=WINDOW):
    """one track in time order: s(t) = mean of a over its valid faces with |t' - t| <= window / 2, summed in time order; 0.0 without any"""
    t, w = [ms(x) for x in times], ms(window)
    out, lo = [], 0
    for i in range(len(t)):
        while 2 * (t[i] - t[lo]) > w:
            lo += 1
        total, n, j = 0.0, 0, lo
        while j < len(t) and 2 * (t[j] - t[i]) <= w:
            if valid[j]:
                total += a[j]
                n += 1
            j += 1
        out.append(total / n if n else 0.0)
    return out


def decide(s, on=ON, off=OFF):
    """hysteresis along a track in time order: on at s >= on, off at s < off, else as before; starts off"""
    out, state = [], False
    for v in s:
        if v >= on:
            state = True
        elif v < off:
            state = False
        out.append(state)
    return out


def spans(times, state, s, min_duration=MIN_DURATION, max_pause=MAX_PAUSE):
    """[(first index, last index, mean s)] of one track in time order: maximal runs of talking faces; runs no more than max_pause apart
    (first time of the later - last time of the earlier) are merged first, then spans shorter than min_duration (last time - first time)
    are dropped.  mean s is over every face of the track from first to last, summed in time order."""
    t = [ms(x) for x in times]
    runs, i, n = [], 0, len(t)
    while i < n:
        if not state[i]:
            i += 1
            continue
        j = i
        while j + 1 < n and state[j + 1]:
            j += 1
        if runs and t[i] - t[runs[-1][1]] <= ms(max_pause):
            runs[-1][1] = j
        else:
            runs.append([i, j])
        i = j + 1
    out = []
    for i, j in runs:
        if t[j] - t[i] < ms(min_duration):
            continue
        total = 0.0
        for k in range(i, j + 1):
            total += s[k]
        out.append((i, j, total / (j - i + 1)))
    return out


def analyse(faces, rows, linked, window=WINDOW, on=ON, off=OFF, min_duration=MIN_DURATION, max_pause=MAX_PAUSE, max_dark=MAX_DARK):
    """faces: [(T, track, points)] in any order; rows: their eight integers; linked: whether each has a predecessor.
    -> ([(open, a, s, talking)] per face, [(track, start, end, mean s)] by track, then start).  talking is 1 inside a kept span."""
    act = [activity(rows[i], linked[i], max_dark) for i in range(len(faces))]
    per = [[openness(f[2]), act[i][0], 0.0, 0] for i, f in enumerate(faces)]
    tracks = {}
    for i, f in enumerate(faces):
        tracks.setdefault(int(f[1]), []).append(i)
    segments = []
    for track in sorted(tracks):
        idx = sorted(tracks[track], key=lambda i: (ms(faces[i][0]), i))
        times = [faces[i][0] for i in idx]
        s = smooth(times, [act[i][0] for i in idx], [act[i][1] for i in idx], window)
        for i, v in zip(idx, s):
            per[i][2] = v
        for first, last, mean in spans(times, decide(s, on, off), s, min_duration, max_pause):
            for i in idx[first:last + 1]:
                per[i][3] = 1
            segments.append((track, times[first], times[last], mean))
    return [tuple(p) for p in per], segments


def face_line(T, track, row, opn, a, s, talking):
    return "%.3f %d %d %d %d %d %d %d %d %d %.5f %.5f %.5f %d\n" % ((T, track) + tuple(int(v) for v in row) + (opn, a, s, 1 if talking else 0))


def segment_line(track, start, end, mean, name=None):
    return "%d %.3f %.3f %.5f%s\n" % (track, start, end, mean, "" if name is None else " %s" % name)
