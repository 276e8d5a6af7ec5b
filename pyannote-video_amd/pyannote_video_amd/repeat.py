"""The host rules of the `fingerprint` and `repeat` verbs (REPEAT.md): a print file's words, which frames are usable, how the runs of
matching prints (runtime.Context.print_runs) become segments, and what is written.  Nothing here touches the device."""
import numpy as np

from .feed import EveryKth
from .talk import ms

RUNS_STRIP = 1024                        # PVF_RUNS_STRIP: rows of A a workgroup of print_runs_k walks
MAX_ROWS = 1 << 24                       # PVF_PRINT_MAX_ROWS


def EveryFrame(first=0, end=None):
    """the `wanted` of a FrameFeed that wants every frame of a video, whatever its length: the frames whose index lies in [first, end),
    at most as many as a print file holds"""
    return EveryKth(first, MAX_ROWS if end is None else end, 1)


def stamp(prints, first, frame_rate):
    """fills the caller's word of the prints of frames first, first + 1, ...: ms(T) | frame index << 32 with T = index / frame_rate"""
    for k in range(len(prints)):
        i = first + k
        prints[k, 3] = np.uint64(ms(i / float(frame_rate)) | i << 32)
    return prints


def load(path):
    """a print file: uint64 [n][4]"""
    try:
        p = np.load(path, allow_pickle=False)
    except Exception as e:                   # noqa: BLE001 -- whatever numpy raises for a file that is no array
        raise ValueError("repeat: %s is not a print file (%s)" % (path, e))
    if p.dtype != np.uint64 or p.ndim != 2 or p.shape[1] != 4:
        raise ValueError("repeat: %s is not a print file: uint64 [n][4] is expected, %s %s found" % (path, p.dtype, list(p.shape)))
    if len(p) > MAX_ROWS:
        raise ValueError("repeat: %s holds more than %d prints" % (path, MAX_ROWS))
    return np.ascontiguousarray(p)


def times_ms(p):
    return (p[:, 3] & np.uint64(0xFFFFFFFF)).astype(np.int64)


def usable(p, flat):
    """a byte per frame: RANGE >= flat"""
    return ((p[:, 2] >> np.uint64(32)) >= np.uint64(max(int(flat), 0))).astype(np.uint8)


def separation_frames(t_ms, min_separation):
    """--min-separation in frames of this file: the first g >= 1 whose frame lies that long after frame 0 (the file's length if none)"""
    want = ms(min_separation)
    g = 1
    while g < len(t_ms) and t_ms[g] - t_ms[0] < want:
        g += 1
    return g


def bridge(runs, t_ms, max_gap):
    """runs ordered by (j - i, i) -> segments [(i, j, len)]: a run joins the segment before it on its diagonal when the time from that
    segment's last frame to the run's first frame, on A's times, is at most max_gap seconds"""
    gap, out = ms(max_gap), []
    for i, j, n in ((int(r[0]), int(r[1]), int(r[2])) for r in runs):
        if out and out[-1][1] - out[-1][0] == j - i and t_ms[i] - t_ms[out[-1][0] + out[-1][2] - 1] <= gap:
            out[-1] = (out[-1][0], out[-1][1], i + n - out[-1][0])
        else:
            out.append((i, j, n))
    return out


def outermost(segs):
    """longest first, ties by (j - i, i): a segment whose A interval and B interval both lie inside those of a kept one is dropped"""
    kept = []
    for i, j, n in sorted(segs, key=lambda s: (-s[2], s[1] - s[0], s[0])):
        if not any(ki <= i and i + n <= ki + kn and kj <= j and j + n <= kj + kn for ki, kj, kn in kept):
            kept.append((i, j, n))
    return kept


def segments(runs, t_ms, min_duration, max_gap):
    long_enough = ms(min_duration)
    return outermost([s for s in bridge(runs, t_ms, max_gap) if t_ms[s[0] + s[2] - 1] - t_ms[s[0]] >= long_enough])


def compare(ctx, files, max_bits=10, flat=16, min_duration=2.0, max_gap=0.5, min_separation=5.0):
    """files: [(name, prints)] -> the list the verb writes: every file against itself and against every later one"""
    if not files:
        raise ValueError("repeat: no print files")
    if not 0 <= int(max_bits) <= 128:
        raise ValueError("repeat: --max-bits is 0 .. 128")
    tables = [(name, p, usable(p, flat), times_ms(p)) for name, p in files]
    out = []
    for x, (na, pa, ua, ta) in enumerate(tables):
        for y in range(x, len(tables)):
            nb, pb, ub, tb = tables[y]
            if y == x:
                g = separation_frames(ta, min_separation)
                runs = ctx.print_runs(pa, ua, tau=max_bits, min_gap=g) if g < len(pa) else ()
            else:
                runs = ctx.print_runs(pa, ua, pb, ub, tau=max_bits) if len(pa) and len(pb) else ()
            for i, j, n in segments(runs, ta, min_duration, max_gap):
                out.append((x, y, {"a": na, "b": nb, "a_start": round(ta[i] / 1000.0, 3), "a_end": round(ta[i + n - 1] / 1000.0, 3),
                                   "b_start": round(tb[j] / 1000.0, 3), "b_end": round(tb[j + n - 1] / 1000.0, 3), "frames": int(n),
                                   "offset": int(j - i)}))
    out.sort(key=lambda s: (s[0], s[1], s[2]["a_start"], s[2]["offset"]))
    return [s[2] for s in out]
