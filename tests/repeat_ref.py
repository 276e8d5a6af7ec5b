"""REPEAT.md restated in numpy and plain Python, independently of pyannote_video_amd/repeat.py and csrc/repeat.hip: the print of a frame
(the grid through tests/storyboard_ref.py's thumbnail, the luma, the bits), the match matrix, the runs by a plain loop over the
diagonals, and every host rule of the `repeat` verb.  The GPU tests hold the kernels to this with np.array_equal;
tests/test_repeat_ref.py holds this to hand-computed cases and shows that the comparison sees planted defects."""
import numpy as np

from tests import storyboard_ref

G = 9
PRINT_DEFECTS = ("le_for_lt", "swap_hv", "bit_order", "luma_floor")
RUN_DEFECTS = ("seam", "flat_matches", "min_gap_off", "min_len_off", "unsorted")


# ---- the print ----------------------------------------------------------------------------------------------------------------------
def grid(frame):
    """uint8 [9, 9, 3]: the thumbnail of the whole frame (STORYBOARD.md, tw = th = 9)"""
    return storyboard_ref.thumb(frame, G, G)


def luma(g, defect=None):
    g = np.asarray(g).astype(np.int64)
    return (77 * g[:, :, 0] + 150 * g[:, :, 1] + 29 * g[:, :, 2] + (0 if defect == "luma_floor" else 128)) >> 8


def bits(y, defect=None):
    """(H, V) as Python ints: bit 8 r + c is y[r][c] < y[r][c + 1], resp. y[r][c] < y[r + 1][c], r and c in 0 .. 7"""
    H = V = 0
    for r in range(8):
        for c in range(8):
            k = 8 * r + ((7 - c) if defect == "bit_order" else c)
            a = int(y[r][c])
            if a < int(y[r][c + 1]) or (defect == "le_for_lt" and a == int(y[r][c + 1])):
                H |= 1 << k
            if a < int(y[r + 1][c]) or (defect == "le_for_lt" and a == int(y[r + 1][c])):
                V |= 1 << k
    return (V, H) if defect == "swap_hv" else (H, V)


def print_of(frame, defect=None):
    """uint64 [4]: H, V, SY | RANGE << 32, 0"""
    y = luma(grid(frame), defect)
    H, V = bits(y, defect)
    return np.array([H, V, int(y.sum()) | (int(y.max()) - int(y.min())) << 32, 0], np.uint64)


def prints(frames, defect=None):
    return np.stack([print_of(f, defect) for f in frames]).reshape(-1, 4) if len(frames) else np.zeros((0, 4), np.uint64)


def ms(t):
    return int(round(float(t) * 1000.0))


def stamp(p, times):
    """the prints with the caller's word filled: ms(T) | frame index << 32"""
    p = np.array(p, np.uint64)
    for i, t in enumerate(times):
        p[i, 3] = np.uint64(ms(t) | i << 32)
    return p


def sy_of(p):
    return np.asarray(p)[:, 2] & np.uint64(0xFFFFFFFF)


def range_of(p):
    return np.asarray(p)[:, 2] >> np.uint64(32)


def ms_of(p):
    return (np.asarray(p)[:, 3] & np.uint64(0xFFFFFFFF)).astype(np.int64)


# ---- matches and runs ---------------------------------------------------------------------------------------------------------------
def distances(A, B):
    """int64 [NA, NB]: popcount(Ha ^ Hb) + popcount(Va ^ Vb)"""
    A, B = np.asarray(A, np.uint64), np.asarray(B, np.uint64)
    return (np.bitwise_count(A[:, None, 0] ^ B[None, :, 0]).astype(np.int64) + np.bitwise_count(A[:, None, 1] ^ B[None, :, 1]))


def match_matrix(A, ua, B, ub, tau, defect=None):
    m = distances(A, B) <= tau
    if defect != "flat_matches":
        m &= (np.asarray(ua) != 0)[:, None] & (np.asarray(ub) != 0)[None, :]
    return m


def runs(A, ua, B=None, ub=None, tau=10, min_len=1, min_gap=1, defect=None, strip=1024):
    """int32 [n, 3]: every maximal run (i, j, len) of matching pairs with len >= min_len, ordered by (j - i, i).  B None: self mode,
    the diagonals j - i >= min_gap of A against A.  defect: one of RUN_DEFECTS (`seam` cuts every run at the multiples of `strip` rows
    of A, as a kernel that does not look behind its strip would)"""
    self_mode = B is None
    if self_mode:
        B, ub = A, ua
    NA, NB = len(A), len(B)
    out = []
    if NA and NB:
        M = match_matrix(A, ua, B, ub, tau, defect)
        lo = (min_gap + (1 if defect == "min_gap_off" else 0)) if self_mode else -(NA - 1)
        for d in range(lo, NB):
            i = max(0, -d)
            step = np.diff(np.concatenate(([0], M.diagonal(d).astype(np.int8), [0])))        # M[i + t, i + t + d] for t = 0 ..
            for a, b in zip(np.nonzero(step == 1)[0], np.nonzero(step == -1)[0]):          # cells [a, b) of the diagonal
                cuts = [a] + ([t for t in range(a + 1, b) if (i + t) % strip == 0] if defect == "seam" else []) + [b]
                for s, e in zip(cuts[:-1], cuts[1:]):
                    out.append((i + s, i + s + d, e - s))
    out = [r for r in out if (r[2] > min_len if defect == "min_len_off" else r[2] >= min_len)]
    if defect == "unsorted":
        out.reverse()
    return np.array(out, np.int32).reshape(-1, 3)


def run_count_all_match(NA, NB, L):
    """runs of a call in which every pair matches (tau = 128, all usable), min_len = L <= min(NA, NB)"""
    return NA + NB - 1 - 2 * (L - 1)


# ---- the host rules -----------------------------------------------------------------------------------------------------------------
def bridge(found, ms_a, max_gap_ms):
    """runs [(i, j, len)] ordered by (j - i, i) -> segments [(i, j, len)]: on one diagonal a later run joins the earlier one when the
    time from frame i1 + len1 - 1 to frame i2 of A is at most max_gap_ms"""
    out = []
    for i, j, n in found:
        if out and out[-1][1] - out[-1][0] == j - i and ms_a[i] - ms_a[out[-1][0] + out[-1][2] - 1] <= max_gap_ms:
            out[-1] = (out[-1][0], out[-1][1], i + n - out[-1][0])
        else:
            out.append((int(i), int(j), int(n)))
    return out


def keep_outermost(segs):
    """longest first (ties by (j - i, i)); a segment whose A interval and B interval both lie inside those of a kept one is dropped"""
    kept = []
    for i, j, n in sorted(segs, key=lambda s: (-s[2], s[1] - s[0], s[0])):
        if not any(ki <= i and i + n <= ki + kn and kj <= j and j + n <= kj + kn for ki, kj, kn in kept):
            kept.append((i, j, n))
    return kept


def segments(pa, pb, tau=10, flat=16, min_duration=2.0, max_gap=0.5, min_separation=5.0):
    """the segments of file A against file B (pb None: against itself) as [(i, j, len)], before the output's order"""
    ua = (range_of(pa) >= flat).astype(np.uint8)
    ta = ms_of(pa)
    if pb is None:
        gap = 1
        while gap < len(pa) and ta[gap] - ta[0] < ms(min_separation):
            gap += 1
        found = runs(pa[:, :2], ua, tau=tau, min_gap=max(1, gap))
    else:
        found = runs(pa[:, :2], ua, pb[:, :2], (range_of(pb) >= flat).astype(np.uint8), tau=tau)
    segs = [s for s in bridge(found, ta, ms(max_gap)) if ta[s[0] + s[2] - 1] - ta[s[0]] >= ms(min_duration)]
    return keep_outermost(segs)


def report(files, tau=10, flat=16, min_duration=2.0, max_gap=0.5, min_separation=5.0):
    """files: [(name, prints uint64 [n, 4])] -> the list the verb writes"""
    out = []
    for x, (na, pa) in enumerate(files):
        for nb, pb in files[x:]:
            same = pb is pa
            tb = ms_of(pb)
            ta = ms_of(pa)
            for i, j, n in segments(pa, None if same else pb, tau, flat, min_duration, max_gap, min_separation):
                out.append({"a": na, "b": nb, "a_start": round(ta[i] / 1000.0, 3), "a_end": round(ta[i + n - 1] / 1000.0, 3),
                            "b_start": round(tb[j] / 1000.0, 3), "b_end": round(tb[j + n - 1] / 1000.0, 3), "frames": int(n),
                            "offset": int(j - i)})
    order = {name: k for k, (name, _) in enumerate(files)}
    out.sort(key=lambda s: (order[s["a"]], order[s["b"]], s["a_start"], s["offset"]))
    return out
