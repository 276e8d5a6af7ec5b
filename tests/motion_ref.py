"""MOTION.md restated in numpy and plain Python, independently of pyannote_video_amd/motion.py and csrc/motion.hip: the motion row of a
pair's flow (quantiser, coordinates, integer least squares, trimmed rounds, the row's words) and the `camera` rules.  The row exists in
two number systems that share one text: int64 arrays, which is what the kernel computes in, and Python ints (object arrays), which cannot
wrap and which record the largest intermediate -- tests/test_motion_ref.py proves with them that nothing reaches 2^63 at the caps.  The
GPU tests hold the kernel to this with np.array_equal; the CPU tests hold this to hand cases and show that planted defects are seen."""
import numpy as np

ROUNDS = 4
TAU_MIN = 16 << 16
Q_MAX = 1 << 20
MAX_PIXELS = 16384
MIN_SIDE, MAX_SIDE = 12, 256
WORDS = 10
DEFECTS = ("components_swapped", "x_not_centred", "truncating_division", "no_trimming", "tau_without_floor", "round_half_up",
           "one_round_fewer", "n_in_from_next_set")
LIMIT = 1 << 63


class Overflow(AssertionError):
    pass


class Track(object):
    """the largest magnitude of every named intermediate"""

    def __init__(self):
        self.most = {}

    def see(self, name, value):
        self.most[name] = max(self.most.get(name, 0), int(value))


def quantise(flow, defect=None):
    """float32 [h, w, 2] -> (valid bool [h, w], u, v int64 [h, w] in 1/64 pixel; 0 where invalid)"""
    f = np.asarray(flow, np.float32)
    assert f.ndim == 3 and f.shape[2] == 2
    valid = np.isfinite(f[..., 0]) & np.isfinite(f[..., 1])
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.clip(f * np.float32(64.0), np.float32(-Q_MAX), np.float32(Q_MAX))      # float32 throughout
    assert s.dtype == np.float32
    s = np.where(valid[..., None], s, np.float32(0))
    q = (np.floor(s.astype(np.float64) + 0.5) if defect == "round_half_up" else np.rint(s)).astype(np.int64)
    u, v = q[..., 0], q[..., 1]
    return (valid, v, u) if defect == "components_swapped" else (valid, u, v)


def coordinates(h, w, defect=None):
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    return (2 * x if defect == "x_not_centred" else 2 * x - (w - 1)), 2 * y - (h - 1)


class _Numbers(object):
    """the arithmetic of one row: every intermediate passes through `s` (a scalar) or `a` (an array), which refuse 2^63 and record"""

    def __init__(self, ints, track, defect):
        self.ints, self.track, self.defect = ints, track, defect

    def s(self, name, value):
        value = int(value)
        if abs(value) >= LIMIT and not self.ints:
            raise Overflow("%s = %d does not fit int64" % (name, value))
        if self.track is not None:
            self.track.see(name, abs(value))
        return value

    def a(self, name, arr):
        if arr.size and self.track is not None:
            self.track.see(name, max(abs(int(arr.min())), abs(int(arr.max()))))
        return arr

    def array(self, arr):
        return arr.astype(object) if self.ints else arr.astype(np.int64)

    def total(self, name, arr):
        return self.s(name, arr.sum()) if arr.size else 0

    def div(self, a, b):
        """floor(a / b), b > 0"""
        assert b > 0
        if self.defect == "truncating_division":
            return abs(a) // b * (1 if a >= 0 else -1)
        return a // b

    def div16(self, name, num, den):
        """floor(num 2^16 / den): quotient and remainder first"""
        q = self.div(num, den)
        r = self.s(name + ".rem", num - self.s(name + ".q*den", q * den))
        out = self.s(name + ".q<<16", q << 16) + self.div(self.s(name + ".rem<<16", r << 16), den)
        if self.defect is None:
            assert out == (num << 16) // den
        return self.s(name, out)


def _fit(N, X, Y, u, v):
    """the model (TX16, TY16, A16, B16) of the pixels given, and their count"""
    s = N.s
    n = len(X)
    SX, SY, ZZ = N.total("SX", X), N.total("SY", Y), N.total("ZZ", N.a("X2+Y2", X * X + Y * Y))
    Su, Sv = N.total("Su", u), N.total("Sv", v)
    Pp = N.total("Pp", N.a("Xu+Yv", N.a("Xu", X * u) + N.a("Yv", Y * v)))
    Qq = N.total("Qq", N.a("Xv-Yu", N.a("Xv", X * v) - N.a("Yu", Y * u)))
    den = s("den", s("n*ZZ", n * ZZ) - s("SX^2", SX * SX) - s("SY^2", SY * SY))
    assert den >= 0
    A = B = 0
    if den != 0:
        A = N.div16("A16", s("numA", s("n*Pp", n * Pp) - s("SXSu+SYSv", s("SX*Su", SX * Su) + s("SY*Sv", SY * Sv))), den)
        B = N.div16("B16", s("numB", s("n*Qq", n * Qq) - s("SXSv-SYSu", s("SX*Sv", SX * Sv) - s("SY*Su", SY * Su))), den)
    TX = N.div(s("numTX", s("TX.2", s("TX.1", s("Su<<16", Su << 16) - s("A*SX", A * SX)) + s("B*SY", B * SY)) + (n >> 1)), n)
    TY = N.div(s("numTY", s("TY.2", s("TY.1", s("Sv<<16", Sv << 16) - s("B*SX", B * SX)) - s("A*SY", A * SY)) + (n >> 1)), n)
    return (s("TX16", TX), s("TY16", TY), A, B), n


def _residuals(N, model, X, Y, u, v):
    TX, TY, A, B = model
    a = N.a
    ru = abs(a("du", a("u<<16", u * 65536) - a("u^", a("TX+AX", TX + a("A*X", A * X)) - a("B*Y", B * Y))))
    rv = abs(a("dv", a("v<<16", v * 65536) - a("v^", a("TY+BX", TY + a("B*X", B * X)) + a("A*Y", A * Y))))
    return ru, rv


def row_of(flow, dfd_bits=0, ints=False, track=None, defect=None):
    """int64 [10]: the motion row of one flow float32 [h, w, 2]; word 8 is 0"""
    flow = np.asarray(flow, np.float32)
    h, w = flow.shape[:2]
    assert MIN_SIDE <= w <= MAX_SIDE and MIN_SIDE <= h <= MAX_SIDE and w * h <= MAX_PIXELS, "outside the caps nothing is promised"
    N = _Numbers(ints, track, defect)
    valid, u, v = quantise(flow, defect)
    X, Y = coordinates(h, w, defect)
    keep = valid.reshape(-1)
    X, Y, u, v = (N.array(t.reshape(-1)[keep]) for t in (X, Y, u, v))          # the valid pixels, from here on
    row = np.zeros(WORDS, np.int64)
    row[7], row[9] = dfd_bits, w | h << 16
    n_valid = len(X)
    row[0] = n_valid
    if n_valid == 0:
        return row
    mag = N.total("mag", abs(u) + abs(v))
    S = np.ones(n_valid, bool)
    model, n_in, m, total = None, 0, 0, 0
    for k in range(ROUNDS - (1 if defect == "one_round_fewer" else 0)):
        if k > 0:
            tau = max(TAU_MIN, N.div(total, n_in) if defect == "tau_without_floor" else 2 * m)
            ru, rv = _residuals(N, model, X, Y, u, v)
            S_next = np.ones(n_valid, bool) if defect == "no_trimming" else np.asarray(np.maximum(ru, rv) <= tau, bool)
            if S_next.sum() < 3:
                break
            S = S_next
        model, n_in = _fit(N, X[S], Y[S], u[S], v[S])
        ru, rv = _residuals(N, model, X[S], Y[S], u[S], v[S])
        total = N.s("sum ru+rv", N.total("sum ru", ru) + N.total("sum rv", rv))
        m = N.div(total, 2 * n_in)
    if defect == "n_in_from_next_set":
        ru, rv = _residuals(N, model, X, Y, u, v)
        n_in = int((np.maximum(ru, rv) <= max(TAU_MIN, 2 * m)).sum())
    row[0] = n_valid | n_in << 32
    row[1:5] = model
    row[5], row[6] = m, mag
    return row


def rows_of(flows, dfd=None, **kw):
    """int64 [n, 10] of flows float32 [n, h, w, 2]; dfd float64 [n] -> word 7 holds its bits"""
    bits = np.zeros(len(flows), np.int64) if dfd is None else np.ascontiguousarray(dfd, np.float64).view(np.int64)
    return np.stack([row_of(f, int(b), **kw) for f, b in zip(flows, bits)]) if len(flows) else np.zeros((0, WORDS), np.int64)


def unpack(row):
    """dict of a row's fields"""
    r = [int(x) for x in row]
    return dict(n_valid=r[0] & 0xFFFFFFFF, n_in=r[0] >> 32, TX16=r[1], TY16=r[2], A16=r[3], B16=r[4], m=r[5], mag=r[6], dfd_bits=r[7],
                ms=r[8] & 0xFFFFFFFF, index=r[8] >> 32, w=r[9] & 0xFFFF, h=r[9] >> 16)


# ---- the file of the `motion` verb -----------------------------------------------------------------------------------------------------
def ms(t):
    return int(round(float(t) * 1000.0))


def stamp(rows, fps, first=0):
    rows = np.array(rows, np.int64)
    for k in range(len(rows)):
        rows[k, 8] = ms((first + k) / float(fps)) | (first + k) << 32
    return rows


def tile_size(width, w, h):
    return int(width), max(1, (2 * int(width) * int(h) + int(w)) // (2 * int(w)))


def video_rows(flows, dfd, tw, th, fps, first=0):
    """what `motion` writes for a video whose consecutive small images have these flows: a first row without valid pixels, then the
    pairs' rows, stamped"""
    head = np.zeros((1, WORDS), np.int64)
    head[0, 9] = tw | th << 16
    return stamp(np.concatenate([head, rows_of(flows, dfd)]), fps, first)


# ---- the `camera` rules ----------------------------------------------------------------------------------------------------------------
MOVING = ("pan-left", "pan-right", "tilt-up", "tilt-down", "zoom-in", "zoom-out")
KINDS = MOVING + ("static",)


def scaled(x, unit):
    return int(np.floor(unit * float(x) + 0.5))


def ratio_half_up(a, b):
    """floor(a / b + 1/2), b > 0"""
    return (2 * a + b) // (2 * b)


def frame_rates(row):
    """(pan, tilt, zoom, roll) of one row per frame, in thousandths"""
    f = unpack(row)
    return (ratio_half_up(1000 * f["TX16"], f["w"] << 22), ratio_half_up(1000 * f["TY16"], f["h"] << 22),
            ratio_half_up(1000 * f["A16"], 1 << 21), ratio_half_up(1000 * f["B16"], 1 << 21))


def shot_of(t_ms, shots_ms):
    for k, (a, b) in enumerate(shots_ms):
        if a <= t_ms < b:
            return k
    return -1


def camera(rows, pan=5.0, zoom=3.0, window=0.5, min_inliers=50, min_duration=0.5, max_gap=0.2, shots=None):
    """-> [(kind, s, e, rate)] in row indices, by (s, e, kind)"""
    pan10, zoom10, inl = scaled(pan, 10), scaled(zoom, 10), int(min_inliers)
    assert pan10 >= 1 and zoom10 >= 1
    n = len(rows)
    f = [unpack(r) for r in rows]
    t = [x["ms"] for x in f]
    shots_ms = None if shots is None else [(ms(a), ms(b)) for a, b in shots]
    shot = [0 if shots_ms is None else shot_of(t[i], shots_ms) for i in range(n)]
    ok = [i > 0 and f[i]["n_valid"] > 0 and 100 * f[i]["n_in"] >= inl * f[i]["n_valid"] and shot[i] >= 0 and shot[i] == shot[i - 1]
          for i in range(n)]
    per = [frame_rates(r) for r in rows]
    wms = ms(window)
    label, value = [None] * n, [0] * n
    for i in range(n):
        if not ok[i]:
            continue
        inside = [j for j in range(n) if ok[j] and shot[j] == shot[i] and 2 * abs(t[j] - t[i]) <= wms]
        D = sum(t[j] - t[j - 1] for j in inside)
        rate = [ratio_half_up(1000 * sum(per[j][q] for j in inside), D) if D > 0 else 0 for q in range(3)]
        thr = (pan10, pan10, zoom10)
        best = 0
        for q in (1, 2):                         # the largest |rate| / threshold; the earlier quantity keeps a tie
            if abs(rate[q]) * thr[best] > abs(rate[best]) * thr[q]:
                best = q
        if abs(rate[best]) >= thr[best]:
            label[i], value[i] = MOVING[2 * best + (0 if rate[best] > 0 else 1)], rate[best]
        else:
            label[i] = "static"
    gap_ms, least = ms(max_gap), ms(min_duration)
    out = []
    for kind in KINDS:
        runs = []
        i = 0
        while i < n:
            if label[i] != kind:
                i += 1
                continue
            a = i
            while i + 1 < n and label[i + 1] == kind:
                i += 1
            if runs and shot[runs[-1][1]] == shot[a] and t[a] - t[runs[-1][1]] <= gap_ms:
                runs[-1] = (runs[-1][0], i)
            else:
                runs.append((a, i))
            i += 1
        for a, b in runs:
            if t[b] - t[a] < least:
                continue
            mine = [value[j] for j in range(a, b + 1) if label[j] == kind]
            out.append((kind, a, b, ratio_half_up(sum(mine), len(mine))))
    return sorted(out, key=lambda r: (r[1], r[2], KINDS.index(r[0])))


def camera_report(rows, **kw):
    return [{"kind": k, "start": round((int(rows[s, 8]) & 0xFFFFFFFF) / 1000.0, 3), "end": round((int(rows[e, 8]) & 0xFFFFFFFF) / 1000.0, 3),
             "first": int(rows[s, 8]) >> 32, "last": int(rows[e, 8]) >> 32, "rate": rate} for k, s, e, rate in camera(rows, **kw)]


def frames_in_motion(rows, **kw):
    """the frame indices that lie inside a pan, tilt or zoom span of the file under the default rules"""
    inside = set()
    for k, s, e, _ in camera(rows, **kw):
        if k in MOVING:
            inside.update(range(int(rows[s, 8]) >> 32, (int(rows[e, 8]) >> 32) + 1))
    return inside
