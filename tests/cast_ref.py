"""The rules of CAST.md restated in numpy int64 and Python sets -- what pvf_cast is held to bit for bit -- and a plain loop that does
what the `cast` verb does.  Nothing here imports the library.

The squared distances come from the Gram form in float64: every term is an integer below 2^49 (SEARCH.md section 2), so the matrix product
is exact whatever the order of its additions, and it equals search_ref.d2_matrix (tests/test_cast_ref.py compares them)."""
import numpy as np
from tests import search_ref

NONE = -1
MAX_N, MAX_K, MAX_FRAC = 1 << 24, 256, 1 << 20
_FAR = np.int64(1) << 62


class Refused(ValueError):
    pass


def check_limits(N, dim, k, max_d2, num, den, group):
    if dim != 128:
        raise Refused("dim")
    if not 1 <= N <= MAX_N:
        raise Refused("N")
    if not 1 <= k <= MAX_K:
        raise Refused("k")
    if max_d2 < -1:
        raise Refused("max_d2")
    if not 0 <= num <= MAX_FRAC:
        raise Refused("num")
    if not 1 <= den <= MAX_FRAC:
        raise Refused("den")
    if group is not None and (np.asarray(group) >= N).any():
        raise Refused("group")


def d2_matrix(X):
    """int64 [N, N]: the exact squared distances of the quantised rows"""
    try:
        q = search_ref.quantise(X, "X").astype(np.float64)
    except search_ref.Refused as e:
        raise Refused(str(e))
    n = (q * q).sum(1)
    return (n[:, None] + n[None, :] - 2.0 * (q @ q.T)).astype(np.int64)


def lists(X, k, max_d2=-1, group=None):
    """-> (idx int32 [N, k], d2 int64 [N, k], count int32 [N]): section 2.  Row a's list: (d2, row) ascending, the first k, under the cut,
    without a and without the rows of a's non-negative group."""
    X = np.asarray(X, np.float64)
    N = len(X)
    check_limits(N, X.shape[1], k, max_d2, 0, 1, group)
    D = d2_matrix(X)
    out = np.eye(N, dtype=bool)
    if group is not None:
        g = np.asarray(group, np.int64)
        out |= (g[:, None] == g[None, :]) & (g[:, None] >= 0)
    if max_d2 >= 0:
        out |= D > max_d2
    Dm = np.where(out, _FAR, D)
    order = np.argsort(Dm, axis=1, kind="stable")[:, :k]          # stable: equal distances keep the order of their rows
    d = np.take_along_axis(Dm, order, 1)
    hit = d < _FAR
    idx, d2 = np.full((N, k), NONE, np.int32), np.full((N, k), NONE, np.int64)
    kk = order.shape[1]
    idx[:, :kk], d2[:, :kk] = np.where(hit, order, NONE), np.where(hit, d, NONE)
    return idx, d2, hit.sum(1).astype(np.int32)


def _miss(Lx, Ly_set, y):
    """miss(x -> y): section 3"""
    p = Lx.index(y) + 1 if y in Lx else len(Lx)
    return len(set(Lx[:p]) - Ly_set - {y})


def links(idx, count, num, den):
    """-> (m int32 [N, k], r int32 [N, k], linked uint8 [N, k]) per (a, slot); -1, -1, 0 past the list"""
    N, k = idx.shape
    L = [[int(v) for v in idx[a, :count[a]]] for a in range(N)]
    S = [set(l) for l in L]
    m, r, linked = np.full((N, k), NONE, np.int32), np.full((N, k), NONE, np.int32), np.zeros((N, k), np.uint8)
    for a in range(N):
        for s, b in enumerate(L[a]):
            ranks = [s + 1] + ([L[b].index(a) + 1] if a in S[b] else [])
            mm = _miss(L[a], S[b], b) + _miss(L[b], S[a], a)
            rr = min(ranks)
            m[a, s], r[a, s], linked[a, s] = mm, rr, int(mm * den <= num * rr)
    return m, r, linked


def labels(idx, linked, group=None):
    """-> (label int32 [N], number of components): section 4, by union-find; the label is the smallest row of the component"""
    N = len(idx)
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(x, y):
        x, y = find(x), find(y)
        if x != y:
            parent[max(x, y)] = min(x, y)

    if group is not None:
        first = {}
        for i, g in enumerate(group):
            if g >= 0:
                union(i, first.setdefault(int(g), i))
    for a, s in zip(*np.nonzero(linked)):
        union(int(a), int(idx[a, s]))
    lab = np.array([find(i) for i in range(N)], np.int32)
    return lab, int((lab == np.arange(N)).sum())


def cast(X, k, max_d2=-1, num=2000, den=1000, group=None):
    """-> (labels, n_components): the whole call"""
    X = np.asarray(X, np.float64)
    check_limits(len(X), X.shape[1], k, max_d2, num, den, group)
    idx, _, count = lists(X, k, max_d2, group)
    _, _, linked = links(idx, count, num, den)
    return labels(idx, linked, group)


# ---- the host side of the verb ----------------------------------------------------------------------------------------------------------
def track_mean(q):
    """the integer mean of a track's quantised rows (int64 [n, 128]) per column: (2 S + n) // (2 n), flooring"""
    q = np.asarray(q, np.int64)
    n = len(q)
    return (2 * q.sum(0) + n) // (2 * n)


def verb(files, k, max_d2, num, den, by, cast_fn=cast):
    """files: [(path, track int64 [n], X [n, 128])] in command-line order -> [(path, track, person)], by file then track; persons are
    numbered 0, 1, ... by ascending label"""
    keys, key_of = [], {}
    for f, (_, track, _) in enumerate(files):
        for t in sorted(set(int(t) for t in track)):
            key_of[(f, t)] = len(keys)
            keys.append((f, t))
    if by == "track":
        rows = []
        for f, t in keys:
            _, track, X = files[f]
            rows.append(track_mean(search_ref.quantise(X[track == t])) / 1e5)
        lab, _ = cast_fn(np.array(rows), k, max_d2, num, den, None)
        node_label = [int(v) for v in lab]
    else:
        X = np.concatenate([x for _, _, x in files])
        group = np.array([key_of[(f, int(t))] for f, (_, track, _) in enumerate(files) for t in track], np.int32)
        lab, _ = cast_fn(X, k, max_d2, num, den, group)
        node_label = [int(lab[np.nonzero(group == g)[0][0]]) for g in range(len(keys))]
    person = {l: i for i, l in enumerate(sorted(set(node_label)))}
    return [(files[f][0], t, person[node_label[g]]) for g, (f, t) in enumerate(keys)]
