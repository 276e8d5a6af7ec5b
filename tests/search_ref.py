"""The rules of SEARCH.md restated in numpy int64 -- what pvf_search is held to bit for bit -- and the host side of the `search` verb
(the merge of a multi-row query by the minimum over its rows, the collapse to tracks).  Nothing here imports the library."""
import numpy as np

Q_MAX = 1 << 20
NONE = -1
DEFAULT_CHUNK = 1 << 18
MIN_PENDING = 64
RANGE_MIN_BLOCKS = 16
TARGET_WORKGROUPS = 768
ARENA_MAX = 1 << 30


class Refused(ValueError):
    pass


def quantise(V, what="X"):
    """q(v) = rint(v * 100000.0) in float64, ties to even -> int64; a value that is not finite or has |q| > 2^20 refuses the whole array"""
    V = np.asarray(V, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(V * 100000.0)
        bad = ~(np.isfinite(V) & (np.abs(q) <= Q_MAX))
    if bad.any():
        r, c = np.argwhere(bad)[0]                      # row-major first
        raise Refused("%s[%d][%d]" % (what, r, c))
    return q.astype(np.int64)


def check_limits(Q, N, dim, k, max_d2, query_group, row_group):
    if dim != 128:
        raise Refused("dim")
    if Q < 1 or N < 1:
        raise Refused("Q and N")
    if not 1 <= k <= 1024:
        raise Refused("k")
    if N > 1 << 30:
        raise Refused("2^30 rows")
    if max_d2 < -1:
        raise Refused("max_d2")
    if (query_group is None) != (row_group is None):
        raise Refused("groups")


def d2_matrix(Qrows, X):
    """int64 [Q, N]: the exact squared distances (differences, squares, sums -- all in int64)"""
    qa, qb = quantise(Qrows, "Qrows"), quantise(X, "X")
    out = np.empty((len(qa), len(qb)), np.int64)
    for i, a in enumerate(qa):
        t = qb - a
        out[i] = (t * t).sum(1)
    return out


def search(Qrows, X, k, max_d2=-1, query_group=None, row_group=None):
    """-> (idx int32 [Q, k], d2 int64 [Q, k], count int32 [Q])"""
    Qrows, X = np.asarray(Qrows, np.float64), np.asarray(X, np.float64)
    check_limits(len(Qrows), len(X), X.shape[1], k, max_d2, query_group, row_group)
    D = d2_matrix(Qrows, X)
    Qn, N = D.shape
    idx, d2, count = np.full((Qn, k), NONE, np.int32), np.full((Qn, k), NONE, np.int64), np.zeros(Qn, np.int32)
    rows = np.arange(N)
    for q in range(Qn):
        keep = np.ones(N, bool)
        if query_group is not None and query_group[q] >= 0:
            keep &= np.asarray(row_group) != query_group[q]
        if max_d2 >= 0:
            keep &= D[q] <= max_d2
        i = rows[keep]
        order = np.lexsort((i, D[q][i]))[:k]
        n = len(order)
        idx[q, :n], d2[q, :n], count[q] = i[order], D[q][i][order], n
    return idx, d2, count


def plan(Q, N, k, chunk=None):
    """how the library cuts a call (csrc/search.hip, search_plan): chunk_rows, n_chunks, n_ranges, range_blocks, pending"""
    chunk = DEFAULT_CHUNK if not chunk or chunk <= 0 else min(chunk, 1 << 22)
    chunk = (min(chunk, N) + 15) // 16 * 16
    kp = MIN_PENDING
    while kp < k:
        kp *= 2
    nbq = (Q + 15) // 16
    row_groups = (nbq + 3) // 4
    nb = chunk // 16
    r = max(1, min(TARGET_WORKGROUPS // row_groups, (nb + RANGE_MIN_BLOCKS - 1) // RANGE_MIN_BLOCKS))
    while r > 1 and nbq * 16 * r * 2 * kp * 12 > ARENA_MAX:
        r = (r + 1) // 2
    range_blocks = (nb + r - 1) // r
    n_ranges = (nb + range_blocks - 1) // range_blocks
    return dict(chunk_rows=chunk, n_chunks=(N + chunk - 1) // chunk, n_ranges=n_ranges, range_blocks=range_blocks, pending=kp,
                arena_bytes=nbq * 16 * n_ranges * 2 * kp * 12)


def compactions(d2_row, k, first_row, last_row, pending):
    """how often the kernel sorts the list of one query inside the table rows [first_row, last_row) (one range of one chunk; first_row a
    multiple of 16): the selection restated -- a row passes when its d2 is below the k-th listed one, a 16-row tile is appended as a
    whole, the list is compacted when fewer than 16 pending entries are free, and once more at the end if anything is pending"""
    lst, pend, n = [], [], 0
    for b0 in range(first_row, last_row, 16):
        bound = lst[k - 1] if len(lst) == k else None
        pend += [int(v) for v in d2_row[b0:min(b0 + 16, last_row)] if bound is None or v < bound]
        if len(pend) + 16 > pending:
            lst, pend, n = sorted(lst + pend)[:k], [], n + 1
    return n + (1 if pend else 0)


# ---- the host side of the verb ----------------------------------------------------------------------------------------------------------
def merge_min(idx, d2, count, k):
    """the lists of the rows of ONE query -> [(d2, i)]: per table row its smallest d2 over the query rows, ordered by (d2, i), the first
    k.  Exact: a row among the k best by the minimum is among the k best of the query row that attains it."""
    best = {}
    for q in range(len(count)):
        for j in range(int(count[q])):
            i, d = int(idx[q, j]), int(d2[q, j])
            if i not in best or d < best[i]:
                best[i] = d
    return sorted((d, i) for i, d in best.items())[:k]


def merge_brute(Qrows, X, k, max_d2=-1, skip=None):
    """the same from the full matrix: min over the query rows, then (d2, i)"""
    D = d2_matrix(Qrows, X).min(0)
    rows = [i for i in range(len(D)) if (skip is None or not skip[i]) and (max_d2 < 0 or D[i] <= max_d2)]
    return sorted((int(D[i]), i) for i in rows)[:k]


def collapse(hits, owner):
    """the best hit of each owner (a (file, track) pair) among the hits, in the order of their nearest face"""
    seen, out = set(), []
    for d, i in hits:
        if owner[i] not in seen:
            seen.add(owner[i])
            out.append((d, i))
    return out


def line(rank, d2, path, track, t):
    return "%d %.5f %s %d %.3f\n" % (rank, np.sqrt(float(d2)) / 1e5, path, track, t)
