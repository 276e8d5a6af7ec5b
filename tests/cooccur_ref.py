"""The do-not-cooccur constraint restated in numpy (test infrastructure): average-linkage agglomeration in which a pair of clusters that
holds a co-occurring pair of tracks is never merged and never stops the loop.  [EXT pyannote.algorithms' DoNotCooccur, absent here; the
reference names it and leaves it off, clustering.py:142-143]

Deliberately NOT the product's formulation: the forbidden pairs are kept as a boolean mask beside finite distances (no +inf in the
matrix), the closest pair is a masked arg-min over the whole upper triangle (no cached row minima), the merged row is
(si * a + sj * b) / (si + sj) in float64 with one IEEE division (no reciprocal, no fma).

Also the seeded generator the CPU and the GPU tests share."""
import numpy as np

PRECISION = 1e-6          # pyannote.core's SEGMENT_PRECISION: a segment is non-empty when it is longer than this


def cooccur(extent):
    """bool [T, T]: tracks i != j whose extents [start, end] intersect, min(end_i, end_j) - max(start_i, start_j) > 1e-6 in float64"""
    e = np.asarray(extent, np.float64)
    s, t = e[:, 0], e[:, 1]
    m = (np.minimum(t[:, None], t[None, :]) - np.maximum(s[:, None], s[None, :])) > PRECISION
    np.fill_diagonal(m, False)
    return m


def n_blocked(extent):
    return int(np.triu(cooccur(extent), 1).sum())


def stamp(D, extent):
    """D with +inf in both mirror entries of every co-occurring pair (what the product's stamping kernel does): the matrix on which the
    UNCHANGED oracle agglomeration is a second reference at finite thresholds"""
    out = np.array(D, np.float64)
    out[cooccur(extent)] = np.inf
    return out


def hac(D, sizes, threshold, forbidden=None):
    """-> (labels int32 [T], log float64 [n, 4] = (kept, merged, distance, new size)); labels[t] = smallest track index of t's cluster.
    First minimum in row-major order over the pairs i < j that are alive and not forbidden; stops when none is left or the closest is
    above the threshold (threshold = +inf: runs until no mergeable pair is left)."""
    W = np.array(D, np.float64)
    T = len(W)
    F = np.zeros((T, T), bool) if forbidden is None else np.array(forbidden, bool)
    sz = np.asarray(sizes, np.float64).copy()
    alive = np.ones(T, bool)
    labels = np.arange(T, dtype=np.int32)
    log = []
    idx = np.arange(T)
    M = np.where(np.triu(np.ones((T, T), bool), 1) & ~F, W, np.inf)        # the candidates: inf = not one
    while T > 1:
        k = int(np.argmin(M))                                               # flat index of the FIRST minimum: row-major order
        i, j = divmod(k, T)
        d = M[i, j]
        if not np.isfinite(d) or d > threshold:
            break
        new = (sz[i] * W[i] + sz[j] * W[j]) / (sz[i] + sz[j])
        W[i, :] = new
        W[:, i] = new
        F[i, :] |= F[j, :]
        F[:, i] = F[i, :]
        sz[i] += sz[j]
        alive[j] = False
        M[j, :] = np.inf
        M[:, j] = np.inf
        ok = alive & ~F[i] & (idx != i)
        M[i, :] = np.where(ok & (idx > i), new, np.inf)
        M[:, i] = np.where(ok & (idx < i), new, np.inf)
        labels[labels == j] = i
        log.append((i, j, d, sz[i]))
    return labels, np.array(log, np.float64).reshape(-1, 4)


def violations(labels, extent):
    """co-occurring pairs of tracks (i < j) that share a label"""
    lab = np.asarray(labels)
    return int(np.triu(cooccur(extent) & (lab[:, None] == lab[None, :]), 1).sum())


def make(T, seed, identities=None, span=None):
    """-> (X float64 [N, 128] rounded to 5 decimals, row_start int32 [T + 1], extent float64 [T, 2]): tracks of 2-4 rows around a few
    identity centres at norm ~0.45 (rows of one identity ~0.3 apart, of two identities ~0.65: they bracket the reference's 0.6), extents
    of 0.5-2.5 s drawn over `span` seconds so that a few per cent of the pairs co-occur -- pairs of one identity among them."""
    rng = np.random.default_rng(seed)
    K = identities if identities is not None else max(2, T // 25)
    span = float(span if span is not None else 100.0)
    cent = rng.normal(size=(K, 128))
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    ident = rng.integers(0, K, T)
    rows = rng.integers(2, 5, T)
    row_start = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    x = cent[np.repeat(ident, rows)] + 0.04 * rng.normal(size=(int(row_start[-1]), 128))
    X = np.round(0.45 * x / np.linalg.norm(x, axis=1, keepdims=True), 5)
    start = np.round(rng.uniform(0.0, span, T), 3)
    extent = np.stack([start, start + np.round(rng.uniform(0.5, 2.5, T), 3)], axis=1)
    return X, row_start, extent


def disjoint_extents(T):
    """extents that never intersect (track k on [2 k, 2 k + 1])"""
    s = 2.0 * np.arange(T)
    return np.stack([s, s + 1.0], axis=1)
