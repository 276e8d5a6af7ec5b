"""Identification against a gallery, restated in numpy float64 with no dependency on the library: the T x K block means of pairwise
distances and the decision per group (include/pvface.h states the rules), plus the inputs the CPU and the GPU tests share."""
import numpy as np

# the shapes of the main distance case: groups start and end on, before and after the 16-row seams, span 2 to 4 blocks on both sides,
# singletons sit next to long groups, K = 17 is no multiple of 16
QUERY_SIZES = [1, 1, 2, 15, 16, 17, 3, 31, 32, 33, 1, 48, 5, 7, 16, 16, 1, 9, 64, 2]       # N = 320
IDENTITY_SIZES = [1, 16, 17, 2, 33, 15, 1, 40, 3, 16, 5, 1, 30, 2, 7, 11, 1]               # M = 201
N_CENTRES = 23                                      # centres 17 .. 22 are in nobody's gallery


def starts(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def mean_dist(X, row_start, G, gal_start, metric=0):
    """D[t][k] = plain mean over the rows of group t and of identity k of the pair distance (0 Euclidean; 1 cosine, 0 at zero norms)"""
    X, G = np.asarray(X, np.float64), np.asarray(G, np.float64)
    T, K = len(row_start) - 1, len(gal_start) - 1
    D = np.zeros((T, K), np.float64)
    for t in range(T):
        x = X[row_start[t]:row_start[t + 1]]
        for k in range(K):
            g = G[gal_start[k]:gal_start[k + 1]]
            if metric == 0:
                d = np.sqrt(((x[:, None] - g[None]) ** 2).sum(-1))
            else:
                den = np.sqrt((x * x).sum(-1))[:, None] * np.sqrt((g * g).sum(-1))[None]
                with np.errstate(divide="ignore", invalid="ignore"):
                    d = np.where(den > 0, 1.0 - (x @ g.T) / den, 0.0)
            D[t, k] = d.mean()
    return D


def pick(D, threshold):
    """(best, best_dist, second, second_dist) per row.  An entry is taken when it is below +inf (NaN and +inf are never taken); best is
    the first minimum of the taken entries, second the first minimum over k != best; nothing to take gives (-1, +inf); then best = -1
    unless best_dist <= threshold, best_dist keeping the measured value."""
    D = np.asarray(D, np.float64)
    T = D.shape[0]
    best, second = np.full(T, -1, np.int32), np.full(T, -1, np.int32)
    bd, sd = np.full(T, np.inf), np.full(T, np.inf)
    for t in range(T):
        row = D[t]
        with np.errstate(invalid="ignore"):
            taken = np.flatnonzero(row < np.inf)
        if len(taken) == 0:
            continue
        b = int(taken[np.argmin(row[taken])])           # (argmin: the first occurrence)
        bd[t] = row[b]
        rest = taken[taken != b]
        if len(rest):
            s = int(rest[np.argmin(row[rest])])
            second[t], sd[t] = s, row[s]
        if bd[t] <= threshold:
            best[t] = b
    return best, bd, second, sd


def main_case():
    """rows = round(centre + N(0, 0.15^2 / 128), 5), centres = 0.7 N(0, 1) / sqrt(128), default_rng(7); query group i takes centre
    (5 i) mod 23, identity k centre k -> (X, row_start, G, gal_start)"""
    rng = np.random.default_rng(7)
    centres = 0.7 * rng.standard_normal((N_CENTRES, 128)) / np.sqrt(128.0)
    sigma = 0.15 / np.sqrt(128.0)
    X = np.concatenate([centres[(5 * i) % N_CENTRES] + sigma * rng.standard_normal((n, 128)) for i, n in enumerate(QUERY_SIZES)])
    G = np.concatenate([centres[k] + sigma * rng.standard_normal((n, 128)) for k, n in enumerate(IDENTITY_SIZES)])
    return np.round(X, 5), starts(QUERY_SIZES), np.round(G, 5), starts(IDENTITY_SIZES)


def main_case_truth():
    """the identity each query group of main_case was drawn around, -1 for the centres nobody enrolled"""
    c = [(5 * i) % N_CENTRES for i in range(len(QUERY_SIZES))]
    return np.array([k if k < len(IDENTITY_SIZES) else -1 for k in c], np.int32)


NAN, INF = float("nan"), float("inf")
ULP_ABOVE = float(np.nextafter(0.6, 1.0))
# (matrix, threshold, best, best_dist, second, second_dist) -- NaN in an expected distance is never used: expectations hold values of D
HAND_MADE = [
    ("exact ties: the lowest index wins, the runner-up is the next of them",
     [[0.5, 0.25, 0.25, 0.25], [0.3, 0.3, 0.7, 0.1]], 0.6, [1, 3], [0.25, 0.1], [2, 0], [0.25, 0.3]),
    ("a distance exactly at the threshold matches, one ulp above it does not",
     [[0.6, 0.9, 1.0], [ULP_ABOVE, 0.9, 1.0], [1.0, 0.6, ULP_ABOVE]], 0.6, [0, -1, 1], [0.6, ULP_ABOVE, 0.6], [1, 1, 2], [0.9, 0.9, ULP_ABOVE]),
    ("a NaN entry is never taken",
     [[NAN, 0.4, 0.2], [0.1, NAN, 0.5], [0.2, 0.1, NAN]], 0.6, [2, 0, 1], [0.2, 0.1, 0.1], [1, 2, 0], [0.4, 0.5, 0.2]),
    ("an all-NaN row, and a row with one entry to take",
     [[NAN, NAN, NAN], [NAN, 0.3, NAN]], 0.6, [-1, 1], [INF, 0.3], [-1, -1], [INF, INF]),
    ("K = 1",
     [[0.2], [0.7], [NAN]], 0.6, [0, -1, -1], [0.2, 0.7, INF], [-1, -1, -1], [INF, INF, INF]),
    ("+inf entries are not taken either, -inf is the smallest value",
     [[INF, 0.5, INF], [INF, INF, INF], [0.1, -INF, INF]], 0.6, [1, -1, 1], [0.5, INF, -INF], [-1, -1, 0], [INF, INF, 0.1]),
    ("an infinite threshold takes every measured distance, a negative one none",
     [[5.0, 7.0], [INF, NAN]], INF, [0, -1], [5.0, INF], [1, -1], [7.0, INF]),
    ("a negative threshold", [[0.0, 0.1]], -1.0, [-1], [0.0], [1], [0.1]),
]


def random_matrix(T, K, seed):
    """values on a grid of 1 / 8 so that ties are common, with NaN and +inf entries and one row of each kind of nothing"""
    rng = np.random.default_rng(seed)
    D = rng.integers(0, 12, (T, K)) / 8.0
    D[rng.random((T, K)) < 0.1] = np.nan
    D[rng.random((T, K)) < 0.1] = np.inf
    if T > 2:
        D[T - 1] = np.nan
        D[T - 2] = np.inf
    return D


def same_picks(got, want):
    """bit-exact equality of two (best, best_dist, second, second_dist)"""
    return all(np.array_equal(np.asarray(g).view(np.int32 if i % 2 == 0 else np.int64), np.asarray(w).view(np.int32 if i % 2 == 0 else np.int64))
               for i, (g, w) in enumerate(zip(got, want)))


def as_picks(best, best_dist, second, second_dist):
    return (np.asarray(best, np.int32), np.asarray(best_dist, np.float64), np.asarray(second, np.int32), np.asarray(second_dist, np.float64))
