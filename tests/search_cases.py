"""Inputs of the search tests, shared by the CPU file (which checks their margins: that they tie, overflow the pending region, span
ranges) and the GPU file (which runs them).  All values are 5-decimal numbers."""
import numpy as np

UNIT = 1e-5


def blobs(seed, n, centres=6, spread=0.7, noise=0.15):
    """n descriptor-like rows around a few centres, as the 5-decimal text gives them back"""
    rng = np.random.default_rng(seed)
    c = spread * rng.standard_normal((centres, 128)) / np.sqrt(128.0)
    return np.round(c[rng.integers(0, centres, n)] + noise / np.sqrt(128.0) * rng.standard_normal((n, 128)), 5)


def ties(seed, n):
    """rows drawn from {0, 1e-5} per component: d2 to a zero query is the number of ones -- a few dozen values cover every row"""
    rng = np.random.default_rng(seed)
    return (rng.random((n, 128)) < 0.1).astype(np.float64) * UNIT


def identical(n):
    return np.tile(np.round(np.linspace(-0.2, 0.2, 128), 5), (n, 1))


def ladder(n, order, seed=0):
    """row i at distance (i + 1) units from the zero query, every d2 distinct; `order`: descending (every row beats the bound),
    ascending (nothing passes after the first k) or shuffled"""
    steps = np.arange(1, n + 1)
    if order == "descending":
        steps = steps[::-1]
    elif order == "shuffled":
        steps = np.random.default_rng(seed).permutation(steps)
    else:
        assert order == "ascending"
    X = np.zeros((n, 128))
    X[:, 0] = np.round(steps * UNIT, 5)
    return X


def groups_across_seams(n, seed=0):
    """row groups as runs of uneven lengths that cross 16-row blocks and range seams, some rows in no group (-1)"""
    rng = np.random.default_rng(seed)
    g = np.repeat(np.arange(n), rng.integers(1, 40, n))[:n].astype(np.int32)
    g[rng.random(n) < 0.1] = -1
    return g


def extreme():
    """+2^20 against -2^20 units in every component: d2 = 128 * (2^21)^2 = 2^49"""
    v = (1 << 20) * UNIT
    return np.full((1, 128), v), np.full((3, 128), -v)


def two_files(seed=11):
    """(time, track, X) of two small embedding files that share faces: what the verb tests write"""
    rng = np.random.default_rng(seed)
    c = 0.7 * rng.standard_normal((5, 128)) / np.sqrt(128.0)
    out = []
    for tracks in ([(0, 0, 7), (1, 1, 5), (2, 0, 4), (3, 2, 6)], [(0, 1, 6), (1, 3, 5), (5, 0, 8), (7, 4, 3)]):     # (track, person, rows)
        t, k, X = [], [], []
        for track, person, n in tracks:
            X.append(np.round(c[person] + 0.15 / np.sqrt(128.0) * rng.standard_normal((n, 128)), 5))
            t += [round(10.0 * track + 0.04 * j, 3) for j in range(n)]
            k += [track] * n
        out.append((np.array(t), np.array(k, np.int64), np.concatenate(X)))
    return out
