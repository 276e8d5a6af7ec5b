"""Inputs of the cast tests, shared by the CPU file (which checks what they are meant to be: a path's diameter, purity of the planted
identities under the restatement) and the GPU file (which runs them).  All values are 5-decimal numbers."""
import numpy as np
from tests import search_cases

UNIT = 1e-5
DEFAULT_MAX_D2 = 60000 ** 2              # --max-distance 0.6
PLANTED = [(600, 6, 20), (1500, 40, 32), (300, 30, 64)]          # (rows, identities, k): the three configurations of CAST.md section 7
PATHS = [(257, 4), (1025, 8)]                                    # (points, k), threshold 1/1, no cut


def path(n):
    """n points on a line, 100 units apart: row i's list is i-1, i+1, i-2, i+2, ... and the graph's diameter in rows is n - 1"""
    X = np.zeros((n, 128))
    X[:, 0] = np.round(np.arange(n) * 100 * UNIT, 5)
    return X


def links_across(idx, count):
    """how many list entries a breadth-first walk from row 0 needs to reach the farthest row, the lists taken as undirected edges:
    the least number of rounds of a labelling that moves one link a round"""
    n = len(idx)
    near = [set() for _ in range(n)]
    for a in range(n):
        for b in idx[a, :count[a]]:
            near[a].add(int(b))
            near[int(b)].add(a)
    depth, front = {0: 0}, [0]
    while front:
        reached = []
        for a in front:
            for b in near[a]:
                if b not in depth:
                    depth[b] = depth[a] + 1
                    reached.append(b)
        front = reached
    return max(depth.values())


def path_links_across(n, k):
    """a lower bound for links_across on path(n): an entry spans at most k / 2 rows, but for the lists of the k rows at either end"""
    return (n - 1 - 2 * k) // (k // 2)


def planted(seed, n, identities):
    """-> (X, identity of every row): equal shares, within an identity about 0.2 apart, between identities about 1.0, rows shuffled"""
    rng = np.random.default_rng(seed)
    c = 0.7 * rng.standard_normal((identities, 128)) / np.sqrt(128.0)
    who = rng.permutation(np.arange(n) % identities)
    return np.round(c[who] + 0.14 / np.sqrt(128.0) * rng.standard_normal((n, 128)), 5), who


def pure_and_complete(labels, who):
    """every component holds one identity and every identity lies in one component"""
    pairs = set(zip((int(l) for l in labels), (int(w) for w in who)))
    return len(pairs) == len(set(l for l, _ in pairs)) == len(set(w for _, w in pairs))


def groups_in_runs(n, seed=0):
    """must-link groups as runs of uneven length (some rows in none), numbered by a row of ANOTHER group where possible: a group's
    number says nothing about its rows"""
    g = search_cases.groups_across_seams(n, seed)
    ids = np.unique(g[g >= 0])
    return np.where(g >= 0, (n - 1) - np.searchsorted(ids, g), -1).astype(np.int32)


def scattered_groups(n, seed=0, groups=7):
    """groups whose rows lie all over the table, so that they cross every query batch"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, groups, n).astype(np.int32)
    g[rng.random(n) < 0.5] = -1
    return g


def distinct_rows(n):
    """rows that are pairwise different: a cut of 0 leaves every list empty"""
    X = np.zeros((n, 128))
    X[:, 1] = np.round(np.arange(n) * UNIT, 5)
    return X
