"""The cases that the tests of the two mean-distance tile kernels share (tests/test_identify_cases.py on the CPU,
tests/test_gpu_identify_layouts.py on the GPU): cross_tiles_k of csrc/identify.hip and pair_tiles_k of csrc/cluster.hip (K10).  No
dependency on the library.

  * THE LADDER: pairs of descriptor rows at chosen values of rho = d^2 / (|a|^2 + |b|^2), the quantity both kernels compare with
    GRAM_SWITCH (csrc/pvf_internal.h) to decide between the Gram form |a|^2 + |b|^2 - 2 a.b and the summed differences.  The base rows are
    real descriptors (tests/golden/c3_clip0.npz, norms 6.2 to 11.8), and once more scaled to |x| = 0.55, the scale of every older table.
    Every pair is a one-row group against a one-row identity, so no mean dilutes its error.
  * GALLERY and QUERY LAYOUTS: size lists whose column ranges are stated (identify.hip's two numbers on 256 compute units; the CPU test
    asserts them from the real csrc/group_blocks.h), with copies and near-copies of gallery rows planted in the query table.
  * THE HUGE-T CASE: more than 65 535 query groups, the slicing of cross_norm_k.
References: squared differences summed in np.longdouble for the ladder; a vectorised float64 reference for the layouts (mean_dist_fast),
which the CPU test proves equal to the loop of tests/identify_ref.py."""
import os

import numpy as np

from tests import cluster_cases as cc
from tests import identify_ref

HERE = os.path.dirname(os.path.abspath(__file__))
N_CU = cc.N_CU                               # compute units of the device the expected ranges are stated for
SWITCHES = (1e-5, 1e-4, 1e-3, 1e-2)          # the value GRAM_SWITCH had first, and the powers of ten it could move to


def identify_wanted(nb_query, nb_gallery, n_cu=N_CU):
    """the two numbers identify.hip passes to cut_ranges: (wanted ranges, floor)"""
    row_groups = (nb_query + 3) // 4
    return (24 * 3 * n_cu + row_groups - 1) // row_groups, (nb_gallery >> 15) + 1


def rho(a, b):
    """d^2 / (|a|^2 + |b|^2) from exact differences, in np.longdouble"""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return float(((a - b) ** 2).sum(-1) / ((a * a).sum(-1) + (b * b).sum(-1)))


# ---- references ------------------------------------------------------------------------------------------------------------------------
def dist_ld(A, B, metric=0):
    """[len(A), len(B)] pair distances: squared differences summed in np.longdouble, then sqrt, returned as float64 (metric 1: 1 - cos from
    longdouble sums, 0 where a norm is zero)"""
    A, B = np.asarray(A, np.float64).astype(np.longdouble), np.asarray(B, np.float64).astype(np.longdouble)
    out = np.zeros((len(A), len(B)), np.float64)
    nb = (B * B).sum(-1)
    for i, a in enumerate(A):
        if metric == 0:
            out[i] = np.sqrt(((B - a) ** 2).sum(-1))
        else:
            den = np.sqrt((a * a).sum() * nb)
            with np.errstate(divide="ignore", invalid="ignore"):
                out[i] = np.where(den > 0, 1 - (B @ a) / den, 0)
    return out


def gram_emulation(a, b):
    """the kernels' Gram form for one pair in numpy float64 (the order of the additions is numpy's, not the MFMA's)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d2 = ((a * a).sum() + (b * b).sum()) - 2.0 * (a @ b)
    return float(np.sqrt(max(d2, 0.0)))


def mean_dist_fast(X, row_start, G, gal_start, metric=0, chunk=8192):
    """identify_ref.mean_dist without its loop over (group, identity): the N x M pair distances in float64, chunk rows at a time, then
    np.add.reduceat over both axes and the division by the two sizes.  Euclidean: pairs with d^2 >= 0.2 (|a|^2 + |b|^2) keep the Gram form
    of a float64 matrix product (three roundings of relative size 2^-53 on |a|^2 + |b|^2: relative error in d below 1.5 * 1.1e-16 / 0.2
    ~ 1e-15), every closer pair is recomputed from its differences."""
    X, G = np.asarray(X, np.float64), np.asarray(G, np.float64)
    rs, gs = np.asarray(row_start, np.int64), np.asarray(gal_start, np.int64)
    nx, ng = (X * X).sum(-1), (G * G).sum(-1)
    S = np.zeros((len(rs) - 1, len(gs) - 1), np.float64)
    # chunks end where a group ends (a group longer than a chunk makes its own)
    t0 = 0
    while t0 < len(rs) - 1:
        t1 = max(t0 + 1, int(np.searchsorted(rs, rs[t0] + chunk, side="right")) - 1)
        x, n = X[rs[t0]:rs[t1]], nx[rs[t0]:rs[t1]]
        dot = x @ G.T
        if metric == 0:
            total = n[:, None] + ng[None]
            d2 = total - 2.0 * dot
            i, j = np.nonzero(d2 < 0.2 * total)
            d2[i, j] = ((x[i] - G[j]) ** 2).sum(-1)
            d = np.sqrt(d2)
        else:
            den = np.sqrt(n)[:, None] * np.sqrt(ng)[None]
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.where(den > 0, 1.0 - dot / den, 0.0)
        S[t0:t1] = np.add.reduceat(np.add.reduceat(d, rs[t0:t1] - rs[t0], axis=0), gs[:-1], axis=1)
        t0 = t1
    return S / (np.diff(rs)[:, None] * np.diff(gs)[None]).astype(np.float64)


# ---- the ladder --------------------------------------------------------------------------------------------------------------------------
# (name, rho): the first nine are the rungs around the first switch; the last six bracket the values the switch could move to
RUNGS = [("copy", 0.0), ("quantum", None), ("0.5e-5", 0.5e-5), ("0.99e-5", 0.99e-5), ("1.01e-5", 1.01e-5), ("2e-5", 2e-5), ("1e-4", 1e-4),
         ("1e-3", 1e-3), ("1e-2", 1e-2),
         ("0.99e-4", 0.99e-4), ("1.01e-4", 1.01e-4), ("0.99e-3", 0.99e-3), ("1.01e-3", 1.01e-3), ("0.99e-2", 0.99e-2), ("1.01e-2", 1.01e-2)]
BRACKETS = [name for name, _ in RUNGS if name[:4] in ("0.99", "1.01")]
LADDER_QUERY_ROWS, LADDER_GALLERY_ROWS = 69, 649          # one-row groups: 5 query blocks; 41 gallery blocks in two ranges, cut at row 320
LADDER_GALLERY_RANGES = [0, 20, 41]
LADDER_K10_RANGES = [0, 22, 45]                           # the concatenated table of 718 one-row tracks under K10's numbers


def fixture_rows():
    """the descriptors of tests/golden/c3_clip0.npz as the library's table holds them: float64, rounded to 5 decimals"""
    with np.load(os.path.join(HERE, "golden", "c3_clip0.npz")) as z:
        return np.round(z["embeddings"].astype(np.float64), 5)


def partner(a, u, target, solve):
    """b = round(a + s u, 5) with s = sqrt(target * 2 |a|^2); with `solve`, s solves s^2 = target (2 |a|^2 + 2 s a.u + s^2) instead, so that
    rho(a, b) is the target up to the rounding of b and not up to |b| ~ |a| (1 % matters for the rungs that bracket a switch)"""
    na = float(a @ a)
    s = np.sqrt(target * 2.0 * na)
    if solve:
        au = float(a @ u)
        s = (target * au + np.sqrt((target * au) ** 2 + (1.0 - target) * 2.0 * target * na)) / (1.0 - target)
    return np.round(a + s * u, 5)


def _positions():
    """45 query rows and 45 gallery rows for the pairs: the first and last row of blocks, the last (partial) block, both sides of the
    gallery's range cut (rows 319 | 320) and of K10's cut in the concatenated table (gallery rows 282 | 283), the rest spread out"""
    q = [0, 15, 16, 31, 32, 47, 48, 63, 64, 65, 66, 67, 68]
    others = [r for r in range(1, 64) if r not in q]
    q += [others[i] for i in np.linspace(0, len(others) - 1, 45 - len(q)).astype(int)]
    g = [0, 15, 16, 31, 282, 283, 303, 304, 319, 320, 335, 336, 639, 640, 641, 642, 643, 644, 645, 646, 647, 648]
    g += [40 + 26 * i for i in range(45 - len(g))]
    assert len(set(q)) == 45 and len(set(g)) == 45 and max(q) < LADDER_QUERY_ROWS and max(g) < LADDER_GALLERY_ROWS
    rng = np.random.default_rng(314)
    return rng.permutation(q), rng.permutation(g)


def ladder(scale=None):
    """-> dict(X, rs, G, gs, pairs): 69 one-row query groups and 649 one-row identities of fixture rows (scaled to |x| = scale when given,
    and rounded again), with the pairs of the ladder among them.  pairs: list of (rung name, base 0..2, query row, gallery row)."""
    E = fixture_rows()
    nrm = np.sqrt((E * E).sum(-1))
    bases = [int(np.argmin(nrm)), int(np.argmin(np.abs(nrm - nrm.mean()))), int(np.argmax(nrm))]
    rest = np.setdiff1d(np.arange(len(E)), bases)
    fill = E[rest[np.linspace(0, len(rest) - 1, LADDER_QUERY_ROWS + LADDER_GALLERY_ROWS).astype(int)]]
    if scale is not None:
        fill = np.round(scale * fill / np.sqrt((fill * fill).sum(-1, keepdims=True)), 5)
    X, G = fill[:LADDER_QUERY_ROWS].copy(), fill[LADDER_QUERY_ROWS:].copy()
    qpos, gpos = _positions()
    rng = np.random.default_rng(2718)
    pairs = []
    for bi, base in enumerate(bases):
        a = E[base] if scale is None else np.round(scale * E[base] / nrm[base], 5)
        for ri, (name, target) in enumerate(RUNGS):
            u = rng.standard_normal(128)
            u /= np.sqrt(u @ u)
            if target is None:
                b = a.copy()
                b[17 * (bi + 1)] = np.round(b[17 * (bi + 1)] + 1e-5, 5)
            else:
                b = a.copy() if target == 0.0 else partner(a, u, target, solve=name in BRACKETS)
            k = bi * len(RUNGS) + ri
            X[qpos[k]], G[gpos[k]] = a, b
            pairs.append((name, bi, int(qpos[k]), int(gpos[k])))
    return dict(X=X, rs=np.arange(LADDER_QUERY_ROWS + 1, dtype=np.int32), G=G, gs=np.arange(LADDER_GALLERY_ROWS + 1, dtype=np.int32), pairs=pairs)


def ladder_errors(D, Dr, pairs):
    """{rung: (worst relative error, worst absolute error)} over the ladder's entries of a distance matrix and its reference (the relative
    error of an exact zero is 0)"""
    out = {}
    for name, _, q, g in pairs:
        e = abs(D[q, g] - Dr[q, g])
        r = e / Dr[q, g] if Dr[q, g] > 0 else (0.0 if e == 0 else np.inf)
        w = out.get(name, (0.0, 0.0))
        out[name] = (max(w[0], r), max(w[1], e))
    return out


def print_ladder_errors(what, errs):
    for name, _ in RUNGS:
        print("%s rung %-8s worst relative error %.3g, absolute %.3g" % (what, name, errs[name][0], errs[name][1]))


# ---- gallery and query layouts -----------------------------------------------------------------------------------------------------------
# a gallery of six ranges: 138 blocks, 8 ranges wanted, even cuts at blocks 17, 34, 51, 69, 86, 103, 120.  17, 34, 86 and 103 lie in
# spanning identities and move to 21, 35, 90 and 109; 51 and 69 lie in the 320-row identity and both move to block 70, where the second
# is dropped; 120 finds no clean block before the end and is dropped; a last block of 5 rows
_LONG = [7] * 91 + [3] + [16] * 10 + [320] + [5] * 64 + [1] * 40 + [33] * 10 + [2] * 29 + [16] * 20 + [9]
LONG_EVEN_CUTS = [17, 34, 51, 69, 86, 103, 120]
# name -> (sizes, M, nb, range_b0)
GALLERIES = dict(cc.LAYOUTS)
GALLERIES["long"] = (_LONG, 2197, 138, [0, 21, 35, 70, 90, 109, 138])
QUERIES = {
    "main": identify_ref.QUERY_SIZES,                     # 20 blocks: full workgroups
    "singletons70": [1] * 70,                             # 5 blocks: a workgroup with three idle waves
    "one100": [100],                                      # one group over 7 blocks
    "tail1": [10] * 51 + [3],                             # every second group spanning, a last block of one row
}
N_CENTRES = 40


def _rows(rng, centres, ident, sizes):
    """cluster_cases.tracks with centres that the query and the gallery tables share"""
    rows = []
    for t, n in enumerate(sizes):
        x = centres[ident[t]] + 0.05 * rng.normal(0, 1, (n, 128))
        rows.append(np.round(0.55 * x / np.linalg.norm(x, axis=1, keepdims=True), 5))
    return np.concatenate(rows)


def _centres():
    c = np.random.default_rng(99).normal(0, 1, (N_CENTRES, 128))
    return c / np.linalg.norm(c, axis=1, keepdims=True)


def gallery_table(name):
    """(G, gal_start) of a gallery layout, seeded by its name"""
    sizes = GALLERIES[name][0]
    rng = np.random.default_rng(3000 + sorted(GALLERIES).index(name))
    return _rows(rng, _centres(), rng.integers(0, N_CENTRES, len(sizes)), sizes), cc.starts(sizes)


def plant_rows(gname):
    """the gallery rows that the query tables copy: inside the first range (the first one-row identity there, so that a copy can make a
    whole entry zero; row 5 where there is none), the first row of the second range, the gallery's last row (in its last block)"""
    sizes, M, nb, ranges = GALLERIES[gname]
    gs = cc.starts(sizes)
    cut = ranges[1] * 16
    ones = [int(gs[k]) for k in range(len(sizes)) if sizes[k] == 1 and gs[k] < cut]
    return [ones[0] if ones else 5, cut, M - 1]


def query_table(qname, gname, G):
    """(X, row_start, planted) of a query layout against gallery `gname`: for each of plant_rows(gname) one query row that is a copy of
    it and one that is the copy + 1e-5, as cluster_cases.table plants them for K10.  The copies go to the first rows of the query table
    (one-row groups in `main` and `singletons70`), the near-copies to its last rows.  planted: dict(copies=[(query row, gallery row)],
    near=[...], zero=[(t, k)]: the entries whose group and identity are one planted copy each)."""
    sizes = QUERIES[qname]
    rng = np.random.default_rng(4000 + 10 * sorted(QUERIES).index(qname) + sorted(GALLERIES).index(gname))
    X, rs = _rows(rng, _centres(), rng.integers(0, N_CENTRES, len(sizes)), sizes), cc.starts(sizes)
    N = len(X)
    gsz, gs = GALLERIES[gname][0], cc.starts(GALLERIES[gname][0])
    rows = plant_rows(gname)
    copies = list(zip([0, 1, 40], rows))
    near = list(zip([N - 1, N - 2, N - 18], rows))
    for q, g in copies:
        X[q] = G[g]
    for q, g in near:
        X[q] = np.round(G[g] + 1e-5, 5)
    zero = []
    for q, g in copies:
        t, k = int(np.searchsorted(rs, q, side="right") - 1), int(np.searchsorted(gs, g, side="right") - 1)
        if sizes[t] == 1 and gsz[k] == 1:
            zero.append((t, k))
    return X, rs, dict(copies=copies, near=near, zero=zero)


# ---- more than 65 535 query groups ---------------------------------------------------------------------------------------------------------
HUGE_QUERY_SIZES = [1] * 65530 + [20, 1, 1, 17, 3, 1, 33] + [1] * 40
HUGE_NAMED = {"the 20-row group": 65530, "the 17-row group": 65533, "the 3-row group": 65534, "group 65535": 65535, "the 33-row group": 65536}
HUGE_GALLERIES = {"four": [3, 20, 1, 16], "three_hundred": [int(v) for v in np.random.default_rng(65535).integers(1, 4, 300)]}
HUGE_GALLERY_RANGES = {"four": [0, 3], "three_hundred": [0, 20, 38]}        # (18 ranges wanted; 38 blocks give two)
HUGE_CENTRES = 300


def huge_case():
    """(X, row_start, {gallery name: (G, gal_start)}): identify_ref.main_case's rows (centres 0.7 N(0, 1) / sqrt(128), spread 0.15) around
    300 centres; query group t takes centre t mod 300, identity k centre k.  T = 65 577 groups in N = 65 646 rows (67 MB): cross_norm_k runs
    in two slices of group indices, and groups that span blocks lie on both sides of index 65 535."""
    rng = np.random.default_rng(655)
    centres = 0.7 * rng.standard_normal((HUGE_CENTRES, 128)) / np.sqrt(128.0)
    sigma = 0.15 / np.sqrt(128.0)
    rs = identify_ref.starts(HUGE_QUERY_SIZES)
    cen = np.repeat(np.arange(len(HUGE_QUERY_SIZES)) % HUGE_CENTRES, HUGE_QUERY_SIZES)
    X = np.round(centres[cen] + sigma * rng.standard_normal((len(cen), 128)), 5)
    gal = {}
    for name, sizes in HUGE_GALLERIES.items():
        G = np.concatenate([centres[k] + sigma * rng.standard_normal((n, 128)) for k, n in enumerate(sizes)])
        gal[name] = (np.round(G, 5), identify_ref.starts(sizes))
    return X, rs, gal
