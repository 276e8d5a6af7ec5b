"""The track layouts that the clustering tests share (tests/test_cluster_cases.py on the CPU, tests/test_gpu_cluster_layouts.py on the GPU),
their tables, and the references that are not the oracle's.

A layout is a list of track sizes.  K10 (csrc/cluster.hip, pair_tiles_k) cuts the 16-row blocks of the table into column ranges and
carries the sums of a track that spans blocks inside a range; which ranges a layout gets is decided on the host (csrc/group_blocks.h)
and cannot be seen from a result, so every layout states the ranges it is meant to reach -- with K10's numbers on 256 compute units --
and the CPU test asserts them from the real header."""
import numpy as np

N_CU = 256                                   # compute units of the device the expected ranges are stated for

_M20 = [1, 1, 2, 15, 16, 17, 3, 31, 32, 33, 1, 48, 5, 7, 16, 16, 1, 9, 64, 2]

# name -> (sizes, N, nb, range_b0)
LAYOUTS = {
    # one segment per block, nothing carried, a clean even cut
    "aligned16": ([16] * 40, 640, 40, [0, 20, 40]),
    # 16 segments in every block, T = 521, a last block of 9 rows
    "singletons": ([1] * 521, 521, 33, [0, 16, 33]),
    # a 70-row track lies across the even cut (block 17): the cut moves to block 22; 25 spanning tracks
    "cut_moved": ([7] * 36 + [70] + [5] * 45 + [3], 550, 35, [0, 22, 35]),
    # three ranges wanted: the 300-row track swallows one cut and moves the other
    "one_cut_dropped": ([9] * 28 + [300] + [11] * 20 + [2] * 8, 788, 50, [0, 40, 50]),
    # a last block of one row, every second track spanning
    "tail1": ([10] * 51 + [3], 513, 33, [0, 20, 33]),
    # three ranges, sizes on, before and after the seams
    "mixed3": (_M20 * 2 + [100, 1, 40, 16, 16, 9], 822, 52, [0, 20, 40, 52]),
}
MULTI_RANGE = sorted(LAYOUTS)                # every layout above has more than one range

# the size list of test_pair_mean_dist_matrix_core_kernel_all_block_shapes (tests/test_gpu_parity.py): two ranges are wanted, the 250-row
# track covers every block from the proposed cut to the end, so ONE range is planned -- why the layouts above exist
ALL_BLOCK_SHAPES_SIZES = [1, 1, 1, 15, 16, 17, 2, 3, 31, 32, 33, 1, 5, 5, 5, 1, 64, 7, 9, 250, 1, 1]


def starts(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def k10_wanted(nb, n_cu=N_CU):
    """the two numbers cluster.hip passes to cut_ranges: (wanted ranges, floor)"""
    row_groups = (nb + 3) // 4
    return (2 * 24 * 3 * n_cu + row_groups - 1) // row_groups, (nb >> 16) + 1


def tracks(rng, sizes, dim=128, K=40, noise=0.05):
    """test_gpu_parity's _tracks at any width: unit centres, noise 0.05, rows scaled to 0.55 and rounded to 5 decimals"""
    centres = rng.normal(0, 1, (K, dim)); centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    ident = rng.integers(0, K, len(sizes))
    rows = []
    for t, n in enumerate(sizes):
        x = centres[ident[t]] + noise * rng.normal(0, 1, (n, dim))
        rows.append(np.round(0.55 * x / np.linalg.norm(x, axis=1, keepdims=True), 5))
    return np.concatenate(rows), starts(sizes), ident


def _track_of(rs, row):
    return int(np.searchsorted(rs, row, side="right") - 1)


def table(name):
    """(X, row_start, planted) of a layout, seeded by its name.  Planted: identical rows inside a track, across two tracks of one range
    and across the first range cut, and a near-identical pair (+1e-5) across that cut -- the pairs for which K10 leaves the Gram form.
    planted["zero_pairs"]: track pairs (i, j), i < j, made of identical rows only: their distance is exactly 0."""
    sizes, N, nb, ranges = LAYOUTS[name]
    rng = np.random.default_rng(1000 + sorted(LAYOUTS).index(name))
    X, rs, _ = tracks(rng, sizes)
    cut = ranges[1] * 16                                     # first row of the second range
    planted = {"zero_pairs": [], "cut_row": cut}
    if name == "singletons":
        # one-row tracks that are copies of each other: in one block, in two blocks of a range, across the cut, in the last block
        for a, b in ((5, 9), (5, 40), (5, 300), (7, cut), (cut - 1, 520)):
            X[b] = X[a]
        planted["zero_pairs"] = [(5, 9), (5, 40), (9, 40), (5, 300), (9, 300), (40, 300), (7, cut), (cut - 1, 520)]
        X[400] = X[6] + 1e-5                                 # near-identical across the cut
        return X, rs, planted
    big = int(np.argmax(np.diff(rs) >= 2))                   # the first track of two rows or more
    X[rs[big] + 1] = X[rs[big]]                              # inside a track
    X[rs[big + 2]] = X[rs[big]]                              # across two tracks
    X[cut] = X[3]                                            # across the range cut: identical ...
    X[cut + 2] = X[cut - 3] + 1e-5                           # ... and near-identical
    planted["tracks"] = [big, big + 2, _track_of(rs, 3), _track_of(rs, cut), _track_of(rs, cut - 3), _track_of(rs, cut + 2)]
    return X, rs, planted


def cosine_mean_dist(X, rs):
    """T x T block means of 1 - cos in numpy float64, 0 where a norm is zero (the convention of tests/identify_ref.py and of the
    kernel's `den > 0 ? ... : 0`), diagonal zero"""
    X = np.asarray(X, np.float64)
    nrm = np.sqrt((X * X).sum(-1))
    den = nrm[:, None] * nrm[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(den > 0, 1.0 - (X @ X.T) / den, 0.0)
    S = np.add.reduceat(np.add.reduceat(d, rs[:-1], axis=0), rs[:-1], axis=1)
    n = np.diff(rs).astype(np.float64)
    D = S / (n[:, None] * n[None])
    np.fill_diagonal(D, 0.0)
    return D


def share_cut_lists(name):
    """three lists of track cuts [0, ..., T] for the stitched-shares test: at the track where the second range begins; one track to either
    side of it; inside the run of spanning tracks (a cut before and after a spanning track, so one share holds that track alone).  Every
    list also holds an empty share and the share [T - 1, T)."""
    sizes, N, nb, ranges = LAYOUTS[name]
    rs = starts(sizes)
    T = len(sizes)
    tc = _track_of(rs, ranges[1] * 16)
    b_first, b_last = rs[:-1] // 16, (rs[1:] - 1) // 16
    span = np.flatnonzero(b_last > b_first)
    lists = [[0, tc, tc, T - 1, T], [0, tc - 1, tc + 1, tc + 1, T - 1, T]]
    if len(span):
        s = int(span[len(span) // 2])
        lists.append(sorted({0, s, s + 1, T - 1, T}) + [T])            # (the doubled T: an empty last share)
    else:
        lists.append([0, 1, 1, tc + 3, T - 1, T])
    return lists


# ---- the agglomeration at the switch between its two paths (HAC_PERSIST_MAX_T = 10 200 in csrc/cluster.hip) -------------------------
HAC_SWITCH_T = 10201


def hac_switch_case():
    """(D float64 [10201, 10201], sizes): 1.0 everywhere (above the threshold 0.6), a zero diagonal, and about 30 planted pairs below 0.6:
    distinct values, exactly equal ones (the first minimum in row-major order decides, within a row and between rows), and chains whose
    merged rows are scanned again.  Rows from every 1024-entry stride of the persistent kernel take part, the last track of the leading
    10 200 block (10 199) and the last track of all (10 200) among them.  The oracle scans T^2 entries per merge: the planted set is
    kept to fewer than 40 merges."""
    T = HAC_SWITCH_T
    D = np.ones((T, T), np.float64)
    np.fill_diagonal(D, 0.0)
    sizes = np.random.default_rng(61).integers(1, 5, T)

    def put(i, j, v):
        D[i, j] = D[j, i] = v
    # distinct values
    for k, (i, j) in enumerate([(3, 10198), (1023, 1024), (2047, 9000), (5000, 5001), (7, 8), (4096, 8191), (9215, 9216), (6000, 10100),
                                (10199, 10200), (10197, 10199)]):
        put(i, j, 0.11 + 0.013 * k)
    # exactly equal values: two in one row, the others in rows before and after it
    for i, j in [(300, 4000), (300, 2500), (100, 9999), (2500, 2600), (8000, 8001), (10190, 10195), (1, 10196)]:
        put(i, j, 0.25)
    # a tie between a planted value and the mean a merge makes: sizes 2 and 2 give (0.25 * 2 + 0.5 * 2) / 4 = 0.375 exactly
    sizes[[700, 701, 702]] = 2
    put(700, 701, 0.125); put(700, 702, 0.25); put(701, 702, 0.5); put(650, 9100, 0.375); put(900, 901, 0.375)
    # chains: every pair of the chain below the threshold, so the merged row merges again
    for chain, v0 in (([1500, 3500, 5500, 7500], 0.2), ([9300, 9301, 9302], 0.3), ([10, 5120, 10188], 0.15)):
        for a in range(len(chain)):
            for b in range(a + 1, len(chain)):
                put(chain[a], chain[b], v0 + 0.03 * (b - a) + 0.001 * a)
    return D, sizes
