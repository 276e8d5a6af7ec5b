"""GPU: the track-pair mean distances (K10: pair_tiles_k and the per-row kernels for other widths) and the agglomeration (K11) of
csrc/cluster.hip where the older tests do not pin them: tables whose column blocks are cut into several ranges (tests/cluster_cases.py;
tests/test_cluster_cases.py asserts the ranges from the real planner), shares of a split that fall on and around those cuts, zero rows
under cosine, widths other than 128, the float32 table at other strides, orders and decimals, the switch between the persistent
agglomeration kernel and the launch-per-merge loop at T = 10 200 / 10 201, and the refusal of bad row_start tables.

References: oracle.pair_mean_dist (the direct float64 double loop), numpy float64 block means of 1 - cos, oracle.hac.  Tolerances: those
of tests/test_gpu_parity.py and tests/test_gpu_identify.py for this arithmetic -- Euclidean rtol 1e-12 / atol 1e-13, cosine rtol 1e-10 /
atol 1e-12; whatever is the same kernels on the same table is compared bit for bit."""
import ctypes as C
import time

import numpy as np
import pytest
import torch          # noqa: F401 -- first, as in bench.py: the process then runs on the HIP runtime torch ships

from tests import cluster_cases as cc

pytestmark = pytest.mark.gpu

TOL = {0: dict(rtol=1e-12, atol=1e-13), 1: dict(rtol=1e-10, atol=1e-12)}


@pytest.fixture(scope="module")
def layouts(oracle):
    """name -> (X, row_start, planted, {metric: reference D}), made once"""
    out = {}
    for name in cc.LAYOUTS:
        X, rs, planted = cc.table(name)
        out[name] = (X, rs, planted, {0: oracle.pair_mean_dist(X, rs), 1: cc.cosine_mean_dist(X, rs)})
    return out


def _against(D, Dr, metric, what):
    err = np.abs(D - Dr)
    print("%s metric %d: T = %d, worst |D - ref| = %.3g (ref up to %.3g)" % (what, metric, len(D), err.max(), np.abs(Dr).max()))
    assert D.shape == Dr.shape and np.allclose(D, Dr, **TOL[metric]), (what, metric, err.max())
    assert np.array_equal(D, D.T) and not D.diagonal().any()


def _stitched(ctx, X, rs, cuts, D):
    """shares [cuts[k], cuts[k + 1]) of both split entries, stitched: the upper triangle and the whole matrix, bit for bit"""
    U, F = np.zeros_like(D), np.zeros_like(D)
    for t0, t1 in zip(cuts, cuts[1:]):
        part = ctx.pair_upper_rows(X, rs, t0, t1)
        assert not part[:t0].any() and not part[t1:].any()
        U[t0:t1] = part[t0:t1]
        full = ctx.pair_mean_dist_rows(X, rs, t0, t1)
        assert not full[:t0].any() and not full[t1:].any()
        F[t0:t1] = full[t0:t1]
    assert np.array_equal(U, np.triu(D, 1)), cuts
    assert np.array_equal(F, D), cuts


# ---- 1. every layout, both metrics -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("name", sorted(cc.LAYOUTS))
def test_layout_against_the_reference(ctx, layouts, name, metric):
    X, rs, planted, Dr = layouts[name]
    D = ctx.pair_mean_dist(X, rs, metric=metric)
    _against(D, Dr[metric], metric, name)
    if metric == 0:
        for i, j in planted["zero_pairs"]:                   # one-row tracks that are copies of each other: exactly zero
            assert D[i, j] == 0.0 and D[j, i] == 0.0, (i, j, D[i, j])
        assert len(planted["zero_pairs"]) > 0 or name != "singletons"
    assert np.array_equal(D, ctx.pair_mean_dist(X, rs, metric=metric))          # the same call twice: the same bits


# ---- 2. shares on and around the range cuts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.MULTI_RANGE)
def test_shares_stitch_bit_for_bit_around_the_range_cuts(ctx, layouts, name):
    """cuts at the track where the second column range begins, one track to either side of it, and around a spanning track (a share that
    holds that track alone: pair_chunks_k only); an empty share and the share [T - 1, T) in every list"""
    X, rs, planted, Dr = layouts[name]
    D = ctx.pair_mean_dist(X, rs)
    for cuts in cc.share_cut_lists(name):
        _stitched(ctx, X, rs, cuts, D)
    # the agglomeration of the stitched triangle is the one of the whole call
    labels, log = ctx.cluster_tracks(X, rs, 0.6)
    l2, log2 = ctx.cluster_upper(np.triu(D, 1), rs, 0.6)
    assert np.array_equal(labels, l2) and np.array_equal(log, log2)


# ---- 3. zero rows under cosine -----------------------------------------------------------------------------------------------------------
def test_zero_rows_under_cosine_in_the_tile_kernel(ctx, oracle, layouts):
    """mixed3 with a whole zero track, zero rows on both sides of a block seam and on both sides of a range cut: 1 - cos counts 0 where a
    norm is zero; the Euclidean matrix of the same table for good measure"""
    X, rs, planted, _ = layouts["mixed3"]
    X = X.copy()
    ranges = cc.LAYOUTS["mixed3"][3]
    X[rs[4]:rs[5]] = 0.0                                     # a whole 16-row track
    X[rs[10]] = 0.0                                          # a whole one-row track
    X[[47, 48]] = 0.0                                        # the last row of block 2 and the first of block 3, inside a 17-row track
    X[[ranges[1] * 16 - 1, ranges[1] * 16, ranges[2] * 16]] = 0.0            # either side of the first cut, the first row after the second
    assert rs[5] < 47 and 48 < rs[6] - 1 and rs[5] - rs[4] == 16 and rs[11] - rs[10] == 1
    _against(ctx.pair_mean_dist(X, rs, metric=1), cc.cosine_mean_dist(X, rs), 1, "mixed3 with zero rows")
    _against(ctx.pair_mean_dist(X, rs, metric=0), oracle.pair_mean_dist(X, rs), 0, "mixed3 with zero rows")
    Z = ctx.pair_mean_dist(X, rs, metric=1)
    assert Z[4, 10] == 0.0 and Z[10, 4] == 0.0              # two zero tracks: every pair counts 0


# ---- 4. other widths -----------------------------------------------------------------------------------------------------------------------
def _other_dim(ctx, oracle, X, rs, cuts, what):
    from pyannote_video_amd import _lib
    sizes = np.diff(rs)
    D = ctx.pair_mean_dist(X, rs)
    Dr = oracle.pair_mean_dist(X, rs)
    _against(D, Dr, 0, what)
    _stitched(ctx, X, rs, cuts, D)
    labels, log = ctx.cluster_tracks(X, rs, 0.6)
    lr, logr = oracle.hac(Dr, sizes, 0.6)
    assert np.array_equal(labels, lr)
    assert len(log) == len(logr) and np.array_equal(log[:, :2], logr[:, :2])
    with pytest.raises(_lib.PvfError, match="cosine is implemented for 128-D rows"):
        ctx.pair_mean_dist(X, rs, metric=1)


@pytest.mark.parametrize("dim", [1, 3, 64, 127, 129, 512])
def test_other_widths_against_the_oracle(ctx, oracle, dim):
    """transpose_k, row_track_sums_k, track_pair_mean_k: the cut_moved sizes (N = 550, T = 83) at widths that are 1, odd, below and above
    128, and larger than a block of threads; shares that start at a row a0 > 0"""
    sizes = cc.LAYOUTS["cut_moved"][0]
    X, rs, _ = cc.tracks(np.random.default_rng(2000 + dim), sizes, dim=dim)
    T = len(sizes)
    _other_dim(ctx, oracle, X, rs, [0, 36, 37, 37, T - 1, T], "dim %d" % dim)


def test_other_width_across_the_2048_row_chunk(ctx, oracle):
    """dim = 64, N = 2100: the track of rows 2040 to 2060 lies across PD_CHUNK = 2048, so its running sums go on from one chunk of
    distances in LDS to the next"""
    sizes = [10] * 204 + [21] + [13] * 3
    X, rs, _ = cc.tracks(np.random.default_rng(2100), sizes, dim=64, K=60)
    assert rs[-1] == 2100 and rs[204] == 2040 and rs[205] == 2061
    _other_dim(ctx, oracle, X, rs, [0, 100, 204, 205, 205, 207, 208], "dim 64 across the chunk")


def test_widest_table_and_the_refusal_above_it(ctx, oracle):
    """dim = 4096, the limit of the entry (the row and a chunk of distances share the LDS), 40 rows in 6 tracks; 4097 is refused"""
    from pyannote_video_amd import _lib
    sizes = [1, 7, 16, 3, 12, 1]
    X, rs, _ = cc.tracks(np.random.default_rng(4096), sizes, dim=4096, K=3)
    _other_dim(ctx, oracle, X, rs, [0, 2, 2, 5, 6], "dim 4096")
    with pytest.raises(_lib.PvfError, match="bad sizes"):
        ctx.pair_mean_dist(np.zeros((40, 4097)), rs)
    with pytest.raises(_lib.PvfError, match="bad sizes"):
        ctx.cluster_tracks(np.zeros((40, 4097)), rs, 0.6)


# ---- 5. the float32 table --------------------------------------------------------------------------------------------------------------------
def _f32_source():
    """float32 rows of the cut_moved layout with the values a rounding can get wrong among them: -0.0, and exact ties of the rounding in
    float64 -- m / 64 (x 1e5 = ... .5), m / 16 (x 1e3), m / 256 (x 1e7), +-0.5 and 1.5 (x 1) for odd m: a float32 times a power of ten
    below 2^29 is exact in float64, so these products ARE k + 0.5"""
    sizes = cc.LAYOUTS["cut_moved"][0]
    rng = np.random.default_rng(77)
    X, rs, _ = cc.tracks(rng, sizes)
    E = X.astype(np.float32)
    ties = np.concatenate([np.arange(1, 35, 2) / 64.0, -np.arange(1, 35, 2) / 64.0, np.arange(1, 9, 2) / 16.0, -np.arange(1, 9, 2) / 16.0,
                           np.arange(1, 141, 2) / 256.0, [0.5, -0.5, 1.5, -0.0, -0.0, 0.0]]).astype(np.float32)
    for d, s in ((5, 1e5), (3, 1e3), (7, 1e7)):
        p = ties.astype(np.float64) * s
        assert (np.abs(p - np.floor(p)) == 0.5).sum() >= 4, d
    at = rng.choice(E.size, 4 * len(ties), replace=False)
    E.reshape(-1)[at] = np.tile(ties, 4)
    return E, rs


def _rounded(E, d):
    """the table the library makes of float32 rows: np.round(float64(E), d); d < 0 means no rounding (not numpy's rounding to tens)"""
    E64 = E.astype(np.float64)
    return E64 if d < 0 else np.round(E64, d)


@pytest.mark.parametrize("decimals", [-1, 0, 3, 5, 7])
def test_float32_table_strides_orders_and_decimals(ctx, decimals):
    """gather_round_rows_k / stage_table: cluster_tracks_f32 and pair_upper_rows_f32 against the float64 entries on
    np.round(float64(E), d)[order], bit for bit -- contiguous rows with a permutation, a 640-byte stride (a [:, :128] view that reaches the
    library uncopied), no order with spare rows behind N, an order with repeated indices, and the same rows in device memory"""
    from pyannote_video_amd.runtime import DeviceRows
    E, rs = _f32_source()
    N, T = len(E), len(rs) - 1
    rng = np.random.default_rng(5 + decimals)
    wide = np.zeros((N + 30, 160), np.float32)
    wide[:, 128:] = 9.0                                      # what lies between the rows must not be read
    wide[:N, :128] = E
    wide[N:, :128] = rng.normal(0, 0.05, (30, 128)).astype(np.float32)
    view = wide[:, :128]
    assert ctx._f32_rows(view)[1] == 640 and ctx._f32_rows(view)[2] == N + 30
    perm = rng.permutation(N)
    inv = np.argsort(perm).astype(np.int32)
    few = rng.integers(0, 200, N).astype(np.int32)           # 550 rows drawn from 200: identical rows inside and across tracks
    dev = torch.from_numpy(np.ascontiguousarray(wide)).cuda()
    dev_e = torch.from_numpy(E[perm]).cuda()
    torch.cuda.synchronize()
    cases = [
        ("permuted", E[perm], inv, E),
        ("stride 640, no order, spare rows", view, None, E),
        ("stride 640, permuted", wide[np.r_[perm, N:N + 30]][:, :128], inv, E),
        ("repeated indices", E, few, E[few]),
        ("device rows", DeviceRows.of_tensor(dev_e), inv, E),
        ("device rows, stride 640, repeated", DeviceRows(dev.data_ptr(), N + 30, 640, keep=dev), few, E[few]),
        ("device rows, stride 640, no order", DeviceRows(dev.data_ptr(), N + 30, 640, keep=dev), None, E),
    ]
    for what, rows, order, table in cases:
        Xr = _rounded(table, decimals)
        lf, logf = ctx.cluster_tracks_f32(rows, order, rs, 0.6, decimals=decimals)
        lw, logw = ctx.cluster_tracks(Xr, rs, 0.6)
        assert np.array_equal(lf, lw) and np.array_equal(logf, logw), (what, decimals)
        U = np.triu(ctx.pair_mean_dist(Xr, rs), 1)
        for t0, t1 in ((0, T), (36, 44), (T - 1, T)):
            Uf = ctx.pair_upper_rows_f32(rows, order, rs, t0, t1, decimals=decimals)
            assert Uf.shape == (t1 - t0, T) and np.array_equal(Uf, U[t0:t1]), (what, decimals, t0, t1)
    assert (wide[:, 128:] == 9.0).all()


# ---- 6. the switch between the two agglomeration paths -------------------------------------------------------------------------------------------
def test_agglomeration_on_both_sides_of_its_switch(ctx, oracle):
    """T = 10 201 runs the launch-per-merge loop, its leading 10 200 x 10 200 block the persistent kernel at its limit (hac_persist_k<10, .>
    with the largest dynamic LDS it may ask for), and the same block the loop again through the test flag of the cooccur entry with
    disjoint extents: labels and the whole merge log -- pairs, distances, sizes -- equal oracle.hac, bit for bit (tests/cluster_cases.py
    plants the pairs; 25 merges, so that the oracle's T^2 scan per merge stays at a few seconds)"""
    t_start = time.perf_counter()
    D, sizes = cc.hac_switch_case()
    T = cc.HAC_SWITCH_T
    rs = cc.starts(sizes)
    lr, logr = oracle.hac(D, sizes, 0.6)
    assert 20 <= len(logr) <= 40
    labels, log = ctx.cluster_dist(D, rs, 0.6)
    assert np.array_equal(log, logr) and np.array_equal(labels, lr)
    B = np.ascontiguousarray(D[:T - 1, :T - 1])
    del D
    lrb, logrb = oracle.hac(B, sizes[:T - 1], 0.6)
    assert 20 <= len(logrb) <= 40 and not np.array_equal(logrb, logr)            # (track 10 200 takes part in the larger one)
    lb, logb = ctx.cluster_dist(B, rs[:T], 0.6)
    assert np.array_equal(logb, logrb) and np.array_equal(lb, lrb)
    extent = np.stack([2.0 * np.arange(T - 1), 2.0 * np.arange(T - 1) + 1.0], axis=1)
    lc, logc, n_blocked = ctx.cluster_dist_cooccur(B, rs[:T], 0.6, extent, flags=1)
    assert n_blocked == 0
    assert np.array_equal(logc, logb) and np.array_equal(lc, lb)
    print("agglomeration at the switch: %d and %d merges, %.1f s" % (len(logr), len(logrb), time.perf_counter() - t_start))


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
BAD_TABLES = [
    ("decreasing", [0, 20, 8, 40], "row_start must be non-decreasing"),
    ("empty track", [0, 8, 8, 40], "row_start holds an empty group"),
    ("end is not N", [0, 8, 20, 39], "row_start must end at the number of rows"),
    ("first is not 0", [1, 8, 20, 40], "row_start must start at 0"),
    ("an entry above N", [0, 8, 1000000, 40], "row_start must be non-decreasing"),
]


def test_bad_row_start_is_refused_before_any_device_work(ctx):
    """every K10 / K11 entry checks its row_start on the host (csrc/group_blocks.h, the check identification has always made): the call
    returns the error with its message, writes nothing to its outputs, and the context goes on.  Through the C ABI, so that the outputs
    are buffers this test owns.  (pvf_cluster_dist has no N: its table ends where it ends, the other four cases apply.)"""
    from pyannote_video_amd import _lib
    from pyannote_video_amd._lib import ptr
    l, h = ctx._l, ctx._h
    rng = np.random.default_rng(9)
    X, good, _ = cc.tracks(rng, [8, 12, 20])
    E = X.astype(np.float32)
    N, T = 40, 3
    before = (ctx.pair_mean_dist(X, good), ctx.cluster_tracks(X, good, 0.6), ctx.cluster_tracks_f32(E, None, good, 0.6))
    Dm = np.ascontiguousarray(before[0])
    extent = np.array([[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]])
    for what, table, message in BAD_TABLES:
        rs = np.array(table, np.int32)
        D = np.full((T, T), 7.0)
        labels = np.full(T, -5, np.int32)
        log = np.full((T, 4), 7.0)
        n, nb = C.c_int32(-5), C.c_int32(-5)
        calls = {
            "pair_mean_dist": lambda: l.pvf_pair_mean_dist_metric(h, ptr(X), N, 128, ptr(rs), T, 0, ptr(D)),
            "pair_upper_rows": lambda: l.pvf_pair_upper_rows(h, ptr(X), N, 128, ptr(rs), T, 0, T, ptr(D)),
            "pair_mean_dist_rows": lambda: l.pvf_pair_mean_dist_rows(h, ptr(X), N, 128, ptr(rs), T, 0, T, ptr(D)),
            "cluster_tracks": lambda: l.pvf_cluster_tracks(h, ptr(X), N, 128, ptr(rs), T, 0.6, ptr(labels), ptr(log), C.byref(n)),
            "cluster_tracks_f32": lambda: l.pvf_cluster_tracks_f32(h, ptr(E), 512, N, 0, None, N, 5, ptr(rs), T, 0, 0.6, ptr(labels), ptr(log),
                                                                  C.byref(n)),
            "pair_upper_rows_f32": lambda: l.pvf_pair_upper_rows_f32(h, ptr(E), 512, N, 0, None, N, 5, ptr(rs), T, 0, T, ptr(D), 0),
            "cluster_tracks_cooccur": lambda: l.pvf_cluster_tracks_cooccur(h, ptr(X), N, 128, ptr(rs), T, 0.6, ptr(labels), ptr(log), C.byref(n),
                                                                          ptr(extent), C.byref(nb), 0),
        }
        if what != "end is not N":
            calls["cluster_dist"] = lambda: l.pvf_cluster_dist(h, ptr(Dm), ptr(rs), T, 0.6, ptr(labels), ptr(log), C.byref(n))
            calls["cluster_upper_cooccur"] = lambda: l.pvf_cluster_upper_cooccur(h, ptr(Dm), 0, ptr(rs), T, 0.6, ptr(labels), ptr(log), C.byref(n),
                                                                                ptr(extent), C.byref(nb), 1)
        for name, call in calls.items():
            with pytest.raises(_lib.PvfError, match=message):
                _lib.check(call())
            assert (D == 7.0).all() and (labels == -5).all() and (log == 7.0).all() and n.value == -5 and nb.value == -5, (what, name)
        # the wrappers raise the same error
        with pytest.raises(_lib.PvfError, match=message):
            ctx.pair_mean_dist(X, rs)
        with pytest.raises(_lib.PvfError, match=message):
            ctx.cluster_tracks(X, rs, 0.6)
    after = (ctx.pair_mean_dist(X, good), ctx.cluster_tracks(X, good, 0.6), ctx.cluster_tracks_f32(E, None, good, 0.6))
    assert np.array_equal(before[0], after[0])
    for b, a in zip(before[1:], after[1:]):
        assert np.array_equal(b[0], a[0]) and np.array_equal(b[1], a[1])


def test_short_order_and_short_table_are_refused_by_the_wrappers(ctx):
    rng = np.random.default_rng(10)
    X, rs, _ = cc.tracks(rng, [8, 12, 20])
    E = X.astype(np.float32)
    with pytest.raises(ValueError, match="order"):
        ctx.cluster_tracks_f32(E, np.arange(39, dtype=np.int32), rs, 0.6)
    with pytest.raises(ValueError, match="order"):
        ctx.pair_upper_rows_f32(E, np.arange(41, dtype=np.int32) % 40, rs, 0, 3)
    with pytest.raises(ValueError, match="rows"):
        ctx.cluster_tracks_f32(E[:39], None, rs, 0.6)
    with pytest.raises(ValueError, match="rows"):
        ctx.pair_upper_rows(X[:39], rs, 0, 3)
    with pytest.raises(ValueError, match="rows"):
        ctx.pair_mean_dist_rows(X[:39], rs, 0, 3)
    labels, log = ctx.cluster_tracks_f32(E, np.arange(40, dtype=np.int32), rs, 0.6)
    assert np.array_equal(labels, ctx.cluster_tracks_f32(E, None, rs, 0.6)[0])
