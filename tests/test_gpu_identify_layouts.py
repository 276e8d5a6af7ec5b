"""GPU: the two mean-distance tile kernels -- cross_tiles_k of csrc/identify.hip and pair_tiles_k of csrc/cluster.hip (K10) -- where the
older tests do not pin them (tests/identify_cases.py holds the cases, tests/test_identify_cases.py asserts on the CPU that they are what
they say):
  * pairs on both sides of GRAM_SWITCH (csrc/pvf_internal.h), on rows at the scale the embedder emits (norms 6 to 12) and at |x| = 0.55,
    every pair a one-row group against a one-row identity;
  * galleries of two to six column ranges with moved and dropped cuts, a tail of one row, 16 segments per block and K > 256, against four
    query layouts, with copies and near-copies of gallery rows planted on the seams;
  * more than 65 535 query groups.
Tolerances: those of tests/test_gpu_identify.py -- Euclidean rtol 1e-12 / atol 1e-13, cosine rtol 1e-10 / atol 1e-12 (include/pvface.h).

MEASURED ON THE LADDER (MI355X, worst relative error of d per rung over three base rows, descriptor scale, against squared differences
summed in np.longdouble; `emulated` is the numpy float64 Gram form of tests/test_identify_cases.py):
                  emulated   switch 1e-5 (before)   switch 1e-3 (now)
  copy, quantum    --         0                      0
  0.5e-5           3.4e-11    1.3e-16                1.3e-16
  0.99e-5          4.9e-12    3.6e-16                3.6e-16
  1.01e-5          1.1e-11    3.65e-11  FAILED       3.9e-16
  2e-5             2.2e-12    2.49e-11  FAILED       3.8e-16
  0.99e-4          1.8e-12    2.13e-12  FAILED       1.6e-16
  1e-4             6.8e-13    3.12e-12  FAILED       1.7e-16
  1.01e-4          6.7e-13    2.71e-12  FAILED       1.7e-16
  0.99e-3          4.8e-14    1.72e-13               2.0e-16
  1e-3             1.0e-13    3.79e-13               2.0e-16   (the three pairs lie just below 1e-3)
  1.01e-3          1.1e-13    1.77e-13               1.77e-13
  0.99e-2 .. 1.01e-2  1.6e-14 2.98e-14               2.98e-14
pair_tiles_k and cross_tiles_k gave the same figures; at |x| = 0.55 the relative errors are the same (1.82e-11 at 1.01e-5, 1.82e-13 at
1.01e-3) and the absolute ones stay below the atol, so only the descriptor scale failed before.  DESIGN.md, section 4, has the whole
table and the timings that set the switch.
"""
import numpy as np
import pytest
import torch          # noqa: F401 -- first, as in bench.py: the process then runs on the HIP runtime torch ships

from tests import identify_cases as ic
from tests import identify_ref as ref

pytestmark = pytest.mark.gpu

TOL = {0: dict(rtol=1e-12, atol=1e-13), 1: dict(rtol=1e-10, atol=1e-12)}
SCALES = {"descriptor": None, "0.55": 0.55}


@pytest.fixture(scope="module", autouse=True)
def stated_device():
    """the column ranges of the cases are stated for 256 compute units: on another device the same calls are right but reach other paths"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    if n_cu != ic.N_CU:
        pytest.skip("the column ranges of tests/identify_cases.py are stated for %d compute units; this device has %d" % (ic.N_CU, n_cu))


@pytest.fixture(scope="module")
def ladders():
    """scale name -> (ladder, {metric: longdouble reference of the 69 x 649 matrix}), made once"""
    out = {}
    for name, scale in SCALES.items():
        L = ic.ladder(scale)
        out[name] = (L, {m: ic.dist_ld(L["X"], L["G"], m) for m in (0, 1)})
    return out


@pytest.fixture(scope="module")
def galleries():
    """gallery name -> (G, gal_start), made once"""
    return {name: ic.gallery_table(name) for name in ic.GALLERIES}


@pytest.fixture(scope="module")
def huge():
    """(X, row_start, {gallery: (G, gal_start, {metric: reference D})}), made once"""
    X, rs, gal = ic.huge_case()
    return X, rs, {name: (G, gs, {m: ic.mean_dist_fast(X, rs, G, gs, m) for m in (0, 1)}) for name, (G, gs) in gal.items()}


def _against(D, Dr, metric, what):
    err = np.abs(D - Dr)
    print("%s metric %d: %d x %d, worst |D - ref| = %.3g (ref up to %.3g)" % (what, metric, D.shape[0], D.shape[1], err.max(), np.abs(Dr).max()))
    assert D.shape == Dr.shape and np.allclose(D, Dr, **TOL[metric]), (what, metric, err.max())


def _ladder_entries(D, Dr, L, metric, what):
    errs = ic.ladder_errors(D, Dr, L["pairs"])
    ic.print_ladder_errors("%s metric %d:" % (what, metric), errs)
    for name, _, q, g in L["pairs"]:
        assert np.allclose(D[q, g], Dr[q, g], **TOL[metric]), (what, metric, name, D[q, g], Dr[q, g])
        if name == "copy":
            assert D[q, g] == 0.0 or metric == 1, (what, name, D[q, g])


# ---- 1. the ladder through identification ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("scale", sorted(SCALES))
def test_ladder_through_gallery_mean_dist(ctx, ladders, scale, metric):
    """every a as a one-row group, every b as a one-row identity: the pairs of the ladder (printed per rung, pytest -s) and the whole
    69 x 649 matrix around them"""
    L, Dr = ladders[scale]
    D = ctx.gallery_mean_dist(L["X"], L["rs"], L["G"], L["gs"], metric=metric)
    _ladder_entries(D, Dr[metric], L, metric, "cross_tiles_k, %s scale," % scale)
    _against(D, Dr[metric], metric, "ladder tables, %s scale" % scale)


# ---- 2. the ladder through K10 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("scale", sorted(SCALES))
def test_ladder_through_pair_mean_dist(ctx, ladders, scale, metric):
    """the same rows as one table of 718 one-row tracks: the arithmetic is shared, so the answer is too"""
    L, Dr = ladders[scale]
    nq = len(L["X"])
    XG = np.concatenate([L["X"], L["G"]])
    full = ctx.pair_mean_dist(XG, np.arange(len(XG) + 1, dtype=np.int32), metric=metric)
    assert np.array_equal(full, full.T) and not full.diagonal().any()
    D = full[:nq, nq:]
    _ladder_entries(D, Dr[metric], L, metric, "pair_tiles_k, %s scale," % scale)
    _against(D, Dr[metric], metric, "ladder tables through K10, %s scale" % scale)


# ---- 3. every gallery layout against every query layout ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("qname", sorted(ic.QUERIES))
@pytest.mark.parametrize("gname", sorted(ic.GALLERIES))
def test_gallery_layout_against_query_layout(ctx, galleries, gname, qname, metric):
    G, gs = galleries[gname]
    X, rs, planted = ic.query_table(qname, gname, G)
    D = ctx.gallery_mean_dist(X, rs, G, gs, metric=metric)
    _against(D, ic.mean_dist_fast(X, rs, G, gs, metric), metric, "%s against %s" % (qname, gname))
    if metric == 0:
        for t, k in planted["zero"]:                         # a one-row group that is a copy of a one-row identity: exactly zero
            assert D[t, k] == 0.0, (t, k, D[t, k])
    if (gname, qname) == ("singletons", "singletons70"):
        assert len(planted["zero"]) == 3


# ---- 4. the same call twice, with the other users of the scratch buffers in between --------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_same_call_twice_same_bits_across_other_scratch_users(ctx, galleries, metric):
    """s_clu0 / s_clu1 hold the tables and D of identification, of K10 and of the search: a search and a pair_mean_dist on a larger table
    between two identical calls leave every bit of the answer as it was"""
    G, gs = galleries["cut_moved"]
    X, rs, _ = ic.query_table("main", "cut_moved", G)
    first = ctx.gallery_mean_dist(X, rs, G, gs, metric=metric)
    big, big_rs = galleries["long"]
    ctx.search(X, big, 5)
    ctx.pair_mean_dist(big, big_rs, metric=metric)
    assert len(big) > len(X) + len(G)
    second = ctx.gallery_mean_dist(X, rs, G, gs, metric=metric)
    assert np.array_equal(first.view(np.int64), second.view(np.int64))
    best = ctx.identify(X, rs, G, gs, 0.6, metric=metric, return_dist=True)
    assert np.array_equal(best[4].view(np.int64), first.view(np.int64))


# ---- 5. more than 65 535 query groups -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", sorted(ic.HUGE_GALLERIES))
def test_more_than_65535_query_groups(ctx, huge, gname):
    """T = 65 577: cross_norm_k runs in two slices of group indices (the second from group 65 535 on), with groups that span blocks --
    cross_chunks_k's -- on both sides of that index: the 20-row and the 17-row group below it, the 33-row group above.  Both metrics
    through gallery_mean_dist, the decision through identify on the D it returns.  (More than 65 535 SPANNING groups -- the slicing of
    cross_chunks_k -- would need more than a million rows: not reached here.)"""
    X, rs, gal = huge
    G, gs, Dr = gal[gname]
    T = len(rs) - 1
    for metric in (0, 1):
        D = ctx.gallery_mean_dist(X, rs, G, gs, metric=metric)
        _against(D, Dr[metric], metric, "T = %d against %s" % (T, gname))
        for what, t in ic.HUGE_NAMED.items():
            assert rs[t + 1] - rs[t] == ic.HUGE_QUERY_SIZES[t]
            assert np.allclose(D[t], Dr[metric][t], **TOL[metric]) and D[t].min() > 0, (what, metric)
    best, bd, second, sd, D = ctx.identify(X, rs, G, gs, 0.6, return_dist=True)
    _against(D, Dr[0], 0, "identify, T = %d against %s" % (T, gname))
    assert ref.same_picks((best, bd, second, sd), ref.pick(D, 0.6))
    want = np.arange(T) % ic.HUGE_CENTRES                    # the centre each group was drawn around
    assert np.array_equal(best, np.where(want < len(gs) - 1, want, -1))
