"""GPU: pvf_search (csrc/search.hip: search_quant_k, search_tiles_k, search_merge_k) and the `search` verb against the numpy restatement
of SEARCH.md, tests/search_ref.py.  Every comparison is np.array_equal: the distances are exact integers and the order (d2, index) is
total, so there is no tolerance anywhere -- but for the one cross-check against pvf_gallery_mean_dist, which has its own."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch          # noqa: F401 -- first, as in bench.py: the process then runs on the HIP runtime torch ships

from tests import search_cases as cases
from tests import search_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEAMS = [1, 15, 16, 17, 33, 255, 256, 257]


def _same(ctx, Qr, X, k, what="", **kw):
    got = ctx.search(Qr, X, k, **kw)
    want = ref.search(Qr, X, k, **kw)
    for g, w, name in zip(got, want, ("idx", "d2", "count")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5])
    return got


@pytest.fixture(scope="module")
def table():
    return cases.blobs(1, 600)


# ---- block seams ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SEAMS)
def test_table_sizes_at_block_seams(ctx, N):
    X = cases.blobs(2, N)
    _same(ctx, cases.blobs(3, 5), X, 10, what="N = %d" % N)


@pytest.mark.parametrize("Q", SEAMS)
def test_query_counts_at_block_seams(ctx, table, Q):
    _same(ctx, cases.blobs(4, Q), table[:100], 7, what="Q = %d" % Q)


def test_more_than_one_column_range(ctx, table):
    p = ctx.search_plan(20, 600, 10)
    assert p == ref.plan(20, 600, 10) and p["n_ranges"] == 3 and p["range_blocks"] == 13 and p["n_chunks"] == 1
    _same(ctx, cases.blobs(5, 20), table, 10, what="three ranges")


# ---- k -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 63, 64, 65, 299, 300, 301, 1024])
def test_k_values(ctx, table, k):
    """1; either side of the pending region's smallest size (64: k = 65 doubles it); N - 1, N, N + 1 at N = 300; the largest"""
    assert ctx.search_plan(3, 300, k)["pending"] == ref.plan(3, 300, k)["pending"] == {1: 64, 63: 64, 64: 64, 65: 128, 299: 512, 300: 512, 301: 512, 1024: 1024}[k]
    idx, d2, count = _same(ctx, cases.blobs(6, 3), table[:300], k, what="k = %d" % k)
    assert list(count) == [min(k, 300)] * 3
    if k > 300:
        assert (idx[:, 300:] == -1).all() and (d2[:, 300:] == -1).all()


def test_k_1024_against_a_longer_table(ctx):
    _same(ctx, cases.blobs(7, 2), cases.blobs(8, 2500), 1024, what="k = 1024, N = 2500")


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
def test_ties_few_distinct_distances(ctx):
    X = cases.ties(9, 3000)
    _same(ctx, np.zeros((1, 128)), X, 100, what="ties, zero query")
    _same(ctx, X[:17], X, 50, what="ties, rows as queries")


def test_identical_rows_the_index_decides(ctx):
    X = cases.identical(700)
    idx, d2, count = _same(ctx, X[:2], X, 130, what="identical rows")
    assert np.array_equal(idx[0], np.arange(130)) and (d2 == 0).all()


# ---- order of arrival ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["descending", "ascending", "shuffled"])
def test_order_of_arrival(ctx, order):
    _same(ctx, np.zeros((1, 128)), cases.ladder(2000, order), 100, what=order)


# ---- exact values --------------------------------------------------------------------------------------------------------------------
def test_queries_that_are_rows_of_the_table(ctx, table):
    idx, d2, _ = _same(ctx, table[40:90], table, 5, what="rows of the table")
    assert np.array_equal(idx[:, 0], np.arange(40, 90)) and (d2[:, 0] == 0).all()


def test_the_two_to_the_49_extreme(ctx):
    Qr, X = cases.extreme()
    idx, d2, count = _same(ctx, Qr, X, 3, what="2^49")
    assert (d2 == 1 << 49).all() and list(idx[0]) == [0, 1, 2]


def test_the_limits_of_the_quantisation(ctx, table):
    edge = (1 << 20) * 1e-5
    X = table[:40].copy()
    X[7, 3], X[20, 127] = edge, -edge
    _same(ctx, table[100:103], X, 40, what="+-2^20")
    for bad in (edge + 1e-5, -edge - 1e-5, np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y[33, 5] = bad
        Y[34, 0] = bad                                  # later in row-major order: not the one named
        with pytest.raises(Exception, match=r"X\[33\]\[5\]"):
            ctx.search(table[100:103], Y, 4)
        Qb = table[100:103].copy()
        Qb[2, 64] = bad
        with pytest.raises(Exception, match=r"Qrows\[2\]\[64\]"):
            ctx.search(Qb, X, 4)
    _same(ctx, table[100:103], X, 4, what="after the refusals")


def test_a_refused_value_in_a_later_chunk(ctx, table, monkeypatch):
    monkeypatch.setenv("PVF_SEARCH_CHUNK", "100")
    Y = table.copy()
    Y[450, 9] = np.nan
    with pytest.raises(Exception, match=r"X\[450\]\[9\]"):
        ctx.search(table[:3], Y, 4)


# ---- exclusion and cut ---------------------------------------------------------------------------------------------------------------
def test_groups_across_block_and_range_seams(ctx, table):
    rg = cases.groups_across_seams(600)
    qrows = np.array([0, 15, 16, 17, 207, 208, 209, 300, 415, 416, 599])
    qg = rg[qrows].copy()
    _same(ctx, table[qrows], table, 20, what="own group excluded", query_group=qg, row_group=rg)
    qg[::2] = -1
    rg2 = rg.copy()
    rg2[rg2 < 0] = -7                                   # every negative value means: in no group
    _same(ctx, table[qrows], table, 20, what="-1 queries exclude nothing", query_group=qg, row_group=rg2)


def test_a_query_whose_whole_table_is_excluded(ctx, table):
    rg = np.full(300, 4, np.int32)
    idx, d2, count = _same(ctx, table[:2], table[:300], 9, what="all excluded", query_group=np.array([4, 5], np.int32), row_group=rg)
    assert count[0] == 0 and (idx[0] == -1).all() and (d2[0] == -1).all() and count[1] == 9


def test_the_cut(ctx, table):
    Qr = table[:6]
    _, d2, _ = ctx.search(Qr, table, 30)
    kth = int(d2[:, 29].min())
    for cut in (kth, kth - 1, 0):
        idx, dd, count = _same(ctx, Qr, table, 30, what="max_d2 = %d" % cut, max_d2=cut)
    assert list(count) == [1] * 6 and (dd[:, 0] == 0).all()                   # max_d2 = 0: each query finds itself alone


# ---- chunks --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [16, 100, 257])
def test_chunks_give_the_bits_of_one_chunk(ctx, table, monkeypatch, chunk):
    Qr, rg = cases.blobs(10, 21), cases.groups_across_seams(600)
    qg = rg[:21].copy()
    one = ctx.search(Qr, table, 70, query_group=qg, row_group=rg)
    monkeypatch.setenv("PVF_SEARCH_CHUNK", str(chunk))
    p = ctx.search_plan(21, 600, 70)
    assert p == ref.plan(21, 600, 70, chunk) and p["n_chunks"] == -(-600 // p["chunk_rows"]) >= 3
    many = _same(ctx, Qr, table, 70, what="chunk %d" % chunk, query_group=qg, row_group=rg)
    assert all(np.array_equal(a, b) for a, b in zip(one, many))


def test_the_same_call_twice(ctx, table):
    a = ctx.search(table[:33], table, 100)
    b = ctx.search(table[:33], table, 100)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- cross-check against existing code (a check, not the criterion) -------------------------------------------------------------------
def test_distances_agree_with_gallery_mean_dist(ctx, table):
    Qr = cases.blobs(12, 9)
    idx, d2, _ = ctx.search(Qr, table, 600)
    D = ctx.gallery_mean_dist(Qr, np.arange(10, dtype=np.int32), table, np.arange(601, dtype=np.int32))
    got = np.sqrt(d2.astype(np.float64)) / 1e5
    assert np.allclose(got, np.take_along_axis(D, idx.astype(np.int64), 1), rtol=1e-12, atol=1e-13)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, table):
    Qr, X = table[:2], table[:50]
    with pytest.raises(Exception, match="dim must be 128"):
        ctx.search(Qr[:, :64], X[:, :64], 3)
    for k in (0, 1025, -1):
        with pytest.raises(Exception, match="k must lie in 1 .. 1024"):
            ctx.search(Qr, X, k)
    with pytest.raises(Exception, match="at least 1"):
        ctx.search(Qr[:0], X, 3)
    with pytest.raises(Exception, match="at least 1"):
        ctx.search(Qr, X[:0], 3)
    with pytest.raises(Exception, match="max_d2"):
        ctx.search(Qr, X, 3, max_d2=-2)
    with pytest.raises(Exception, match="together"):
        ctx.search(Qr, X, 3, query_group=np.zeros(2, np.int32))
    from pyannote_video_amd import _lib
    out = np.zeros(6, np.int64)
    assert _lib.lib().pvf_search_plan(1, (1 << 30) + 1, 1, _lib.ptr(out)) != 0 and b"2^30" in _lib.lib().pvf_last_error()
    idx, d2, cnt = np.zeros(3, np.int32), np.zeros(3, np.int64), np.zeros(1, np.int32)
    g = np.zeros(50, np.int32)
    rc = _lib.lib().pvf_search(ctx._h, _lib.ptr(Qr), 1, _lib.ptr(X), 50, 128, 3, -1, None, _lib.ptr(g), _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(cnt))
    assert rc != 0 and b"together" in _lib.lib().pvf_last_error()
    _same(ctx, Qr, X, 3, what="after the refusals")


# ---- the verb, in a process of its own -----------------------------------------------------------------------------------------------
def test_the_search_verb(tmp_path):
    from pyannote_video_amd import formats
    files = cases.two_files()
    paths = [str(tmp_path / n) for n in ("a.txt", "b.txt")]
    for p, (t, track, X) in zip(paths, files):
        with open(p, "w") as f:
            for i in range(len(t)):
                f.write(formats.embedding_line(t[i], int(track[i]), X[i]))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "pyannote-video_amd"), ROOT]))
    for extra, collapse in ((["--rows"], False), ([], True)):
        out = subprocess.run([sys.executable, "-m", "pyannote_video_amd", "search", "-k", "12", "--from", paths[0], "--track", "0"] + extra + ["-"] + paths,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        X = np.concatenate([f[2] for f in files])
        owner = [(p, int(k)) for p, f in zip(paths, files) for k in f[1]]
        times = np.concatenate([f[0] for f in files])
        skip = [o == (paths[0], 0) for o in owner]
        hits = ref.merge_brute(files[0][2][files[0][1] == 0], X, 12, skip=skip)
        if collapse:
            hits = ref.collapse(hits, owner)
        want = "".join(ref.line(r, d, owner[i][0], owner[i][1], times[i]) for r, (d, i) in enumerate(hits))
        assert out.stdout == want and len(hits) >= 2
