"""GPU: pvf_cast (csrc/cast.hip: the resident self-join through search_tiles_k / search_merge_k, cast_links_k, cast_hook_k / cast_jump_k)
and the `cast` verb against the restatement of CAST.md, tests/cast_ref.py.  Every comparison is np.array_equal: lists, miss counts,
ranks, link bytes and labels are integers and a pure function of the inputs."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch          # noqa: F401 -- first, as in bench.py: the process then runs on the HIP runtime torch ships

from tests import cast_cases as cases
from tests import cast_ref as ref
from tests import search_cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = [(0, 1), (1, 1), (2000, 1000), (1 << 20, 1)]


def _inputs(name, N):
    if name == "blobs":
        return search_cases.blobs(2, N), None
    if name == "ties":
        return search_cases.ties(3, N), None
    if name == "identical":
        return search_cases.identical(N), None
    if name == "ladder":
        return search_cases.ladder(N, "shuffled"), None
    if name == "extreme":
        a, b = search_cases.extreme()
        return np.concatenate([a, b, search_cases.blobs(5, N - 4)]), None
    if name == "groups":
        return search_cases.blobs(4, N), cases.groups_in_runs(N)
    if name == "scattered":
        return search_cases.blobs(4, N), cases.scattered_groups(N)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _want(name, N, k, max_d2):
    """the restatement, once per input: lists, then m and r (which no threshold changes)"""
    X, group = _inputs(name, N)
    idx, d2, count = ref.lists(X, k, max_d2, group)
    m, r, _ = ref.links(idx, count, 0, 1)
    for a in (idx, d2, count, m, r):
        a.setflags(write=False)
    return idx, d2, count, m, r


def _check(ctx, name, N, k, max_d2=-1, thresholds=THRESHOLDS, search_too=True):
    X, group = _inputs(name, N)
    idx, d2, count, m, r = _want(name, N, k, max_d2)
    what = (name, N, k, max_d2)
    got = ctx.cast_lists(X, k, max_d2, group)
    for g, w, part in zip(got, (idx, d2, count), ("idx", "d2", "count")):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, part, np.argwhere(g != w)[:5])
    if search_too:                                      # the same rows through pvf_search: every row its own or its group's group
        eff = (np.arange(N) + N if group is None else np.where(group >= 0, group, np.arange(N) + N)).astype(np.int32)
        for g, w, part in zip(ctx.search(X, X, k, max_d2=max_d2, query_group=eff, row_group=eff), got, ("idx", "d2", "count")):
            assert np.array_equal(g, w), (what, "search", part)
    inside = np.arange(k)[None, :] < count[:, None]
    for num, den in thresholds:
        linked = (inside & (m.astype(np.int64) * den <= num * r.astype(np.int64))).astype(np.uint8)
        gm, gr, gl = ctx.cast_links(X, k, max_d2, num, den, group)
        assert gm.dtype == np.int32 and gr.dtype == np.int32 and gl.dtype == np.uint8
        assert np.array_equal(gm, m) and np.array_equal(gr, r) and np.array_equal(gl, linked), (what, num, den, np.argwhere(gl != linked)[:5])
        lab, comps = ref.labels(idx, linked, group)
        glab, gcomps = ctx.cast(X, k, max_d2, num, den, group)
        assert glab.dtype == np.int32 and np.array_equal(glab, lab) and gcomps == comps, (what, num, den, "labels")


# ---- sizes, k and inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,k", [(1, 1), (2, 2), (15, 64), (16, 256), (17, 1), (63, 63), (64, 64), (65, 65), (257, 256), (1000, 63), (4097, 24)])
def test_sizes_and_k(ctx, N, k):
    """N at the seams of the 16-row blocks and of the 64-lane pieces of a list; k at 1, 2, either side of 64, 256, and k >= N; the
    largest table has two query batches (k = 24 keeps the restatement's set arithmetic to a few seconds)"""
    _check(ctx, "blobs", N, k, thresholds=THRESHOLDS if N < 4097 else THRESHOLDS[2:3], search_too=N < 4097)


@pytest.mark.parametrize("name,N,k,max_d2", [("ties", 1000, 64, -1), ("ties", 257, 65, 20), ("identical", 65, 2, -1), ("identical", 130, 64, 0),
                                            ("ladder", 257, 63, -1), ("ladder", 1000, 2, 40 * 40), ("extreme", 64, 64, -1),
                                            ("groups", 1000, 65, -1), ("groups", 257, 256, cases.DEFAULT_MAX_D2), ("scattered", 1000, 20, -1)])
def test_inputs(ctx, name, N, k, max_d2):
    _check(ctx, name, N, k, max_d2)


@pytest.mark.parametrize("chunk", [16, 256, None])
@pytest.mark.parametrize("qblock", [16, 48, None])
def test_batches_and_chunks_give_the_same_bits(ctx, monkeypatch, qblock, chunk):
    """1000 rows: 63 batches of 16 with a last one of 8, 21 of 48 with a last one of 40; 63 chunks of 16 rows, 4 of 256; groups whose
    rows lie in every batch"""
    if qblock:
        monkeypatch.setenv("PVF_CAST_QBLOCK", str(qblock))
    if chunk:
        monkeypatch.setenv("PVF_SEARCH_CHUNK", str(chunk))
    p = ctx.cast_plan(1000, 20)
    assert p["qblock"] == (qblock or 1008) and p["n_batches"] == -(-1000 // p["qblock"]) and p["chunk_rows"] == (chunk or 1008)
    assert p["n_chunks"] == -(-1000 // p["chunk_rows"]) and p["device_bytes"] > 1000 * 512
    _check(ctx, "scattered", 1000, 20, thresholds=THRESHOLDS[2:3], search_too=False)
    _check(ctx, "groups", 1000, 65, thresholds=THRESHOLDS[1:2], search_too=False)


# ---- labels --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", cases.PATHS)
def test_a_path_is_one_component(ctx, n, k):
    """one component, in fewer launches of the components kernels than the graph is links across: a labelling that moved one link a
    round could not do that (pointer jumping flattens a chain of d rows in log2 d launches)"""
    X = cases.path(n)
    ctx.prof_reset(); ctx.prof_enable(True)
    try:
        lab, comps = ctx.cast(X, k, -1, 1, 1)
    finally:
        ctx.prof_enable(False)
    launches = ctx.prof_get("cast_cc")[1]
    want, wcomps = ref.cast(X, k, -1, 1, 1)
    assert np.array_equal(lab, want) and comps == wcomps == 1
    across = cases.path_links_across(n, k)                # tests/test_cast_ref.py holds the case to this by a breadth-first walk
    print("components launches", launches, "links across", across)
    assert 0 < launches < across // 2


@pytest.mark.parametrize("n,identities,k", cases.PLANTED)
def test_planted_identities(ctx, n, identities, k):
    X, who = cases.planted(1, n, identities)
    lab, comps = ctx.cast(X, k, cases.DEFAULT_MAX_D2, 2000, 1000)
    want, wcomps = ref.cast(X, k, cases.DEFAULT_MAX_D2, 2000, 1000)
    assert np.array_equal(lab, want) and comps == wcomps == identities and cases.pure_and_complete(lab, who)


def test_everyone_in_one_group(ctx):
    X, g = search_cases.blobs(9, 300), np.full(300, 299, np.int32)
    idx, d2, count = ctx.cast_lists(X, 5, group=g)
    assert (count == 0).all() and (idx == -1).all() and (d2 == -1).all()
    m, r, linked = ctx.cast_links(X, 5, group=g)
    assert (m == -1).all() and (r == -1).all() and (linked == 0).all()
    lab, comps = ctx.cast(X, 5, group=g)
    assert (lab == 0).all() and comps == 1 and np.array_equal(lab, ref.cast(X, 5, group=g)[0])


def test_all_singletons_under_a_cut_of_zero(ctx):
    X = cases.distinct_rows(257)
    lab, comps = ctx.cast(X, 8, max_d2=0)
    assert np.array_equal(lab, np.arange(257, dtype=np.int32)) and comps == 257 and (ctx.cast_lists(X, 8, max_d2=0)[2] == 0).all()


def test_host_arrays_at_unaligned_addresses(ctx):
    X, g = _inputs("groups", 257)
    bx, bg = np.zeros(X.nbytes + 1, np.uint8), np.zeros(g.nbytes + 1, np.uint8)
    Xu, gu = bx[1:].view(np.float64).reshape(X.shape), bg[1:].view(np.int32)
    Xu[...], gu[...] = X, g
    assert not Xu.flags.aligned and not gu.flags.aligned and Xu.flags.c_contiguous
    lab, comps = ctx.cast(Xu, 9, cases.DEFAULT_MAX_D2, 2000, 1000, gu)
    want, wcomps = ref.cast(X, 9, cases.DEFAULT_MAX_D2, 2000, 1000, g)
    assert np.array_equal(lab, want) and comps == wcomps


def test_calls_in_either_order_and_after_other_work(ctx):
    A, B = search_cases.blobs(11, 300), cases.planted(2, 600, 6)[0]
    wa, wb = ref.cast(A, 10, -1, 1, 1)[0], ref.cast(B, 70, cases.DEFAULT_MAX_D2)[0]
    for first in (0, 1):
        for i in (first, 1 - first, first):
            got = ctx.cast(A, 10, -1, 1, 1)[0] if i == 0 else ctx.cast(B, 70, cases.DEFAULT_MAX_D2)[0]
            assert np.array_equal(got, wa if i == 0 else wb)
    ctx.search(A[:5], B, 1024)                            # the search's and the clustering's buffers are the cast's
    ctx.cluster_tracks(B, np.arange(0, 601, 3, dtype=np.int32), 0.6)
    assert np.array_equal(ctx.cast(A, 10, -1, 1, 1)[0], wa) and np.array_equal(ctx.cast(B, 70, cases.DEFAULT_MAX_D2)[0], wb)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refused_values_write_nothing(ctx):
    from pyannote_video_amd import _lib
    X = search_cases.blobs(12, 100)
    edge = (1 << 20) * 1e-5
    for bad in (np.nan, np.inf, edge + 1e-5, -edge - 1e-5):
        Y = X.copy()
        Y[70, 9] = bad
        Y[71, 0] = bad                                  # later in row-major order: not the one named
        labels, n = np.full(100, -7, np.int32), np.full(1, -7, np.int32)
        rc = _lib.lib().pvf_cast(ctx._h, _lib.ptr(Y), 100, 128, 5, -1, 2000, 1000, None, _lib.ptr(labels), _lib.ptr(n))
        msg = _lib.lib().pvf_last_error()
        assert rc != 0 and b"pvf_cast: X[70][9] is not finite or lies beyond 2^20" in msg, msg
        assert (labels == -7).all() and n[0] == -7
        with pytest.raises(Exception, match=r"X\[70\]\[9\]"):
            ctx.cast_lists(Y, 5)
    Y = X.copy()
    Y[3, 3], Y[99, 127] = edge, -edge                     # the largest values that are taken
    assert np.array_equal(ctx.cast(Y, 5)[0], ref.cast(Y, 5)[0])


def test_refused_limits(ctx):
    from pyannote_video_amd import _lib
    X = search_cases.blobs(13, 50)
    for kw, message in ((dict(k=0), "k must lie in 1 .. 256"), (dict(k=257), "k must lie in 1 .. 256"), (dict(max_d2=-2), "max_d2 must be at least -1"),
                        (dict(num=-1), "num must lie in 0 .. 2\\^20"), (dict(num=(1 << 20) + 1), "num must lie in 0 .. 2\\^20"),
                        (dict(den=0), "den must lie in 1 .. 2\\^20"), (dict(den=(1 << 20) + 1), "den must lie in 1 .. 2\\^20"),
                        (dict(group=np.full(50, 50, np.int32)), "a group must be negative \\(none\\) or below N")):
        with pytest.raises(Exception, match=message):
            ctx.cast(X, **dict(dict(k=4), **kw))
    with pytest.raises(Exception, match="dim must be 128"):
        ctx.cast(X[:, :64], 4)
    with pytest.raises(Exception, match="N must lie in 1 .. 2\\^24"):
        ctx.cast(X[:0], 4)
    out = np.zeros(6, np.int64)
    assert _lib.lib().pvf_cast_plan((1 << 24) + 1, 4, _lib.ptr(out)) != 0 and b"2^24" in _lib.lib().pvf_last_error()
    assert _lib.lib().pvf_cast_plan(1 << 24, 64, _lib.ptr(out)) == 0 and out[1] == (1 << 24) // 4096
    with pytest.raises(Exception, match="k must lie in 1 .. 256"):
        ctx.cast_lists(X, 300)
    with pytest.raises(Exception, match="den must lie"):
        ctx.cast_links(X, 4, den=0)
    g = np.full(50, -5, np.int32)
    g[10:20] = 49
    assert np.array_equal(ctx.cast(X, 4, group=g)[0], ref.cast(X, 4, group=g)[0])          # the context goes on working


# ---- the verb, in a process of its own -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by", ["track", "face"])
def test_the_cast_verb(tmp_path, by):
    from pyannote_video_amd import formats, identification
    files = search_cases.two_files()
    paths = [str(tmp_path / n) for n in ("a.txt", "b.txt")]
    for p, (t, track, X) in zip(paths, files):
        with open(p, "w") as f:
            for i in range(len(t)):
                f.write(formats.embedding_line(t[i], int(track[i]), X[i]))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "pyannote-video_amd"), ROOT]))
    graph = str(tmp_path / "graph.npz")
    out = subprocess.run([sys.executable, "-m", "pyannote_video_amd", "cast", "--by", by, "-k", "6", "--labels", ".persons", "--graph", graph, "-"] + paths,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    table = [(p, f[1], f[2]) for p, f in zip(paths, files)]
    want = ref.verb(table, 6, cases.DEFAULT_MAX_D2, 2000, 1000, by)
    assert out.stdout == "".join("%s %d %d\n" % l for l in want)
    assert [l[2] for l in want] == [0, 1, 0, 2, 1, 3, 0, 4]                   # the persons search_cases.two_files plants
    for p in paths:
        assert identification.read_label_map(p + ".persons") == {t: person for q, t, person in want if q == p}
    g = np.load(graph)
    idx, d2, count = ref.lists(g["X"], 6, cases.DEFAULT_MAX_D2, None if by == "track" else g["owner"])
    assert np.array_equal(g["idx"], idx) and np.array_equal(g["d2"], d2) and np.array_equal(g["count"], count)
    assert len(g["X"]) == (8 if by == "track" else 44)
