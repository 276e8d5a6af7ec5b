"""GPU: the do-not-cooccur constraint inside the agglomeration kernels (csrc/cluster.hip: cooccur_stamp_k, hac_persist_k<U, true>,
hac_merge_k<true>) through the C ABI's pvf_cluster_*_cooccur entries, against tests/cooccur_ref.py (numpy: a boolean mask, a masked
arg-min, one IEEE division) and, at finite thresholds, against the unchanged oracle agglomeration on a stamped matrix.  Everything is
compared bit for bit: labels, the merge log (kept, merged, distance, size) and the number of forbidden pairs.  The distance matrix both
references start from is the device's own (pvf_pair_mean_dist, pinned against the oracle elsewhere), so what is under test here is the
agglomeration alone.

Sizes: 2 and 3 (nothing mergeable), 33 (the alive bits' word boundary), 1024 / 1025 (one / three entries per thread of the persistent
kernel), 3073 (the smallest with ten), 300 for the launch-per-merge path and `force`."""
import numpy as np
import pytest
import torch          # noqa: F401  first, as in bench.py: the process then runs on the HIP runtime torch ships

from tests import cooccur_ref as R

pytestmark = pytest.mark.gpu

# at T = 3073 the threshold is low enough that the O(T^2)-per-merge references make a few hundred merges, not three thousand
THRESHOLD = {3073: 0.246}
_cache = {}


def case(ctx, oracle, T, threshold=None):
    """(X, row_start, extent, D, reference labels, reference log) for the seeded case of T tracks, made once"""
    threshold = THRESHOLD.get(T, 0.6) if threshold is None else threshold
    if T not in _cache:
        X, rs, ext = R.make(T, seed=100 + T)
        _cache[T] = (X, rs, ext, ctx.pair_mean_dist(X, rs))
    X, rs, ext, D = _cache[T]
    key = (T, threshold)
    if key not in _cache:
        _cache[key] = R.hac(D, np.diff(rs), threshold, R.cooccur(ext))
    return (X, rs, ext, D) + _cache[key]


def same(got, labels, log, nb):
    assert np.array_equal(got[0], labels)
    assert got[1].shape == log.shape and np.array_equal(got[1], log)      # bit for bit: kept, merged, distance, size
    assert not np.isnan(got[1]).any()
    assert got[2] == nb


def test_two_tracks_and_three_all_forbidden(ctx):
    X, rs, _ = R.make(3, seed=1, identities=1)
    for T, ext, nb in ((2, [[0.0, 2.0], [1.0, 3.0]], 1), (3, [[0.0, 2.0], [1.0, 3.0], [0.5, 1.5]], 3)):
        for threshold in (0.6, np.inf):
            labels, log, n = ctx.cluster_tracks_cooccur(X[:rs[T]], rs[:T + 1], threshold, extent=ext)
            assert labels.tolist() == list(range(T)) and len(log) == 0 and n == nb
        for flags in (0, 1):      # ... and free to merge: one identity, one cluster
            labels, log, n = ctx.cluster_tracks_cooccur(X[:rs[T]], rs[:T + 1], 0.6, extent=R.disjoint_extents(T), flags=flags)
            assert labels.tolist() == [0] * T and len(log) == T - 1 and n == 0


@pytest.mark.parametrize("T", (33, 300, 1024, 1025, 3073))
def test_persistent_kernel_equals_reference_and_oracle(ctx, oracle, T):
    X, rs, ext, D, labels, log = case(ctx, oracle, T)
    threshold = THRESHOLD.get(T, 0.6)
    nb = R.n_blocked(ext)
    assert nb > 0 and 0 < len(log) < T - 1 and (T != 3073 or len(log) <= 600)
    got = ctx.cluster_tracks_cooccur(X, rs, threshold, extent=ext)
    same(got, labels, log, nb)
    lo, logo = oracle.hac(R.stamp(D, ext), np.diff(rs), threshold)
    assert np.array_equal(got[0], lo) and np.array_equal(got[1], logo)
    assert R.violations(got[0], ext) == 0
    if T == 300:
        # in substance: the same call without the constraint puts tracks that are on screen together into one cluster
        free, _ = ctx.cluster_tracks(X, rs, threshold)
        assert R.violations(free, ext) > 0 and len(set(free.tolist())) < len(set(got[0].tolist()))


@pytest.mark.parametrize("T", (33, 300))
def test_launch_per_merge_path_equals_persistent(ctx, oracle, T):
    X, rs, ext, D, labels, log = case(ctx, oracle, T)
    nb = R.n_blocked(ext)
    same(ctx.cluster_tracks_cooccur(X, rs, 0.6, extent=ext, flags=1), labels, log, nb)
    same(ctx.cluster_dist_cooccur(D, rs, 0.6, extent=ext, flags=1), labels, log, nb)
    # ... and with `force`
    lf, logf = R.hac(D, np.diff(rs), np.inf, R.cooccur(ext))
    same(ctx.cluster_tracks_cooccur(X, rs, np.inf, extent=ext, flags=1), lf, logf, nb)


def test_force_runs_until_nothing_is_mergeable(ctx, oracle):
    X, rs, ext, D, _, _ = case(ctx, oracle, 300)
    labels, log = R.hac(D, np.diff(rs), np.inf, R.cooccur(ext))
    got = ctx.cluster_tracks_cooccur(X, rs, np.inf, extent=ext)
    same(got, labels, log, R.n_blocked(ext))
    assert np.isfinite(got[1][:, 2]).all()                    # no forbidden pair was merged
    assert len(set(got[0].tolist())) > 1 and R.violations(got[0], ext) == 0
    assert len(log) > len(case(ctx, oracle, 300)[5])          # it went on past the threshold


@pytest.mark.parametrize("T", (300, 1025))
def test_extents_that_never_intersect_change_nothing(ctx, oracle, T):
    X, rs, _, D, _, _ = case(ctx, oracle, T)
    for threshold in (0.6, np.inf):
        l0, log0 = ctx.cluster_tracks(X, rs, threshold)
        l1, log1, nb = ctx.cluster_tracks_cooccur(X, rs, threshold, extent=R.disjoint_extents(T))
        assert nb == 0 and np.array_equal(l0, l1) and log0.shape == log1.shape and np.array_equal(log0, log1)


def test_boundary_extents(ctx):
    """six tracks of one identity (any two would merge): which pairs the stamp forbids decides the clusters"""
    X, rs, _ = R.make(6, seed=2, identities=1)
    D = ctx.pair_mean_dist(X, rs)
    assert D.max() < 0.6
    up = float(np.nextafter(1e-6, 1.0))
    for name, ext, nb in (
            ("touching", [[0, 5], [5, 9], [9, 12], [12, 13], [13, 20], [20, 21]], 0),
            ("an overlap of exactly 1e-6", [[0, 5], [-3, 1e-6], [10, 11], [12, 13], [14, 15], [16, 17]], 0),
            ("the next float64 above 1e-6", [[0, 5], [-3, up], [10, 11], [12, 13], [14, 15], [16, 17]], 1),
            ("identical extents", [[1, 2]] * 6, 15),
            ("one track containing all others", [[0, 100], [1, 2], [3, 4], [5, 6], [7, 8], [9, 10]], 5),
            ("the containing track last", [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [0, 100]], 5)):
        ext = np.array(ext, np.float64)
        assert R.n_blocked(ext) == nb, name
        for threshold in (0.6, np.inf):
            labels, log = R.hac(D, np.diff(rs), threshold, R.cooccur(ext))
            for flags in (0, 1):
                same(ctx.cluster_tracks_cooccur(X, rs, threshold, extent=ext, flags=flags), labels, log, nb)
        assert len(set(labels.tolist())) == {0: 1, 1: 2, 15: 6, 5: 2}[nb], name


class _OneRank(object):
    """the exchange step of a job of one rank: everybody's rows are this rank's"""
    on_host = True

    def allgather(self, t):
        return t.clone(), [int(t.shape[0])]


def _rows_of(rs, ext):
    """(time, track) columns whose tracks have exactly the extents `ext` (first row at the start, last at the end)"""
    time, track = [], []
    for k in range(len(rs) - 1):
        n = int(rs[k + 1] - rs[k])
        time += np.linspace(ext[k, 0], ext[k, 1], n).tolist()[:-1] + [ext[k, 1]]
        track += [1000 + 7 * k] * n
    return np.array(time, np.float64), np.array(track, np.int64)


@pytest.mark.parametrize("metric", ("euclidean", "cosine"))
def test_every_entry_form_agrees(ctx, oracle, monkeypatch, metric):
    from pyannote_video_amd import dist
    from pyannote_video_amd.clustering import FaceClustering
    T = 300
    X, rs, ext, D, labels, log = case(ctx, oracle, T)
    threshold, m = 0.6, 0
    if metric == "cosine":
        threshold, m = 0.25, 1
        D = ctx.pair_mean_dist(X, rs, metric=1)
        labels, log = R.hac(D, np.diff(rs), threshold, R.cooccur(ext))
        assert 0 < len(log) < T - 1
    nb = R.n_blocked(ext)
    E = X.astype(np.float32)                       # round(float64(E), 5) on the device gives X back (|x| < 0.5: float32 is exact to 3e-8)
    same(ctx.cluster_dist_cooccur(D, rs, threshold, extent=ext), labels, log, nb)                              # a float64 matrix
    same(ctx.cluster_tracks_f32_cooccur(E, None, rs, threshold, decimals=5, metric=m, extent=ext), labels, log, nb)     # float32 rows, device rounding
    time, track = _rows_of(rs, ext)
    want = {int(track[rs[t]]): int(track[rs[labels[t]]]) for t in range(T)}
    perm = np.random.default_rng(3).permutation(len(time))      # rows in any order: plan_rows finds the tracks and their extents
    fc = FaceClustering(threshold=threshold, metric=metric, ctx=ctx, constraint="cooccur")
    assert fc.cluster_rows(time[perm], track[perm], E[perm]) == want and fc.n_blocked == nb
    fc.n_blocked = None
    sp, feats = fc.model.preprocess((time[perm], track[perm], X[perm]))
    res = fc(sp, features=feats)                                 # the reference's usage contract: preprocess + __call__ (float64 table)
    assert {int(t): int(l) for _, t, l in res.itertracks(yield_label=True)} == want and fc.n_blocked == nb
    if metric == "euclidean":
        same(ctx.cluster_tracks_cooccur(X, rs, threshold, extent=ext), labels, log, nb)                        # the float64 table
        same(ctx.cluster_upper_cooccur(ctx.pair_upper_rows(X, rs, 0, T), rs, threshold, extent=ext), labels, log, nb)
        # the split form with one rank: upper-triangle rows -> exchange -> every rank mirrors, stamps and agglomerates
        monkeypatch.setitem(dist._exchange, "tried", True)
        monkeypatch.setitem(dist._exchange, "comm", _OneRank())
        sh = FaceClustering(threshold=threshold, ctx=ctx, constraint="cooccur")
        sh.shard = dist.DistanceShard(0, 1, device="cpu")
        assert sh.cluster_rows(time[perm], track[perm], E[perm]) == want and sh.n_blocked == nb
        sh.n_blocked = None
        res = sh(sp, features=feats)
        assert {int(t): int(l) for _, t, l in res.itertracks(yield_label=True)} == want and sh.n_blocked == nb
        # `force`: the history goes on, the partition is the one at the threshold
        ff = FaceClustering(threshold=threshold, force=True, ctx=ctx, constraint="cooccur")
        assert ff.cluster_rows(time, track, E) == want and len(ff.history) > len(log)


def test_pipeline_and_cluster_verb(ctx, oracle, model_paths, small_video, tmp_path):
    """FacePipeline.run(cluster=True) and the `cluster` verb on the embedding file it would write: the faces of one shot are on screen
    together, so with a threshold that merges everything they are what is left apart"""
    from pyannote_video_amd import cli, formats, pipeline
    from pyannote_video_amd.clustering import FaceClustering
    v = small_video
    frames = [ctx.upload(v.frame(i)) for i in range(v.n_frames)]
    times = [v.timestamp(i) for i in range(v.n_frames)]
    pipe = pipeline.FacePipeline(ctx, model_paths[0], model_paths[1], threshold=1e3, constraint="cooccur")
    res = pipe.run(frames, times, v.frame_rate, v.shots())
    labels = res["labels"]
    ids, order, rs, ext = FaceClustering.plan_rows(res["face_T"], res["face_id"], extents=True)
    nb = R.n_blocked(ext)
    assert len(ids) >= 4 and nb > 0 and pipe.clustering.n_blocked == nb
    lab = np.array([labels[int(t)] for t in ids])
    assert R.violations(lab, ext) == 0 and 1 < len(set(lab.tolist())) < len(ids)
    free = FaceClustering(threshold=1e3, ctx=ctx).cluster_rows(res["face_T"], res["face_id"], res["embeddings"])
    assert R.violations(np.array([free[int(t)] for t in ids]), ext) > 0 and len(set(free.values())) == 1
    # against the restatement, from the table the reference would read back
    Xq = np.round(res["embeddings"].astype(np.float64), 5)[order]
    want, _ = R.hac(ctx.pair_mean_dist(Xq, rs), np.diff(rs), 1e3, R.cooccur(ext))
    assert lab.tolist() == [int(ids[l]) for l in want]
    # the verb
    em, out = str(tmp_path / "embedding.txt"), str(tmp_path / "labels.txt")
    with open(em, "wb") as f:
        f.write(formats.embedding_rows(res["face_T"], res["face_id"], res["embeddings"]))
    assert cli.main(["cluster", "--do-not-cooccur", "--threshold", "1000", em, out]) == 0
    rows = dict(tuple(int(x) for x in l.split()) for l in open(out).read().splitlines())
    assert {t: rows[t] for t in labels} == labels
    assert cli.main(["cluster", "--threshold", "1000", em, out]) == 0
    rows = dict(tuple(int(x) for x in l.split()) for l in open(out).read().splitlines())
    assert len(set(rows[int(t)] for t in ids)) == 1


def test_refused_inputs(ctx):
    from pyannote_video_amd import _lib
    X, rs, ext = R.make(5, seed=4)
    bad = ext.copy(); bad[2, 1] = np.nan
    with pytest.raises(_lib.PvfError, match="not finite"):
        ctx.cluster_tracks_cooccur(X, rs, 0.6, extent=bad)
    bad = ext.copy(); bad[0, 0] = np.inf
    with pytest.raises(_lib.PvfError, match="not finite"):
        ctx.cluster_dist_cooccur(ctx.pair_mean_dist(X, rs), rs, 0.6, extent=bad)
    bad = ext.copy(); bad[3] = bad[3, ::-1]
    with pytest.raises(_lib.PvfError, match="ends before it starts"):
        ctx.cluster_tracks_f32_cooccur(X.astype(np.float32), None, rs, 0.6, extent=bad)
    with pytest.raises(_lib.PvfError, match="unknown flags"):
        ctx.cluster_tracks_cooccur(X, rs, 0.6, extent=ext, flags=2)
    with pytest.raises(ValueError):
        ctx.cluster_tracks_cooccur(X, rs, 0.6, extent=ext[:4])
    # the entry itself refuses a missing extent: the entries without a constraint stay for that
    import ctypes as C
    labels, n, nb = np.zeros(5, np.int32), C.c_int32(0), C.c_int32(0)
    rc = _lib.lib().pvf_cluster_tracks_cooccur(ctx._h, _lib.ptr(X), X.shape[0], 128, _lib.ptr(rs), 5, 0.6, _lib.ptr(labels), None, C.byref(n),
                                               None, C.byref(nb), 0)
    assert rc < 0 and b"extent" in _lib.lib().pvf_last_error()
    # ... and the context is as usable as before
    assert ctx.cluster_tracks_cooccur(X, rs, 0.6, extent=ext)[2] == R.n_blocked(ext)
