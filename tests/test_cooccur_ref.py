"""CPU: tests/cooccur_ref.py -- the numpy restatement of the do-not-cooccur constraint (clustering.py:142-143 names it and leaves it
off; [EXT], parity unpinned) that tests/test_gpu_cooccur.py holds the kernels to -- checked against the unchanged oracle agglomeration
on a stamped matrix, against the definition (means over union blocks of an N x N pdist), and for the properties the constraint promises.
Plus the CLI flags and the library's exports."""
import numpy as np
import pytest

from tests import cooccur_ref as R

SIZES = (2, 3, 33, 300, 1100)


@pytest.fixture(scope="module")
def cases(oracle):
    """{T: (X, row_start, extent, D)} with D the oracle's track-pair means, made once"""
    out = {}
    for T in SIZES:
        X, rs, ext = R.make(T, seed=100 + T)
        out[T] = (X, rs, ext, oracle.pair_mean_dist(X, rs))
    return out


@pytest.mark.parametrize("T", SIZES)
@pytest.mark.parametrize("threshold", (0.6, 0.35))
def test_reference_equals_unchanged_oracle_on_stamped_matrix(oracle, cases, T, threshold):
    """a forbidden pair is a pair at distance +inf: the oracle's plain average linkage on the stamped matrix takes the same decisions,
    bit for bit, at a finite threshold -- and its log holds no NaN"""
    X, rs, ext, D = cases[T]
    labels, log = R.hac(D, np.diff(rs), threshold, R.cooccur(ext))
    lo, logo = oracle.hac(R.stamp(D, ext), np.diff(rs), threshold)
    assert np.array_equal(labels, lo)
    assert log.shape == logo.shape and np.array_equal(log, logo) and not np.isnan(logo).any()


def test_oracle_is_no_reference_for_force(oracle, cases):
    """with threshold = +inf the oracle DOES merge the +inf pairs: only the restatement states `force`"""
    X, rs, ext, D = cases[300]
    lo, logo = oracle.hac(R.stamp(D, ext), np.diff(rs), np.inf)
    labels, log = R.hac(D, np.diff(rs), np.inf, R.cooccur(ext))
    assert np.isinf(logo[:, 2]).any() and len(set(lo.tolist())) == 1
    assert np.isfinite(log[:, 2]).all() and len(set(labels.tolist())) > 1 and R.violations(labels, ext) == 0
    assert R.violations(lo, ext) > 0


def test_reference_distances_equal_union_block_means(cases):
    """the Lance-Williams distance of every merge in the log == the mean over the union block of the N x N pdist (clustering.py:116-119)"""
    X, rs, ext, D = cases[300]
    labels, log = R.hac(D, np.diff(rs), 0.6, R.cooccur(ext))
    P = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    rows = {t: list(range(rs[t], rs[t + 1])) for t in range(300)}
    assert len(log) > 100
    for a, b, d, size in log:
        a, b = int(a), int(b)
        assert abs(P[np.ix_(rows[a], rows[b])].mean() - d) <= 1e-12
        rows[a] += rows.pop(b)
        assert len(rows[a]) == size


@pytest.mark.parametrize("T", (33, 300, 1100))
@pytest.mark.parametrize("threshold", (0.6, np.inf))
def test_no_violation_and_maximal(cases, T, threshold):
    """no cluster holds a co-occurring pair; every pair of final clusters whose mean distance is within the threshold is forbidden"""
    X, rs, ext, D = cases[T]
    F = R.cooccur(ext)
    labels, log = R.hac(D, np.diff(rs), threshold, F)
    assert R.violations(labels, ext) == 0
    sizes = np.diff(rs).astype(np.float64)
    reps = sorted(set(labels.tolist()))
    member = np.stack([(labels == r) * sizes for r in reps])                      # [clusters, T], weighted by rows
    mean = member @ D @ member.T / np.outer(member.sum(1), member.sum(1))         # mean over the union block of each pair of clusters
    blocked = ((np.stack([labels == r for r in reps]).astype(np.int64) @ F.astype(np.int64)) @ np.stack([labels == r for r in reps]).T.astype(np.int64)) > 0
    iu = np.triu_indices(len(reps), 1)
    # (1e-12: `mean` is recomputed from the blocks, the loop's value is the chain of weighted means; both are within 1e-12 of the definition)
    assert blocked[iu][mean[iu] <= threshold - 1e-12].all()
    assert len(reps) > 1


@pytest.mark.parametrize("T", (33, 300))
def test_without_cooccurring_tracks_nothing_changes(oracle, cases, T):
    X, rs, ext, D = cases[T]
    free = R.disjoint_extents(T)
    assert R.n_blocked(free) == 0
    for threshold in (0.6, np.inf):
        l0, log0 = R.hac(D, np.diff(rs), threshold)
        l1, log1 = R.hac(D, np.diff(rs), threshold, R.cooccur(free))
        lo, logo = oracle.hac(D, np.diff(rs), threshold)
        assert np.array_equal(l0, l1) and np.array_equal(log0, log1)
        assert np.array_equal(l0, lo) and np.array_equal(log0, logo)


@pytest.mark.parametrize("T", (33, 300, 1100))
def test_twins_fixture_is_not_vacuous(oracle, cases, T):
    """the generator's co-occurring tracks include pairs of ONE identity: the unconstrained agglomeration puts them together"""
    X, rs, ext, D = cases[T]
    lo, _ = oracle.hac(D, np.diff(rs), 0.6)
    frac = R.n_blocked(ext) / (T * (T - 1) / 2.0)
    assert 0.01 < frac < 0.08
    assert R.violations(lo, ext) > 0
    labels, _ = R.hac(D, np.diff(rs), 0.6, R.cooccur(ext))
    assert len(set(labels.tolist())) > len(set(lo.tolist()))


def test_stamp_expression_at_the_boundary():
    """min(end) - max(start) > 1e-6, in float64, in that form"""
    up = np.nextafter(1e-6, 1.0)
    assert R.n_blocked([[0.0, 5.0], [5.0, 9.0]]) == 0                  # touching
    assert R.n_blocked([[0.0, 5.0], [-3.0, 1e-6]]) == 0                # an overlap of exactly 1e-6
    assert R.n_blocked([[0.0, 5.0], [-3.0, up]]) == 1                  # the next float64 above
    assert R.n_blocked([[1.0, 2.0], [1.0, 2.0], [1.0, 2.0]]) == 3      # identical extents
    assert R.n_blocked([[0.0, 100.0], [1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]) == 3    # one track containing all others
    m = R.cooccur([[0.0, 100.0], [1.0, 2.0], [3.0, 4.0]])
    assert np.array_equal(m, m.T) and not m.diagonal().any()


def test_cli_flags_parse():
    from pyannote_video_amd import cli
    a = cli.parse_args(["cluster", "--do-not-cooccur", "emb.txt", "labels.txt"])
    assert a.do_not_cooccur is True and a.threshold == 0.6
    assert cli.parse_args(["cluster", "emb.txt", "labels.txt"]).do_not_cooccur is False
    a = cli.parse_args(["process", "--do-not-cooccur", "--labels", "l.txt", "v.npy", "s.json", "lm", "em", "t", "l", "e"])
    assert a.do_not_cooccur is True
    assert cli.parse_args(["process", "v.npy", "s.json", "lm", "em", "t", "l", "e"]).do_not_cooccur is False


def test_library_exports_the_constrained_entries():
    from pyannote_video_amd import _lib
    l = _lib.lib()
    for name in ("pvf_cluster_dist_cooccur", "pvf_cluster_upper_cooccur", "pvf_cluster_tracks_cooccur", "pvf_cluster_tracks_f32_cooccur"):
        assert name in _lib.EXPORTS and hasattr(l, name)


def test_python_surface():
    """the keyword, its refusal of other values, extents out of plan_rows, and no path that drops the constraint silently"""
    from pyannote_video_amd.clustering import FaceClustering
    with pytest.raises(ValueError):
        FaceClustering(constraint="never")
    fc = FaceClustering(constraint="cooccur")
    assert fc.constraint == "cooccur" and fc.n_blocked is None and FaceClustering().constraint is None
    time = np.array([0.0, 0.5, 1.0, 0.2, 0.2, 3.0, 3.5])
    track = np.array([7, 7, 7, 9, 9, 4, 4])
    ids, order, rs, ext = FaceClustering.plan_rows(time, track, extents=True)
    assert ids.tolist() == [4, 7] and ext.tolist() == [[3.0, 3.5], [0.0, 1.0]] and ext.dtype == np.float64      # track 9: one timestamp, left out
    assert len(FaceClustering.plan_rows(time, track)) == 3
    with pytest.raises(ValueError, match="timestamps"):
        fc.cluster_arrays(np.array([4, 7]), track, np.zeros((7, 128)))
