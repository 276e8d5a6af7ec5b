"""GPU: identification against a gallery through the C ABI (csrc/identify.hip: cross_tiles_k, identify_pick_k; pvf_gallery_mean_dist,
pvf_identify_dist, pvf_identify) and through the verbs, against tests/identify_ref.py.  The shapes are the smallest at which the
rectangular tile kernel can still go wrong; the tolerances are those of tests/test_gpu_parity.py for K10 (the same arithmetic against
the same kind of reference): Euclidean rtol 1e-12 / atol 1e-13, cosine rtol 1e-10 / atol 1e-12.  The decision is bit-exact."""
import numpy as np
import pytest
import torch          # noqa: F401 -- first, as in bench.py: the process then runs on the HIP runtime torch ships

from tests import identify_ref as ref

pytestmark = pytest.mark.gpu

TOL = {0: dict(rtol=1e-12, atol=1e-13), 1: dict(rtol=1e-10, atol=1e-12)}


@pytest.fixture(scope="module")
def main_case():
    X, rs, G, gs = ref.main_case()
    return X, rs, G, gs, {m: ref.mean_dist(X, rs, G, gs, m) for m in (0, 1)}


def _blobs(seed, q_sizes, g_sizes, spread=0.7, noise=0.15):
    rng = np.random.default_rng(seed)
    centres = spread * rng.standard_normal((max(len(q_sizes), len(g_sizes)), 128)) / np.sqrt(128.0)
    X = np.concatenate([centres[i] + noise / np.sqrt(128.0) * rng.standard_normal((n, 128)) for i, n in enumerate(q_sizes)])
    G = np.concatenate([centres[k] + noise / np.sqrt(128.0) * rng.standard_normal((n, 128)) for k, n in enumerate(g_sizes)])
    return np.round(X, 5), ref.starts(q_sizes), np.round(G, 5), ref.starts(g_sizes)


def _check(ctx, X, rs, G, gs, metrics=(0, 1), what=""):
    for m in metrics:
        D = ctx.gallery_mean_dist(X, rs, G, gs, metric=m)
        Dr = ref.mean_dist(X, rs, G, gs, m)
        err = np.abs(D - Dr)
        print("%s metric %d: %d x %d, worst |D - ref| = %.3g (ref up to %.3g)" % (what, m, D.shape[0], D.shape[1], err.max(), np.abs(Dr).max()))
        assert D.shape == Dr.shape and np.allclose(D, Dr, **TOL[m]), (what, m)
    return D


# ---- distances -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1])
def test_main_case_distances(ctx, main_case, metric):
    X, rs, G, gs, Dr = main_case
    D = ctx.gallery_mean_dist(X, rs, G, gs, metric=metric)
    print("metric %d: worst |D - ref| = %.3g" % (metric, np.abs(D - Dr[metric]).max()))
    assert D.shape == (20, 17) and np.allclose(D, Dr[metric], **TOL[metric])
    assert np.array_equal(D, ctx.gallery_mean_dist(X, rs, G, gs, metric=metric))          # the same call twice: the same bits
    # the T x K corner of K10's matrix on the concatenated table: a cross-check against existing code, not the criterion
    full = ctx.pair_mean_dist(np.concatenate([X, G]), np.concatenate([rs, gs[1:] + rs[-1]]).astype(np.int32), metric=metric)
    assert np.allclose(D, full[:20, 20:], **TOL[metric])


@pytest.mark.parametrize("q_sizes,g_sizes", [([1], [1]), ([2, 3], [1, 2]), ([100], [100])], ids=["1x1", "5x3", "100x100"])
def test_small_and_single_group_shapes(ctx, q_sizes, g_sizes):
    _check(ctx, *_blobs(3, q_sizes, g_sizes), what="%s against %s" % (q_sizes, g_sizes))


def test_gallery_of_more_than_one_column_range(ctx):
    """M = 600 rows = 38 blocks (two column ranges); a 40-row identity lies across row 300, where the even cut would fall"""
    g_sizes = [16] * 17 + [8, 40] + [7] * 40
    assert sum(g_sizes) == 600 and sum(g_sizes[:18]) == 280
    q_sizes = [3, 20, 1, 40, 9, 16, 2]
    _check(ctx, *_blobs(4, q_sizes, g_sizes), what="M = 600")


def test_query_rows_that_are_copies_of_gallery_rows(ctx):
    """a person enrolled from the same video: distance exactly 0 inside the block mean (the branch that recomputes from differences)"""
    _, _, G, gs = _blobs(5, [1], [5, 17, 9, 33])
    rows = [np.arange(0, 3), np.arange(5, 22), np.r_[np.arange(22, 31), np.arange(31, 42)], np.arange(31, 64)]
    X = np.concatenate([G[r] for r in rows])
    rs = ref.starts([len(r) for r in rows])
    D = _check(ctx, X, rs, G, gs, metrics=(0,), what="copies")
    one = ctx.gallery_mean_dist(G[7:8], [0, 1], G[7:8], [0, 1])
    assert one.shape == (1, 1) and one[0, 0] == 0.0                                         # a row against itself: exactly zero
    assert D[1, 1] < D[1, 0] and D[3, 3] < D[3, 2]
    _check(ctx, X, rs, G, gs, metrics=(1,), what="copies")


def test_zero_rows_under_cosine(ctx):
    X, rs, G, gs = _blobs(6, [4, 17, 2], [3, 20, 1])
    X[[0, 5, 22]] = 0.0
    X[4:6] = 0.0
    G[[1, 3, 23]] = 0.0
    _check(ctx, X, rs, G, gs, what="zero rows")
    Z = ctx.gallery_mean_dist(np.zeros((3, 128)), [0, 3], G[:3], [0, 3], metric=1)
    assert Z[0, 0] == ref.mean_dist(np.zeros((3, 128)), [0, 3], G[:3], [0, 3], 1)[0, 0] == 0.0


# ---- decision ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.HAND_MADE, ids=[c[0] for c in ref.HAND_MADE])
def test_decision_on_hand_made_matrices(ctx, case):
    _, D, threshold, *want = case
    got = ctx.identify_dist(np.array(D, np.float64), threshold)
    assert ref.same_picks(got, ref.as_picks(*want)), got
    assert ref.same_picks(got, ref.pick(D, threshold))


@pytest.mark.parametrize("T,K", [(1, 1), (3, 17), (70, 64), (5, 65), (2, 1000)])
def test_decision_shapes(ctx, T, K):
    D = ref.random_matrix(T, K, 100 * T + K)
    for threshold in (0.6, 0.0, np.inf):
        got = ctx.identify_dist(D, threshold)
        assert ref.same_picks(got, ref.pick(D, threshold)), (T, K, threshold)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,threshold", [(0, 0.6), (1, 0.3)])
def test_identify_names_every_group_of_the_main_case(ctx, main_case, metric, threshold):
    X, rs, G, gs, Dr = main_case
    best, bd, second, sd, D = ctx.identify(X, rs, G, gs, threshold, metric=metric, return_dist=True)
    wb, wbd, ws, wsd = ref.pick(Dr[metric], threshold)
    assert np.array_equal(best, wb) and np.array_equal(second, ws)                           # every group, none excluded
    assert np.allclose(bd, wbd, **TOL[metric]) and np.allclose(sd, wsd, **TOL[metric])
    assert np.array_equal(best, ref.main_case_truth())
    assert (best >= 0).sum() == 15 and (best < 0).sum() == 5
    assert np.allclose(D, Dr[metric], **TOL[metric])
    assert ref.same_picks((best, bd, second, sd), ref.pick(D, threshold))                    # the decision is the one on the D it returns
    assert ref.same_picks(ctx.identify(X, rs, G, gs, threshold, metric=metric), (best, bd, second, sd))      # D = NULL


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_errors_and_the_context_goes_on(ctx, main_case):
    from pyannote_video_amd import _lib
    X, rs, G, gs, Dr = main_case
    empty = rs.copy()
    empty[3] = empty[2]
    with pytest.raises(_lib.PvfError, match="row_start holds an empty group"):
        ctx.gallery_mean_dist(X, empty, G, gs)
    with pytest.raises(_lib.PvfError, match="gal_start holds an empty group"):
        ctx.identify(X, rs, G, np.r_[gs[:5], gs[4:]], 0.6)
    with pytest.raises(_lib.PvfError, match="row_start must end at the number of rows"):
        ctx.gallery_mean_dist(X[:-1], rs, G, gs)
    with pytest.raises(_lib.PvfError, match="must start at 0"):
        ctx.gallery_mean_dist(X, np.r_[1, rs[1:]], G, gs)
    with pytest.raises(_lib.PvfError, match="non-decreasing"):
        ctx.gallery_mean_dist(X, np.r_[rs[:2], 0, rs[3:]], G, gs)
    with pytest.raises(_lib.PvfError, match="dim must be 128"):
        ctx.gallery_mean_dist(X[:, :64], rs, G[:, :64], gs)
    with pytest.raises(_lib.PvfError, match="T and K must be at least 1"):
        ctx.gallery_mean_dist(X, rs, G[:0], [0])
    with pytest.raises(_lib.PvfError, match="T and K must be at least 1"):
        ctx.identify_dist(np.zeros((3, 0)), 0.6)
    with pytest.raises(_lib.PvfError, match="threshold is NaN"):
        ctx.identify(X, rs, G, gs, float("nan"))
    with pytest.raises(_lib.PvfError, match="threshold is NaN"):
        ctx.identify_dist(Dr[0], float("nan"))
    with pytest.raises(_lib.PvfError, match="metric"):
        ctx.gallery_mean_dist(X, rs, G, gs, metric=2)
    assert np.allclose(ctx.gallery_mean_dist(X, rs, G, gs), Dr[0], **TOL[0])


# ---- the verbs -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip(tmp_path_factory, ctx, model_paths, small_video):
    """`process` on the small synthetic clip, then a gallery: `enroll` from the clip itself, `enroll-track` of its first track"""
    import json
    from pyannote_video_amd import cli
    d = tmp_path_factory.mktemp("identify")
    v = small_video
    p = {k: str(d / (k + ".txt")) for k in ("tracking", "landmarks", "embeddings", "labels", "gallery")}
    p["shots"] = str(d / "shots.json")
    with open(p["shots"], "w") as f:
        json.dump(v.shots(), f)
    cli.process(v, p["shots"], model_paths[0], model_paths[1], p["tracking"], p["landmarks"], p["embeddings"], p["labels"], ctx=ctx)
    p["enrolled"] = cli.enroll(v, model_paths[0], model_paths[1], "anna", p["gallery"], ctx=ctx)
    with pytest.raises(FileExistsError):
        cli.enroll(v, model_paths[0], model_paths[1], "anna", p["gallery"], ctx=ctx)
    first = int(open(p["embeddings"]).readline().split()[1])
    p["ben_rows"] = cli.enroll_track(p["embeddings"], first, "ben", p["gallery"], append=True)
    p["dir"] = d
    return p


def _expected(emb_path, gallery_path, labels=None, threshold=0.6):
    """identify_ref on the written files -> (groups in order, {track: group}, picks, names, D)"""
    from pyannote_video_amd import formats, render
    time, track, X = formats.read_embeddings(emb_path)
    names, gs, G = formats.read_gallery(gallery_path)
    group = {int(t): int(t) for t in track}
    if labels is not None:
        group.update({t: int(l) for t, l in render.read_labels(labels).items()})
    row_group = np.array([group[int(t)] for t in track])
    order = np.lexsort((time, track, row_group))
    groups, counts = np.unique(row_group, return_counts=True)
    D = ref.mean_dist(X[order], ref.starts(counts), G, gs, 0)
    return groups.tolist(), group, ref.pick(D, threshold), names, D


def _read(path):
    return [l.split() for l in open(path).read().splitlines()]


def test_enroll_then_identify(clip, ctx, small_video):
    from pyannote_video_amd import cli, formats
    assert clip["enrolled"]["faces"] >= 1 and clip["enrolled"]["faces"] + clip["enrolled"]["skipped"] == small_video.n_frames
    names, gs, G = formats.read_gallery(clip["gallery"])
    assert names == ["anna", "ben"] and gs.tolist() == [0, clip["enrolled"]["faces"], clip["enrolled"]["faces"] + clip["ben_rows"]]
    out, sc = str(clip["dir"] / "names.txt"), str(clip["dir"] / "scores.txt")
    got = cli.identify(clip["embeddings"], clip["gallery"], out, unknown="nobody", scores=sc, ctx=ctx)
    groups, _, (best, bd, second, sd), names, D = _expected(clip["embeddings"], clip["gallery"])
    assert len(groups) >= 2
    assert _read(out) == [[str(t), names[b] if b >= 0 else "nobody"] for t, b in zip(groups, best)]          # one line per track
    rows = _read(sc)
    assert [r[0] for r in rows] == [str(t) for t in groups]
    for r, d, s, s_d in zip(rows, D, second, sd):
        assert r[1] == names[int(np.argmin(d))] and r[3] == (names[s] if s >= 0 else "-")
        assert abs(float(r[2]) - d.min()) <= 1e-6 and abs(float(r[4]) - s_d) <= 1e-6
    assert list(got) == groups and all(got[t][0] == (names[b] if b >= 0 else None) for t, b in zip(groups, best))
    # without --unknown the unmatched tracks are left out
    cli.identify(clip["embeddings"], clip["gallery"], out, ctx=ctx)
    assert _read(out) == [[str(t), names[b]] for t, b in zip(groups, best) if b >= 0]
    # ben was enrolled from the first track's own rows: that track is at distance 0 + its own spread from him, below any other track's
    first = int(open(clip["embeddings"]).readline().split()[1])
    assert D[groups.index(first), 1] == D[:, 1].min()


def test_process_with_a_gallery_equals_identify_on_its_own_outputs(clip, ctx, model_paths, small_video):
    from pyannote_video_amd import cli, render
    d = clip["dir"]
    p = {k: str(d / ("g_" + k + ".txt")) for k in ("tracking", "landmarks", "embeddings", "labels", "clusters", "names")}
    res = cli.process(small_video, clip["shots"], model_paths[0], model_paths[1], p["tracking"], p["landmarks"], p["embeddings"], p["labels"],
                      ctx=ctx, gallery=clip["gallery"], unknown=None)
    for k in ("tracking", "landmarks", "embeddings"):
        assert open(p[k], "rb").read() == open(clip[k], "rb").read(), k                   # the gallery changes the labels file only
    cli.cluster(p["embeddings"], p["clusters"], ctx=ctx)
    assert open(p["clusters"]).read() == open(clip["labels"]).read()                      # what the same run writes without a gallery
    cli.identify(p["embeddings"], clip["gallery"], p["names"], labels=p["clusters"], ctx=ctx)
    assert open(p["labels"]).read() == open(p["names"]).read()                            # line for line
    groups, group, (best, _, _, _), names, _ = _expected(p["embeddings"], clip["gallery"], p["clusters"])
    want = [[str(t), names[best[groups.index(g)]] if best[groups.index(g)] >= 0 else str(g)] for t, g in sorted(group.items())]
    assert _read(p["labels"]) == want and len(res["identification"]) == len(groups)
    # the file is what `demo --label` reads
    labels = render.read_labels(p["labels"])
    assert sorted(labels) == sorted(group)
    frames = np.stack([small_video.frame(i) for i in range(small_video.n_frames)])
    npy = str(d / "clip.npy")
    np.save(npy, frames)
    r = cli.demo(cli.open_video(npy, small_video.frame_rate), p["tracking"], str(d / "demo.y4m"), height=120, label=p["labels"], ctx=ctx)
    assert r["frames"] == small_video.n_frames
