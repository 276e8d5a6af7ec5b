"""GPU: the order the rest of the suite does not run -- scratch buffers that start EMPTY, grow, and are carved again for a smaller call
and by another subsystem (csrc/scratch_layout.h sizes and carves them; `s_misc` alone is shared by the agglomeration, the landmarks, ORB
extraction, the shot detector and the decision of `identify`; tests/test_gpu_scratch_sharers.py runs every sharer of every buffer behind
every other).  The session context has usually grown every buffer to its largest case before a small one runs, so
this file opens a context of its own.  Every step is compared with the reference the entry's own tests use, with their equality: the
oracle (the agglomeration on the device's matrix bit for bit, the matrix itself to 1e-12 relative), tests/cooccur_ref.py, tests/orb_ref.py
(bit for bit).  The matrices the references start from are computed on the SESSION context, which leaves the buffers under test alone."""
import numpy as np
import pytest

import orb_check
import orb_ref
from tests import cooccur_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def own(model_paths):
    from pyannote_video_amd.runtime import Context
    c = Context(device=0, landmarks=model_paths[0])
    yield c
    c.close()


def _tracks(seed, sizes, dim):
    """rows of a few identities at norm ~0.45, rounded to 5 decimals, `sizes[t]` rows for track t"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes)
    cent = rng.normal(size=(max(2, len(sizes) // 8), dim))
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    x = cent[np.repeat(rng.integers(0, len(cent), len(sizes)), sizes)] + 0.04 * rng.normal(size=(int(sizes.sum()), dim))
    X = np.round(0.45 * x / np.linalg.norm(x, axis=1, keepdims=True), 5)
    return X, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _equals_oracle(got, ctx, oracle, X, rs, threshold=0.6):
    labels, log = got
    D = ctx.pair_mean_dist(X, rs)
    Dr = oracle.pair_mean_dist(X, rs)
    assert np.allclose(D, Dr, rtol=1e-12, atol=1e-13), np.abs(D - Dr).max()
    lr, logr = oracle.hac(D, np.diff(rs), threshold)
    assert np.array_equal(labels, lr)
    assert log.shape == logr.shape and np.array_equal(log, logr)          # bit for bit: kept, merged, distance, size
    lo, logo = oracle.hac(Dr, np.diff(rs), threshold)
    assert np.array_equal(labels, lo) and np.array_equal(log[:, :2], logo[:, :2])
    return len(log)


def test_clustering_128d_small_large_small(own, ctx, oracle):
    sizes = np.random.default_rng(1).integers(10, 25, 40)
    sizes[7] = 40                                       # spans three blocks of 16 rows: the per-chunk sums and the big_* arrays are in use
    assert 650 <= sizes.sum() <= 750
    small, large, again = _tracks(2, [1, 1], 128), _tracks(3, sizes, 128), _tracks(4, [1, 1], 128)
    merges = []
    for X, rs in (small, large, again):
        E = X.astype(np.float32)                        # round(float64(E), 5) on the device gives X back (|x| < 0.5)
        assert np.array_equal(np.round(E.astype(np.float64), 5), X)
        merges.append(_equals_oracle(own.cluster_tracks_f32(E, None, rs, 0.6), ctx, oracle, X, rs))
    assert 0 < merges[1] < 39


def test_clustering_generic_path_small_large_small(own, ctx, oracle):
    merges = []
    for seed, T in ((5, 3), (6, 50), (7, 3)):
        X, rs = _tracks(seed, np.random.default_rng(seed).integers(1, 6, T), 7)
        merges.append(_equals_oracle(own.cluster_tracks(X, rs, 0.3), ctx, oracle, X, rs, 0.3))
    assert 0 < merges[1] < 49


def _cooccur_step(own, ctx, T, seed):
    X, rs, ext = R.make(T, seed=seed)
    D = ctx.pair_mean_dist(X, rs)
    labels, log = R.hac(D, np.diff(rs), 0.6, R.cooccur(ext))
    got = own.cluster_tracks_cooccur(X, rs, 0.6, extent=ext)
    assert np.array_equal(got[0], labels)
    assert got[1].shape == log.shape and np.array_equal(got[1], log) and not np.isnan(got[1]).any()
    assert got[2] == R.n_blocked(ext)
    return len(log), got[2]


def _landmark_step(own, sp, frame, boxes):
    pts = own.landmarks([frame] * len(boxes), boxes)
    for k, b in enumerate(boxes):
        assert np.array_equal(pts[k], sp(frame, b)), (k, b)


def _shot_step(own, oracle, tables, frames):
    dfd, flow = own.shot_dfd(frames, 12, 12, tables, want_flow=True)
    small = [oracle.shot_convert(f, 12, 12) for f in frames]
    for i in range(1, len(frames)):
        assert np.array_equal(flow[i - 1], oracle.farneback(small[i - 1], small[i], tables)), i
        assert dfd[i - 1] == oracle.shot_dfd(small[i - 1], small[i], tables)


def _identify_step(own):
    """the fifth user of s_misc: the decision per group (identify_pick_k) carves its four result arrays there"""
    from tests import identify_ref
    from tests.scratch_cases import TOL
    X, rs, G, gs = identify_ref.main_case()
    best, bd, second, sd, D = own.identify(X, rs, G, gs, 0.6, return_dist=True)
    assert np.allclose(D, identify_ref.mean_dist(X, rs, G, gs), **TOL[0])
    assert identify_ref.same_picks((best, bd, second, sd), identify_ref.pick(D, 0.6))
    assert np.array_equal(best, identify_ref.main_case_truth())


def test_s_misc_recarved_by_its_four_users_in_turn(own, ctx, oracle, small_video, model_paths):
    from pyannote_video_amd import models, structure
    sp = oracle.ShapePredictor(models.load_container(model_paths[0]))
    frame = small_video.frame(0)
    boxes = [(40 + 55 * k, 30 + 25 * k, 130 + 55 * k, 120 + 25 * k) for k in range(8)] + [(-20, -10, 60, 70)]     # the last leaves the frame
    tables = structure.shot_tables()
    clip = [small_video.frame(i)[40:200, 60:300].copy() for i in range(6)]
    _cooccur_step(own, ctx, 3, seed=11)
    _landmark_step(own, sp, frame, boxes[:1])
    n, nb = _cooccur_step(own, ctx, 65, seed=12)        # one 64 x 64 stamp tile plus one row
    assert n > 0 and nb > 0
    _landmark_step(own, sp, frame, boxes)
    _identify_step(own)                                 # (a fifth user since the `identify` verb; behind the landmarks, in front of the flows)
    _shot_step(own, oracle, tables, clip[:2])
    _shot_step(own, oracle, tables, clip)
    X, rs, _ = R.make(3, seed=13)
    D = ctx.pair_mean_dist(X, rs)
    labels, log = own.cluster_dist(D, rs, 0.6)
    lr, logr = oracle.hac(D, np.diff(rs), 0.6)
    assert np.array_equal(labels, lr) and log.shape == logr.shape and np.array_equal(log, logr)


def test_orb_resident_set_and_explicit_descriptors(own):
    import thread_clip

    def textured(w, h, n, seed):
        return [thread_clip.make_clip(width=w, height=h, frames_per_shot=1, setups="A", seed=seed + k)[0][0] for k in range(n)]
    # the two smallest geometries of test_gpu_orb_edges.py: a small image without a level, then one with a single interior row
    counts, _, _, _ = orb_check.check_frames(own, textured(62, 200, 2, seed=3), height=200)
    assert orb_ref.thread_size(62, 200, 200) == (200, 62) and counts.tolist() == [0, 0]
    frames = textured(63, 200, 5, seed=3)
    assert orb_ref.thread_size(63, 200, 200) == (200, 63)
    counts, kp, desc, refs = orb_check.check_frames(own, frames, height=200)
    assert counts.max() >= 1
    pairs = [(a, b) for a in range(5) for b in range(5)]
    want = [orb_ref.match_count(refs[a][1], refs[b][1]) for a, b in pairs]
    np.testing.assert_array_equal(own.orb_match_counts(pairs), want)                  # the resident set: found through the shared layout
    np.testing.assert_array_equal(own.orb_match_counts(pairs, desc, counts), want)    # ... and the same sets brought by the call
    # (beyond the two smallest: 7 levels and hundreds of rows per set, so that the match counts are far from zero)
    counts, kp, desc, refs = orb_check.check_frames(own, textured(160, 120, 3, seed=3), height=200)
    pairs = [(a, b) for a in range(3) for b in range(3)]
    want = [orb_ref.match_count(refs[a][1], refs[b][1]) for a, b in pairs]
    assert counts.min() > 200 and min(want) > 0
    np.testing.assert_array_equal(own.orb_match_counts(pairs), want)
    np.testing.assert_array_equal(own.orb_match_counts(pairs, desc, counts), want)
