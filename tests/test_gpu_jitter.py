"""GPU: num_jitters (JITTER.md; csrc/jitter.hip: jitter_k; pvf_debug_jitter_chips, pvf_embed_jitter, pvf_landmarks_embed_jitter,
pvf_embed_chips_jitter) against tests/jitter_ref.py.  The jittered chips are the oracle's bit for bit; a descriptor is the fp32 mean of
what the embedder gives for those chips, the same in any batch and under any round size; 0 and 1 jitters are the plain entries."""
import json
import numpy as np
import pytest

from pyannote_video_amd import _lib
from tests import jitter_ref as ref

pytestmark = pytest.mark.gpu

J_MAX = 13          # the plan of (seed, j) does not depend on J (tests/test_jitter_ref.py): one reference serves J = 1, 8 and 13


@pytest.fixture(scope="module")
def chips3():
    """uniform noise, all 255 (any change in the order of the f64 blend shows: 255 blended with 255 is not always 255), a horizontal ramp"""
    rng = np.random.default_rng(20261019)
    noise = rng.integers(0, 256, (150, 150, 3), dtype=np.uint8)
    white = np.full((150, 150, 3), 255, np.uint8)
    ramp = np.zeros((150, 150, 3), np.uint8)
    ramp[:, :, 0] = (np.arange(150) * 255 // 149)[None, :]
    ramp[:, :, 1] = 255 - ramp[:, :, 0]
    ramp[:, :, 2] = (np.arange(150) * 7 % 256)[None, :]
    return np.stack([noise, white, ramp])


@pytest.fixture(scope="module")
def ref_chips(oracle, chips3):
    """[3][J_MAX] jittered chips by the oracle's extract_chip and the mirror, driven by the library's own plan rows (seed 0)"""
    rows = _lib.jitter_plan(J_MAX, 0)
    out = np.stack([np.stack([ref.jitter(oracle, c, ref.row_of_library(r)) for r in rows]) for c in chips3])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("J", [8, 1, 13])
def test_jittered_chips_bit_for_bit(ctx, chips3, ref_chips, J):
    got = ctx.jitter_chips(chips3, J)
    assert got.shape == (3, J, 150, 150, 3)
    want = ref_chips[:, :J]
    bad = [(i, j, int((got[i, j] != want[i, j]).sum())) for i in range(3) for j in range(J) if not np.array_equal(got[i, j], want[i, j])]
    assert not bad, bad
    if J == 8:
        assert np.array_equal(ctx.jitter_chips(chips3[2:], J), want[2:])          # n = 1
        assert (want[1] == 0).any() and ((want[1] != 0) & (want[1] != 255)).any()  # the all-255 chip: black corners, blended values


def test_another_seed_bit_for_bit(ctx, oracle, chips3):
    rows = _lib.jitter_plan(5, 12345678901234567890)
    got = ctx.jitter_chips(chips3[:1], 5, seed=12345678901234567890)
    for j, r in enumerate(rows):
        assert np.array_equal(got[0, j], ref.jitter(oracle, chips3[0], ref.row_of_library(r))), j


@pytest.mark.parametrize("split", [True, False])
def test_descriptor_is_the_mean_of_what_the_chips_give(ctx, chips3, split):
    ctx.embedder_split(split)
    try:
        got = ctx.embed_chips(chips3, num_jitters=8)
        each = ctx.embed_chips(ctx.jitter_chips(chips3, 8).reshape(-1, 150, 150, 3)).reshape(3, 8, 128)
    finally:
        ctx.embedder_split(True)
    assert np.array_equal(got, ref.mean32(each))
    assert not np.array_equal(got, each[:, 0])


@pytest.fixture(scope="module")
def faces(ctx, oracle, small_video, model_paths):
    """4 faces of the small clip: frames, detector boxes, the oracle's landmarks"""
    from pyannote_video_amd import models
    sp = oracle.ShapePredictor(models.load_container(model_paths[0]))
    frames, boxes, pts = [], [], []
    for i in (0, 5):
        f = small_video.frame(i)
        for b in ctx.detect(f, 1)[0]:
            frames.append(f); boxes.append(b); pts.append(sp(f, b))
    assert len(frames) >= 4
    return frames[:4], boxes[:4], np.array(pts[:4], np.int32)


def test_against_the_oracle(ctx, oracle, faces, model_paths):
    from pyannote_video_amd import models
    frames, boxes, pts = faces
    emb = oracle.Embedder(models.load_container(model_paths[1]))
    rows = [ref.row_of_library(r) for r in _lib.jitter_plan(4, 0)]
    want = ref.mean32(np.stack([np.stack([emb.forward(ref.jitter(oracle, emb.chip(f, p), r)) for r in rows]) for f, p in zip(frames, pts)]))
    got = ctx.embed(frames, pts, num_jitters=4)
    err = np.linalg.norm(got - want, axis=1)
    print("jitter descriptors against the oracle: L2 error per face", err, "max abs", np.abs(got - want).max())
    assert err.max() <= 1e-4, err
    # landmarks and descriptors in one call: the bits of the two calls
    p2, e2 = ctx.landmarks_embed(frames, boxes, num_jitters=4)
    p1 = ctx.landmarks(frames, boxes)
    assert np.array_equal(p1, p2) and np.array_equal(e2, ctx.embed(frames, p1, num_jitters=4))
    assert np.array_equal(p1, pts) and np.array_equal(e2, got)


def test_off_means_off(ctx, faces, chips3):
    frames, boxes, pts = faces
    plain = ctx.embed(frames, pts)
    plain_lm = ctx.landmarks_embed(frames, boxes)
    plain_chips = ctx.embed_chips(chips3)
    for J in (0, 1):
        assert np.array_equal(ctx.embed(frames, pts, num_jitters=J, seed=9), plain)
        p, e = ctx.landmarks_embed(frames, boxes, num_jitters=J, seed=9)
        assert np.array_equal(p, plain_lm[0]) and np.array_equal(e, plain_lm[1])
        assert np.array_equal(ctx.embed_chips(chips3, num_jitters=J, seed=9), plain_chips)
    # J = 1 through the library's own entry, not only through the Python default
    out = np.zeros((3, 128), np.float32)
    _lib.check(_lib.lib().pvf_embed_chips_jitter(ctx._h, _lib.ptr(chips3), 3, 1, 5, _lib.ptr(out)))
    assert np.array_equal(out, plain_chips)
    assert not np.array_equal(ctx.embed_chips(chips3, num_jitters=2), plain_chips)


def test_batch_independence_and_rounds(ctx, chips3, model_paths, monkeypatch):
    from pyannote_video_amd.runtime import Context
    five = np.concatenate([chips3, chips3[:2, ::-1]])               # 5 faces
    together = ctx.embed_chips(five, num_jitters=3, seed=4)
    for i in range(5):
        assert np.array_equal(ctx.embed_chips(five[i:i + 1], num_jitters=3, seed=4)[0], together[i]), i
    jit = ctx.jitter_chips(five, 3, seed=4)
    monkeypatch.setenv("PVF_JITTER_CHUNK", "8")                     # J = 3: rounds of 2 faces
    fresh = Context(device=0, detector=None, embedding=model_paths[1])
    try:
        assert np.array_equal(fresh.embed_chips(five, num_jitters=3, seed=4), together)
        assert np.array_equal(fresh.jitter_chips(five, 3, seed=4), jit)
    finally:
        fresh.close()


def test_refusals_are_errors_and_the_context_goes_on(ctx, faces, chips3):
    frames, boxes, pts = faces
    for J in (-1, 4097):
        with pytest.raises(_lib.PvfError, match="jitters"):
            ctx.embed_chips(chips3, num_jitters=J)
        with pytest.raises(_lib.PvfError, match="jitters"):
            ctx.embed(frames, pts, num_jitters=J)
        with pytest.raises(_lib.PvfError, match="jitters"):
            ctx.landmarks_embed(frames, boxes, num_jitters=J)
        with pytest.raises(_lib.PvfError, match="jitters"):
            ctx.jitter_chips(chips3, J)
    with pytest.raises(_lib.PvfError, match="bad arguments"):
        ctx.jitter_chips(chips3, 0)
    l = _lib.lib()
    out = np.zeros((3, 128), np.float32)
    for J in (0, 1, 2):
        assert l.pvf_embed_chips_jitter(ctx._h, None, 3, J, 0, _lib.ptr(out)) == -1 and b"pvf_embed_chips_jitter" in l.pvf_last_error()
        assert l.pvf_embed_chips_jitter(ctx._h, _lib.ptr(chips3), 3, J, 0, None) == -1
        assert l.pvf_embed_jitter(ctx._h, None, None, 2, J, 0, _lib.ptr(out)) == -1 and b"pvf_embed_jitter" in l.pvf_last_error()
        assert l.pvf_landmarks_embed_jitter(ctx._h, None, None, 2, J, 0, None, None) == -1 and b"pvf_landmarks_embed_jitter" in l.pvf_last_error()
    assert l.pvf_debug_jitter_chips(ctx._h, None, 3, 2, 0, None) == -1 and b"pvf_debug_jitter_chips" in l.pvf_last_error()
    assert l.pvf_embed_chips_jitter(ctx._h, _lib.ptr(chips3), -1, 2, 0, _lib.ptr(out)) == -1
    assert l.pvf_jitter_plan(3, 0, None) == -1
    assert ctx.embed_chips(chips3, num_jitters=2).shape == (3, 128)          # the context goes on


def _track(cli, ctx, v, d):
    p = {k: str(d / (k + ".txt")) for k in ("tracking", "landmarks", "embeddings", "landmarks0", "embeddings0", "gallery", "gallery0", "names")}
    shots = str(d / "shots.json")
    with open(shots, "w") as f:
        json.dump(v.shots(), f)
    cli.track(v, shots, p["tracking"], ctx=ctx)
    return p


def _distances(formats, p):
    """identify_ref on the written files -> (tracks in order, names, mean distance of every track to every identity, best identity)"""
    from tests import identify_ref
    time, track, X = formats.read_embeddings(p["embeddings"])
    names, gs, G = formats.read_gallery(p["gallery"])
    order = np.lexsort((time, track))
    groups, counts = np.unique(track, return_counts=True)
    D = identify_ref.mean_dist(X[order], identify_ref.starts(counts), G, gs, 0)
    return [int(t) for t in groups], names, D, identify_ref.pick(D, 0.6)[0]


def test_extract_verb_with_jitters(ctx, small_video, model_paths, tmp_path):
    from pyannote_video_amd import cli, formats, pipeline
    v = small_video
    p = _track(cli, ctx, v, tmp_path)
    cli.extract(v, model_paths[0], model_paths[1], p["tracking"], p["landmarks"], p["embeddings"], ctx=ctx, num_jitters=3)
    # the rows of the file: formats.embedding_rows of landmarks_embed(..., num_jitters=3) on the faces getFaceGenerator's pairing gives
    w, h = v.frame_size
    plan = pipeline.faces_per_frame(formats.read_tracks(p["tracking"]), [i / v.frame_rate for i in range(len(v))], w, h)
    fr, bx, T, ident = [], [], [], []
    for fi, t, g in plan:
        for k, box in g:
            fr.append(v.frame(fi)); bx.append(box); T.append(t); ident.append(k)
    assert len(bx) >= 6
    pts, emb = ctx.landmarks_embed(fr, bx, num_jitters=3)
    assert open(p["embeddings"], "rb").read() == formats.embedding_rows(T, ident, emb)
    assert open(p["landmarks"], "rb").read() == formats.landmark_rows(T, ident, pts, w, h)
    # the default writes what it wrote before the option existed: the plain descriptors
    cli.extract(v, model_paths[0], model_paths[1], p["tracking"], p["landmarks0"], p["embeddings0"], ctx=ctx)
    assert open(p["embeddings0"], "rb").read() == formats.embedding_rows(T, ident, ctx.landmarks_embed(fr, bx)[1])
    assert open(p["embeddings0"], "rb").read() != open(p["embeddings"], "rb").read()
    assert open(p["landmarks0"], "rb").read() == open(p["landmarks"], "rb").read()
    # `enroll --jitters 3` from the same clip, then `identify`: the decision is identify_ref's on the written files.  (The clip shows three
    # people and `enroll` takes the largest face of every frame: its gallery entry is a mix, and nobody needs to be within 0.6 of it.)
    res = cli.enroll(v, model_paths[0], model_paths[1], "anna", p["gallery"], ctx=ctx, num_jitters=3)
    assert res["faces"] >= 1
    cli.enroll(v, model_paths[0], model_paths[1], "anna", p["gallery0"], ctx=ctx)
    assert open(p["gallery0"], "rb").read() != open(p["gallery"], "rb").read()
    got = cli.identify(p["embeddings"], p["gallery"], p["names"], ctx=ctx)
    groups, names, D, best = _distances(formats, p)
    assert names == ["anna"] and [got[t][0] for t in groups] == [names[b] if b >= 0 else None for b in best]


def test_enroll_with_jitters_then_identify_names_the_enrolled_track(ctx, model_paths, tmp_path):
    """`enroll` takes the largest face of every frame, so a person is enrolled from a video that shows them alone: the small clip's
    generator with one face and one shot.  Enrolled with 3 jitters and extracted with 3 jitters, the clip's track is that person: the
    gallery rows are the track's own faces (the detector's box instead of the tracker's), so the mean distance is the track's spread over
    8 frames -- far below dlib's 0.6."""
    from pyannote_video_amd import cli, formats, synth
    v = synth.SyntheticVideo(width=640, height=360, n_frames=8, n_shots=1, faces=1, min_face=50, max_face=110, seed=7)
    p = _track(cli, ctx, v, tmp_path)
    cli.extract(v, model_paths[0], model_paths[1], p["tracking"], p["landmarks"], p["embeddings"], ctx=ctx, num_jitters=3)
    res = cli.enroll(v, model_paths[0], model_paths[1], "anna", p["gallery"], ctx=ctx, num_jitters=3)
    assert res == {"faces": 8, "skipped": 0}
    got = cli.identify(p["embeddings"], p["gallery"], p["names"], ctx=ctx)
    groups, names, D, best = _distances(formats, p)
    print("enroll --jitters 3: mean distance of the track to the enrolled faces", D[:, 0])
    assert len(groups) == 1 and names == ["anna"] and best.tolist() == [0]
    assert got[groups[0]][0] == "anna" and [l.split() for l in open(p["names"]).read().splitlines()] == [[str(groups[0]), "anna"]]
