"""GPU: image chips (csrc/chip.hip: chip_plan / pyr_down2_k / transform_k / chip_extract_batch) against the oracle's chip
(oracle/pvo_image.c) on the geometry table of tests/chip_cases.py -- row pitches of every remainder modulo 4, frames smaller than a chip,
pyramid levels on the seams of the 32 x 8 tiles, chips on the seam of the 64-column blocks, sample grids exactly on integers, exact quarter
turns, empty, collapsed and non-finite jobs, batches that mix all of them and frames of different sizes, and frames that reach the
kernels by every route (upload, a wrapped tensor, views 1, 2 and 3 bytes into a buffer of 0xAA, the ingest ring).
tests/test_chip_cases.py proves on the plan and the oracle alone that the table contains those conditions.  Chips are compared bit for bit;
descriptors within the suite's 1e-4 of the oracle's network on the oracle's chip (tests/test_gpu_chip_edges.py).
Reference: pyannote/video/face/face.py:73-76; pyannote/video/tracking.py:203,251."""
import numpy as np
import pytest
import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships

import chip_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(model_paths):
    from pyannote_video_amd import models
    return models.load_container(model_paths[1])


@pytest.fixture(scope="module")
def emb(oracle, model):
    return oracle.Embedder(model)


_ref = {}     # the oracle's chips of this module's runs: several tests meet the same (frame, request)


def _ref_chip(oracle, g, content, r):
    key = (g.name, content, r.name)
    if key not in _ref:
        _ref[key] = oracle.extract_chip(cc.frame(g, content), r.rect, r.cs, r.sn, r.rows, r.cols)
    return _ref[key]


def _ref_face(emb, g, content, name, pts):
    key = (g.name, content, "face", name)
    if key not in _ref:
        _ref[key] = emb.chip(cc.frame(g, content), pts)
    return _ref[key]


_desc = {}


def _ref_descriptor(emb, chip):
    key = chip.tobytes()
    if key not in _desc:
        _desc[key] = emb.forward(chip)
    return _desc[key]


def _differs(tag, got, want):
    if np.array_equal(got, want):
        return []
    at = tuple(int(v) for v in np.argwhere(got != want)[0])
    return [(tag, "first differing (row, column, channel)", at, "gpu", int(got[at]), "oracle", int(want[at]), "%d bytes differ" % int((got != want).sum()))]


def _requests(ctx, oracle, g, content, fr, how=""):
    bad = []
    for r in cc.requests(g):
        got = ctx.extract_chip(fr, r.rect, r.cs, r.sn, r.rows, r.cols)
        bad += _differs("%s_%s_%s%s" % (g.name, content, r.name, how), got, _ref_chip(oracle, g, content, r))
    return bad


def _faces(ctx, emb, model, g, content, fr, how="", one_by_one=False):
    names, pts = cc.face_points(model["emb.mean_shape"], g)
    ref = [_ref_face(emb, g, content, n, p) for n, p in zip(names, pts)]
    chips = ctx.face_chips([fr] * len(pts), pts)                     # one batch per geometry
    bad = []
    for n, a, b in zip(names, chips, ref):
        bad += _differs("%s_%s_face_%s%s" % (g.name, content, n, how), a, b)
    if one_by_one:
        for n, p, b in zip(names, pts, ref):
            bad += _differs("%s_%s_face_%s_alone" % (g.name, content, n), ctx.face_chips([fr], p[None])[0], b)
    return bad


# ---- every request and every landmark set of every geometry ------------------------------------------------------------------------------
@pytest.mark.parametrize("g", cc.GEOMETRY, ids=lambda g: g.name)
def test_every_request_equals_the_oracle(ctx, oracle, g):
    bad = []
    for content in ("blobs", "tail", "noise", "black"):
        fr = ctx.upload(cc.frame(g, content))
        try:
            bad += _requests(ctx, oracle, g, content, fr)
        finally:
            fr.release()
    assert not bad, bad[:10]


@pytest.mark.parametrize("g", cc.GEOMETRY, ids=lambda g: g.name)
def test_face_chips_and_descriptors_equal_the_oracle(ctx, emb, model, g):
    bad = []
    for content in ("blobs", "tail"):
        fr = ctx.upload(cc.frame(g, content))
        try:
            bad += _faces(ctx, emb, model, g, content, fr, one_by_one=True)
            if content == "blobs":
                names, pts = cc.face_points(model["emb.mean_shape"], g)
                out = ctx.embed([fr] * len(pts), pts)
                want = np.stack([_ref_descriptor(emb, _ref_face(emb, g, content, n, p)) for n, p in zip(names, pts)])
                err = np.linalg.norm(out - want, axis=1)
                print(g.name, "descriptor error", dict(zip(names, err.tolist())))
                assert err.max() <= 1e-4, dict(zip(names, err.tolist()))
        finally:
            fr.release()
    assert not bad, bad[:10]


# ---- batch composition: the batch-maximum grids of chip_extract_batch and its null descriptors ------------------------------------------
@pytest.mark.parametrize("name", ["854x480", "97x81"])
def test_one_batch_of_every_kind_of_job_equals_one_call_per_chip(ctx, emb, model, name):
    """chips of 0, 1, 2 and 3 levels beside an empty, a collapsed and a non-finite job in ONE call, in the listed order and in reverse"""
    g = cc.by_name(name)
    names, pts = cc.face_points(model["emb.mean_shape"], g)
    pick = [names.index(n) for n in cc.COMPOSITION]
    fr = ctx.upload(cc.frame(g, "blobs"))
    bad = []
    try:
        alone = {i: ctx.face_chips([fr], pts[i][None])[0] for i in pick}
        for i in pick:
            bad += _differs("%s_face_%s_alone" % (name, names[i]), alone[i], _ref_face(emb, g, "blobs", names[i], pts[i]))
        assert not alone[names.index("empty")].any() and not alone[names.index("collapsed")].any() and not alone[names.index("not_finite")].any()
        assert all(alone[names.index("levels_%d" % k)].any() for k in range(3))
        for order in (pick, pick[::-1], pick[3:] + pick[:3]):
            chips = ctx.face_chips([fr] * len(order), pts[order])
            for i, c in zip(order, chips):
                bad += _differs("%s_face_%s_in_%s" % (name, names[i], [names[k] for k in order][:2]), c, alone[i])
    finally:
        fr.release()
    assert not bad, bad[:10]


def test_one_batch_over_frames_of_different_sizes_equals_one_call_per_chip(ctx, emb, model):
    """a 7 x 5 and a 2 x 2 frame beside 854 x 480 in one call: every level's grid is sized by the largest job, the others leave early"""
    frames, pts, tags, ref = [], [], [], []
    held = {}
    try:
        for name in cc.MIXED_SIZES:
            g = cc.by_name(name)
            held[name] = ctx.upload(cc.frame(g, "blobs"))
            names, p = cc.face_points(model["emb.mean_shape"], g)
            for n in ("inside", "larger_than_frame", "levels_2", "collapsed"):
                if n in names:
                    frames.append(held[name])
                    pts.append(p[names.index(n)])
                    tags.append("%s_%s" % (name, n))
                    ref.append(_ref_face(emb, g, "blobs", n, p[names.index(n)]))
        assert len({(f.height, f.width) for f in frames}) == len(cc.MIXED_SIZES)
        bad = []
        for i, tag in enumerate(tags):
            bad += _differs("mixed_alone_" + tag, ctx.face_chips([frames[i]], pts[i][None])[0], ref[i])
        for order in (list(range(len(tags))), list(range(len(tags)))[::-1]):
            chips = ctx.face_chips([frames[i] for i in order], np.stack([pts[i] for i in order]))
            for i, c in zip(order, chips):
                bad += _differs("mixed_" + tags[i], c, ref[i])
        assert not bad, bad[:10]
    finally:
        for f in held.values():
            f.release()


# ---- frames by every route ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.ROUTES)
def test_chips_of_frames_by_every_route(ctx, oracle, emb, model, name):
    """a byte read from beside the frame changes a value: the views lie in a buffer of 0xAA"""
    g = cc.by_name(name)
    h, w, n = g.h, g.w, g.h * g.w * 3
    bad = []
    for content in ("tail", "blobs"):
        f = cc.frame(g, content)

        def check(fr, how):
            return _requests(ctx, oracle, g, content, fr, "_" + how) + _faces(ctx, emb, model, g, content, fr, "_" + how)

        fr = ctx.upload(f)
        bad += check(fr, "upload")
        fr.release()
        t = torch.from_numpy(f.copy()).cuda()                        # an allocation of exactly the frame
        fr = ctx.wrap_torch(t)
        bad += check(fr, "wrap")
        fr.release()
        for off in (1, 2, 3):                                        # 1, 2 and 3 bytes into a larger byte buffer
            buf = torch.full((n + 8,), 0xAA, dtype=torch.uint8, device="cuda")
            view = buf[off:off + n].view(h, w, 3)
            view.copy_(torch.from_numpy(f.copy()))
            torch.cuda.synchronize()
            assert view.data_ptr() % 4 == off and view.is_contiguous()
            fr = ctx.wrap_torch(view)
            bad += check(fr, "offset%d" % off)
            fr.release()
            assert bool((buf[:off] == 0xAA).all()) and bool((buf[off + n:] == 0xAA).all())
        ring = ctx.ingest_ring(h, w, depth=4)
        try:
            fr = ring.push(f)
            ring.wait()
            bad += check(fr, "ring")
            fr.release()
        finally:
            ring.close()
    assert not bad, bad[:10]
