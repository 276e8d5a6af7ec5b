"""GPU: the 68-point landmark kernel (csrc/ert.hip: ert_k; pvf_landmarks, pvf_debug_landmarks_shape, pvf_landmarks_embed) against the CPU
oracle on the edge-case table tests/ert_cases.py: twelve model geometries (tree counts on both sides of the leaf sum's groups of twenty
and of the 256 lanes, 1 .. 1024 feature pixels, depth 1 .. 6, integer thresholds so that diff == thresh occurs), boxes inside, across,
outside, of zero area, inverted, dwarfing the frame and at the int32 extremes, frames from 1 x 1 to 2 x 1000000.  The float32 shape of the
last cascade is compared BIT FOR BIT -- tests/test_ert_edge_cases.py shows that this sees a wrong summation order, which the integer
points alone do not -- and the integer points are compared as well.  Also here: batches against single calls, frames at unaligned device
addresses, the embedding paths on the same boxes, model reloads, refused model files (the context keeps the model it had) and refused
arguments.  An own Context: the models change under it.  Reference: pyannote/video/face/face.py:58,69-70."""
import numpy as np
import pytest
import torch

import ert_cases as ec
import ert_ref as er

pytestmark = pytest.mark.gpu

A, B = "c3_t40_p120_d4", "c3_t21_p257_d4"


@pytest.fixture(scope="module")
def table(small_video):
    return ec.frames(small_video), ec.faces(small_video)


@pytest.fixture(scope="module")
def c(model_paths):
    from pyannote_video_amd.runtime import Context
    ctx = Context(device=0, detector=None, embedding=model_paths[1])
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def dev(c, table):
    """the table's frames, uploaded once"""
    out = {name: c.upload(f) for name, f in table[0].items()}
    yield out
    for f in out.values():
        f.release()


@pytest.fixture(scope="module")
def model_file(tmp_path_factory):
    """name -> path of the model's container, written on first use"""
    from pyannote_video_amd import models
    d = tmp_path_factory.mktemp("ert_models")
    paths = {}

    def get(name):
        if name not in paths:
            paths[name] = str(d / (name + ".pvfm"))
            models.save_container(paths[name], ec.tensors(name))
        return paths[name]
    return get


@pytest.fixture(scope="module")
def want(table, oracle):
    """name -> (int32 [n, 68, 2], float32 [n, 68, 2]) of the oracle over all faces of the table, computed once per model"""
    frames, faces = table
    cache = {}

    def get(name):
        if name not in cache:
            sp = oracle.ShapePredictor(ec.tensors(name))
            res = [sp.shape_f32(frames[f], b) for f, _, b in faces]
            cache[name] = (np.stack([p for p, _ in res]), np.stack([s for _, s in res]))
        return cache[name]
    return get


def _differing(faces, got_p, got_s, want_p, want_s):
    bad = []
    for i, (f, cls, _) in enumerate(faces):
        if not np.array_equal(got_p[i], want_p[i]):
            bad.append((f, cls, "points", int((got_p[i] != want_p[i]).sum())))
        if got_s is not None and not er.same_bits(got_s[i], want_s[i]):
            bad.append((f, cls, "shape", float(np.abs(got_s[i].astype(np.float64) - want_s[i]).max())))
    return bad


@pytest.mark.parametrize("model", ec.MODELS, ids=repr)
def test_every_model_every_frame_every_box(c, dev, table, model_file, want, model):
    """one call of all 305 faces -- frames of eleven sizes, every box class -- per model"""
    _, faces = table
    c.load_shape_predictor(model_file(model.name))
    fr = [dev[f] for f, _, _ in faces]
    boxes = [b for _, _, b in faces]
    want_p, want_s = want(model.name)
    pts, shape = c.landmarks_shape(fr, boxes)
    bad = _differing(faces, pts, shape, want_p, want_s)
    assert not bad, (len(bad), bad[:10])
    assert np.array_equal(c.landmarks(fr, boxes), want_p)


def test_one_call_equals_one_face_per_call_and_unaligned_frames(c, dev, table, model_file, want):
    frames, faces = table
    c.load_shape_predictor(model_file(B))
    want_p, want_s = want(B)
    bad = []
    for i, (f, cls, b) in enumerate(faces):
        p, s = c.landmarks_shape([dev[f]], [b])
        bad += _differing([faces[i]], p, s, want_p[i:i + 1], want_s[i:i + 1])
    assert not bad, (len(bad), bad[:10])
    # every frame 1, 2 and 3 bytes into a larger byte buffer; face i reads the copy at offset 1 + i % 3
    held, keep = {}, []
    for name, f in frames.items():
        n = f.size
        for off in (1, 2, 3):
            buf = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
            view = buf[off:off + n].view(f.shape[0], f.shape[1], 3)
            view.copy_(torch.from_numpy(f))
            assert view.data_ptr() % 4 == off and view.is_contiguous()
            keep.append(buf)
            held[name, off] = c.wrap_torch(view)
    torch.cuda.synchronize()
    try:
        for shift in range(3):
            fr = [held[f, 1 + (i + shift) % 3] for i, (f, _, _) in enumerate(faces)]
            pts, shape = c.landmarks_shape(fr, [b for _, _, b in faces])
            bad = _differing(faces, pts, shape, want_p, want_s)
            assert not bad, (shift, len(bad), bad[:10])
    finally:
        for fr in held.values():
            fr.release()


def test_embedding_paths_on_the_edge_boxes(c, dev, table, model_file, want, oracle, model_paths):
    from pyannote_video_amd import models
    frames, faces = table
    c.load_shape_predictor(model_file(A))
    want_p, _ = want(A)
    sel = [i for i, (f, cls, _) in enumerate(faces) if f in ("video0", "noise") or cls in ec.ZERO_AREA]
    fr = [dev[faces[i][0]] for i in sel]
    boxes = [faces[i][2] for i in sel]
    pts, desc = c.landmarks_embed(fr, boxes)
    assert np.array_equal(pts, want_p[sel])
    pts2, desc2 = c.landmarks_embed(fr, boxes, num_jitters=2)
    assert np.array_equal(pts2, pts)
    assert np.array_equal(desc, c.embed(fr, pts))
    assert np.array_equal(desc2, c.embed(fr, pts, num_jitters=2))
    assert np.isfinite(desc).all() and np.isfinite(desc2).all()
    # zero-area boxes: 68 identical points, NaN chip details in the oracle, a black chip, the descriptor of a black chip
    zero = [k for k, i in enumerate(sel) if faces[i][1] in ec.ZERO_AREA]
    assert len(zero) >= 20
    chips = c.face_chips([fr[k] for k in zero], pts[zero])
    assert chips.shape == (len(zero), 150, 150, 3) and not chips.any()
    emb = oracle.Embedder(models.load_container(model_paths[1]))
    black = emb.forward(np.zeros((150, 150, 3), np.uint8)).astype(np.float64)
    err = np.linalg.norm(desc[zero].astype(np.float64) - black, axis=1)
    print("descriptors of zero-area faces against the oracle's forward of a black chip: L2", err.max())
    assert err.max() <= 1e-4


def _check_model(c, dev, table, want, name, every=9):
    _, faces = table
    some = faces[::every]
    want_p, want_s = want(name)
    pts, shape = c.landmarks_shape([dev[f] for f, _, _ in some], [b for _, _, b in some])
    bad = _differing(some, pts, shape, want_p[::every], want_s[::every])
    assert not bad, (name, len(bad), bad[:10])


def test_model_reload(c, dev, table, model_file, want):
    """A, B, A again: each load replaces sizes and arrays together"""
    assert not np.array_equal(want(A)[0], want(B)[0])
    for name in (A, B, A):
        c.load_shape_predictor(model_file(name))
        _check_model(c, dev, table, want, name)


def test_reloading_frees_the_replaced_model(c, dev, table, model_file, want):
    """a load frees the seven device arrays of the model it replaces: six rounds of an 18 MiB model and a small one would otherwise keep
    107 MiB (the full model is 65 MB a load); less than half of that may be missing afterwards"""
    big = "c2_t257_p120_d6"
    assert 17 < ec.model_by_name(big).leaf_mib() < 19
    c.load_shape_predictor(model_file(big))
    c.load_shape_predictor(model_file(A))
    # free memory is the whole device's, and other processes may use it: a leak shows in EVERY attempt, a neighbour's allocation in one
    lost = []
    for attempt in range(3):
        free0 = c.mem_info()[0]
        for _ in range(6):
            c.load_shape_predictor(model_file(big))
            c.load_shape_predictor(model_file(A))
        lost.append(free0 - c.mem_info()[0])
        if lost[-1] < (48 << 20):
            break
    print("device memory missing after six reloads: %s MiB" % ["%.1f" % (v / 2.0 ** 20) for v in lost])
    assert min(lost) < (48 << 20)
    _check_model(c, dev, table, want, A)


def _broken(tmp_path, name, how):
    from pyannote_video_amd import models
    t = {k: v.copy() for k, v in ec.tensors(name).items()}
    if how == "more_trees_than_tensors":
        t["sp.meta"][1] += 1
    elif how == "split_index":
        t["sp.split_idx2"].reshape(-1)[-1] = t["sp.meta"][3]            # n_pix: one past the last pixel
    elif how == "negative_split_index":
        t["sp.split_idx1"].reshape(-1)[0] = -1
    elif how == "anchor":
        t["sp.anchor_idx"].reshape(-1)[-1] = 68
    p = str(tmp_path / (how + ".pvfm"))
    models.save_container(p, t)
    return p


@pytest.mark.parametrize("how,message", [("more_trees_than_tensors", "tensor sizes do not match sp.meta"),
                                         ("split_index", "split feature index out of range"),
                                         ("negative_split_index", "split feature index out of range"),
                                         ("anchor", "anchor index out of range")])
def test_a_refused_model_file_leaves_the_loaded_model_in_place(c, dev, table, model_file, want, tmp_path, how, message):
    """load_shape reads and checks a file into a model of its own and swaps only after the upload: after a refusal the context holds A's
    sizes AND A's arrays.  (Before, the sizes were the refused file's: this test is only valid with that fix in the library.)
    The refused files are made from B, whose sizes differ from A's."""
    from pyannote_video_amd import _lib
    c.load_shape_predictor(model_file(A))
    _check_model(c, dev, table, want, A)
    with pytest.raises(_lib.PvfError, match=message):
        c.load_shape_predictor(_broken(tmp_path, B, how))
    _check_model(c, dev, table, want, A)
    c.load_shape_predictor(model_file(B))                               # and a good file still loads afterwards
    _check_model(c, dev, table, want, B)


def test_refused_arguments(c, dev, table, model_file, want):
    from pyannote_video_amd import _lib
    c.load_shape_predictor(model_file(A))
    l = _lib.lib()
    err = lambda: l.pvf_last_error()
    fr = _lib.handles([dev["video0"].handle] * 2)
    boxes = np.array([[10, 10, 60, 60], [20, 20, 90, 90]], np.int32)
    pts = np.zeros((2, 68, 2), np.int32)
    shape = np.zeros((2, 68, 2), np.float32)
    out = np.zeros((2, 128), np.float32)
    P = _lib.ptr
    for args in ((None, P(boxes), 2, P(pts)), (P(fr), None, 2, P(pts)), (P(fr), P(boxes), 2, None), (P(fr), P(boxes), -1, P(pts))):
        assert l.pvf_landmarks(c._h, *args) == -1 and b"pvf_landmarks:" in err(), args
    for args in ((None, P(boxes), 2, P(pts), P(shape)), (P(fr), P(boxes), 2, P(pts), None), (P(fr), P(boxes), -1, P(pts), P(shape))):
        assert l.pvf_debug_landmarks_shape(c._h, *args) == -1 and b"pvf_debug_landmarks_shape:" in err(), args
    for args in ((None, P(boxes), 2, P(pts), P(out)), (P(fr), P(boxes), 2, P(pts), None), (P(fr), P(boxes), -1, P(pts), P(out)),
                 (None, None, -1, None, None)):
        assert l.pvf_landmarks_embed(c._h, *args) == -1 and b"pvf_landmarks_embed:" in err(), args
    assert l.pvf_landmarks(c._h, None, None, 0, None) == 0
    assert l.pvf_debug_landmarks_shape(c._h, None, None, 0, None, None) == 0
    assert l.pvf_landmarks_embed(c._h, None, None, 0, None, None) == 0
    assert not pts.any() and not shape.any() and not out.any()
    _check_model(c, dev, table, want, A)                                # the context goes on


def test_full_geometry_edge_boxes(ctx_full, oracle, full_model_paths, table):
    """15 cascades x 500 trees x 500 pixels, what bench.py runs: eight boxes of the edge classes, float shape bit for bit"""
    from pyannote_video_amd import models
    frames, faces = table
    classes = ("inside", "cross_left", "corner_br", "outside_top", "zero_area", "inverted_both", "dwarfing", "i32_whole")
    some = [(f, cls, b) for f, cls, b in faces if f == "video0" and cls in classes]
    assert len(some) == 8
    sp = oracle.ShapePredictor(models.load_container(full_model_paths[0]))
    res = [sp.shape_f32(frames[f], b) for f, _, b in some]
    fr = ctx_full.upload(frames["video0"])
    try:
        pts, shape = ctx_full.landmarks_shape([fr] * 8, [b for _, _, b in some])
        bad = _differing(some, pts, shape, np.stack([p for p, _ in res]), np.stack([s for _, s in res]))
        assert not bad, bad
        assert np.array_equal(ctx_full.landmarks([fr] * 8, [b for _, _, b in some]), pts)
    finally:
        fr.release()
