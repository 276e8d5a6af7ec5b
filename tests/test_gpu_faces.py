"""GPU: the `faces` verb's kernels (csrc/faces.hip) bit for bit against FACES.md as tests/faces_ref.py restates it: the five quality
sums of chips at every alignment of their start address and across a round of 4096, the sums of faces whose chips are made on the
device (on a context without an embedder, and after detector and tracker work), sheets of tiles at every tile size with tiles inside,
across every edge, off the sheet, overlapping and duplicated, primitives over tiles, every refusal of the C ABI, and the verb end to end
in a process of its own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import demo_ref, faces_ref as fr
from tests.test_gpu_chip_edges import landmarks, small_sets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = fr.named_chips()
_CACHE = {}


def pool():
    """(chips uint8 [P, 150, 150, 3], sums int64 [P, 5]): the named contents and a few more noise chips, their reference made once"""
    if "pool" not in _CACHE:
        rng = np.random.default_rng(77)
        extra = [rng.integers(0, 256, (150, 150, 3)).astype(np.uint8) for _ in range(3)]
        extra.append((rng.integers(0, 256, (150, 150, 3)) // 16).astype(np.uint8))            # dark noise
        extra.append((255 - rng.integers(0, 256, (150, 150, 3)) // 16).astype(np.uint8))      # bright noise
        chips = np.stack(list(NAMED.values()) + extra)
        _CACHE["pool"] = (chips, fr.qualities(chips))
    return _CACHE["pool"]


def batch(n):
    """n chips drawn from the pool so that every pool chip meets every alignment of the start address (67500 i mod 16 = 12 i mod 16)"""
    chips, sums = pool()
    assert len(chips) % 5 and len(chips) % 2                       # the stride below and the four alignments reach every pool chip
    idx = (np.arange(n) * 5 + 3) % len(chips)
    return idx, chips[idx], sums[idx]


@pytest.fixture(scope="module")
def dlib_ctx(model_paths, tmp_path_factory):
    """a context whose embedder carries dlib's mean face shape, as a dlib file does: its face_chips are the chips the faces calls make"""
    from pyannote_video_amd import models
    from pyannote_video_amd.runtime import Context
    m = models.load_container(model_paths[1])
    m["emb.mean_shape"] = np.stack([np.asarray(models.DLIB_MEAN_FACE_X), np.asarray(models.DLIB_MEAN_FACE_Y)], 1).astype(np.float32)
    path = str(tmp_path_factory.mktemp("dlib_shape") / "embedder.pvfm")
    models.save_container(path, m)
    c = Context(device=0, embedding=path)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bare_ctx():
    from pyannote_video_amd.runtime import Context
    c = Context(device=0)                   # a detector, no landmark model, no embedder
    yield c
    c.close()


# ---- chip_quality ------------------------------------------------------------------------------------------------------------------
def test_named_contents_give_their_known_sums(bare_ctx):
    got = bare_ctx.chip_quality(np.stack(list(NAMED.values())))
    want = fr.qualities(NAMED.values())
    bad = [(k, g.tolist(), w.tolist()) for k, g, w in zip(NAMED, got, want) if not np.array_equal(g, w)]
    assert not bad, bad
    by = dict(zip(NAMED, got.tolist()))
    assert by["checker"][:2] == [0, 22788921600] and by["dot"][0] == -255 and by["frame"][0] == -150960
    assert fr.sharpness(by["ramp"]) == 275530416 and fr.sharpness(by["dot"]) == 65025 * (fr.N - 1)
    assert [by["y%d" % y][3:] for y in (16, 17, 238, 239)] == [[22500, 0], [0, 0], [0, 0], [0, 22500]]
    assert by["equal_luma_edge"][:2] == [0, 0]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 257, 4097])
def test_chip_quality_counts_and_positions(bare_ctx, n):
    idx, chips, want = batch(n)
    got = bare_ctx.chip_quality(chips)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(int(i), int(idx[i]), got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    if n >= 257:                                                    # one chip, every position it takes: one result
        for p in range(len(pool()[0])):
            rows = got[idx == p]
            assert len(rows) >= 4 and (rows == rows[0]).all(), p
    if n == 4097:                                                   # both sides of the round of 4096, and every start alignment
        assert np.array_equal(got[4094:4097], want[4094:4097]) and {(12 * i) % 16 for i in range(4093, 4097)} == {0, 4, 8, 12}
    # one chip per call gives what the batch gives
    if n == 5:
        for i in range(n):
            assert np.array_equal(bare_ctx.chip_quality(chips[i:i + 1])[0], want[i])
    assert bare_ctx.chip_quality(np.zeros((0, 150, 150, 3), np.uint8)).shape == (0, 5)


# ---- face_quality ------------------------------------------------------------------------------------------------------------------
def _geometries(model_paths, small_video):
    from pyannote_video_amd import models
    mean = np.stack([np.asarray(models.DLIB_MEAN_FACE_X), np.asarray(models.DLIB_MEAN_FACE_Y)], 1)
    sets = small_sets(mean, 640, 360) + [("touch_right", (640 - 56, 180, 80, 0)), ("touch_bottom", (320, 360 - 62, 80, 0)), ("turned", (300, 170, 120, 25))]
    return [n for n, _ in sets], [landmarks(mean, *a) for _, a in sets]


def test_face_quality_equals_chip_quality_of_the_chips(ctx, bare_ctx, dlib_ctx, model_paths, small_video):
    names, pts = _geometries(model_paths, small_video)
    f = small_video.frame(2)
    chips = dlib_ctx.face_chips([f] * len(pts), pts)
    want = fr.qualities(chips)
    by = dict(zip(names, chips))
    assert not by["off_frame"].any() and by["inside"].any() and by["off_left"].any() and (by["off_left"].reshape(-1, 3).max(axis=1) == 0).mean() > 0.1
    assert len({tuple(w) for w in want.tolist()}) >= len(names) - 2            # the geometries give different chips (the two off-frame ones are black)
    assert np.array_equal(dlib_ctx.chip_quality(chips), want)
    for c in (bare_ctx, dlib_ctx):                                  # without an embedder; with one
        got = c.face_quality([f] * len(pts), pts)
        bad = [(n, g.tolist(), w.tolist()) for n, g, w in zip(names, got, want) if not np.array_equal(g, w)]
        assert not bad, bad
        for i in (0, 1, 7):                                         # one face per call == the batch
            assert np.array_equal(c.face_quality([f], pts[i:i + 1])[0], want[i])
    # after detector and tracker work on the context, and whatever embedder it holds (the suite's synthetic one has another mean shape)
    frames = [small_video.frame(i) for i in range(3)]
    dets = ctx.detect_batch(frames)
    boxes = [b for b in dets[0][0]][:2]
    assert boxes
    trk = ctx.tracker_create_many(len(boxes))
    ctx.tracker_start_many(trk, [frames[0]] * len(boxes), [tuple(float(v) for v in b) for b in boxes])
    ctx.tracker_update_many(trk, [frames[1]] * len(boxes))
    ctx.tracker_destroy_many(trk)
    ctx.embed([f] * 2, pts[:2])
    got = ctx.face_quality([f] * len(pts), pts)
    assert np.array_equal(got, want)
    assert bare_ctx.face_quality([], np.zeros((0, 68, 2), np.int32)).shape == (0, 5)


# ---- sheets --------------------------------------------------------------------------------------------------------------------------
def _prims(W, H):
    return [(demo_ref.RECT, 3, 2, W - 5, H - 4, (250, 10, 20)), (demo_ref.LINE, -5, -3, W + 4, H + 2, (0, 255, 0)),
            (demo_ref.TEXT, 4, H - 3, (255, 255, 0), 2, b"#12 ann"), (demo_ref.TEXT, W - 20, 9, (1, 2, 3), 1, b"edge~"),
            (demo_ref.RECT, -40, -40, 8, 8, (9, 8, 7))]


def _same(got, want):
    assert got.shape == want.shape
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), [got[y, x].tolist() for y, x in bad[:5]], [want[y, x].tolist() for y, x in bad[:5]])


@pytest.mark.parametrize("S", [48, 149, 150, 151, 600])
def test_chip_sheet_tile_sizes_edges_overlap(bare_ctx, S):
    chips = pool()[0]
    use = [chips[list(NAMED).index(k)] for k in ("noise", "ramp", "checker", "frame", "stripes_v", "dot")] + [chips[-3], chips[-2], chips[-1]]
    W, H = 2 * S + 37, S + S // 2 + 11
    big = 2 ** 31 - 1
    xy = [(5, 7),                                   # inside
          (-S // 3, 20), (W - S // 2, 3), (S // 2, -S // 4), (S + 9, H - S // 3),      # across the left, right, top and bottom edges
          (-S, 0), (W, 5), (0, H), (3, -S), (big, big), (-big - 1, -big - 1), (-big - 1, big),      # wholly off the sheet, the last beside int32's ends
          (S // 2 + 1, S // 3), (S // 2 + 9, S // 3 + 4),     # overlapping the first and each other: the later one shows
          (5, 7)]                                   # the first corner again, with another chip: it replaces the first where they both lie
    batch_chips = np.stack([use[i % len(use)] for i in range(len(xy))])
    want = fr.sheet(batch_chips, xy, S, W, H, (10, 20, 30))
    got = bare_ctx.chip_sheet(batch_chips, xy, S, W, H, (10, 20, 30))
    _same(got, want)
    assert not np.array_equal(want, fr.sheet(batch_chips, xy, S, W, H, (10, 20, 30), first_wins=True))       # the case tells the two orders apart
    if S == 150:
        assert np.array_equal(got[100:157, 5:40], batch_chips[14][93:150, 0:35])        # a tile is the chip byte for byte
    prims = _prims(W, H)
    _same(bare_ctx.chip_sheet(batch_chips, xy, S, W, H, (10, 20, 30), prims), fr.sheet(batch_chips, xy, S, W, H, (10, 20, 30), prims))
    # the same chip twice: two tiles
    two = bare_ctx.chip_sheet(np.stack([use[0], use[0]]), [(0, 0), (S + 3, 2)], S, W, H)
    _same(two, fr.sheet([use[0], use[0]], [(0, 0), (S + 3, 2)], S, W, H))


@pytest.mark.parametrize("W,H", [(1, 1), (49, 7), (16384, 4)])
def test_chip_sheet_sheet_sizes(bare_ctx, W, H):
    chips = pool()[0][[5, 2, 3]]
    xy = [(-20, -30), (W - 30, -10), (W // 2, 1)]
    prims = [(demo_ref.LINE, 0, 0, W - 1, H - 1, (200, 100, 50)), (demo_ref.TEXT, W // 3, H - 1, (5, 6, 7), 1, b"x")]
    _same(bare_ctx.chip_sheet(chips, xy, 48, W, H, (3, 2, 1), prims), fr.sheet(chips, xy, 48, W, H, (3, 2, 1), prims))
    # n = 0: background and primitives
    none = np.zeros((0, 150, 150, 3), np.uint8)
    _same(bare_ctx.chip_sheet(none, [], 48, W, H, (3, 2, 1), prims), fr.sheet([], [], 48, W, H, (3, 2, 1), prims))
    _same(bare_ctx.chip_sheet(none, [], 600, W, H, (255, 0, 128)), fr.sheet([], [], 600, W, H, (255, 0, 128)))


def test_chip_sheet_across_rounds_the_last_tile_of_the_list_wins(bare_ctx):
    """4100 tiles go through in two rounds of chips: which tile shows is decided by the list, not by the round"""
    n = 4100
    idx, chips, _ = batch(n)
    xy = np.full((n, 2), -1000, np.int32)                           # most of them off the sheet
    on = {3: (0, 0), 4095: (20, 10), 4096: (30, 15), 4099: (10, 30), 7: (100, 5), 4098: (110, 20), 4097: (160, 40), 9: (170, 45)}
    for i, c in on.items():
        xy[i] = c
    got = bare_ctx.chip_sheet(chips, xy, 64, 240, 110, (40, 40, 40))
    _same(got, fr.sheet(chips, xy, 64, 240, 110, (40, 40, 40)))
    assert np.array_equal(got[50, 175], fr.tile(chips[4097], 64)[10, 15])       # 4097 (second round) over 9 (first round), though 9 is placed later on the sheet


def test_face_sheet_equals_chip_sheet_of_the_chips(bare_ctx, dlib_ctx, model_paths, small_video):
    names, pts = _geometries(model_paths, small_video)
    f = small_video.frame(2)
    chips = dlib_ctx.face_chips([f] * len(pts), pts)
    xy = [(7 + 60 * (i % 6), 5 + 70 * (i // 6)) for i in range(len(pts))]
    prims = _prims(400, 230)
    want = fr.sheet(chips, xy, 96, 400, 230, fr.BACKGROUND, prims)
    _same(bare_ctx.face_sheet([f] * len(pts), pts, xy, 96, 400, 230, fr.BACKGROUND, prims), want)
    _same(dlib_ctx.face_sheet([f] * len(pts), pts, xy, 96, 400, 230, fr.BACKGROUND, prims), want)
    _same(bare_ctx.face_sheet([], np.zeros((0, 68, 2), np.int32), [], 96, 40, 23, fr.BACKGROUND, _prims(40, 23)), fr.sheet([], [], 96, 40, 23, fr.BACKGROUND, _prims(40, 23)))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(bare_ctx, small_video):
    from pyannote_video_amd import _lib
    c, l, P = bare_ctx, bare_ctx._l, _lib.ptr
    err = lambda: l.pvf_last_error().decode()
    chips = np.ascontiguousarray(pool()[0][:2])
    q = np.zeros((2, 5), np.int64)
    xy = np.array([[0, 0], [10, 10]], np.int32)
    rgb = np.zeros((64, 64, 3), np.uint8)
    empty = np.zeros(0, np.uint8)
    f = c.upload(small_video.frame(0))
    hs = np.array([f.handle, f.handle], np.uint64)
    pts = np.zeros((2, 68, 2), np.int32)
    pts[:, :, 0] = np.arange(68) * 3 + 100
    pts[:, :, 1] = (np.arange(68) * 7) % 90 + 100
    bad_handles = np.array([f.handle, 987654321], np.uint64)
    for call, message in ((lambda: l.pvf_chip_quality(c._h, P(chips), -1, P(q)), "PVF_SHEET_MAX_TILES"),
                          (lambda: l.pvf_chip_quality(c._h, P(chips), 65537, P(q)), "PVF_SHEET_MAX_TILES"),
                          (lambda: l.pvf_chip_quality(c._h, None, 2, P(q)), "null chips"), (lambda: l.pvf_chip_quality(c._h, P(chips), 2, None), "null output"),
                          (lambda: l.pvf_face_quality(c._h, None, P(pts), 2, P(q)), "null chips, frames or landmarks"),
                          (lambda: l.pvf_face_quality(c._h, P(hs), None, 2, P(q)), "null chips, frames or landmarks"),
                          (lambda: l.pvf_face_quality(c._h, P(hs), P(pts), 2, None), "null output"),
                          (lambda: l.pvf_face_quality(c._h, P(hs), P(pts), 65537, P(q)), "PVF_SHEET_MAX_TILES"),
                          (lambda: l.pvf_face_quality(c._h, P(bad_handles), P(pts), 2, P(q)), "unknown frame handle")):
        assert call() != 0 and message in err(), (message, err())

    def sheet(n=2, S=48, W=64, H=64, bg=0, prims=None, text=empty, text_bytes=None, chips_=chips, xy_=xy, out=rgb, n_prims=None):
        p = np.array(prims if prims is not None else [], np.int64).astype(np.int32).reshape(-1, 8)
        return l.pvf_chip_sheet(c._h, P(chips_) if chips_ is not None else None, n, P(xy_) if xy_ is not None else None, S, W, H, bg, P(p) if len(p) else None,
                                len(p) if n_prims is None else n_prims, P(text) if len(text) else None, len(text) if text_bytes is None else text_bytes,
                                P(out) if out is not None else None)
    T = np.frombuffer(b"hello", np.uint8).copy()
    for kw, message in ((dict(S=47), "PVF_SHEET_MIN_TILE"), (dict(S=601), "PVF_SHEET_MIN_TILE"), (dict(W=0), "PVF_SHEET_MAX_SIDE"), (dict(H=0), "PVF_SHEET_MAX_SIDE"),
                        (dict(W=-3), "PVF_SHEET_MAX_SIDE"), (dict(W=16385, H=1), "PVF_SHEET_MAX_SIDE"), (dict(W=1, H=16385), "PVF_SHEET_MAX_SIDE"),
                        (dict(W=16384, H=4097), "PVF_SHEET_MAX_PIXELS"), (dict(n=65537), "PVF_SHEET_MAX_TILES"), (dict(n=-1), "PVF_SHEET_MAX_TILES"),
                        (dict(xy_=None), "null tile corners"), (dict(chips_=None), "null chips"), (dict(out=None), "null output"),
                        (dict(bg=0x1000000), "background"),
                        (dict(prims=[[3, 0, 0, 5, 5, 0, 2, 0]]), "takes no redactions"), (dict(prims=[[4, 0, 0, 5, 5, 0, 0, 0]]), "unknown primitive type"),
                        (dict(prims=[[-1, 0, 0, 5, 5, 0, 0, 0]]), "unknown primitive type"),
                        (dict(prims=[[0, 0, 0, 5, 5, 0, 0, 0]] * 4097), "PVF_RENDER_MAX_PRIMS"), (dict(n_prims=-1), "PVF_RENDER_MAX_PRIMS"),
                        (dict(n_prims=1), "null primitive list"),
                        (dict(text=T, text_bytes=(1 << 20) + 1), "PVF_RENDER_MAX_TEXT"), (dict(text_bytes=3), "null text pool"),
                        (dict(prims=[[2, 0, 9, 3, 3, 0, 1, 0]], text=T), "outside the text pool"), (dict(prims=[[2, 0, 9, -1, 3, 0, 1, 0]], text=T), "outside the text pool"),
                        (dict(prims=[[2, 0, 9, 0, 65, 0, 1, 0]], text=np.zeros(80, np.uint8)), "PVF_RENDER_MAX_RUN"),
                        (dict(prims=[[2, 0, 9, 0, 5, 0, 0, 0]], text=T), "PVF_RENDER_MAX_SCALE"), (dict(prims=[[2, 0, 9, 0, 5, 0, 65, 0]], text=T), "PVF_RENDER_MAX_SCALE")):
        assert sheet(**kw) != 0 and message in err(), (kw.keys(), message, err())
    assert l.pvf_face_sheet(c._h, None, P(pts), 2, P(xy), 48, 64, 64, 0, None, 0, None, 0, P(rgb)) != 0 and "null chips, frames or landmarks" in err()
    assert l.pvf_face_sheet(c._h, P(hs), P(pts), 2, P(xy), 601, 64, 64, 0, None, 0, None, 0, P(rgb)) != 0 and "PVF_SHEET_MIN_TILE" in err()
    assert l.pvf_face_sheet(c._h, P(np.array([f.handle, 987654321], np.uint64)), P(pts), 2, P(xy), 48, 64, 64, 0, None, 0, None, 0, P(rgb)) != 0 \
        and "unknown frame handle" in err()
    # the limits themselves pass, and the context goes on
    assert sheet(S=48) == 0 and sheet(S=600) == 0 and sheet(bg=0xffffff) == 0
    assert sheet(prims=[[2, 0, 9, 0, 5, 0xff, 64, 0], [2, 0, 9, 5, 0, 0xff, 1, 0]], text=T) == 0
    _same(rgb, fr.sheet(chips, xy, 48, 64, 64, (0, 0, 0), [(demo_ref.TEXT, 0, 9, (255, 0, 0), 64, b"hello")]))
    with pytest.raises(_lib.PvfError, match="PVF_SHEET_MAX_PIXELS"):
        c.chip_sheet(chips, xy, 48, 16384, 4097)
    with pytest.raises(ValueError, match="tile corners"):
        c.chip_sheet(chips, xy[:1], 48, 64, 64)
    assert np.array_equal(c.chip_quality(chips), pool()[1][:2])
    f.release()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_process_then_faces(tmp_path, ctx, dlib_ctx, model_paths, small_video):
    from pyannote_video_amd import cli, faces, formats
    v = small_video
    frames = [v.frame(i) for i in range(v.n_frames)]
    npy = str(tmp_path / "clip.npy")
    np.save(npy, np.stack(frames))
    shots = str(tmp_path / "shots.json")
    with open(shots, "w") as f:
        json.dump(v.shots(), f)
    p = {k: str(tmp_path / (k + ".txt")) for k in ("tracking", "landmarks", "embeddings", "labels", "index", "quality", "index2")}
    res = cli.process(cli.open_video(npy, v.frame_rate), shots, model_paths[0], model_paths[1], p["tracking"], p["landmarks"], p["embeddings"],
                      p["labels"], ctx=ctx)
    assert len(res["tracks"]) >= 2
    # the restated verb, fed with the GPU's own chips
    times = [i / v.frame_rate for i in range(len(frames))]
    F = faces.landmark_faces(formats.read_tracks(p["tracking"]), formats.read_landmarks(p["landmarks"]), times, 640, 360)
    assert len(F) >= 10 and F[-1][0] == max(f[0] for f in F)                       # the landmark file's last group takes part
    chips = dlib_ctx.face_chips([frames[f[2]] for f in F], np.stack([f[4] for f in F]))
    Q = fr.qualities(chips)
    sym = [fr.symmetry(f[4]) for f in F]
    sc = [fr.score(q, s) for q, s in zip(Q, sym)]

    def restated(per, S, columns, labels=None, **elig):
        ok = [fr.eligible(q, f[3][3] - f[3][1], 360, **elig) for q, f in zip(Q, F)]
        names = {}
        for i, f in enumerate(F):
            names.setdefault((labels or {}).get(f[1]) or "#%d" % f[1], []).append(i)
        order = sorted(names, key=lambda n: (min(F[i][1] for i in names[n]), n))
        shown = [[names[n][k] for k in fr.choose([(sc[i], F[i][0], F[i][1], ok[i]) for i in names[n]], per, 1.0)] for n in order]
        W, H, corners, prims = fr.layout([(n, min(F[i][1] for i in names[n]), len(s)) for n, s in zip(order, shown)], per, S, columns)
        flat = [i for s in shown for i in s]
        img = fr.sheet(chips[flat], [c for g in corners for c in g], S, W, H, fr.BACKGROUND, prims)
        index = ["%s %d %.3f %d" % (n, r, F[i][0], F[i][1]) for n, s in zip(order, shown) for r, i in enumerate(s)]
        return img, index, ok
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pyannote-video_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "pyannote_video_amd", "--fps", str(v.frame_rate), "faces"]
    # to a file: a group per track, the chip itself as the tile
    out = str(tmp_path / "sheet.ppm")
    run = subprocess.run(base + ["--index", p["index"], "--quality", p["quality"], npy, p["tracking"], p["landmarks"], out],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    img, index, ok = restated(4, 150, 1)
    assert open(out, "rb").read() == fr.ppm(img)
    assert [" ".join(line.split()[:4]) for line in open(p["index"])] == index and len(index) >= 4
    want_q = ["%.3f %d %d %d %d %d %d %.5f %.5f %d" % ((f[0], f[1]) + tuple(int(x) for x in q) + (s, c, int(o))) for f, q, s, c, o in zip(F, Q, sym, sc, ok)]
    assert [line.rstrip("\n") for line in open(p["quality"])] == want_q
    for line in open(p["index"]):                                                 # an index line is its face's quality line behind group and rank
        assert line.split(" ", 2)[2].rstrip("\n") in want_q
    # through `-`, as a user would: a group per cluster, smaller tiles, two columns
    labels = demo_ref.read_label_file(p["labels"])
    run = subprocess.run(base + ["--per", "2", "--tile", "64", "--columns", "2", "--label", p["labels"], "--max-dark", "0.5", "--index", p["index2"],
                                 npy, p["tracking"], p["landmarks"], "-"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    img, index, _ = restated(2, 64, 2, labels, max_dark=0.5)
    assert run.stdout == fr.ppm(img)
    assert [" ".join(line.split()[:4]) for line in open(p["index2"])] == index
