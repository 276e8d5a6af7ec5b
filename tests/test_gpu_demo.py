"""GPU: the `demo` verb's kernel and rings (csrc/render.hip: render_k, pvf_render_batch, pvf_egress_*, pvf_debug_render_rgb).  Every
comparison is bit for bit against tests/demo_ref.py, the numpy restatement of DEMO.md: integer arithmetic, no tolerance to choose.
The debug entry returns the drawn RGB before colour conversion, so a failure says which of resize, drawing and conversion it is.
  * the resize stage also equals the oracle's cv_resize; source sizes are detector_cases.py's odd geometries;
  * outputs 2 x 2, odd x odd, 711 x 400 from 1920 x 1080, an up-scale, identity;
  * primitives crossing, touching, leaving and dwarfing the frame, negative and huge coordinates, inverted boxes, text off every edge,
    every printable byte, bytes outside 32 .. 126, scales 1 .. 4, 4096 primitives on a frame, overlaps in both orders;
  * black, white, noise and saturated checkerboard content; all four matrix / range combinations;
  * batches with different lists, the ring against the batch, frames from the YUV ingest ring, after detector and tracker work;
  * the refusals; `process` then `demo` end to end, to a file and through `-`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships

from tests import demo_ref, yuv_ref
from tests import detector_cases as dc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [("601", False), ("601", True), ("709", False), ("709", True)]
RECT, LINE, TEXT = demo_ref.RECT, demo_ref.LINE, demo_ref.TEXT
BIG, SMALL = 2 ** 31 - 1, -2 ** 31


def _src(name, content="noise", seed=0):
    return dc.case_frame(dc.by_name(name), content, seed)


def _check(ctx, src, ow, oh, prims, combos=COMBOS, what=""):
    """debug RGB and the planes of every combination against the restatement; returns the reference RGB"""
    want_rgb = demo_ref.render_rgb(src, ow, oh, prims)
    frame = ctx.upload(src)
    try:
        got_rgb = ctx.render_rgb(frame, prims, ow, oh)
        assert got_rgb.shape == want_rgb.shape
        bad = np.argwhere((got_rgb != want_rgb).any(2))
        assert len(bad) == 0, "%s: drawn RGB differs at %d pixels, first (y, x) = %s" % (what, len(bad), bad[:4].tolist())
        for matrix, full in combos:
            got = ctx.render([frame], [prims], ow, oh, matrix, full)
            want = np.frombuffer(b"".join(p.tobytes() for p in demo_ref.to_yuv420(want_rgb, matrix, full)), np.uint8)
            assert got.shape == (1, len(want))
            diff = np.flatnonzero(got[0] != want)
            assert len(diff) == 0, "%s %s %s: planes differ at %d bytes, first offsets %s (Y plane has %d bytes)" % (
                what, matrix, "full" if full else "limited", len(diff), diff[:6].tolist(), ow * oh)
    finally:
        frame.release()
    return want_rgb


# ---- resize and output geometry ------------------------------------------------------------------------------------------------------
ODD_SOURCES = ["641x361_up1", "385x97_up1", "257x255_up0", "642x361_up1", "255x100_up1", "1543x41_up1", "7x5_up0"]


@pytest.mark.parametrize("name", ODD_SOURCES)
def test_resize_stage_and_output_geometries(ctx, oracle, name):
    g = dc.by_name(name)
    src = _src(name)
    outs = [(2, 2), (g.w, g.h), (g.w * 3 // 2 + 1, g.h * 2 + 1), (max(2, g.w // 3) | 1, max(2, g.h // 3) | 1), (max(2, g.w // 2) & ~1, max(3, g.h // 2) | 1)]
    for ow, oh in outs:
        rgb = _check(ctx, src, ow, oh, [], COMBOS if (ow, oh) == outs[3] else COMBOS[:1], "%s -> %dx%d" % (name, ow, oh))
        assert np.array_equal(rgb, oracle.cv_resize(src, ow, oh))
        if (ow, oh) == (g.w, g.h):
            assert np.array_equal(rgb, src)                      # identity goes through the same formula and comes out unchanged


def test_1080p_to_the_default_height(ctx, oracle):
    src = dc.frame("renderer", 1080, 1920, 3)
    ow, oh = int(400 / 1080 * 1920), 400
    assert (ow, oh) == (711, 400)
    prims = [(TEXT, 10, 390, (255, 0, 0), 2, b"12.345"), (RECT, 100, 80, 260, 300, tuple(demo_ref.PALETTE[3])),
             (TEXT, 100, 315, (255, 0, 0), 2, b"#3"), (TEXT, 100, 73, (255, 0, 0), 2, b"label"), (LINE, 180, 150, 184, 210, tuple(demo_ref.PALETTE[3])),
             (RECT, 600, 300, 720, 420, tuple(demo_ref.PALETTE[7])), (TEXT, 690, 200, (255, 0, 0), 2, b"#1234567")]
    rgb = _check(ctx, src, ow, oh, prims, COMBOS, "1080p -> 711x400")
    assert not np.array_equal(rgb, oracle.cv_resize(src, ow, oh))
    _check(ctx, src, ow, oh, [], COMBOS[:1], "1080p -> 711x400, nothing drawn")


# ---- content -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", ["black", "white", "noise", "checker1", "checker2", "checker1_r", "checker1_b", "noise_tail"])
def test_content(ctx, content):
    src = _src("385x97_up1", content, 1)
    prims = [(RECT, 20, 10, 90, 40, (0, 255, 0)), (LINE, 0, 0, 200, 50, (0, 0, 255)), (TEXT, 5, 48, (255, 255, 255), 1, b"content")]
    _check(ctx, src, 201, 51, prims, COMBOS, content)
    _check(ctx, src, 385, 97, [], COMBOS, content + " identity")


# ---- primitives ----------------------------------------------------------------------------------------------------------------------
W, H = 301, 61          # the output of the primitive cases (from a 255 x 100 source: an up-scale in x, a down-scale in y)
C1, C2, C3 = (250, 10, 20), (5, 200, 90), (40, 60, 255)
PRINTABLE = bytes(range(32, 127))


def _random_prims(n, seed):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        kind = i % 3
        colour = tuple(int(v) for v in rng.randint(0, 256, 3))
        if kind == RECT:
            x, y = int(rng.randint(-20, W + 20)), int(rng.randint(-20, H + 20))
            out.append((RECT, x, y, x + int(rng.randint(-3, 40)), y + int(rng.randint(-3, 30)), colour))
        elif kind == LINE:
            out.append((LINE, int(rng.randint(-30, W + 30)), int(rng.randint(-30, H + 30)), int(rng.randint(-30, W + 30)), int(rng.randint(-30, H + 30)), colour))
        else:
            text = bytes(rng.randint(0, 256, int(rng.randint(0, 9))).astype(np.uint8))
            out.append((TEXT, int(rng.randint(-30, W + 10)), int(rng.randint(-5, H + 20)), colour, int(rng.randint(1, 4)), text))
    return out


PRIM_CASES = {
    "nothing": [],
    "rectangles crossing, touching, leaving, dwarfing": [
        (RECT, -10, -10, 30, 20, C1), (RECT, 0, 0, W - 1, H - 1, C2), (RECT, 1, 1, W - 2, H - 2, C3), (RECT, 280, 40, 400, 90, C1),
        (RECT, W, 10, W + 30, 30, C2), (RECT, W + 1, 10, W + 30, 30, C2), (RECT, 50, -30, 80, -1, C3), (RECT, 50, -30, 80, -2, C3),
        (RECT, -1000, -1000, 1000, 1000, C1), (RECT, -1, -1, W, H, C2)],
    "negative and huge coordinates": [
        (RECT, SMALL, SMALL, BIG, BIG, C1), (RECT, SMALL, 20, BIG, 30, C2), (RECT, 100, SMALL, 110, BIG, C3), (RECT, BIG, BIG, SMALL, SMALL, C1),
        (RECT, SMALL, SMALL, SMALL, SMALL, C2), (RECT, BIG, BIG, BIG, BIG, C2), (RECT, SMALL, SMALL, 5, 5, C3), (RECT, W - 5, H - 5, BIG, BIG, C1),
        (LINE, SMALL, SMALL, BIG, BIG, C2), (LINE, SMALL, 5, BIG, 6, C3), (LINE, BIG, 40, SMALL, 10, C1), (LINE, 7, SMALL, 9, BIG, C2),
        (LINE, SMALL, BIG, BIG, SMALL, C3), (LINE, -100000, -3, 100000, 70, C1), (LINE, 40000, 33000, -40000, -32000, C2),
        (LINE, BIG, BIG, BIG, BIG, C1), (LINE, SMALL, 0, SMALL, 0, C1),
        (TEXT, SMALL, 30, C1, 4, b"far left"), (TEXT, BIG, 30, C1, 4, b"far right"), (TEXT, 10, SMALL, C2, 4, b"far up"), (TEXT, 10, BIG, C2, 4, b"far down"),
        (TEXT, BIG - 100, BIG, C3, 1, b"x" * 64), (TEXT, SMALL, SMALL, C3, 1, b"x" * 64)],
    "inverted and degenerate boxes": [
        (RECT, 40, 10, 38, 30, C1), (RECT, 60, 10, 57, 30, C2), (RECT, 80, 30, 100, 28, C3), (RECT, 120, 30, 120, 30, C1), (RECT, 140, 30, 141, 31, C2),
        (RECT, 160, 40, 150, 20, C3), (RECT, 180, 20, 179, 50, C1), (RECT, 200, 20, 202, 22, C2), (RECT, 0, 0, 0, 0, C3), (RECT, W - 1, H - 1, W - 1, H - 1, C1)],
    "lines": [
        (LINE, 0, 0, W - 1, H - 1, C1), (LINE, W - 1, 0, 0, H - 1, C2), (LINE, 10, 30, 290, 30, C3), (LINE, 150, -5, 150, 70, C1), (LINE, 20, 20, 20, 20, C2),
        (LINE, 0, 10, 40, 30, C3), (LINE, 40, 30, 0, 10, C1), (LINE, 100, 5, 104, 55, C2), (LINE, 104, 5, 100, 55, C3), (LINE, 200, 50, 260, 50 - 60, C1),
        (LINE, -40, 20, 30, -15, C2), (LINE, 295, 58, 320, 70, C3), (LINE, 50, 10, 54, 12, C1), (LINE, 54, 14, 50, 12, C2)],
    "text off every edge": [
        (TEXT, -14, 20, C1, 2, b"left edge"), (TEXT, W - 30, 40, C2, 2, b"right edge"), (TEXT, 100, 5, C3, 2, b"top edge"), (TEXT, 150, H + 6, C1, 2, b"bottom"),
        (TEXT, -3, 3, C2, 1, b"corner"), (TEXT, W - 8, H + 3, C3, 1, b"corner"), (TEXT, -200, 30, C1, 1, b"gone"), (TEXT, 10, -1, C2, 1, b"gone"),
        (TEXT, 10, H + 7, C2, 1, b"gone"), (TEXT, W, 30, C3, 1, b"gone"), (TEXT, 30, 58, C1, 3, b""), (TEXT, -380, 55, C3, 1, b"#" * 64)],
    "every printable byte": [(TEXT, 2, 10, C1, 1, PRINTABLE[:48]), (TEXT, 2, 20, C2, 1, PRINTABLE[48:]), (TEXT, -300, 40, C3, 2, PRINTABLE[:64]),
                             (TEXT, 1, 58, C1, 2, PRINTABLE[64:])],
    "bytes outside 32 .. 126": [(TEXT, 2, 10, C1, 1, bytes(range(0, 32))), (TEXT, 2, 20, C2, 1, bytes(range(127, 175))), (TEXT, 2, 30, C3, 1, bytes(range(175, 239))),
                                (TEXT, 2, 40, C1, 1, bytes(range(239, 256)) + "né€".encode("utf-8")), (TEXT, 2, 58, C2, 2, b"a\x00b\xffc\x7f")],
    "scales 1 .. 4": [(TEXT, 3, 9, C1, 1, b"scale 1 #0.123"), (TEXT, 3, 25, C2, 2, b"scale 2 #0.123"), (TEXT, 120, 24, C3, 3, b"scale 3"), (TEXT, 100, 58, C1, 4, b"scale 4"),
                      (TEXT, 0, 60, C2, 64, b"Q")],
    "overlap, one order": [(RECT, 30, 10, 120, 50, C1), (LINE, 0, 30, 300, 31, C2), (TEXT, 28, 34, C3, 3, b"over"), (RECT, 60, 5, 90, 58, C2), (TEXT, 58, 30, C1, 2, b"under")],
    "overlap, the other order": [(TEXT, 58, 30, C1, 2, b"under"), (RECT, 60, 5, 90, 58, C2), (TEXT, 28, 34, C3, 3, b"over"), (LINE, 0, 30, 300, 31, C2), (RECT, 30, 10, 120, 50, C1)],
    "4096 primitives": _random_prims(4096, 4),
    "257 primitives": _random_prims(257, 5),
}


@pytest.mark.parametrize("case", sorted(PRIM_CASES))
def test_primitives(ctx, case):
    src = _src("255x100_up1", "noise", 2)
    prims = PRIM_CASES[case]
    rgb = _check(ctx, src, W, H, prims, [("601", False), ("709", True)], case)
    if case != "nothing":
        assert not np.array_equal(rgb, demo_ref.resize(src, W, H)), "the case draws nothing"


def test_primitives_on_a_2x2_and_an_odd_output(ctx):
    src = _src("385x97_up1", "noise", 3)
    _check(ctx, src, 2, 2, [(RECT, 0, 0, 5, 5, C1), (LINE, 1, 0, 1, 1, C2)], COMBOS, "2x2")
    _check(ctx, src, 3, 3, [(TEXT, 0, 2, C3, 1, b"#")], COMBOS, "3x3")
    _check(ctx, src, 33, 35, _random_prims(60, 9), COMBOS, "33x35")


# ---- ways of calling -----------------------------------------------------------------------------------------------------------------
def _batch_case():
    g = dc.by_name(dc.BATCH_SIZE)
    frames = [dc.frame(c, g.h, g.w, s) for c, s in dc.BATCH_FRAMES]
    lists = [_random_prims(n, 20 + i) for i, n in enumerate((0, 5, 300, 0, 1, 64, 0))]
    return frames, lists, 193, 49


def _want(frames, lists, ow, oh, matrix="601", full=False):
    return [np.frombuffer(demo_ref.render(f, ow, oh, p, matrix, full), np.uint8) for f, p in zip(frames, lists)]


def test_batch_with_different_lists(ctx):
    frames, lists, ow, oh = _batch_case()
    dev = [ctx.upload(f) for f in frames]
    got = ctx.render(dev, lists, ow, oh, "709", False)
    for i, want in enumerate(_want(frames, lists, ow, oh, "709", False)):
        assert np.array_equal(got[i], want), i
    none = ctx.render(dev, None, ow, oh)
    for i, want in enumerate(_want(frames, [[]] * len(frames), ow, oh)):
        assert np.array_equal(none[i], want), i
    # the same into device memory
    out = torch.zeros((len(dev), got.shape[1]), dtype=torch.uint8, device="cuda")
    assert ctx.render(dev, lists, ow, oh, "709", False, out_ptr=out.data_ptr()) is None
    assert np.array_equal(out.cpu().numpy(), got)
    for d in dev:
        d.release()


def test_ring_equals_batch(ctx):
    frames, lists, ow, oh = _batch_case()
    want = _want(frames, lists, ow, oh, "601", True)
    ring = ctx.egress_ring(ow, oh, "601", True, depth=3)
    dev = [ctx.upload(f) for f in frames]
    got, pending = [], []
    for d, p in zip(dev, lists):
        if len(pending) == 3:
            s = pending.pop(0)
            got.append(ring.wait(s).copy())
            ring.release(s)
        pending.append(ring.submit(d, p))
        d.release()                                   # released as soon as the render is queued
    for s in pending:
        got.append(ring.wait(s).copy())
        ring.release(s)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), i
    ring.close()


def test_frames_from_the_yuv_ingest_ring(ctx):
    w, h = 67, 45
    planes = [yuv_ref.noise_planes(h, w, "420", s) for s in range(3)]
    ring = ctx.ingest_ring_yuv(h, w, "420", "709", False, depth=2)
    lists = [_random_prims(20, 40 + i) for i in range(3)]
    for pl, prims in zip(planes, lists):
        y, u, v = ring.slot()
        np.copyto(y, pl[0]); np.copyto(u, pl[1]); np.copyto(v, pl[2])
        f = ring.submit()
        src = yuv_ref.to_rgb(pl[0], pl[1], pl[2], "420", "709", False)
        got = ctx.render([f], [prims], 41, 27, "709", False)
        assert np.array_equal(got[0], np.frombuffer(demo_ref.render(src, 41, 27, prims, "709", False), np.uint8))
        f.release()
    ring.close()


def test_after_detector_and_tracker_work(ctx, small_video):
    src = small_video.frame(0)
    f = ctx.upload(src)
    boxes, _ = ctx.detect(f)
    trk = ctx.tracker_create()
    ctx.tracker_start_many([trk], [f], [(200.0, 100.0, 280.0, 180.0)])
    ctx.tracker_update_many([trk], [f])
    prims = [(RECT, int(b[0] * 200 / 360), int(b[1] * 200 / 360), int(b[2] * 200 / 360), int(b[3] * 200 / 360), C1) for b in boxes] + [(TEXT, 10, 190, C2, 1, b"0.000")]
    got = ctx.render([f], [prims], 355, 200)
    assert np.array_equal(got[0], np.frombuffer(demo_ref.render(src, 355, 200, prims), np.uint8))
    ctx.tracker_destroy(trk)
    f.release()


def test_refusals_return_errors_and_the_context_goes_on(ctx):
    import ctypes as C
    from pyannote_video_amd import _lib, render
    src = _src("385x97_up1")
    f = ctx.upload(src)
    one = [[(RECT, 1, 1, 5, 5, C1)]]
    with pytest.raises(_lib.PvfError, match="2 x 2"):
        ctx.render([f], one, 1, 2)
    with pytest.raises(_lib.PvfError, match="2 x 2"):
        ctx.render([f], one, 40, 1)
    with pytest.raises(_lib.PvfError, match="2 x 2"):
        ctx.egress_ring(0, 10)
    with pytest.raises(_lib.PvfError, match="2 x 2"):
        ctx.render_rgb(f, [], 1, 1)
    # the caps, given to the library directly (pack_primitives refuses them before it would)
    prims = np.zeros((4097, 8), np.int32)
    prims[:, 3:5] = 4
    out = np.zeros(40 * 20 * 3, np.uint8)
    hs = np.array([f.handle], np.uint64)
    call = lambda start, p, text: ctx._l.pvf_render_batch(ctx._h, _lib.ptr(hs), 1, 40, 20, 0, _lib.ptr(np.array(start, np.int32)), _lib.ptr(p),
                                                          _lib.ptr(text), len(text), _lib.ptr(out), 0)
    err = lambda: ctx._l.pvf_last_error().decode()
    empty = np.zeros(1, np.uint8)
    assert call([0, 4097], prims, empty[:0]) != 0 and "PVF_RENDER_MAX_PRIMS" in err()
    assert call([0, 4096], prims, empty[:0]) == 0
    text = np.full(200, ord("a"), np.uint8)
    run = np.array([[render.PRIM_TEXT, 0, 10, 0, 65, 255, 1, 0]], np.int32)
    assert call([0, 1], run, text) != 0 and "PVF_RENDER_MAX_RUN" in err()
    run[0, 4] = 64
    assert call([0, 1], run, text) == 0
    run[0, 3] = 150                                   # 150 + 64 > 200: outside the pool
    assert call([0, 1], run, text) != 0 and "outside the text pool" in err()
    run[0, 3], run[0, 6] = 0, 0
    assert call([0, 1], run, text) != 0 and "scale" in err()
    run[0, 6], run[0, 0] = 1, 7
    assert call([0, 1], run, text) != 0 and "unknown primitive type" in err()
    run[0, 0] = render.PRIM_TEXT
    too_much = np.zeros(render.MAX_TEXT_BYTES + 1, np.uint8)
    assert call([0, 1], run, too_much) != 0 and "PVF_RENDER_MAX_TEXT" in err()
    assert ctx._l.pvf_render_batch(ctx._h, _lib.ptr(hs), 1, 40, 20, 4, None, None, None, 0, _lib.ptr(out), 0) != 0 and "flags" in err()
    # null and released frames
    zero = np.zeros(1, np.uint64)
    assert ctx._l.pvf_render_batch(ctx._h, _lib.ptr(zero), 1, 40, 20, 0, None, None, None, 0, _lib.ptr(out), 0) != 0 and "unknown frame handle" in err()
    ring = ctx.egress_ring(40, 20, depth=2)
    g = ctx.upload(src)
    stale = g.handle
    g.release()
    s = C.c_int32(0)
    assert ctx._l.pvf_egress_submit(ctx._h, ring._r, stale, None, 0, None, 0, C.byref(s)) != 0 and "unknown frame handle" in err()
    assert ctx._l.pvf_debug_render_rgb(ctx._h, stale, 40, 20, None, 0, None, 0, _lib.ptr(out)) != 0 and "unknown frame handle" in err()
    # a full ring refuses, a slot given back twice too; the ring goes on
    a, b = ring.submit(f, one[0]), ring.submit(f, [])
    with pytest.raises(_lib.PvfError, match="full"):
        ring.submit(f, [])
    with pytest.raises(_lib.PvfError, match="not held"):
        ring.release(a)
    first = ring.wait(a).copy()
    ring.release(a)
    with pytest.raises(_lib.PvfError, match="not held"):
        ring.release(a)
    with pytest.raises(_lib.PvfError, match="no frame in flight"):
        ring.wait(a)
    ring.wait(b)
    ring.release(b)
    c = ring.submit(f, one[0])
    assert np.array_equal(ring.wait(c), first)
    ring.release(c)
    ring.close()
    assert np.array_equal(first, np.frombuffer(demo_ref.render(src, 40, 20, one[0]), np.uint8))
    f.release()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_process_then_demo(tmp_path, ctx, model_paths, small_video):
    import json
    from pyannote_video_amd import cli, y4m
    v = small_video
    frames = [v.frame(i) for i in range(v.n_frames)]
    npy = str(tmp_path / "clip.npy")
    np.save(npy, np.stack(frames))
    shots = str(tmp_path / "shots.json")
    with open(shots, "w") as f:
        json.dump(v.shots(), f)
    p = {k: str(tmp_path / (k + ".txt")) for k in ("tracking", "landmarks", "embeddings", "labels")}
    res = cli.process(cli.open_video(npy, v.frame_rate), shots, model_paths[0], model_paths[1], p["tracking"], p["landmarks"], p["embeddings"],
                      p["labels"], ctx=ctx)
    assert len(res["tracks"]) >= 2
    rows = demo_ref.read_track_file(p["tracking"])
    marks = demo_ref.read_landmark_file(p["landmarks"])
    labels = demo_ref.read_label_file(p["labels"])
    assert rows and marks and labels
    rate = "%d:1" % int(v.frame_rate)
    assert float(int(v.frame_rate)) == v.frame_rate
    out = str(tmp_path / "demo.y4m")
    r = cli.demo(cli.open_video(npy, v.frame_rate), p["tracking"], out, height=200, landmark=p["landmarks"], label=p["labels"], ctx=ctx)
    want = demo_ref.demo_bytes(frames, v.frame_rate, rate, rows, 200, marks, labels)
    got = open(out, "rb").read()
    assert r["frames"] == v.n_frames and (r["width"], r["height"]) == (355, 200)
    assert len(got) == len(want) and got == want
    plan = demo_ref.plan(rows, v.frame_rate, len(frames), 355, 200, marks, labels)
    kinds = [p_[0] for _, _, prims in plan for p_ in prims]
    assert kinds.count(RECT) >= 4 and kinds.count(LINE) >= 4 and kinds.count(TEXT) > len(plan) + kinds.count(RECT)      # labels are drawn too
    back = y4m.Y4mVideo(out)
    assert len(back) == v.n_frames and back.size == (355, 200)
    # through `-`, as a user would: the verb in a process of its own, BT.709 full range, a window of the video, a shift
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pyannote-video_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "pyannote_video_amd", "--fps", str(v.frame_rate), "--matrix", "709", "--range", "full", "demo", "--height", "121",
           "--from", "0.08", "--until", "0.4", "--shift", "0.04", "--landmark", p["landmarks"], "--label", p["labels"], npy, p["tracking"], "-"]
    piped = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert piped.returncode == 0, piped.stderr.decode()[-2000:]
    want = demo_ref.demo_bytes(frames, v.frame_rate, rate, rows, 121, marks, labels, "709", True, t_from=0.08, t_until=0.4, shift=0.04)
    assert want.startswith(b"YUV4MPEG2 W215 H121 F%s C420 XCOLORRANGE=FULL\n" % rate.encode())
    assert len(piped.stdout) == len(want) and piped.stdout == want
