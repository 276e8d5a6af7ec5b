"""GPU: the `redact` verb's kernels (csrc/render.hip: redact_means_k, render_k's REDACT instantiation, pvf_debug_redact_means).  Every
comparison is bit for bit against tests/redact_ref.py, the numpy restatement of REDACT.md: integer arithmetic, no tolerance to choose.
Each case checks the table of cell means, then the drawn RGB, then the planes, in that order, so a failure names the stage:
reduction, composition or colour conversion.
  * sources 7x5, 385x97, 257x255, 641x361; outputs identity, an odd down-scale, an up-scale, 2 x 2;
  * regions inside the frame, crossing each edge, wholly off it, covering it, 1 x 1, inverted, at the coordinate limits;
  * cells 1, 2, 3, 7, 32, 64, 65 (the first the block-per-cell form sums), larger than the region, sides no multiple of the cell;
  * both shapes, all three modes, `smooth` across a frame edge;
  * black, white, noise, checker1 (an even cell of it is a rounding tie); white 641x361 as one cell (a sum beyond 2^24); a 2049 x 3
    white region at cell = 2048 in `smooth` (the widest product);
  * order, two overlapping redactions, 4096 one-pixel redactions, 40 faces on 1080p -> 711x400;
  * batches, the four matrix / range tables, the egress ring, the YUV ingest ring, after detector and tracker work, every refusal;
  * `process` then `redact` end to end, to a file and through `-`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships

from tests import demo_ref, yuv_ref, redact_ref as rr
from tests import detector_cases as dc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [("601", False), ("601", True), ("709", False), ("709", True)]
REDACT, ELLIPSE, MOSAIC, SMOOTH, FILL = rr.REDACT, rr.ELLIPSE, rr.MOSAIC, rr.SMOOTH, rr.FILL
RECT, LINE, TEXT = demo_ref.RECT, demo_ref.LINE, demo_ref.TEXT
LIM = 1 << 20
C1, C2, C3 = (250, 10, 20), (5, 200, 90), (40, 60, 255)
SHAPES_MODES = [(s, m) for s in (0, ELLIPSE) for m in (MOSAIC, SMOOTH, FILL)]


def _src(name, content="noise", seed=0):
    return dc.case_frame(dc.by_name(name), content, seed)


def _p(l, t, r, b, cell, flags, colour=C1):
    return (REDACT, l, t, r, b, colour, cell, flags)


def _check(ctx, src, ow, oh, prims, combos=COMBOS[:1], what=""):
    """the means table, the debug RGB and the planes of every combination against the restatement; returns the reference RGB"""
    want_means = rr.cell_means(src, ow, oh, prims)
    want_rgb = rr.render_rgb(src, ow, oh, prims)
    frame = ctx.upload(src)
    try:
        got_means = ctx.redact_means(frame, prims, ow, oh)
        assert got_means.shape == want_means.shape, "%s: %d cells in the table, not %d" % (what, len(got_means), len(want_means))
        bad = np.flatnonzero((got_means != want_means).any(1))
        assert len(bad) == 0, "%s: cell means differ at %d of %d cells, first %s: got %s, want %s" % (
            what, len(bad), len(want_means), bad[:4].tolist(), got_means[bad[:4]].tolist(), want_means[bad[:4]].tolist())
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


# ---- geometry and regions ------------------------------------------------------------------------------------------------------------
def _regions(ow, oh):
    """lists of redactions on an ow x oh output; within a list the later ones lie over the earlier ones"""
    whole = max(2, -(-max(ow, oh) // 64))
    qx, qy = max(1, ow // 4), max(1, oh // 4)
    k = max(1, max(ow, oh) // 200)              # the cells of the larger regions grow with the output: at most 4096 a redaction
    return {
        "covering the frame": [_p(0, 0, ow - 1, oh - 1, whole, MOSAIC), _p(-100, -100, 16283, 16283, 256, SMOOTH | ELLIPSE)],
        "inside, 1 x 1, inverted, off the frame": [
            _p(qx, qy, qx + ow // 3, qy + oh // 3, 3 * k, MOSAIC | ELLIPSE), _p(ow // 2, oh // 2, ow // 2, oh // 2, 1, MOSAIC), _p(0, 0, 0, 0, 5, SMOOTH),
            _p(ow - 1, oh - 1, ow - 1, oh - 1, 2, MOSAIC | ELLIPSE), _p(qx + 3, qy, qx, qy + 5, 2, MOSAIC), _p(qx, qy + 3, qx + 5, qy, 2, FILL), _p(qx, qy, qx - 1, qy, 1, SMOOTH),
            _p(ow, 0, ow + 40, 20, 4, MOSAIC), _p(-50, -50, -1, -1, 7, SMOOTH | ELLIPSE), _p(0, oh, ow, oh + 9, 3, MOSAIC), _p(3 * ow, -5 * oh, 3 * ow + 70, 9, 32, SMOOTH)],
        "crossing each edge": [
            _p(-ow // 5 - 1, oh // 3, ow // 6, oh // 3 + qy, 7 * k, SMOOTH), _p(ow // 3, -oh // 4 - 2, ow // 3 + qx, oh // 5, 3 * k, MOSAIC | ELLIPSE),
            _p(ow - qx, oh // 2, ow + qx + 1, oh // 2 + qy, 2 * k, SMOOTH | ELLIPSE), _p(ow // 2, oh - qy, ow // 2 + qx, oh + 37, 32, MOSAIC),
            _p(-9, -9, 2, 2, 4, SMOOTH), _p(ow - 3, oh - 3, ow + 8, oh + 8, 4, SMOOTH), _p(-20, oh - 2, 1, oh + 64, 64, MOSAIC), _p(ow - 2, -70, ow + 70, 1, 65, SMOOTH | ELLIPSE)],
        "at the coordinate limits": [
            _p(-LIM, -LIM, -LIM + 16383, -LIM + 16383, 2048, SMOOTH), _p(LIM - 16383, LIM - 16383, LIM, LIM, 256, MOSAIC | ELLIPSE), _p(LIM, LIM, LIM, LIM, 1, MOSAIC),
            _p(-LIM, 0, -LIM + 63, 63, 1, SMOOTH), _p(LIM, -LIM, -LIM, LIM, 2048, MOSAIC), _p(-16383 + 1, -16383 + 1, 1, 1, 2048, MOSAIC | ELLIPSE),
            _p(-16383 + qx, -16383 + qy, qx, qy, 2048, SMOOTH)],
    }


@pytest.mark.parametrize("name", ["7x5_up0", "385x97_up1", "257x255_up0", "641x361_up0"])
def test_geometries_and_regions(ctx, name):
    g = dc.by_name(name)
    src = _src(name)
    outs = [(g.w, g.h), (max(2, g.w // 3) | 1, max(2, g.h // 3) | 1), (g.w * 3 // 2 + 1, g.h * 2 + 1), (2, 2)]
    for ow, oh in outs:
        for what, prims in sorted(_regions(ow, oh).items()):
            rgb = _check(ctx, src, ow, oh, prims, what="%s -> %dx%d, %s" % (name, ow, oh, what))
            if what != "at the coordinate limits" and min(ow, oh) > 8:
                assert not np.array_equal(rgb, demo_ref.resize(src, ow, oh)), "the case draws nothing"


# ---- cells, shapes, modes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [1, 2, 3, 7, 32, 64, 65, 200])
def test_cells_shapes_and_modes(ctx, cell):
    """a 150 x 90 region (no multiple of any of the cells but 1, 2 and 3) on 385 x 97, and one hanging over the right and bottom edges"""
    src = _src("385x97_up1", "noise", 4)
    w, h = (63, 44) if cell == 1 else (150, 90)
    for shape, mode in SHAPES_MODES:
        prims = [_p(5, 3, 5 + w - 1, 3 + h - 1, cell, shape | mode), _p(385 - w // 3, 97 - h // 3, 385 - w // 3 + w - 1, 97 - h // 3 + h - 1, cell, shape | mode, C2)]
        _check(ctx, src, 385, 97, prims, what="cell %d shape %d mode %d" % (cell, shape, mode))
    _check(ctx, src, 201, 51, [_p(-7, -5, -7 + w - 1, -5 + h - 1, cell, SMOOTH | ELLIPSE)], what="cell %d, smooth over the corner of 201x51" % cell)


def test_smooth_across_every_frame_edge(ctx):
    """the neighbours of a pixel near an edge are cells without a pixel in the frame: they are clamped to those that have one"""
    src = _src("257x255_up0", "noise", 5)
    for cell in (3, 16, 50):
        prims = [_p(-2 * cell - 1, 40, 3 * cell, 40 + 3 * cell, cell, SMOOTH), _p(100, -3 * cell + 1, 100 + 4 * cell, cell + 1, cell, SMOOTH | ELLIPSE),
                 _p(257 - cell - 1, 120, 257 + 2 * cell, 120 + 2 * cell + 1, cell, SMOOTH), _p(30, 255 - 2, 30 + 5 * cell, 255 + 3 * cell, cell, SMOOTH)]
        _check(ctx, src, 257, 255, prims, what="smooth over the edges, cell %d" % cell)
    _check(ctx, src, 257, 255, [_p(-300, -300, 600, 600, 100, SMOOTH)], what="smooth, the frame inside one ring of cells")


# ---- content -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", ["black", "white", "noise", "checker1"])
def test_content(ctx, content):
    src = _src("385x97_up1", content, 1)
    prims = [_p(3, 2, 120, 60, 2, MOSAIC), _p(130, 5, 250, 90, 4, SMOOTH | ELLIPSE), _p(260, -4, 390, 50, 3, MOSAIC | ELLIPSE), _p(255, 55, 384, 96, 6, SMOOTH)]
    rgb = _check(ctx, src, 385, 97, prims, COMBOS, content)
    if content == "checker1":
        assert (rgb[2:61, 3:121] == 128).all()                  # 2 x 2 of a 0 / 255 checkerboard: 510 / 4 = 127.5, the tie rounds up
    _check(ctx, src, 201, 51, prims, what=content + " down-scaled")


def test_white_641x361_as_one_cell(ctx):
    """S = 255 * 641 * 361 = 59 007 255 > 2^24: a float accumulator, or a narrow one, shows"""
    src = _src("641x361_up0", "white")
    for flags in (MOSAIC, SMOOTH | ELLIPSE):
        rgb = _check(ctx, src, 641, 361, [_p(0, 0, 640, 360, 641, flags)], what="white as one cell")
        assert (rgb == 255).all()
    noise = _src("641x361_up0", "noise", 2)
    _check(ctx, noise, 641, 361, [_p(0, 0, 640, 360, 641, MOSAIC), _p(-5, -5, 700, 400, 353, SMOOTH)], what="noise as one cell and as four")


def test_the_widest_product(ctx):
    """a 2049 x 3 white region at cell = 2048 in `smooth`: the numerator reaches 255 * 2^24 + 2^23 = 4 286 578 688, held in uint32"""
    src = _src("2049x41_up0", "white")
    rgb = _check(ctx, src, 2049, 41, [_p(0, 1, 2048, 3, 2048, SMOOTH)], what="2049 x 3 at cell 2048")
    assert (rgb == 255).all()
    noise = _src("2049x41_up0", "noise", 3)
    _check(ctx, noise, 2049, 41, [_p(0, 1, 2048, 3, 2048, SMOOTH), _p(-2048, 10, 2047, 39, 2048, SMOOTH | ELLIPSE)], what="2049 x 3 at cell 2048, noise")


# ---- order and volume ----------------------------------------------------------------------------------------------------------------
def test_order(ctx):
    src = _src("385x97_up1", "noise", 6)
    red, rect, text = _p(40, 10, 200, 80, 9, MOSAIC), (RECT, 60, 20, 150, 70, C2), (TEXT, 50, 60, C3, 3, b"over")
    a = _check(ctx, src, 385, 97, [red, rect, text], what="redaction then rectangle")
    b = _check(ctx, src, 385, 97, [rect, text, red], what="rectangle then redaction")
    assert not np.array_equal(a, b)
    assert np.array_equal(b, rr.render_rgb(src, 385, 97, [red]))                  # the redaction is made from the source: the rectangle is gone
    two = [_p(20, 5, 180, 90, 11, MOSAIC), _p(100, 20, 300, 70, 40, SMOOTH | ELLIPSE), _p(150, 0, 170, 96, 5, FILL, C3), _p(160, 30, 260, 60, 7, MOSAIC)]
    _check(ctx, src, 385, 97, two, COMBOS, "overlapping redactions")
    _check(ctx, src, 385, 97, two[::-1], what="overlapping redactions, reversed")


def test_4096_one_pixel_redactions(ctx):
    """every R_CHUNK pass of render_k, and 4096 records for the means kernel to bisect"""
    src = _src("385x97_up1", "noise", 7)
    rng = np.random.RandomState(8)
    xs, ys = rng.randint(-3, 388, 4096), rng.randint(-3, 100, 4096)
    prims = [_p(int(x), int(y), int(x), int(y), 1 + i % 3, (MOSAIC, SMOOTH, FILL)[i % 3] | (i & 1), (i % 256, 255 - i % 256, 77)) for i, (x, y) in enumerate(zip(xs, ys))]
    _check(ctx, src, 385, 97, prims, what="4096 one-pixel redactions")


def test_40_faces_on_1080p(ctx):
    src = dc.frame("noise", 1080, 1920, 9)
    rng = np.random.RandomState(10)
    prims = []
    for i in range(40):
        s = int(rng.randint(20, 110))
        l, t = int(rng.randint(-20, 711 - s + 20)), int(rng.randint(-20, 400 - s + 20))
        prims.append(_p(l, t, l + s, t + s * 5 // 4, -(-(s * 5 // 4 + 1) // 8), SHAPES_MODES[i % 6][0] | SHAPES_MODES[i % 6][1], (i, 2 * i, 3 * i)))
        prims.append((RECT, l, t, l + s, t + s * 5 // 4, C2))
    _check(ctx, src, 711, 400, prims, [("601", False), ("709", True)], "40 faces, 1080p -> 711x400")


# ---- ways of calling -----------------------------------------------------------------------------------------------------------------
def _random_prims(n, seed, w, h):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        x, y = int(rng.randint(-20, w)), int(rng.randint(-20, h))
        if i % 3 == 2:
            out.append((RECT, x, y, x + int(rng.randint(0, 40)), y + int(rng.randint(0, 30)), C3))
        else:
            shape, mode = SHAPES_MODES[int(rng.randint(0, 6))]
            out.append(_p(x, y, x + int(rng.randint(-2, 60)), y + int(rng.randint(-2, 40)), int(rng.randint(1, 20)), shape | mode, tuple(int(v) for v in rng.randint(0, 256, 3))))
    return out


def _batch_case():
    g = dc.by_name(dc.BATCH_SIZE)
    frames = [dc.frame(c, g.h, g.w, s) for c, s in dc.BATCH_FRAMES]
    lists = [_random_prims(n, 20 + i, 193, 49) for i, n in enumerate((0, 5, 300, 0, 1, 64, 2))]
    lists[4] = [(RECT, 5, 5, 50, 30, C1)]                     # a frame without a redaction between frames with some
    return frames, lists, 193, 49


def _want(frames, lists, ow, oh, matrix="601", full=False):
    return [np.frombuffer(rr.render(f, ow, oh, p, matrix, full), np.uint8) for f, p in zip(frames, lists)]


def test_batch_with_different_lists_and_with_none(ctx):
    frames, lists, ow, oh = _batch_case()
    dev = [ctx.upload(f) for f in frames]
    got = ctx.render(dev, lists, ow, oh, "709", False)
    for i, want in enumerate(_want(frames, lists, ow, oh, "709", False)):
        assert np.array_equal(got[i], want), i
    plain = [[p for p in prims if p[0] != REDACT] for prims in lists]              # the same call without redactions: the other instantiation
    got = ctx.render(dev, plain, ow, oh, "709", False)
    for i, want in enumerate(_want(frames, plain, ow, oh, "709", False)):
        assert np.array_equal(got[i], want), i
    none = ctx.render(dev, None, ow, oh)
    for i, want in enumerate(_want(frames, [[]] * len(frames), ow, oh)):
        assert np.array_equal(none[i], want), i
    out = torch.zeros((len(dev), got.shape[1]), dtype=torch.uint8, device="cuda")
    assert ctx.render(dev, lists, ow, oh, "601", True, out_ptr=out.data_ptr()) is None
    for i, want in enumerate(_want(frames, lists, ow, oh, "601", True)):
        assert np.array_equal(out[i].cpu().numpy(), want), i
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
        d.release()                                   # released as soon as the kernels are queued
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
    lists = [_random_prims(20, 40 + i, 41, 27) for i in range(3)]
    for pl, prims in zip(planes, lists):
        y, u, v = ring.slot()
        np.copyto(y, pl[0]); np.copyto(u, pl[1]); np.copyto(v, pl[2])
        f = ring.submit()
        src = yuv_ref.to_rgb(pl[0], pl[1], pl[2], "420", "709", False)
        assert np.array_equal(ctx.redact_means(f, prims, 41, 27), rr.cell_means(src, 41, 27, prims))
        got = ctx.render([f], [prims], 41, 27, "709", False)
        assert np.array_equal(got[0], np.frombuffer(rr.render(src, 41, 27, prims, "709", False), np.uint8))
        f.release()
    ring.close()


def test_after_detector_and_tracker_work(ctx, small_video):
    src = small_video.frame(0)
    f = ctx.upload(src)
    boxes, _ = ctx.detect(f)
    trk = ctx.tracker_create()
    ctx.tracker_start_many([trk], [f], [(200.0, 100.0, 280.0, 180.0)])
    ctx.tracker_update_many([trk], [f])
    prims = [_p(int(b[0]), int(b[1]), int(b[2]), int(b[3]), 11, MOSAIC | ELLIPSE) for b in boxes] + [_p(200, 100, 280, 180, 10, SMOOTH)]
    assert np.array_equal(ctx.redact_means(f, prims, 640, 360), rr.cell_means(src, 640, 360, prims))
    got = ctx.render([f], [prims], 640, 360)
    assert np.array_equal(got[0], np.frombuffer(rr.render(src, 640, 360, prims), np.uint8))
    ctx.tracker_destroy(trk)
    f.release()


def test_refusals_return_errors_and_the_context_goes_on(ctx):
    from pyannote_video_amd import _lib
    src = _src("385x97_up1")
    f = ctx.upload(src)
    out = np.zeros(40 * 20 * 3, np.uint8)
    hs = np.array([f.handle], np.uint64)
    empty = np.zeros(0, np.uint8)
    err = lambda: ctx._l.pvf_last_error().decode()

    def row(l, t, r, b, cell, flags):
        return [REDACT, l, t, r, b, 0x0A0B0C | flags << 24, cell, 12345]           # `reserved` is the library's, whatever the caller puts there

    def call(rows):
        p = np.array(rows, np.int64).astype(np.int32).reshape(-1, 8)
        return ctx._l.pvf_render_batch(ctx._h, _lib.ptr(hs), 1, 40, 20, 0, _lib.ptr(np.array([0, len(p)], np.int32)), _lib.ptr(p), _lib.ptr(empty), 0, _lib.ptr(out), 0)
    for rows, message in (([row(-LIM - 1, 0, 5, 5, 2, 0)], "PVF_REDACT_MAX_COORD"), ([row(0, 0, 5, LIM + 1, 2, 0)], "PVF_REDACT_MAX_COORD"),
                          ([row(9, 0, -LIM - 1, 5, 2, 0)], "PVF_REDACT_MAX_COORD"),
                          ([row(0, 0, 16384, 5, 2048, 0)], "PVF_REDACT_MAX_SIDE"), ([row(0, 0, 5, 16384, 2048, FILL)], "PVF_REDACT_MAX_SIDE"),
                          ([row(0, 0, 5, 5, 0, 0)], "cell outside 1 .. PVF_REDACT_MAX_CELL"), ([row(0, 0, 5, 5, 2049, 0)], "cell outside 1 .. PVF_REDACT_MAX_CELL"),
                          ([row(0, 0, 5, 5, -1, FILL)], "cell outside 1 .. PVF_REDACT_MAX_CELL"),
                          ([row(0, 0, 64, 63, 1, 0)], "PVF_REDACT_MAX_CELLS"), ([row(0, 0, 64, 63, 1, FILL)], "PVF_REDACT_MAX_CELLS"),
                          ([row(0, 0, 5, 5, 2, 8)], "redaction flags"), ([row(0, 0, 5, 5, 2, 6)], "redaction flags"), ([row(0, 0, 5, 5, 2, 128)], "redaction flags"),
                          ([row(0, 0, 63, 63, 1, 0)] * 1025, "PVF_REDACT_MAX_TABLE")):
        assert call(rows) != 0 and message in err(), (rows[0], message, err())
    assert call([row(0, 0, 63, 63, 1, 0)] * 1024) == 0                            # 2^22 cells: the limit itself
    assert call([row(-LIM, -LIM, -LIM + 16383, -LIM + 16383, 2048, SMOOTH), row(LIM, LIM, -LIM, -LIM, 1, 0), row(0, 0, 16383, 16383, 256, MOSAIC | ELLIPSE)]) == 0
    good = [_p(0, 0, 5, 5, 2, MOSAIC)]
    want = np.frombuffer(rr.render(src, 40, 20, good), np.uint8)
    assert call([row(0, 0, 5, 5, 2, 0)]) == 0                                     # the context goes on, and `reserved` = 12345 did no harm
    assert np.array_equal(out[:len(want)], want)
    # the debug entry: its capacity, its frame
    p = np.array([row(0, 0, 5, 5, 2, 0)], np.int64).astype(np.int32)
    means = np.zeros(27, np.uint8)
    assert ctx._l.pvf_debug_redact_means(ctx._h, f.handle, 40, 20, _lib.ptr(p), 1, _lib.ptr(means), 26) != 0 and "the tables need 27 bytes" in err()
    assert ctx._l.pvf_debug_redact_means(ctx._h, f.handle, 40, 20, _lib.ptr(p), 1, _lib.ptr(means), 27) == 0
    assert np.array_equal(means.reshape(9, 3), rr.cell_means(src, 40, 20, good))
    assert ctx._l.pvf_debug_redact_means(ctx._h, f.handle, 1, 20, _lib.ptr(p), 1, _lib.ptr(means), 27) != 0 and "2 x 2" in err()
    assert ctx._l.pvf_debug_redact_means(ctx._h, f.handle, 40, 20, None, 1, _lib.ptr(means), 27) != 0 and "null primitive list" in err()
    g = ctx.upload(src)
    stale = g.handle
    g.release()
    assert ctx._l.pvf_debug_redact_means(ctx._h, stale, 40, 20, _lib.ptr(p), 1, _lib.ptr(means), 27) != 0 and "unknown frame handle" in err()
    with pytest.raises(ValueError, match="cells"):                                  # the Python side refuses before the library would
        ctx.render_rgb(f, [_p(0, 0, 64, 63, 1, MOSAIC)], 40, 20)
    ring = ctx.egress_ring(40, 20, depth=2)
    s = ring.submit(f, good)
    assert np.array_equal(ring.wait(s), want)
    ring.release(s)
    ring.close()
    f.release()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_process_then_redact(tmp_path, ctx, model_paths, small_video):
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
    labels = demo_ref.read_label_file(p["labels"])
    assert rows and labels
    rate = "%d:1" % int(v.frame_rate)
    # to a file, source size, every track, `demo`'s drawing on top
    out = str(tmp_path / "redacted.y4m")
    r = cli.redact(cli.open_video(npy, v.frame_rate), p["tracking"], out, label=p["labels"], draw=True, ctx=ctx)
    want = rr.redact_bytes(frames, v.frame_rate, rate, rows, labels=labels, draw=True)
    got = open(out, "rb").read()
    plan = rr.plan(rows, v.frame_rate, len(frames), 640, 360)
    assert r["frames"] == v.n_frames and (r["width"], r["height"]) == (640, 360)
    assert r["redactions"] == sum(len(prims) for _, _, prims in plan) >= v.n_frames
    assert len(plan[-1][2]) >= 1                                                   # the last time's faces are hidden too
    assert len(got) == len(want) and got == want
    back = y4m.Y4mVideo(out)
    assert len(back) == v.n_frames and back.size == (640, 360)
    # through `-`, as a user would: the verb in a process of its own; one label is kept, the others and the tracks without one are hidden
    kept = sorted(set(labels.values()))[0]
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pyannote-video_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "pyannote_video_amd", "--fps", str(v.frame_rate), "--matrix", "709", "--range", "full", "redact", "--height", "200",
           "--from", "0.08", "--until", "0.44", "--shift", "0.04", "--label", p["labels"], "--keep", kept, "--pad", "10", "--cells", "5", "--shape", "box",
           "--mode", "smooth", npy, p["tracking"], "-"]
    piped = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert piped.returncode == 0, piped.stderr.decode()[-2000:]
    options = dict(labels=labels, keep={kept}, pad=10, cells=5, shape="box", mode="smooth", t_from=0.08, t_until=0.44, shift=0.04)
    want = rr.redact_bytes(frames, v.frame_rate, rate, rows, 200, "709", True, **options)
    head = b"YUV4MPEG2 W355 H200 F%s C420 XCOLORRANGE=FULL\n" % rate.encode()
    assert want.startswith(head)
    assert len(piped.stdout) == len(want) and piped.stdout == want
    # the kept track's box, in the stream: the luma of the un-redacted resize wherever no redaction reaches
    hidden = rr.plan(rows, v.frame_rate, len(frames), 355, 200, **options)
    everyone = rr.plan(rows, v.frame_rate, len(frames), 355, 200, **dict(options, keep=None, labels=None))
    fb = 355 * 200 + 2 * 178 * 100
    seen = 0
    for k, ((i, _, some), (_, _, every)) in enumerate(zip(hidden, everyone)):
        at = len(head) + k * (6 + fb) + 6
        luma = np.frombuffer(piped.stdout[at:at + 355 * 200], np.uint8).reshape(200, 355)
        plain = demo_ref.to_yuv420(demo_ref.resize(frames[i], 355, 200), "709", True)[0]
        free = np.ones((200, 355), bool)
        for o in some:
            free[max(o[2], 0):max(o[4] + 1, 0), max(o[1], 0):max(o[3] + 1, 0)] = False
        for q in every:
            if q in some:
                continue
            box = np.zeros((200, 355), bool)
            box[max(q[2], 0):max(q[4] + 1, 0), max(q[1], 0):max(q[3] + 1, 0)] = True
            assert np.array_equal(luma[box & free], plain[box & free])
            seen += int((box & free).sum())
    assert seen > 0, "no kept face was on screen"
