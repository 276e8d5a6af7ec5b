"""CPU: REDACT.md on its restatement (tests/redact_ref.py) and on the host code of the `redact` verb (render.build_redaction_plan,
render.pack_primitives, the parser).  The properties a redaction must have whatever computes it -- a mosaic cell shows one value and
hides a changed pixel, a fill shows nothing of the source, what is not covered is untouched -- the selection table, the last time's
faces, the padding and cell rules on hand-computed boxes, the limits."""
import os

import numpy as np
import pytest

from tests import demo_ref, redact_ref as rr
from tests import detector_cases as dc
from pyannote_video_amd import cli, render

REDACT, ELLIPSE, MOSAIC, SMOOTH, FILL = rr.REDACT, rr.ELLIPSE, rr.MOSAIC, rr.SMOOTH, rr.FILL
K = (9, 8, 7)


def _src(content="noise", name="385x97_up1", seed=0):
    return dc.case_frame(dc.by_name(name), content, seed)


def _p(l, t, r, b, cell, flags, colour=K):
    return (REDACT, l, t, r, b, colour, cell, flags)


def test_constants_agree_with_the_package():
    assert (render.PRIM_REDACT, render.REDACT_ELLIPSE, render.REDACT_MOSAIC, render.REDACT_SMOOTH, render.REDACT_FILL) == (REDACT, ELLIPSE, MOSAIC, SMOOTH, FILL)
    assert (render.REDACT_MAX_SIDE, render.REDACT_MAX_COORD, render.REDACT_MAX_CELL, render.REDACT_MAX_CELLS) == (rr.MAX_SIDE, rr.MAX_COORD, rr.MAX_CELL, rr.MAX_CELLS)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvface.h")).read()
    for name, value in (("PVF_PRIM_REDACT", "3"), ("PVF_REDACT_ELLIPSE", "1"), ("PVF_REDACT_MOSAIC", "0"), ("PVF_REDACT_SMOOTH", "2"), ("PVF_REDACT_FILL", "4"),
                        ("PVF_REDACT_MAX_SIDE", "16384"), ("PVF_REDACT_MAX_CELL", "2048"), ("PVF_REDACT_MAX_CELLS", "4096")):
        assert "#define %s %s" % (name, value) in hdr, name


def test_mosaic_cells_show_one_value_and_a_changed_pixel_stays_in_its_cell():
    src = _src()
    ow, oh = 385, 97
    p = _p(30, 10, 30 + 16 * 5 - 1, 10 + 16 * 4 - 1, 16, MOSAIC)                # 5 x 4 cells of 256 pixels
    one = rr.render_rgb(src, ow, oh, [p])
    for j in range(4):
        for i in range(5):
            block = one[10 + 16 * j:26 + 16 * j, 30 + 16 * i:46 + 16 * i].reshape(-1, 3)
            assert (block == block[0]).all()
            assert np.array_equal(block[0], rr.cell_means(src, ow, oh, [p])[j * 5 + i])
    big = _p(30, 10, 30 + 17 * 5 - 1, 10 + 17 * 4 - 1, 17, MOSAIC)              # 289 > 255 pixels a cell: one pixel moves a mean by 1 at most
    base = rr.render_rgb(src, ow, oh, [big]).astype(int)
    other = src.copy()
    other[10 + 17 * 2 + 3, 30 + 17 * 3 + 5] ^= 255                              # inside cell (3, 2)
    changed = rr.render_rgb(other, ow, oh, [big]).astype(int)
    diff = np.abs(changed - base)
    assert diff.max() <= 1
    ys, xs = np.nonzero(diff.any(2))
    assert len(ys) == 0 or (ys.min() >= 10 + 34 and ys.max() < 10 + 51 and xs.min() >= 30 + 51 and xs.max() < 30 + 68)
    small = rr.render_rgb(other, ow, oh, [p]).astype(int) - one.astype(int)      # 256 pixels a cell: still one cell, by more than 1 perhaps
    ys, xs = np.nonzero(small.any(2))
    assert len(ys) and ys.min() >= 10 + 32 and ys.max() < 10 + 48 and xs.min() >= 30 + 48 and xs.max() < 30 + 64


@pytest.mark.parametrize("shape", [0, ELLIPSE])
def test_fill_shows_nothing_of_the_source_and_uncovered_pixels_are_untouched(shape):
    a, b = _src("noise", seed=1), _src("noise", seed=2)
    ow, oh = 201, 51
    others = [(demo_ref.RECT, 20, 10, 90, 40, (0, 255, 0)), (demo_ref.TEXT, 5, 48, (255, 255, 255), 1, b"under")]
    p = _p(-5, 8, 120, 45, 7, FILL | shape)
    ra, rb = rr.render_rgb(a, ow, oh, others + [p]), rr.render_rgb(b, ow, oh, others + [p])
    xa, ya, mask = rr.covered(p, ow, oh)
    full = np.zeros((oh, ow), bool)
    full[ya:ya + mask.shape[0], xa:xa + mask.shape[1]] = mask
    assert full.sum() > 1000 and (shape == 0) == bool(mask.all())
    assert np.array_equal(ra[full], rb[full]) and (ra[full] == K).all()
    for mode in (MOSAIC, SMOOTH, FILL):
        q = _p(-5, 8, 120, 45, 7, mode | shape)
        got = rr.render_rgb(a, ow, oh, others + [q])
        assert np.array_equal(got[~full], demo_ref.render_rgb(a, ow, oh, others)[~full])


def test_cell_one_is_the_identity_and_order_matters():
    src = _src()
    q = _p(10, 10, 60, 60, 1, MOSAIC)
    assert np.array_equal(rr.render_rgb(src, 385, 97, [q]), src)
    assert np.array_equal(rr.render_rgb(src, 201, 51, [q]), demo_ref.resize(src, 201, 51))
    rect = (demo_ref.RECT, 20, 20, 50, 50, (255, 0, 255))
    over = rr.render_rgb(src, 385, 97, [rect, q])          # the redaction is made from the source: it wipes the rectangle
    assert np.array_equal(over, src)
    under = rr.render_rgb(src, 385, 97, [q, rect])
    assert np.array_equal(under, demo_ref.render_rgb(src, 385, 97, [rect]))
    two = rr.render_rgb(src, 385, 97, [_p(0, 0, 99, 96, 50, MOSAIC), _p(50, 0, 149, 96, 100, MOSAIC)])
    alone = rr.render_rgb(src, 385, 97, [_p(50, 0, 149, 96, 100, MOSAIC)])
    assert np.array_equal(two[:, 50:150], alone[:, 50:150])                      # never made from an earlier redaction


def test_smooth_of_a_constant_and_the_widest_product():
    for v in (0, 1, 128, 254, 255):
        src = np.full((40, 60, 3), v, np.uint8)
        for cell in (1, 2, 3, 7, 64):
            out = rr.render_rgb(src, 60, 40, [_p(-4, 5, 70, 33, cell, SMOOTH | ELLIPSE)])
            assert (out == v).all(), (v, cell)
    white = np.full((5, 2060, 3), 255, np.uint8)
    out = rr.render_rgb(white, 2060, 5, [_p(3, 1, 3 + 2048, 3, 2048, SMOOTH)])    # 2049 x 3 at cell = 2048
    assert (out == 255).all()
    assert 255 * 4 * 2048 * 2048 + 2 * 2048 * 2048 == 4286578688 < 2 ** 32
    ramp = dc.frame("ramp_x", 20, 100)
    out = rr.render_rgb(ramp, 100, 20, [_p(0, 0, 99, 19, 10, SMOOTH)]).astype(int)
    assert (np.diff(out[5, :, 0]) >= 0).all() and len(set(out[5, :, 0])) > 20     # blended, not stepped
    mosaic = rr.render_rgb(ramp, 100, 20, [_p(0, 0, 99, 19, 10, MOSAIC)])
    assert len(set(mosaic[5, :, 0])) == 10


def test_smooth_across_a_frame_edge_uses_only_cells_with_pixels():
    src = _src("noise", seed=3)
    p = _p(-36, -20, 50, 30, 16, SMOOTH)
    means = rr.cell_means(src, 385, 97, [p]).reshape(4, 6, 3)
    resized = demo_ref.resize(src, 385, 97)
    assert (means[0] == 0).all() and (means[:, :2] == 0).all()                   # cells wholly outside read 0 ...
    out = rr.render_rgb(src, 385, 97, [p])
    # ... and are never shown: cell (2, 1) holds the frame's pixels 0 .. 11 x 0 .. 11, its centre lies at 3.5; the pixels before it would
    # blend with a cell outside the frame, the clamp puts both neighbours onto the cell itself
    for y, x in ((0, 0), (3, 3), (0, 3)):
        assert np.array_equal(out[y, x], means[1, 2])
    n = 12 * 12
    assert np.array_equal(means[1, 2], (resized[0:12, 0:12].astype(int).sum((0, 1)) + n // 2) // n)


def test_the_ellipse_of_a_one_wide_box_is_the_whole_column():
    for p in (_p(5, 2, 5, 30, 4, FILL | ELLIPSE), _p(2, 5, 30, 5, 4, FILL | ELLIPSE), _p(7, 7, 7, 7, 1, FILL | ELLIPSE)):
        assert rr.covered(p, 40, 40)[2].all()
    _, _, m = rr.covered(_p(0, 0, 20, 10, 4, ELLIPSE), 40, 40)
    assert not m[0, 0] and m[5, 0] and m[0, 10] and m[5, 10] and not m[10, 20]
    assert np.array_equal(m, m[::-1]) and np.array_equal(m, m[:, ::-1])
    assert rr.covered(_p(10, 10, 9, 20, 4, 0), 40, 40) is None                   # inverted
    assert rr.covered(_p(40, 0, 50, 10, 4, 0), 40, 40) is None                   # off the frame


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
ROWS = [(0.00, 0, (0.10, 0.20, 0.30, 0.60), "detection"), (0.00, 1, (0.50, 0.10, 0.70, 0.50), "detection"),
        (0.04, 0, (0.11, 0.20, 0.31, 0.60), "forward"), (0.04, 1, (0.51, 0.10, 0.71, 0.50), "forward"), (0.04, 2, (0.80, 0.60, 0.95, 0.90), "detection"),
        (0.08, 0, (0.12, 0.20, 0.32, 0.60), "forward"), (0.08, 2, (0.80, 0.60, 0.95, 0.90), "forward")]
ROWS = [(T, i, tuple(np.float32(v) for v in box), s) for T, i, box, s in ROWS]
LABELS = {0: "anna", 1: "bob"}                                                   # track 2 has no label


def _ids(plan):
    return [[p[1:5] for p in prims] for _, _, prims in plan]


def _who(plan, k=1):
    by_box = {render.redaction_box(render_box, 25): ident for T, ident, render_box in
              ((T, i, tuple(int(float(c) * s) for c, s in zip(box, (200, 100, 200, 100)))) for T, i, box, _ in ROWS)}
    return sorted(by_box[p[1:5]] for p in plan[k][2])


@pytest.mark.parametrize("options, want", [({}, [0, 1, 2]), ({"only": {"anna"}}, [0]), ({"only": {"anna", "bob"}}, [0, 1]), ({"only": {"carl"}}, []),
                                           ({"keep": {"anna"}}, [1, 2]), ({"keep": {"anna", "bob"}}, [2]), ({"keep": set()}, [0, 1, 2])])
def test_selection_table(options, want):
    labels = LABELS if options else None
    plan = render.build_redaction_plan(ROWS, 25.0, 3, 200, 100, labels, **options)
    assert _who(plan) == want
    assert plan == rr.plan(ROWS, 25.0, 3, 200, 100, labels, **options)


def test_selection_refusals():
    with pytest.raises(ValueError):
        render.build_redaction_plan(ROWS, 25.0, 3, 200, 100, LABELS, only={"anna"}, keep={"bob"})
    with pytest.raises(ValueError):
        render.build_redaction_plan(ROWS, 25.0, 3, 200, 100, None, only={"anna"})
    with pytest.raises(ValueError):
        render.build_redaction_plan(ROWS, 25.0, 3, 200, 100, None, keep={"anna"})
    with pytest.raises(ValueError):
        render.build_redaction_plan(ROWS, 25.0, 3, 200, 100, mode="blur")
    with pytest.raises(ValueError):
        render.build_redaction_plan(ROWS, 25.0, 3, 200, 100, shape="star")


def test_the_last_times_faces_are_in_the_plan_and_demo_still_drops_them():
    plan = render.build_redaction_plan(ROWS, 25.0, 3, 200, 100)
    assert [len(prims) for _, _, prims in plan] == [2, 3, 2]
    drawn = render.build_plan(ROWS, 25.0, 3, 200, 100)
    assert [sum(1 for p in prims if p[0] == render.PRIM_RECT) for _, _, prims in drawn] == [2, 3, 0]
    for kw in ({}, {"shift": 0.04}, {"t_from": 0.04}, {"t_until": 0.08}, {"pad": 0, "cells": 3, "shape": "box", "mode": "fill", "colour": (1, 2, 3)}):
        assert render.build_redaction_plan(ROWS, 25.0, 3, 200, 100, **kw) == rr.plan(ROWS, 25.0, 3, 200, 100, **kw), kw
    shifted = render.build_redaction_plan(ROWS, 25.0, 3, 200, 100, shift=0.04)
    assert [len(prims) for _, _, prims in shifted] == [0, 2, 3]
    assert plan[0][2][0] == (REDACT, 10, 10, 70, 70, (0, 0, 0), 8, ELLIPSE)      # box (20, 20, 60, 60): 25 % of 40 = 10 a side; 61 / 8 -> 8


def test_padding_and_cell_rules_on_hand_computed_boxes():
    assert render.redaction_box((100, 50, 200, 90), 25) == (75, 40, 225, 100)     # 100 * 25 = 2500 -> 25; 40 * 25 = 1000 -> 10
    assert render.redaction_box((100, 50, 201, 91), 25) == (75, 40, 226, 101)     # 101 * 25 + 50 = 2575 -> 25; 41 * 25 + 50 = 1075 -> 10
    assert render.redaction_box((100, 50, 202, 92), 25) == (74, 39, 228, 103)     # 102 * 25 + 50 = 2600 -> 26; 42 * 25 + 50 = 1100 -> 11
    assert render.redaction_box((0, 0, 10, 10), 0) == (0, 0, 10, 10)
    assert render.redaction_box((0, 0, 1, 1), 50) == (-1, -1, 2, 2)               # 50 + 50 = 100 -> 1
    assert render.redaction_box((10, 10, 5, 5), 25) == (11, 11, 4, 4)             # an inverted box stays inverted: (-5 * 25 + 50) // 100 = -1
    assert render.redaction_cell((0, 0, 79, 39), 8) == 10
    assert render.redaction_cell((0, 0, 80, 39), 8) == 11                         # 81 / 8 -> 11
    assert render.redaction_cell((0, 0, 39, 80), 8) == 11
    assert render.redaction_cell((0, 0, 3, 3), 8) == 1
    assert render.redaction_cell((5, 5, 4, 4), 8) == 1
    assert render.redaction_cell((0, 0, 16383, 16383), 1) == 2048                 # the cap on the cell side: 8 x 8 cells
    assert render.redaction_cell((0, 0, 999, 999), 100) == 16                     # 10 would be 100 x 100 cells: raised until ceil(1000 / c)^2 <= 4096
    assert (-(-1000 // 16)) ** 2 <= 4096 < (-(-1000 // 15)) ** 2
    for box, cells in (((0, 0, 79, 39), 8), ((0, 0, 999, 999), 100), ((0, 0, 16383, 16383), 1), ((5, 5, 4, 4), 8)):
        assert render.redaction_cell(box, cells) == rr.cell_side(box, cells)
        assert render.redaction_box(box, 25) == rr.pad_box(box, 25)


# ---- packing and its limits -----------------------------------------------------------------------------------------------------------
def test_pack_round_trip():
    lists = [[_p(-7, 3, 90, 44, 5, SMOOTH | ELLIPSE, (1, 2, 3)), (demo_ref.RECT, 1, 2, 3, 4, (9, 9, 9))], [], [_p(0, 0, 9, 9, 2048, FILL, (255, 254, 253))]]
    start, prims, text = render.pack_primitives(lists)
    assert start.tolist() == [0, 2, 2, 3] and prims.shape == (3, 8) and prims.dtype == np.int32 and len(text) == 0
    assert prims[0].tolist() == [3, -7, 3, 90, 44, 1 | 2 << 8 | 3 << 16 | (SMOOTH | ELLIPSE) << 24, 5, 0]
    assert prims[1].tolist() == [0, 1, 2, 3, 4, 9 | 9 << 8 | 9 << 16, 0, 0]
    assert prims[2].tolist() == [3, 0, 0, 9, 9, 255 | 254 << 8 | 253 << 16 | FILL << 24, 2048, 0]
    back = [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), (r[5] & 255, (r[5] >> 8) & 255, (r[5] >> 16) & 255), int(r[6]), int(r[5]) >> 24) for r in prims[[0, 2]]]
    assert back == [lists[0][0], lists[2][0]]
    assert render.redaction_cells(lists[0][0]) == 20 * 9 and render.redaction_cells(lists[2][0]) == 0
    assert render.redaction_cells(_p(5, 5, 4, 9, 1, MOSAIC)) == 0


@pytest.mark.parametrize("prim, message", [
    (_p(-(1 << 20) - 1, 0, 5, 5, 2, MOSAIC), "coordinate"), (_p(0, 0, 5, (1 << 20) + 1, 2, MOSAIC), "coordinate"),
    (_p(0, 0, 16384, 5, 2048, MOSAIC), "side"), (_p(0, 0, 5, 16384, 2048, FILL), "side"),
    (_p(0, 0, 5, 5, 0, MOSAIC), "cell"), (_p(0, 0, 5, 5, 2049, MOSAIC), "cell"),
    (_p(0, 0, 64, 63, 1, MOSAIC), "cells"), (_p(0, 0, 5, 5, 2, 8), "flags"), (_p(0, 0, 5, 5, 2, 6), "flags")])
def test_pack_refuses_each_limit(prim, message):
    with pytest.raises(ValueError, match=message):
        render.pack_primitives([[prim]])


def test_pack_accepts_the_limits_themselves():
    at = [_p(-(1 << 20), -(1 << 20), -(1 << 20) + 16383, -(1 << 20) + 16383, 2048, MOSAIC), _p((1 << 20) - 63, 0, 1 << 20, 63, 1, SMOOTH),
          _p(0, 0, 16383, 16383, 256, FILL | ELLIPSE), _p(9, 9, -(1 << 20), -(1 << 20), 1, MOSAIC)]
    _, prims, _ = render.pack_primitives([at])
    assert len(prims) == 4
    with pytest.raises(ValueError, match="in one call"):
        render.pack_primitives([[_p(0, 0, 63, 63, 1, MOSAIC)] * 1024] * 2)          # 2 * 1024 * 4096 cells


# ---- the parser -----------------------------------------------------------------------------------------------------------------------
def test_parser_accepts_redact_and_refuses_only_with_keep():
    a = cli.parse_args(["redact", "v.y4m", "t.txt", "-"])
    assert (a.verb, a.height, a.pad, a.cells, a.shape, a.mode, a.colour, a.draw, a.only, a.keep, a.label) == ("redact", 0, 25, 8, "ellipse", "mosaic", (0, 0, 0), False, None, None, None)
    a = cli.parse_args(["redact", "--height", "200", "--from", "1", "--until", "2", "--shift", "0.5", "--label", "l.txt", "--only", "anna,bob", "--pad", "10", "--cells", "4",
                        "--shape", "box", "--mode", "fill", "--colour", "1,2,3", "--draw", "v.y4m", "t.txt", "o.y4m"])
    assert (a.height, a.t_from, a.t_until, a.shift, a.label, a.only, a.pad, a.cells, a.shape, a.mode, a.colour, a.draw) == (200, 1.0, 2.0, 0.5, "l.txt", {"anna", "bob"}, 10, 4, "box", "fill", (1, 2, 3), True)
    assert cli.parse_args(["redact", "--label", "l", "--keep", "anna", "v", "t", "o"]).keep == {"anna"}
    for bad in (["--only", "a", "--keep", "b"], ["--mode", "blur"], ["--shape", "star"], ["--colour", "1,2"], ["--colour", "1,2,300"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["redact"] + bad + ["v", "t", "o"])
    with pytest.raises(SystemExit):                                               # a selection without labels: refused before anything is opened
        cli.main(["redact", "--only", "anna", "v.y4m", "t.txt", "o.y4m"])
