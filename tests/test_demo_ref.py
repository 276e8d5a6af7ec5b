"""CPU: the semantics of the `demo` verb (DEMO.md) as tests/demo_ref.py restates them -- font, rectangle, line, draw order, colour
conversion -- and the host side of the package against them: the font and palette tables, the plan builder against a transcription of
the reference generators' pacing, the Y4M writer against the project's own reader, the command line."""
import os
import re
import numpy as np
import pytest

from tests import demo_ref
from tests import yuv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [("601", False), ("601", True), ("709", False), ("709", True)]


def rows_of(ch):
    return ["".join("#" if (r >> (4 - c)) & 1 else "." for c in range(5)) for r in demo_ref.FONT[ord(ch) - 32]]


# ---- font --------------------------------------------------------------------------------------------------------------------------
def test_font_glyphs_distinct_and_non_empty():
    assert len(demo_ref.FONT) == 95
    assert len(set(demo_ref.FONT)) == 95
    for i, g in enumerate(demo_ref.FONT):
        assert len(g) == 7 and all(0 <= r < 32 for r in g)
        assert (sum(g) == 0) == (i == 0), chr(32 + i)


def test_font_pinned_glyphs():
    assert rows_of("0") == [".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."]
    assert rows_of("1") == ["..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."]
    assert rows_of("#") == [".#.#.", ".#.#.", "#####", ".#.#.", "#####", ".#.#.", ".#.#."]
    assert rows_of(".") == [".....", ".....", ".....", ".....", ".....", ".##..", ".##.."]
    assert rows_of("A") == [".###.", "#...#", "#...#", "#####", "#...#", "#...#", "#...#"]


def test_package_tables_equal_the_restatement():
    from pyannote_video_amd import render
    assert [tuple(g) for g in render.FONT] == [tuple(g) for g in demo_ref.FONT]
    assert [tuple(c) for c in render.PALETTE] == [tuple(c) for c in demo_ref.PALETTE]
    assert len(set(map(tuple, demo_ref.PALETTE))) == 26
    assert {k: (v[0], tuple(v[1]), tuple(v[2]), tuple(v[3])) for k, v in render.YUV_TABLES.items()} == demo_ref.TABLES
    assert render.glyph(7) == render.glyph(200) == render.glyph(ord("?"))
    assert (render.PRIM_RECT, render.PRIM_LINE, render.PRIM_TEXT) == (demo_ref.RECT, demo_ref.LINE, demo_ref.TEXT)


def test_kernel_font_table_equals_the_package():
    """csrc/render_font.h is the table render_k reads"""
    src = open(os.path.join(ROOT, "pyannote-video_amd", "csrc", "render_font.h")).read()
    body = src[src.index("render_font[95][7]"):]
    vals = [int(v, 16) for v in re.findall(r"0x([0-9A-Fa-f]{2})", body)]
    assert len(vals) == 95 * 7
    assert [tuple(vals[7 * i:7 * i + 7]) for i in range(95)] == [tuple(g) for g in demo_ref.FONT]


def test_text_blocks_scale_and_origin():
    img = np.zeros((40, 60, 3), np.uint8)
    demo_ref.draw_text(img, 3, 30, (9, 8, 7), 2, b"1")
    on = np.argwhere(img[..., 0] == 9)
    assert on[:, 0].max() == 30 and on[:, 0].min() == 30 - 14 + 1        # the 5 x 7 box sits on row y, 7 * scale rows high
    assert on[:, 1].min() == 3 + 2 and on[:, 1].max() == 3 + 4 * 2 - 1   # '1' uses columns 1 .. 3
    assert len(on) == 4 * sum(bin(r).count("1") for r in demo_ref.FONT[ord("1") - 32])
    a, b = np.zeros((20, 40, 3), np.uint8), np.zeros((20, 40, 3), np.uint8)
    demo_ref.draw_text(a, 0, 10, (1, 1, 1), 1, bytes([7, 200]))
    demo_ref.draw_text(b, 0, 10, (1, 1, 1), 1, b"??")
    assert np.array_equal(a, b) and a.any()
    c = np.zeros((20, 800, 3), np.uint8)
    demo_ref.draw(c, [(demo_ref.TEXT, 0, 10, (1, 1, 1), 1, b"#" * 100)])
    assert c[:, :64 * 6].any() and not c[:, 64 * 6:].any()             # a run is cut at 64 bytes


# ---- rectangle ---------------------------------------------------------------------------------------------------------------------
def test_rectangle_pixel_counts():
    W, H = 40, 30
    count = lambda *box: len(demo_ref.rect_pixels(*box, W, H))
    assert count(10, 10, 20, 20) == 13 * 13 - 9 * 9               # outer 9 .. 21, inner 11 .. 19
    assert count(10, 10, 11, 11) == 16                            # inner is empty: a filled 4 x 4 blob
    assert count(10, 10, 10, 10) == 9                             # a point: 3 x 3
    assert count(10, 10, 8, 20) == 13                             # inverted by two: the outer box is the column x = 9, y 9 .. 21
    assert count(10, 10, 7, 20) == 0                              # inverted by three: the outer box is empty
    assert count(12, 10, 10, 20) == 13                            # outer x 11 .. 11; the inner box is empty
    assert count(100, 100, 120, 120) == 0                         # wholly outside
    assert count(-50, -50, -10, -10) == 0
    assert count(-5, -5, 100, 100) == 0                           # dwarfs the frame: the outline lies outside
    img = np.zeros((H, W, 3), np.uint8)
    demo_ref.draw_rect(img, 10, 10, 20, 20, (5, 6, 7))
    assert set(map(tuple, np.argwhere(img[..., 0] == 5)[:, ::-1])) == demo_ref.rect_pixels(10, 10, 20, 20, W, H)


def test_rectangle_touching_each_border():
    W, H = 40, 30
    for box, edge in (((0, 5, 10, 15), "left"), ((5, 0, 15, 10), "top"), ((29, 5, 39, 15), "right"), ((5, 19, 15, 29), "bottom")):
        px = demo_ref.rect_pixels(*box, W, H)
        full = 13 * 13 - 9 * 9
        lost = 13                                                 # the outer row / column that falls off the frame
        assert len(px) == full - lost, edge
        assert all(0 <= x < W and 0 <= y < H for x, y in px)
        img = np.zeros((H, W, 3), np.uint8)
        demo_ref.draw_rect(img, *box, (1, 2, 3))
        assert int((img[..., 0] == 1).sum()) == full - lost


# ---- line --------------------------------------------------------------------------------------------------------------------------
LINES = [(3, 4, 17, 4), (17, 4, 3, 4), (5, 2, 5, 19), (2, 2, 12, 12), (12, 2, 2, 12), (0, 0, 19, 7), (19, 7, 0, 0), (3, 18, 9, 1),
         (6, 6, 6, 6), (1, 1, 18, 2), (4, 0, 5, 19), (0, 0, 10, 5), (0, 0, 4, 2), (10, 3, 0, 8)]


@pytest.mark.parametrize("line", LINES)
def test_line_endpoints_count_and_reversal(line):
    x1, y1, x2, y2 = line
    px = demo_ref.line_pixels(x1, y1, x2, y2)
    D = max(abs(x2 - x1), abs(y2 - y1))
    assert len(px) == D + 1 and len(set(px)) == D + 1
    assert px[0] == (x1, y1) and px[-1] == (x2, y2)
    for (xa, ya), (xb, yb) in zip(px, px[1:]):
        assert max(abs(xb - xa), abs(yb - ya)) == 1               # connected, one pixel per major step
    # drawn from the other end: the same set, except that an exact half step goes to the other side (ties round towards the END point)
    back = demo_ref.line_pixels(x2, y2, x1, y1)
    assert set(back) == set(demo_ref.line_pixels(x1, y1, x2, y2, ties_down=True))
    d = min(abs(x2 - x1), abs(y2 - y1))
    has_tie = any((2 * k * d) % (2 * D) == D for k in range(D + 1)) if D else False
    assert (set(back) == set(px)) == (not has_tie)


def test_line_shapes():
    assert demo_ref.line_pixels(3, 4, 6, 4) == [(3, 4), (4, 4), (5, 4), (6, 4)]
    assert demo_ref.line_pixels(5, 2, 5, 4) == [(5, 2), (5, 3), (5, 4)]
    assert demo_ref.line_pixels(2, 2, 4, 4) == [(2, 2), (3, 3), (4, 4)]
    assert demo_ref.line_pixels(4, 2, 2, 4) == [(4, 2), (3, 3), (2, 4)]              # a tie of the deltas: x is the major axis
    assert demo_ref.line_pixels(6, 6, 6, 6) == [(6, 6)]
    assert demo_ref.line_pixels(0, 0, 4, 2) == [(0, 0), (1, 1), (2, 1), (3, 2), (4, 2)]      # half steps round up
    assert demo_ref.line_pixels(0, 0, 4, 2, ties_down=True) == [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2)]


def test_line_clipping_and_far_endpoints():
    W, H = 20, 10
    whole = demo_ref.line_pixels(-30, -7, 45, 16)
    assert demo_ref.line_pixels(-30, -7, 45, 16, W, H) == [p for p in whole if 0 <= p[0] < W and 0 <= p[1] < H]
    far = demo_ref.line_pixels(-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, W, H)
    assert far == [(i, i) for i in range(H)]
    far = demo_ref.line_pixels(-2 ** 31, 5, 2 ** 31 - 1, 6, W, H)             # 2 k d passes 2^32; the half step lies at x = -0.5
    assert far == [(x, 6) for x in range(W)]
    assert demo_ref.line_pixels(100, 100, 200, 300, W, H) == []


# ---- order -------------------------------------------------------------------------------------------------------------------------
def test_later_primitives_win():
    a = (demo_ref.RECT, 2, 2, 12, 12, (10, 0, 0))
    b = (demo_ref.LINE, 0, 2, 19, 2, (0, 20, 0))
    c = (demo_ref.TEXT, 1, 9, (0, 0, 30), 1, b"#")
    x = demo_ref.draw(np.zeros((16, 20, 3), np.uint8), [a, b, c])
    y = demo_ref.draw(np.zeros((16, 20, 3), np.uint8), [c, b, a])
    assert tuple(x[2, 5]) == (0, 20, 0) and tuple(y[2, 5]) == (10, 0, 0)
    assert tuple(x[3, 2]) == (0, 0, 30) and tuple(y[3, 2]) == (10, 0, 0)        # '#' row 0 at y = 3: columns 1 and 3 -> x = 2 and 4
    assert not np.array_equal(x, y)


# ---- colour ------------------------------------------------------------------------------------------------------------------------
def _colours():
    rng = np.random.RandomState(1)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)])
    return np.concatenate([rng.randint(0, 256, (200000, 3)), corners])


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_tables_follow_the_rule(matrix, full):
    yoff, y, u, v = demo_ref.derive_table(matrix, full)
    assert (yoff, tuple(y), tuple(u), tuple(v)) == demo_ref.TABLES[(matrix, full)]
    assert sum(u) == 0 and sum(v) == 0


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_colour_range_and_greys(matrix, full):
    yoff, yc, uc, vc = demo_ref.TABLES[(matrix, full)]
    c = _colours().astype(np.int64)
    Y = (c @ np.array(yc) + (yoff << 16) + 32768) >> 16
    U = (4 * (c @ np.array(uc)) + (128 << 18) + (1 << 17)) >> 18
    V = (4 * (c @ np.array(vc)) + (128 << 18) + (1 << 17)) >> 18
    if full:
        # full range: Y covers 0 .. 255; the positive chroma extreme (pure blue / pure red) comes out at 256 and NEEDS the clamp
        assert (Y.min(), Y.max()) == (0, 255) and (U.min(), U.max()) == (1, 256) and (V.min(), V.max()) == (1, 256)
    else:
        assert (Y.min(), Y.max()) == (16, 235) and (U.min(), U.max()) == (16, 240) and (V.min(), V.max()) == (16, 240)
    for g in range(256):
        y, u, v = demo_ref.unclamped_yuv((g, g, g), matrix, full)
        assert u == 128 and v == 128
    y, u, v = demo_ref.to_yuv420(np.full((3, 5, 3), 255, np.uint8), matrix, full)
    assert y.shape == (3, 5) and u.shape == v.shape == (2, 3)
    assert set(y.ravel()) == {255 if full else 235} and set(u.ravel()) == {128} and set(v.ravel()) == {128}


# measured here over the 200 008 colours of _colours(), constant-colour frames, back through tests/yuv_ref.py
ROUND_TRIP = {("601", False): (1, 1, 2), ("709", False): (1, 1, 2), ("601", True): (1, 1, 1), ("709", True): (1, 1, 1)}


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_round_trip_through_the_ingest_conversion(matrix, full):
    c = _colours()
    rows = np.repeat(np.repeat(c[:, None, :], 2, 0), 2, 1).astype(np.uint8)           # [2 N, 2, 3]: every 2 x 2 block holds one colour
    Y, U, V = demo_ref.to_yuv420(rows, matrix, full)
    back = yuv_ref.to_rgb(Y, U, V, "420", matrix, full).astype(np.int64)
    worst = np.abs(back - rows.astype(np.int64)).reshape(-1, 3).max(0)
    print("round trip", matrix, "full" if full else "limited", worst)
    assert all(w <= b for w, b in zip(worst, ROUND_TRIP[(matrix, full)]))


def test_odd_sizes_replicate_the_last_column_and_row():
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (5, 7, 3)).astype(np.uint8)
    padded = np.pad(img, ((0, 1), (0, 1), (0, 0)), mode="edge")
    y0, u0, v0 = demo_ref.to_yuv420(img)
    y1, u1, v1 = demo_ref.to_yuv420(padded)
    assert np.array_equal(y0, y1[:5, :7]) and np.array_equal(u0, u1) and np.array_equal(v0, v1)


# ---- resize ------------------------------------------------------------------------------------------------------------------------
def test_resize_equals_the_oracle(oracle):
    rng = np.random.RandomState(5)
    for (h, w), (oh, ow) in (((97, 385), (40, 158)), ((1080 // 4, 1920 // 4), (100, 177)), ((41, 39), (82, 78)), ((50, 60), (50, 60)),
                             ((7, 5), (2, 2)), ((33, 47), (45, 71))):
        img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        assert np.array_equal(demo_ref.resize(img, ow, oh), oracle.cv_resize(img, ow, oh)), ((h, w), (oh, ow))


# ---- plan --------------------------------------------------------------------------------------------------------------------------
TRACK = """0.000 0 0.100 0.100 0.300 0.400 detection
0.040 0 0.110 0.100 0.310 0.400 forward
0.040 1 0.500 0.200 0.700 0.600 detection
0.120 1 0.510 0.200 0.710 0.600 forward
0.120 0 0.120 0.100 0.320 0.400 forward
0.200 27 0.175 0.250 0.425 0.750 backward
0.440 3 0.000 0.000 1.000 1.000 detection
"""


def _landmarks(path, rows):
    rng = np.random.RandomState(11)
    with open(path, "w") as f:
        for T, ident in rows:
            f.write("%.3f %d" % (T, ident) + "".join(" %.5f" % v for v in rng.uniform(0.05, 0.95, 136)) + "\n")


def _plan_files(tmp_path):
    track = tmp_path / "track.txt"
    track.write_text(TRACK)
    marks = tmp_path / "landmarks.txt"
    # the faces of 0.040 and 0.120 in the OTHER order than the track file's; 0.200 has none; 0.440 is the last group
    _landmarks(str(marks), [(0.0, 0), (0.04, 1), (0.04, 0), (0.12, 0), (0.12, 1), (0.44, 3)])
    return str(track), str(marks)


def _same_plan(a, b):
    assert len(a) == len(b)
    for (ia, ta, pa), (ib, tb, pb) in zip(a, b):
        assert ia == ib and ta == tb
        assert [tuple(tuple(v) if isinstance(v, (list, tuple)) else v for v in p) for p in pa] == \
               [tuple(tuple(v) if isinstance(v, (list, tuple)) else v for v in p) for p in pb]


# shift 1.0: no frame reaches the first group, which blocks every group behind it; shift 0.41: the last frame is sent 0.110, so the
# groups of 0.120 and 0.200 stay ahead of every frame; until 0.1: the frames end before the later groups; shift -1.0: every group is overdue at once
@pytest.mark.parametrize("kw", [{}, {"shift": 0.08}, {"shift": -0.05}, {"t_from": 0.08}, {"t_until": 0.3}, {"t_from": 0.1, "t_until": 0.41, "shift": 0.04},
                                {"shift": 1.0}, {"shift": 0.41}, {"t_until": 0.1}, {"shift": -1.0}, {"t_from": 0.3, "shift": 0.3}])
def test_plan_builder_against_the_generators(tmp_path, kw):
    from pyannote_video_amd import render, formats
    track, marks = _plan_files(tmp_path)
    labels = {0: "anna", 27: "x" * 80}
    for with_marks in (False, True):
        got = render.build_plan(formats.read_tracks(track), 25.0, 14, 355, 200, formats.read_landmarks(marks) if with_marks else None, labels, **kw)
        want = demo_ref.plan(demo_ref.read_track_file(track), 25.0, 14, 355, 200, demo_ref.read_landmark_file(marks) if with_marks else None,
                             labels, **kw)
        _same_plan(got, want)


def _package_plan(track, marks, labels=None, **kw):
    """render.build_plan's output in the restatement's vocabulary (tuples; the primitive codes are asserted equal elsewhere)"""
    from pyannote_video_amd import render, formats
    plan = render.build_plan(formats.read_tracks(track), 25.0, 14, 400, 200, formats.read_landmarks(marks) if marks else None, labels, **kw)
    return [(i, t, [tuple(tuple(v) if isinstance(v, (list, tuple)) else v for v in p) for p in prims]) for i, t, prims in plan]


def _restated_plan(track, marks, labels=None, **kw):
    return demo_ref.plan(demo_ref.read_track_file(track), 25.0, 14, 400, 200, demo_ref.read_landmark_file(marks) if marks else None, labels, **kw)


@pytest.mark.parametrize("make", [_package_plan, _restated_plan], ids=["render.build_plan", "demo_ref.plan"])
def test_plan_pacing_by_hand(tmp_path, make):
    """the same hand-made expectations for the package's plan builder and for the restatement"""
    track, marks = _plan_files(tmp_path)
    plan = make(track, marks, {1: "bob"})
    assert [i for i, _, _ in plan] == list(range(14))
    rects = [[p for p in prims if p[0] == demo_ref.RECT] for _, _, prims in plan]
    # one group per frame at most, a group waiting for its time; 0.040 is shown on frame 1, 0.120 on frame 3, 0.200 on frame 5; the
    # group of 0.440 is the last and never shown, although frames 11 .. 13 reach it
    assert [len(r) for r in rects] == [1, 2, 0, 2, 0, 1] + [0] * 8
    assert rects[5][0][1:5] == (int(float(np.float32(0.175)) * 400), 50, int(float(np.float32(0.425)) * 400), 150)
    assert rects[5][0][5] == tuple(demo_ref.PALETTE[27 % 26])
    for _, t, prims in plan:
        assert prims[0] == (demo_ref.TEXT, 10, 190, (255, 0, 0), 1, ("%.3f" % t).encode())
    # landmarks pair with faces by identifier: on frame 1 the file lists track 1 before track 0, the track file 0 before 1
    lines = [p for p in plan[1][2] if p[0] == demo_ref.LINE]
    order = [p[5] for p in plan[1][2] if p[0] == demo_ref.RECT]
    assert [l[5] for l in lines] == order == [tuple(demo_ref.PALETTE[0]), tuple(demo_ref.PALETTE[1])]
    rows = {(T, i): p for T, i, p in demo_ref.read_landmark_file(marks)}
    p = rows[(0.04, 1)]
    assert lines[1][1:5] == tuple(int(v) for v in (np.round(p[27, 0] * np.float32(400)), np.round(p[27, 1] * np.float32(200)),
                                                   np.round(p[33, 0] * np.float32(400)), np.round(p[33, 1] * np.float32(200))))
    assert [p for p in plan[5][2] if p[0] == demo_ref.LINE] == []                 # no landmark row for the face of 0.200
    labels = [p for _, _, prims in plan for p in prims if p[0] == demo_ref.TEXT and p[5] == b"bob"]
    assert len(labels) == 2 and labels[0][1:3] == (int(float(np.float32(0.5)) * 400), int(float(np.float32(0.2)) * 200) - 7)
    # a shift so large that no frame reaches the first group
    late = make(track, None, shift=1.0)
    assert len(late) == 14 and all(len(prims) == 1 and prims[0][0] == demo_ref.TEXT for _, _, prims in late)
    # a shift of 0.41: frames 11, 12 and 13 are sent 0.030, 0.070 and 0.110 and show the groups of 0.000 and 0.040; the group of 0.120 is
    # ahead of the last frame and blocks the group of 0.200 behind it
    part = make(track, None, shift=0.41)
    assert [sum(p[0] == demo_ref.RECT for p in prims) for _, _, prims in part] == [0] * 11 + [1, 2, 0]
    # overdue groups come out one per frame, oldest first, never two on one frame
    rush = make(track, None, shift=-1.0)
    assert [sum(p[0] == demo_ref.RECT for p in prims) for _, _, prims in rush] == [1, 2, 2, 1] + [0] * 10


def test_pack_primitives_refusals():
    from pyannote_video_amd import render
    start, prims, text = render.pack_primitives([[], [(render.PRIM_RECT, 1, 2, 3, 4, (5, 6, 7)), (render.PRIM_TEXT, -3, 9, (255, 0, 0), 2, b"ab")], []])
    assert start.tolist() == [0, 0, 2, 2] and prims.dtype == np.int32 and prims.shape == (2, 8)
    assert prims[0].tolist() == [0, 1, 2, 3, 4, 5 | 6 << 8 | 7 << 16, 0, 0] and prims[1].tolist() == [2, -3, 9, 0, 2, 255, 2, 0]
    assert text.tobytes() == b"ab"
    with pytest.raises(ValueError):
        render.pack_primitives([[(render.PRIM_RECT, 0, 0, 1, 1, (0, 0, 0))] * 4097])
    with pytest.raises(ValueError):
        render.pack_primitives([[(render.PRIM_TEXT, 0, 0, (0, 0, 0), 1, b"x" * 65)]])
    with pytest.raises(ValueError):
        render.pack_primitives([[(render.PRIM_LINE, 0, 0, 2 ** 31, 1, (0, 0, 0))]])


# ---- Y4M ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True])
def test_y4m_writer_reads_back(tmp_path, full):
    from pyannote_video_amd import render, y4m
    w, h = 37, 23
    rng = np.random.RandomState(2)
    frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(3)]
    path = str(tmp_path / "out.y4m")
    with render.Y4mWriter(path, w, h, rate="30000:1001", full_range=full) as wr:
        for f in frames:
            wr.write(np.frombuffer(b"".join(p.tobytes() for p in demo_ref.to_yuv420(f, "601", full)), np.uint8))
        assert wr.frames == 3
    data = open(path, "rb").read()
    assert data.startswith(b"YUV4MPEG2 W37 H23 F30000:1001 C420" + (b" XCOLORRANGE=FULL\n" if full else b"\n"))
    v = y4m.Y4mVideo(path)
    assert len(v) == 3 and v.size == (w, h) and v.layout == "420" and v.full_range == full
    assert abs(v.frame_rate - 30000 / 1001.0) < 1e-12 and v.rate_tag == "30000:1001"
    for i, f in enumerate(frames):
        got = v.frame(i)
        for a, b in zip((got.y, got.u, got.v), demo_ref.to_yuv420(f, "601", full)):
            assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        render.Y4mWriter(str(tmp_path / "x.y4m"), w, h).write(np.zeros(5, np.uint8))


def test_rate_tag():
    from pyannote_video_amd import render

    class V(object):
        rate_tag = "24000:1001"
    assert render.rate_tag(V(), 25.0) == "24000:1001"
    assert render.rate_tag(object(), 25.0) == "25:1"
    assert render.rate_tag(object(), 29.97) in ("2997:100",)
    assert render.rate_tag(object(), 30000 / 1001.0) == "30000:1001"
    assert render.demo_size(1920, 1080, 400) == (711, 400) and render.text_scale(400) == 2 and render.text_scale(50) == 1


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_cli_parses_demo_and_refuses_stdin_video(capsys):
    from pyannote_video_amd import cli
    a = cli.parse_args(["demo", "--height", "300", "--from", "1.5", "--until", "9", "--shift", "0.04", "--landmark", "lm.txt", "--label", "lab.txt",
                        "film.y4m", "track.txt", "-"])
    assert (a.verb, a.height, a.t_from, a.t_until, a.shift, a.landmark, a.label, a.video, a.tracking, a.output) == \
           ("demo", 300, 1.5, 9.0, 0.04, "lm.txt", "lab.txt", "film.y4m", "track.txt", "-")
    a = cli.parse_args(["demo", "film.y4m", "track.txt", "out.y4m"])
    assert (a.height, a.t_from, a.t_until, a.shift, a.landmark, a.label) == (400, 0.0, None, 0.0, None, None)
    with pytest.raises(SystemExit):
        cli.main(["demo", "-", "track.txt", "out.y4m"])
    assert "needs the length" in capsys.readouterr().err
    assert "out of scope" not in cli.__doc__ and "demo" in cli.__doc__


def test_overlapping_primitives_in_both_orders_differ():
    """the two overlap cases of tests/test_gpu_demo.py are not the same picture: the order is what they test"""
    c1, c2, c3 = (250, 10, 20), (5, 200, 90), (40, 60, 255)
    one = [(demo_ref.RECT, 30, 10, 120, 50, c1), (demo_ref.LINE, 0, 30, 300, 31, c2), (demo_ref.TEXT, 28, 34, c3, 3, b"over"),
           (demo_ref.RECT, 60, 5, 90, 58, c2), (demo_ref.TEXT, 58, 30, c1, 2, b"under")]
    a = demo_ref.draw(np.zeros((61, 301, 3), np.uint8), one)
    b = demo_ref.draw(np.zeros((61, 301, 3), np.uint8), one[::-1])
    assert not np.array_equal(a, b)


def test_read_labels_names_a_malformed_line(tmp_path):
    from pyannote_video_amd import render
    path = tmp_path / "labels.txt"
    path.write_text("0 anna\n\n3 7\n")
    assert render.read_labels(str(path)) == {0: "anna", 3: "7"}
    path.write_text("0 anna\n5\n")
    with pytest.raises(ValueError, match="labels.txt:2"):
        render.read_labels(str(path))
