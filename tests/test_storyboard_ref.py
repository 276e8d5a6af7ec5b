"""STORYBOARD.md without a GPU: the restatement (tests/storyboard_ref.py) on hand-computed cases, the comparison of the GPU tests on
planted defects, what the case table reaches, the host rules of pyannote_video_amd/storyboard.py, and the `storyboard` and `scene`
verbs on a scripted context."""
import json
import warnings

import numpy as np
import pytest

from pyannote_video_amd import cli, render, storyboard
from pyannote_video_amd._core import Annotation, Segment
from tests import demo_ref, storyboard_cases as sc, storyboard_ref as sr


# ---- the thumbnail by hand ------------------------------------------------------------------------------------------------------------
def test_weights_of_three_columns_into_two():
    assert sr.weights(3, 2).tolist() == [[2, 1, 0], [0, 1, 2]]
    f = np.array([[[10, 0, 255], [20, 3, 255], [60, 6, 0]]], np.uint8)        # one row
    # (2 * 10 + 20 + 1) // 3 = 13, (20 + 2 * 60 + 1) // 3 = 47; (3 + 1) // 3 = 1, (3 + 12 + 1) // 3 = 5; 255, (255 + 1) // 3 = 85
    assert sr.thumb(f, 2, 1).tolist() == [[[13, 1, 255], [47, 5, 85]]]


def test_weights_sum_to_the_source_length():
    for n_src, n_out in ((1, 1), (3, 2), (2, 3), (17, 5), (5, 17), (1920, 160), (7, 7)):
        w = sr.weights(n_src, n_out)
        assert w.shape == (n_out, n_src) and (w.sum(axis=1) == n_src).all() and (w.sum(axis=0) == n_out).all()


def test_constant_identity_and_one_pixel():
    rng = np.random.default_rng(1)
    f = rng.integers(0, 256, (9, 14, 3), dtype=np.uint8)
    for v in (0, 1, 128, 255):
        for tw, th in ((1, 1), (5, 4), (14, 9), (31, 20)):
            assert (sr.thumb(np.full((9, 14, 3), v, np.uint8), tw, th) == v).all()
    assert np.array_equal(sr.thumb(f, 14, 9), f)
    want = [(int(f[:, :, c].astype(np.int64).sum()) + 63) // 126 for c in range(3)]
    assert sr.thumb(f, 1, 1).tolist() == [[want]]


def test_integer_reductions_round_half_up():
    f = np.zeros((2, 4, 3), np.uint8)
    f[:, :, 0] = [[1, 2, 10, 11], [2, 3, 10, 11]]       # means 2.0 and 10.5
    f[:, :, 1] = [[0, 1, 0, 0], [0, 0, 255, 255]]       # means 0.25 and 127.5
    f[:, :, 2] = [[255, 255, 255, 254], [255, 255, 255, 255]]      # means 255 and 254.75
    assert sr.thumb(f, 2, 1).tolist() == [[[2, 0, 255], [11, 128, 255]]]
    g = np.zeros((3, 3, 3), np.uint8)
    g[:, :, 0] = [[1, 2, 3], [4, 5, 6], [7, 8, 10]]     # 46 / 9 = 5.11
    g[:, :, 1] = [[0, 0, 0], [0, 0, 0], [0, 4, 0]]      # 4 / 9 = 0.44
    g[:, :, 2] = [[0, 0, 0], [0, 0, 0], [0, 5, 0]]      # 5 / 9 = 0.56
    assert sr.thumb(g, 1, 1).tolist() == [[[5, 0, 1]]]
    assert sr.thumb(f, 2, 1, defect="truncate").tolist() == [[[2, 0, 255], [10, 127, 254]]]


def test_integer_enlargement_replicates():
    f = np.array([[[7, 8, 9]]], np.uint8)
    assert (sr.thumb(f, 3, 1) == [7, 8, 9]).all() and sr.thumb(f, 3, 1).shape == (1, 3, 3)
    rng = np.random.default_rng(2)
    g = rng.integers(0, 256, (4, 5, 3), dtype=np.uint8)
    assert np.array_equal(sr.thumb(g, 15, 8), np.repeat(np.repeat(g, 2, axis=0), 3, axis=1))


# ---- the comparison sees planted defects ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    return sc.cases()


@pytest.mark.parametrize("defect", sr.DEFECTS)
def test_the_comparison_sees_a_planted_defect(table, defect):
    seen = 0
    for case in table:
        if case.w * case.h > 4096 or case.tw * case.th > 4096:
            continue
        f = sc.make_frame(case)
        if sr.mismatch(sr.thumb(f, case.tw, case.th, defect), sr.thumb(f, case.tw, case.th)) is not None:
            seen += 1
    if defect == "wrap32":                       # no small case has a sum of 2^32: the large one of the table has, and must be reached
        w, h = sc.BIG.w, sc.BIG.h
        total = 255 * w * h
        assert total + w * h // 2 >= 1 << 32 and ((total & 0xFFFFFFFF) + w * h // 2) // (w * h) != 255
        return
    assert seen > 0, defect


def test_the_comparison_sees_first_tile_wins_and_shape():
    tiles = np.stack([np.full((3, 4, 3), v, np.uint8) for v in (10, 20)])
    xy = [(0, 0), (2, 1)]
    assert sr.mismatch(sr.sheet(tiles, xy, 8, 6, first_wins=True), sr.sheet(tiles, xy, 8, 6)) is not None
    assert sr.sheet(tiles, xy, 8, 6)[1, 2].tolist() == [20, 20, 20] and sr.sheet(tiles, xy, 8, 6)[0, 2].tolist() == [10, 10, 10]
    assert sr.mismatch(np.zeros((2, 3), np.uint8), np.zeros((3, 2), np.uint8)) is not None
    assert sr.mismatch(np.zeros((2, 3), np.uint8), np.zeros((2, 3), np.uint8)) is None


# ---- what the case table reaches --------------------------------------------------------------------------------------------------------
def test_the_case_table_reaches_alignments_sum_widths_ratios_and_seams(table):
    # every residue of 3 w mod 16, and with it every alignment of a row start (row i starts i * 3 w bytes in)
    assert set((3 * c.w) % 16 for c in table) == set(range(16))
    starts = set((i * 3 * c.w) % 16 for c in table if c.name == "align" for i in range(c.h))
    assert starts == set(range(16))
    # both sum widths: a pixel's sum below 2^32 everywhere in the table, beyond it in the large case
    assert all(255 * c.w * c.h + c.w * c.h // 2 < 1 << 32 for c in table)
    assert 255 * sc.BIG.w * sc.BIG.h > 1 << 32 and sc.BIG.w * sc.BIG.h * 3 <= 2 ** 31 - 1
    # reducing, identity and enlarging on each axis independently
    sign = lambda a, b: (a > b) - (a < b)        # noqa: E731
    assert set((sign(c.tw, c.w), sign(c.th, c.h)) for c in table) == set((a, b) for a in (-1, 0, 1) for b in (-1, 0, 1))
    # column segments: output widths one below, on and above one and two segments
    assert set(c.tw for c in table) >= set(k * sc.SEG_PX + d for k in (1, 2) for d in (-1, 0, 1))
    # LDS pieces: blocks whose source columns are one below, on and above one and two pieces
    spans = set()
    for c in table:
        for seg in range(-(-c.tw // sc.SEG_PX)):
            J0, J1 = sc.block_columns(c.w, c.tw, seg)
            spans.add(J1 - J0)
    assert spans >= set(k * sc.PIECE_COLS + d for k in (1, 2) for d in (-1, 0, 1))
    # row bands: output rows of one below, on and above the staged rows, of a wide and of a narrow piece
    for ncols in (sc.PIECE_COLS, 5):
        R = sc.stage_rows(ncols)
        rows = set(sc.row_count(c.h, c.th, Y) for c in table for Y in range(c.th)
                   if min(sc.block_columns(c.w, c.tw, 0)[1] - sc.block_columns(c.w, c.tw, 0)[0], sc.PIECE_COLS) == ncols)
        assert rows >= {R - 1, R, R + 1}, (ncols, R)
    assert sc.stage_rows(sc.PIECE_COLS) == 6 and set(c.content for c in table) == set(sc.CONTENTS)


def test_ramp_content_lands_on_ties(table):
    case = next(c for c in table if c.content == "ramp" and (c.w, c.tw) == (16, 8) and c.h == c.th)
    f = sc.make_frame(case).astype(np.int64)
    pair = f[:, 0::2] + f[:, 1::2]
    assert (pair % 2 == 1).sum() > pair.size // 2       # .5 ties
    assert sr.mismatch(sr.thumb(f.astype(np.uint8), 8, 16, "truncate"), sr.thumb(f.astype(np.uint8), 8, 16)) is not None


# ---- the host rules ---------------------------------------------------------------------------------------------------------------------
def test_picks():
    pk = storyboard.shot_frames
    # 25 fps; a shot of frames 10 .. 19 (m = 10)
    assert pk(0.4, 0.8, 25.0, 100, 1) == [15] and pk(0.4, 0.8, 25.0, 100, 2) == [12, 17] and pk(0.4, 0.8, 25.0, 100, 3) == [11, 15, 18]
    assert pk(0.4, 0.76, 25.0, 100, 1) == [14] and pk(0.4, 0.76, 25.0, 100, 3) == [11, 14, 17]                 # m = 9, odd
    assert pk(0.4, 0.52, 25.0, 100, 3) == [10, 11, 12]                                                         # m = K
    assert pk(0.4, 0.48, 25.0, 100, 3) == [10, 11] and pk(0.4, 0.44, 25.0, 100, 8) == [10]                     # m < K: duplicates dropped
    assert pk(0.4, 0.4, 25.0, 100, 2) == [10]                                                                   # an empty shot shows its first frame
    assert pk(3.6, 9.0, 25.0, 100, 2) == [92, 97]                                                               # ends past the film: b = 99, m = 10
    assert pk(4.0, 5.0, 25.0, 100, 1) is None and pk(3.96, 5.0, 25.0, 100, 4) == [99]                           # starts past it / on its last frame
    for args in ((0.4, 0.8, 25.0, 100, 3), (3.6, 9.0, 25.0, 100, 2), (0.0, 0.04, 25.0, 1, 8), (1.0, 1.3, 29.97, 40, 5)):
        assert pk(*args) == sr.picks(*args)


def test_tile_size_caption_and_scale():
    assert storyboard.tile_size(160, 1920, 1080) == (160, 90) and storyboard.tile_size(160, 640, 360) == (160, 90)
    assert storyboard.tile_size(160, 720, 576) == (160, 128) and storyboard.tile_size(3, 1000, 1) == (3, 1)
    assert storyboard.tile_size(5, 2, 1) == (5, 3)        # 2.5 rounds half up
    assert storyboard.caption(212, 754.26) == "212 12:34.3" and storyboard.caption(0, 59.96, "C") == "0 1:00.0 C"
    assert storyboard.text_scale(79) == 1 and storyboard.text_scale(160) == 2
    for a in ((212, 754.26, None), (3, 0.04, "AB")):
        assert storyboard.caption(*a) == sr.caption(*a)


CELLS = [(0, 0.0, "A", 2), (1, 1.0, "B", 2), (2, 2.0, "A", 1), (3, 3.0, None, 2), (4, 4.0, "C", 2), (5, 5.0, "B", 2)]


def test_layout_by_time_and_by_thread():
    W, H, corners, prims, order = storyboard.layout(CELLS, 2, 160, 90, 4)
    assert order == [0, 1, 2, 3, 4, 5]
    cw, ch = storyboard.cell_size(2, 160, 90)
    assert (cw, ch) == (6 + 2 * 166, 18 + 14 + 90) and (W, H) == (4 * cw, 2 * ch)
    assert corners[0] == [(6, 26), (172, 26)] and corners[2] == [(2 * cw + 6, 26)] and corners[4] == [(6, ch + 26), (172, ch + 26)]
    assert prims[0] == (render.PRIM_TEXT, 6, 6 + 14 - 1, render.PALETTE[0], 2, b"0 0:00.0 A")
    assert prims[1] == (render.PRIM_RECT, 5, 25, 172 + 160, 26 + 90, render.PALETTE[0])
    assert prims[5] == (render.PRIM_RECT, 2 * cw + 5, 25, 2 * cw + 6 + 160, 26 + 90, render.PALETTE[0])       # one tile shown
    assert prims[6][3] == storyboard.NEUTRAL and prims[8][3] == render.PALETTE[2] and prims[2][3] == render.PALETTE[1]
    # by thread: A A / B B / C / the unlabelled shot; every thread on a row of its own
    W, H, corners, prims, order = storyboard.layout(CELLS, 2, 160, 90, 4, by="thread")
    assert order == [0, 2, 1, 5, 4, 3] and (W, H) == (2 * cw, 4 * ch)
    assert [c[0] for c in corners] == [(6, 26), (6, ch + 26), (cw + 6, 26), (6, 3 * ch + 26), (6, 2 * ch + 26), (cw + 6, ch + 26)]
    # a thread longer than a row wraps
    many = [(i, float(i), "A", 1) for i in range(5)] + [(5, 5.0, "B", 1)]
    W, H, corners, _, order = storyboard.layout(many, 1, 80, 45, 2, by="thread")
    cw, ch = storyboard.cell_size(1, 80, 45)
    assert (W, H) == (2 * cw, 4 * ch) and corners[4][0] == (6, 2 * ch + 6 + 6 + 7) and corners[5][0] == (6, 3 * ch + 19)
    for by in ("time", "thread"):
        for cols in (1, 3, 7):
            got, want = storyboard.layout(CELLS, 2, 100, 57, cols, by), sr.layout(CELLS, 2, 100, 57, cols, by)
            assert got[:3] == want[:3] and got[4] == want[4]
            assert [tuple(p) for p in got[3]] == [tuple(p[:3]) + (tuple(p[3]),) + tuple(p[4:]) if p[0] == demo_ref.TEXT else
                                                   tuple(p[:5]) + (tuple(p[5]),) for p in want[3]]
    with pytest.raises(ValueError):
        storyboard.layout([], 1, 160, 90, 4)


def test_labels_and_ranks():
    a = Annotation()
    a[Segment(0.0, 2.0), "x"] = "B"              # `thread` merged two touching shots
    a[Segment(2.0, 3.0), "y"] = "A"
    shots = [cli._Shot(0.0, 1.0), cli._Shot(1.0, 2.0), cli._Shot(2.0, 3.0), cli._Shot(3.0, 4.0)]
    assert storyboard.shot_labels(shots, a) == ["B", "B", "A", None] and storyboard.shot_labels(shots, None) == [None] * 4
    assert storyboard.thread_ranks(["B", "B", None, "A", "B", "C"]) == {"B": 0, "A": 1, "C": 2}
    assert sr.labels_of([(0.0, 1.0), (1.0, 2.0), (2.0, 3.0), (3.0, 4.0)], [(0.0, 2.0, "B"), (2.0, 3.0, "A")]) == ["B", "B", "A", None]


def test_check_sheet_names_the_cap_and_the_way_out():
    storyboard.check_sheet(16384, 4096, 65536, 4096)
    for args, cap in (((16385, 10, 1, 1), "PVF_SHEET_MAX_SIDE"), ((16384, 4097, 1, 1), "PVF_SHEET_MAX_PIXELS"),
                      ((10, 10, 65537, 1), "PVF_SHEET_MAX_TILES"), ((10, 10, 1, 4097), "PVF_RENDER_MAX_PRIMS")):
        with pytest.raises(ValueError) as e:
            storyboard.check_sheet(*args)
        assert cap in str(e.value) and "--width" in str(e.value) and "--from" in str(e.value) and "--until" in str(e.value)


# ---- the verbs on a scripted context ------------------------------------------------------------------------------------------------
class ScriptVideo(object):
    def __init__(self, n, w=48, h=27, fps=25.0):
        self.n, self.frame_size, self.size, self.frame_rate = n, (w, h), (w, h), fps
        self.read = []

    def __len__(self):
        return self.n

    def frame(self, i):
        self.read.append(i)
        return frame_of(i, *self.frame_size)

    def __iter__(self):
        for i in range(self.n):
            yield i / self.frame_rate, self.frame(i)


def frame_of(i, w=48, h=27):
    return np.random.default_rng(1000 + i).integers(0, 256, (h, w, 3), dtype=np.uint8)


class Dev(object):
    def __init__(self, rgb):
        self.rgb, self.released = rgb, False

    def release(self):
        assert not self.released
        self.released = True


class Ring(object):
    def __init__(self, ctx):
        self.ctx = ctx

    def push(self, rgb):
        d = Dev(rgb)
        self.ctx.live.append(d)
        return d

    def close(self):
        pass


class ScriptContext(object):
    """frame_thumbs and thumb_sheet are the restatement"""

    def __init__(self):
        self.live, self.calls, self.sheets, self.peak = [], [], 0, 0

    def ingest_ring(self, h, w, depth=16):
        return Ring(self)

    def frame_thumbs(self, frames, tw, th, out_ptr=None):
        assert all(not f.released for f in frames), "a thumbnail asked of a released frame"
        self.calls.append(len(frames))
        return sr.thumbs([f.rgb for f in frames], tw, th)

    def thumb_sheet(self, thumbs, xy, W, H, background, prims):
        self.sheets += 1
        assert all(f.released for f in self.live), "frames still resident at the sheet call"
        return sr.sheet(np.asarray(thumbs), list(xy), W, H, background, list(prims))


SHOTS = [(0.0, 0.4), (0.4, 0.44), (0.44, 1.2), (1.2, 1.6), (1.6, 2.36), (2.36, 9.0), (12.0, 13.0)]       # the last starts past the film
THREADS = [(0.0, 0.4, "A"), (0.4, 0.44, "B"), (0.44, 1.2, "A"), (1.6, 2.36, "B"), (2.36, 9.0, "C")]


def write_inputs(tmp_path):
    sp, tp = str(tmp_path / "shot.json"), str(tmp_path / "thread.json")
    with open(sp, "w") as f:
        json.dump({"pyannote": "Timeline", "content": [{"start": a, "end": b} for a, b in SHOTS]}, f)
    a = Annotation()
    for k, (s, e, l) in enumerate(THREADS):
        a[Segment(s, e), "t%d" % k] = l
    with open(tp, "w") as f:
        json.dump(a.for_json(), f)
    return sp, tp


@pytest.mark.parametrize("batch", [1, 3, 64])
@pytest.mark.parametrize("by,per,with_thread", [("time", 1, False), ("thread", 3, True), ("time", 2, True)])
def test_storyboard_equals_the_plain_loop(tmp_path, batch, by, per, with_thread):
    sp, tp = write_inputs(tmp_path)
    video, ctx = ScriptVideo(70), ScriptContext()
    out, ix = str(tmp_path / "board.npy"), str(tmp_path / "index.txt")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = cli.storyboard(video, sp, out, per=per, width=20, columns=3, thread=tp if with_thread else None, by=by, index=ix, batch=batch,
                             ctx=ctx)
    assert any("past the end" in str(w.message) for w in caught)
    labels = sr.labels_of(SHOTS, THREADS) if with_thread else [None] * len(SHOTS)
    want, lines = sr.board(frame_of, SHOTS, labels, 25.0, 70, 48, 27, per=per, width=20, columns=3, by=by)
    got = np.load(out)
    assert sr.mismatch(got, want) is None
    assert open(ix).read() == lines
    assert res == {"width": want.shape[1], "height": want.shape[0], "shots": 6, "tiles": len(lines.splitlines())}
    n = len(set(int(l.split()[2]) for l in lines.splitlines()))
    assert sorted(video.read) == sorted(set(video.read)) and len(video.read) == n        # every wanted frame read once, nothing else
    assert ctx.calls == [batch] * (n // batch) + ([n % batch] if n % batch else []) and ctx.sheets == 1
    assert all(f.released for f in ctx.live)


def test_storyboard_ppm_range_and_refusals(tmp_path):
    sp, tp = write_inputs(tmp_path)
    out = str(tmp_path / "board.ppm")
    res = cli.storyboard(ScriptVideo(70), sp, out, width=20, columns=2, t_from=0.4, t_until=1.6, ctx=ScriptContext())
    assert res["shots"] == 3 and res["tiles"] == 3
    want, _ = sr.board(frame_of, SHOTS, [None] * len(SHOTS), 25.0, 70, 48, 27, width=20, columns=2, t_from=0.4, t_until=1.6)
    assert open(out, "rb").read() == b"P6\n%d %d\n255\n" % (want.shape[1], want.shape[0]) + want.tobytes()
    for kw, word in ((dict(per=0), "--per"), (dict(per=9), "--per"), (dict(width=0), "--width"), (dict(width=1025), "--width"),
                     (dict(t_from=100.0), "no shot"), (dict(by="scene"), "--by")):
        with pytest.raises(ValueError) as e:
            cli.storyboard(ScriptVideo(70), sp, out, ctx=ScriptContext(), **{**dict(width=20), **kw})
        assert word in str(e.value)
    with pytest.raises(ValueError) as e:
        cli.storyboard(ScriptVideo(70), sp, str(tmp_path / "board.png"), ctx=ScriptContext())
    assert ".ppm" in str(e.value)
    with pytest.raises(ValueError) as e:         # beyond the caps: the message of check_sheet
        cli.storyboard(ScriptVideo(70), sp, out, width=1024, per=8, columns=3, ctx=ScriptContext())
    assert "PVF_SHEET_MAX_SIDE" in str(e.value) and "--width" in str(e.value)


def test_scene_round_trip(tmp_path):
    a = Annotation()
    for k, l in enumerate("ABABC"):
        a[Segment(float(k), float(k + 1)), "t%d" % k] = l
    tp, op = str(tmp_path / "thread.json"), str(tmp_path / "scene.json")
    with open(tp, "w") as f:
        json.dump(a.for_json(), f)
    scenes = cli.scene(str(tmp_path / "no-such-video.y4m"), tp, op)
    back = Annotation.from_json(json.load(open(op)))
    assert back == scenes
    assert [l for _, _, l in back.itertracks(yield_label=True)] == list("AAAAC")
    assert [(s.start, s.end) for s, _ in back.itertracks()] == [(float(k), float(k + 1)) for k in range(5)]
    assert cli.main(["scene", str(tmp_path / "no-such-video.y4m"), tp, op]) == 0
    # what `scene` wrote is a --thread file
    assert storyboard.shot_labels([cli._Shot(float(k), float(k + 1)) for k in range(5)], back) == list("AAAAC")


def test_parser():
    a = cli.parse_args(["storyboard", "film.y4m", "shot.json", "-"])
    assert (a.per, a.width, a.columns, a.thread, a.by, a.t_from, a.t_until, a.index, a.batch) == (1, 160, None, None, "time", 0.0, None, None, 64)
    a = cli.parse_args(["storyboard", "--per", "8", "--width", "320", "--columns", "5", "--thread", "t.json", "--by", "thread", "--from", "10",
                        "--until", "20.5", "--index", "i.txt", "--batch", "16", "film.y4m", "shot.json", "out.ppm"])
    assert (a.per, a.width, a.columns, a.thread, a.by, a.t_from, a.t_until, a.index, a.batch, a.output) == \
        (8, 320, 5, "t.json", "thread", 10.0, 20.5, "i.txt", 16, "out.ppm")
    a = cli.parse_args(["scene", "film.y4m", "thread.json", "scene.json"])
    assert (a.video, a.thread, a.output) == ("film.y4m", "thread.json", "scene.json")
    for bad in (["storyboard", "--per", "0", "v", "s", "o.ppm"], ["storyboard", "--per", "9", "v", "s", "o.ppm"],
                ["storyboard", "--by", "scene", "v", "s", "o.ppm"], ["storyboard", "v", "s"], ["scene", "v", "t"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)
    for bad in (["storyboard", "-", "s.json", "o.ppm"], ["storyboard", "--width", "0", "synthetic:64x36x4", "s.json", "o.ppm"],
                ["storyboard", "--width", "1025", "synthetic:64x36x4", "s.json", "o.ppm"]):
        with pytest.raises(SystemExit):          # a stream on stdin has no length; --width outside 1 .. 1024
            cli.main(bad)
