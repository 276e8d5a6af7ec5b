"""CPU: CLOTHES.md's worked values on the restatement (tests/clothes_ref.py), the reach of the case table (tests/clothes_cases.py), the
planted defects the comparison must see, the window and skip rules and every rule of `link` on hand-made boxes and tables -- the package
(pyannote_video_amd/clothes.py) against the restatement and against written-down answers -- `clothes` through cli.main on a scripted
context at several batch sizes, and the planted clip."""
import json

import numpy as np
import pytest

from pyannote_video_amd import cli, clothes, formats, runtime
from pyannote_video_amd.pipeline import faces_per_frame
from tests import clothes_cases as cc, clothes_ref as cr
from tests.test_motion_ref import ClipVideo, Ring


def one(frame, win, B=1):
    return cr.hist_of([frame], [win], [0], 1, B)[0].astype(int)


# ---- worked values ---------------------------------------------------------------------------------------------------------------------
def test_the_bin_of_a_pixel_by_hand():
    # grey: Y = v, c1 = c2 = 0, q = 4 -> bin (v >> 6) * 64 + 36
    assert [int(cr.bins_of(np.array([v, v, v]))) for v in (0, 63, 64, 255)] == [36, 36, 100, 228]
    # (101, 100, 50): 2 B - R - G = -101, floor(-101 / 2) = -51 -> q = (13 >> 4) = 0; c1 = 1 -> q = 4; Y = (7777 + 15000 + 1450 + 128) >> 8 = 95
    assert int(cr.bins_of(np.array([101, 100, 50]))) == 64 + 32 + 0
    assert int(cr.chroma(np.array([101, 100, 50]))[1]) == -51 and int(cr.chroma(np.array([101, 100, 50]), "truncate")[1]) == -50
    assert [int(cr.q(c)) for c in (-200, -65, -64, -49, -48, 47, 48, 63, 64, 300)] == [0, 0, 0, 0, 1, 6, 7, 7, 7, 7]
    assert int(cr.luma(np.array([255, 255, 255]))) == 255 and int(cr.luma(np.array([0, 255, 0]))) == 149


def test_a_constant_frame_gives_its_area_in_one_bin():
    f = cc.frame_of("mid", 21, 17)
    b = int(cr.bins_of(np.array(cc.MID)))
    h = one(f, (3, 2, 10, 9))
    assert h[0, b] == 49 and h.sum() == 49
    assert one(f, (-5, -5, 100, 100))[0, b] == 21 * 17                              # clipped: only the frame's pixels, no black
    assert one(cc.frame_of("black", 5, 3), (-5, -5, 100, 100))[0, 36] == 15


def test_halves_and_the_clipping_arithmetic():
    f = cc.frame_of("halves", 21, 17)                                                # columns 0 .. 9 left, 10 .. 20 right
    bl, br = int(cr.bins_of(np.array(cc.LEFT))), int(cr.bins_of(np.array(cc.RIGHT)))
    assert bl != br
    h = one(f, (8, 1, 13, 4))                                                       # 2 left and 3 right columns, 3 rows
    assert h[0, bl] == 6 and h[0, br] == 9
    h = one(f, (-4, 15, 12, 40))                                                    # columns 0 .. 11, rows 15 and 16
    assert h[0, bl] == 20 and h[0, br] == 4
    for empty in ((5, 5, 5, 9), (9, 5, 5, 9), (5, 9, 9, 5), (21, 0, 30, 17), (-9, 0, 0, 17), (0, 17, 21, 20), (0, -3, 21, 0)):
        assert one(f, empty).sum() == 0


def test_a_three_row_window_in_two_and_four_bands():
    f = cc.frame_of("mid", 5, 17)
    b = int(cr.bins_of(np.array(cc.MID)))
    assert one(f, (0, 4, 5, 7), 2)[:, b].tolist() == [10, 5]                        # rows 0, 1, 2 -> bands 0, 0, 1
    assert one(f, (0, 4, 5, 7), 4)[:, b].tolist() == [5, 5, 5, 0]                   # bands 0, 1, 2: band 3 gets no row
    assert one(f, (0, 4, 5, 5), 4)[:, b].tolist() == [5, 0, 0, 0]
    # clipped at the top: rows -5 .. 3 of a window of height 9 in 3 bands; the frame holds its rows 5 .. 8: band 1 once, band 2 three times
    assert one(f, (0, -5, 5, 4), 3)[:, b].tolist() == [0, 5, 15]


def test_groups_add_and_a_group_without_windows_is_zero():
    f, g = cc.frame_of("noise", 21, 17), cc.frame_of("noise", 5, 3)
    wins = [(0, 0, 21, 17), (2, 2, 4, 3), (1, 1, 9, 9)]
    got = cr.hist_of([f, g, f], wins, [2, 0, 2], 4, 2)
    assert got.dtype == np.uint32 and got.shape == (4, 2, 256)
    assert not got[1].any() and not got[3].any()
    assert np.array_equal(got[2], cr.hist_of([f], wins[:1], [0], 1, 2)[0] + cr.hist_of([f], wins[2:], [0], 1, 2)[0])
    assert int(got.sum()) == 21 * 17 + 2 + 64


def test_the_reachable_bins():
    bins, colours = cr.every_colour()
    assert len(bins) == len(colours) and np.array_equal(cr.bins_of(colours), bins)
    # the scan finds all 256: the chroma classes saturate at -64 and 64, and every pair of saturated classes is within reach in every luma
    # class -- bin 0 is (0, 97, 0): Y = 57, c1 = -97, c2 = floor(-97 / 2) = -49 -> classes 0, 0, 0
    assert bins.tolist() == list(range(256))
    assert int(cr.bins_of(np.array([0, 97, 0]))) == 0 and int(cr.bins_of(np.array([255, 158, 255]))) == 255


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_seam():
    geo = cc.GEOMETRIES
    assert {(3 * w) % 16 for w, h in geo} >= {0, 3, 6, 9, 15} and {(3 * w) % 4 for w, h in geo} == {0, 1, 2, 3}
    assert {h for w, h in geo} == {1, 2, 3, 17} and len(geo) == 32
    for w, h in geo + list(cc.LARGE):
        wins = [tuple(int(v) for v in q) for q in (cc.windows_for(w, h) if (w, h) in geo else cc.large_windows(w, h))]
        clips = [cr.clip_of(q, w, h) for q in wins]
        if (w, h) in geo:
            assert any(c == (0, 0, w, h) and q != (0, 0, w, h) for q, c in zip(wins, clips))             # containing
            assert sum(c is None for c in clips) >= 12                                                  # outside, empty, inverted
            assert any(q[2] - q[0] == 1 and q[3] - q[1] == 1 and c is not None for q, c in zip(wins, clips))
            assert all(any(q[k] == e for q in wins) for k in range(4) for e in (cc.I32_MIN, cc.I32_MAX))
            assert any(q[1] < 0 and c is not None for q, c in zip(wins, clips))                         # clipped at the top
            assert {q[3] - q[1] for q in wins} >= {1, 2, 3, 4, 5}                                       # below, at and above every band count
        if w >= 257:
            assert {c[2] - c[0] for c in clips if c} >= set(cc.SIZES) | {cc.PIECE_COLS - 1, cc.PIECE_COLS, cc.PIECE_COLS + 1}
        if h >= 17:
            assert {c[3] - c[1] for c in clips if c} >= {1, 15, 16, 17} | {cc.PIECE_ROWS - 1, cc.PIECE_ROWS, cc.PIECE_ROWS + 1}
        if h >= 1080:
            assert {c[3] - c[1] for c in clips if c} >= set(cc.SIZES)
    # each edge and each corner is crossed by a window that keeps pixels
    w, h = 21, 17
    crossed = set()
    for q in cc.windows_for(w, h):
        if cr.clip_of(q, w, h) is not None:
            crossed.add((q[0] < 0, q[1] < 0, q[2] > w, q[3] > h))
    assert {(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True),
            (True, True, False, False), (False, True, True, False), (True, False, False, True), (False, False, True, True), (True, True, True, True)} <= crossed


def test_the_table_reaches_every_bin_and_every_class_boundary():
    bins, _ = cr.every_colour()
    seen = set()
    for w, h in cc.GEOMETRIES:
        if w * h >= len(bins):
            seen |= set(np.unique(cr.bins_of(cc.frame_of("every", w, h))).tolist())
    assert seen == set(bins.tolist())
    f = cc.frame_of("seams", 85, 17).reshape(-1, 3)
    assert len(f) >= len(cc.SEAMS)
    y, (c1, c2) = cr.luma(f), cr.chroma(f)
    assert {63, 64, 127, 128, 191, 192} <= set(y.tolist())
    assert set(cc.EDGES) <= set(c1.tolist()) and set(cc.EDGES) <= set(c2.tolist())
    d = 2 * f[:, 2].astype(int) - f[:, 0] - f[:, 1]
    assert ((d < 0) & (d % 2 == 1)).any()


# ---- planted defects -------------------------------------------------------------------------------------------------------------------
def test_the_comparison_on_the_table_sees_every_planted_defect():
    assert len(cr.DEFECTS) >= 8
    unseen = set(cr.DEFECTS)
    for w, h in ((21, 17), (257, 17), (5, 3)):
        wins = cc.windows_for(w, h)
        n = len(wins)
        for content in ("noise", "seams", "halves"):
            f = cc.frame_of(content, w, h)
            for B in (1, 4):
                right = cr.hist_of([f] * n, wins, np.arange(n), n, B)
                for defect in sorted(unseen):
                    if not np.array_equal(right, cr.hist_of([f] * n, wins, np.arange(n), n, B, defect=defect)):
                        unseen.discard(defect)
    assert not unseen, unseen


# ---- the window and the skip rules -----------------------------------------------------------------------------------------------------
def test_the_torso_window_by_hand():
    assert cr.torso((100, 50, 140, 90)) == (80, 100, 160, 180) == clothes.torso((100, 50, 140, 90))
    # w = 25, h = 31: floor(12.5 + 0.5) = 13, floor(7.75 + 0.5) = 8, floor(62 + 0.5) = 62
    assert cr.torso((10, 20, 35, 51)) == (-3, 59, 48, 121) == clothes.torso((10, 20, 35, 51))
    assert clothes.torso((10, 20, 35, 51), widen=0.0, drop=0.0, height=0.3) == (10, 51, 35, 60) == cr.torso((10, 20, 35, 51), 0.0, 0.0, 0.3)
    assert clothes.half_up(2.5) == 3 and clothes.half_up(2.4999) == 2 and clothes.half_up(0.0) == 0
    rng = np.random.default_rng(3)
    for _ in range(200):
        l, t = (int(v) for v in rng.integers(-50, 300, 2))
        box = (l, t, l + int(rng.integers(1, 200)), t + int(rng.integers(1, 200)))
        p = tuple(float(v) for v in rng.uniform(0, 3, 3))
        assert clothes.torso(box, *p) == cr.torso(box, *p)


def test_the_skip_rules_by_hand():
    W, H = 400, 300
    alone = [(7, (100, 50, 140, 90))]
    assert clothes.windows_of(alone, W, H) == [(80, 100, 160, 180)] == cr.counted(alone, W, H)
    # somebody's face box inside the window: skipped; the other's own window (low in the frame) is kept
    front = alone + [(8, (120, 120, 150, 150))]
    assert clothes.windows_of(front, W, H) == [None, (105, 158, 165, 218)] == cr.counted(front, W, H)
    assert clothes.windows_of(front, W, H, keep_overlapped=True)[0] == (80, 100, 160, 180) == cr.counted(front, W, H, keep_overlapped=True)[0]
    # touching is not meeting: a box that starts at the window's right edge
    beside = alone + [(8, (160, 120, 190, 150))]
    assert clothes.windows_of(beside, W, H)[0] is not None and cr.counted(beside, W, H)[0] is not None
    # the same track twice on a frame does not hide itself
    assert clothes.windows_of(alone + [(7, (100, 120, 140, 160))], W, H)[0] is not None
    # --min-size: a face of 40 rows against 0.13 * 300 = 39 and 0.14 * 300 = 42
    assert clothes.windows_of(alone, W, H, min_size=0.13) == cr.counted(alone, W, H, min_size=0.13) == [(80, 100, 160, 180)]
    assert clothes.windows_of(alone, W, H, min_size=0.14) == cr.counted(alone, W, H, min_size=0.14) == [None]
    # a face at the bottom of the frame: the window lies below it
    low = [(7, (100, 250, 140, 290))]
    assert clothes.windows_of(low, W, H) == [None] == cr.counted(low, W, H)
    assert clothes.windows_of(low, W, H, drop=0.0) == [(80, 290, 160, 370)]         # ten rows are inside


# ---- link ------------------------------------------------------------------------------------------------------------------------------
def row(track, first, last, hist, faces=5, bands=1):
    r = np.zeros(cr.HEAD + 256 * bands, np.int64)
    r[:6] = track, first, last, faces, 0, bands
    r[6:] = np.asarray(hist).reshape(-1)
    return r


def spread(**at):
    """a histogram of 30000 pixels: {bin: share in percent}"""
    h = np.zeros(256, np.int64)
    for b, pc in at.items():
        h[int(b[1:])] = 300 * pc
    assert h.sum() == 30000
    return h


def both(table, **kw):
    got, want = clothes.links(table, **kw), cr.links_of(table, **kw)
    assert got == want, (got, want)
    return got


RED, GREEN = spread(b10=100), spread(b20=100)


def test_score_is_the_histogram_intersection():
    a, c = row(0, 0, 100, spread(b10=60, b11=40)), row(1, 200, 300, spread(b10=50, b12=50))
    assert cr.score(a, a) == 65536 - 1                                              # floor(0.6) + floor(0.4) of 65536: one lost to the floors
    assert cr.score(a, c) == 32768 and cr.score(a, row(2, 0, 0, GREEN)) == 0
    t = np.stack([a, c])
    assert clothes.scores(t, np.array([True, True])).tolist() == [[-1, 32768], [32768, -1]]
    two = np.stack([row(0, 0, 1, np.stack([RED, GREEN]), bands=2), row(1, 5, 6, np.stack([RED, RED]), bands=2)])
    assert cr.score(two[0], two[1]) == 32768 and int(clothes.scores(two, np.array([True, True]))[0, 1]) == 32768
    assert cr.threshold(0.75) == 49152 and cr.threshold(0.05) == 3277 and clothes.fraction(0.05, "margin") == 3277


def test_a_mutual_best_pair_links_and_the_output_is_sorted():
    t = np.stack([row(3, 0, 1000, RED), row(5, 2000, 3000, RED), row(8, 0, 1000, GREEN), row(9, 2000, 3000, GREEN)])
    assert both(t) == [(3, 5, 65536), (8, 9, 65536)]


def test_a_tie_goes_to_the_smaller_track_and_fails_the_margin():
    t = np.stack([row(1, 0, 100, RED), row(2, 1000, 1100, RED), row(3, 2000, 2100, RED)])
    assert both(t) == []                                                            # everybody has two equal candidates: ambiguous
    assert both(t, margin=0.0) == [(1, 2, 65536)]                                   # without a margin the tie goes to the smaller number: 3 -> 1, but 1 -> 2


def test_the_margin_from_one_side_only():
    a = row(1, 0, 100, spread(b10=100))
    c = row(2, 1000, 1100, spread(b10=90, b11=10))
    d = row(3, 2000, 2100, spread(b10=88, b11=12))                                  # c's candidates: a at 0.9, d at 0.98 -> d; a's: c 0.9, d 0.88: a lead of 0.02
    t = np.stack([a, c, d])
    assert both(t, min_score=0.5) == [(2, 3, cr.score(c, d))]                       # a -> nobody (its lead is below 0.05); c <-> d
    assert both(t, min_score=0.5, margin=0.01) == [(2, 3, cr.score(c, d))]          # a -> c by 0.02 now, but c -> d: not mutual
    assert both(np.stack([a, c]), min_score=0.5) == [(1, 2, cr.score(a, c))]        # a single candidate has the full margin


def test_gap_cooccurrence_usability_and_the_least_score():
    t = np.stack([row(1, 0, 1000, RED), row(2, 121000, 122000, RED)])
    assert both(t) == [(1, 2, 65536)] and both(t, max_gap=119.9) == [] and both(t, max_gap=120.0) == [(1, 2, 65536)]
    t = np.stack([row(1, 0, 1000, RED), row(2, 1000, 2000, RED)])
    assert both(t) == []                                                            # they share the instant 1000: on screen together
    t = np.stack([row(1, 0, 1000, RED), row(2, 1001, 2000, RED)])
    assert both(t) == [(1, 2, 65536)]
    assert both(np.stack([row(1, 0, 1000, RED, faces=2), row(2, 1001, 2000, RED)])) == []
    assert both(np.stack([row(1, 0, 1000, RED, faces=2), row(2, 1001, 2000, RED)]), min_faces=2) == [(1, 2, 65536)]
    assert both(np.stack([row(1, 0, 1000, RED // 2), row(2, 1001, 2000, RED)])) == [] and both(np.stack([row(1, 0, 1000, RED // 2), row(2, 1001, 2000, RED)]), min_pixels=15000) != []
    empty_band = np.stack([row(1, 0, 1, np.stack([RED, 0 * RED]), bands=2), row(2, 5, 6, np.stack([RED, 0 * RED]), bands=2)])
    assert both(empty_band) == []                                                   # every band must hold pixels
    c = row(2, 2000, 3000, spread(b10=75, b11=25))
    assert both(np.stack([row(1, 0, 1000, RED), c])) == [(1, 2, 49152)] and both(np.stack([row(1, 0, 1000, RED), c]), min_score=0.7501) == []
    # an unusable track is nobody's candidate: it cannot make a usable one ambiguous
    t = np.stack([row(1, 0, 100, RED), row(2, 1000, 1100, RED), row(3, 2000, 2100, RED, faces=1)])
    assert both(t) == [(1, 2, 65536)]


def test_labels_are_merged_along_the_links_and_a_blocked_union_is_skipped():
    t = np.stack([row(1, 0, 1000, RED), row(2, 2000, 3000, RED), row(3, 0, 1000, GREEN), row(4, 2000, 3000, GREEN), row(5, 2500, 2600, RED)])
    labels = {1: "10", 2: "11", 3: "12", 4: "13", 5: "10"}
    found = [(1, 2, 60000), (3, 4, 65000)]
    for merge in (clothes.merge_labels, cr.merged_labels):
        # 3-4 first (the better score): equal sizes, the side holding track 3 names it.  1-2: cluster "10" holds 5, on screen with 2: blocked
        assert merge(labels, found, t) == {1: "10", 2: "11", 3: "12", 4: "12", 5: "10"}
        free = dict(labels)
        free[5] = "14"
        assert merge(free, found, t) == {1: "10", 2: "10", 3: "12", 4: "12", 5: "14"}
        # the side with more tracks keeps its name
        assert merge({1: "a", 2: "b", 3: "b"}, [(1, 2, 5)], t[:1]) == {1: "b", 2: "b", 3: "b"}
        # a track without a label stays without one, and takes its link with it
        assert merge({1: "a", 3: "c"}, [(1, 2, 5)], t) == {1: "a", 3: "c"}
        # links are taken best first: 1-2 merges, then 2-5 would join 5 (on screen with 2): blocked either way; then 1-5 is one cluster already
        assert merge({1: "a", 2: "b", 5: "c"}, [(2, 5, 9), (1, 2, 7)], t) == {1: "a", 2: "a", 5: "c"}


def test_link_through_main(tmp_path, capsys):
    t = np.stack([row(1, 0, 1000, RED), row(2, 2000, 3000, RED), row(3, 0, 1000, GREEN)])
    src, out, lab, merged = (str(tmp_path / n) for n in ("c.npy", "l.json", "labels.txt", "merged.txt"))
    np.save(src, t)
    with open(lab, "w") as f:
        f.write("1 7\n2 9\n3 3\n")
    assert cli.main(["link", "--labels", lab, "--merged", merged, src, out]) == 0
    doc = json.load(open(out))
    assert doc["links"] == [{"a": 1, "b": 2, "score": 65536}]
    assert doc["parameters"] == {"min_score": 49152, "margin": 3277, "max_gap_ms": 120000, "min_faces": 3, "min_pixels": 20000}
    assert open(merged).read() == "1 7\n2 7\n3 3\n"
    from pyannote_video_amd import render
    assert render.read_labels(merged) == {1: "7", 2: "7", 3: "3"}
    assert cli.main(["link", src, "-"]) == 0 and json.loads(capsys.readouterr().out) == doc
    a = cli.parse_args(["link", "c.npy", "o.json"])
    assert (a.min_score, a.margin, a.max_gap, a.min_faces, a.min_pixels, a.labels, a.merged) == (0.75, 0.05, 120.0, 3, 20000, None, None)
    bad = str(tmp_path / "bad.npy")
    np.save(bad, t.astype(np.int32))
    for args in ([bad, out], ["--labels", lab, src, out], ["--min-score", "1.5", src, out], ["--margin", "-1", src, out], ["--max-gap", "-1", src, out],
                 [str(tmp_path / "absent.npy"), out]):
        with pytest.raises(SystemExit):
            cli.main(["link"] + args)
    np.save(bad, t[::-1])
    with pytest.raises(ValueError, match="out of order"):
        cli.link(bad, out)


# ---- the verb `clothes` ------------------------------------------------------------------------------------------------------------------
class ScriptContext(object):
    """frame_hist is the restatement, one call at a time"""

    def __init__(self):
        self.live, self.calls = [], []

    def ingest_ring(self, h, w, depth=16):
        return Ring(self)

    def frame_hist(self, frames, windows, group, G, bands=2, out_ptr=None):
        assert all(not f.released for f in frames), "a histogram asked of a released frame"
        assert sorted(set(int(g) for g in group)) == list(range(G)), "a group per track present in the call"
        self.calls.append(len(frames))
        return cr.hist_of([f.rgb for f in frames], windows, group, G, bands)

    def mem_info(self):
        return 0, 0


def write_tracking(path, lines):
    with open(path, "w") as f:
        for T, i, box, status in lines:
            f.write("%.3f %d %.3f %.3f %.3f %.3f %s\n" % ((T, i) + tuple(float(v) for v in box) + (status,)))


def plain_loop(frames, path, t_from=0.0, t_until=None, **kw):
    """the file by the restatement's loop over what the tracking file holds"""
    rows = formats.read_tracks(path)
    n, h, w = frames.shape[:3]
    per = [(fi, T, [(int(t), b) for t, b in g]) for fi, T, g in faces_per_frame(rows, [i / cc.CLIP_FPS for i in range(n)], w, h, drop_last=False)
           if T >= t_from and (t_until is None or T < t_until)]
    return cr.table_of(frames, per, set(int(r[1]) for r in rows), **kw)


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    frames, lines = cc.planted_clip()
    path = str(tmp_path_factory.mktemp("clothes") / "track.txt")
    write_tracking(path, lines)
    return frames, path, plain_loop(frames, path)


def test_clothes_through_main_equals_the_plain_loop_at_every_batch(tmp_path, monkeypatch, clip):
    frames, tracking, want = clip
    assert want.dtype == np.int64 and want.shape == (5, 6 + 512) and want[:, 0].tolist() == [0, 1, 2, 3, 4]
    assert want[:, 3].tolist() == [15, 15, 20, 20, 3] and not want[:, 4].any() and (want[:, 5] == 2).all()
    assert want[:, 1].tolist() == [0, 0, 800, 800, 640] and want[:, 2].tolist() == [560, 560, 1560, 1560, 720]
    # the boxes the tracking file's three decimals give are 24 x 24, 24 x 25, 24 x 25, 24 x 23 and 24 x 24: windows of 48 x 48, 50, 50, 46, 48
    assert want[:, 6:].sum(axis=1).tolist() == [15 * 48 * 48, 15 * 48 * 50, 20 * 48 * 50, 20 * 48 * 46, 3 * 48 * 48]
    ctx = ScriptContext()
    monkeypatch.setattr(runtime, "default_context", lambda: ctx)
    monkeypatch.setattr(cli, "open_video", lambda spec, fps, **kw: ClipVideo(list(frames), cc.CLIP_FPS))
    files = {}
    for batch in (1, 7, 2048):
        ctx.calls[:] = []
        del ctx.live[:]
        files[batch] = str(tmp_path / ("clothes%d.npy" % batch))
        assert cli.main(["clothes", "--batch", str(batch), "film", tracking, files[batch]]) == 0
        assert sum(ctx.calls) == 73 and max(ctx.calls) <= batch and (batch > 7 or all(c == batch for c in ctx.calls[:-1]))
        assert len(ctx.live) == 38 and all(f.released for f in ctx.live)            # only the frames with faces were uploaded; none is left
        got = np.load(files[batch])
        assert got.dtype == np.int64 and np.array_equal(got, want), batch
    assert open(files[1], "rb").read() == open(files[7], "rb").read() == open(files[2048], "rb").read()
    # a range, other parameters
    out = str(tmp_path / "part.npy")
    args = ["--from", "0.4", "--until", "1.0", "--bands", "3", "--widen", "0.25", "--drop", "0.1", "--height", "1.5", "--min-size", "0.1"]
    assert cli.main(["clothes"] + args + ["film", tracking, out]) == 0
    part = plain_loop(frames, tracking, 0.4, 1.0, bands=3, widen=0.25, drop=0.1, height=1.5, min_size=0.1)
    assert np.array_equal(np.load(out), part) and part.shape == (5, 6 + 768) and part[:, 3].tolist() == [5, 5, 5, 5, 3]
    # a face skipped for its size still moves its track's extent and is counted as skipped
    assert cli.main(["clothes", "--min-size", "0.5", "film", tracking, out]) == 0
    small = np.load(out)
    assert np.array_equal(small, plain_loop(frames, tracking, min_size=0.5)) and small[:, 4].tolist() == [15, 15, 20, 20, 3] and not small[:, 6:].any()
    a = cli.parse_args(["clothes", "-", "track.txt", "clothes.npy"])
    assert (a.video, a.tracking, a.output, a.widen, a.drop, a.height, a.bands, a.min_size, a.keep_overlapped, a.t_from, a.t_until, a.batch) == \
        ("-", "track.txt", "clothes.npy", 0.5, 0.25, 2.0, 2, 0.0, False, 0.0, None, 2048)
    for args in (["--bands", "0"], ["--bands", "5"], ["--batch", "0"], ["--batch", "65537"], ["--widen", "-1"], ["--height", "-0.5"]):
        with pytest.raises(SystemExit):
            cli.main(["clothes"] + args + ["film", tracking, out])


def test_somebody_in_front_is_skipped_and_kept_on_request(tmp_path, monkeypatch):
    frames = np.stack([cc.frame_of("noise", 192, 144)] * 4)
    lines = []
    for fi in range(3):
        lines.append((fi / cc.CLIP_FPS, 0, tuple(np.float32(v) for v in (0.25, 0.125, 0.375, 0.25)), "detection"))           # window 36 .. 84 by 40 .. 76
        lines.append((fi / cc.CLIP_FPS, 1, tuple(np.float32(v) for v in (0.3125, 0.3125, 0.4375, 0.4375)), "detection"))      # box 60 .. 84 by 45 .. 63: in front
    tracking, out = str(tmp_path / "t.txt"), str(tmp_path / "c.npy")
    write_tracking(tracking, lines)
    ctx = ScriptContext()
    monkeypatch.setattr(runtime, "default_context", lambda: ctx)
    monkeypatch.setattr(cli, "open_video", lambda spec, fps, **kw: ClipVideo(list(frames), cc.CLIP_FPS))
    res = cli.clothes(cli.open_video("film", 25.0), tracking, out)
    got = np.load(out)
    assert res == {"tracks": 2, "faces": 3, "skipped": 3} and got[:, 3].tolist() == [0, 3] and got[:, 4].tolist() == [3, 0]
    assert np.array_equal(got, plain_loop(frames, tracking))
    res = cli.clothes(cli.open_video("film", 25.0), tracking, out, keep_overlapped=True)
    assert res == {"tracks": 2, "faces": 6, "skipped": 0} and np.array_equal(np.load(out), plain_loop(frames, tracking, keep_overlapped=True))


# ---- the planted clip --------------------------------------------------------------------------------------------------------------------
def test_the_planted_clip_gives_the_two_planted_links_and_the_merged_labels(tmp_path, clip):
    frames, tracking, table = clip
    found = both(table, min_pixels=5000)
    print(found)
    assert [(a, b) for a, b, s in found] == cc.CLIP_LINKS and all(s >= cr.threshold(0.9) for a, b, s in found)
    assert clothes.usable(table, min_pixels=5000).all() and [cr.is_usable(r, 3, 5000) for r in table] == [True] * 5
    assert both(table) == found                                                     # the grey track is too small at the default: nothing changes
    src, out, lab, merged = (str(tmp_path / n) for n in ("c.npy", "l.json", "labels.txt", "merged.txt"))
    np.save(src, table)
    with open(lab, "w") as f:
        f.write("0 0\n1 1\n2 2\n3 3\n4 4\n")
    assert cli.main(["link", "--min-pixels", "5000", "--labels", lab, "--merged", merged, src, out]) == 0
    assert [(d["a"], d["b"]) for d in json.load(open(out))["links"]] == cc.CLIP_LINKS
    assert open(merged).read() == "0 0\n1 1\n2 0\n3 1\n4 4\n"
