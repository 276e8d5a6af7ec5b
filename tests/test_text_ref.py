"""CPU: CAPTION.md's worked values on the restatement (tests/text_ref.py), the reach of the case table (tests/text_cases.py), the planted
defects the comparison must see, the host rules of `caption` on hand-made masks -- the package (pyannote_video_amd/text.py) against the
restatement and against written-down answers -- every refusal, the planted clips, and both verbs through cli.main on a scripted context."""
import json

import numpy as np
import pytest

from pyannote_video_amd import cli, runtime, text
from tests import text_cases as tc, text_ref as tr
from tests.test_motion_ref import ClipVideo, Dev, Ring


def counts_of(y, yp=None, edge=48, still=8, on=24):
    """(E, S, M, NP, bits) per cell of a grey frame and its grey predecessor"""
    rows, counts = tr.rows_of([tc.grey(y)], None if yp is None else tc.grey(yp), edge, still, on)
    c = counts[0].astype(int)
    return c[..., 0], c[..., 1], c[..., 2], c[..., 3], tr.bits_of(rows)[0]


# ---- the worked values of CAPTION.md -------------------------------------------------------------------------------------------------
def test_a_constant_frame_gives_all_zeros():
    rows, counts = tr.rows_of([tc.grey(np.full((20, 40), 77))] * 2)
    assert not rows[:, 2:].any() and not counts[..., :3].any()
    assert rows[0, 0] == 40 | 20 << 16 and rows[0, 1] == 48 | 8 << 8 | 24 << 16 and rows[1, 1] == rows[0, 1] | 1 << 31
    assert counts[0, :, :, 3].tolist() == [[256, 256, 128], [64, 64, 32]]            # NP: the right and lower cells are partial


def test_a_step_gives_two_stroke_columns_in_two_cells():
    y = 255 * (np.arange(40)[None, :] >= 16) * np.ones((16, 1), int)
    E = counts_of(y)[0]
    assert E.tolist() == [[16, 16, 0]]                                               # column 15 and column 16 of every row
    assert (tr.gx_of(y)[0] > 0).nonzero()[0].tolist() == [15, 16]


def test_the_central_difference_is_blind_to_period_2():
    y = 255 * (np.arange(37)[None, :] & 1) * np.ones((3, 1), int)
    g = tr.gx_of(y)
    assert (g[:, 1:-1] == 0).all() and (g[:, 0] == 255).all() and (g[:, -1] == 255).all()


def test_a_ramp_counts_the_inside_columns_at_2k_and_none_above():
    k = 3
    y = k * np.arange(30)[None, :] * np.ones((2, 1), int)
    g = tr.gx_of(y)
    assert (g[:, 1:-1] == 2 * k).all() and (g[:, 0] == k).all() and (g[:, -1] == k).all()
    assert counts_of(y, edge=2 * k)[0].sum() == 2 * 28 and counts_of(y, edge=2 * k + 1)[0].sum() == 0


def test_persistence_and_the_still_threshold():
    rng = np.random.default_rng(1)
    y = rng.integers(0, 200, (33, 50))
    E, S, M, NP, _ = counts_of(y, y)
    assert E.sum() > 0 and (S == E).all() and not M.any()                           # two identical frames
    E2, S2, M2, _, _ = counts_of(y + 8, y)
    assert (E2 == E).all() and (S2 == E).all() and not M2.any()                     # plus `still` everywhere, unsaturated
    E3, S3, M3, NP3, _ = counts_of(y + 9, y)
    assert (E3 == E).all() and not S3.any() and (M3 == NP3).all()                   # plus still + 1
    assert not counts_of(y)[1].any() and not counts_of(y)[2].any()                  # no predecessor: S = M = 0


def test_a_cell_with_exactly_on_persistent_strokes_sets_its_bit():
    for on in (1, 24, 256):
        y = np.zeros((16, 82), int) + tc.cell_with(on, 16, 82) + tc.cell_with(on - 1, 48, 82)
        E, S, M, NP, bits = counts_of(y, y, on=on)
        assert S[0, 1] == on and S[0, 3] == on - 1 and bits[0, 1] and not bits[0, 3]


def test_luma_of_grey_and_of_the_pure_colours():
    assert all(tr.luma(np.array([v, v, v])) == v for v in range(256))
    assert [int(tr.luma(np.array(c))) for c in ((255, 0, 0), (0, 255, 0), (0, 0, 255))] == [77, 149, 29]     # (19635 + 128) >> 8, ...
    assert int(tr.luma(np.array((0, 255, 0)), "no_round")) == 149 and int(tr.luma(np.array((1, 1, 2)))) == 1


def test_mask_words_and_bit_order():
    y = np.zeros((16, 1030), int)
    for base in (16, 496, 512, 1008):                                                # cells 1, 31, 32 and 63
        y += tc.cell_with(30, base, 1030)
    rows, _ = tr.rows_of([tc.grey(y)] * 2)
    assert rows.shape == (2, 8 + 3) and not rows[0, 8:].any()
    assert [int(v) for v in rows[1, 8:]] == [1 << 1 | 1 << 31, 1 << 0 | 1 << 31, 0] and rows[1, 5] == 4


# ---- the table ------------------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_seam():
    geo = set(tc.GEOMETRIES)
    cws = {tr.geometry(w, h)[0] for w, h in geo}
    assert {1, 2, 32, 33, 65} <= cws and {(1, 1), (2, 1), (1, 2)} <= geo
    assert {(3 * w) % 16 for w, h in geo if h > 1} >= {15, 5, 3}                    # rows that start at odd byte offsets of a 16-byte chunk
    assert {(tc.S * 16 - 1, 17), (tc.S * 16, 17), (tc.S * 16 + 1, 17)} <= geo and tc.S * 16 == 256
    assert any(w % 16 == 15 for w, h in geo) and any(w % 16 == 1 for w, h in geo) and any(h % 16 == 1 and h > 256 for w, h in geo)
    assert len(tc.cases()) == len(tc.GEOMETRIES) * len(tc.CONTENTS) * len(tc.PARAMS)


@pytest.mark.parametrize("params", tc.PARAMS)
def test_the_table_reaches_every_equality(params):
    edge, still, on = params
    seen = set()
    for w, h in tc.GEOMETRIES:
        for content in ("edge_eq", "still_eq", "on_eq"):
            frames = tc.frames_of(content, w, h, params)[:2]
            y0, y1 = tr.luma(frames[0]), tr.luma(frames[1])
            g, d = tr.gx_of(y1), np.abs(y1 - y0)
            S = tr.rows_of(frames, None, edge, still, on)[1][1, :, :, 1]
            seen |= {name for name, hit in (("gx = edge", (g == edge).any()), ("gx = edge - 1", (g == edge - 1).any()),
                                            ("dY = still", (d == still).any()), ("dY = still + 1", (d == still + 1).any()),
                                            ("S = on", (S == on).any()), ("S = on - 1", (S == on - 1).any())) if hit}
    assert len(seen) == 6, seen


# ---- planted defects ------------------------------------------------------------------------------------------------------------------
SEES = {"forward": ("step", 33, 32), "wrap": ("step", 33, 32), "edge_gt": ("edge_eq", 33, 32), "still_lt": ("still_eq", 33, 32),
        "no_prev_stroke": ("noise", 33, 32), "cell15": ("noise", 33, 32), "bit_reversed": ("repeat", 33, 32), "tail_bits": ("repeat", 33, 32),
        "two_back": ("noise", 33, 32), "no_round": ("noise", 33, 32)}


def test_the_comparison_sees_every_planted_defect():
    assert set(SEES) == set(tr.DEFECTS)
    for defect, (content, w, h) in SEES.items():
        frames = tc.frames_of(content, w, h, (48, 8, 24))
        right = tr.rows_of(frames, None, 48, 8, 8)
        wrong = tr.rows_of(frames, None, 48, 8, 8, defect=defect)
        assert not (np.array_equal(right[0], wrong[0]) and np.array_equal(right[1], wrong[1])), defect
    # and the table as a whole sees each of them somewhere with its own parameters
    for defect in tr.DEFECTS:
        assert any(not np.array_equal(tr.rows_of(tc.frames_of(c, 33, 32, p), None, *p)[0], tr.rows_of(tc.frames_of(c, 33, 32, p), None, *p, defect=defect)[0])
                   for c in tc.CONTENTS for p in tc.PARAMS), defect


# ---- the host rules on hand-made masks -------------------------------------------------------------------------------------------------
W, H = 320, 176                          # 20 x 11 cells


def mask_rows(cells_at, n, fps=25.0, first_usable=0):
    """a text file of n rows of W x H: cells_at(t) -> iterable of (r, c) with the bit set"""
    cw, ch, wpr = tr.geometry(W, H)
    rows = np.zeros((n, 8 + ch * wpr), np.uint32)
    for t in range(n):
        rows[t, 0], rows[t, 1] = W | H << 16, 48 | 8 << 8 | 24 << 16 | (1 << 31 if t >= first_usable else 0)
        rows[t, 6], rows[t, 7] = tr.ms(t / fps), t
        for r, c in cells_at(t):
            rows[t, 8 + r * wpr + (c >> 5)] |= np.uint32(1 << (c & 31))
    return rows


def both(rows, **kw):
    """the package's list, after checking it against the restatement's"""
    got = text.report(rows, text.analyse(rows, **kw))
    want = tr.captions(rows, **kw)
    assert got == want, (got, want)
    return got


def strap(t0, t1, r=8, c0=4, c1=9):
    """(away from the file's ends the majority vote keeps a span's ends; within half a window of them the window is cut and they move)"""
    return lambda t: [(r, c) for c in range(c0, c1 + 1)] if t0 <= t <= t1 else []


def test_a_strap_becomes_one_caption_with_its_box_in_pixels():
    found = both(mask_rows(strap(20, 60), 100))
    assert found == [{"start": 0.8, "end": 2.4, "first": 20, "last": 60, "left": 64, "top": 128, "right": 160, "bottom": 144, "cells": 6 * 41}]


def test_rule_1_unusable_rows_and_rule_2_the_vote():
    rows = mask_rows(strap(0, 60), 100, first_usable=1)
    assert both(rows)[0]["first"] == 1                                               # the row without a predecessor holds nothing
    flicker = mask_rows(lambda t: strap(20, 60)(t) if t % 3 else [], 100)           # two frames of three: above the default half
    # ... where the window lies inside the span: a bit that is set two frames of three needs three quarters of the window, so the ends move in
    assert [(f["first"], f["last"]) for f in both(flicker)] == [(26, 53)]
    assert both(flicker, hold=0.7) == []
    assert [(f["first"], f["last"]) for f in both(flicker, window=0.0, min_duration=0.0, hold=1.0)][:2] == [(20, 20), (22, 23)]
    # exactly at the threshold: a window of 5 rows (0.16 s) with 3 set bits holds at 0.6 and not at 0.61
    five = mask_rows(lambda t: strap(0, 99)(t) if t % 5 in (0, 1, 2) else [], 100)
    assert len(both(five, window=0.16, hold=0.6)) == 1 and both(five, window=0.16, hold=0.61) == []


def test_rule_3_the_band_of_cell_rows():
    rows = mask_rows(lambda t: strap(10, 60, r=2)(t) + strap(10, 60, r=9)(t), 100)
    assert [f["top"] for f in both(rows)] == [32, 144]
    assert [f["top"] for f in both(rows, band=(0.5, 1.0))] == [144]
    assert [f["top"] for f in both(rows, band=(0.0, 0.5))] == [32]
    # the centre of cell row 5 is 88 = 0.5 H exactly: it belongs to [0.5, 1) and not to [0, 0.5)
    mid = mask_rows(strap(10, 60, r=5), 100)
    assert len(both(mid, band=(0.5, 1.0))) == 1 and both(mid, band=(0.0, 0.5)) == []


def test_rule_4_gaps_between_words():
    two = lambda t: strap(20, 70, c0=2, c1=5)(t) + strap(20, 70, c0=7, c1=10)(t)     # noqa: E731 -- one unheld cell between
    assert [(f["left"], f["right"], f["cells"]) for f in both(mask_rows(two, 100))] == [(32, 176, 9 * 51)]
    assert [(f["left"], f["right"]) for f in both(mask_rows(two, 100), gap=0)] == [(32, 96), (112, 176)]
    far = lambda t: strap(20, 70, c0=2, c1=5)(t) + strap(20, 70, c0=8, c1=11)(t)     # noqa: E731 -- two cells between
    assert len(both(mask_rows(far, 100))) == 2 and len(both(mask_rows(far, 100), gap=2)) == 1


def test_rule_5_components_join_in_time_and_space():
    moving = lambda t: [(8, c) for c in range(4 + (t >= 40), 10 + (t >= 40))] if 10 <= t <= 70 else []       # noqa: E731
    assert [(f["left"], f["right"]) for f in both(mask_rows(moving, 100), window=0.0)] == [(64, 176)]
    stacked = lambda t: strap(10, 60, r=7)(t) + strap(10, 60, r=8, c0=9, c1=12)(t)   # noqa: E731 -- the two share column 9
    assert [(f["left"], f["top"], f["right"], f["bottom"]) for f in both(mask_rows(stacked, 100))] == [(64, 112, 208, 144)]
    apart = lambda t: strap(10, 40)(t) + strap(42, 80)(t)                            # noqa: E731 -- one empty row in time
    assert [(f["first"], f["last"]) for f in both(mask_rows(apart, 100), window=0.0)] == [(10, 40), (42, 80)]


def test_rule_6_each_drop_condition_at_and_beyond_its_threshold():
    rows = mask_rows(strap(20, 45), 100)                                             # 25 rows later: exactly 1.000 s
    assert len(both(rows, min_duration=1.0)) == 1 and both(rows, min_duration=1.001) == []
    assert len(both(rows, min_width=6)) == 1 and both(rows, min_width=7) == []
    tall = mask_rows(lambda t: [(r, c) for r in (4, 5) for c in range(4, 10)] if 10 <= t <= 60 else [], 100)
    assert len(both(tall, max_height=0.182)) == 1 and both(tall, max_height=0.181) == []      # 1000 * 32 = 32000 against mh1000 * 176
    # an L of 6 + 2 cells in a box of 6 x 3: K = 8 of 18 a row, 100 * 8 = 800 against fill100 * 18
    ell = mask_rows(lambda t: [(6, c) for c in range(4, 10)] + [(7, 4), (8, 4)] if 10 <= t <= 60 else [], 100)
    assert len(both(ell, fill=0.44, max_height=0.5)) == 1 and both(ell, fill=0.45, max_height=0.5) == []


def test_rule_7_order_and_the_file(tmp_path):
    rows = mask_rows(lambda t: strap(20, 60, r=9)(t) + strap(20, 60, r=2, c0=12, c1=16)(t) + strap(20, 60, r=2, c0=3, c1=7)(t) + strap(15, 60, r=5)(t), 100)
    found = both(rows)
    assert [(f["first"], f["top"], f["left"]) for f in found] == [(15, 80, 64), (20, 32, 48), (20, 32, 192), (20, 144, 64)]
    src, out = str(tmp_path / "t.npy"), str(tmp_path / "c.json")
    np.save(src, rows)
    assert cli.main(["caption", src, out]) == 0
    assert json.load(open(out)) == found and open(out).read() == json.dumps(found, indent=1) + "\n"
    assert cli.main(["caption", src, "-"]) == 0


def test_rule_8_the_tracks_on_screen(tmp_path):
    rows = mask_rows(strap(25, 75), 100)                                             # 1.0 s .. 3.0 s
    lines = ([(t / 25.0, 0, (0.1, 0.1, 0.2, 0.2), "detection") for t in range(20, 80)]           # all of it
             + [(t / 25.0, 1, (0.5, 0.1, 0.6, 0.2), "detection") for t in range(25, 51)]         # 1.0 .. 2.0: exactly half
             + [(t / 25.0, 2, (0.7, 0.1, 0.8, 0.2), "detection") for t in range(25, 50)]         # 1.0 .. 1.96: less
             + [(t / 25.0, 3, (0.7, 0.5, 0.8, 0.6), "detection") for t in range(80, 90)])        # after it
    assert text.report(rows, text.analyse(rows), lines) == tr.captions(rows, tracks=lines)
    found = tr.captions(rows, tracks=lines)
    assert found[0]["tracks"] == [0, 1] and found[0]["alone"] is False
    assert tr.captions(rows, tracks=lines[:60] + lines[86:])[0] == dict(found[0], tracks=[0], alone=True)
    from pyannote_video_amd import formats
    src, trk, out = str(tmp_path / "t.npy"), str(tmp_path / "track.txt"), str(tmp_path / "c.json")
    np.save(src, rows)
    with open(trk, "w") as f:
        for T, i, box, status in lines[:60]:
            f.write("%.3f %d %.3f %.3f %.3f %.3f %s\n" % ((T, i) + box + (status,)))
    assert len(formats.read_tracks(trk)) == 60
    assert cli.main(["caption", "--tracking", trk, src, out]) == 0
    assert json.load(open(out)) == [dict(found[0], tracks=[0], alone=True)]


def test_every_refusal_of_caption(tmp_path):
    good = mask_rows(strap(10, 60), 100)
    mixed = good.copy()
    mixed[50, 1] = 47 | 8 << 8 | 24 << 16 | 1 << 31
    other_size = good.copy()
    other_size[3, 0] = 321 | 176 << 16
    backwards = good.copy()
    backwards[7, 6] = 0
    files = {"int32": good.astype(np.int32), "flat": good.reshape(-1), "short": good[:, :7], "words": good[:, :-1], "mixed": mixed,
             "other_size": other_size, "backwards": backwards, "zero_size": np.zeros((2, 8), np.uint32)}
    out = str(tmp_path / "c.json")
    for name, table in files.items():
        path = str(tmp_path / (name + ".npy"))
        np.save(path, table)
        with pytest.raises(ValueError, match="caption: "):
            cli.caption(path, out)
        with pytest.raises(SystemExit):
            cli.main(["caption", path, out])
    with pytest.raises(ValueError, match="not a text file"):
        cli.caption(str(tmp_path / "absent.npy"), out)
    src = str(tmp_path / "good.npy")
    np.save(src, good)
    for args in (["--hold", "1.2"], ["--hold", "-0.1"], ["--fill", "1.01"], ["--fill", "-1"], ["--rows", "0.5,0.5"], ["--rows", "0.6,0.4"],
                 ["--rows", "-0.1,1"], ["--rows", "0,1.1"], ["--rows", "0.5"], ["--window", "-1"], ["--min-duration", "-1"], ["--gap", "-1"],
                 ["--min-width", "-1"], ["--max-height", "-0.5"]):
        with pytest.raises(SystemExit):
            cli.main(["caption"] + args + [src, out])
    assert cli.main(["caption", "--hold", "1", "--fill", "0", "--rows", "0,1", "--gap", "0", src, out]) == 0       # the ends of the ranges
    empty = str(tmp_path / "empty.npy")
    np.save(empty, good[:0])
    assert cli.main(["caption", empty, out]) == 0 and json.load(open(out)) == []
    with pytest.raises(SystemExit):
        cli.main(["caption", "--hold", "2", empty, out])


# ---- the planted clips -----------------------------------------------------------------------------------------------------------------
def test_the_strap_on_a_moving_background_is_the_one_caption():
    rows = tr.video_rows(tc.planted_clip(), tc.CLIP_FPS)
    bits = [int(v) for v in rows[:, 5]]
    assert sum(bits[:tc.STRAP_FRAMES[0]]) + sum(bits[tc.STRAP_FRAMES[1] + 1:]) == 0              # no bit on any frame without the strap
    found = both(rows)
    print(found)
    assert len(found) == 1
    f = found[0]
    assert (f["left"], f["top"], f["right"], f["bottom"]) == tc.STRAP                            # the box exactly
    assert 0 <= f["first"] - (tc.STRAP_FRAMES[0] + 1) <= 2 and 0 <= tc.STRAP_FRAMES[1] - f["last"] <= 2
    # what the restatement gives on this clip, written down: the strap's first frame differs from its predecessor
    assert (f["first"], f["last"], f["cells"], f["start"], f["end"]) == (31, 79, 980, 1.24, 3.16)


def test_the_same_clip_on_a_still_background_is_dropped_by_the_height_rule():
    rows = tr.video_rows(tc.planted_clip(moving=False), tc.CLIP_FPS)
    assert both(rows) == []
    whole = both(rows, max_height=1.0)
    assert [(f["first"], f["last"], f["left"], f["top"], f["right"], f["bottom"]) for f in whole] == [(1, 99, 0, 0, 320, 176)]


def test_a_moving_background_without_a_strap_gives_nothing():
    rows = tr.video_rows(tc.planted_clip(strap=False), tc.CLIP_FPS)
    assert not rows[:, 5].any() and both(rows, max_height=1.0, min_duration=0.0, min_width=0) == []


# ---- the verbs --------------------------------------------------------------------------------------------------------------------------
class ScriptContext(object):
    """frame_text is the restatement, one call at a time; given: every frame an earlier call was given -- its last is carried as `prev`
    of the next, no other"""

    def __init__(self):
        self.live, self.calls, self.given = [], [], []

    def ingest_ring(self, h, w, depth=16):
        return Ring(self)

    def frame_text(self, frames, prev=None, edge=48, still=8, on=24, want_counts=False):
        assert all(not f.released for f in frames) and (prev is None or not prev.released), "a row asked of a released frame"
        assert all(f.released for f in self.given if f is not prev), "a frame of an earlier call, not the carried one, is still resident"
        self.given.extend(frames)
        self.calls.append((len(frames), prev is not None))
        rows, counts = tr.rows_of([f.rgb for f in frames], None if prev is None else prev.rgb, edge, still, on)
        return rows, (counts if want_counts else None)

    def mem_info(self):
        return 0, 0


def test_text_through_main_equals_the_plain_loop_at_every_batch_and_step(tmp_path, monkeypatch):
    frames = tc.planted_clip()[20:60]
    n = len(frames)
    ctx = ScriptContext()
    monkeypatch.setattr(runtime, "default_context", lambda: ctx)
    monkeypatch.setattr(cli, "open_video", lambda spec, fps, **kw: ClipVideo(frames, tc.CLIP_FPS))
    for step, k in ((0.0, 1), (0.12, 3)):
        want = tr.video_rows(frames, tc.CLIP_FPS, step=step)
        assert len(want) == -(-n // k) and [int(v) for v in want[:3, 7]] == [0, k, 2 * k]
        files = {}
        for batch in (1, 7, 64):
            ctx.calls[:] = []
            del ctx.live[:]
            files[batch] = str(tmp_path / ("text%d_%d.npy" % (k, batch)))
            assert cli.main(["text", "--step", str(step), "--batch", str(batch), "film", files[batch]]) == 0
            m = len(want)
            sizes = [batch] * (m // batch) + ([m % batch] if m % batch else [])
            assert ctx.calls == [(s, i > 0) for i, s in enumerate(sizes)]           # every later call carries the frame before as prev
            assert len(ctx.live) == m and all(f.released for f in ctx.live)         # only the wanted frames were uploaded; none is left
            got = np.load(files[batch])
            assert got.dtype == np.uint32 and np.array_equal(got, want), (step, batch)
        assert open(files[1], "rb").read() == open(files[7], "rb").read() == open(files[64], "rb").read()
    # a range of the video, other parameters
    out = str(tmp_path / "part.npy")
    assert cli.main(["text", "--from", "0.4", "--until", "1.0", "--edge", "30", "--still", "4", "--on", "12", "film", out]) == 0
    assert np.array_equal(np.load(out), tr.video_rows(frames, tc.CLIP_FPS, edge=30, still=4, on=12, first=10, end=25))
    # caption on what text wrote
    cap = str(tmp_path / "cap.json")
    assert cli.main(["caption", "--min-duration", "0.5", files[7], cap]) == 0
    assert json.load(open(cap)) == tr.captions(tr.video_rows(frames, tc.CLIP_FPS, step=0.12), min_duration=0.5)
    a = cli.parse_args(["text", "-", "text.npy"])
    assert (a.video, a.output, a.step, a.edge, a.still, a.on, a.t_from, a.t_until, a.batch) == ("-", "text.npy", 0.0, 48, 8, 24, 0.0, None, 64)
    a = cli.parse_args(["caption", "text.npy", "out.json"])
    assert (a.window, a.hold, a.gap, a.min_duration, a.min_width, a.max_height, a.fill, a.band, a.tracking) == (1.0, 0.5, 1, 1.0, 3, 0.25, 0.5, "0,1", None)
    for args in (["--edge", "0"], ["--edge", "256"], ["--still", "255"], ["--on", "0"], ["--on", "257"], ["--batch", "0"], ["--batch", "4097"],
                 ["--step", "-1"]):
        with pytest.raises(SystemExit):
            cli.main(["text"] + args + ["film", out])


def test_the_carrier_hands_back_all_but_the_frame_it_carries():
    """measure -> (rows, the frames the caller may release now): the one held from before and all but the last of the call's;
    ScriptContext checks at every call that no other is left"""
    clip = tc.planted_clip()[20:27]
    ctx = ScriptContext()
    carry = text.Carry(ctx)
    frames = [Dev(f) for f in clip]
    parts, held = [], []
    for part in (frames[:3], frames[3:6], frames[6:]):
        rows, done = carry.measure(part)
        assert len(rows) == len(part) and sorted(map(id, done)) == sorted(map(id, held + part[:-1]))
        parts.append(rows)
        for f in done:
            f.release()
        held = part[-1:]
    assert ctx.calls == [(3, False), (3, True), (1, True)] and [f.released for f in frames] == [True] * 6 + [False] and carry.held is frames[6]
    assert np.array_equal(np.concatenate(parts), tr.rows_of(clip, None, 48, 8, 24)[0])


def test_the_wanted_set_and_the_stamp():
    wanted = text.EveryKth(10, 25, 4)
    assert [i for i in range(40) if i in wanted] == [10, 14, 18, 22] and len(wanted) == 4 and max(wanted) == 22
    assert len(text.EveryKth(10, 10, 4)) == 0 and not text.EveryKth(10, 10, 4)
    assert 10 ** 9 in text.EveryKth(0, None, 1)
    assert text.every(0.0, 25.0) == 1 and text.every(0.1, 25.0) == 3 and text.every(0.5, 25.0) == 13 and text.every(1.0, 29.97) == 30
    rows = text.stamp(np.zeros((3, 9), np.uint32), 7, 25.0, 5)
    assert rows[:, 6].tolist() == [280, 480, 680] and rows[:, 7].tolist() == [7, 12, 17]
    assert text.geometry(1920, 1080) == (120, 68, 4) and text.row_words(1920, 1080) == 280
