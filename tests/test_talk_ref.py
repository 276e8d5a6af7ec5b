"""CPU: TALK.md on its restatement (tests/talk_ref.py) and on the host code of the `talk` verb (talk.py, the parser, cli.talk on a
scripted context).  Worked values of the eight integers on contents whose sums can be found by hand, that the comparison the GPU tests
make sees each of a list of planted defects, the host rules on hand-made points and series, and the verb's files against a plain
loop."""
import os

import numpy as np
import pytest

from tests import talk_ref as tr
from tests.test_faces_ref import Ring, ScriptVideo, make_inputs
from pyannote_video_amd import cli, formats, pipeline, talk

CASES = tr.named_cases()
GOOD = dict((name, tr.motion(*case)) for name, case in CASES.items())


# ---- the restatement alone ---------------------------------------------------------------------------------------------------------
def test_constants_agree_with_the_package_and_the_header():
    assert (talk.WINDOW_ROWS, talk.WINDOW_COLS, talk.COL0, talk.MOUTH_ROW0, talk.CONTROL_ROW0, talk.MARGIN, talk.ZERO_SHIFT) == \
        (tr.ROWS, tr.COLS, tr.COL0, tr.MOUTH0, tr.CONTROL0, tr.MARGIN, tr.ZERO) == (40, 64, 42, 94, 52, 3, 24)
    assert (talk.WINDOW_PIXELS, talk.BOTH_PIXELS, talk.MAX_FACES) == (tr.PIXELS, 2 * tr.PIXELS, tr.MAX_FACES) == (2560, 5120, 32768)
    assert dict(window=talk.WINDOW, on=talk.ON, off=talk.OFF, min_duration=talk.MIN_DURATION, max_pause=talk.MAX_PAUSE,
                max_dark=talk.MAX_DARK) == tr.DEFAULTS == dict(window=0.4, on=3.0, off=1.5, min_duration=0.3, max_pause=0.3, max_dark=0.25)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvface.h")).read()
    assert "#define PVF_MOTION_MAX_FACES %d " % talk.MAX_FACES in hdr
    assert talk.MAX_FACES * 2 * 46 * 72 == 217055232                                # the header's 217 MB of patches


def test_worked_values():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (150, 150, 3), dtype=np.uint8)
    assert tr.motion([a, a], [-1, 0])[1, :6].tolist() == [0, 0, 24, 0, 0, 24]       # identical chips
    black, white = tr.grey(np.zeros((150, 150))), tr.grey(np.full((150, 150), 255))
    assert tr.motion([black, white], [-1, 0])[1].tolist() == [652800, 652800, 24, 652800, 652800, 24, 652800, 0]
    assert tr.motion([white, black], [-1, 0])[1].tolist() == [652800, 652800, 24, 652800, 652800, 24, 0, 5120]
    cur = np.zeros_like(a)
    cur[2:, :149] = a[:148, 1:]                                                     # the content moved 2 rows down and 1 column left
    DM0, DMmin, kM, DC0, DCmin, kC = tr.motion([a, cur], [-1, 0])[1, :6].tolist()
    assert (DMmin, kM, DCmin, kC) == (0, 11, 0, 11) and DM0 > 0 and DC0 > 0
    assert np.array_equal(cur, tr.shifted(a, -2, 1)) and 11 == (-2 + 3) * 7 + (1 + 3)
    assert GOOD["moved"][1, :6].tolist()[1:3] == [0, 11]
    first = tr.motion([a], [-1])[0]                                                 # no predecessor: SM and NZ still computed
    assert first[:6].tolist() == [-1] * 6 and first[6] == tr.luma(a)[94:134, 42:106].sum() and first[7] > 0


def test_a_change_inside_the_mouth_window_and_changes_outside_what_is_read():
    prev = tr.grey(np.full((150, 150), 100))
    cur = prev.copy()
    cur[100:110, 50:60] = 130                                                       # 100 pixels, 30 grey levels each
    assert tr.motion([prev, cur], [-1, 0])[1].tolist() == [3000, 3000, 24, 0, 0, 24, 100 * 2560 + 3000, 0]
    rng = np.random.default_rng(4)
    a, b = (rng.integers(0, 256, (150, 150, 3), dtype=np.uint8) for _ in range(2))
    want = tr.motion([a, b], [-1, 0])
    for rows, cols in ((slice(40, 49), slice(0, 150)), (slice(0, 150), slice(0, 39)), (slice(137, 150), slice(0, 150)), (slice(0, 150), slice(109, 150))):
        a2, b2 = a.copy(), b.copy()
        a2[rows, cols] = 255 - a2[rows, cols]
        b2[rows, cols] = 255 - b2[rows, cols]
        assert np.array_equal(tr.motion([a2, b2], [-1, 0]), want)
    chips, _ = CASES["shifts"]                                                      # the corners of what is read are live: they are the
    for k, (r, c), col in ((0, (49, 39), 4), (48, (136, 108), 1)):                  # predecessor's, where the minimum is at a corner shift
        p2 = chips[k].copy()
        p2[r, c] = 255 - p2[r, c]
        got = tr.motion([p2, chips[k + 1]], [-1, 0])[1]
        assert got[col] == abs(255 - 2 * int(chips[k][r, c, 0])) > 0 and got[col + 1] == k and GOOD["shifts"][k + 1, col] == 0


def test_every_shift_is_found_and_is_the_only_minimum():
    chips, prev = CASES["shifts"]
    got = GOOD["shifts"]
    for k in range(49):
        assert got[1 + k, :6].tolist()[1:3] == [0, k] and got[1 + k, 4:6].tolist() == [0, k], k
        for r0 in (tr.MOUTH0, tr.CONTROL0):
            D = tr.displaced(tr.luma(chips[1 + k]), tr.luma(chips[k]), r0)
            assert (D == 0).sum() == 1 and D[k // 7, k % 7] == 0, k               # smooth, non-periodic content: one minimum
        assert (got[1 + k, 0] == 0) == (k == 24)


def test_planted_defects_are_visible():
    """each defect changes what the GPU tests compare, on the contents those tests use"""
    defects = (("row_off", dict(row_off=1)), ("col_off", dict(col_off=1)), ("range_2", dict(margin=2)), ("wrong_face", dict(wrong_face=True)),
               ("squared", dict(squared=True)), ("no_rounding", dict(rounding=False)), ("plain_row_major", dict(plain_row_major=True)),
               ("nz_mouth_only", dict(nz_mouth_only=True)))
    seen = {}
    for name, kw in defects:
        seen[name] = [c for c in CASES if not np.array_equal(tr.motion(*CASES[c], **kw), GOOD[c])]
        assert seen[name], name
    assert "chain" in seen["row_off"] and "chain" in seen["col_off"] and "one" in seen["row_off"] and "one" in seen["col_off"]      # SM moves too
    assert "shifts" in seen["range_2"] and "moved" not in seen["range_2"]           # (-2, 1) is inside the smaller range
    assert "chain" in seen["wrong_face"] and "shifts" in seen["wrong_face"]         # the shift's sign turns round
    assert "chain" in seen["squared"] and "extremes" in seen["squared"]
    assert "rounding" in seen["no_rounding"]                                        # 77 * 2 + 128 = 282 >> 8 = 1, without the term 0
    assert seen["plain_row_major"] == ["extremes", "constant", "dark", "rounding"]  # where D is the same at several shifts, the zero shift among them
    assert "dark" in seen["nz_mouth_only"] and "extremes" in seen["nz_mouth_only"]


# ---- host rules ------------------------------------------------------------------------------------------------------------------
def _pts(top, bottom, left, right):
    p = np.zeros((68, 2), np.int32)
    p[62], p[66], p[48], p[54] = top, bottom, left, right
    return p


def test_openness():
    assert talk.openness(_pts((50, 60), (50, 70), (30, 65), (70, 65))) == 0.25      # gap 10 over width 40
    assert talk.openness(_pts((50, 60), (50, 60), (30, 65), (70, 65))) == 0.0       # closed
    assert talk.openness(_pts((50, 60), (53, 64), (30, 65), (30, 65))) == 0.0       # no width
    assert talk.openness(_pts((0, 0), (3, 4), (0, 0), (6, 8))) == 0.5               # any direction
    rng = np.random.default_rng(6)
    for _ in range(20):
        p = rng.integers(-2000, 4000, (68, 2)).astype(np.int32)
        assert talk.openness(p) == tr.openness(p)


def test_activity_and_validity():
    row = [900, 800, 3, 500, 288, 24, 1000, 1280]
    assert talk.activity(row, True) == (0.2, True) == tr.activity(row, True)        # (800 - 288) / 2560; NZ = 0.25 * 5120 is still valid
    assert talk.activity(row[:7] + [1281], True) == (0.0, False) == tr.activity(row[:7] + [1281], True)
    assert talk.activity(row, False) == (0.0, False) and talk.activity(row, True, max_dark=0.2) == (0.0, False)
    assert talk.activity([5, 5, 24, 9, 7, 24, 0, 0], True) == (0.0, True)           # the control window moved more: clamped at 0


def test_link_across_a_hole():
    faces = [(3, 1), (3, 2), (4, 1), (4, 2), (6, 1), (5, 2), (7, 1), (6, 2)]       # track 1 has no face on frame 5
    assert talk.link(faces) == [-1, -1, 0, 1, -1, 3, 4, 5] == tr.link(faces)


def test_smoothing_window_edges():
    times = [0.0, 0.04, 0.08, 0.12, 0.16, 0.2, 0.24, 0.28, 0.32, 0.36, 0.4]
    a = [float(i * i) for i in range(11)]
    valid = [i != 3 for i in range(11)]
    s = talk.smooth(times, a, valid, 0.4)
    assert s == tr.smooth(times, a, valid, 0.4)
    assert s[5] == sum(a[j] for j in range(11) if j != 3) / 10                       # |t' - t| = 0.2 = window / 2 is inside, on both sides
    assert talk.smooth(times, a, valid, 0.39)[5] == sum(a[j] for j in range(1, 10) if j != 3) / 8
    assert s[0] == (a[0] + a[1] + a[2] + a[4] + a[5]) / 5
    assert talk.smooth(times, a, [False] * 11, 0.4) == [0.0] * 11
    assert talk.smooth(times, a, valid, 0.0)[3] == 0.0 and talk.smooth(times, a, valid, 0.0)[4] == 16.0


def test_hysteresis():
    s = [0.0, 2.9, 3.0, 2.0, 1.5, 1.49, 2.9, 3.5, 1.6, 0.1]
    want = [False, False, True, True, True, False, False, True, True, False]
    assert talk.decide(s, 3.0, 1.5) == want == tr.decide(s, 3.0, 1.5)
    assert talk.decide([2.0, 2.0]) == [False, False]                                # between the thresholds from the start: off


def test_spans_merge_then_drop():
    times = [0.04 * i for i in range(40)]
    state = [False] * 40
    for i in list(range(2, 6)) + list(range(12, 15)) + list(range(30, 33)):         # 0.08-0.20, 0.48-0.56, 1.20-1.28
        state[i] = True
    s = [float(i) for i in range(40)]
    got = talk.spans(times, state, s, 0.3, 0.3)
    assert got == tr.spans(times, state, s, 0.3, 0.3)
    # 0.48 - 0.20 = 0.28 <= 0.3: merged into 0.08-0.56, which lasts 0.48 and stays, though each part alone is shorter than 0.3;
    # 1.20 - 0.56 > 0.3: alone, 0.08 long, dropped
    assert [(i, j) for i, j, _ in got] == [(2, 14)] and got[0][2] == sum(range(2, 15)) / 13.0
    assert [(i, j) for i, j, _ in talk.spans(times, state, s, 0.3, 0.27)] == []     # not merged: every part too short
    assert [(i, j) for i, j, _ in talk.spans(times, state, s, 0.08, 0.0)] == [(2, 5), (12, 14), (30, 32)]
    assert talk.spans(times, [False] * 40, s) == [] and [(i, j) for i, j, _ in talk.spans(times, [True] * 40, s)] == [(0, 39)]


def test_analyse_equals_the_rules_one_by_one():
    rng = np.random.default_rng(8)
    faces, rows, linked = [], [], []
    for track in (4, 2):
        for f in range(30):
            faces.append((f / 25.0, track, rng.integers(0, 200, (68, 2)).astype(np.int32)))
            burst = 10 <= f < 24 and track == 4
            rows.append([0, int(rng.integers(9000, 12000)) if burst else 500, 24, 0, 400, 24, 0, 3000 if f == 15 else 0])
            linked.append(f > 0)
    per, segs = talk.analyse(faces, rows, linked)
    assert [t for t, _, _, _ in segs] == [4] and segs[0][1] >= 0.3 and segs[0][2] <= 1.0
    idx = [i for i, f in enumerate(faces) if f[1] == 4]
    a = [tr.activity(rows[i], linked[i])[0] for i in idx]
    valid = [tr.activity(rows[i], linked[i])[1] for i in idx]
    assert not valid[0] and not valid[15] and a[15] == 0.0
    s = tr.smooth([faces[i][0] for i in idx], a, valid)
    (first, last, mean), = tr.spans([faces[i][0] for i in idx], tr.decide(s), s)
    assert segs == [(4, faces[idx[first]][0], faces[idx[last]][0], mean)]
    for k, i in enumerate(idx):
        assert per[i] == (tr.openness(faces[i][2]), a[k], s[k], 1 if first <= k <= last else 0)
    assert all(p[3] == 0 for i, p in enumerate(per) if faces[i][1] == 2)


def test_line_formats():
    assert talk.face_line(1.04, 7, [9, 8, 3, 7, 6, 24, 100, 2], 0.25, 0.5, 1.25, True) == "1.040 7 9 8 3 7 6 24 100 2 0.25000 0.50000 1.25000 1\n"
    assert talk.face_line(0.0, 0, [-1] * 6 + [5, 0], 0.0, 0.0, 0.0, 0) == "0.000 0 -1 -1 -1 -1 -1 -1 5 0 0.00000 0.00000 0.00000 0\n"
    assert talk.segment_line(3, 0.4, 1.0, 4.5) == "3 0.400 1.000 4.50000\n" and talk.segment_line(3, 0.4, 1.0, 4.5, "ann") == "3 0.400 1.000 4.50000 ann\n"


# ---- the verb on a scripted context ----------------------------------------------------------------------------------------------
def script_row(fi, pts, pfi, ppts):
    """eight integers that depend on the face AND on the face it was compared with, with bursts of activity and some dark faces"""
    k = int(pts[30, 0]) * 31 + int(pts[2, 1]) * 17 + fi
    tail = [k % 100000, 3000 if k % 11 == 0 else k % 50]
    if pfi is None:
        return [-1] * 6 + tail
    j = int(ppts[30, 0]) * 13 + int(ppts[8, 1]) * 7 + pfi
    dmin = 400 + (12000 if (fi // 8) % 2 else 0) + (k + j) % 700
    return [dmin + j % 90, dmin, (k + j) % 49, 500 + k % 60, 350 + j % 40, j % 49] + tail


class ScriptContext(object):
    def __init__(self, fail_at=None):
        self.calls, self.frames, self.fail_at = [], [], fail_at

    def ingest_ring(self, h, w, depth=16):
        return Ring(self.frames)

    def face_motion(self, frames, pts, prev):
        self.calls.append((len(pts), [f.i for f in frames], list(prev)))
        if self.fail_at is not None and len(self.calls) > self.fail_at:
            raise RuntimeError("scripted device error")
        assert all(not f.released for f in frames), "motion asked of a released frame"
        assert all(-1 <= p < i for i, p in enumerate(prev)) and len(frames) == len(pts) == len(prev)
        assert [f.i for f in frames] == sorted(f.i for f in frames)                 # whole frames, in order
        assert all(frames[p].i == frames[i].i - 1 for i, p in enumerate(prev) if p >= 0)
        return np.array([script_row(f.i, q, None if p < 0 else frames[p].i, None if p < 0 else pts[p]) for f, q, p in zip(frames, pts, prev)],
                        np.int32).reshape(-1, 8)


def plain_loop(video, tp, lp, labels=None, t_from=0.0, t_until=None, **params):
    """the files of the verb by a loop over the landmark file: no threads, no batches"""
    p = dict(tr.DEFAULTS, **params)
    w, h = video.frame_size
    rows = formats.read_tracks(tp)
    times = [i / video.frame_rate for i in range(len(video))]
    where = {}
    for fi, T, g in pipeline.faces_per_frame(rows, times, w, h):
        for ident, box in g:
            where[("%.3f" % T, ident)] = fi
    F = []
    for T, ident, pts in formats.read_landmarks(lp):
        if T < t_from or (t_until is not None and T >= t_until):
            continue
        q = np.array(pts, np.float32)
        q[:, 0] = np.round(q[:, 0] * w)
        q[:, 1] = np.round(q[:, 1] * h)
        F.append((T, ident, where[("%.3f" % T, ident)], q.astype(np.int32)))
    at = dict(((f[2], f[1]), i) for i, f in enumerate(F))
    out, lines, segs = [], [None] * len(F), []
    for T, ident, fi, pts in F:
        j = at.get((fi - 1, ident))
        out.append(script_row(fi, pts, None if j is None else F[j][2], None if j is None else F[j][3]))
    for track in sorted(set(f[1] for f in F)):
        idx = [i for i, f in enumerate(F) if f[1] == track]
        act = [tr.activity(out[i], out[i][0] >= 0, p["max_dark"]) for i in idx]
        tt = [F[i][0] for i in idx]
        s = tr.smooth(tt, [a for a, _ in act], [v for _, v in act], p["window"])
        kept = tr.spans(tt, tr.decide(s, p["on"], p["off"]), s, p["min_duration"], p["max_pause"])
        for k, i in enumerate(idx):
            talking = any(a <= k <= b for a, b, _ in kept)
            lines[i] = "%.3f %d " % (F[i][0], track) + " ".join("%d" % v for v in out[i]) + " %.5f %.5f %.5f %d\n" % (
                tr.openness(F[i][3]), act[k][0], s[k], talking)
        for a, b, mean in kept:
            name = "" if labels is None else " " + (labels.get(track) or "#%d" % track)
            segs.append("%d %.3f %.3f %.5f%s\n" % (track, tt[a], tt[b], mean, name))
    return "".join(lines), "".join(segs), F


@pytest.mark.parametrize("batch", [1, 7, 2048])
def test_talk_verb_files_equal_the_plain_loop(tmp_path, batch):
    video = ScriptVideo(60)
    tp, lp = make_inputs(tmp_path)
    labels = {0: "ann", 3: "7"}
    want, want_segs, F = plain_loop(video, tp, lp, labels, on=2.0, off=1.0, min_duration=0.1)
    assert want.count("\n") > 50 and " 1\n" in want and " 0\n" in want and want_segs.count("\n") >= 2 and " ann\n" in want_segs and " #" in want_segs
    ctx = ScriptContext()
    op, sp = str(tmp_path / "talk.txt"), str(tmp_path / "segments.txt")
    res = cli.talk(video, tp, lp, op, on=2.0, off=1.0, min_duration=0.1, label=labels, segments=sp, ctx=ctx, batch=batch, ahead=4)
    assert open(op).read() == want and open(sp).read() == want_segs
    assert res["faces"] == len(F) and res["linked"] == sum(1 for line in want.splitlines() if line.split()[2] != "-1")
    assert all(d.released for d in ctx.frames) and len(ctx.frames) == len(set(f[2] for f in F))       # ONE pass, every frame given back
    if batch == 2048:
        assert len(ctx.calls) == 1
    else:
        assert len(ctx.calls) > 5
        firsts = [frames[0] for _, frames, _ in ctx.calls[1:]]
        lasts = [frames[-1] for _, frames, _ in ctx.calls[:-1]]
        assert firsts == lasts                                                      # the frame before leads the next call
        for n, frames, prev in ctx.calls[1:]:
            lead = frames.count(frames[0])
            assert prev[:lead] == [-1] * lead
        # links reach into the carried frame
        assert sum(any(0 <= p < frames.count(frames[0]) for p in prev) for _, frames, prev in ctx.calls[1:]) > len(ctx.calls) // 2
        # a track whose first face is on the first new frame of a call: no predecessor, though the carried frame leads the call
        starts = set(min(f[2] for f in F if f[1] == k) for k in set(f[1] for f in F))
        assert any(len(frames) > frames.count(frames[0]) and frames[frames.count(frames[0])] in starts for _, frames, _ in ctx.calls[1:])


def test_talk_verb_window_options_and_stdout(tmp_path, capsys):
    video = ScriptVideo(60)
    tp, lp = make_inputs(tmp_path)
    want, _, F = plain_loop(video, tp, lp, t_from=0.4, t_until=0.8, window=0.2, max_dark=0.9)
    assert want and all(0.4 <= float(line.split()[0]) < 0.8 for line in want.splitlines())
    cli.talk(video, tp, lp, "-", window=0.2, max_dark=0.9, t_from=0.4, t_until=0.8, ctx=ScriptContext(), batch=3)
    assert capsys.readouterr().out == want
    class Stream(ScriptVideo):                                                      # a pipe: no length before it has been read
        def __len__(self):
            raise TypeError("a stream has no length")
    want_all, _, _ = plain_loop(video, tp, lp)
    cli.talk(Stream(60), tp, lp, str(tmp_path / "s.txt"), ctx=ScriptContext(), batch=9)
    assert open(str(tmp_path / "s.txt")).read() == want_all
    res = cli.talk(video, tp, lp, str(tmp_path / "o.txt"), t_from=50.0, ctx=ScriptContext())         # nothing left: an empty file
    assert res["faces"] == 0 and open(str(tmp_path / "o.txt")).read() == ""


def test_talk_verb_hands_on_errors_and_refuses(tmp_path, capsys):
    video = ScriptVideo(60)
    tp, lp = make_inputs(tmp_path)
    ctx = ScriptContext(fail_at=2)
    with pytest.raises(RuntimeError, match="scripted device error"):
        cli.talk(video, tp, lp, str(tmp_path / "o.txt"), ctx=ctx, batch=5, ahead=2)
    assert all(d.released for d in ctx.frames)
    other = str(tmp_path / "other.txt")                                             # a landmark file of another tracking file
    with open(other, "wb") as f:
        f.write(formats.landmark_rows([0.04], [99], np.zeros((1, 68, 2), np.int32), 64, 48))
    with pytest.raises(KeyError, match="no face of track 99"):
        cli.talk(video, tp, other, str(tmp_path / "o.txt"), ctx=ScriptContext())


def test_parser_defaults():
    a = cli.parse_args(["talk", "-", "t.txt", "l.txt", "o.txt"])
    assert (a.window, a.on, a.off, a.min_duration, a.max_pause, a.max_dark, a.t_from, a.t_until, a.label, a.segments) == \
        (0.4, 3.0, 1.5, 0.3, 0.3, 0.25, 0.0, None, None, None)
    assert (a.video, a.tracking, a.landmarks, a.output) == ("-", "t.txt", "l.txt", "o.txt")
    a = cli.parse_args(["talk", "--window", "0.2", "--on", "4", "--off", "2", "--min-duration", "0.5", "--max-pause", "0.1", "--max-dark", "0.5",
                        "--from", "1", "--until", "2.5", "--label", "n.txt", "--segments", "s.txt", "v", "t", "l", "o"])
    assert (a.window, a.on, a.off, a.min_duration, a.max_pause, a.max_dark, a.t_from, a.t_until, a.label, a.segments) == \
        (0.2, 4.0, 2.0, 0.5, 0.1, 0.5, 1.0, 2.5, "n.txt", "s.txt")
