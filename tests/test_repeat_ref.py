"""CPU: REPEAT.md's worked values on the restatement (tests/repeat_ref.py), planted defects shown to be seen by the comparison the GPU
tests make, the margins of the GPU tests' inputs (tests/repeat_cases.py), the host rules on hand-made runs, and the two verbs through
cli.main on a scripted context against a plain loop."""
import json
import os
import re

import numpy as np
import pytest

from pyannote_video_amd import cli, repeat, runtime
from tests import repeat_cases as rc, repeat_ref as rr, storyboard_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = rc.S
ALL = (1 << 64) - 1


def gray(y):
    """a frame whose three channels are the array y (its luma is y: 77 + 150 + 29 = 256)"""
    y = np.asarray(y, np.uint8)
    return np.stack([y, y, y], -1)


# ---- the print: worked values --------------------------------------------------------------------------------------------------------
def test_constant_frames():
    for v, (w, h) in ((0, (9, 9)), (255, (64, 36)), (131, (10, 7)), (7, (1, 1))):
        p = rr.print_of(np.full((h, w, 3), v, np.uint8))
        assert int(p[0]) == 0 and int(p[1]) == 0 and int(p[3]) == 0
        assert int(p[2]) == 81 * v                                   # SY = 81 v, RANGE = 0


def test_ramps_and_the_transposed_frame():
    ramp = np.tile(np.arange(9, dtype=np.uint8) * 20 + 3, (9, 1))   # luma rises strictly along every row
    p = rr.print_of(gray(ramp))
    assert (int(p[0]), int(p[1])) == (ALL, 0)
    assert int(p[2]) == int(ramp.astype(int).sum()) | 160 << 32
    q = rr.print_of(gray(ramp.T))
    assert (int(q[0]), int(q[1])) == (0, ALL) and q[2] == p[2]
    noise = rc.make_frame(9, 9, "noise")
    a, b = rr.print_of(noise), rr.print_of(noise.transpose(1, 0, 2))

    def transposed(word):            # bit 8 r + c <-> bit 8 c + r
        return sum(1 << (8 * c + r) for r in range(8) for c in range(8) if word >> (8 * r + c) & 1)
    assert int(b[0]) == transposed(int(a[1])) and int(b[1]) == transposed(int(a[0])) and b[2] == a[2]
    for w, h in ((64, 36), (641, 359)):          # the ramps of the GPU cases are strict on the grid at these sizes
        assert int(rr.print_of(rc.make_frame(w, h, "ramp_x"))[0]) == ALL and int(rr.print_of(rc.make_frame(w, h, "ramp_y"))[1]) == ALL


def test_a_9_x_9_frame_is_its_own_grid_and_a_small_side_replicates():
    f = rc.make_frame(9, 9, "noise")
    assert np.array_equal(rr.grid(f), f)
    y = rr.luma(f)
    assert y[2, 3] == (77 * int(f[2, 3, 0]) + 150 * int(f[2, 3, 1]) + 29 * int(f[2, 3, 2]) + 128) >> 8
    p = rr.print_of(f)
    assert (int(p[0]) >> (8 * 2 + 3) & 1) == int(y[2, 3] < y[2, 4]) and (int(p[1]) >> (8 * 2 + 3) & 1) == int(y[2, 3] < y[3, 3])
    assert int(p[2]) & 0xFFFFFFFF == int(y.sum()) and int(p[2]) >> 32 == int(y.max() - y.min())
    small = rc.make_frame(3, 3, "noise")
    assert np.array_equal(rr.grid(small), small.repeat(3, axis=0).repeat(3, axis=1))         # 3 x 3: every pixel three times
    one = rc.make_frame(1, 1, "noise")
    assert (rr.grid(one) == one[0, 0]).all()
    assert np.array_equal(rr.luma(np.array([[[255, 255, 255], [0, 0, 1]]], np.uint8)), [[255, 0]])       # 29 + 128 < 256


def test_the_stamp_is_talks_milliseconds_and_the_frame_index():
    p = rr.stamp(np.zeros((4, 4), np.uint64), [0.0, 0.04, 1 / 3.0, 2.0004])
    assert [int(v) & 0xFFFFFFFF for v in p[:, 3]] == [0, 40, 333, 2000] and [int(v) >> 32 for v in p[:, 3]] == [0, 1, 2, 3]
    q = repeat.stamp(np.zeros((3, 4), np.uint64), 5, 25.0)
    assert [int(v) & 0xFFFFFFFF for v in q[:, 3]] == [200, 240, 280] and [int(v) >> 32 for v in q[:, 3]] == [5, 6, 7]
    assert np.array_equal(q, rr.stamp(np.zeros((8, 4), np.uint64), [i / 25.0 for i in range(8)])[5:])


def test_the_constants_the_kernel_the_header_and_the_host_share():
    hdr = open(os.path.join(ROOT, "include", "pvface.h")).read()
    assert int(re.search(r"#define PVF_RUNS_STRIP (\d+)", hdr).group(1)) == repeat.RUNS_STRIP == S
    assert int(re.search(r"#define PVF_PRINT_MAX_ROWS (\d+)", hdr).group(1)) == repeat.MAX_ROWS == 1 << 24
    src = open(os.path.join(ROOT, "pyannote-video_amd", "csrc", "repeat.hip")).read()
    assert "PR_S = PVF_RUNS_STRIP" in src and "PR_D = %d" % rc.GROUP in src


# ---- runs: worked values -------------------------------------------------------------------------------------------------------------
def test_the_run_count_when_every_pair_matches():
    for NA, NB, L, want in ((5, 7, 1, 11), (5, 7, 3, 7), (257, 300, 4, 550), (1, 1, 1, 1), (3, 9, 3, 7)):
        c = rc.all_equal(NA, NB)
        other = rc.planted("x", NA, NB, [], seed=5)                  # random prints match as well at tau = 128
        for case in (c, other):
            got = rr.runs(case.A, case.ua, case.B, case.ub, tau=128, min_len=L)
            assert len(got) == want == rr.run_count_all_match(NA, NB, L)
            assert got.tolist() == sorted(got.tolist(), key=lambda r: (r[1] - r[0], r[0]))


def test_random_prints_never_match_at_the_verbs_default():
    A, B = rc.random_prints(300, 1), rc.random_prints(400, 2)
    assert rr.distances(A, B).min() > 30
    assert len(rr.runs(A, np.ones(300, np.uint8), B, np.ones(400, np.uint8), tau=rc.TAU_RANDOM)) == 0


def test_an_unusable_frame_splits_a_planted_copy_into_two_runs_on_one_diagonal():
    case = rc.planted("split", 60, 80, [rc.Plant(10, 30, 12, rc.PLANT_BITS, "")], seed=9)
    assert rr.runs(case.A, case.ua, case.B, case.ub, tau=rc.PLANT_BITS).tolist() == [[10, 30, 12]]
    ub = case.ub.copy()
    ub[34] = 0
    assert rr.runs(case.A, case.ua, case.B, ub, tau=rc.PLANT_BITS).tolist() == [[10, 30, 4], [15, 35, 7]]
    ua = case.ua.copy()
    ua[10] = 0                                   # a flat frame matches nothing, itself included
    assert rr.runs(case.A, ua, case.B, case.ub, tau=rc.PLANT_BITS).tolist() == [[11, 31, 11]]
    assert len(rr.runs(case.A, ua, case.A, ua, tau=0, min_len=1)) == 2       # the main diagonal, cut at the flat frame


# ---- planted defects are seen --------------------------------------------------------------------------------------------------------
def test_print_defects_are_seen_on_the_gpu_tests_frames():
    frames = [rc.make_frame(w, h, c) for w, h in rc.SIZES[:6] for c in rc.CONTENTS]
    good = rr.prints(frames)
    for defect in rr.PRINT_DEFECTS:
        assert not np.array_equal(rr.prints(frames, defect), good), defect
    # each by the content that shows it
    flat = [rc.make_frame(64, 36, "full")]
    assert int(rr.prints(flat, "le_for_lt")[0, 0]) == ALL and int(rr.prints(flat)[0, 0]) == 0
    ramp = [rc.make_frame(64, 36, "ramp_x")]
    assert int(rr.prints(ramp, "swap_hv")[0, 1]) == ALL and int(rr.prints(ramp)[0, 1]) == 0
    noise = [rc.make_frame(64, 36, "noise")]
    assert rr.prints(noise, "bit_order")[0, 0] != rr.prints(noise)[0, 0]
    assert (rr.sy_of(rr.prints(frames, "luma_floor")) != rr.sy_of(good)).any()


@pytest.fixture(scope="module")
def seams():
    return rc.seam_case()


def test_run_defects_are_seen_on_the_gpu_tests_tables(seams):
    good = rr.runs(seams.A, seams.ua, seams.B, seams.ub, tau=rc.PLANT_BITS)
    cut = rr.runs(seams.A, seams.ua, seams.B, seams.ub, tau=rc.PLANT_BITS, defect="seam", strip=S)
    assert len(cut) == len(good) + 1 + 1 + 3                         # the runs that cross one, one and three seams
    assert not np.array_equal(rr.runs(seams.A, seams.ua, seams.B, seams.ub, tau=rc.PLANT_BITS, defect="unsorted"), good)
    for L in (4, 5, 2 * S + 10):                                     # a run of exactly this length is there
        assert len(rr.runs(seams.A, seams.ua, seams.B, seams.ub, tau=rc.PLANT_BITS, min_len=L, defect="min_len_off")) < \
            len(rr.runs(seams.A, seams.ua, seams.B, seams.ub, tau=rc.PLANT_BITS, min_len=L))
    ub = seams.ub.copy()
    ub[1500] = 0
    assert len(rr.runs(seams.A, seams.ua, seams.B, ub, tau=rc.PLANT_BITS, defect="flat_matches")) == len(good) == \
        len(rr.runs(seams.A, seams.ua, seams.B, ub, tau=rc.PLANT_BITS)) - 1
    me = rc.self_case()
    for g in (1, 2, 390, 391):                   # a run lies on diagonals 1, 2, 390 and none on 391: 390 is the last that shows it
        a, b = rr.runs(me.A, me.ua, tau=rc.PLANT_BITS, min_gap=g), rr.runs(me.A, me.ua, tau=rc.PLANT_BITS, min_gap=g, defect="min_gap_off")
        assert (len(a) != len(b)) == (g != 391)


# ---- the margins of the GPU tests' inputs --------------------------------------------------------------------------------------------
def test_random_rows_of_the_gpu_tables_never_come_within_tau(seams):
    D = rr.distances(seams.A, seams.B)
    for p in seams.plants:
        d = D[np.arange(p.i, p.i + p.n), np.arange(p.j, p.j + p.n)]
        assert (d == p.bits).all()                                   # every planted row lies exactly at its distance
        D[np.arange(p.i, p.i + p.n), np.arange(p.j, p.j + p.n)] = 128
    assert D.min() > 2 * rc.TAU_RANDOM
    me = rc.self_case()
    D = rr.distances(me.A, me.A)
    for p in me.plants:
        assert (D[np.arange(p.i, p.i + p.n), np.arange(p.j, p.j + p.n)] == p.bits).all()
    close = np.argwhere(np.triu(D <= 2 * rc.TAU_RANDOM, 1))
    planted = set((p.i + t, p.j + t) for p in me.plants for t in range(p.n))
    assert set(map(tuple, close.tolist())) == planted
    for NA, NB in rc.SIZE_PAIRS + rc.THIN:
        c = rc.size_case(NA, NB)
        D = rr.distances(c.A, c.B)
        p = c.plants[0]
        D[np.arange(p.i, p.i + p.n), np.arange(p.j, p.j + p.n)] = 128
        assert D.min() > 2 * rc.TAU_RANDOM, (NA, NB)


def test_the_seams_are_reached_and_planted_runs_cross_them(seams):
    NA, NB = rc.SEAM_NA, rc.SEAM_NB
    assert NA > 3 * S and NB > 3 * S
    by = dict((p.what, p) for p in seams.plants)
    crosses = lambda p: [k for k in range(1, 4) if p.i < k * S <= p.i + p.n - 1]          # noqa: E731
    assert crosses(by["crosses one seam"]) == [2] and crosses(by["crosses three seams"]) == [1, 2, 3]
    assert by["starts on the last row of a strip"].i % S == S - 1 and by["starts on the first row of a strip"].i % S == 0
    d0 = -(NA - 1)
    lanes = [(p.j - p.i - d0) % rc.GROUP for p in seams.plants]
    assert lanes[seams.plants.index(by["the first diagonal of a group"])] == 0
    assert lanes[seams.plants.index(by["the last diagonal of a group"])] == rc.GROUP - 1
    diagonals = [p.j - p.i for p in seams.plants]
    assert min(diagonals) == d0 and max(diagonals) == NB - 1        # the first and the last diagonal
    assert any(p.i == 0 for p in seams.plants) and any(p.j == 0 for p in seams.plants)
    assert any(p.i + p.n == NA for p in seams.plants) and any(p.j + p.n == NB for p in seams.plants)
    assert set(p.bits for p in seams.plants) == {0, rc.PLANT_BITS}
    sizes = set(n for pair in rc.SIZE_PAIRS for n in pair)
    assert sizes >= set(rc.EDGE_SIZES) and rc.THIN == ((3, 5000), (5000, 3))
    me = rc.self_case()
    assert any(p.i < S <= p.i + p.n - 1 for p in me.plants) and len(me.A) > S


# ---- the host rules ------------------------------------------------------------------------------------------------------------------
T25 = [40 * i for i in range(4000)]              # milliseconds of a 25 fps file


def test_bridging_at_the_gap_and_one_frame_beyond():
    # 0.5 s at 25 fps: from the last matched frame to the next matched frame at most 500 ms = 12 frames (480 ms); 13 frames are 520 ms
    runs = [(100, 300, 10), (121, 321, 5)]       # frame 109 -> frame 121: 12 frames
    assert rr.bridge(runs, T25, 500) == [(100, 300, 26)] == repeat.bridge(runs, T25, 0.5)
    runs = [(100, 300, 10), (122, 322, 5)]       # 13 frames: 520 ms
    assert rr.bridge(runs, T25, 500) == runs == repeat.bridge(runs, T25, 0.5)
    runs = [(100, 300, 10), (115, 315, 5), (130, 330, 2), (150, 350, 1), (115, 316, 5)]      # a chain, a far one, another diagonal
    want = [(100, 300, 32), (150, 350, 1), (115, 316, 5)]
    assert rr.bridge(runs, T25, 500) == want == repeat.bridge(runs, T25, 0.5)
    assert repeat.bridge([], T25, 0.5) == []


def test_a_static_shot_keeps_its_longest_diagonal():
    n = 50
    A, B = rc.random_prints(120, 41), rc.random_prints(150, 42)
    A[30:30 + n] = A[30]
    B[70:70 + n] = A[30]
    found = rr.runs(A, np.ones(120, np.uint8), B, np.ones(150, np.uint8), tau=0)
    assert len(found) == 2 * n - 1 == 99
    segs = [tuple(int(v) for v in r) for r in found]
    assert rr.keep_outermost(segs) == [(30, 70, n)] == repeat.outermost(segs)
    t = [40 * i for i in range(150)]
    assert repeat.segments(found, t, 1.0, 0.5) == [(30, 70, n)]
    assert repeat.segments(found, t, 2.0, 0.5) == []                 # 49 frames at 25 fps are 1.96 s


def test_containment_needs_both_intervals_and_ties_go_by_diagonal_then_row():
    a, b, c = (10, 110, 20), (12, 212, 10), (12, 114, 10)            # b: inside a on A's side only; c: inside on both
    assert repeat.outermost([c, b, a]) == [a, b] == rr.keep_outermost([c, b, a])
    x, y, z = (50, 60, 8), (10, 25, 8), (10, 20, 8)                  # equal lengths: (j - i, i) decides
    assert repeat.outermost([y, x, z]) == [z, x, y] == rr.keep_outermost([y, x, z])
    same = [(5, 9, 6), (5, 9, 6)]
    assert repeat.outermost(same) == [(5, 9, 6)]


def test_separation_in_frames_of_the_files_own_times():
    assert repeat.separation_frames(np.array(T25[:1000]), 5.0) == 125
    assert repeat.separation_frames(np.array(T25[:1000]), 0.0) == 1
    assert repeat.separation_frames(np.array(T25[:10]), 5.0) == 10   # none: the file's length, so no diagonal exists
    assert repeat.separation_frames(np.array([], np.int64), 5.0) == 1


# ---- the verbs on a scripted context -------------------------------------------------------------------------------------------------
def frame_of(i, w=40, h=24):
    return np.random.default_rng(2000 + i).integers(0, 256, (h, w, 3), dtype=np.uint8)


class ScriptVideo(object):
    """frames 30 .. 44 are frames 5 .. 19 again"""

    def __init__(self, n, fps=5.0, shift=0):
        self.n, self.frame_size, self.size, self.frame_rate, self.shift = n, (40, 24), (40, 24), fps, shift

    def __len__(self):
        return self.n

    def frame(self, i):
        i += self.shift
        return frame_of(i - 25 if 30 <= i < 45 else i)

    def __iter__(self):
        for i in range(self.n):
            yield i / self.frame_rate, self.frame(i)


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
    """frame_prints and print_runs are the restatement"""

    def __init__(self):
        self.live, self.calls, self.joins = [], [], []

    def ingest_ring(self, h, w, depth=16):
        return Ring(self)

    def frame_prints(self, frames, out_ptr=None):
        assert all(not f.released for f in frames), "a print asked of a released frame"
        self.calls.append(len(frames))
        return rr.prints([f.rgb for f in frames])

    def print_runs(self, A, usable_a, B=None, usable_b=None, tau=10, min_len=1, min_gap=1, cap=None):
        self.joins.append((len(A), None if B is None else len(B), tau, min_gap))
        return rr.runs(np.asarray(A)[:, :2], usable_a, None if B is None else np.asarray(B)[:, :2], usable_b, tau=tau, min_len=min_len,
                       min_gap=min_gap)

    def mem_info(self):
        return 0, 0


@pytest.fixture
def scripted(monkeypatch):
    ctx = ScriptContext()
    videos = {"film-a": ScriptVideo(50), "film-b": ScriptVideo(40, shift=3)}
    monkeypatch.setattr(runtime, "default_context", lambda: ctx)
    monkeypatch.setattr(cli, "open_video", lambda spec, fps, **kw: videos[spec])
    return ctx, videos


def test_both_verbs_through_main_equal_the_plain_loop(tmp_path, scripted):
    ctx, videos = scripted
    pa, pb, out = str(tmp_path / "a.npy"), str(tmp_path / "b.npy"), str(tmp_path / "out.json")
    assert cli.main(["fingerprint", "--batch", "7", "film-a", pa]) == 0
    assert ctx.calls == [7] * 7 + [1] and all(f.released for f in ctx.live)           # one pass, every frame, released batch by batch
    assert cli.main(["fingerprint", "film-b", pb]) == 0
    want_a = rr.stamp(rr.prints([videos["film-a"].frame(i) for i in range(50)]), [i / 5.0 for i in range(50)])
    want_b = rr.stamp(rr.prints([videos["film-b"].frame(i) for i in range(40)]), [i / 5.0 for i in range(40)])
    got_a, got_b = np.load(pa), np.load(pb)
    assert got_a.dtype == np.uint64 and np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b)
    assert cli.main(["repeat", "--min-duration", "1.0", "--min-separation", "2.0", out, pa, pb]) == 0
    assert ctx.joins == [(50, None, 10, 10), (50, 40, 10, 1), (40, None, 10, 10)]     # a x a, a x b, b x b; 2 s at 5 fps are 10 frames
    found = json.load(open(out))
    assert found == rr.report([(pa, want_a), (pb, want_b)], min_duration=1.0, min_separation=2.0)
    keys = [(s["a"], s["b"], s["offset"], s["frames"]) for s in found]
    # a: 5 .. 19 again at 30 .. 44; b is a from frame 3 on, so a's frame i is b's i - 3 and a's 30 .. 44 are also b's 2 .. 16; a's 5 .. 17
    # against b's 27 .. 39 (offset 22) lies inside the 40 frames of offset -3 on both sides and is dropped
    assert keys == [(pa, pa, 25, 15), (pa, pb, -3, 40), (pa, pb, -28, 15), (pb, pb, 25, 13)]
    assert found == sorted(found, key=lambda s: ((pa, pb).index(s["a"]), (pa, pb).index(s["b"]), s["a_start"]))
    first = found[keys.index((pa, pa, 25, 15))]
    assert first == {"a": pa, "b": pa, "a_start": 1.0, "a_end": 3.8, "b_start": 6.0, "b_end": 8.8, "frames": 15, "offset": 25}
    # a range of the video, and stdout
    ctx.calls[:] = []
    assert cli.main(["fingerprint", "--from", "1.0", "--until", "3.0", "film-a", pa]) == 0
    assert np.array_equal(np.load(pa), want_a[5:15]) and ctx.calls == [10]
    assert cli.main(["repeat", "--max-bits", "0", "--min-duration", "0.5", "--min-separation", "1", "-", pb]) == 0


def test_repeat_refuses_with_a_message(tmp_path, scripted, capsys):
    good, bad, other = str(tmp_path / "good.npy"), str(tmp_path / "bad.npy"), str(tmp_path / "other.npy")
    np.save(good, np.zeros((3, 4), np.uint64))
    np.save(bad, np.zeros((3, 4), np.int64))
    np.save(other, np.zeros((3, 2), np.uint64))
    out = str(tmp_path / "out.json")
    for args, word in ((["repeat", out, bad], "uint64 [n][4]"), (["repeat", out, good, other], "uint64 [n][4]"),
                       (["repeat", out, str(tmp_path / "missing.npy")], "not a print file"), (["repeat", "--max-bits", "129", out, good], "--max-bits"),
                       (["repeat", "--max-bits", "-1", out, good], "--max-bits"), (["repeat", out], "prints"),
                       (["fingerprint", "--batch", "0", "film-a", out], "--batch")):
        with pytest.raises(SystemExit):
            cli.main(args)
        assert word in capsys.readouterr().err, args
    with pytest.raises(ValueError, match="no print files"):
        cli.repeat(out, [])
    with pytest.raises(ValueError, match="no print files"):
        repeat.compare(None, [])
    assert cli.main(["repeat", out, good]) == 0 and json.load(open(out)) == []      # flat frames (RANGE 0) match nothing


def test_every_frame_is_wanted():
    w = repeat.EveryFrame(3, 9)
    assert 3 in w and 8 in w and 2 not in w and 9 not in w and max(w) == 8 and bool(w)
    assert not repeat.EveryFrame(4, 4)
    assert (1 << 24) - 1 in repeat.EveryFrame() and max(repeat.EveryFrame()) == (1 << 24) - 1
    assert storyboard_ref.thumb(frame_of(0), 9, 9).shape == (9, 9, 3)


def test_fingerprint_of_a_stream_without_a_length(tmp_path):
    class Stream(object):                        # what `-` gives: frames in order, no len(), no frame(i)
        frame_rate, frame_size, size = 5.0, (40, 24), (40, 24)

        def __iter__(self):
            for i in range(23):
                yield i / 5.0, frame_of(i)
    ctx, out = ScriptContext(), str(tmp_path / "stream.npy")
    assert cli.fingerprint(Stream(), out, batch=10, ctx=ctx) == {"frames": 23, "first": 0}
    want = rr.stamp(rr.prints([frame_of(i) for i in range(23)]), [i / 5.0 for i in range(23)])
    assert np.array_equal(np.load(out), want) and ctx.calls == [10, 10, 3] and all(f.released for f in ctx.live)
    assert cli.fingerprint(Stream(), out, t_from=2.0, t_until=3.0, ctx=ScriptContext()) == {"frames": 5, "first": 10}
    assert np.array_equal(np.load(out), want[10:15])
    a = cli.parse_args(["fingerprint", "-", "prints.npy"])
    assert (a.video, a.output, a.t_from, a.t_until, a.batch) == ("-", "prints.npy", 0.0, None, 64)
    a = cli.parse_args(["repeat", "out.json", "a.npy", "b.npy"])
    assert (a.prints, a.max_bits, a.flat, a.min_duration, a.max_gap, a.min_separation) == (["a.npy", "b.npy"], 10, 16, 2.0, 0.5, 5.0)
