"""CPU: BLEND.md's worked values on the restatement (tests/blend_ref.py), planted defects shown to be seen by the comparison the GPU tests
make on the inputs of tests/blend_cases.py, the transition rules on hand-made rows and on the planted clip, the refinement of the shots,
and the two verbs through cli.main on a scripted context against a plain loop."""
import json

import numpy as np
import pytest

from pyannote_video_amd import blend, cli, runtime
from tests import blend_cases as bc, blend_ref as br

A = br.ABSENT


def lag_words(row):
    """{L: (E, R)}"""
    return {L: (int(row[4 + 2 * k]), int(row[5 + 2 * k])) for k, L in enumerate(br.LAGS)}


# ---- the row: worked values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 5, 64, 2304])
def test_constant_planes(P):
    rows = br.rows_of(np.full((40, P), 131, np.uint8))
    for t, r in enumerate(rows):
        assert (int(r[0]), int(r[1]), int(r[2])) == (P, 131 * P, P * 131 * 131)
        assert int(r[3]) == (0 if t >= 1 else A)
        for L, (E, R) in lag_words(r).items():
            assert (E, R) == ((0, 0) if t >= L else (A, A))
        assert not r[12:].any()


def test_zero_against_255():
    P = 7
    y = np.zeros((70, P), np.uint8)
    y[33:] = 255                                 # the jump lies between 32 and 33
    rows = br.rows_of(y)
    assert int(rows[33, 3]) == 255 * P and int(rows[34, 3]) == 0
    for L in br.LAGS:
        for t in range(33, 33 + L):              # a = t - L <= 32 < 33 <= t: the window holds the jump, mid on either side of it
            E, R = lag_words(rows[t])[L]
            assert E == 255 * P and R == E, (L, t)
        assert lag_words(rows[33 + L])[L] == (0, 0)
    assert int(rows[40, 1]) == 255 * P and int(rows[40, 2]) == 65025 * P
    spike = np.zeros((33, P), np.uint8)
    spike[16] = 255                              # 0, 255, 0 at the lag 32: the largest R
    assert lag_words(br.rows_of(spike)[32])[32] == (0, 510 * P)
    assert 510 * br.MAX_PIXELS < 1 << 32 and 65025 * br.MAX_PIXELS < 1 << 32


def test_an_exact_linear_ramp():
    P, c, k = 11, 9, 3
    y = np.array([[c + k * t] * P for t in range(70)], np.uint8)
    rows = br.rows_of(y)
    for t in range(70):
        for L, (E, R) in lag_words(rows[t]).items():
            assert (E, R) == ((k * L * P, 0) if t >= L else (A, A))
    rows = br.rows_of(bc.planes("ramp", 70, 257))            # k = 1 + p % 3 per pixel
    k_sum = sum(1 + p % 3 for p in range(257))
    assert lag_words(rows[69]) == {L: (k_sum * L, 0) for L in br.LAGS} and int(rows[69, 3]) == k_sum


def test_a_ramp_with_rounding_stays_within_one_level_a_pixel():
    rng = np.random.default_rng(3)
    P = 300
    Aa, Bb = rng.integers(0, 256, P), rng.integers(0, 256, P)
    for D in (16, 32, 17):
        y = np.array([(Aa * (D - k) + Bb * k + D // 2) // D for k in range(D + 1)], np.uint8)
        rows = br.rows_of(y)
        for L in br.LAGS:
            for t in range(L, D + 1):
                E, R = lag_words(rows[t])[L]
                assert R <= P, (D, L, t, R)      # |2 r_m - r_a - r_t| <= 1: each rounding moves a value by at most 1/2
        if D in br.LAGS:
            assert lag_words(rows[D])[D][0] == int(np.abs(Aa - Bb).sum())


def test_luma_and_the_thumbnail_rule():
    f = np.zeros((4, 4, 3), np.uint8)
    f[..., 0], f[..., 1], f[..., 2] = 10, 200, 77
    assert br.plane(f, 2, 2).tolist() == [(77 * 10 + 150 * 200 + 29 * 77 + 128) >> 8] * 4
    assert br.luma_of(np.full((1, 1, 3), 255, np.uint8)).tolist() == [255]
    g = np.arange(48, dtype=np.uint8).reshape(4, 4, 3) * 5
    want = g.reshape(2, 2, 2, 2, 3).transpose(0, 2, 1, 3, 4).reshape(2, 2, 4, 3).astype(int).sum(2)
    assert br.plane(g, 2, 2).tolist() == br.luma_of((want + 2) // 4).tolist()         # 2 x 2 blocks, rounded half up
    assert br.tile_size(64, 1920, 1080) == (64, 36) == blend.tile_size(64, 1920, 1080)
    assert br.tile_size(32, 160, 90) == (32, 18) and br.tile_size(5, 1000, 10) == (5, 1)
    rows, luma = br.frame_rows([f, g], 2, 2)
    assert rows[:, 14].tolist() == [2 | 2 << 16] * 2 and luma.shape == (2, 4) and int(rows[1, 3]) == br.sad(luma[0], luma[1])


def test_rows_depend_on_the_planes_in_front_only():
    y = bc.planes("random", 70, 65)
    whole = br.rows_of(y)
    for N in bc.COUNTS:
        for first in bc.firsts(N):
            assert np.array_equal(br.rows_of(y[:N], first), whole[first:N])           # what lets the GPU tests share one reference
    assert br.rows_of(y[:0].reshape(0, 65)).shape == (0, 16)


# ---- planted defects ------------------------------------------------------------------------------------------------------------------
def differs(defect, planes):
    return not np.array_equal(br.rows_of(planes), br.rows_of(planes, defect=defect))


def test_the_comparison_sees_every_planted_defect():
    random5 = bc.planes("random", 70, 5)
    assert set(br.DEFECTS) == {"mid_off_by_one", "lag_swapped", "e_r_exchanged", "luma_floor", "tail_dropped", "history_reversed",
                               "no_sentinel", "s2_wraps"}
    for defect in ("mid_off_by_one", "lag_swapped", "e_r_exchanged", "tail_dropped", "no_sentinel"):
        assert differs(defect, random5), defect
    assert differs("mid_off_by_one", bc.planes("jump2", 70, 4)) and differs("lag_swapped", bc.planes("ramp", 70, 64))
    assert not differs("tail_dropped", bc.planes("random", 70, 64))                # a multiple of 4 has no tail: the odd sizes are needed
    for P in (1, 2, 3, 5, 63, 65, 255, 257, 16383):
        assert differs("tail_dropped", bc.planes("random", 33, P)), P
    assert np.array_equal(br.rows_of(random5, first=33), br.rows_of(random5, first=33, defect="no_sentinel"))      # seen below row 32 only
    # through the frames: the luma's rounding, and the order of the history
    frames = bc.frames_of(33, 21, 6)
    want, luma = br.frame_rows(frames, 16, 9)
    assert not np.array_equal(want, br.frame_rows(frames, 16, 9, defect="luma_floor")[0])
    hist = luma[:5]
    later = br.frame_rows(frames[5:], 16, 9, hist=hist)[0]
    assert np.array_equal(later, want[5:])                                        # carried history gives the rows of one call
    assert not np.array_equal(later, br.frame_rows(frames[5:], 16, 9, hist=hist, defect="history_reversed")[0])
    # S2 at the cap fits; beyond the cap a 32-bit sum wraps, which is why the cap is where it is
    top = np.full(br.MAX_PIXELS, 255, np.uint8)
    assert br.sums(top) == br.sums(top, "s2_wraps") == (255 * 16384, 65025 * 16384)
    beyond = np.full(70000, 255, np.uint8)
    assert br.sums(beyond)[1] == 65025 * 70000 > 1 << 32 and br.sums(beyond, "s2_wraps")[1] == 65025 * 70000 - (1 << 32)
    with pytest.raises(AssertionError):
        br.rows_of(beyond[None, :])


# ---- the transition rules on hand-made rows ---------------------------------------------------------------------------------------------
def hand_rows(n, P=100, fps=25.0, mean=100, var=400):
    """still rows: nothing moves, every sum present from its lag on, luma of the given mean and variance"""
    rows = np.zeros((n, 16), np.uint32)
    rows[:, 0] = P
    rows[:, 1] = mean * P
    rows[:, 2] = (var + mean * mean) * P
    for t in range(n):
        rows[t, 3] = 0 if t >= 1 else A
        for k, L in enumerate(br.LAGS):
            rows[t, 4 + 2 * k:6 + 2 * k] = (0, 0) if t >= L else (A, A)
    return br.stamp(rows, [t / fps for t in range(n)])


def both(rows, **kw):
    got = blend.analyse(rows, **kw)
    assert got == br.transitions(rows, **kw)
    assert blend.report(rows, got[0]) == br.report(rows, **kw)
    return got


def test_pass_marks_the_centre_and_the_narrowest_window_wins():
    rows = hand_rows(80)
    assert both(rows) == ([], [])
    P = 100
    rows[40, 8:10] = (4 * P, P)                  # lag 16 at t = 40: E / P = 4 = move, R / E = 0.25 = linear: passes at equality
    assert both(rows) == ([("dissolve", 24, 40)], [32])
    rows[40, 8:10] = (4 * P - 1, 0)
    assert both(rows) == ([], [])                # one below move
    rows[40, 8:10] = (4 * P, P + 1)
    assert both(rows) == ([], [])                # one above linear
    rows[40, 8:10] = (4 * P, P)
    rows[36, 6:8] = (4 * P, 0)                   # lag 8 at t = 36 has the same centre 32: the span is the narrower window's
    assert both(rows) == ([("dissolve", 28, 36)], [32])
    assert br.centre_halves(rows, 64, 64)[32] == 4 == blend.halves(rows, 64, 64)[32]
    rows[37, 6:8] = (4 * P, 0)                   # the next centre: one run, the union of the two windows
    assert both(rows)[0] == [("dissolve", 28, 37)]
    rows[60, 4:6] = (4 * P, 0)                   # lag 4, centre 58, span 56 .. 60: 0.16 s
    assert both(rows)[0] == [("dissolve", 28, 37), ("dissolve", 56, 60)]
    assert both(rows, min_duration=0.2)[0] == [("dissolve", 28, 37)]
    assert both(rows, move=4.1)[0] == [] and both(rows, linear=0.0)[0] == [("dissolve", 28, 37), ("dissolve", 56, 60)]
    rows[41, 4:6] = (4 * P, 0)                   # centre 39, span 37 .. 41 touches 28 .. 37: merged
    assert both(rows)[0][0] == ("dissolve", 28, 41)
    rows[41, 4:6] = (0, 0)
    rows[43, 4:6] = (4 * P, 0)                   # 39 .. 43: a pure frame 38 lies between, not merged
    assert both(rows)[0][:2] == [("dissolve", 28, 37), ("dissolve", 39, 43)]
    rows[2, 4:6] = (4 * P, 0)                    # a sum that cannot be there (t < L) is not read
    rows[3, 4:6] = (A, A)
    assert both(rows)[0][0] == ("dissolve", 28, 37)


def test_flat_frames_kinds_and_blank_runs():
    rows = hand_rows(80)
    P = 100
    black = slice(40, 50)
    rows[black, 1], rows[black, 2] = 0, 0
    assert both(rows) == ([("blank", 40, 49)], [])
    for var, flat in ((4, True), (5, False)):    # variance 4 = flat^2 at the default 2.0
        r = hand_rows(1, var=var)[0]
        assert br.is_flat(r, 32) is flat and blend.flat_frames(r[None, :], 32) == [flat]
    rows[40, 6:8] = (50 * P, 0)                  # lag 8: span 32 .. 40 ends on a flat frame
    rows[57, 6:8] = (50 * P, 0)                  # span 49 .. 57 starts on one
    found, cuts = both(rows)
    assert found == [("fade-out", 32, 40), ("blank", 40, 49), ("fade-in", 49, 57)] and cuts == [44]        # one cut for the run, not two
    assert both(rows, min_duration=0.5)[0] == [] and both(rows, min_duration=0.36)[0] == [("blank", 40, 49)]
    listed = blend.report(rows, found)
    assert listed[0] == {"kind": "fade-out", "start": 1.28, "end": 1.6, "first": 32, "last": 40}
    assert [d["first"] for d in listed] == sorted(d["first"] for d in listed)
    rows[:, 1], rows[:, 2] = 0, 0                # everything flat: a ramp between flat frames is a dissolve
    assert [f[0] for f in both(rows)[0]] == ["blank", "dissolve", "dissolve"]


# ---- the planted clip -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip():
    c = bc.planted_clip()
    tw, th = br.tile_size(bc.CLIP_WIDTH, bc.CLIP_W, bc.CLIP_H)
    return c, br.video_rows(c.frames, tw, th, bc.CLIP_FPS)


def test_the_planted_clip_gives_the_planted_spans_and_nothing_else(clip):
    c, rows = clip
    found, cuts = both(rows)
    spans = [f for f in found if f[0] != "blank"]
    assert [f[0] for f in spans] == [p.kind for p in c.plants] == ["dissolve", "fade-out", "fade-in"]
    for (kind, s, e), p in zip(spans, c.plants):
        assert abs(s - p.first) <= 1 and abs(e - p.last) <= 1, (kind, s, e, p)
    blanks = [f for f in found if f[0] == "blank"]
    assert len(blanks) == 1 and abs(blanks[0][1] - c.plants[1].last) <= 1 and blanks[0][2] == c.plants[2].first
    for what, a, b in c.quiet:                   # no span reaches into a still, the cut, the pan or the flash
        inside = [f for f in spans if f[1] < b and f[2] > a]
        assert not inside, (what, a, b, inside)
    assert {w for w, _, _ in c.quiet} == {"still", "cut", "pan", "flash"}
    assert cuts == [(spans[0][1] + spans[0][2]) // 2, (blanks[0][1] + blanks[0][2]) // 2]
    # the margins BLEND.md quotes: R / E inside the dissolve's passing windows, and on the pan
    _, pa, pb = [q for q in c.quiet if q[0] == "pan"][0]
    pan = [int(rows[t, 5 + 2 * k]) / float(rows[t, 4 + 2 * k]) for k, L in enumerate(br.LAGS) for t in range(pa + L, pb + 1)]
    assert min(pan) > 0.5
    d = c.plants[0]
    assert max(int(rows[t, 9]) / float(rows[t, 8]) for t in (d.last,)) < 0.1


def test_refined_tiles_the_shots_and_cuts_once_per_blank_run(clip, tmp_path):
    c, rows = clip
    fps, n = bc.CLIP_FPS, len(c.frames)
    cut_at = [q for q in c.quiet if q[0] == "cut"][0][2] / fps
    shots = [(0.0, cut_at), (cut_at, n / fps)]
    pieces = br.refined(rows, shots)
    d, fo, fi = c.plants
    assert len(pieces) == 4
    assert [a for a, _ in pieces[1:]] == [b for _, b in pieces[:-1]] and pieces[0][0] == 0.0 and pieces[-1][1] == n / fps
    assert d.first / fps < pieces[0][1] < d.last / fps               # inside the dissolve
    assert pieces[1][1] == cut_at
    assert fo.last / fps <= pieces[2][1] <= fi.first / fps           # inside the black, once
    assert blend.refine(shots, [int(rows[k, 12]) / 1000.0 for k in blend.analyse(rows)[1]]) == pieces
    assert blend.refine([(0.0, 1.0)], [0.0, 1.0, 2.0]) == [(0.0, 1.0)]            # only cuts strictly inside apply
    assert blend.refine([(0.0, 1.0), (3.0, 4.0)], [0.5, 2.0, 3.5, 3.5]) == [(0.0, 0.5), (0.5, 1.0), (3.0, 3.5), (3.5, 4.0)]
    # through the verb
    rows_path, shot_path, out, ref_path = (str(tmp_path / n) for n in ("blend.npy", "shot.json", "out.json", "refined.json"))
    np.save(rows_path, rows)
    with open(shot_path, "w") as fp:
        json.dump({"pyannote": "Timeline", "content": [{"start": a, "end": b} for a, b in shots]}, fp)
    assert cli.main(["transition", "--shots", shot_path, "--refined", ref_path, rows_path, out]) == 0
    assert json.load(open(out)) == br.report(rows)
    assert [(s.start, s.end) for s in cli.load_shots(ref_path)] == pieces


# ---- the verbs on a scripted context ----------------------------------------------------------------------------------------------------
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
    """frame_blend is the restatement; given: every frame an earlier call was given -- planes are carried, no frame is"""

    def __init__(self):
        self.live, self.calls, self.given = [], [], []

    def ingest_ring(self, h, w, depth=16):
        return Ring(self)

    def frame_blend(self, frames, tw, th, hist=None, want_luma=True):
        assert all(not f.released for f in frames), "a row asked of a released frame"
        assert all(f.released for f in self.given), "a frame of an earlier call is still resident"
        self.given.extend(frames)
        self.calls.append((len(frames), 0 if hist is None else len(hist)))
        return br.frame_rows([f.rgb for f in frames], tw, th, hist=hist)

    def mem_info(self):
        return 0, 0


class ClipVideo(object):
    def __init__(self, frames, fps):
        self.frames, self.frame_rate = frames, fps
        self.frame_size = self.size = (frames[0].shape[1], frames[0].shape[0])

    def __len__(self):
        return len(self.frames)

    def frame(self, i):
        return self.frames[i]

    def __iter__(self):
        for i, f in enumerate(self.frames):
            yield i / self.frame_rate, f


@pytest.fixture
def scripted(monkeypatch, clip):
    ctx = ScriptContext()
    videos = {"film": ClipVideo(clip[0].frames, bc.CLIP_FPS)}
    monkeypatch.setattr(runtime, "default_context", lambda: ctx)
    monkeypatch.setattr(cli, "open_video", lambda spec, fps, **kw: videos[spec])
    return ctx, videos


def test_both_verbs_through_main_equal_the_plain_loop(tmp_path, scripted, clip):
    ctx, videos = scripted
    c, want = clip
    n = len(c.frames)
    files = {}
    for batch in (1, 7, 64):
        ctx.calls[:] = []
        files[batch] = str(tmp_path / ("blend%d.npy" % batch))
        assert cli.main(["blend", "--width", str(bc.CLIP_WIDTH), "--batch", str(batch), "film", files[batch]]) == 0
        assert [k for k, _ in ctx.calls] == [batch] * (n // batch) + ([n % batch] if n % batch else [])
        assert [h for _, h in ctx.calls] == [min(32, i * batch) for i in range(len(ctx.calls))]      # the last 32 planes are carried
        assert all(f.released for f in ctx.live)
        got = np.load(files[batch])
        assert got.dtype == np.uint32 and np.array_equal(got, want), batch
    assert open(files[1], "rb").read() == open(files[7], "rb").read() == open(files[64], "rb").read()
    out = str(tmp_path / "out.json")
    assert cli.main(["transition", files[7], out]) == 0
    found = json.load(open(out))
    assert found == br.report(want) and [f["kind"] for f in found] == ["dissolve", "fade-out", "blank", "fade-in"]
    assert found[0] == {"kind": "dissolve", "start": round(c.plants[0].first / 25.0, 3), "end": round(c.plants[0].last / 25.0, 3),
                        "first": c.plants[0].first, "last": c.plants[0].last}
    # a range of the video: the rows start without history at --from
    assert cli.main(["blend", "--width", "32", "--from", "0.4", "--until", "2.0", "film", files[1]]) == 0
    part = np.load(files[1])
    assert np.array_equal(part, br.video_rows(c.frames[10:50], 32, 18, 25.0, first=10)) and part[0, 13] == 10 and part[0, 12] == 400
    assert cli.main(["transition", "--move", "8", "--linear", "0.1", "--flat", "1", "--min-duration", "0.3", files[7], "-"]) == 0


def test_the_carrier_hands_back_every_frame_it_was_given(clip):
    """measure -> (rows, the frames the caller may release now): all of them; ScriptContext checks at every call that none is left"""
    ctx = ScriptContext()
    carry = blend.Carry(ctx, 32, 18)
    frames = [Dev(f) for f in clip[0].frames[:7]]
    parts = []
    for part in (frames[:3], frames[3:6], frames[6:]):
        rows, done = carry.measure(part)
        assert len(rows) == len(part) and sorted(map(id, done)) == sorted(map(id, part))
        parts.append(rows)
        for f in done:
            f.release()
    assert ctx.calls == [(3, 0), (3, 3), (1, 6)] and all(f.released for f in frames)
    assert np.array_equal(np.concatenate(parts), br.frame_rows(clip[0].frames[:7], 32, 18)[0])


def test_a_stream_without_a_length_and_the_arguments(tmp_path, clip):
    c, want = clip

    class Stream(object):
        frame_rate, frame_size, size = bc.CLIP_FPS, (bc.CLIP_W, bc.CLIP_H), (bc.CLIP_W, bc.CLIP_H)

        def __iter__(self):
            for i, f in enumerate(c.frames[:45]):
                yield i / self.frame_rate, f
    ctx, out = ScriptContext(), str(tmp_path / "stream.npy")
    assert cli.blend(Stream(), out, width=32, batch=20, ctx=ctx) == {"frames": 45, "first": 0, "tw": 32, "th": 18}
    assert np.array_equal(np.load(out), want[:45]) and ctx.calls == [(20, 0), (20, 20), (5, 32)]
    a = cli.parse_args(["blend", "-", "blend.npy"])
    assert (a.video, a.output, a.width, a.t_from, a.t_until, a.batch) == ("-", "blend.npy", 64, 0.0, None, 64)
    a = cli.parse_args(["transition", "blend.npy", "out.json"])
    assert (a.rows, a.output, a.move, a.linear, a.flat, a.min_duration, a.shots, a.refined) == ("blend.npy", "out.json", 4.0, 0.25, 2.0, 0.12, None, None)


def test_refusals_with_a_message(tmp_path, scripted, capsys):
    good, bad, other = str(tmp_path / "good.npy"), str(tmp_path / "bad.npy"), str(tmp_path / "other.npy")
    np.save(good, np.zeros((0, 16), np.uint32))
    np.save(bad, np.zeros((3, 16), np.int32))
    np.save(other, np.zeros((3, 4), np.uint32))
    out = str(tmp_path / "out.json")
    for args, word in ((["transition", bad, out], "uint32 [n][16]"), (["transition", other, out], "uint32 [n][16]"),
                       (["transition", str(tmp_path / "missing.npy"), out], "not a blend file"),
                       (["transition", "--shots", good, good, out], "go together"), (["transition", "--move", "0", good, out], "--move"),
                       (["blend", "--batch", "0", "film", out], "--batch"), (["blend", "--width", "0", "film", out], "--width"),
                       (["blend", "--width", "400", "film", out], "at most 16384 pixels")):
        with pytest.raises(SystemExit):
            cli.main(args)
        assert word in capsys.readouterr().err, args
    assert cli.main(["transition", good, out]) == 0 and json.load(open(out)) == []
    with pytest.raises(ValueError, match="lower --width"):
        blend.Carry(None, 200, 100)
