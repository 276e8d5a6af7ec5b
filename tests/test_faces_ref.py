"""CPU: FACES.md on its restatement (tests/faces_ref.py) and on the host code of the `faces` verb (faces.py, the parser, cli.faces on a
scripted context).  Known values of the quality sums on contents whose sums can be worked out by hand, the properties a sharpness
measure and a resampled tile must have, that the comparison the GPU tests make sees each of a list of planted defects, the choice and
layout rules, the PPM bytes, and the verb's files against a plain loop."""
import itertools
import os

import numpy as np
import pytest

from tests import demo_ref, faces_ref as fr
from pyannote_video_amd import cli, faces, formats, pipeline, render

N = 148 * 148
CHIPS = fr.named_chips()


def V(chip, **kw):
    return fr.sharpness(fr.quality(chip, **kw))


# ---- the restatement alone ---------------------------------------------------------------------------------------------------------
def test_constants_agree_with_the_package_and_the_header():
    assert (faces.INTERIOR, faces.CHIP_PIXELS, faces.GAP, faces.BACKGROUND) == (fr.N, fr.PIXELS, fr.GAP, fr.BACKGROUND)
    assert [tuple(c) for c in demo_ref.PALETTE] == [tuple(c) for c in render.PALETTE]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvface.h")).read()
    for name, value in (("PVF_SHEET_MIN_TILE", faces.MIN_TILE), ("PVF_SHEET_MAX_TILE", faces.MAX_TILE), ("PVF_SHEET_MAX_SIDE", faces.MAX_SIDE),
                        ("PVF_SHEET_MAX_TILES", faces.MAX_TILES)):
        assert "#define %s %d " % (name, value) in hdr, name
    assert "#define PVF_SHEET_MAX_PIXELS (1 << 26)" in hdr and faces.MAX_PIXELS == 1 << 26


def test_known_values():
    assert V(CHIPS["black"]) == 0 and V(CHIPS["white"]) == 0 and V(CHIPS["ramp"]) == 275530416
    S1, S2, SY, ND, NB = fr.quality(CHIPS["checker"])
    assert S1 == 0 and S2 == 22788921600 and S2 > 1 << 32 and (SY, ND, NB) == (11250 * 255, 11250, 11250)
    assert fr.sharpness((S1, S2)) == N * S2 <= 5 * 10 ** 14
    S1, S2, SY, ND, NB = fr.quality(CHIPS["dot"])                  # (0, 5) is on the border ring: only (1, 5) sees it, as -255
    assert S1 == -255 and S2 == 65025 and fr.sharpness((S1, S2)) == 65025 * (N - 1) and (SY, ND, NB) == (255, 22499, 1)
    assert fr.quality(CHIPS["frame"])[0] == -150960                # 4 x 148 interior neighbours of the frame, the corners' none
    assert fr.quality(CHIPS["equal_luma_edge"])[:2] == (0, 0)      # a colour edge of equal luma is no edge
    assert fr.quality(CHIPS["black"])[3:] == (22500, 0) and fr.quality(CHIPS["white"])[3:] == (0, 22500)
    assert [fr.quality(CHIPS["y%d" % y])[3:] for y in (16, 17, 238, 239)] == [(22500, 0), (0, 0), (0, 0), (0, 22500)]
    assert fr.quality(CHIPS["round_at"])[2] == 22500 and fr.quality(CHIPS["round_below"])[2] == 0
    assert fr.quality(fr.grey(np.full((150, 150), 93)))[2] == 93 * 22500       # R = G = B = Y gives Y


def test_blur_and_upsampling_score_below_the_sharp_chip():
    noise = CHIPS["noise"].astype(np.int64)
    blurred = ((noise + np.roll(noise, 1, 0) + np.roll(noise, 1, 1) + np.roll(np.roll(noise, 1, 0), 1, 1) + 2) // 4).astype(np.uint8)
    upsampled = np.repeat(np.repeat(CHIPS["noise"][:75, :75], 2, axis=0), 2, axis=1)
    assert 0 < V(blurred) < V(CHIPS["noise"]) and 0 < V(upsampled) < V(CHIPS["noise"])
    assert fr.score(fr.quality(blurred), 1.0) < fr.score(fr.quality(CHIPS["noise"]), 1.0)


@pytest.mark.parametrize("S", [48, 149, 150, 151, 600])
def test_tiles(S):
    for name in ("noise", "ramp", "checker"):
        t = fr.tile(CHIPS[name], S)
        assert t.shape == (S, S, 3) and t.min() >= CHIPS[name].min() and t.max() <= CHIPS[name].max()
        if S == 150:
            assert np.array_equal(t, CHIPS[name])
    assert np.array_equal(fr.tile(CHIPS["y17"], S), np.full((S, S, 3), 17, np.uint8))
    corners = fr.tile(CHIPS["noise"], S)
    if S >= 150:                                                    # the clamp: the outermost samples are the chip's own border pixels
        assert np.array_equal(corners[0, 0], CHIPS["noise"][0, 0]) and np.array_equal(corners[-1, -1], CHIPS["noise"][-1, -1])


def test_sheet_composition_rules():
    a, b = CHIPS["noise"], CHIPS["ramp"]
    img = fr.sheet([a, b, a], [(-10, 3), (20, 10), (400, 0)], 48, 90, 70, (1, 2, 3), [(demo_ref.RECT, 5, 5, 30, 30, (9, 9, 9))])
    ta, tb = fr.tile(a, 48), fr.tile(b, 48)
    assert np.array_equal(img[60, 80], (1, 2, 3))                                   # background
    assert np.array_equal(img[3, 0], ta[0, 10]) and np.array_equal(img[50, 10], ta[47, 20])      # clipped at the left edge
    assert np.array_equal(img[12, 25], tb[2, 5])                                    # the later tile over the earlier one
    assert np.array_equal(img[5, 10], (9, 9, 9)) and np.array_equal(img[30, 30], (9, 9, 9))      # primitives over tiles
    assert np.array_equal(fr.sheet([], [], 48, 5, 4, (7, 8, 9)), np.tile(np.array([7, 8, 9], np.uint8), (4, 5, 1)))


# ---- the comparison sees planted defects -------------------------------------------------------------------------------------------
def test_planted_defects_are_visible():
    """each defect changes what the GPU tests compare, on the contents those tests use"""
    chips = list(CHIPS.values())
    good = fr.qualities(chips)
    seen = {}
    for name, kw in (("border", dict(border=True)), ("s2_32bit", dict(bits32=True)), ("no_rounding", dict(rounding=False)), ("dark_strict", dict(dark_strict=True))):
        bad = fr.qualities(chips, **kw)
        seen[name] = [k for k, g, b in zip(CHIPS, good, bad) if not np.array_equal(g, b)]
        assert seen[name], name
    assert "dot" in seen["border"] and "frame" in seen["border"]                    # the ring is live
    assert seen["s2_32bit"] == ["checker", "stripes_v", "stripes_h"]               # the only sums beyond 2^32
    assert "round_at" in seen["no_rounding"] and "y16" in seen["dark_strict"] and "y17" not in seen["dark_strict"]
    for S in (151, 600):                                                            # u = 150 - S < 0 in the first column and row
        assert not np.array_equal(fr.tile(CHIPS["noise"], S), fr.tile(CHIPS["noise"], S, clamp=False)), S
    for S in (48, 149, 150):                                                        # 0 < 150 - S and 299 S - 150 <= 298 S: never at the clamp
        assert np.array_equal(fr.tile(CHIPS["noise"], S), fr.tile(CHIPS["noise"], S, clamp=False)), S
    args = ([CHIPS["noise"], CHIPS["ramp"]], [(0, 0), (20, 10)], 48, 80, 70)
    assert not np.array_equal(fr.sheet(*args), fr.sheet(*args, first_wins=True))


# ---- host rules ------------------------------------------------------------------------------------------------------------------
def _pts(nose, left, right):
    p = np.zeros((68, 2), np.int32)
    p[30], p[2], p[14] = nose, left, right
    return p


def test_symmetry():
    assert faces.symmetry(_pts((50, 60), (20, 60), (80, 60))) == 1.0
    assert faces.symmetry(_pts((50, 60), (20, 60), (80, 60))) == faces.symmetry(_pts((50, 60), (80, 60), (20, 60)))      # mirrored
    assert faces.symmetry(_pts((5, 5), (5, 5), (5, 5))) == 0.0                      # degenerate: both distances 0
    assert faces.symmetry(_pts((20, 60), (20, 60), (80, 60))) == 0.0                # the nose on the jaw: full profile
    prof = faces.symmetry(_pts((30, 60), (20, 60), (80, 60)))
    assert prof == (100 / 2500) ** 0.5 == 0.2
    rng = np.random.default_rng(3)
    for _ in range(50):
        p = rng.integers(-2000, 4000, (68, 2)).astype(np.int32)
        assert faces.symmetry(p) == fr.symmetry(p) and 0.0 <= faces.symmetry(p) <= 1.0


def test_score_and_eligibility_equal_the_restatement():
    for name, chip in CHIPS.items():
        q = fr.quality(chip)
        assert faces.sharpness(q) == fr.sharpness(q) >= 0
        assert faces.score(q, 0.37) == fr.score(q, 0.37)
    q = [0, 0, 0, 5625, 5625]
    assert faces.eligible(q, 10, 100) and fr.eligible(q, 10, 100)
    assert not faces.eligible([0, 0, 0, 5626, 0], 10, 100) and not faces.eligible([0, 0, 0, 0, 5626], 10, 100)
    assert faces.eligible(q, 20, 100, min_size=0.2) and not faces.eligible(q, 19, 100, min_size=0.2)
    assert faces.eligible([0, 0, 0, 22500, 0], 1, 100, max_dark=1.0) and not faces.eligible([0, 0, 0, 1, 0], 1, 100, max_dark=0.0)


def test_choose():
    F = [(5.0, 0.0, 1, True), (9.0, 0.4, 1, True), (8.0, 0.8, 1, True), (7.0, 3.0, 1, True), (99.0, 5.0, 1, False), (7.0, 2.0, 2, True)]
    assert faces.choose(F, 1) == [1]
    assert faces.choose(F, 2, spread=1.0) == [1, 5]                  # 2 (0.8) is within a second of 1 (0.4): passed over; 5 before 3: the earlier time
    assert faces.choose(F, 3, spread=1.0) == [1, 5, 3]
    assert faces.choose(F, 5, spread=1.0) == [1, 5, 3, 4, 2]         # 4 is ineligible but far from everything; 2 and 0 fill up in rank order
    assert faces.choose(F, 6, spread=1.0) == [1, 5, 3, 4, 2, 0] and faces.choose(F, 60, spread=1.0) == [1, 5, 3, 4, 2, 0]
    assert faces.choose(F, 3, spread=0.0) == [1, 2, 5]               # no spread: plain rank order; the tie 3 / 5 goes to the earlier time
    assert faces.choose([(1.0, 0.0, 7, False), (0.5, 9.0, 7, False)], 2) == [0, 1]        # a group never comes up empty
    assert faces.choose([(1.0, 1.0, 9, True), (1.0, 1.0, 3, True)], 2) == [1, 0]          # score and time tie: the smaller track
    assert faces.choose([], 4) == []
    rng = np.random.default_rng(11)
    for trial in range(200):
        n = int(rng.integers(1, 30))
        G = [(float(rng.integers(0, 5)), float(rng.integers(0, 40)) / 4, int(rng.integers(0, 3)), bool(rng.integers(0, 4))) for _ in range(n)]
        for K, spread in itertools.product((1, 4, 9), (0.0, 1.0, 2.5)):
            got = faces.choose(G, K, spread)
            assert got == fr.choose(G, K, spread) and len(got) == min(K, n) == len(set(got))


def _boxes(W, H, corners, prims, S):
    out = []
    for c in corners:
        for x, y in c:
            out.append((x - 2, y - 2, x + S + 1, y + S + 1))         # a tile with its outline
    for p in prims:
        if p[0] == render.PRIM_TEXT:
            out.append((p[1], p[2] - 7 * p[4] + 1, p[1] + 6 * p[4] * len(p[5]) - 1, p[2]))
    return out


@pytest.mark.parametrize("K,S,columns,n", [(4, 150, 1, 3), (1, 48, 1, 1), (3, 64, 4, 9), (2, 600, 2, 3), (5, 97, 3, 30)])
def test_layout(K, S, columns, n):
    groups = [("name-%d-with-a-long-tail-that-must-be-cut-to-fit-its-panel-and-the-run-cap-of-64-bytes" % g, g * 7, 1 + (g * 5) % (K + 2)) for g in range(n)]
    W, H, corners, prims = faces.layout(groups, K, S, columns)
    assert (W, H, corners) == fr.layout(groups, K, S, columns)[:3]
    want = fr.layout(groups, K, S, columns)[3]
    assert [(p[0], p[1], p[2]) + tuple(p[3:]) for p in prims] == [(q[0], q[1], q[2]) + tuple(q[3:]) for q in want]
    assert [len(c) for c in corners] == [min(g[2], K) for g in groups]              # a partial group leaves background
    assert sum(1 for p in prims if p[0] == render.PRIM_RECT) == sum(len(c) for c in corners) and sum(1 for p in prims if p[0] == render.PRIM_TEXT) == n
    boxes = _boxes(W, H, corners, prims, S)
    for l, t, r, b in boxes:
        assert 0 <= l <= r < W and 0 <= t <= b < H
    for (a, b) in itertools.combinations(boxes, 2):
        assert a[2] < b[0] or b[2] < a[0] or a[3] < b[1] or b[3] < a[1], (a, b)
    for p in prims:
        if p[0] == render.PRIM_TEXT:
            assert p[4] == max(1, S // 48) and 1 <= len(p[5]) <= 64
    _, packed, _ = render.pack_primitives([prims])                                  # what the sheet call is handed
    assert len(packed) == len(prims)
    assert faces.default_columns(1) == 1 and faces.default_columns(24) == 1 and faces.default_columns(25) == 2 and faces.default_columns(49) == 3


def test_ppm_header_and_bytes():
    img = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    assert faces.ppm_bytes(img) == b"P6\n3 2\n255\n" + bytes(range(18)) == fr.ppm(img)
    with pytest.raises(ValueError):
        faces.ppm_bytes(np.zeros((2, 3), np.uint8))


# ---- the verb on a scripted context ---------------------------------------------------------------------------------------------------
class ScriptVideo(object):
    def __init__(self, n, w=64, h=48, fps=25.0):
        self.n, self.frame_size, self.size, self.frame_rate = n, (w, h), (w, h), fps

    def __len__(self):
        return self.n

    def _frame(self, i):
        w, h = self.frame_size
        a = np.zeros((h, w, 3), np.uint8)
        a[0, 0, 0], a[0, 0, 1] = i // 256, i % 256
        return a

    def __iter__(self):
        for i in range(self.n):
            yield i / self.frame_rate, self._frame(i)


class SeekVideo(ScriptVideo):
    def frame(self, i):
        return self._frame(i)


class Dev(object):
    def __init__(self, i):
        self.i, self.released = i, False

    def release(self):
        assert not self.released
        self.released = True


class Ring(object):
    def __init__(self, log):
        self.log = log

    def push(self, rgb):
        d = Dev(int(rgb[0, 0, 0]) * 256 + int(rgb[0, 0, 1]))
        self.log.append(d)
        return d

    def close(self):
        pass


def script_quality(i, pts):
    """five sums that depend on the frame and the points, with a spread of scores and some ineligible faces"""
    k = int(pts[30, 0]) * 31 + int(pts[2, 1]) * 17 + i
    return [-(k % 97), 10 ** 6 + (k * 7919) % 10 ** 7, k % 1000, 9000 if k % 5 == 0 else k % 300, k % 200]


class ScriptContext(object):
    def __init__(self, fail_at=None):
        self.calls, self.frames, self.sheets, self.fail_at = [], [], [], fail_at

    def ingest_ring(self, h, w, depth=16):
        return Ring(self.frames)

    def face_quality(self, frames, pts):
        self.calls.append(len(pts))
        if self.fail_at is not None and len(self.calls) > self.fail_at:
            raise RuntimeError("scripted device error")
        assert all(not f.released for f in frames), "quality asked of a released frame"
        return np.array([script_quality(f.i, p) for f, p in zip(frames, pts)], np.int64).reshape(-1, 5)

    def face_sheet(self, frames, pts, xy, S, W, H, background, prims):
        assert all(not f.released for f in frames), "a sheet asked of a released frame"
        self.sheets.append(([f.i for f in frames], np.array(pts), list(xy), S, W, H, background, list(prims)))
        img = np.zeros((H, W, 3), np.uint8)
        img[:, :] = background
        for f, (x, y) in zip(frames, xy):
            img[y, x] = (f.i % 256, 1, 2)
        return img


def make_inputs(tmp_path, n_frames=60, fps=25.0):
    from tests.test_cli_host import make_tracks
    tp, lp = str(tmp_path / "track.txt"), str(tmp_path / "landmarks.txt")
    formats.write_tracks(tp, make_tracks(n_frames, fps))
    rows = formats.read_tracks(tp)
    times = [i / fps for i in range(n_frames)]
    rng = np.random.default_rng(5)
    with open(lp, "wb") as f:
        for fi, T, g in pipeline.faces_per_frame(rows, times, 64, 48):
            for ident, box in g:
                pts = rng.integers(0, 48, (1, 68, 2)).astype(np.int32)
                f.write(formats.landmark_rows([T], [ident], pts, 64, 48))
    return tp, lp


def plain_loop(video, tp, lp, per, spread, labels=None, only=None, **elig):
    """the files of the verb by a loop over the landmark file: no threads, no batches"""
    w, h = video.frame_size
    rows = formats.read_tracks(tp)
    times = [i / video.frame_rate for i in range(len(video))]
    where = {}
    for fi, T, g in pipeline.faces_per_frame(rows, times, w, h):
        for ident, box in g:
            where[("%.3f" % T, ident)] = (fi, box)
    F, quality = [], []
    for T, ident, pts in formats.read_landmarks(lp):
        p = np.array(pts, np.float32)
        p[:, 0] = np.round(p[:, 0] * w)
        p[:, 1] = np.round(p[:, 1] * h)
        p = p.astype(np.int32)
        fi, box = where[("%.3f" % T, ident)]
        q = script_quality(fi, p)
        sym = fr.symmetry(p)
        ok = fr.eligible(q, box[3] - box[1], h, **elig)
        F.append((T, ident, fi, q, sym, fr.score(q, sym), ok))
        quality.append("%.3f %d %d %d %d %d %d %.5f %.5f %d\n" % (T, ident, q[0], q[1], q[2], q[3], q[4], sym, fr.score(q, sym), int(ok)))
    names = {}
    for i, f in enumerate(F):
        names.setdefault((labels or {}).get(f[1]) or "#%d" % f[1], []).append(i)
    order = sorted(names, key=lambda n: (min(F[i][1] for i in names[n]), n))
    if only is not None:
        order = [n for n in order if n in only or n.lstrip("#") in only]
    index, shown = [], []
    for n in order:
        idx = names[n]
        pick = fr.choose([(F[i][5], F[i][0], F[i][1], F[i][6]) for i in idx], per, spread)
        shown.append((n, min(F[i][1] for i in idx), [idx[k] for k in pick]))
        for rank, k in enumerate(pick):
            index.append("%s %d " % (n, rank) + quality[idx[k]])
    return "".join(quality), "".join(index), shown, F


@pytest.mark.parametrize("batch,video_class", [(1, ScriptVideo), (7, SeekVideo), (2048, ScriptVideo)])
def test_faces_verb_files_equal_the_plain_loop(tmp_path, batch, video_class):
    video = video_class(60)
    tp, lp = make_inputs(tmp_path)
    labels = {0: "ann", 2: "ann", 3: "7"}
    want_q, want_i, shown, F = plain_loop(video, tp, lp, 3, 0.2, labels, max_dark=0.3)
    assert want_q.count("\n") > 50 and " 0\n" in want_q and " 1\n" in want_q       # eligible and ineligible faces both occur
    ctx = ScriptContext()
    out, ip, qp = str(tmp_path / "sheet.npy"), str(tmp_path / "index.txt"), str(tmp_path / "quality.txt")
    res = cli.faces(video, tp, lp, out, per=3, tile=48, label=labels, spread=0.2, max_dark=0.3, index=ip, quality=qp, ctx=ctx, batch=batch, ahead=4)
    assert open(qp).read() == want_q and open(ip).read() == want_i
    assert res["groups"] == [n for n, _, _ in shown] and "ann" in res["groups"] and "#1" in res["groups"] and "7" in res["groups"]
    assert res["faces"] == len(F) and res["shown"] == sum(len(s) for _, _, s in shown)
    (frames, pts, xy, S, W, H, background, prims), = ctx.sheets                     # ONE sheet call
    W2, H2, corners, want_prims = fr.layout([(n, c, len(s)) for n, c, s in shown], 3, 48, 1)
    assert (S, W, H, background) == (48, W2, H2, fr.BACKGROUND) and xy == [c for g in corners for c in g]
    assert frames == [F[i][2] for _, _, s in shown for i in s]
    assert [tuple(p[:3]) + tuple(p[3:]) for p in prims] == [tuple(q[:3]) + tuple(q[3:]) for q in want_prims]
    img = np.load(out)
    assert img.shape == (H, W, 3) and all(np.array_equal(img[y, x], (f % 256, 1, 2)) for f, (x, y) in zip(frames, xy))
    assert all(d.released for d in ctx.frames) and len(ctx.frames) > 0             # both passes gave their frames back
    if batch == 2048:
        assert len(ctx.calls) == 1
    if batch == 1:
        assert len(ctx.calls) >= want_q.count("\n") // 5
    if video_class is SeekVideo:                                                    # pass 2 reads the chosen frames only
        assert len(ctx.frames) == len(set(F[i][2] for i in range(len(F)))) + len(set(frames))


def test_faces_verb_options_and_ppm_output(tmp_path):
    video = SeekVideo(60)
    tp, lp = make_inputs(tmp_path)
    _, want_i, shown, F = plain_loop(video, tp, lp, 2, 1.0, None, {"#1", "3"})
    ctx = ScriptContext()
    out, ip = str(tmp_path / "sheet.ppm"), str(tmp_path / "index.txt")
    res = cli.faces(video, tp, lp, out, per=2, tile=64, only={"#1", "3"}, index=ip, ctx=ctx)
    assert res["groups"] == ["#1", "#3"] == [n for n, _, _ in shown] and open(ip).read() == want_i
    data = open(out, "rb").read()
    head = b"P6\n%d %d\n255\n" % (res["width"], res["height"])
    assert data.startswith(head) and len(data) == len(head) + res["width"] * res["height"] * 3
    # --from / --until: only faces inside the window are shown
    cli.faces(video, tp, lp, out, per=50, tile=48, t_from=0.4, t_until=0.8, index=ip, ctx=ScriptContext())
    times = [float(line.split()[2]) for line in open(ip)]
    assert times and all(0.4 <= t < 0.8 for t in times)
    with pytest.raises(ValueError, match="no face to show"):
        cli.faces(video, tp, lp, out, only={"nobody"}, ctx=ScriptContext())


def test_faces_verb_hands_on_errors_and_refuses(tmp_path, capsys):
    video = ScriptVideo(60)
    tp, lp = make_inputs(tmp_path)
    ctx = ScriptContext(fail_at=2)
    with pytest.raises(RuntimeError, match="scripted device error"):
        cli.faces(video, tp, lp, str(tmp_path / "s.ppm"), ctx=ctx, batch=5, ahead=2)
    assert all(d.released for d in ctx.frames) and len(ctx.frames) > 0              # every frame the reader had staged was given back
    with pytest.raises(ValueError, match=r"--tile.*--per.*--only"):                 # 5 tracks x 600-pixel tiles x 30 a row: beyond 16384
        cli.faces(video, tp, lp, str(tmp_path / "s.ppm"), per=30, tile=600, ctx=ScriptContext())
    with pytest.raises(ValueError, match=r"\.ppm or \.npy"):
        cli.faces(video, tp, lp, str(tmp_path / "s.png"), ctx=ScriptContext())
    with pytest.raises(ValueError, match="--tile is 48 .. 600"):
        cli.faces(video, tp, lp, str(tmp_path / "s.ppm"), tile=47, ctx=ScriptContext())
    with pytest.raises(ValueError, match="--tile.*--per.*--only"):
        faces.check_sheet(100, 100, 5000, 5000)
    faces.check_sheet(16384, 4096, 65536, 4096)                                     # the caps themselves pass
    with pytest.raises(SystemExit):                                                 # the video cannot be read twice from a pipe
        cli.main(["faces", "-", tp, lp, str(tmp_path / "s.ppm")])
    assert "reads the video twice" in capsys.readouterr().err


def test_parser_defaults():
    a = cli.parse_args(["faces", "v.y4m", "t.txt", "l.txt", "-"])
    assert (a.per, a.tile, a.columns, a.label, a.only, a.spread, a.min_size, a.max_dark, a.max_bright, a.t_from, a.t_until, a.index, a.quality) == \
        (4, 150, None, None, None, 1.0, 0.0, 0.25, 0.25, 0.0, None, None, None)
    a = cli.parse_args(["faces", "--per", "2", "--tile", "96", "--columns", "3", "--only", "ann,#4", "--from", "1", "--until", "2.5", "v", "t", "l", "o.npy"])
    assert (a.per, a.tile, a.columns, a.only, a.t_from, a.t_until, a.output) == (2, 96, 3, {"ann", "#4"}, 1.0, 2.5, "o.npy")
