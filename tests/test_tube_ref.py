"""CPU: TUBE.md on its restatement (tests/tube_ref.py) and on the host code of the `tube` verb (tube.py, the parser, cli.tube on a
scripted context).  Worked values whose sums can be found by hand, that the comparison the GPU tests make sees each of a list of
planted defects, the host rules on hand-made tracks, and the verb's files against a plain loop."""
import os

import numpy as np
import pytest

from tests import tube_ref as tr
from tests.test_faces_ref import Ring, ScriptVideo, make_inputs
from pyannote_video_amd import cli, faces as _faces, formats, pipeline, tube

FRAME = tr.picture(37, 50, 1)


# ---- the restatement alone ---------------------------------------------------------------------------------------------------------
def test_constants_agree_with_the_package_and_the_header():
    assert (tube.MIN_SIZE, tube.MAX_SIZE, tube.MIN_SIDE, tube.MAX_SIDE, tube.MAX_COORD, tube.MAX_CROPS) == \
        (tr.MIN_SIZE, tr.MAX_SIZE, tr.MIN_SIDE, tr.MAX_SIDE, tr.MAX_COORD, tr.MAX_CROPS) == (1, 1024, 16, 1 << 18, 1 << 30, 65536)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvface.h")).read()
    for name, text in (("MIN_SIZE", "1"), ("MAX_SIZE", "1024"), ("MIN_SIDE", "16"), ("MAX_SIDE", "(1 << 18)"), ("MAX_COORD", "(1 << 30)"),
                       ("MAX_CROPS", "65536"), ("YUV420", "4")):
        assert "#define PVF_CROP_%s %s " % (name, text) in hdr, name
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyannote-video_amd", "csrc", "tube.hip")).read()
    for name, v in (("C_COLS", tr.C_COLS), ("C_BAND", tr.C_BAND), ("C_TILE_PX", tr.C_TILE_PX)):
        assert "constexpr int %s = %d;" % (name, v) in src, name
    # the caps' overflow arguments (TUBE.md "Caps")
    assert tr.MAX_SIDE * 255 < 2 ** 31 and tr.MAX_SIDE ** 2 * 255 + tr.MAX_SIDE ** 2 // 2 < 2 ** 63 and tr.MAX_SIDE ** 2 * 255 >= 2 ** 32
    assert 1024 * tr.MAX_SIZE ** 2 * 255 >= 2 ** 32 and 15 * tr.MAX_SIZE + tr.MAX_SIZE * tr.MAX_SIDE + 32 * tr.MAX_SIZE < 2 ** 31
    assert tr.MAX_SIZE * tr.MAX_COORD >= 2 ** 31                     # why S X0 is never formed


def test_identity_and_aligned_windows_return_the_source_bytes():
    assert np.array_equal(tr.crop(FRAME, (0, 0, 16 * 37), 37), FRAME[:37, :37])
    assert np.array_equal(tr.crop(FRAME, (16 * 5, 16 * 3, 16 * 20), 20), FRAME[3:23, 5:25])
    got = tr.crop(FRAME, (16 * 40, 16 * 30, 16 * 20), 20)           # past the right and bottom edges: black
    assert np.array_equal(got[:7, :10], FRAME[30:, 40:]) and not got[7:].any() and not got[:, 10:].any()


def test_aligned_two_to_one_reduction():
    got = tr.crop(FRAME, (16 * 4, 16 * 2, 16 * 24), 12)
    f = FRAME.astype(np.int64)
    for r, c in ((0, 0), (5, 7), (11, 11)):
        y, x = 2 + 2 * r, 4 + 2 * c
        assert got[r, c].tolist() == ((f[y, x] + f[y, x + 1] + f[y + 1, x] + f[y + 1, x + 1] + 2) // 4).tolist()


def test_constant_frames_inside_and_half_off():
    const = np.full((40, 60, 3), (201, 7, 90), np.uint8)
    for win, S in (((37, 21, 16 * 9 + 5), 9), ((16, 16, 16 * 20 - 3), 7), ((100, 50, 100), 13), ((19, 21, 16), 4), ((0, 0, 16 * 40), 3)):     # (enlarging: half a pixel from the edges)
        assert (tr.crop(const, win, S) == np.array((201, 7, 90))).all(), (win, S)
    # the left half of the window off the frame: every output pixel sees half its weight, (v L^2 / 2 + L^2 // 2) // L^2 = (v + 1) // 2
    # for even L (rounding half up: 201 -> 101, 7 -> 4, 90 -> 45)
    got = tr.crop(const, (-16 * 10, 16 * 4, 16 * 20), 1)
    assert got.reshape(3).tolist() == [101, 4, 45]
    # enlarging, one pixel left of the frame's first column centre: the tap at -1 is black, not the edge pixel
    got = tr.crop(const, (-16, 16, 32), 4)
    # (u = -160, -96, -32, 32 in 1 / 128 pixel: taps (-2, -1), (-1, 0) with fx = 32, (-1, 0) with fx = 96, (0, 1))
    assert got[0, 0].tolist() == [0, 0, 0] and got[0, 1].tolist() == [(201 + 2) // 4, (7 + 2) // 4, (90 + 2) // 4]
    assert got[0, 2].tolist() == [(201 * 3 + 2) // 4, (7 * 3 + 2) // 4, (90 * 3 + 2) // 4] and got[0, 3].tolist() == [201, 7, 90]


def test_one_pixel_window_enlarged():
    S, (y, x) = 4, (10, 20)
    got = tr.crop(FRAME, (16 * x, 16 * y, 16), S)
    f = FRAME.astype(np.int64)
    # u = 2 S X0 + (2 j + 1) L - 16 S: the samples lie at (2 j + 1) / 8 - 1 / 2 of the pixel: -3/8, -1/8, 1/8, 3/8 from its centre
    for j, (x0, fx) in enumerate(((x - 1, 80), (x - 1, 112), (x, 16), (x, 48))):
        for i, (y0, fy) in enumerate(((y - 1, 80), (y - 1, 112), (y, 16), (y, 48))):
            want = ((128 - fx) * (128 - fy) * f[y0, x0] + fx * (128 - fy) * f[y0, x0 + 1] + (128 - fx) * fy * f[y0 + 1, x0] +
                    fx * fy * f[y0 + 1, x0 + 1] + 512 * 16) // (1024 * 16)
            assert got[i, j].tolist() == want.tolist()


def test_the_seam():
    S = 5
    f = FRAME.astype(np.int64)
    for fy in range(16):
        for fx in range(16):
            X0, Y0 = 16 * 3 + fx, 16 * 2 + fy
            at = tr.crop(FRAME, (X0, Y0, 16 * S), S)
            # both regimes evaluated at L = 16 S
            tx, ty = tr.enlarge_weights(X0, 16 * S, S, 50), tr.enlarge_weights(Y0, 16 * S, S, 37)
            for (i, j) in ((0, 0), (2, 3), (4, 4)):
                num = sum(wy * wx * f[y, x] for y, wy in ty[i] for x, wx in tx[j])
                assert ((num + 512 * S * S) // (1024 * S * S)).tolist() == at[i, j].tolist()
                b = f[2 + i:4 + i, 3 + j:5 + j]
                want = ((16 - fx) * (16 - fy) * b[0, 0] + fx * (16 - fy) * b[0, 1] + (16 - fx) * fy * b[1, 0] + fx * fy * b[1, 1] + 128) // 256
                assert want.tolist() == at[i, j].tolist()
            for L in (16 * S - 1, 16 * S + 1):                       # one sixteenth of a pixel over five pixels: no byte moves by more than a few
                d = np.abs(tr.crop(FRAME, (X0, Y0, L), S).astype(int) - at.astype(int))
                assert d.max() <= 24, (fx, fy, L, d.max())
    assert np.array_equal(tr.crop(FRAME, (48, 32, 16 * S), S), FRAME[2:7, 3:8])


def test_weights_sum_to_the_side():
    for P0, L, S in ((0, 160, 10), (-77, 1000, 7), (5, 16 * 9 + 1, 9), (123456, tr.MAX_SIDE, 3), (-tr.MAX_COORD, 5000, 63), (3, 16, 1)):
        assert all(sum(w for _, w in t) == L for t in tr.reduce_weights(P0, L, S, 1 << 40, clamp=True))
        assert all(w > 0 for t in tr.reduce_weights(P0, L, S, 1 << 40, clamp=True) for _, w in t)
    for P0, L, S in ((0, 16, 10), (-77, 100, 7), (5, 16 * 9 - 1, 9)):
        assert all(sum(w for _, w in t) == 32 * S for t in tr.enlarge_weights(P0, L, S, 1 << 40, clamp=True))


def test_quotient_by_float_estimate_is_exact(tmp_path):
    """crop_k divides by L^2 or 1024 S^2 through a float estimate and the exact residual (tests/csrc/crop_quotient_check.c)"""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "crop_quotient_check")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "crop_quotient_check.c")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-400:]
    assert " 0 differ" in out.stdout


def test_yuv_form():
    rgb = tr.crop(FRAME, (9, 4, 400), 7)
    yuv = tr.to_yuv(rgb, "709", True)
    assert yuv.shape == (49 + 2 * 16,)
    black = tr.crops([FRAME], [(tr.MAX_COORD, 0, 160)], 6, "yuv420")[0]
    assert black[:36].tolist() == [16] * 36 and black[36:].tolist() == [128] * 18


def test_planted_defects_are_visible():
    """each defect changes what the GPU tests compare, on the frames and windows those tests use"""
    frames = [tr.picture(61, 97, 2), tr.picture(61, 97, 3)]
    S = 9
    cases = tr.window_cases(61, 97, S)
    cases["large"] = (-16 * 150, -16 * 170, 6400)                     # an output pixel of 44 x 44 source pixels inside the frame: its sum passes 2^32
    good = dict((k, tr.crops(frames, [w, w], S)) for k, w in cases.items())
    good_yuv = dict((k, tr.crops(frames, [w, w], S, "yuv420")) for k, w in cases.items())

    def seen(layout="rgb", **kw):
        ref = good if layout == "rgb" else good_yuv
        return [k for k, w in cases.items() if not np.array_equal(tr.crops(frames, [w, w], S, layout, **kw), ref[k])]
    assert "seam_above" in seen(rounding=False) and "enlarge" in seen(rounding=False)
    assert "seam_above" in seen(last_off=1) and "reduce" in seen(last_off=-1)
    s = seen(clamp=True)
    assert "cross_left" in s and "corner_br" in s and "outside_top" in s and "identity" not in s
    s = seen(swap=True)
    assert "seam_below" in s and "seam_above" in s and "seam" not in s and "identity" not in s
    s = seen(truncate=True)
    assert "one_pixel" not in s                                      # positive u: the same
    neg = (-16 * 2 + 3, -16 * 1, 16 * 4)                             # enlarging across the top-left corner: u < 0 for the first samples
    assert not np.array_equal(tr.crop(frames[0], neg, S, truncate=True), tr.crop(frames[0], neg, S))
    s = seen(wrap32=True)
    assert "large" in s and "dwarf" in s and "identity" not in s and "seam" not in s
    assert "identity" in seen("yuv420", wrong_chroma=True) and "reduce" in seen("yuv420", wrong_chroma=True)
    assert "identity" in seen(neighbour=True) and "last_pixel" in seen(neighbour=True)


# ---- host rules ------------------------------------------------------------------------------------------------------------------
def test_regions_and_quantisation():
    assert tube.face_region((10, 20, 50, 80)) == (30.0, 50.0, 1.6 * 60.0) and tube.face_region((11, 20, 50, 40), 2.0) == (30.5, 30.0, 78.0)
    pts = np.zeros((68, 2), np.int32)
    pts[48:68] = [(100 + k, 200 + (k % 3)) for k in range(20)]
    pts[:48] = 999
    assert tube.mouth_region((10, 20, 50, 80), pts) == (109.5, (200 * 20 + 7 + 6 * 2) / 20.0, 30.0)
    assert tube.quantise(30.0, 50.0, 96.0) == (16 * 30 - 768, 16 * 50 - 768, 1536)
    assert tube.quantise(30.5, 50.25, 10.03) == (488 - 80, 804 - 80, 160)           # 160.48 -> 160
    assert tube.quantise(0.0, 0.0, 10.04) == (-80, -80, 161)                         # 160.64 -> 161; X0 = floor(-80.5 + 0.5)
    assert tube.quantise(1.0, 1.0, 0.01)[2] == 16 and tube.quantise(1.0, 1.0, 1e9)[2] == tr.MAX_SIDE
    assert tube.quantise(1e12, -1e12, 10.0)[:2] == (tr.MAX_COORD, -tr.MAX_COORD)
    rng = np.random.default_rng(1)
    for _ in range(50):
        a = rng.uniform(-500, 3000, 3)
        assert tube.quantise(*a) == tr.quantise(*a)


def test_smoothing_ends_and_milliseconds():
    t = [0.0, 0.04, 0.08, 0.12, 0.16, 0.2]
    v = [1.0, 2.0, 4.0, 8.0, 16.0, 32.0]
    assert tube.smooth(t, v, 0.0) == v                               # the raw values
    assert tube.smooth(t, v, 0.08) == [(1.0 + 2.0) / 2, (1.0 + 2.0 + 4.0) / 3, (2.0 + 4.0 + 8.0) / 3, (4.0 + 8.0 + 16.0) / 3, (8.0 + 16.0 + 32.0) / 3,
                                       (16.0 + 32.0) / 2]          # the ends average what is there
    # 2 * 40 ms <= 80 ms holds in whole milliseconds; 0.12 - 0.08 = 0.03999... in floats would not decide it
    assert tube.smooth([0.08, 0.12], [1.0, 3.0], 0.08) == [2.0, 2.0] and tube.smooth([0.08, 0.12], [1.0, 3.0], 0.0804) == [2.0, 2.0]
    assert tube.smooth([0.08, 0.12], [1.0, 3.0], 0.0794) == [1.0, 3.0]             # ms(0.0794) = 79 < 80
    assert tube.smooth([0.0, 1.0, 1.04], [5.0, 1.0, 2.0], 0.5) == [5.0, 1.5, 1.5]  # a gap: nothing is filled in
    rng = np.random.default_rng(2)
    tt = sorted(round(float(x), 3) for x in rng.uniform(0, 3, 40))
    vv = [float(x) for x in rng.uniform(0, 100, 40)]
    assert tube.smooth(tt, vv, 0.5) == tr.smooth(tt, vv, 0.5)


def _faces_of(n=30):
    out = []
    for fi in range(n):
        out.append((fi / 25.0, 3, fi, (10 + fi, 5, 40 + fi, 45), np.full((68, 2), fi, np.int32)))
        if 5 <= fi < 12:
            out.append((fi / 25.0, 1, fi, (100, 50 + fi, 120, 90 + fi), np.full((68, 2), 2 * fi, np.int32)))
    return out


def test_plan_spans_and_min_length():
    F = _faces_of()
    p = tube.plan(F)
    assert [(f, t, len(r)) for f, t, r in p] == [("track_00001.npy", 1, 7), ("track_00003.npy", 3, 30)]
    assert p == tr.plan(F)
    assert [r[1] for r in p[0][2]] == [fi / 25.0 for fi in range(5, 12)]
    assert p[1][2][15][2] == tube.quantise(sum(25.0 + k for k in range(9, 22)) / 13, 25.0, 1.6 * 40.0)    # 0.5 s: six rows either side
    assert tube.plan(F, smooth_window=0.0)[1][2][15][2] == tube.quantise(40.0, 25.0, 64.0)
    assert [f for f, _, _ in tube.plan(F, min_length=0.25)] == ["track_00003.npy"]  # track 1 lasts 0.24 s
    assert [f for f, _, _ in tube.plan(F, min_length=0.24)] == ["track_00001.npy", "track_00003.npy"]
    assert [f for f, _, _ in tube.plan(F, only={"1"}, ext="y4m")] == ["track_00001.y4m"]
    assert [f for f, _, _ in tube.plan(F, labels={3: "ann"}, only={"ann"})] == ["track_00003.npy"]
    segs = [(3, 0.2, 0.4), (1, 0.0, 0.2), (3, 0.8, 0.801), (3, 5.0, 6.0)]
    p = tube.plan(F, segments=segs)
    assert [(f, len(r)) for f, _, r in p] == [("track_00001_000.npy", 1), ("track_00003_000.npy", 6), ("track_00003_001.npy", 1)]
    assert [r[1] for r in p[1][2]] == [k / 25.0 for k in range(5, 11)]              # ms(start) <= ms(T) <= ms(end), both ends in
    assert p == tr.plan(F, segments=segs)
    a, b = tube.plan(F, t_from=0.4, t_until=0.8), tube.plan(F)
    assert a[1][2] == [r for r in b[1][2] if 0.4 <= r[1] < 0.8]                     # selection does not move a window
    m = tube.plan(F, region="mouth")
    assert m == tr.plan(F, region="mouth") and m[1][2][0][2][2] == 16 * 20          # 0.5 x 40


def test_read_segments(tmp_path):
    p = str(tmp_path / "s.txt")
    with open(p, "w") as f:
        f.write("3 0.400 1.000 4.50000 ann\n\n1 2.000 2.500 3.00000\n")
    assert tube.read_segments(p) == [(3, 0.4, 1.0), (1, 2.0, 2.5)]
    with open(p, "w") as f:
        f.write("3 0.4\n")
    with pytest.raises(ValueError, match="expected `track start end`"):
        tube.read_segments(p)


def test_file_pool_bounds_open_files(tmp_path):
    pool = tube.FilePool(3)
    paths = [str(tmp_path / ("f%d" % k)) for k in range(10)]
    for rnd in range(4):
        for k, p in enumerate(paths):
            pool.write(p, bytes([rnd, k]))
            assert len(pool._open) <= 3
    pool.close()
    assert pool.peak == 3 and not pool._open
    for k, p in enumerate(paths):
        assert open(p, "rb").read() == bytes([0, k, 1, k, 2, k, 3, k])


# ---- the verb on a scripted context ----------------------------------------------------------------------------------------------
def script_picture(fi, win, S, layout):
    n = S * S * 3 if layout == "rgb" else S * S + 2 * ((S + 1) // 2) ** 2
    k = (fi * 31 + win[0] * 7 + win[1] * 3 + win[2]) % 251
    return ((np.arange(n) + k) % 256).astype(np.uint8).reshape((S, S, 3) if layout == "rgb" else (n,))


class ScriptContext(object):
    def __init__(self, fail_at=None):
        self.calls, self.frames, self.fail_at = [], [], fail_at

    def ingest_ring(self, h, w, depth=16):
        return Ring(self.frames)

    def frame_crops(self, frames, windows, size, layout="rgb", matrix="601", full_range=False):
        self.calls.append((len(windows), layout, matrix, full_range))
        if self.fail_at is not None and len(self.calls) > self.fail_at:
            raise RuntimeError("scripted device error")
        assert len(frames) == len(windows) and all(not f.released for f in frames), "crops asked of a released frame"
        return np.stack([script_picture(f.i, w, size, layout) for f, w in zip(frames, windows)])


def all_faces(video, tp, lp, region):
    w, h = video.frame_size
    rows = formats.read_tracks(tp)
    times = [i / video.frame_rate for i in range(len(video))]
    if region == "mouth":
        return _faces.landmark_faces(rows, formats.read_landmarks(lp), times, w, h)
    return [(T, ident, fi, box, None) for fi, T, g in pipeline.faces_per_frame(rows, times, w, h, drop_last=False) for ident, box in g]


def plain_loop(video, tp, lp, S, fmt, region="face", full_range=False, **kw):
    """the files of the verb by a loop over the plan: no threads, no batches, no pool"""
    F = all_faces(video, tp, lp, region)
    files, index = {}, []
    for fname, track, rows in tr.plan(F, region=region, ext=fmt, **kw):
        pics = [script_picture(F[i][2], win, S, "rgb" if fmt == "npy" else "yuv420") for i, _, win in rows]
        files[fname] = tr.file_bytes(pics, S, fmt, "25:1", full_range)
        index += ["%s %d %.3f %d %d %d %d\n" % ((fname, k, T, track) + tuple(win)) for k, (_, T, win) in enumerate(rows)]
    return files, "".join(index)


def read_dir(d):
    return dict((n, open(os.path.join(d, n), "rb").read()) for n in sorted(os.listdir(d)))


@pytest.mark.parametrize("batch", [1, 7, 2048])
@pytest.mark.parametrize("fmt", ["y4m", "npy"])
def test_tube_verb_files_equal_the_plain_loop(tmp_path, batch, fmt):
    video = ScriptVideo(60)
    tp, lp = make_inputs(tmp_path)
    want, want_index = plain_loop(video, tp, lp, 6, fmt)
    assert len(want) >= 3 and sum(len(v) for v in want.values()) > 5000
    ctx = ScriptContext()
    out, ip = str(tmp_path / "tubes"), str(tmp_path / "index.txt")
    res = cli.tube(video, tp, None, out, size=6, fmt=fmt, index=ip, ctx=ctx, batch=batch, ahead=4, max_open=2)
    assert read_dir(out) == want and open(ip).read() == want_index
    assert res["tubes"] == len(want) and res["files"] == sorted(want) and res["pictures"] == want_index.count("\n")
    assert res["open_peak"] <= 2                                                     # the open-file bound, with more tracks than that on screen
    assert all(d.released for d in ctx.frames) and len(ctx.frames) == len(set(d.i for d in ctx.frames))    # ONE pass, every frame given back
    assert all(n <= batch for n, _, _, _ in ctx.calls) and (len(ctx.calls) == 1 if batch == 2048 else len(ctx.calls) > 5)
    if fmt == "npy":
        for name, data in want.items():
            a = np.load(os.path.join(out, name))
            assert a.dtype == np.uint8 and a.shape[1:] == (6, 6, 3) and a.shape[0] == sum(1 for l in want_index.splitlines() if l.startswith(name))


@pytest.mark.parametrize("fmt", ["y4m", "npy"])
def test_tube_verb_segments_mouth_and_options(tmp_path, fmt):
    video = ScriptVideo(60)
    tp, lp = make_inputs(tmp_path)
    F = all_faces(video, tp, lp, "mouth")
    tracks = sorted(set(f[1] for f in F))
    sp = str(tmp_path / "segments.txt")
    with open(sp, "w") as f:
        for k in tracks[:3]:
            tt = sorted(x[0] for x in F if x[1] == k)
            f.write("%d %.3f %.3f 2.50000 name\n%d %.3f %.3f 1.00000 name\n" % (k, tt[1], tt[len(tt) // 2], k, tt[-2], tt[-1] + 1.0))
    segs = tube.read_segments(sp)
    want, want_index = plain_loop(video, tp, lp, 5, fmt, region="mouth", full_range=True, segments=segs, scale=0.75, smooth_window=0.2,
                                  min_length=0.04, t_from=0.08)
    assert len(want) >= 4 and all("_00" in n for n in want)
    out, ip = str(tmp_path / "tubes"), str(tmp_path / "index.txt")
    ctx = ScriptContext()
    res = cli.tube(video, tp, lp, out, size=5, region="mouth", scale=0.75, smooth=0.2, segments=sp, min_length=0.04, t_from=0.08, fmt=fmt,
                   matrix="709", full_range=True, index=ip, ctx=ctx, batch=11)
    assert read_dir(out) == want and open(ip).read() == want_index and res["tubes"] == len(want)
    assert all(c[1:] == ("rgb" if fmt == "npy" else "yuv420", "709", True) for c in ctx.calls)
    if fmt == "y4m":
        assert all(v.startswith(b"YUV4MPEG2 W5 H5 F25:1 C420 XCOLORRANGE=FULL\nFRAME\n") for v in want.values())

    class Stream(ScriptVideo):                                                       # a pipe: no length before it has been read
        def __len__(self):
            raise TypeError("a stream has no length")
    want_all, _ = plain_loop(video, tp, lp, 4, fmt, only={"0", "#2"}, labels={0: "0"})
    out2 = str(tmp_path / "tubes2")
    cli.tube(Stream(60), tp, None, out2, size=4, fmt=fmt, label={0: "0"}, only={"0", "#2"}, ctx=ScriptContext(), batch=9)
    assert read_dir(out2) == want_all and len(want_all) == 2


def test_tube_verb_hands_on_errors_and_refuses(tmp_path):
    video = ScriptVideo(60)
    tp, lp = make_inputs(tmp_path)
    ctx = ScriptContext(fail_at=2)
    with pytest.raises(RuntimeError, match="scripted device error"):
        cli.tube(video, tp, None, str(tmp_path / "o"), size=4, fmt="npy", ctx=ctx, batch=5, ahead=2)
    assert all(d.released for d in ctx.frames)                                       # the reader ran out, every frame was given back
    with pytest.raises(ValueError, match="--region mouth needs the landmarks file"):
        cli.tube(video, tp, None, str(tmp_path / "o"), region="mouth", ctx=ScriptContext())
    with pytest.raises(ValueError, match="--size is 1 .. 1024"):
        cli.tube(video, tp, None, str(tmp_path / "o"), size=2000, ctx=ScriptContext())
    with pytest.raises(ValueError, match="y4m or npy"):
        cli.tube(video, tp, None, str(tmp_path / "o"), fmt="mp4", ctx=ScriptContext())
    res = cli.tube(video, tp, None, str(tmp_path / "none"), t_from=50.0, ctx=ScriptContext())    # nothing left: an empty directory
    assert res["tubes"] == 0 and os.listdir(str(tmp_path / "none")) == []


def test_parser():
    a = cli.parse_args(["tube", "-", "t.txt", "out"])
    assert (a.size, a.region, a.scale, a.smooth, a.label, a.only, a.segments, a.min_length, a.t_from, a.t_until, a.fmt, a.out_matrix, a.out_range,
            a.index) == (224, "face", None, 0.5, None, None, None, 0.0, 0.0, None, "y4m", None, None, None)
    assert (a.video, a.tracking, a.rest) == ("-", "t.txt", ["out"])
    a = cli.parse_args(["tube", "--size", "96", "--region", "mouth", "--scale", "0.6", "--smooth", "0.2", "--label", "n.txt", "--only", "ann,#3",
                        "--segments", "s.txt", "--min-length", "1.5", "--from", "1", "--until", "2.5", "--format", "npy", "--matrix", "709",
                        "--range", "full", "--index", "i.txt", "v", "t", "l", "o"])
    assert (a.size, a.region, a.scale, a.smooth, a.label, a.only, a.segments, a.min_length, a.t_from, a.t_until, a.fmt, a.out_matrix, a.out_range,
            a.index) == (96, "mouth", 0.6, 0.2, "n.txt", {"ann", "#3"}, "s.txt", 1.5, 1.0, 2.5, "npy", "709", "full", "i.txt")
    assert a.rest == ["l", "o"]
    with pytest.raises(SystemExit):
        cli.parse_args(["tube", "--format", "mp4", "v", "t", "o"])
    with pytest.raises(SystemExit):
        cli.parse_args(["tube", "v", "t"])
