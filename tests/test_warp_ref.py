"""CPU: TUBE.md "Oriented window" on its restatement (tests/warp_ref.py) and on the host code of `tube --align` (tube.py, the parser,
cli.tube on a scripted context).  Worked values whose answers come from a pencil, that the comparison the GPU tests make sees each of a
list of planted defects, the kernel's quotient for every divisor, the host rules on hand-made landmarks, and the verb's files against a
plain loop."""
import math
import os

import numpy as np
import pytest

from tests import tube_ref as tr
from tests import warp_ref as wr
from tests.test_faces_ref import ScriptVideo, make_inputs
from tests.test_tube_ref import ScriptContext as CropContext, all_faces, plain_loop as crop_plain_loop, read_dir
from pyannote_video_amd import cli, tube

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME = tr.picture(37, 50, 1)
ONE = wr.ONE


# ---- the restatement alone ---------------------------------------------------------------------------------------------------------
def test_constants_agree_with_the_package_the_header_and_the_kernel():
    assert (tube.MAX_K, tube.MAX_STEP) == (wr.MAX_K, wr.MAX_STEP) == (16, 1 << 20)
    hdr = open(os.path.join(ROOT, "include", "pvface.h")).read()
    assert "#define PVF_WARP_MAX_K 16 " in hdr and "#define PVF_WARP_MAX_STEP (1 << 20) " in hdr
    src = open(os.path.join(ROOT, "pyannote-video_amd", "csrc", "tube.hip")).read()
    for name, v in (("W_SIDE", wr.W_SIDE), ("W_TILE", wr.W_TILE)):
        assert "constexpr int %s = %d;" % (name, v) in src, name
    # the overflow arguments of TUBE.md: positions are 64-bit, tile-relative positions and a pixel's sum are 32-bit
    assert 8192 * wr.MAX_COORD >= 2 ** 31
    assert 131071 + 2 * 2 * wr.W_SIDE * wr.MAX_K * wr.MAX_STEP < 2 ** 31
    assert 65536 * wr.MAX_K ** 2 * 255 + 32768 * wr.MAX_K ** 2 < 2 ** 32 and (65536 * wr.MAX_K ** 2 * 255 + 32768 * wr.MAX_K ** 2) >> 16 < 2 ** 16


def test_identity():
    for S, x, y in ((8, 5, 3), (2, 0, 0), (36, 14, 1)):
        assert np.array_equal(wr.warp(FRAME, wr.identity(x, y, S), S), FRAME[y:y + S, x:x + S])
    got = wr.warp(FRAME, wr.identity(40, 30, 20), 20)              # past the right and bottom edges: black
    assert np.array_equal(got[:7, :10], FRAME[30:, 40:]) and not got[7:].any() and not got[:, 10:].any()


def test_quarter_turns():
    S, x, y = 8, 5, 3
    CX, CY = wr.identity(x, y, S)[:2]
    src = FRAME[y:y + S, x:x + S]
    # the row step (0, 1) walks down the source: output row 0 is the source's last column read downwards, np.rot90 once
    assert np.array_equal(wr.warp(FRAME, (CX, CY, 0, ONE, 1), S), np.rot90(src, 1))
    assert np.array_equal(wr.warp(FRAME, (CX, CY, 0, ONE, 1), S)[0], src[:, -1])
    assert np.array_equal(wr.warp(FRAME, (CX, CY, -ONE, 0, 1), S), np.rot90(src, 2))
    assert np.array_equal(wr.warp(FRAME, (CX, CY, 0, -ONE, 1), S), np.rot90(src, 3))


def test_two_to_one_block_mean_rounds_half_up():
    S, x, y = 6, 4, 2
    got = wr.warp(FRAME, (16 * x + 16 * S, 16 * y + 16 * S, ONE, 0, 2), S)
    f = FRAME.astype(np.int64)
    for r in range(S):
        for c in range(S):
            yy, xx = y + 2 * r, x + 2 * c
            assert got[r, c].tolist() == ((f[yy, xx] + f[yy, xx + 1] + f[yy + 1, xx] + f[yy + 1, xx + 1] + 2) // 4).tolist()
    two = np.zeros((2, 2, 3), np.uint8)
    two[0, 0] = (1, 2, 3)                                           # sums 1, 2, 3 over four pixels: 0.25 -> 0, 0.5 -> 1, 0.75 -> 1
    assert wr.warp(two, (16, 16, ONE, 0, 2), 1).reshape(3).tolist() == [0, 1, 1]


def test_constant_frames_inside_half_off_and_still():
    const = np.full((40, 60, 3), (201, 7, 90), np.uint8)
    for win, S in (((480, 320) + wr.direction(17.0, ONE) + (1,), 9), ((485, 311) + wr.direction(-63.0, 40000) + (3,), 7),
                   ((480, 320) + wr.direction(45.0, ONE // 7) + (16,), 5), ((480, 320, 0, 0, 2), 4)):
        assert (wr.warp(const, win, S) == np.array((201, 7, 90))).all(), (win, S)
    # the left half of the window off the frame: K = 2, two of an output pixel's four sub-samples are black: (2 v + 2) // 4
    got = wr.warp(const, (0, 320, ONE, 0, 2), 1)
    assert got.reshape(3).tolist() == [(2 * 201 + 2) // 4, (2 * 7 + 2) // 4, (2 * 90 + 2) // 4] == [101, 4, 45]
    # S = 4 centred on the frame's left edge, K = 1: columns 0, 1 lie at pixels -2, -1 and are black, columns 2, 3 are the frame
    got = wr.warp(const, (0, 320, ONE, 0, 1), 4)
    assert not got[:, :2].any() and (got[:, 2:] == np.array((201, 7, 90))).all()
    # B = (0, 0): every sub-sample is the centre: (CX, CY) = (16 x + 8, 16 y + 8) is the centre of pixel (x, y)
    for K in (1, 3, 16):
        assert (wr.warp(FRAME, (16 * 20 + 8, 16 * 10 + 8, 0, 0, K), 5) == FRAME[10, 20]).all()
    f = FRAME.astype(np.int64)                                      # and a centre on a pixel corner is the mean of four
    assert wr.warp(FRAME, (16 * 20, 16 * 10, 0, 0, 2), 3)[1, 1].tolist() == ((f[9, 19] + f[9, 20] + f[10, 19] + f[10, 20] + 2) // 4).tolist()


def test_floor_of_a_negative_coordinate():
    """S = 1, K = 1, B = 0: the one sub-sample lies at PX = 8192 CX - 65536.  CX = -8 puts it at -131072: pixel -1 exactly, fx = 0;
    one sub-unit either side of the boundary the floor and the truncation differ"""
    f = np.zeros((3, 3, 3), np.uint8)
    f[:, 0] = 200
    row = 16 * 1 + 8

    def left(CX):
        return int(wr.warp(f, (CX, row, 0, 0, 1), 1)[0, 0, 0])
    assert left(8) == 200                                           # PX = 0: pixel 0
    assert left(-8) == 0                                            # PX = -131072: pixel -1, weight 256; pixel 0 has weight 0
    # CX = -7: PX = -122880, x0 = floor = -1, fx = (8192 >> 9) = 16: 16 / 256 of pixel 0: (16 * 256 * 200 + 32768) >> 16 = 13
    assert left(-7) == (16 * 256 * 200 + 32768) >> 16 == 13
    assert left(-9) == 0                                            # x0 = -2, x1 = -1: both black
    assert left(7) == (240 * 256 * 200 + 32768) >> 16               # x0 = -1 still (PX = -8192), fx = 240
    # truncation would put x0 = 0 with fx = 240 there: 16 / 256 of pixel 0 and 240 / 256 of pixel 1 (which is 0)
    assert int(wr.warp(f, (7, row, 0, 0, 1), 1, truncate=True)[0, 0, 0]) != left(7)


def test_all_fractions_on_a_two_pixel_ramp():
    """S = 2, K = 1, B = (BX, 0): m, n = -1, +1, so picture column 1 lies at PX = 8192 CX + BX - 65536 = BX for CX = 8: x0 = 0 and
    fx = BX >> 9 takes every value.  The rows of the frame are equal, and PY = 8192 CY -+ BX - 65536 stays between rows 0 and 3, so the
    two row weights, which sum to 256, meet equal bytes."""
    f = np.zeros((4, 2, 3), np.uint8)
    f[:, 0], f[:, 1] = (10, 0, 255), (250, 255, 0)
    for fx in range(256):
        for BX in (512 * fx, 512 * fx + 511):                      # fx is floored, not rounded
            got = wr.warp(f, (8, 32, BX, 0, 1), 2)
            want = [((256 - fx) * 256 * int(a) + fx * 256 * int(b) + 32768) >> 16 for a, b in zip(f[0, 0], f[0, 1])]
            assert got[0, 1].tolist() == want and got[1, 1].tolist() == want, (fx, BX)
    assert wr.warp(f, (8, 32, 512 * 128, 0, 1), 2)[0, 1].tolist() == [130, 128, 128]               # half way: (10 + 250) / 2, 127.5 -> 128


def test_quotient_is_exact_for_every_divisor():
    v = np.arange(65536, dtype=np.int64)
    for d in range(1, 257):
        M = (1 << 24) // d + 1
        assert np.array_equal((v * M) >> 24, v // d), d
    assert wr.quotient(65535, 256) == 255 and wr.quotient(255 * 256 + 128, 256) == 255 and wr.quotient(0, 1) == 0


def test_quotient_check_in_c(tmp_path):
    """warp_k's own division, (uint32)(((uint64) v * M) >> 24), compiled for the host (tests/csrc/warp_quotient_check.c)"""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "warp_quotient_check")
    subprocess.check_call(["gcc", "-O2", "-o", exe, os.path.join(ROOT, "tests", "csrc", "warp_quotient_check.c")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-400:]
    assert "256 divisors" in out.stdout and " 0 differ" in out.stdout


def test_planted_defects_are_visible():
    """each defect changes what the GPU tests compare, on the windows those tests use"""
    frame = tr.picture(48, 64, 10)
    S = 9
    cases = wr.window_cases(48, 64, S)
    good = dict((k, wr.warp(frame, w, S)) for k, w in cases.items())

    def seen(**kw):
        return [k for k, w in cases.items() if not np.array_equal(wr.warp(frame, w, S, **kw), good[k])]
    s = seen(perp_sign=True)
    assert "east" in s and "any_1" in s and "diagonal" in s
    s = seen(no_half=True)
    assert "east" in s and "still" in s and "any_2" in s
    s = seen(truncate=True)
    assert "corner_tl" in s and "cross_left" in s and "east" not in s            # only where a tap has a negative coordinate
    s = seen(clamp=True)
    assert "cross_left" in s and "corner_br" in s and "outside_top" in s and "east" not in s
    s = seen(round_fx=True)
    assert "any_1" in s and "enlarge" in s
    s = seen(rounding=False)
    assert "any_1" in s and "diagonal_k2" in s
    s = seen(k_off=True)
    assert "east" in s and "any_3" in s and "still" not in s
    s = seen(swap_channels=True)
    assert "east" in s and "still" in s and "outside_left" not in s


def test_which_path_a_tile_takes():
    """the restated box: a small frame is staged whole; a 45 degree window of a large frame at K = 16 is beyond the tile; off the frame
    nothing is loaded"""
    assert set(wr.tile_paths(48, 64, wr.identity(3, 2, 32), 32)) == {"lds"}
    assert set(wr.tile_paths(1080, 1920, (16 * 900, 16 * 500) + wr.direction(45.0, ONE) + (16,), 32)) == {"direct"}
    assert set(wr.tile_paths(48, 64, (-16 * 4000, 0, ONE, 0, 1), 32)) == {"empty"}
    # an axis-aligned tile of 16 x 16 pixels at K = 1 and a step of one pixel touches 17 x 17 source pixels
    assert wr.tile_paths(1080, 1920, (16 * 900 + 5, 16 * 500 + 3, ONE, 0, 1), 16) == ["lds"]
    assert (16 * 16 * 2 * 0.7071 + 2) * ((3 + 3 * (16 * 16 * 2 * 0.7071 + 2) + 15) // 16 * 16) > wr.W_TILE


# ---- host rules ------------------------------------------------------------------------------------------------------------------
def points(e0, e1):
    p = np.zeros((68, 2), np.int32)
    p[:] = 999
    p[36:42], p[42:48] = e0, e1
    return p


def test_eye_direction():
    assert tube.eye_direction(points((100, 50), (140, 50))) == (1.0, 0.0)                          # 0 degrees
    assert tube.eye_direction(points((100, 50), (100, 90))) == (0.0, 1.0)                          # 90
    c, s = tube.eye_direction(points((100, 50), (130, 80)))                                          # 45
    assert c == s == 30.0 / math.hypot(30.0, 30.0)
    assert tube.eye_direction(points((140, 50), (100, 50))) == (-1.0, 0.0)                         # 180
    assert tube.eye_direction(points((7, 7), (7, 7))) == (1.0, 0.0) and tube.eye_direction(None) == (1.0, 0.0)       # coincident eyes; no row
    p = points((0, 0), (0, 0))                                      # integer sums divided by 6.0, not a rounded mean
    p[36:42, 0] = (1, 1, 1, 1, 1, 2)
    p[42:48, 0] = 10
    assert tube.eye_direction(p) == (1.0, 0.0) and wr.eye_direction(p) == (1.0, 0.0)
    rng = np.random.default_rng(3)
    for _ in range(20):
        q = rng.integers(0, 500, (68, 2)).astype(np.int32)
        assert tube.eye_direction(q) == wr.eye_direction(q)


def test_quantisation_and_the_k_rule():
    S = 10
    # side / S = 1: a step of one pixel along the direction, K = 1
    assert tube.quantise_oriented(30.0, 50.25, 10.0, 1.0, 0.0, S) == (480, 804, ONE, 0, 1)
    assert tube.quantise_oriented(30.03, -0.04, 10.0, 0.0, -1.0, S) == (480, -1, 0, -ONE, 1)       # 480.48 -> 480, -0.64 + 0.5 -> floor -1
    # A = (3, 4) pixels: |A| = 5 pixels exactly, K = 5; one unit more, K = 6
    assert tube.quantise_oriented(0.0, 0.0, 50.0, 0.6, 0.8, S)[2:] == wr.quantise_oriented(0.0, 0.0, 50.0, 0.6, 0.8, S)[2:]
    side = 5.0 * S
    c, s = 3.0 / 5.0, 4.0 / 5.0
    ax, ay = side / S * 65536.0 * c, side / S * 65536.0 * s
    assert (math.floor(ax + 0.5), math.floor(ay + 0.5)) == (3 * ONE, 4 * ONE)
    assert tube.quantise_oriented(0.0, 0.0, side, c, s, S)[4] == 5
    assert tube.quantise_oriented(0.0, 0.0, side, c, s, S)[2:4] == (math.floor(ax / 5 + 0.5), math.floor(ay / 5 + 0.5))

    def K_of(AX, AY):                                               # the rule on exact integers, through the float path: side / S = 1 / 65536
        return tube.quantise_oriented(0.0, 0.0, 1.0, float(AX), float(AY), 65536.0)[4]
    assert K_of(3 * ONE, 4 * ONE) == 5 and K_of(3 * ONE + 1, 4 * ONE) == 6 and K_of(3 * ONE, 4 * ONE + 1) == 6
    assert K_of(ONE, 0) == 1 and K_of(ONE + 1, 0) == 2 and K_of(0, -ONE) == 1 and K_of(0, 0) == 1
    assert K_of(15 * ONE, 0) == 15 and K_of(16 * ONE, 0) == 16 and K_of(16 * ONE + 1, 0) == 16 and K_of(400 * ONE, 0) == 16     # the cap
    assert tube.quantise_oriented(0.0, 0.0, 1.0, 400.0 * ONE, -1e30, 65536.0)[2:] == (wr.MAX_STEP, -wr.MAX_STEP, 16)               # B is clipped
    assert tube.quantise_oriented(1e12, -1e12, 10.0, 1.0, 0.0, S)[:2] == (wr.MAX_COORD, -wr.MAX_COORD)
    # the effective side S K |B| / 65536 is within S K / 65536 * sqrt(2) / 2 pixels of the side (half a unit per component and sub-sample)
    rng = np.random.default_rng(4)
    for _ in range(200):
        side, ang, S2 = float(rng.uniform(5, 900)), float(rng.uniform(-math.pi, math.pi)), int(rng.integers(1, 300))
        a = (float(rng.uniform(-50, 2000)), float(rng.uniform(-50, 2000)), side, math.cos(ang), math.sin(ang), S2)
        CX, CY, BX, BY, K = tube.quantise_oriented(*a)
        assert (CX, CY, BX, BY, K) == wr.quantise_oriented(*a)
        if side / S2 <= 16.0:
            assert abs(S2 * K * math.hypot(BX, BY) / 65536.0 - side) <= S2 * K * math.sqrt(0.5) / 65536.0 + 1e-9
            assert math.hypot(BX, BY) < 65538.0                                              # a sub-step of at most a pixel


def _track(angles, fps=25.0):
    out = []
    for k, deg in enumerate(angles):
        r = math.radians(deg)
        e0 = (200 - int(round(40 * math.cos(r))), 100 - int(round(40 * math.sin(r))))
        e1 = (200 + int(round(40 * math.cos(r))), 100 + int(round(40 * math.sin(r))))
        out.append((k / fps, 0, k, (150, 50, 250, 150), points(e0, e1)))
    return out


def test_a_track_through_180_degrees_stays_there():
    F = _track([170, 175, 180, -175, -170, -170, 170])
    p = tube.plan(F, align=True, size=20, smooth_window=0.2)
    assert p == wr.plan(F, 20, smooth_window=0.2)
    for _, _, win in p[0][2]:
        ang = math.degrees(math.atan2(win[3], win[2]))
        assert abs(abs(ang) - 180.0) < 8.0, ang                    # near 180, not near 0 as the mean of the angles would be
    raw = tube.plan(F, align=True, size=20, smooth_window=0.0)
    assert raw == wr.plan(F, 20, smooth_window=0.0)
    assert [w[2:] for _, _, w in raw[0][2]][0] == tube.quantise_oriented(0, 0, 160.0, *tube.eye_direction(F[0][4]), 20)[2:]     # the raw direction
    # opposite directions cancel: the smoothed vector of length 0 is (1, 0)
    G = [(0.0, 0, 0, (150, 50, 250, 150), points((100, 50), (140, 50))), (0.04, 0, 1, (150, 50, 250, 150), points((140, 50), (100, 50)))]
    assert [w[2:4] for _, _, w in tube.plan(G, align=True, size=160, smooth_window=0.5)[0][2]] == [(ONE, 0), (ONE, 0)]
    # a face without points has direction (1, 0); the centre and the side are those of the unaligned plan
    H = [(0.0, 0, 0, (150, 50, 250, 150), None)]
    (CX, CY, BX, BY, K), (X0, Y0, L) = tube.plan(H, align=True, size=160)[0][2][0][2], tube.plan(H)[0][2][0][2]
    assert (CX, CY, BX, BY, K) == (16 * 200, 16 * 100, ONE, 0, 1) and (X0 + L // 2, Y0 + L // 2, L) == (CX, CY, 16 * 160)
    assert tube.index_line("f", 3, 0.04, 7, (1, -2, 3, -4, 5)) == "f 3 0.040 7 1 -2 3 -4 5\n" == wr.index_line("f", 3, 0.04, 7, (1, -2, 3, -4, 5))
    assert tube.index_line("f", 3, 0.04, 7, (1, -2, 3)) == "f 3 0.040 7 1 -2 3\n"


# ---- the verb on a scripted context ----------------------------------------------------------------------------------------------
def script_picture(fi, win, S, layout):
    n = S * S * 3 if layout == "rgb" else S * S + 2 * ((S + 1) // 2) ** 2
    k = (fi * 31 + win[0] * 7 + win[1] * 3 + win[2] + win[3] * 5 + win[4] * 11) % 251
    return ((np.arange(n) + k) % 256).astype(np.uint8).reshape((S, S, 3) if layout == "rgb" else (n,))


class ScriptContext(CropContext):
    def frame_warps(self, frames, windows, size, layout="rgb", matrix="601", full_range=False):
        self.calls.append((len(windows), layout, matrix, full_range))
        assert len(frames) == len(windows) and all(not f.released for f in frames) and all(len(w) == 5 for w in windows)
        return np.stack([script_picture(f.i, w, size, layout) for f, w in zip(frames, windows)])

    def frame_crops(self, *a, **k):
        raise AssertionError("an aligned tube asks for warps")


def aligned_faces(video, tp, lp, region):
    """the faces `tube --align` sees: for mouth tubes the rows of the landmark file, for face tubes every face of the tracking file with
    the points of its landmark row, if it has one"""
    if region == "mouth":
        return all_faces(video, tp, lp, "mouth")
    pts = dict(((tr.ms(f[0]), f[1]), f[4]) for f in all_faces(video, tp, lp, "mouth"))
    return [(T, ident, fi, box, pts.get((tr.ms(T), ident))) for T, ident, fi, box, _ in all_faces(video, tp, lp, "face")]


def plain_loop(video, tp, lp, S, fmt, region="face", full_range=False, **kw):
    F = aligned_faces(video, tp, lp, region)
    files, index = {}, []
    for fname, track, rows in wr.plan(F, S, region=region, ext=fmt, **kw):
        pics = [script_picture(F[i][2], win, S, "rgb" if fmt == "npy" else "yuv420") for i, _, win in rows]
        files[fname] = tr.file_bytes(pics, S, fmt, "25:1", full_range)
        index += [wr.index_line(fname, k, T, track, win) for k, (_, T, win) in enumerate(rows)]
    return files, "".join(index)


@pytest.mark.parametrize("batch", [1, 7, 2048])
@pytest.mark.parametrize("fmt", ["y4m", "npy"])
def test_aligned_tube_files_equal_the_plain_loop(tmp_path, batch, fmt):
    video = ScriptVideo(60)
    tp, lp = make_inputs(tmp_path)
    want, want_index = plain_loop(video, tp, lp, 6, fmt)
    assert len(want) >= 3 and sum(len(v) for v in want.values()) > 5000
    assert len(set(tuple(l.split()[6:8]) for l in want_index.splitlines())) > 10                    # directions of many kinds
    assert all(len(l.split()) == 9 for l in want_index.splitlines())                                 # file picture T track CX CY BX BY K
    ctx = ScriptContext()
    out, ip = str(tmp_path / "tubes"), str(tmp_path / "index.txt")
    res = cli.tube(video, tp, lp, out, size=6, fmt=fmt, index=ip, ctx=ctx, batch=batch, ahead=4, max_open=2, align=True)
    assert read_dir(out) == want and open(ip).read() == want_index
    assert res["tubes"] == len(want) and res["files"] == sorted(want) and res["pictures"] == want_index.count("\n") and res["open_peak"] <= 2
    assert all(d.released for d in ctx.frames) and len(ctx.frames) == len(set(d.i for d in ctx.frames))
    assert all(n <= batch for n, _, _, _ in ctx.calls) and (len(ctx.calls) == 1 if batch == 2048 else len(ctx.calls) > 5)


@pytest.mark.parametrize("fmt", ["y4m", "npy"])
def test_aligned_mouth_tubes_with_segments_and_options(tmp_path, fmt):
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
                   matrix="709", full_range=True, index=ip, ctx=ctx, batch=11, align=True)
    assert read_dir(out) == want and open(ip).read() == want_index and res["tubes"] == len(want)
    assert all(c[1:] == ("rgb" if fmt == "npy" else "yuv420", "709", True) for c in ctx.calls)
    want2, _ = plain_loop(video, tp, lp, 4, fmt, only={"0", "#2"}, labels={0: "0"}, smooth_window=0.0)
    out2 = str(tmp_path / "tubes2")
    cli.tube(video, tp, lp, out2, size=4, fmt=fmt, label={0: "0"}, only={"0", "#2"}, smooth=0.0, ctx=ScriptContext(), batch=9, align=True)
    assert read_dir(out2) == want2 and len(want2) == 2


def test_refusal_without_landmarks_and_unaligned_output_unchanged(tmp_path):
    video = ScriptVideo(60)
    tp, lp = make_inputs(tmp_path)
    with pytest.raises(ValueError, match="--align needs the landmarks file"):
        cli.tube(video, tp, None, str(tmp_path / "o"), ctx=ScriptContext(), align=True)
    assert not os.path.exists(str(tmp_path / "o"))
    # without --align: what the verb wrote before, whether or not a landmark file is given
    for fmt in ("y4m", "npy"):
        for region, marks in (("face", None), ("face", lp), ("mouth", lp)):
            want, want_index = crop_plain_loop(video, tp, lp, 6, fmt, region=region)
            out, ip = str(tmp_path / ("plain_%s_%s_%s" % (fmt, region, marks is None))), str(tmp_path / "index.txt")
            cli.tube(video, tp, marks, out, size=6, region=region, fmt=fmt, index=ip, ctx=CropContext(), batch=7)
            assert read_dir(out) == want and open(ip).read() == want_index
            assert all(len(l.split()) == 7 for l in want_index.splitlines())


def test_parser():
    a = cli.parse_args(["tube", "-", "t.txt", "out"])
    assert a.align is False
    a = cli.parse_args(["tube", "--align", "--size", "96", "--region", "mouth", "v", "t", "l", "o"])
    assert a.align is True and (a.size, a.region, a.rest) == (96, "mouth", ["l", "o"])
