"""GPU: the oriented windows of `tube --align` (warp_k in csrc/tube.hip) bit for bit against TUBE.md as tests/warp_ref.py restates it:
the named windows on frames of every byte length mod 4 and every base alignment, the picture sizes on the seams of the kernel's tiles,
both of its load paths (which one a case takes is asserted from the restated box), both layouts and all colour flags (and
pvf_render_batch as an independent check of the YUV form), how a call is made (batches, rounds, where the output lies), the existing
kernel on the windows both can express, every refusal of the C ABI, and the verb end to end in a process of its own."""
import os
import subprocess
import sys

import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships
import numpy as np
import pytest

from tests import tube_ref as tr
from tests import warp_ref as wr
from tests.test_gpu_faces import bare_ctx      # noqa: F401 -- fixture
from tests.test_gpu_tube import GEOMETRIES, frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the minimum, 2, odd and even ones, and the sizes either side of one and of two tiles (the picture is square: both directions)
SIZES = [1, 2, 7, 10, wr.W_SIDE - 1, wr.W_SIDE, wr.W_SIDE + 1, 2 * wr.W_SIDE - 1, 2 * wr.W_SIDE, 2 * wr.W_SIDE + 1]
ONE = wr.ONE


def _same(got, ref, names=None):
    assert got.shape == ref.shape and got.dtype == np.uint8, (got.shape, ref.shape)
    bad = [i for i in range(len(ref)) if not np.array_equal(got[i], ref[i])]
    assert not bad, [(names[i] if names else i, int((got[i] != ref[i]).sum()), np.argwhere(got[i] != ref[i])[:3].tolist()) for i in bad[:6]]


def _both_layouts(ctx, frames, windows, S, names=None, matrix="601", full_range=False, arrays=None):
    arrays = frames if arrays is None else arrays
    rgb = wr.warps(arrays, windows, S)
    _same(ctx.frame_warps(frames, windows, S), rgb, names)
    yuv = np.stack([tr.to_yuv(p, matrix, full_range) for p in rgb])
    _same(ctx.frame_warps(frames, windows, S, "yuv420", matrix, full_range), yuv, names)
    return rgb


def _paths(f, windows, S):
    out = set()
    for w in windows:
        out |= set(wr.tile_paths(f.shape[0], f.shape[1], w, S))
    return out


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_named_windows_equal_the_restatement(bare_ctx, name, S):
    f = frame(name)
    cases = wr.window_cases(f.shape[0], f.shape[1], S)
    assert set(w[4] for w in cases.values()) >= {1, 2, 3, 16}
    rgb = _both_layouts(bare_ctx, [f] * len(cases), list(cases.values()), S, list(cases))
    by = dict(zip(cases, rgb))
    for k in wr.BLACK:
        assert not by[k].any(), k                                   # black, not garbage
        assert wr.tile_paths(f.shape[0], f.shape[1], cases[k], S) == ["empty"] * ((S + wr.W_SIDE - 1) // wr.W_SIDE) ** 2
    assert by["east"].any() and by["still"].any() and (by["still"] == by["still"][0, 0]).all()
    paths = _paths(f, cases.values(), S)                            # (a frame of less than W_TILE bytes is staged whole, whatever the window)
    assert paths >= {"lds", "empty"}
    if f.shape[0] * ((3 + 3 * f.shape[1] + 15) & ~15) <= wr.W_TILE:
        assert "direct" not in paths


def test_black_in_limited_range_yuv(bare_ctx):
    f = frame("64x48")
    cases = wr.window_cases(48, 64, 6)
    got = bare_ctx.frame_warps([f] * len(wr.BLACK), [cases[k] for k in wr.BLACK], 6, "yuv420")
    assert (got[:, :36] == 16).all() and (got[:, 36:] == 128).all()


@pytest.mark.parametrize("off", [1, 2, 3])
def test_frames_off_alignment(bare_ctx, off):
    for name in GEOMETRIES:
        f = frame(name)
        h, w = f.shape[:2]
        n = f.size
        buf = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
        buf[:] = 255                                                # what lies around the frame is not black: a read past it would show
        view = buf[off:off + n].view(h, w, 3)
        view.copy_(torch.from_numpy(f))
        torch.cuda.synchronize()
        assert view.data_ptr() % 4 == off and view.is_contiguous()
        fr = bare_ctx.wrap_torch(view)
        for S in (9, 18):
            cases = wr.window_cases(h, w, S)
            _same(bare_ctx.frame_warps([fr] * len(cases), list(cases.values()), S), wr.warps([f] * len(cases), list(cases.values()), S), list(cases))
        fr.release()


def test_identity_quarter_turns_and_reduction(bare_ctx):
    f = frame("97x61")
    for S in (8, 17, 32):
        x, y = 5, 3
        CX, CY = wr.identity(x, y, S)[:2]
        src = f[y:y + S, x:x + S]
        got = bare_ctx.frame_warps([f] * 4, [(CX, CY, ONE, 0, 1), (CX, CY, 0, ONE, 1), (CX, CY, -ONE, 0, 1), (CX, CY, 0, -ONE, 1)], S)
        for k in range(4):
            assert np.array_equal(got[k], np.rot90(src, k)), (S, k)
    S = 12
    got = bare_ctx.frame_warps([f], [(16 * 4 + 16 * S, 16 * 2 + 16 * S, ONE, 0, 2)], S)[0]
    blocks = f[2:2 + 2 * S, 4:4 + 2 * S].astype(np.int64).reshape(S, 2, S, 2, 3).sum(axis=(1, 3))
    assert np.array_equal(got, (blocks + 2) // 4)
    const = np.full((40, 60, 3), (201, 7, 90), np.uint8)
    wins = [(480, 320) + wr.direction(17.0, ONE) + (1,), (485, 311) + wr.direction(-63.0, 40000) + (3,), (480, 320) + wr.direction(45.0, ONE // 7) + (16,)]
    assert (bare_ctx.frame_warps([const] * 3, wins, 9) == np.array((201, 7, 90), np.uint8)).all()


# ---- the two load paths ------------------------------------------------------------------------------------------------------------
def test_a_mid_sized_frame_takes_both_paths(bare_ctx):
    """200 x 150: too large to be staged whole (150 rows of 608 bytes), so wide windows leave the tile budget while face-sized ones stay"""
    f = tr.picture(150, 200, 21)
    fr = bare_ctx.upload(f)
    for S in (17, 33):
        cases = wr.window_cases(150, 200, S)
        cases["wide_45"] = (1600, 1200) + wr.direction(45.0, 3 * ONE) + (2,)
        cases["wide_k16"] = (1600 + 3, 1200 - 7) + wr.direction(-30.0, ONE // 2) + (16,)
        cases["wide_axis"] = (1600, 1200, 0, 7 * ONE, 1)
        per = dict((k, set(wr.tile_paths(150, 200, w, S))) for k, w in cases.items())
        assert "direct" in per["wide_45"] and "direct" in per["wide_k16"] and "direct" in per["dwarf"]
        assert per["enlarge"] == {"lds"} and per["still"] == {"lds"} and per["k16_east"] == {"lds"}
        assert any(p >= {"lds", "direct", "empty"} for p in per.values())       # one picture, all three kinds of tile
        _both_layouts(bare_ctx, [fr] * len(cases), list(cases.values()), S, list(cases), arrays=[f] * len(cases))
    fr.release()


def test_a_1080p_frame_staged_and_direct(bare_ctx):
    f = tr.picture(1080, 1920, 5)
    fr = bare_ctx.upload(f)
    # the direct path alone: K = 16 at 45 degrees and a sub-step of about a pixel: a tile spans some 360 x 360 source pixels
    S = 32
    direct = [(16 * 900 + 3, 16 * 500 + 9) + wr.direction(45.0, ONE) + (16,), (16 * 30, 16 * 1060) + wr.direction(-135.0, ONE - 77) + (16,)]
    assert set(wr.tile_paths(1080, 1920, direct[0], S)) == {"direct"}
    assert set(wr.tile_paths(1080, 1920, direct[1], S)) == {"direct", "lds"}                   # in the frame's corner: what the frame clips is staged
    _both_layouts(bare_ctx, [fr] * 2, direct, S, arrays=[f] * 2)
    # face-sized aligned windows: staged, every tile of them
    rng = np.random.RandomState(8)
    for S in (96, 112):
        wins = []
        for side, deg in ((80, 5.0), (150, -30.0), (224, 12.0), (333, 29.0), (112, -90.0)):
            c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
            wins.append(wr.quantise_oriented(float(rng.randint(200, 1700)), float(rng.randint(200, 900)), float(side), c, s, S))
        wins.append(wr.quantise_oriented(1915.0, 1075.0, 200.0, np.cos(0.3), np.sin(0.3), S))      # across the last pixel
        assert set(w[4] for w in wins) >= {1, 2, 3}
        assert all(set(wr.tile_paths(1080, 1920, w, S)) == {"lds"} for w in wins[:3])        # (the 333-pixel face at 29 degrees may go either way)
        _same(bare_ctx.frame_warps([fr] * len(wins), wins, S), wr.warps([f] * len(wins), wins, S))
        _same(bare_ctx.frame_warps([fr] * 2, wins[2:4], S, "yuv420", "709"), wr.warps([f] * 2, wins[2:4], S, "yuv420", "709"))
    fr.release()


# ---- output --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full_range", [("601", False), ("709", False), ("601", True), ("709", True)])
def test_colour_flags_and_the_renderer(bare_ctx, matrix, full_range):
    f = frame("97x61")
    for S in (11, 17):                                              # odd: the last chroma row and column count a pixel twice
        cases = wr.window_cases(61, 97, S)
        rgb = _both_layouts(bare_ctx, [f] * len(cases), list(cases.values()), S, list(cases), matrix, full_range)
        wins = list(cases.values())[:4]
        assert np.array_equal(bare_ctx.frame_warps([f] * 4, wins, S, "rgb", matrix, full_range), bare_ctx.frame_warps([f] * 4, wins, S))
        # existing product code converts the RGB picture to the same planes
        pick = [list(cases).index(k) for k in ("any_1", "diagonal_k2", "corner_br", "outside_left")]
        got = bare_ctx.frame_warps([f] * len(pick), [list(cases.values())[i] for i in pick], S, "yuv420", matrix, full_range)
        for g, i in zip(got, pick):
            assert np.array_equal(g[None], bare_ctx.render([rgb[i]], None, S, S, matrix, full_range))


def _mixed(n, S):
    names = list(GEOMETRIES)
    frames, wins = [], []
    for i in range(n):
        f = frame(names[i % 4])
        c = list(wr.window_cases(f.shape[0], f.shape[1], S).values())
        frames.append(f); wins.append(c[(7 * i) % len(c)])
    return frames, wins


def test_batches_single_warps_and_rounds(bare_ctx):
    S = 10
    frames, wins = _mixed(40, S)
    ref = wr.warps(frames, wins, S)
    got = bare_ctx.frame_warps(frames, wins, S)
    _same(got, ref)
    for i in range(0, 40, 3):                                       # one call per picture gives what the batch gives
        assert np.array_equal(bare_ctx.frame_warps([frames[i]], [wins[i]], S)[0], ref[i])
    yuv = bare_ctx.frame_warps(frames, wins, S, "yuv420")
    for rnd in ("1", "3", "7", "13", "39", "40"):                   # 40, 14, 6 and 4 rounds with a last partial one; one round
        os.environ["PVF_CROP_ROUND"] = rnd
        try:
            assert np.array_equal(bare_ctx.frame_warps(frames, wins, S), got), rnd
            assert np.array_equal(bare_ctx.frame_warps(frames, wins, S, "yuv420"), yuv), rnd
        finally:
            del os.environ["PVF_CROP_ROUND"]
    assert bare_ctx.frame_warps([], np.zeros((0, 5), np.int32), S).shape == (0, S, S, 3)       # n = 0
    # the two calls share the rounds' buffers: one after the other, in any order, disturbs neither
    cw = [(16 * 2, 16 * 1, 16 * S)] * 40
    crops = tr.crops(frames, cw, S)
    os.environ["PVF_CROP_ROUND"] = "7"
    try:
        assert np.array_equal(bare_ctx.frame_crops(frames, cw, S), crops) and np.array_equal(bare_ctx.frame_warps(frames, wins, S), got)
        assert np.array_equal(bare_ctx.frame_crops(frames, cw, S), crops)
    finally:
        del os.environ["PVF_CROP_ROUND"]


def test_where_the_output_lies(bare_ctx):
    from pyannote_video_amd import _lib
    S = 7
    frames, wins = _mixed(9, S)
    ref = wr.warps(frames, wins, S)
    staged = [bare_ctx.upload(f) for f in frames]
    hs = np.array([f.handle for f in staged], np.uint64)
    w = np.ascontiguousarray(wins, np.int32)
    for layout, flags, want in (("rgb", 0, ref), ("yuv420", 4, np.stack([tr.to_yuv(p) for p in ref]))):
        nb = want[0].size * 9
        for off in range(4):                                        # host memory at four alignments, the bytes around it untouched
            buf = np.full(nb + 16, 0xA5, np.uint8)
            os.environ["PVF_CROP_ROUND"] = "4"
            try:
                assert bare_ctx._l.pvf_frame_warps(bare_ctx._h, _lib.ptr(hs), _lib.ptr(w), 9, S, flags, buf[8 + off:].ctypes.data, 0) == 0
            finally:
                del os.environ["PVF_CROP_ROUND"]
            assert np.array_equal(buf[8 + off:8 + off + nb], want.reshape(-1)) and (buf[:8 + off] == 0xA5).all() and (buf[8 + off + nb:] == 0xA5).all()
        for off in (0, 1):                                          # device memory
            dev = torch.full((nb + 16,), 0x5A, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert bare_ctx.frame_warps(staged, wins, S, layout, out_ptr=dev.data_ptr() + 8 + off) is None
            back = dev.cpu().numpy()
            assert np.array_equal(back[8 + off:8 + off + nb], want.reshape(-1)) and (back[:8 + off] == 0x5A).all() and (back[8 + off + nb:] == 0x5A).all()
    for f in staged:
        f.release()


def test_identity_windows_equal_the_axis_aligned_kernel(bare_ctx):
    """the windows both kernels can express: whole-pixel windows at 1 : 1, and at 2 : 1 with K = 2 (a 2 x 2 area average either way)"""
    for name in GEOMETRIES:
        f = frame(name)
        h, w = f.shape[:2]
        for S in (1, 6, 17, 33):
            spots = [(0, 0), (3, 2), (w - S // 2, h - S // 2), (-S // 2, -3), (w - 1, h - 1), (w + 5, 0)]
            crops = bare_ctx.frame_crops([f] * len(spots), [(16 * x, 16 * y, 16 * S) for x, y in spots], S)
            _same(bare_ctx.frame_warps([f] * len(spots), [wr.identity(x, y, S) for x, y in spots], S), crops)
            half = bare_ctx.frame_crops([f] * len(spots), [(16 * x, 16 * y, 32 * S) for x, y in spots], S, "yuv420", "709", True)
            _same(bare_ctx.frame_warps([f] * len(spots), [(16 * x + 16 * S, 16 * y + 16 * S, ONE, 0, 2) for x, y in spots], S, "yuv420", "709", True), half)


def test_refusals(bare_ctx):
    from pyannote_video_amd import _lib
    c, l, P = bare_ctx, bare_ctx._l, _lib.ptr
    f = c.upload(frame("64x48"))
    gone = c.upload(frame("50x37"))
    gone_handle = gone.handle
    gone.release()
    hs = np.array([f.handle, f.handle], np.uint64)
    good = np.array([[500, 400, ONE, 0, 1], [480, 333, 40000, -30000, 2]], np.int32)
    out = np.zeros((2, 6, 6, 3), np.uint8)
    ref = wr.warps([frame("64x48")] * 2, good, 6)
    assert ref.any()

    def wins(*rows):
        return np.array(rows, np.int32)
    ok = (0, 0, ONE, 0, 1)
    for call, message in ((lambda: l.pvf_frame_warps(c._h, P(hs), P(good), -1, 6, 0, P(out), 0), "PVF_CROP_MAX_CROPS"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(good), wr.MAX_CROPS + 1, 6, 0, P(out), 0), "PVF_CROP_MAX_CROPS"),
                          (lambda: l.pvf_frame_warps(c._h, None, P(good), 2, 6, 0, P(out), 0), "null frames, windows or output"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), None, 2, 6, 0, P(out), 0), "null frames, windows or output"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(good), 2, 6, 0, None, 0), "null frames, windows or output"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(good), 2, 0, 0, P(out), 0), "PVF_CROP_MIN_SIZE"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(good), 2, wr.MAX_SIZE + 1, 0, P(out), 0), "PVF_CROP_MAX_SIZE"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(wins(ok, (0, 0, ONE, 0, 0))), 2, 6, 0, P(out), 0), "PVF_WARP_MAX_K"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(wins((0, 0, ONE, 0, 17), ok)), 2, 6, 0, P(out), 0), "PVF_WARP_MAX_K"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(wins(ok, (0, 0, ONE, 0, -1))), 2, 6, 0, P(out), 0), "PVF_WARP_MAX_K"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(wins((0, 0, wr.MAX_STEP + 1, 0, 1), ok)), 2, 6, 0, P(out), 0), "PVF_WARP_MAX_STEP"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(wins(ok, (0, 0, -wr.MAX_STEP - 1, 0, 1))), 2, 6, 0, P(out), 0), "PVF_WARP_MAX_STEP"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(wins(ok, (0, 0, 0, wr.MAX_STEP + 1, 1))), 2, 6, 0, P(out), 0), "PVF_WARP_MAX_STEP"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(wins((0, 0, 0, -wr.MAX_STEP - 1, 16), ok)), 2, 6, 0, P(out), 0), "PVF_WARP_MAX_STEP"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(wins((wr.MAX_COORD + 1, 0, ONE, 0, 1), ok)), 2, 6, 0, P(out), 0), "PVF_CROP_MAX_COORD"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(wins(ok, (-wr.MAX_COORD - 1, 0, ONE, 0, 1))), 2, 6, 0, P(out), 0), "PVF_CROP_MAX_COORD"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(wins(ok, (0, wr.MAX_COORD + 1, ONE, 0, 1))), 2, 6, 0, P(out), 0), "PVF_CROP_MAX_COORD"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(wins((0, -wr.MAX_COORD - 1, ONE, 0, 1), ok)), 2, 6, 0, P(out), 0), "PVF_CROP_MAX_COORD"),
                          (lambda: l.pvf_frame_warps(c._h, P(np.array([f.handle, 987654321], np.uint64)), P(good), 2, 6, 0, P(out), 0), "unknown frame handle"),
                          (lambda: l.pvf_frame_warps(c._h, P(np.array([gone_handle, f.handle], np.uint64)), P(good), 2, 6, 0, P(out), 0), "unknown frame handle"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(good), 2, 6, 8, P(out), 0), "unknown flags"),
                          (lambda: l.pvf_frame_warps(c._h, P(hs), P(good), 2, 6, -1, P(out), 0), "unknown flags")):
        assert call() != 0, message
        err = l.pvf_last_error().decode()
        assert message in err, (message, err)
        assert not out.any()                                        # refused before any work
        assert l.pvf_frame_warps(c._h, P(hs), P(good), 2, 6, 0, P(out), 0) == 0 and np.array_equal(out, ref)       # the context goes on
        out[:] = 0
    assert l.pvf_frame_warps(c._h, None, None, 0, 6, 0, None, 0) == 0                # n = 0 does nothing
    with pytest.raises(ValueError, match="one frame per window"):
        c.frame_warps([f], good, 6)
    with pytest.raises(ValueError, match="layout must be"):
        c.frame_warps([f, f], good, 6, "nv12")
    f.release()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,region", [("y4m", "face"), ("npy", "face"), ("y4m", "mouth"), ("npy", "mouth")])
def test_aligned_tube_verb_in_a_process_of_its_own(tmp_path, fmt, region):
    from pyannote_video_amd import cli, faces, formats, models, pipeline
    from tests.test_gpu_chip_edges import landmarks
    spec, fps = "synthetic:640x360x9:2:3:7", 25.0
    video = cli.open_video(spec, fps)
    mean = np.stack([np.asarray(models.DLIB_MEAN_FACE_X), np.asarray(models.DLIB_MEAN_FACE_Y)], 1)
    # three hand-made tracks: one in the middle that drifts and rolls, one on the left edge (partly off the frame) tilted by 25 degrees,
    # one that starts on frame 3 and rolls the other way through the vertical
    geo = {0: lambda i: (300 + 2 * i, 170 + i, 90 + i, 4 * i), 1: lambda i: (14 - i, 200, 80, 25), 2: lambda i: (520, 120 + 3 * i, 70, -75 - 5 * i)}
    first = {0: 0, 1: 0, 2: 3}
    box = lambda g: ((g[0] - g[2] / 2) / 640.0, (g[1] - g[2] / 2) / 360.0, (g[0] + g[2] / 2) / 640.0, (g[1] + g[2] / 2) / 360.0)
    tp, lp, ip, out = (str(tmp_path / n) for n in ("track.txt", "landmarks.txt", "index.txt", "tubes"))
    formats.write_tracks(tp, [[(i / fps, box(geo[k](i)), "forward") for i in range(first[k], 9)] for k in (0, 1, 2)])
    rows = formats.read_tracks(tp)
    times = [i / fps for i in range(9)]
    with open(lp, "wb") as f:
        for fi, T, g in pipeline.faces_per_frame(rows, times, 640, 360):
            for ident, _ in g:
                f.write(formats.landmark_rows([T], [ident], landmarks(mean, *geo[ident](fi))[None], 640, 360))
    F = faces.landmark_faces(rows, formats.read_landmarks(lp), times, 640, 360)
    if region == "face":                                            # every face of the tracking file, with its points where it has a landmark row
        pts = dict(((tr.ms(x[0]), x[1]), x[4]) for x in F)
        F = [(T, ident, fi, b, pts.get((tr.ms(T), ident))) for fi, T, g in pipeline.faces_per_frame(rows, times, 640, 360, drop_last=False) for ident, b in g]
    frames = [video.frame(i) for i in range(9)]
    S = 48 if region == "face" else 64                              # face tubes reduce (K > 1), mouth tubes enlarge
    want, index = wr.tube_files(frames, F, S, fmt, "709", True, region=region, smooth_window=0.1)
    assert len(want) == 3 and len(index) >= 18
    ks = [int(line.split()[8]) for line in index]
    assert all(k > 1 for k in ks) if region == "face" else all(k == 1 for k in ks)
    assert len(set(tuple(line.split()[6:8]) for line in index)) >= 12              # the windows turn with the faces
    assert any(abs(int(line.split()[7])) > abs(int(line.split()[6])) for line in index)      # some closer to the vertical than the horizontal
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pyannote-video_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "pyannote_video_amd", "--fps", str(fps), "tube", "--align", "--size", str(S), "--region", region,
                          "--smooth", "0.1", "--format", fmt, "--matrix", "709", "--range", "full", "--index", ip, spec, tp, lp, out],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    assert sorted(os.listdir(out)) == sorted(want)
    for name, data in want.items():
        assert open(os.path.join(out, name), "rb").read() == data, name
    assert open(ip).read() == "".join(index)
