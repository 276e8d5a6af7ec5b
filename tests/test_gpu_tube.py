"""GPU: the `tube` verb's kernel (csrc/tube.hip) bit for bit against TUBE.md as tests/tube_ref.py restates it: the named windows on
frames of every byte length mod 4 and every base alignment, every sub-pixel phase, the picture sizes on the seams of the kernel's
column pieces and row bands, both layouts and all colour flags (and pvf_render_batch as an independent check of the YUV form), how a
call is made (batches, single crops, rounds, where the output lies), large frames, every refusal of the C ABI, and the verb end to
end in a process of its own."""
import os
import subprocess
import sys

import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships
import numpy as np
import pytest

from tests import tube_ref as tr
from tests.test_gpu_faces import bare_ctx      # noqa: F401 -- fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = {"64x48": (48, 64), "97x61": (61, 97), "50x37": (37, 50), "33x23": (23, 33)}        # bytes: 4k, 4k + 3, 4k + 2, 4k + 1
# the minimum, an odd one, 63 / 64 / 65, and the sizes on the seams of the kernel: its row band and its column piece
SIZES = [tr.MIN_SIZE, 7, 63, 64, 65, tr.C_BAND - 1, tr.C_BAND, tr.C_BAND + 1, tr.C_COLS - 1, tr.C_COLS, tr.C_COLS + 1]
_FRAMES = {}


def frame(name):
    if name not in _FRAMES:
        h, w = GEOMETRIES[name]
        _FRAMES[name] = tr.picture(h, w, len(_FRAMES) + 10)
    return _FRAMES[name]


def _same(got, ref, names=None):
    assert got.shape == ref.shape and got.dtype == np.uint8, (got.shape, ref.shape)
    bad = [i for i in range(len(ref)) if not np.array_equal(got[i], ref[i])]
    assert not bad, [(names[i] if names else i, int((got[i] != ref[i]).sum()), np.argwhere(got[i] != ref[i])[:3].tolist()) for i in bad[:6]]


def _both_layouts(ctx, frames, windows, S, names=None, matrix="601", full_range=False):
    rgb = tr.crops(frames, windows, S)
    _same(ctx.frame_crops(frames, windows, S), rgb, names)
    yuv = np.stack([tr.to_yuv(p, matrix, full_range) for p in rgb])
    _same(ctx.frame_crops(frames, windows, S, "yuv420", matrix, full_range), yuv, names)
    return rgb


def test_geometries_have_every_byte_length():
    assert [h * w * 3 % 4 for h, w in GEOMETRIES.values()] == [0, 3, 2, 1]


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_named_windows_equal_the_restatement(bare_ctx, name, S):
    f = frame(name)
    cases = tr.window_cases(f.shape[0], f.shape[1], S)
    rgb = _both_layouts(bare_ctx, [f] * len(cases), list(cases.values()), S, list(cases))
    by = dict(zip(cases, rgb))
    for k in ("outside_left", "outside_right", "outside_top", "outside_bottom", "cap_far", "cap_far2"):
        assert not by[k].any(), k                                   # black, not garbage
    if S <= min(f.shape[:2]):
        assert np.array_equal(by["identity"], f[:S, :S])
    assert by["last_pixel_only"].any()


@pytest.mark.parametrize("name", ["97x61", "33x23"])
def test_all_phases_at_the_seam(bare_ctx, name):
    f, S = frame(name), 5
    wins = tr.phase_windows(S)
    rgb = _both_layouts(bare_ctx, [f] * len(wins), wins, S)
    assert np.array_equal(rgb[0], f[1:6, 1:6])
    for L in (16 * S - 1, 16 * S + 1):
        w2 = [(x, y, L) for x, y, _ in wins]
        _same(bare_ctx.frame_crops([f] * len(w2), w2, S), tr.crops([f] * len(w2), w2, S))


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
        for S in (9, 16):
            cases = tr.window_cases(h, w, S)
            _same(bare_ctx.frame_crops([fr] * len(cases), list(cases.values()), S), tr.crops([f] * len(cases), list(cases.values()), S), list(cases))
        fr.release()


@pytest.mark.parametrize("matrix,full_range", [("601", False), ("709", False), ("601", True), ("709", True)])
def test_colour_flags_and_the_renderer(bare_ctx, matrix, full_range):
    f = frame("97x61")
    cases = tr.window_cases(61, 97, 11)
    _both_layouts(bare_ctx, [f] * len(cases), list(cases.values()), 11, list(cases), matrix, full_range)
    # the colour flags mean nothing to an RGB picture
    wins = list(cases.values())[:4]
    assert np.array_equal(bare_ctx.frame_crops([f] * 4, wins, 11, "rgb", matrix, full_range), bare_ctx.frame_crops([f] * 4, wins, 11))
    # a square frame through its whole-frame window is the frame: existing product code converts it to the same planes
    for side in (48, 37):
        sq = tr.picture(side, side, side)
        got = bare_ctx.frame_crops([sq], [(0, 0, 16 * side)], side, "yuv420", matrix, full_range)
        assert np.array_equal(got, bare_ctx.render([sq], None, side, side, matrix, full_range))
        assert np.array_equal(got[0], tr.to_yuv(sq, matrix, full_range))


def _mixed(n, S):
    names = list(GEOMETRIES)
    frames, wins = [], []
    for i in range(n):
        f = frame(names[i % 4])
        c = list(tr.window_cases(f.shape[0], f.shape[1], S).values())
        frames.append(f); wins.append(c[(7 * i) % len(c)])
    return frames, wins


def test_batches_single_crops_and_rounds(bare_ctx):
    S = 10
    frames, wins = _mixed(40, S)
    ref = tr.crops(frames, wins, S)
    got = bare_ctx.frame_crops(frames, wins, S)
    _same(got, ref)
    for i in range(0, 40, 3):                                       # one call per crop gives what the batch gives
        assert np.array_equal(bare_ctx.frame_crops([frames[i]], [wins[i]], S)[0], ref[i])
    one = [frames[1]] * 40                                          # many crops of one frame
    _same(bare_ctx.frame_crops(one, wins, S), tr.crops(one, wins, S))
    yuv = bare_ctx.frame_crops(frames, wins, S, "yuv420")
    for rnd in ("1", "3", "7", "39", "40"):                         # rounds that end inside, at and past the call: nothing moves
        os.environ["PVF_CROP_ROUND"] = rnd
        try:
            assert np.array_equal(bare_ctx.frame_crops(frames, wins, S), got), rnd
            assert np.array_equal(bare_ctx.frame_crops(frames, wins, S, "yuv420"), yuv), rnd
        finally:
            del os.environ["PVF_CROP_ROUND"]
    assert bare_ctx.frame_crops([], np.zeros((0, 3), np.int32), S).shape == (0, S, S, 3)       # n = 0


def test_where_the_output_lies(bare_ctx):
    from pyannote_video_amd import _lib
    S = 7
    frames, wins = _mixed(9, S)
    ref = tr.crops(frames, wins, S)
    staged = [bare_ctx.upload(f) for f in frames]
    hs = np.array([f.handle for f in staged], np.uint64)
    w = np.ascontiguousarray(wins, np.int32)
    for layout, flags, want in (("rgb", 0, ref), ("yuv420", 4, np.stack([tr.to_yuv(p) for p in ref]))):
        nb = want[0].size * 9
        for off in range(4):                                        # host memory at four alignments, the bytes around it untouched
            buf = np.full(nb + 16, 0xA5, np.uint8)
            os.environ["PVF_CROP_ROUND"] = "4"
            try:
                assert bare_ctx._l.pvf_frame_crops(bare_ctx._h, _lib.ptr(hs), _lib.ptr(w), 9, S, flags, buf[8 + off:].ctypes.data, 0) == 0
            finally:
                del os.environ["PVF_CROP_ROUND"]
            assert np.array_equal(buf[8 + off:8 + off + nb], want.reshape(-1)) and (buf[:8 + off] == 0xA5).all() and (buf[8 + off + nb:] == 0xA5).all()
        for off in (0, 1):                                          # device memory
            dev = torch.full((nb + 16,), 0x5A, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert bare_ctx.frame_crops(staged, wins, S, layout, out_ptr=dev.data_ptr() + 8 + off) is None
            back = dev.cpu().numpy()
            assert np.array_equal(back[8 + off:8 + off + nb], want.reshape(-1)) and (back[:8 + off] == 0x5A).all() and (back[8 + off + nb:] == 0x5A).all()
    for f in staged:
        f.release()


def test_a_1080p_frame_with_face_sized_windows(bare_ctx):
    f = tr.picture(1080, 1920, 5)
    fr = bare_ctx.upload(f)
    rng = np.random.RandomState(8)
    for S in (112, 224):
        wins = [(int(rng.randint(-16 * 100, 16 * 1800)), int(rng.randint(-16 * 100, 16 * 900)), 16 * side + int(rng.randint(0, 16)))
                for side in (80, 150, 223, 224, 333, 600)]
        wins.append((16 * 1920 - 16 * 300, 16 * 1080 - 16 * 300, 16 * 300))       # touching the last pixel
        _same(bare_ctx.frame_crops([fr] * len(wins), wins, S), tr.crops([f] * len(wins), wins, S))
        _same(bare_ctx.frame_crops([fr] * 2, wins[4:6], S, "yuv420", "709"), tr.crops([f] * 2, wins[4:6], S, "yuv420", "709"))
    fr.release()


def test_a_2160p_frame_and_the_large_sums(bare_ctx):
    f = tr.picture(2160, 3840, 6)
    f[500:1500, 1000:3000] |= 0xC0                                  # bright, so that sums of 125 x 125 pixels pass 2^32 by far
    fr = bare_ctx.upload(f)
    wins = [(16 * 900 + 5, 16 * 100 + 9, 16 * 2000), (16 * 2500, -16 * 300, 16 * 2000 + 7)]
    _same(bare_ctx.frame_crops([fr] * 2, wins, 96), tr.crops([f] * 2, wins, 96))
    assert (16 * 2000) ** 2 * 192 > 2 ** 36                        # the vertical sums are far beyond 32 bits
    # a row piece of more than C_TILE_PX source pixels: the staged piece is cut, the sums are not
    wide = [(3, 16 * 200, 16 * 3840)]
    assert 3840 > tr.C_TILE_PX
    _same(bare_ctx.frame_crops([fr], wide, 3), tr.crops([f], wide, 3))
    fr.release()


def test_refusals(bare_ctx):
    from pyannote_video_amd import _lib
    c, l, P = bare_ctx, bare_ctx._l, _lib.ptr
    f = c.upload(frame("64x48"))
    gone = c.upload(frame("50x37"))
    gone_handle = gone.handle
    gone.release()
    hs = np.array([f.handle, f.handle], np.uint64)
    good = np.array([[0, 0, 160], [5, 7, 100]], np.int32)
    out = np.zeros((2, 6, 6, 3), np.uint8)
    ref = tr.crops([frame("64x48")] * 2, good, 6)

    def wins(*rows):
        return np.array(rows, np.int32)
    big = np.zeros((2, 3), np.int32)
    for call, message in ((lambda: l.pvf_frame_crops(c._h, P(hs), P(good), -1, 6, 0, P(out), 0), "PVF_CROP_MAX_CROPS"),
                          (lambda: l.pvf_frame_crops(c._h, P(hs), P(good), tr.MAX_CROPS + 1, 6, 0, P(out), 0), "PVF_CROP_MAX_CROPS"),
                          (lambda: l.pvf_frame_crops(c._h, None, P(good), 2, 6, 0, P(out), 0), "null frames, windows or output"),
                          (lambda: l.pvf_frame_crops(c._h, P(hs), None, 2, 6, 0, P(out), 0), "null frames, windows or output"),
                          (lambda: l.pvf_frame_crops(c._h, P(hs), P(good), 2, 6, 0, None, 0), "null frames, windows or output"),
                          (lambda: l.pvf_frame_crops(c._h, P(hs), P(good), 2, 0, 0, P(out), 0), "PVF_CROP_MIN_SIZE"),
                          (lambda: l.pvf_frame_crops(c._h, P(hs), P(good), 2, tr.MAX_SIZE + 1, 0, P(out), 0), "PVF_CROP_MAX_SIZE"),
                          (lambda: l.pvf_frame_crops(c._h, P(hs), P(wins((0, 0, 160), (0, 0, 15))), 2, 6, 0, P(out), 0), "PVF_CROP_MIN_SIDE"),
                          (lambda: l.pvf_frame_crops(c._h, P(hs), P(wins((0, 0, tr.MAX_SIDE + 1), (0, 0, 16))), 2, 6, 0, P(out), 0), "PVF_CROP_MAX_SIDE"),
                          (lambda: l.pvf_frame_crops(c._h, P(hs), P(wins((0, 0, -160), (0, 0, 16))), 2, 6, 0, P(out), 0), "PVF_CROP_MIN_SIDE"),
                          (lambda: l.pvf_frame_crops(c._h, P(hs), P(wins((tr.MAX_COORD + 1, 0, 160), (0, 0, 16))), 2, 6, 0, P(out), 0), "PVF_CROP_MAX_COORD"),
                          (lambda: l.pvf_frame_crops(c._h, P(hs), P(wins((0, 0, 160), (0, -tr.MAX_COORD - 1, 16))), 2, 6, 0, P(out), 0), "PVF_CROP_MAX_COORD"),
                          (lambda: l.pvf_frame_crops(c._h, P(np.array([f.handle, 987654321], np.uint64)), P(good), 2, 6, 0, P(out), 0), "unknown frame handle"),
                          (lambda: l.pvf_frame_crops(c._h, P(np.array([gone_handle, f.handle], np.uint64)), P(good), 2, 6, 0, P(out), 0), "unknown frame handle"),
                          (lambda: l.pvf_frame_crops(c._h, P(hs), P(good), 2, 6, 8, P(out), 0), "unknown flags"),
                          (lambda: l.pvf_frame_crops(c._h, P(hs), P(good), 2, 6, -1, P(out), 0), "unknown flags")):
        assert call() != 0, message
        assert message in l.pvf_last_error().decode(), (message, l.pvf_last_error().decode())
        assert not out.any()                                        # refused before any work
        assert l.pvf_frame_crops(c._h, P(hs), P(good), 2, 6, 0, P(out), 0) == 0 and np.array_equal(out, ref)       # the context goes on
        out[:] = 0
    assert l.pvf_frame_crops(c._h, None, None, 0, 6, 0, None, 0) == 0                # n = 0 does nothing
    with pytest.raises(ValueError, match="one frame per window"):
        c.frame_crops([f], good, 6)
    with pytest.raises(ValueError, match="layout must be"):
        c.frame_crops([f, f], good, 6, "nv12")
    del big
    f.release()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,region", [("y4m", "face"), ("npy", "face"), ("y4m", "mouth"), ("npy", "mouth")])
def test_tube_verb_in_a_process_of_its_own(tmp_path, fmt, region):
    from pyannote_video_amd import cli, faces, formats, models, pipeline
    from tests.test_gpu_chip_edges import landmarks
    spec, fps = "synthetic:640x360x9:2:3:7", 25.0
    video = cli.open_video(spec, fps)
    mean = np.stack([np.asarray(models.DLIB_MEAN_FACE_X), np.asarray(models.DLIB_MEAN_FACE_Y)], 1)
    # three hand-made tracks: one in the middle that drifts, one on the left edge (partly off the frame), one that starts on frame 3
    geo = {0: lambda i: (300 + 2 * i, 170 + i, 90 + i, i), 1: lambda i: (14 - i, 200, 80, 0), 2: lambda i: (520, 120 + 3 * i, 70, -2 * i)}
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
    if region == "mouth":
        F = faces.landmark_faces(rows, formats.read_landmarks(lp), times, 640, 360)
    else:
        F = [(T, ident, fi, b, None) for fi, T, g in pipeline.faces_per_frame(rows, times, 640, 360, drop_last=False) for ident, b in g]
    frames = [video.frame(i) for i in range(9)]
    S = 48 if region == "face" else 64                              # face tubes reduce, mouth tubes enlarge
    want, index = tr.tube_files(frames, F, S, fmt, "709", True, region=region, smooth_window=0.1)
    assert len(want) == 3 and len(index) >= 18
    sides = [int(line.split()[6]) for line in index]
    assert all(L > 16 * S for L in sides) if region == "face" else all(L < 16 * S for L in sides)
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pyannote-video_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "pyannote_video_amd", "--fps", str(fps), "tube", "--size", str(S), "--region", region, "--smooth", "0.1",
                          "--format", fmt, "--matrix", "709", "--range", "full", "--index", ip, spec, tp] + ([lp] if region == "mouth" else []) + [out],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    assert sorted(os.listdir(out)) == sorted(want)
    for name, data in want.items():
        assert open(os.path.join(out, name), "rb").read() == data, name
    assert open(ip).read() == "".join(index)
    if region == "face":                                            # the track on the left edge is partly black, the others are not
        a = np.load(os.path.join(out, "track_00001.npy")) if fmt == "npy" else None
        assert a is None or (not a[:, :, 0].any() and a.any())
