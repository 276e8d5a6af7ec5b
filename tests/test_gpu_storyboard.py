"""GPU: the `storyboard` verb's kernels (csrc/board.hip) bit for bit against STORYBOARD.md as tests/storyboard_ref.py restates it:
the case table of tests/storyboard_cases.py (row alignments, ratios, the kernel's seams, contents), the 64-bit sum, how a call is made
(batches, rounds, where the output lies), where the frames came from, full-size frames, the sheet, every refusal of the two entries,
and the verbs end to end in processes of their own."""
import json
import os
import subprocess
import sys

import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships
import numpy as np
import pytest

from tests import storyboard_cases as sc, storyboard_ref as sr
from tests.test_gpu_faces import bare_ctx      # noqa: F401 -- fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = sc.cases()
GROUPS = sorted(set(c.name for c in TABLE))


def _same(got, want, what=None):
    bad = sr.mismatch(got, want)
    assert bad is None, (what, bad)


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


class rounds(object):
    """PVF_THUMB_ROUND for the calls of a block"""

    def __init__(self, n):
        self.n = str(n)

    def __enter__(self):
        os.environ["PVF_THUMB_ROUND"] = self.n

    def __exit__(self, *a):
        del os.environ["PVF_THUMB_ROUND"]


# ---- the thumbnail ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_the_case_table_equals_the_restatement(bare_ctx, group):
    by_frame = {}
    for c in TABLE:
        if c.name == group:
            by_frame.setdefault((c.w, c.h, c.content), []).append(c)
    assert by_frame
    for cases in by_frame.values():
        f = sc.make_frame(cases[0])
        dev = bare_ctx.upload(f)
        for c in cases:
            got = bare_ctx.frame_thumbs([dev], c.tw, c.th)
            _same(got[0], sr.thumb(f, c.tw, c.th), c)
        dev.release()


def test_the_sum_of_a_pixel_is_64_bit(bare_ctx):
    c = sc.BIG
    assert 255 * c.w * c.h > 1 << 32
    dev = bare_ctx.upload(np.full((c.h, c.w, 3), 255, np.uint8))              # one upload of 50 MB
    for tw, th in sc.BIG_TARGETS:
        got = bare_ctx.frame_thumbs([dev], tw, th)
        assert got.shape == (1, th, tw, 3) and (got == 255).all(), (tw, th, got.tolist())
    dev.release()


def test_batches_rounds_and_where_the_output_lies(bare_ctx):
    from pyannote_video_amd import _lib
    h, w, tw, th = 21, 33, 7, 5
    frames = [noise(h, w, 50 + i) for i in range(257)]
    want = sr.thumbs(frames, tw, th)
    staged = [bare_ctx.upload(f) for f in frames]
    for n in (1, 2, 257):
        _same(bare_ctx.frame_thumbs(staged[:n], tw, th), want[:n], n)
    for rnd in (1, 3, 100, 256, 257, 300):                          # rounds that end inside, at and past the call: nothing moves
        with rounds(rnd):
            _same(bare_ctx.frame_thumbs(staged, tw, th), want, rnd)
    assert bare_ctx.frame_thumbs([], tw, th).shape == (0, th, tw, 3)            # n = 0
    hs = np.array([f.handle for f in staged[:9]], np.uint64)
    nb = want[:9].size
    for off in range(4):                                            # host memory at four alignments, the bytes around it untouched
        buf = np.full(nb + 16, 0xA5, np.uint8)
        with rounds(4):
            assert bare_ctx._l.pvf_frame_thumbs(bare_ctx._h, _lib.ptr(hs), 9, tw, th, 0, buf[8 + off:].ctypes.data, 0) == 0
        assert np.array_equal(buf[8 + off:8 + off + nb], want[:9].reshape(-1)) and (buf[:8 + off] == 0xA5).all() and (buf[8 + off + nb:] == 0xA5).all()
    for off in (0, 1):                                              # device memory
        dev = torch.full((nb + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with rounds(4):
            assert bare_ctx.frame_thumbs(staged[:9], tw, th, out_ptr=dev.data_ptr() + 8 + off) is None
        back = dev.cpu().numpy()
        assert np.array_equal(back[8 + off:8 + off + nb], want[:9].reshape(-1)) and (back[:8 + off] == 0x5A).all() and (back[8 + off + nb:] == 0x5A).all()
    for f in staged:
        f.release()


def test_frames_from_the_rings_and_from_resize(bare_ctx):
    from pyannote_video_amd.y4m import YuvFrame
    from tests import yuv_ref
    from tests.test_gpu_yuv import _download
    h, w = 270, 480
    clip = [noise(h, w, 70 + i) for i in range(12)]
    ring = bare_ctx.ingest_ring(h, w, depth=4)
    devs = [ring.push(f) for f in clip]                             # uploads still in flight: the call waits for every frame's event
    got = bare_ctx.frame_thumbs(devs, 40, 23)
    ring.close()
    _same(got, sr.thumbs(clip, 40, 23), "rgb ring")
    for d in devs:
        d.release()
    planes = [yuv_ref.noise_planes(h, w, "420", 90 + i) for i in range(12)]
    yring = bare_ctx.ingest_ring_yuv(h, w, layout="420", depth=4)
    devs = [yring.push(YuvFrame(*p)) for p in planes]
    got = bare_ctx.frame_thumbs(devs, 40, 23)
    yring.close()
    _same(got, sr.thumbs([yuv_ref.to_rgb(*p) for p in planes], 40, 23), "yuv ring")
    for d in devs:
        d.release()
    src = bare_ctx.upload(clip[0])
    small = bare_ctx.resize(src, 101, 57)
    got = bare_ctx.frame_thumbs([small, small], 13, 9)
    _same(got, sr.thumbs([_download(bare_ctx, small)] * 2, 13, 9), "resize")
    small.release()
    src.release()


@pytest.mark.parametrize("h,w", [(1080, 1920), (2160, 3840)])
def test_a_full_size_frame(bare_ctx, h, w):
    f = noise(h, w, h)
    f[: h // 3] |= 0xC0                          # not all of it averages to 127
    dev = bare_ctx.upload(f)
    got = bare_ctx.frame_thumbs([dev], 160, 90)
    dev.release()
    _same(got[0], sr.thumb(f, 160, 90))


# ---- the sheet ----------------------------------------------------------------------------------------------------------------------
PRIMS = [(0, 2, 1, 30, 12, (255, 0, 0)), (1, -5, -5, 60, 40, (0, 255, 0)), (2, 4, 20, (0, 0, 255), 2, b"shot 12"), (2, -3, 5, (9, 9, 9), 1, b"A"),
         (0, 40, 3, 47, 6, (1, 2, 3))]


def tiles(n, th, tw, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, th, tw, 3), dtype=np.uint8)


@pytest.mark.parametrize("tw,th", [(13, 7), (1, 1), (40, 33)])
def test_thumb_sheet_edges_corners_outside_overlap(bare_ctx, tw, th):
    W, H = 97, 61
    xy = [(-tw // 2, -th // 2), (W - tw // 2 - 1, -1), (-1, H - th // 2 - 1), (W - 1, H - 1), (W // 2, -th + 1), (W // 2, H - 1), (-tw + 1, H // 2),
          (W - 1, H // 2), (-tw, 5), (W, 5), (5, -th), (5, H), (-2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, -2 ** 31), (30, 20), (30 + tw // 2, 20 + th // 2),
          (30, 20), (0, 0)]
    t = tiles(len(xy), th, tw)
    _same(bare_ctx.thumb_sheet(t, xy, W, H, (10, 20, 30)), sr.sheet(t, xy, W, H, (10, 20, 30)))
    _same(bare_ctx.thumb_sheet(t, xy, W, H, (10, 20, 30), PRIMS), sr.sheet(t, xy, W, H, (10, 20, 30), PRIMS))
    assert sr.mismatch(sr.sheet(t, xy, W, H, (10, 20, 30), first_wins=True), sr.sheet(t, xy, W, H, (10, 20, 30))) is not None


@pytest.mark.parametrize("W,H", [(1, 1), (49, 7), (16384, 4)])
def test_thumb_sheet_sheet_sizes_and_no_tiles(bare_ctx, W, H):
    t = tiles(3, 5, 6)
    xy = [(0, 0), (W - 3, H - 2), (W // 2, 1)]
    _same(bare_ctx.thumb_sheet(t, xy, W, H, (3, 2, 1), PRIMS), sr.sheet(t, xy, W, H, (3, 2, 1), PRIMS))
    none = np.zeros((0, 5, 6, 3), np.uint8)
    _same(bare_ctx.thumb_sheet(none, [], W, H, (3, 2, 1), PRIMS), sr.sheet(none, [], W, H, (3, 2, 1), PRIMS))
    _same(bare_ctx.thumb_sheet(none, [], W, H, (255, 0, 128)), sr.sheet(none, [], W, H, (255, 0, 128)))


def test_thumb_sheet_across_rounds_the_last_tile_of_the_list_wins(bare_ctx):
    n = 300
    t = tiles(n, 20, 30)
    xy = np.full((n, 2), -1000, np.int32)
    on = {3: (0, 0), 255: (20, 10), 256: (30, 15), 299: (10, 30), 7: (100, 5), 298: (110, 20), 257: (160, 40), 9: (170, 45)}
    for i, c in on.items():
        xy[i] = c
    want = sr.sheet(t, xy, 240, 110, (40, 40, 40))
    _same(bare_ctx.thumb_sheet(t, xy, 240, 110, (40, 40, 40)), want)
    for rnd in (1, 7, 256, 299, 300):
        with rounds(rnd):
            _same(bare_ctx.thumb_sheet(t, xy, 240, 110, (40, 40, 40)), want, rnd)
    assert np.array_equal(want[50, 175], t[257][10, 15])           # 257 (a later round) over 9 (an earlier one), though 9 is placed later on the sheet


def test_thumb_sheet_of_chips_is_chip_sheet_at_150(bare_ctx):
    chips = tiles(7, 150, 150, seed=11)
    xy = [(-40, -20), (100, 10), (180, 90), (420, 200), (421, 201), (0, 300), (500, -100)]
    a = bare_ctx.chip_sheet(chips, xy, 150, 600, 400, (5, 6, 7), PRIMS)
    b = bare_ctx.thumb_sheet(chips, xy, 600, 400, (5, 6, 7), PRIMS)
    _same(b, a)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_frame_thumbs(bare_ctx):
    from pyannote_video_amd import _lib
    c, l, P = bare_ctx, bare_ctx._l, _lib.ptr
    fa, fb = noise(12, 20, 1), noise(13, 20, 2)
    a, b, gone = c.upload(fa), c.upload(fb), c.upload(fb)
    gone_handle = gone.handle
    gone.release()
    hs = np.array([a.handle, a.handle], np.uint64)
    out = np.zeros((2, 3, 4, 3), np.uint8)
    ref = sr.thumbs([fa, fa], 4, 3)

    def call(frames=hs, n=2, tw=4, th=3, flags=0, o=out):
        return l.pvf_frame_thumbs(c._h, P(frames) if frames is not None else None, n, tw, th, flags, P(o) if o is not None else None, 0)
    for kw, message in ((dict(n=-1), "PVF_THUMB_MAX_FRAMES"), (dict(n=65537), "PVF_THUMB_MAX_FRAMES"), (dict(frames=None), "null frames or output"),
                        (dict(o=None), "null frames or output"), (dict(tw=0), "PVF_THUMB_MAX_SIDE"), (dict(tw=1025), "PVF_THUMB_MAX_SIDE"),
                        (dict(th=0), "PVF_THUMB_MAX_SIDE"), (dict(th=1025), "PVF_THUMB_MAX_SIDE"), (dict(th=-3), "PVF_THUMB_MAX_SIDE"),
                        (dict(flags=1), "unknown flags"), (dict(flags=-1), "unknown flags"),
                        (dict(frames=np.array([a.handle, 987654321], np.uint64)), "unknown frame handle"),
                        (dict(frames=np.array([gone_handle, a.handle], np.uint64)), "unknown frame handle"),
                        (dict(frames=np.array([a.handle, b.handle], np.uint64)), "frames of different sizes")):
        assert call(**kw) != 0, message
        assert message in l.pvf_last_error().decode(), (message, l.pvf_last_error().decode())
        assert not out.any()                                        # refused before any work
        assert call() == 0 and np.array_equal(out, ref)             # the context goes on
        out[:] = 0
    assert l.pvf_frame_thumbs(c._h, None, 0, 4, 3, 0, None, 0) == 0                  # n = 0 does nothing
    a.release()
    b.release()


def test_refusals_of_thumb_sheet(bare_ctx):
    from pyannote_video_amd import _lib, render
    c, l, P = bare_ctx, bare_ctx._l, _lib.ptr
    t = tiles(2, 3, 4)
    xy = np.array([[0, 0], [5, 2]], np.int32)
    _, prims, text = render.pack_primitives([PRIMS])
    out = np.zeros((8, 12, 3), np.uint8)
    ref = sr.sheet(t, xy, 12, 8, (1, 2, 3), PRIMS)

    def call(th_=t, n=2, xy_=xy, tw=4, th=3, W=12, H=8, bg=1 | 2 << 8 | 3 << 16, p=prims, np_=None, tx=text, tb=None, o=out):
        return l.pvf_thumb_sheet(c._h, P(th_) if th_ is not None else None, n, P(xy_) if xy_ is not None else None, tw, th, W, H, bg,
                                 P(p) if p is not None else None, len(prims) if np_ is None else np_, P(tx) if tx is not None else None,
                                 len(text) if tb is None else tb, P(o) if o is not None else None)

    def with_prim(row):
        q = prims.copy()
        q[0] = row
        return q
    for kw, message in ((dict(n=-1), "PVF_SHEET_MAX_TILES"), (dict(n=65537), "PVF_SHEET_MAX_TILES"), (dict(th_=None), "null thumbnails"),
                        (dict(xy_=None), "null tile corners"), (dict(tw=0), "PVF_THUMB_MAX_SIDE"), (dict(th=1025), "PVF_THUMB_MAX_SIDE"),
                        (dict(W=0), "PVF_SHEET_MAX_SIDE"), (dict(H=16385), "PVF_SHEET_MAX_SIDE"), (dict(W=16384, H=4097), "PVF_SHEET_MAX_PIXELS"),
                        (dict(o=None), "null output"), (dict(bg=1 << 24), "background"), (dict(np_=4097), "PVF_RENDER_MAX_PRIMS"),
                        (dict(np_=-1), "PVF_RENDER_MAX_PRIMS"), (dict(p=None), "null primitive list"), (dict(tb=(1 << 20) + 1), "PVF_RENDER_MAX_TEXT"),
                        (dict(tx=None), "null text pool"), (dict(p=with_prim((3, 0, 0, 5, 5, 0, 2, 0))), "takes no redactions"),
                        (dict(p=with_prim((7, 0, 0, 5, 5, 0, 0, 0))), "unknown primitive type"),
                        (dict(p=with_prim((2, 0, 0, 0, 65, 0, 1, 0))), "PVF_RENDER_MAX_RUN"),
                        (dict(p=with_prim((2, 0, 0, len(text), 1, 0, 1, 0))), "outside the text pool"),
                        (dict(p=with_prim((2, 0, 0, 0, 1, 0, 0, 0))), "PVF_RENDER_MAX_SCALE")):
        assert call(**kw) != 0, message
        assert message in l.pvf_last_error().decode(), (message, l.pvf_last_error().decode())
        assert not out.any()                                        # refused before any work
        assert call() == 0 and np.array_equal(out, ref)             # the context goes on
        out[:] = 0
    with pytest.raises(ValueError, match="tile corners"):
        c.thumb_sheet(t, xy[:1], 12, 8)
    with pytest.raises(ValueError, match="thumbnails are"):
        c.thumb_sheet(t[0], xy, 12, 8)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_the_verbs_in_processes_of_their_own(tmp_path, small_video):
    fps = small_video.frame_rate
    spec, sp, tp, scp, out, ip = (str(tmp_path / n) for n in ("video.npy", "shot.json", "thread.json", "scene.json", "board.ppm", "index.txt"))
    np.save(spec, np.stack([small_video.frame(i) for i in range(len(small_video))]))        # the fixture's frames, as a video the verbs read
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pyannote-video_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for args in (["shot", spec, sp], ["thread", spec, sp, tp], ["scene", spec, tp, scp],
                 ["storyboard", "--thread", scp, "--by", "thread", "--per", "3", "--index", ip, spec, sp, out]):
        run = subprocess.run([sys.executable, "-m", "pyannote_video_amd", "--fps", str(fps)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             env=env, timeout=600)
        assert run.returncode == 0, (args, run.stderr.decode()[-2000:])
    shots = [(s["start"], s["end"]) for s in json.load(open(sp))["content"]]
    tracks = sorted((i["segment"]["start"], i["segment"]["end"], str(i["track"]), i["label"]) for i in json.load(open(scp))["content"])
    assert shots and tracks
    labels = sr.labels_of(shots, [(a, b, l) for a, b, _, l in tracks])
    want, lines = sr.board(small_video.frame, shots, labels, fps, len(small_video), 640, 360, per=3, width=160, by="thread")
    assert open(out, "rb").read() == b"P6\n%d %d\n255\n" % (want.shape[1], want.shape[0]) + want.tobytes()
    assert open(ip).read() == lines and len(lines.splitlines()) >= len(shots)
