"""GPU: YUV frames at ingest (csrc/ingest.hip: yuv_to_rgb_k, pvf_ingest_create_yuv, pvf_frame_from_yuv).  Every comparison is bit for
bit against tests/yuv_ref.py -- the arithmetic is integer, there is no tolerance to choose.
  * the ring path (pinned planes -> HBM -> kernel on the copy stream) and the HBM-plane path (planar, NV12, tight and pitched) for
    4:2:0 / 4:2:2 / 4:4:4, BT.601 / BT.709, limited / full range, from 1x1 to the 4K shape of BASELINE.json configs[4];
  * a ring of depth 2 fed 9 frames without a wait in between (slot and staging reuse);
  * refused arguments raise and leave the context usable;
  * `Context.upload` / `stage` of a YuvFrame (what `shot` and `thread` use);
  * end to end: `process`, `shot` and `thread` on a .y4m file write what they write for the .npy of the same frames."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships

from tests import yuv_ref

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (1, 1), (3, 5), (20, 7), (67, 45), (640, 360), (1918, 1078), (1920, 1080), (3840, 2160)]          # (width, height)
CONSTANTS = [(0, 0, 0), (255, 255, 255), (16, 128, 128), (235, 128, 128)]


def _download(ctx, frame):
    """the RGB bytes of a DeviceFrame"""
    from pyannote_video_amd._lib import check
    p = C.c_void_p(0)
    check(ctx._l.pvf_frame_device_ptr(ctx._h, frame.handle, C.byref(p)))       # orders the context's streams behind the frame's upload
    ctx.sync()
    out = np.empty((frame.height, frame.width, 3), np.uint8)
    with open("/proc/self/maps") as maps:          # the HIP runtime this process already runs on, not a second copy of it
        loaded = sorted(set(line.split()[-1] for line in maps if "libamdhip64" in line))
    assert len(loaded) == 1, loaded
    hip = C.CDLL(loaded[0])
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, p.value, out.nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return out


def _pitched(t, pitch):
    """a [rows, cols] device tensor as a view of rows `pitch` bytes apart (the rest of each row holds 0xAA)"""
    buf = torch.full((t.shape[0], pitch), 0xAA, dtype=torch.uint8, device="cuda")
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _hbm_frames(ctx, planes, layout, matrix, full):
    """the HBM-plane path four ways: planar tight, planar pitched, NV12-style interleaved tight and pitched"""
    y, u, v = (torch.from_numpy(p).cuda() for p in planes)
    uv = torch.stack([u, v], dim=-1).contiguous()
    ch, cw = u.shape
    wide = torch.full((ch, 2 * cw + 70), 0x55, dtype=torch.uint8, device="cuda")
    wide[:, :2 * cw] = uv.reshape(ch, 2 * cw)
    uv_p = wide[:, :2 * cw].unflatten(1, (cw, 2))
    yp, up, vp = _pitched(y, y.shape[1] + 24), _pitched(u, cw + 13), _pitched(v, cw + 13)
    torch.cuda.synchronize()
    kw = dict(layout=layout, matrix=matrix, full_range=full)
    out = {"planar": ctx.frame_from_yuv_torch(y, u, v, **kw), "planar pitched": ctx.frame_from_yuv_torch(yp, up, vp, **kw),
           "nv12": ctx.frame_from_yuv_torch(y, uv, **kw), "nv12 pitched": ctx.frame_from_yuv_torch(yp, uv_p, **kw)}
    return out


def _check(ctx, ring, planes, ref, layout, matrix, full, what):
    from pyannote_video_amd.y4m import YuvFrame
    got = {"ring": ring.push(YuvFrame(*planes, layout=layout, matrix=matrix, full_range=full))}
    got.update(_hbm_frames(ctx, planes, layout, matrix, full))
    for name, frame in got.items():
        assert (frame.height, frame.width) == ref.shape[:2]
        rgb = _download(ctx, frame)
        bad = np.argwhere(rgb != ref)
        assert len(bad) == 0, "%s %s: %d bytes differ, first at (y, x, c) = %s: %d for %d" % (
            what, name, len(bad), tuple(bad[0]), rgb[tuple(bad[0])], ref[tuple(bad[0])])
        frame.release()


@pytest.mark.parametrize("w,h", SIZES)
def test_conversion_is_bit_exact(ctx, w, h):
    for layout in ("420", "422", "444"):
        for matrix in ("601", "709"):
            for full in (False, True):
                ring = ctx.ingest_ring_yuv(h, w, layout=layout, matrix=matrix, full_range=full, depth=2)
                what = "%dx%d %s %s %s" % (w, h, layout, matrix, "full" if full else "limited")
                planes = yuv_ref.noise_planes(h, w, layout, seed=w * 7 + h)
                ref = yuv_ref.to_rgb(*planes, layout=layout, matrix=matrix, full_range=full)
                if w * h >= 15:         # (the reference alone) noise over 0..255 makes every clamp fire
                    assert (ref == 0).any() and (ref == 255).any(), what
                if w * h >= 67 * 45:
                    assert all((ref[..., c] == 0).any() and (ref[..., c] == 255).any() for c in range(3)), what
                _check(ctx, ring, planes, ref, layout, matrix, full, what + " noise")
                for const in CONSTANTS:
                    planes = yuv_ref.constant_planes(h, w, layout, const)
                    ref = yuv_ref.to_rgb(*planes, layout=layout, matrix=matrix, full_range=full)
                    _check(ctx, ring, planes, ref, layout, matrix, full, what + " constant %s" % (const,))
                ring.close()
    assert ctx.pool_trim(0) == 0


def test_grey_constants_are_black_and_white(ctx):
    """(16, 128, 128) is black and (235, 128, 128) white in limited range, whatever the matrix"""
    for matrix in ("601", "709"):
        ring = ctx.ingest_ring_yuv(6, 10, matrix=matrix, depth=2)
        for yv, want in ((16, 0), (235, 255)):
            f = ring.slot()
            f[0][:], f[1][:], f[2][:] = yv, 128, 128
            assert (_download(ctx, ring.submit()) == want).all()
        ring.close()


def test_ring_of_depth_two_fed_nine_frames_without_waiting(ctx):
    from pyannote_video_amd.y4m import YuvFrame
    for w, h, layout in ((1920, 1080, "420"), (67, 45, "422")):
        ring = ctx.ingest_ring_yuv(h, w, layout=layout, depth=2)
        clip = [yuv_ref.noise_planes(h, w, layout, seed=100 + i) for i in range(9)]
        frames = [ring.push(YuvFrame(*p, layout=layout)) for p in clip]          # slots and staging buffers are reused four times over
        ring.wait()
        for i, (f, p) in enumerate(zip(frames, clip)):
            assert (_download(ctx, f) == yuv_ref.to_rgb(*p, layout=layout)).all(), (w, h, i)
            f.release()
        ring.close()


def test_refused_arguments_raise_and_the_context_goes_on(ctx):
    from pyannote_video_amd._lib import PvfError
    from pyannote_video_amd.y4m import YuvFrame
    with pytest.raises(PvfError, match="size"):
        ctx.ingest_ring_yuv(0, 16)
    with pytest.raises(PvfError, match="exceeds"):
        ctx.ingest_ring_yuv(40000, 40000)
    with pytest.raises(ValueError, match="layout"):
        ctx.ingest_ring_yuv(16, 16, layout="411")
    with pytest.raises(ValueError, match="matrix"):
        ctx.ingest_ring_yuv(16, 16, matrix="2020")
    r = C.c_uint64(0)
    assert ctx._l.pvf_ingest_create_yuv(ctx._h, 16, 16, 2, 411, 0, C.byref(r)) != 0             # the C ABI checks what Python checked above
    assert ctx._l.pvf_ingest_create_yuv(ctx._h, 16, 16, 2, 420, 8, C.byref(r)) != 0
    assert ctx._l.pvf_ingest_create_yuv(ctx._h, 16, 16, 0, 420, 0, C.byref(r)) != 0
    y = torch.zeros((16, 16), dtype=torch.uint8, device="cuda")
    c = torch.full((8, 8), 128, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    yp, cp = y.data_ptr(), c.data_ptr()
    for args, msg in (((0, 16, cp, cp, 8, 16, 16), "null"), ((yp, 16, 0, cp, 8, 16, 16), "null"), ((yp, 16, cp, 0, 8, 16, 16), "null"),
                      ((yp, 15, cp, cp, 8, 16, 16), "luma pitch"), ((yp, 16, cp, cp, 7, 16, 16), "chroma pitch"),
                      ((yp, 16, cp, cp, 8, 0, 16), "size"), ((yp, 16, cp, cp, 8, 16, -1), "size"),
                      ((yp, 16, cp, cp, 8, 40000, 40000), "exceeds")):
        with pytest.raises(PvfError, match=msg):
            ctx.frame_from_yuv_device(*args)
    with pytest.raises(PvfError, match="c_step"):
        ctx.frame_from_yuv_device(yp, 16, cp, cp, 8, 16, 16, c_step=3)
    with pytest.raises(PvfError, match="one byte apart"):
        ctx.frame_from_yuv_device(yp, 16, cp, cp + 2, 16, 16, 16, c_step=2)
    with pytest.raises(PvfError, match="chroma pitch"):
        ctx.frame_from_yuv_device(yp, 16, cp, cp + 1, 15, 16, 16, c_step=2)          # interleaved rows are twice as long
    with pytest.raises(PvfError, match="layout"):
        h = C.c_uint64(0)
        from pyannote_video_amd._lib import check
        check(ctx._l.pvf_frame_from_yuv(ctx._h, C.c_void_p(yp), 16, C.c_void_p(cp), C.c_void_p(cp), 8, 1, 16, 16, 440, 0, C.byref(h)))
    ring = ctx.ingest_ring_yuv(16, 16, depth=2)
    with pytest.raises(ValueError, match="this ring was made for"):
        ring.push(YuvFrame(*yuv_ref.noise_planes(16, 18, "420", 0)))
    # the context still converts
    f = ctx.frame_from_yuv_torch(y, c, c)
    assert (_download(ctx, f) == 0).all()
    planes = yuv_ref.noise_planes(16, 16, "420", 3)
    assert (_download(ctx, ring.push(YuvFrame(*planes))) == yuv_ref.to_rgb(*planes)).all()
    ring.close()


def test_upload_and_stage_take_yuv_frames(ctx):
    """what structure.Shot / Thread rely on: Context.upload (and stage / frame_handles over it) converts a YuvFrame on the device; other
    objects are treated as before"""
    from pyannote_video_amd.y4m import YuvFrame
    clip = [YuvFrame(*yuv_ref.noise_planes(45, 67, "420", i), matrix="709") for i in range(6)] + \
           [YuvFrame(*yuv_ref.noise_planes(36, 64, "444", 9), layout="444", full_range=True)]
    for f in clip:
        d = ctx.upload(f)
        assert (_download(ctx, d) == yuv_ref.to_rgb(f.y, f.u, f.v, f.layout, f.matrix, f.full_range)).all()
        d.release()
    hs = ctx.frame_handles(clip)
    assert len(set(hs.tolist())) == len(clip) and ctx.stage(clip[0]) is ctx.stage(clip[0])
    assert (_download(ctx, ctx.stage(clip[3])) == clip[3].rgb()).all()
    ctx.unstage_all()
    with pytest.raises(TypeError):
        ctx.upload(np.zeros((4, 4), np.uint8))


def test_verbs_on_y4m_equal_verbs_on_npy(tmp_path, ctx, model_paths):
    """The clip of test_gpu_stream.py (640x360, 36 frames, 6 shots, 3 faces, seed 17) written as 4:2:0 Y4M, and the same frames converted
    by tests/yuv_ref.py saved as .npy: `process` writes identical tracking / landmark / embedding / label files, `shot` and `thread`
    identical JSON.  The CPU oracle flow on the yuv_ref frames of this very clip finds 18 tracks and 18 labels (as on the RGB clip), so
    the seed and the face count are the stream test's own; the run has to find at least its 12 tracks and 6 labels."""
    from pyannote_video_amd import cli, synth
    v = synth.SyntheticVideo(width=640, height=360, n_frames=36, n_shots=6, faces=3, min_face=50, max_face=110, seed=17)
    clip = [yuv_ref.from_rgb(v.frame(i), "420") for i in range(v.n_frames)]
    y4m = yuv_ref.write_y4m(str(tmp_path / "clip.y4m"), clip, rate="%d:1" % int(v.frame_rate))
    assert float(int(v.frame_rate)) == v.frame_rate
    npy = str(tmp_path / "clip.npy")
    np.save(npy, np.stack([yuv_ref.to_rgb(*p) for p in clip]))
    shots = str(tmp_path / "shots.json")
    with open(shots, "w") as f:
        json.dump(v.shots(), f)
    names = ("tracking", "landmarks", "embeddings", "labels")
    out = {}
    for kind, path in (("y4m", y4m), ("npy", npy)):
        video = cli.open_video(path, v.frame_rate)
        p = {k: str(tmp_path / ("%s.%s" % (k, kind))) for k in names}
        res = cli.process(video, shots, model_paths[0], model_paths[1], p["tracking"], p["landmarks"], p["embeddings"], p["labels"], ctx=ctx)
        assert len(res["tracks"]) >= 12 and len(res["labels"]) >= 6 and res["frames"] == v.n_frames
        cli.shot(cli.open_video(path, v.frame_rate), str(tmp_path / ("shot.%s" % kind)), window=0.4, ctx=ctx)
        cli.thread(cli.open_video(path, v.frame_rate), shots, str(tmp_path / ("thread.%s" % kind)), min_match=5, ctx=ctx)
        out[kind] = {k: open(p[k], "rb").read() for k in names}
        out[kind].update(shot=open(str(tmp_path / ("shot.%s" % kind)), "rb").read(), thread=open(str(tmp_path / ("thread.%s" % kind)), "rb").read())
        # `track` + `extract` (the reader thread of `extract` stages YuvFrames too) write what `process` wrote
        t2, l2, e2 = (str(tmp_path / ("%s2.%s" % (k, kind))) for k in names[:3])
        cli.track(cli.open_video(path, v.frame_rate), shots, t2, ctx=ctx)
        cli.extract(cli.open_video(path, v.frame_rate), model_paths[0], model_paths[1], t2, l2, e2, ctx=ctx)
        assert open(t2, "rb").read() == out[kind]["tracking"] and open(l2, "rb").read() == out[kind]["landmarks"]
        assert open(e2, "rb").read() == out[kind]["embeddings"]
    for k in out["y4m"]:
        assert len(out["y4m"][k]) > 0 and out["y4m"][k] == out["npy"][k], k
    assert len(json.loads(out["y4m"]["shot"])["content"]) >= 2
    assert os.path.getsize(y4m) < 0.51 * os.path.getsize(npy)
