"""GPU: the `talk` verb's kernels (csrc/talk.hip) bit for bit against TALK.md as tests/talk_ref.py restates it: the eight integers of
chips under every pattern of predecessors, at every shift of the search, on extreme and constant contents, across a round of 4096 and
at every alignment of the host buffer; of faces whose chips are made on the device; every refusal of the C ABI; and the verb end to end
in a process of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import talk_ref as tr
from tests.test_gpu_chip_edges import landmarks
from tests.test_gpu_faces import bare_ctx, dlib_ctx      # noqa: F401 -- fixtures

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tr.named_cases()
_CACHE = {}


def want(name):
    if name not in _CACHE:
        _CACHE[name] = tr.motion(*CASES[name])
    return _CACHE[name]


def _same(got, ref, names=None):
    assert got.shape == ref.shape and got.dtype == np.int32
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert len(bad) == 0, [(int(i), got[i].tolist(), ref[i].tolist()) for i in bad[:5]]


# ---- chip_motion -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_chip_motion_equals_the_restatement(bare_ctx, name):
    chips, prev = CASES[name]
    got = bare_ctx.chip_motion(np.stack(chips), prev)
    _same(got, want(name))
    if name == "shifts":                                            # every shift of the search, found where it is
        assert got[1:, 1].tolist() == [0] * 49 and got[1:, 2].tolist() == list(range(49)) and got[1:, 5].tolist() == list(range(49))
    if name == "extremes":
        assert got[1].tolist() == [652800, 652800, 24, 652800, 652800, 24, 652800, 0] and got[4, :3].tolist() == [652800, 0, 0]
    if name == "constant":                                          # ties everywhere: the zero shift
        assert got[1, :6].tolist() == [0, 0, 24, 0, 0, 24] and got[2, :6].tolist() == [7680, 7680, 24, 7680, 7680, 24]
    if name == "moved":
        assert got[1, 1:3].tolist() == [0, 11] and got[1, 4:6].tolist() == [0, 11] and got[1, 0] > 0
    if name == "none_linked":
        assert (got[:, :6] == -1).all() and (got[:, 6] > 0).all()


def test_chip_motion_one_call_per_pair_gives_what_the_batch_gives(bare_ctx):
    chips, prev = CASES["shared"]
    for i, p in enumerate(prev):
        if p >= 0:
            assert np.array_equal(bare_ctx.chip_motion(np.stack([chips[p], chips[i]]), [-1, 0])[1], want("shared")[i])
    assert bare_ctx.chip_motion(np.zeros((0, 150, 150, 3), np.uint8), []).shape == (0, 8)


def test_chip_motion_across_the_round_of_4096(bare_ctx):
    """4100 chips go through in two rounds; links from the second round into the first and across the boundary"""
    n = 4100
    distinct = CASES["chain"][0] + [tr.smooth_chip(), tr.smooth_chip(-1, 2)]
    chips = [distinct[(i * 5 + 3) % len(distinct)] for i in range(n)]
    prev = np.full(n, -1, np.int32)
    for i, p in ((4096, 4095), (4097, 3), (4095, 4094), (4098, 4096), (4099, 0), (5, 4), (4094, 17), (2000, 1999), (4093, 17)):
        prev[i] = p
    ref = tr.motion(chips, prev)
    assert (ref[[4096, 4097], 1] > 0).all() and len(set(ref[prev >= 0, 1].tolist())) >= 5
    got = bare_ctx.chip_motion(np.stack(chips), prev)
    _same(got, ref)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_chip_motion_host_buffer_alignment(bare_ctx, offset):
    chips, prev = CASES["chain"]
    flat = np.stack(chips).reshape(-1)
    buf = np.zeros(len(flat) + 64, np.uint8)
    base = (-buf.ctypes.data) % 16 + offset                         # the chips start `offset` bytes behind a multiple of 16
    buf[base:base + len(flat)] = flat
    view = buf[base:base + len(flat)].reshape(-1, 150, 150, 3)
    assert view.ctypes.data % 16 == offset
    _same(bare_ctx.chip_motion(view, prev), want("chain"))


# ---- face_motion -------------------------------------------------------------------------------------------------------------------
def _faces():
    from pyannote_video_amd import models
    mean = np.stack([np.asarray(models.DLIB_MEAN_FACE_X), np.asarray(models.DLIB_MEAN_FACE_Y)], 1)
    # (frame, geometry): two faces a frame, the second partly off the frame; they move and turn a little from frame to frame
    geo = [(0, (320, 180, 80, 0)), (0, (12, 180, 80, 0)), (1, (322, 181, 82, 2)), (1, (10, 182, 80, 0)), (2, (325, 181, 84, 3)),
           (2, (9, 183, 78, -2)), (3, (640 - 56, 180, 80, 0)), (3, (300, 170, 120, 25))]
    return [f for f, _ in geo], np.stack([landmarks(mean, *g) for _, g in geo]), [-1, -1, 0, 1, 2, 3, 4, 4]


def test_face_motion_equals_chip_motion_of_the_chips(ctx, bare_ctx, dlib_ctx, small_video):
    fi, pts, prev = _faces()
    frames = [small_video.frame(i) for i in fi]
    chips = dlib_ctx.face_chips(frames, pts)
    ref = tr.motion(list(chips), prev)
    assert ref[1, 7] > 0 and ref[3, 7] > 0 and ref[0, 7] < ref[1, 7]              # the face on the left edge is partly black
    assert (ref[2:, 1] > 0).all() and len({tuple(r) for r in ref.tolist()}) == len(ref)
    _same(dlib_ctx.chip_motion(chips, prev), ref)
    for c in (bare_ctx, dlib_ctx, ctx):                             # without an embedder; with dlib's shape; with the suite's synthetic one
        _same(c.face_motion(frames, pts, prev), ref)
    one = bare_ctx.face_motion([frames[1], frames[3]], pts[[1, 3]], [-1, 0])        # one pair per call == the batch
    assert np.array_equal(one[1], ref[3])
    assert bare_ctx.face_motion([], np.zeros((0, 68, 2), np.int32), []).shape == (0, 8)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(bare_ctx, small_video):
    """host-side checks, each with its message; after each the context still answers a good call"""
    from pyannote_video_amd import _lib
    c, l, P = bare_ctx, bare_ctx._l, _lib.ptr
    chips = np.ascontiguousarray(np.stack(CASES["two"][0]))
    good = np.array([-1, 0], np.int32)
    out = np.zeros((2, 8), np.int32)
    f = c.upload(small_video.frame(0))
    hs = np.array([f.handle, f.handle], np.uint64)
    bad_handles = np.array([f.handle, 987654321], np.uint64)
    _, pts, _ = _faces()
    pts = np.ascontiguousarray(pts[:2])

    def prevs(*v):
        return np.array(v, np.int32)
    for call, message in ((lambda: l.pvf_chip_motion(c._h, P(chips), -1, P(good), P(out)), "PVF_MOTION_MAX_FACES"),
                          (lambda: l.pvf_chip_motion(c._h, P(chips), 32769, P(good), P(out)), "PVF_MOTION_MAX_FACES"),
                          (lambda: l.pvf_chip_motion(c._h, None, 2, P(good), P(out)), "null chips"),
                          (lambda: l.pvf_chip_motion(c._h, P(chips), 2, None, P(out)), "null predecessor"),
                          (lambda: l.pvf_chip_motion(c._h, P(chips), 2, P(good), None), "null output"),
                          (lambda: l.pvf_chip_motion(c._h, P(chips), 2, P(prevs(-2, 0)), P(out)), "below -1"),
                          (lambda: l.pvf_chip_motion(c._h, P(chips), 2, P(prevs(-1, 1)), P(out)), "prev[i] < i"),
                          (lambda: l.pvf_chip_motion(c._h, P(chips), 2, P(prevs(0, 0)), P(out)), "prev[i] < i"),
                          (lambda: l.pvf_chip_motion(c._h, P(chips), 2, P(prevs(-1, 2 ** 31 - 1)), P(out)), "prev[i] < i"),
                          (lambda: l.pvf_face_motion(c._h, P(hs), P(pts), -1, P(good), P(out)), "PVF_MOTION_MAX_FACES"),
                          (lambda: l.pvf_face_motion(c._h, P(hs), P(pts), 32769, P(good), P(out)), "PVF_MOTION_MAX_FACES"),
                          (lambda: l.pvf_face_motion(c._h, None, P(pts), 2, P(good), P(out)), "null chips, frames or landmarks"),
                          (lambda: l.pvf_face_motion(c._h, P(hs), None, 2, P(good), P(out)), "null chips, frames or landmarks"),
                          (lambda: l.pvf_face_motion(c._h, P(hs), P(pts), 2, None, P(out)), "null predecessor"),
                          (lambda: l.pvf_face_motion(c._h, P(hs), P(pts), 2, P(good), None), "null output"),
                          (lambda: l.pvf_face_motion(c._h, P(hs), P(pts), 2, P(prevs(-1, -7)), P(out)), "below -1"),
                          (lambda: l.pvf_face_motion(c._h, P(hs), P(pts), 2, P(prevs(-1, 1)), P(out)), "prev[i] < i"),
                          (lambda: l.pvf_face_motion(c._h, P(bad_handles), P(pts), 2, P(good), P(out)), "unknown frame handle")):
        assert call() != 0, message
        assert message in l.pvf_last_error().decode(), (message, l.pvf_last_error().decode())
        assert l.pvf_chip_motion(c._h, P(chips), 2, P(good), P(out)) == 0 and np.array_equal(out, want("two"))       # the context goes on
        out[:] = 0
    assert l.pvf_chip_motion(c._h, None, 0, None, None) == 0 and l.pvf_face_motion(c._h, None, None, 0, None, None) == 0      # n = 0 does nothing
    with pytest.raises(ValueError, match="one predecessor per chip"):
        c.chip_motion(chips, [-1])
    with pytest.raises(_lib.PvfError, match="prev\\[i\\] < i"):
        c.chip_motion(chips, [1, 0])
    assert l.pvf_face_motion(c._h, P(hs), P(pts), 2, P(good), P(out)) == 0 and (out[0, :6] == -1).all() and (out[1, :6] >= 0).all()
    f.release()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_talk_verb_in_a_process_of_its_own(tmp_path, bare_ctx):
    from pyannote_video_amd import cli, faces, formats, models, pipeline, talk
    spec, fps = "synthetic:640x360x9:2:3:7", 25.0
    video = cli.open_video(spec, fps)
    mean = np.stack([np.asarray(models.DLIB_MEAN_FACE_X), np.asarray(models.DLIB_MEAN_FACE_Y)], 1)
    # three hand-made tracks: one in the middle that drifts, one on the left edge (partly off the frame), one that starts on frame 3
    geo = {0: lambda i: (300 + 2 * i, 170 + i, 90 + i, i), 1: lambda i: (14 - i, 200, 80, 0), 2: lambda i: (520, 120 + 3 * i, 70, -2 * i)}
    first = {0: 0, 1: 0, 2: 3}
    box = lambda g: ((g[0] - g[2] / 2) / 640.0, (g[1] - g[2] / 2) / 360.0, (g[0] + g[2] / 2) / 640.0, (g[1] + g[2] / 2) / 360.0)
    tp, lp, op, sp = (str(tmp_path / n) for n in ("track.txt", "landmarks.txt", "talk.txt", "segments.txt"))
    formats.write_tracks(tp, [[(i / fps, box(geo[k](i)), "forward") for i in range(first[k], 9)] for k in (0, 1, 2)])
    rows = formats.read_tracks(tp)
    times = [i / fps for i in range(9)]
    with open(lp, "wb") as f:
        for fi, T, g in pipeline.faces_per_frame(rows, times, 640, 360):
            for ident, _ in g:
                f.write(formats.landmark_rows([T], [ident], landmarks(mean, *geo[ident](fi))[None], 640, 360))
    # the plain loop: every face in one call, then talk.py
    F = faces.landmark_faces(rows, formats.read_landmarks(lp), times, 640, 360)
    assert len(F) >= 18 and all(np.array_equal(f[4], landmarks(mean, *geo[f[1]](f[2]))) for f in F)
    prev = talk.link([(f[2], f[1]) for f in F])
    assert sum(p >= 0 for p in prev) == len(F) - 3
    got = bare_ctx.face_motion([video.frame(f[2]) for f in F], np.stack([f[4] for f in F]), prev)
    params = dict(window=0.2, on=0.5, off=0.25, min_duration=0.04, max_pause=0.1, max_dark=0.5)
    per, segs = talk.analyse([(f[0], f[1], f[4]) for f in F], got, [p >= 0 for p in prev], **params)
    lines = "".join(talk.face_line(f[0], f[1], got[i], *per[i]) for i, f in enumerate(F))
    assert any(p[1] > 0 for p in per) and any(int(r[7]) > 0 for r in got)           # something moves; the face on the edge is partly black
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pyannote-video_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "pyannote_video_amd", "--fps", str(fps), "talk", "--window", "0.2", "--on", "0.5", "--off", "0.25",
                          "--min-duration", "0.04", "--max-pause", "0.1", "--max-dark", "0.5", "--segments", sp, spec, tp, lp, op],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    assert open(op).read() == lines
    assert open(sp).read() == "".join(talk.segment_line(*s) for s in segs)
    # in this process with batches of three faces: the carried frame links across calls
    cli.talk(video, tp, lp, op, segments=sp, ctx=bare_ctx, batch=3, **params)
    assert open(op).read() == lines
