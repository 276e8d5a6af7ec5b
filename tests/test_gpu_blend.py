"""GPU: the `blend` verb's kernels (csrc/blend.hip) against BLEND.md as tests/blend_ref.py restates it, with np.array_equal: the lag sums
over the plane sizes, counts, firsts and contents of tests/blend_cases.py (whose reach tests/test_blend_ref.py proves on the CPU), the
rows of resident frames over frame sizes, histories, call splits and rounds, every refusal, and the two verbs in processes of their own."""
import json
import os
import subprocess
import sys

import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships
import numpy as np
import pytest

from tests import blend_cases as bc, blend_ref as br
from tests.test_gpu_faces import bare_ctx      # noqa: F401 -- fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want, what=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "%d differ, first at %s: %s against %s" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


# ---- pvf_blend_measure ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", bc.PIXELS)
def test_lag_sums_of_every_content_count_and_first(bare_ctx, P):
    for content in bc.CONTENTS:
        y = bc.planes(content, bc.N_MOST, P)
        want = br.rows_of(y)                                        # once: a row depends on the planes in front of it only
        _same(bare_ctx.blend_measure(y), want, (content, P))
        if content == "jump16":
            assert int(want[32, 11]) == 510 * P                     # the largest R there is
        if content != "random":
            continue
        _same(bare_ctx.blend_measure(y), want, "the same call twice")
        for N in bc.COUNTS:
            for first in bc.firsts(N):
                _same(bare_ctx.blend_measure(y[:N], first), want[first:N], (P, N, first))


def test_a_round_boundary_of_planes(bare_ctx, monkeypatch):
    y = bc.planes("random", 70, 257)
    want = br.rows_of(y)
    for round_ in ("1", "7", "33"):
        monkeypatch.setenv("PVF_THUMB_ROUND", round_)
        _same(bare_ctx.blend_measure(y), want, round_)
        _same(bare_ctx.blend_measure(y, 31), want[31:], round_)


# ---- pvf_frame_blend ------------------------------------------------------------------------------------------------------------------
def rows_after(hist, luma, tw, th):
    return br.rows_of(np.concatenate([hist, luma]), first=len(hist), size_word=tw | th << 16)


@pytest.mark.parametrize("w,h,tw,th", bc.FRAME_SIZES)
def test_rows_of_resident_frames(bare_ctx, monkeypatch, w, h, tw, th):
    n = 6 if w * h > 100000 else 40
    P = tw * th
    frames = bc.frames_of(w, h, n)
    luma = np.stack([br.plane(f, tw, th) for f in frames]).reshape(n, P)      # the thumbnail rule and the luma, once
    none = np.zeros((0, P), np.uint8)
    want = rows_after(none, luma, tw, th)
    devs = [bare_ctx.upload(f) for f in frames]
    rows, got_luma = bare_ctx.frame_blend(devs, tw, th)
    _same(got_luma, luma, "luma")
    _same(rows, want, "one call")
    assert (rows[:, 0] == P).all() and (rows[:, 14] == (tw | th << 16)).all() and not rows[:, 12:14].any() and not rows[:, 15].any()
    rows, no_luma = bare_ctx.frame_blend(devs, tw, th, want_luma=False)         # without luma_out
    assert no_luma is None
    _same(rows, want, "no luma_out")
    rng = np.random.default_rng(P)
    for nh in bc.HISTORIES:                                         # any planes may stand in front
        hist = rng.integers(0, 256, (nh, P), dtype=np.uint8)
        rows, _ = bare_ctx.frame_blend(devs[:5], tw, th, hist=hist)
        _same(rows, rows_after(hist, luma[:5], tw, th), ("nh", nh))
    for cuts in ((3, 4, n), (1, 2, 3, n), (n - 1, n)):              # several calls with carried history are one call
        hist, parts, a = none, [], 0
        for b in cuts:
            r, l = bare_ctx.frame_blend(devs[a:b], tw, th, hist=hist)
            hist = np.concatenate([hist, l])[-32:]
            parts.append(r)
            a = b
        _same(np.concatenate(parts), want, cuts)
    for round_ in ("1", "4"):                                       # rounds inside one call: nothing depends on them
        monkeypatch.setenv("PVF_THUMB_ROUND", round_)
        hist = rng.integers(0, 256, (32, P), dtype=np.uint8)
        rows, l = bare_ctx.frame_blend(devs, tw, th, hist=hist)
        _same(rows, rows_after(hist, luma, tw, th), ("round", round_))
        _same(l, luma, ("round luma", round_))
    monkeypatch.delenv("PVF_THUMB_ROUND")
    for d in devs:
        d.release()
    assert bare_ctx.frame_blend([], tw, th)[0].shape == (0, 16)


def test_refusals(bare_ctx):
    from pyannote_video_amd import _lib
    c, l, P_ = bare_ctx, bare_ctx._l, _lib.ptr
    f = bc.frames_of(12, 7, 1)[0]
    a, other, gone = c.upload(f), c.upload(bc.frames_of(13, 7, 1)[0]), c.upload(f)
    gone_handle = gone.handle
    gone.release()
    hs = np.array([a.handle, a.handle], np.uint64)
    hist = np.zeros((2, 12), np.uint8)
    ref, _ = br.frame_rows([f, f], 4, 3, hist=hist)
    rows = np.full((2, 16), 0xA5A5A5A5, np.uint32)

    def call(frames=hs, n=2, tw=4, th=3, h=hist, nh=2, r=rows, luma=None):
        return l.pvf_frame_blend(c._h, P_(frames), n, tw, th, P_(h), nh, P_(r), P_(luma))
    big = 65536 + 1
    for kw, message in ((dict(n=-1), "n outside"), (dict(n=big), "n outside"), (dict(nh=-1), "nh outside"), (dict(nh=33), "nh outside"),
                        (dict(tw=0), "tw or th outside"), (dict(th=0), "tw or th outside"), (dict(th=-3), "tw or th outside"),
                        (dict(tw=1025), "tw or th outside"), (dict(tw=129, th=128, nh=0), "PVF_BLEND_MAX_PIXELS"),
                        (dict(frames=None), "null frames or rows"), (dict(r=None), "null frames or rows"), (dict(h=None), "null history"),
                        (dict(frames=np.array([a.handle, 987654321], np.uint64)), "unknown frame handle"),
                        (dict(frames=np.array([gone_handle, a.handle], np.uint64)), "unknown frame handle"),
                        (dict(frames=np.array([a.handle, other.handle], np.uint64)), "frames of different sizes")):
        assert call(**kw) != 0, message
        assert message in l.pvf_last_error().decode(), (message, l.pvf_last_error().decode())
        assert (rows == 0xA5A5A5A5).all()                           # refused before any work
        assert call() == 0 and np.array_equal(rows, ref)            # the context goes on
        rows[:] = 0xA5A5A5A5
    assert l.pvf_frame_blend(c._h, None, 0, 4, 3, None, 0, None, None) == 0
    a.release(); other.release()
    with pytest.raises(ValueError, match="history"):
        c.frame_blend([], 4, 3, hist=np.zeros((2, 11), np.uint8))
    # planes
    y = bc.planes("random", 9, 12)
    want = br.rows_of(y, 2)
    out = np.full((7, 16), 0xA5A5A5A5, np.uint32)

    def measure(luma=y, N=9, P=12, first=2, r=out):
        return l.pvf_blend_measure(c._h, P_(luma), N, P, first, P_(r))
    for kw, message in ((dict(N=-1), "N outside"), (dict(N=(1 << 24) + 1), "N outside"), (dict(first=-1), "first outside"),
                        (dict(first=10), "first outside"), (dict(P=0), "PVF_BLEND_MAX_PIXELS"), (dict(P=-5), "PVF_BLEND_MAX_PIXELS"),
                        (dict(P=16385), "PVF_BLEND_MAX_PIXELS"), (dict(luma=None), "null planes"), (dict(r=None), "null rows")):
        assert measure(**kw) != 0, message
        assert message in l.pvf_last_error().decode(), (message, l.pvf_last_error().decode())
        assert (out == 0xA5A5A5A5).all()
        assert measure() == 0 and np.array_equal(out, want)
        out[:] = 0xA5A5A5A5
    assert l.pvf_blend_measure(c._h, None, 0, 12, 0, None) == 0 and measure(first=9, r=None) == 0      # nothing to measure is legal
    assert c.blend_measure(y, 9).shape == (0, 16)
    with pytest.raises(ValueError, match="uint8"):
        c.blend_measure(y.reshape(-1))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_the_verbs_in_processes_of_their_own(tmp_path):
    from tests import yuv_ref
    clip = bc.planted_clip()
    fps, tw, th = bc.CLIP_FPS, bc.CLIP_WIDTH, br.tile_size(bc.CLIP_WIDTH, bc.CLIP_W, bc.CLIP_H)[1]
    video, rows_a, rows_b, out_a, out_b, y4m = (str(tmp_path / n) for n in ("clip.npy", "a.npy", "b.npy", "a.json", "b.json", "clip.y4m"))
    np.save(video, np.stack(clip.frames))
    planes = [yuv_ref.from_rgb(f, "420") for f in clip.frames]
    yuv_ref.write_y4m(y4m, planes, rate="25:1")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pyannote-video_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for args, stdin in ((["blend", "--width", str(tw), "--batch", "7", video, rows_a], None), (["transition", rows_a, out_a], None),
                        (["blend", "--width", str(tw), "-", rows_b], y4m), (["transition", rows_b, out_b], None)):
        with open(stdin or os.devnull, "rb") as fi:
            run = subprocess.run([sys.executable, "-m", "pyannote_video_amd", "--fps", str(fps)] + args, stdin=fi, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, env=env, timeout=600)
        assert run.returncode == 0, (args, run.stderr.decode()[-2000:])
    want = br.video_rows(clip.frames, tw, th, fps)
    _same(np.load(rows_a), want)
    found = json.load(open(out_a))
    assert found == br.report(want) and [f["kind"] for f in found] == ["dissolve", "fade-out", "blank", "fade-in"]
    want = br.video_rows([yuv_ref.to_rgb(*p) for p in planes], tw, th, fps)
    _same(np.load(rows_b), want)
    assert json.load(open(out_b)) == br.report(want)
