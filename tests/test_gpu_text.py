"""GPU: the `text` verb's kernels (csrc/text.hip) against CAPTION.md as tests/text_ref.py restates it, with np.array_equal on rows and
counts: every geometry, content and parameter triple of tests/text_cases.py (whose reach tests/test_text_ref.py proves on the CPU), with
and without a predecessor and counts, repeated handles and calls, call splits and rounds, 1080p and 2160p, every refusal, and the two
verbs in processes of their own."""
import json
import os
import subprocess
import sys

import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships
import numpy as np
import pytest

from tests import text_cases as tc, text_ref as tr
from tests.test_gpu_faces import bare_ctx      # noqa: F401 -- fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want, what=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "%d differ, first at %s: %s against %s" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def uploaded(ctx, frames):
    """the frames on the device; a frame that appears more than once in the list is uploaded once"""
    known = {}
    for f in frames:
        if id(f) not in known:
            known[id(f)] = ctx.upload(f)
    return [known[id(f)] for f in frames], list(known.values())


@pytest.mark.parametrize("w,h", tc.GEOMETRIES)
def test_every_content_and_parameter_triple(bare_ctx, w, h):
    for content in tc.CONTENTS:
        devs = None
        for params in tc.PARAMS:
            if devs is None or content in ("edge_eq", "still_eq", "on_eq"):         # (the other contents do not depend on the parameters)
                frames = tc.frames_of(content, w, h, params)
                devs, owned = uploaded(bare_ctx, frames)
            edge, still, on = params
            want_rows, want_counts = tr.rows_of(frames, None, edge, still, on)      # once: a row depends on the frame before it only
            what = (w, h, content, params)
            rows, counts = bare_ctx.frame_text(devs, edge=edge, still=still, on=on, want_counts=True)
            _same(counts, want_counts, what)
            _same(rows, want_rows, what)
            rows, none = bare_ctx.frame_text(devs[1:], prev=devs[0], edge=edge, still=still, on=on)         # with a predecessor, without counts
            assert none is None
            _same(rows, want_rows[1:], what + ("prev",))


def test_repeated_handles_calls_splits_and_rounds(bare_ctx, monkeypatch):
    w, h = 300, 37
    frames = tc.frames_of("noise", w, h, n=9)
    frames = frames[:4] + [frames[3], frames[1]] + frames[4:]                       # the same frame twice in a row, and once more later
    devs, owned = uploaded(bare_ctx, frames)
    assert len(owned) == 9 and len(devs) == 11
    want_rows, want_counts = tr.rows_of(frames)
    assert int(want_rows[4, 4]) == 0 and int(want_rows[4, 3]) == int(want_rows[4, 2]) > 0              # M = 0 and S = E after the repeat
    for k in range(2):                                                               # the same call twice
        rows, counts = bare_ctx.frame_text(devs, want_counts=True)
        _same(rows, want_rows, k)
        _same(counts, want_counts, k)
    for cuts in ((1, 2, 11), (5, 11), (3, 4, 10, 11)):                              # several calls with prev carried are one call
        parts, a, prev = [], 0, None
        for b in cuts:
            parts.append(bare_ctx.frame_text(devs[a:b], prev=prev, want_counts=True))
            a, prev = b, devs[b - 1]
        _same(np.concatenate([p[0] for p in parts]), want_rows, cuts)
        _same(np.concatenate([p[1] for p in parts]), want_counts, cuts)
    for round_ in ("1", "4"):                                                        # rounds inside one call: nothing depends on them
        monkeypatch.setenv("PVF_TEXT_ROUND", round_)
        rows, counts = bare_ctx.frame_text(devs, want_counts=True)
        _same(rows, want_rows, ("round", round_))
        _same(counts, want_counts, ("round", round_))
        rows, _ = bare_ctx.frame_text(devs[2:], prev=devs[1])
        _same(rows, want_rows[2:], ("round with prev", round_))
    monkeypatch.delenv("PVF_TEXT_ROUND")
    rows, none = bare_ctx.frame_text([])
    assert rows.shape == (0, 8) and none is None


@pytest.mark.parametrize("w,h,n", ((1920, 1080, 3), (3840, 2160, 2)))
def test_full_size_frames_after_unrelated_work(bare_ctx, w, h, n):
    rng = np.random.default_rng(w)
    base = np.kron(rng.integers(0, 256, (h // 8, w // 8, 3)), np.ones((8, 8, 1), np.int64))
    frames = [np.clip(np.roll(base, 3 * t, axis=1) + rng.integers(-6, 7, base.shape), 0, 255).astype(np.uint8) for t in range(n)]
    frames[-1][h // 2:] = frames[-2][h // 2:]                                        # the lower half stands still: strokes persist there
    devs, owned = uploaded(bare_ctx, frames)
    bare_ctx.frame_blend(devs, 64, 36)                                               # unrelated work in the scratch this call uses
    want_rows, want_counts = tr.rows_of(frames)
    assert int(want_rows[-1, 5]) > 100                                               # bits are set
    rows, counts = bare_ctx.frame_text(devs, want_counts=True)
    _same(counts, want_counts)
    _same(rows, want_rows)
    assert rows.shape[1] == (280 if w == 1920 else 8 + 135 * 8)


def test_refusals(bare_ctx):
    from pyannote_video_amd import _lib
    c, l, P_ = bare_ctx, bare_ctx._l, _lib.ptr
    f = tc.frames_of("noise", 20, 7)[0]
    a, other, gone = c.upload(f), c.upload(tc.frames_of("noise", 21, 7)[0]), c.upload(f)
    gone_handle = gone.handle
    gone.release()
    hs = np.array([a.handle, a.handle], np.uint64)
    ref, _ = tr.rows_of([f, f], f)
    rows = np.full((2, 9), 0xA5A5A5A5, np.uint32)

    def call(frames=hs, n=2, prev=a.handle, edge=48, still=8, on=24, r=rows, counts=None):
        return l.pvf_frame_text(c._h, P_(frames), n, prev, edge, still, on, P_(r), P_(counts))
    for kw, message in ((dict(n=-1), "n outside"), (dict(n=4097), "n outside"), (dict(edge=0), "edge outside"), (dict(edge=256), "edge outside"),
                        (dict(still=-1), "still outside"), (dict(still=255), "still outside"), (dict(on=0), "on outside"), (dict(on=257), "on outside"),
                        (dict(frames=None), "null frames or rows"), (dict(r=None), "null frames or rows"),
                        (dict(frames=np.array([a.handle, 987654321], np.uint64)), "unknown frame handle"),
                        (dict(frames=np.array([gone_handle, a.handle], np.uint64)), "unknown frame handle"),
                        (dict(prev=gone_handle), "unknown frame handle"), (dict(prev=987654321), "unknown frame handle"),
                        (dict(frames=np.array([a.handle, other.handle], np.uint64)), "frames of different sizes"),
                        (dict(prev=other.handle), "frames of different sizes")):
        assert call(**kw) != 0, message
        assert message in l.pvf_last_error().decode(), (message, l.pvf_last_error().decode())
        assert (rows == 0xA5A5A5A5).all()                           # refused before any work
        assert call() == 0 and np.array_equal(rows, ref)            # the context goes on
        rows[:] = 0xA5A5A5A5
    assert l.pvf_frame_text(c._h, None, 0, 0, 48, 8, 24, None, None) == 0
    a.release(); other.release()
    wide = torch.zeros((1, 8193, 3), dtype=torch.uint8, device="cuda")               # a side above the cap
    dev = c.wrap_torch(wide)
    assert l.pvf_frame_text(c._h, P_(np.array([dev.handle], np.uint64)), 1, 0, 48, 8, 24, P_(np.zeros(8 + 17, np.uint32)), None) != 0
    assert "PVF_TEXT_MAX_SIDE" in l.pvf_last_error().decode()
    dev.release()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_the_verbs_in_processes_of_their_own(tmp_path):
    from tests import yuv_ref
    frames = tc.planted_clip()
    fps = tc.CLIP_FPS
    video, rows_a, rows_b, rows_c, rows_d, out_a, y4m = (str(tmp_path / n) for n in ("clip.npy", "a.npy", "b.npy", "c.npy", "d.npy", "a.json", "clip.y4m"))
    np.save(video, np.stack(frames))
    planes = [yuv_ref.from_rgb(f, "420") for f in frames]
    yuv_ref.write_y4m(y4m, planes, rate="25:1")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pyannote-video_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for args, stdin in ((["text", "--batch", "7", video, rows_a], None), (["text", video, rows_b], None), (["caption", rows_a, out_a], None),
                        (["text", "-", rows_c], y4m), (["text", y4m, rows_d], None)):
        with open(stdin or os.devnull, "rb") as fi:
            run = subprocess.run([sys.executable, "-m", "pyannote_video_amd", "--fps", str(fps)] + args, stdin=fi, stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, env=env, timeout=600)
        assert run.returncode == 0, (args, run.stderr.decode()[-2000:])
    want = tr.video_rows(frames, fps)
    _same(np.load(rows_a), want)
    assert open(rows_a, "rb").read() == open(rows_b, "rb").read()                    # --batch 7 and the default batch: the same bytes
    found = json.load(open(out_a))
    assert found == tr.captions(want) and len(found) == 1
    assert (found[0]["left"], found[0]["top"], found[0]["right"], found[0]["bottom"]) == tc.STRAP
    assert open(rows_c, "rb").read() == open(rows_d, "rb").read()                    # the stream on stdin and the same file by its path
    _same(np.load(rows_c), tr.video_rows([yuv_ref.to_rgb(*p) for p in planes], fps))         # the stream equals the .npy route on its own pixels
