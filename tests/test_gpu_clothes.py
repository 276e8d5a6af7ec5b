"""GPU: pvf_frame_hist (csrc/clothes.hip) against CLOTHES.md as tests/clothes_ref.py restates it, with np.array_equal: every frame size,
content and window of tests/clothes_cases.py (whose reach tests/test_clothes_ref.py proves on the CPU), one window a call and batched,
at every band count, at device addresses off alignment, with frames of mixed sizes, every grouping, rounds, the result in host and in
device memory, call splits, 1080p and 2160p, every refusal, and the verbs in processes of their own."""
import json
import os
import subprocess
import sys

import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships
import numpy as np
import pytest

from tests import clothes_cases as cc, clothes_ref as cr
from tests.test_gpu_faces import bare_ctx      # noqa: F401 -- fixture

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want, what=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, "%d differ, first at %s: %s against %s" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def shifted(ctx, frame, k):
    """the frame at a device address k bytes behind a 256-byte boundary, through pvf_frame_wrap_device: (device frame, the tensor kept)"""
    h, w = frame.shape[:2]
    buf = torch.zeros(3 * w * h + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[k:k + 3 * w * h] = torch.from_numpy(np.ascontiguousarray(frame).reshape(-1)).cuda()
    return ctx.wrap_device(buf.data_ptr() + k, h, w, keep=buf)


@pytest.mark.parametrize("w,h", cc.GEOMETRIES)
def test_the_whole_table_one_window_a_call_and_batched(bare_ctx, w, h):
    wins = cc.windows_for(w, h)
    n = len(wins)
    for content in cc.CONTENTS:
        f = cc.frame_of(content, w, h)
        known = {}
        want = dict((B, cr.hist_of([f] * n, wins, np.arange(n), n, B, known=known)) for B in cc.BANDS)
        assert int(want[1].sum()) > 0
        dev = bare_ctx.upload(f)
        for B in cc.BANDS:                                                           # batched: a group per window
            _same(bare_ctx.frame_hist([dev] * n, wins, np.arange(n), n, bands=B), want[B], (w, h, content, B))
        for i in range(n):                                                           # one window a call, the band counts in turn
            B = cc.BANDS[i % 4]
            _same(bare_ctx.frame_hist([dev], wins[i:i + 1], [0], 1, bands=B), want[B][i:i + 1], (w, h, content, "window", i, wins[i].tolist(), B))
        dev.release()


@pytest.mark.parametrize("k", (1, 2, 3))
def test_frames_at_device_addresses_off_alignment(bare_ctx, k):
    for w, h in cc.GEOMETRIES:
        wins = cc.windows_for(w, h)
        n = len(wins)
        f = cc.frame_of("noise" if (w + h) % 2 else "every", w, h)
        dev = shifted(bare_ctx, f, k)
        B = cc.BANDS[(w + h + k) % 4]
        _same(bare_ctx.frame_hist([dev] * n, wins, np.arange(n), n, bands=B), cr.hist_of([f] * n, wins, np.arange(n), n, B), (w, h, k, B))
        dev.release()


@pytest.fixture(scope="module")
def mixed(bare_ctx):
    """windows of frames of many sizes for one call: (device frames per window, host frames per window, windows, the frames to release)"""
    frames, devs, wins = [], [], []
    for w, h in cc.GEOMETRIES[1::3] + [(300, 40)]:
        f = cc.frame_of("noise", w, h)
        d = bare_ctx.upload(f)
        for q in cc.windows_for(w, h)[::2]:
            frames.append(f); devs.append(d); wins.append(q)
    yield devs, frames, np.array(wins, np.int32)
    for d in set(devs):
        d.release()


def test_mixed_sizes_groupings_rounds_splits_and_where_the_result_lies(bare_ctx, mixed, monkeypatch):
    devs, frames, wins = mixed
    n = len(wins)
    assert n > 300 and len(set(f.shape for f in frames)) == 12
    bare_ctx.frame_text(devs[-2:])                                                   # other library work in the scratch this call uses
    known = {}
    for name, group, G in cc.groupings(n):
        want = cr.hist_of(frames, wins, group, G, 2, known=known)
        _same(bare_ctx.frame_hist(devs, wins, group, G, bands=2), want, name)
    # the same window twice, in one group and in two
    group, G = np.arange(2 * n, dtype=np.int32) % n, n
    want = cr.hist_of(frames, wins, np.arange(n), n, 3, known=known)
    _same(bare_ctx.frame_hist(devs + devs, np.concatenate([wins, wins]), group, G, bands=3), 2 * want, "twice")
    # the windows split over two calls add up to one call's result
    group = np.arange(n, dtype=np.int32) % 5
    whole = bare_ctx.frame_hist(devs, wins, group, 5, bands=4)
    _same(whole, cr.hist_of(frames, wins, group, 5, 4, known=known), "whole")
    for cut in (1, n // 2, n - 1):
        _same(bare_ctx.frame_hist(devs[:cut], wins[:cut], group[:cut], 5, bands=4) + bare_ctx.frame_hist(devs[cut:], wins[cut:], group[cut:], 5, bands=4), whole, cut)
    # rounds inside one call: nothing depends on them
    for round_ in ("1", "7", "100000"):
        monkeypatch.setenv("PVF_HIST_ROUND", round_)
        _same(bare_ctx.frame_hist(devs, wins, group, 5, bands=4), whole, ("round", round_))
    monkeypatch.delenv("PVF_HIST_ROUND")
    # the result in device memory, over what the buffer held before
    out = torch.full((5, 4, 256), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert bare_ctx.frame_hist(devs, wins, group, 5, bands=4, out_ptr=out.data_ptr()) is None
    _same(out.cpu().numpy().view(np.uint32), whole, "on the device")
    # no windows: zeros
    _same(bare_ctx.frame_hist([], np.zeros((0, 4), np.int32), [], 3, bands=2), np.zeros((3, 2, 256), np.uint32))


def test_the_cap_of_rows_and_five_thousand_one_pixel_windows(bare_ctx):
    f = cc.frame_of("every", 85, 17)
    dev = bare_ctx.upload(f)
    G, B = 16384, 4                                                                  # G * B = PVF_HIST_MAX_ROWS: 64 MiB of result
    wins = np.array([(0, 0, 85, 17), (3, 1, 80, 9), (-5, -5, 20, 20)], np.int32)
    group = np.array([0, G - 1, 8191], np.int32)
    got = bare_ctx.frame_hist([dev] * 3, wins, group, G, bands=B)
    assert got.shape == (G, B, 256) and int(got.sum()) == 85 * 17 + 77 * 8 + 20 * 17
    small = cr.hist_of([f] * 3, wins, [0, 1, 2], 3, B)
    for k, g in enumerate(group):
        _same(got[g], small[k], g)
    rng = np.random.default_rng(5)
    xy = np.stack([rng.integers(-2, 87, 5000), rng.integers(-2, 19, 5000)], axis=1)
    wins = np.concatenate([xy, xy + 1], axis=1).astype(np.int32)
    group = np.arange(5000, dtype=np.int32) % 7
    _same(bare_ctx.frame_hist([dev] * 5000, wins, group, 7, bands=1), cr.hist_of([f] * 5000, wins, group, 7, 1), "one-pixel windows")
    dev.release()


@pytest.mark.parametrize("w,h", cc.LARGE)
def test_full_size_frames(bare_ctx, w, h):
    f = cc.frame_of("noise", w, h)
    dev = bare_ctx.upload(f)
    wins = cc.large_windows(w, h)
    n = len(wins)
    group = np.arange(n, dtype=np.int32) % 11
    _same(bare_ctx.frame_hist([dev] * n, wins, group, 11, bands=3), cr.hist_of([f] * n, wins, group, 11, 3), (w, h))
    dev.release()
    # one colour everywhere: every lane of a wave adds to one bin
    flat = cc.frame_of("mid", w, h)
    dev = bare_ctx.upload(flat)
    got = bare_ctx.frame_hist([dev] * 2, wins[:2], [0, 0], 1, bands=1)
    assert int(got[0, 0, int(cr.bins_of(np.array(cc.MID)))]) == 600 * 600 + w * h == int(got.sum())
    dev.release()


def test_refusals(bare_ctx):
    from pyannote_video_amd import _lib
    c, l, P_ = bare_ctx, bare_ctx._l, _lib.ptr
    f = cc.frame_of("noise", 256, 256)
    a, gone = c.upload(f), c.upload(f)
    gone_handle = gone.handle
    gone.release()
    hs = np.array([a.handle, a.handle], np.uint64)
    wins = np.array([(0, 0, 256, 256), (10, 10, 20, 300)], np.int32)
    grp = np.array([0, 1], np.int32)
    ref = cr.hist_of([f, f], wins, grp, 2, 2)
    out = np.full((2, 2, 256), 0xA5A5A5A5, np.uint32)
    many = 65536
    whole = np.tile(np.array([(0, 0, 256, 256)], np.int32), (many, 1))               # 65536 windows of 2^16 pixels: 2^32 in one group

    def call(frames=hs, w=wins, g=grp, n=2, G=2, B=2, o=out, dev=0):
        return l.pvf_frame_hist(c._h, P_(frames), P_(w), P_(g), n, G, B, P_(o), dev)
    for kw, message in ((dict(n=-1), "n outside"), (dict(n=65537), "n outside"), (dict(G=0), "G below 1"), (dict(B=0), "B outside"), (dict(B=5), "B outside"),
                        (dict(G=16385, B=4), "PVF_HIST_MAX_ROWS"), (dict(G=65537, B=1), "PVF_HIST_MAX_ROWS"),
                        (dict(frames=None), "null"), (dict(w=None), "null"), (dict(g=None), "null"), (dict(o=None), "null"),
                        (dict(g=np.array([0, 2], np.int32)), "a group outside"), (dict(g=np.array([-1, 0], np.int32)), "a group outside"),
                        (dict(frames=np.array([a.handle, 987654321], np.uint64)), "unknown frame handle"),
                        (dict(frames=np.array([gone_handle, a.handle], np.uint64)), "unknown frame handle"),
                        (dict(frames=np.full(many, a.handle, np.uint64), w=whole, g=np.zeros(many, np.int32), n=many), "2^32 pixels")):
        assert call(**kw) != 0, message
        assert message in l.pvf_last_error().decode(), (message, l.pvf_last_error().decode())
        assert (out == 0xA5A5A5A5).all()                            # refused before any work
        assert call() == 0 and np.array_equal(out, ref)             # the context goes on
        out[:] = 0xA5A5A5A5
    # one window fewer in the group stays below 2^32 and is not refused on that ground; n = 0 writes zeros
    assert l.pvf_frame_hist(c._h, None, None, None, 0, 2, 2, P_(out), 0) == 0 and not out.any()
    a.release()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_the_verbs_in_processes_of_their_own(tmp_path):
    from pyannote_video_amd import cli, formats
    from pyannote_video_amd.pipeline import faces_per_frame
    spec, fps = "synthetic:320x180x12:2:2:3", 25.0
    video = cli.open_video(spec, fps)
    frames = [np.asarray(f) for _, f in video]
    lines = []
    for fi in range(12):                                                             # two tracks that cross nobody, one cut by the frame's lower edge
        lines.append((fi / fps, 0, (0.1 + 0.01 * fi, 0.1, 0.2 + 0.01 * fi, 0.3), "detection"))
        lines.append((fi / fps, 1, (0.6, 0.05 + 0.02 * fi, 0.75, 0.35 + 0.02 * fi), "detection"))
    for fi in range(3, 9):
        lines.append((fi / fps, 5, (0.4, 0.85, 0.5, 0.99), "detection"))             # its window lies below the frame: skipped
    tracking, table, out, lab, merged = (str(tmp_path / n) for n in ("track.txt", "clothes.npy", "links.json", "labels.txt", "merged.txt"))
    with open(tracking, "w") as fo:
        for T, i, box, status in lines:
            fo.write("%.3f %d %.3f %.3f %.3f %.3f %s\n" % ((T, i) + box + (status,)))
    with open(lab, "w") as fo:
        fo.write("0 0\n1 1\n5 5\n")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pyannote-video_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for args in (["clothes", "--batch", "5", spec, tracking, table], ["link", "--labels", lab, "--merged", merged, table, out]):
        run = subprocess.run([sys.executable, "-m", "pyannote_video_amd", "--fps", str(fps)] + args, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, env=env, timeout=600)
        assert run.returncode == 0, (args, run.stderr.decode()[-2000:])
    rows = formats.read_tracks(tracking)
    per = [(fi, T, [(int(t), b) for t, b in g]) for fi, T, g in faces_per_frame(rows, [i / fps for i in range(12)], 320, 180, drop_last=False)]
    want = cr.table_of(dict(enumerate(frames)), per, {0, 1, 5})
    got = np.load(table)
    _same(got, want)
    assert got[:, 3].tolist() == [12, 12, 0] and got[:, 4].tolist() == [0, 0, 6] and int(got[0, 6:].sum()) > 0
    doc = json.load(open(out))
    assert [(d["a"], d["b"], d["score"]) for d in doc["links"]] == cr.links_of(want)
    assert sorted(open(merged).read().split("\n")[:-1]) == sorted("%d %s" % kv for kv in cr.merged_labels({0: "0", 1: "1", 5: "5"}, cr.links_of(want), want).items())
