"""CPU: feed.FrameFeed -- the reader thread, bounded queue, pinned ring and frame ownership that the verbs reading chosen frames share
(cli.py: extract, faces, talk, tube, demo / redact) -- on a scripted video and ring: order and filter, seeking, the bound on what is
staged ahead, whose error comes out, and that every frame the feed staged is given back exactly once however the block is left.  Then
FrameFeed.batches, the lists the verbs make one library call on: by frame count, by weight, with a failing reader, left early.  Then
cli._render_plan (the body of demo and redact) on a scripted egress ring: one picture per plan entry, in plan order."""
import threading

import numpy as np
import pytest

from pyannote_video_amd import cli
from pyannote_video_amd.feed import FrameFeed


class Dev(object):
    def __init__(self, i):
        self.i, self.released = i, False

    def release(self):
        assert not self.released
        self.released = True


class Ring(object):
    def __init__(self, ctx):
        self.ctx = ctx

    def push(self, rgb):
        d = Dev(int(rgb[0, 0, 0]))
        with self.ctx.pushed:
            self.ctx.frames.append(d)
            self.ctx.lead = max(self.ctx.lead, len(self.ctx.frames) - self.ctx.done)
            self.ctx.pushed.notify_all()
        return d

    def close(self):
        self.ctx.rings_open -= 1


class Context(object):
    """frames: every frame a ring of this context made; lead: the most that were ever staged beyond the `done` the consumer counts"""

    def __init__(self):
        self.frames, self.done, self.lead, self.rings_open = [], 0, 0, 0
        self.pushed = threading.Condition()

    def ingest_ring(self, h, w, depth=16):
        self.rings_open += 1
        return Ring(self)


def picture(i):
    a = np.zeros((2, 4, 3), np.uint8)
    a[0, 0, 0] = i
    return a


class Video(object):
    """n frames, numbered in their first byte; fail_at: the frame whose decoding fails"""

    def __init__(self, n, fail_at=None):
        self.n, self.fail_at, self.read = n, fail_at, []

    def __iter__(self):
        for i in range(self.n):
            if i == self.fail_at:
                raise IOError("scripted decode error")
            self.read.append(i)
            yield i / 25.0, picture(i)


class SeekVideo(Video):
    def __init__(self, n):
        Video.__init__(self, n)
        self.sought = []

    def frame(self, i):
        self.sought.append(i)
        return picture(i)


class NoIterVideo(SeekVideo):
    def __iter__(self):
        raise AssertionError("the video was iterated")


def settled(ctx, threads):
    """everything staged went back, the ring is closed and the reader thread is gone"""
    return all(d.released for d in ctx.frames) and ctx.rings_open == 0 and threading.active_count() == threads


@pytest.mark.parametrize("wanted", [{0, 5, 11}, {3}, set()])
def test_frames_come_in_order_and_only_the_wanted_ones(wanted):
    threads = threading.active_count()
    ctx, video = Context(), Video(12) if wanted else NoIterVideo(12)
    with FrameFeed(ctx, video, wanted, ahead=2) as feed:
        got = []
        for fi, dev in feed:
            assert dev.i == fi and not dev.released
            got.append(fi)
            feed.release(dev)
    assert got == sorted(wanted) and [d.i for d in ctx.frames] == sorted(wanted)
    assert video.read == list(range(max(wanted) + 1 if wanted else 0))             # no frame beyond the last wanted one; none at all
    assert settled(ctx, threads)


def test_a_dictionary_keyed_by_the_indices_serves_as_wanted():
    ctx, threads = Context(), threading.active_count()
    with FrameFeed(ctx, Video(12), {4: "a", 2: "b"}, ahead=2) as feed:
        assert [fi for fi, _ in feed] == [2, 4]
        assert list(feed) == []                                                     # a second iteration ends at once
    assert settled(ctx, threads)


def test_device_frames_of_the_video_pass_through_and_stay_its_own():
    class DeviceVideo(object):
        def __init__(self):
            self.frames = [Dev(i) for i in range(6)]

        def __iter__(self):
            for d in self.frames:
                yield d.i / 25.0, d
    ctx, video = Context(), DeviceVideo()
    with FrameFeed(ctx, video, {1, 4}, ahead=2) as feed:
        got = list(feed)
        feed.release(got[0][1])
    assert got == [(1, video.frames[1]), (4, video.frames[4])]
    assert not ctx.frames and not any(d.released for d in video.frames)


def test_seeking_reads_the_wanted_frames_alone():
    wanted, threads = {7, 2, 9}, threading.active_count()
    ctx, video = Context(), NoIterVideo(12)
    with FrameFeed(ctx, video, wanted, ahead=2, seek=True) as feed:
        assert [(fi, dev.i) for fi, dev in feed] == [(2, 2), (7, 7), (9, 9)]
    assert video.sought == [2, 7, 9]
    plain = Video(12)                                                               # nothing to seek with: iterated and filtered
    with FrameFeed(ctx, plain, wanted, ahead=2, seek=True) as feed:
        assert [fi for fi, _ in feed] == [2, 7, 9]
    assert plain.read == list(range(10))
    video = SeekVideo(12)                                                           # seeking is the caller's choice
    with FrameFeed(ctx, video, wanted, ahead=2) as feed:
        assert [fi for fi, _ in feed] == [2, 7, 9]
    assert video.sought == [] and video.read == list(range(10))
    assert settled(ctx, threads)


def test_the_reader_stays_within_ahead_of_the_consumer():
    """ahead = 2: while the consumer holds its first frame, two wait in the queue and the reader holds one it cannot queue"""
    ahead, threads = 2, threading.active_count()
    ctx = Context()
    with FrameFeed(ctx, Video(12), set(range(12)), ahead=ahead) as feed:
        for k, (fi, dev) in enumerate(feed):
            if k == 0:
                with ctx.pushed:                                                    # as far ahead as it gets
                    assert ctx.pushed.wait_for(lambda: len(ctx.frames) >= ahead + 2, timeout=10)
            feed.release(dev)
            with ctx.pushed:
                ctx.done += 1
    assert len(ctx.frames) == 12 and ctx.lead == ahead + 2                          # (a reader that ran on past the bound is seen by the end)
    assert settled(ctx, threads)


def test_an_error_of_the_reader_reaches_the_caller():
    threads = threading.active_count()
    ctx, got = Context(), []
    with pytest.raises(IOError, match="scripted decode error"):
        with FrameFeed(ctx, Video(12, fail_at=7), set(range(12)), ahead=2) as feed:
            for fi, dev in feed:
                got.append(fi)
    assert got == list(range(7)) and len(ctx.frames) == 7
    assert settled(ctx, threads)
    ctx = Context()                                                                 # a consumer that left early learns of it on the way out
    with pytest.raises(IOError, match="scripted decode error"):
        with FrameFeed(ctx, Video(12, fail_at=1), set(range(12)), ahead=2) as feed:
            for fi, dev in feed:
                break
    assert settled(ctx, threads)


def test_an_error_of_the_consumer_comes_out_and_stops_the_reader():
    ahead, threads = 2, threading.active_count()
    ctx, video, got = Context(), Video(200), []
    with pytest.raises(RuntimeError, match="scripted device error"):
        with FrameFeed(ctx, video, set(range(200)), ahead=ahead) as feed:
            for fi, dev in feed:
                got.append(fi)
                if len(got) == 3:
                    raise RuntimeError("scripted device error")
                feed.release(dev)
    assert got == [0, 1, 2] and len(ctx.frames) <= 3 + ahead + 2
    assert settled(ctx, threads)
    ctx = Context()                                                                 # ... even when the reader failed as well
    with pytest.raises(RuntimeError, match="scripted device error"):
        with FrameFeed(ctx, Video(12, fail_at=1), set(range(12)), ahead=ahead) as feed:
            for fi, dev in feed:
                raise RuntimeError("scripted device error")
    assert settled(ctx, threads)


def test_leaving_early_gives_everything_back():
    threads = threading.active_count()
    ctx = Context()
    with FrameFeed(ctx, Video(50), set(range(50)), ahead=4) as feed:
        for fi, dev in feed:
            if fi == 5:
                break                                                               # frames 0 .. 5 handed out and kept, more in the queue
    assert 6 <= len(ctx.frames) < 50
    assert settled(ctx, threads)


def test_release_is_safe_to_repeat_and_ignores_foreign_frames():
    ctx, foreign = Context(), Dev(99)
    with FrameFeed(ctx, Video(4), {0, 1, 2, 3}, ahead=2) as feed:
        devs = [dev for _, dev in feed]
        feed.release(devs[0])
        assert devs[0].released
        feed.release(devs[0])                                                       # (Dev.release asserts that it is called once)
        feed.release_all([devs[1], devs[1], foreign, devs[0]])
        feed.release(foreign)
        feed.release(None)
        assert [d.released for d in devs] == [True, True, False, False] and not foreign.released
    assert settled(ctx, threading.active_count()) and not foreign.released


# ---- FrameFeed.batches: the same frames, a library call's worth at a time ----
@pytest.mark.parametrize("n,size", [(0, 4), (3, 4), (8, 4), (9, 4), (5, 1)])
def test_batches_by_frame_count(n, size):
    threads = threading.active_count()
    ctx, parts = Context(), []
    with FrameFeed(ctx, Video(n), set(range(n)), ahead=2) as feed:
        for part in feed.batches(size):
            assert part and all(dev.i == fi and not dev.released for fi, dev in part)
            parts.append([fi for fi, _ in part])
            feed.release_all(dev for _, dev in part)
    assert [len(p) for p in parts] == [size] * (n // size) + ([n % size] if n % size else [])
    assert [fi for p in parts for fi in p] == list(range(n))
    assert settled(ctx, threads)


@pytest.mark.parametrize("weights,want", [((1, 3, 2, 5, 1, 1), [[0, 1], [2, 3], [4, 5]]),       # closed by the frame that brings the sum to 4
                                          ((5, 1, 3, 9, 2), [[0], [1, 2], [3], [4]])])          # a frame heavier than the size: a list of its own
def test_batches_by_weight(weights, want):
    threads = threading.active_count()
    ctx, parts, asked = Context(), [], []

    def weight(fi):
        asked.append(fi)
        return weights[fi]
    with FrameFeed(ctx, Video(len(weights)), set(range(len(weights))), ahead=2) as feed:
        for part in feed.batches(4, weight):
            parts.append([fi for fi, _ in part])
            assert not any(dev.released for _, dev in part)                         # nothing is released on the way: the caller does
    assert parts == want and asked == list(range(len(weights)))
    assert settled(ctx, threads)


def test_batches_raise_an_error_of_the_reader_where_they_end():
    threads = threading.active_count()
    ctx, parts = Context(), []
    with FrameFeed(ctx, Video(12, fail_at=7), set(range(12)), ahead=2) as feed:
        with pytest.raises(IOError, match="scripted decode error"):
            for part in feed.batches(3):
                parts.append([fi for fi, _ in part])
        assert parts == [[0, 1, 2], [3, 4, 5]]                                      # the lists in front of it; frame 6 was in no list
        assert not any(d.released for d in ctx.frames)
    assert len(ctx.frames) == 7 and settled(ctx, threads)


def test_leaving_the_batches_early_gives_everything_back():
    threads = threading.active_count()
    ctx = Context()
    with FrameFeed(ctx, Video(50), set(range(50)), ahead=4) as feed:
        for part in feed.batches(4):
            assert [fi for fi, _ in part] == [0, 1, 2, 3]
            feed.release(part[0][1])                                                # one given back here, the rest kept
            break
    assert 4 <= len(ctx.frames) < 50
    assert settled(ctx, threads)                                                    # (Dev.release asserts that it is called once)


# ---- cli._render_plan: the feed in front, the egress ring and the writer thread behind ----
WIDTH, HEIGHT = 4, 2
FRAME_BYTES = WIDTH * HEIGHT + 2 * (WIDTH // 2) * (HEIGHT // 2)


class EgressRing(object):
    """the contract of runtime.EgressRing: submit takes the next slot and refuses one that has not been given back"""

    def __init__(self, ctx, depth):
        self.ctx, self.depth, self.n, self.busy, self.closed = ctx, depth, 0, {}, False

    def submit(self, dev, prims):
        assert not dev.released, "a render asked of a released frame"
        self.ctx.submits.append((dev.i, prims))
        if len(self.ctx.submits) == self.ctx.fail_at:
            raise RuntimeError("scripted render error")
        slot, self.n = self.n % self.depth, self.n + 1
        assert slot not in self.busy, "slot %d has not been given back" % slot
        self.busy[slot] = prims
        return slot

    def wait(self, slot):
        return np.full(FRAME_BYTES, self.busy[slot], np.uint8)

    def release(self, slot):
        del self.busy[slot]

    def close(self):
        self.closed = True


class RenderContext(Context):
    def __init__(self, fail_at=None):
        Context.__init__(self)
        self.submits, self.fail_at, self.ring = [], fail_at, None

    def egress_ring(self, width, height, matrix, full_range, depth=8):
        assert (width, height) == (WIDTH, HEIGHT)
        self.ring = EgressRing(self, depth)
        return self.ring


# (source frame, time, primitives: here the number the scripted ring fills the picture with); frame 2 is shown twice, 1 and 4 never
PLAN = [(0, 0.0, 10), (2, 0.04, 11), (2, 0.08, 12), (3, 0.12, 13), (5, 0.16, 14), (6, 0.2, 15)]


@pytest.mark.parametrize("video", [Video, NoIterVideo], ids=["iterated", "sought"])
def test_render_plan_writes_one_picture_per_plan_entry(tmp_path, video):
    threads = threading.active_count()
    ctx, video, out = RenderContext(), video(12), str(tmp_path / "out.y4m")
    res = cli._render_plan(video, PLAN, out, WIDTH, HEIGHT, "601", False, 25.0, ctx, 2)
    assert res == {"frames": len(PLAN), "width": WIDTH, "height": HEIGHT}
    assert ctx.submits == [(i, prims) for i, _, prims in PLAN]
    assert open(out, "rb").read() == b"YUV4MPEG2 W4 H2 F25:1 C420\n" + b"".join(b"FRAME\n" + bytes([prims]) * FRAME_BYTES for _, _, prims in PLAN)
    assert [d.i for d in ctx.frames] == [0, 2, 3, 5, 6]                             # each shown frame staged once, the others never
    assert settled(ctx, threads) and ctx.ring.closed and not ctx.ring.busy


def test_render_plan_hands_on_an_error_of_the_ring(tmp_path):
    threads = threading.active_count()
    ctx, out = RenderContext(fail_at=3), str(tmp_path / "out.y4m")
    with pytest.raises(RuntimeError, match="scripted render error"):
        cli._render_plan(Video(12), PLAN, out, WIDTH, HEIGHT, "601", False, 25.0, ctx, 2)
    assert len(ctx.submits) == 3 and len(ctx.frames) >= 2
    assert settled(ctx, threads) and ctx.ring.closed
