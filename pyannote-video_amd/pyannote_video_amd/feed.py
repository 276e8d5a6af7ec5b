"""`FrameFeed`: the chosen frames of a video, read in a thread of their own and staged in HBM ahead of the thread that computes on them.
What the verbs that read some frames of a film share (cli.py: extract, faces, talk, tube, clothes, demo / redact and storyboard.build) and,
with `EveryKth` as the chosen frames and `frame_range` as its bounds, the verbs that measure every frame (fingerprint, blend, motion,
text); all but clothes and demo / redact take the frames a library call's worth at a time (`FrameFeed.batches`).  The verbs that read every
frame and cut it into shots go through engine.StreamSource."""
import queue
import threading
from .runtime import HostFrameStager


def frame_range(video, t_from=0.0, t_until=None):
    """(first, end): the frames of `video` whose time index / frame_rate lies in [t_from, t_until), cut at the video's length; end is None
    for a stream, which has no length, without t_until: as far as it goes"""
    rate = float(video.frame_rate)
    first = 0
    while first / rate < t_from:
        first += 1
    end = None
    if t_until is not None:
        end = first
        while end / rate < t_until:
            end += 1
    try:
        end = len(video) if end is None else min(end, len(video))
    except TypeError:
        pass
    return first, end


class EveryKth(object):
    """the `wanted` of a FrameFeed that wants every k-th frame from `first` on, below `end`, whatever the video's length"""

    def __init__(self, first=0, end=None, k=1):
        self.first, self.end, self.k = int(first), (1 << 40 if end is None else int(end)), int(k)

    def __contains__(self, i):
        return self.first <= i < self.end and (i - self.first) % self.k == 0

    def __iter__(self):                  # (the feed reads up to max(wanted))
        return iter((self.first + (len(self) - 1) * self.k,))

    def __len__(self):
        return max((self.end - self.first + self.k - 1) // self.k, 0)


class FrameFeed(object):
    """The frames of `video` (an iterable of (t, frame): numpy RGB, YuvFrame or DeviceFrame) whose index is in `wanted`, as
    (index, device frame) in ascending index:

        with FrameFeed(ctx, video, wanted, ahead=96, name="pvface-talk-reader") as feed:
            for fi, dev in feed:
                ...
                feed.release(dev)

    A reader thread pushes them through a pinned ingest ring of `ring_depth` slots (runtime.HostFrameStager: asynchronous uploads) and
    is never more than `ahead` queued frames in front of the consumer.  It reads up to the last wanted frame and no further; nothing
    at all when `wanted` is empty.  seek: a source that has .frame(i) is asked for the wanted frames alone instead of being iterated.
    The feed owns the frames it staged: release() gives one back, leaving the block gives back the rest, queued or handed out.  A
    DeviceFrame the video itself yielded is passed through and stays the video's.  An error of the reader thread is raised where the
    iteration ends, or on leaving the block; it never replaces an exception of the consumer."""

    def __init__(self, ctx, video, wanted, ahead=96, ring_depth=16, seek=False, name="pvface-reader"):
        self._video, self._wanted = video, wanted
        self._seek = seek and hasattr(video, "frame")
        self._q = queue.Queue(maxsize=max(2, int(ahead)))
        self._stager = HostFrameStager(ctx, ring_depth)
        self._staged = {}                    # id(frame) -> frame, for every frame staged here and not yet released
        self._stop = False
        self.error = None
        self._th = threading.Thread(target=self._read, name=name)

    def _read(self):
        video, wanted = self._video, self._wanted
        try:
            if not wanted:
                source = ()
            elif self._seek:                 # only the wanted frames are read (--from deep into a file)
                source = ((fi, video.frame(fi)) for fi in sorted(wanted))
            else:
                source = ((fi, frame) for fi, (_, frame) in zip(range(max(wanted) + 1), video))
            for fi, frame in source:
                if self._stop:
                    break
                if fi not in wanted:
                    continue
                frame, owned = self._stager.stage(frame)
                if owned:
                    self._staged[id(frame)] = frame
                self._q.put((fi, frame))
            self._stager.close()             # waits for the last uploads
        except BaseException as e:           # noqa: BLE001 -- re-raised in the consumer
            self.error = e
        finally:
            self._q.put(None)

    def __enter__(self):
        self._th.start()
        return self

    def __iter__(self):
        while True:
            item = self._q.get()
            if item is None:
                self._q.put(None)            # the end mark stays: a second iteration ends at once
                self._raise_reader_error()
                return
            yield item

    def batches(self, size, weight=None):
        """the same frames as lists of (index, device frame), a library call's worth each: a list is closed by the frame that brings the
        sum of weight(index) -- 1 a frame without `weight` -- to `size` or more; what is left at the end is the last, shorter list.
        Nothing is released here: the caller gives back what its call is done with."""
        part, held = [], 0
        for item in self:
            part.append(item)
            held += 1 if weight is None else weight(item[0])
            if held >= size:
                yield part
                part, held = [], 0
        if part:
            yield part

    def _raise_reader_error(self):
        e, self.error = self.error, None
        if e is not None:
            raise e

    def release(self, frame):
        """give back a frame of this feed; a frame it did not stage, or has given back already, is left alone"""
        mine = self._staged.pop(id(frame), None)
        if mine is not None:
            mine.release()

    def release_all(self, frames):
        for frame in frames:
            self.release(frame)

    def __exit__(self, exc_type, exc, tb):
        self._stop = True
        while self._th.is_alive():           # the reader may be waiting for room in the queue: make some until it has seen the flag
            try:
                self._q.get(timeout=0.05)
            except queue.Empty:
                pass
        self._th.join()
        while True:
            try:
                self._q.get_nowait()
            except queue.Empty:
                break
        self.release_all(list(self._staged.values()))
        self._stager.close()
        if exc_type is None:
            self._raise_reader_error()
        return False
