"""CPU: the YUV -> RGB definition (tests/yuv_ref.py) and its pins, the YUV4MPEG2 reader (pyannote_video_amd/y4m.py), `open_video`'s
choice of reader, and the streaming source fed from a Y4M file on the scripted context of tests/test_engine.py."""
import io
import json

import numpy as np
import pytest

from tests import yuv_ref


# ---- the definition -------------------------------------------------------------------------------------------------------------------

def test_constant_sets():
    assert (65536 * 255) // 219 == 76309
    assert yuv_ref.constants("601", False) == (104597, 132201, 25675, 53279)
    assert yuv_ref.constants("709", False) == (117504, 138453, 13954, 34903)
    assert yuv_ref.constants("601", True) == (91881, 116129, 22553, 46801)
    assert yuv_ref.constants("709", True) == (103219, 121621, 12257, 30659)


@pytest.mark.parametrize("matrix", ["601", "709"])
def test_grey_ramp_end_points(matrix):
    Y = np.arange(256, dtype=np.uint8).reshape(1, 256)
    g = np.full((1, 256), 128, np.uint8)
    lim = yuv_ref.to_rgb(Y, g, g, "444", matrix, False)
    assert (lim[0, :, 0] == lim[0, :, 1]).all() and (lim[0, :, 1] == lim[0, :, 2]).all()
    assert lim[0, 16, 0] == 0 and lim[0, 235, 0] == 255 and lim[0, 0, 0] == 0 and lim[0, 255, 0] == 255
    assert lim[0, 17, 0] == 1 and lim[0, 234, 0] == 254
    full = yuv_ref.to_rgb(Y, g, g, "444", matrix, True)
    assert (full[0] == Y[0][:, None]).all()


def test_accumulators_fit_int32_over_the_whole_cube():
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = {}
    for matrix in ("601", "709"):
        for full in (False, True):
            m = 0
            for Y in range(256):
                m = max(m, max(int(np.abs(a).max()) for a in yuv_ref.accumulators(np.full_like(U, Y), U, V, matrix, full)))
            worst[matrix, full] = m
    assert max(worst.values()) == 35854150 < 2 ** 31
    assert worst == {("601", False): 35060146, ("601", True): 31492831, ("709", False): 35854150, ("709", True): 32190315}


def test_chroma_is_replicated():
    Y = np.full((3, 5), 128, np.uint8)
    U = np.array([[0, 128, 255], [64, 200, 30]], np.uint8)
    V = np.array([[255, 128, 0], [10, 90, 250]], np.uint8)
    out = yuv_ref.to_rgb(Y, U, V, "420")
    for y in range(3):
        for x in range(5):
            one = yuv_ref.to_rgb(Y[:1, :1], U[y >> 1:(y >> 1) + 1, x >> 1:(x >> 1) + 1], V[y >> 1:(y >> 1) + 1, x >> 1:(x >> 1) + 1], "444")
            assert (out[y, x] == one[0, 0]).all()
    assert yuv_ref.chroma_shape(45, 67, "420") == (23, 34) and yuv_ref.chroma_shape(45, 67, "422") == (45, 34)
    assert yuv_ref.chroma_shape(1, 1, "420") == (1, 1) and yuv_ref.chroma_shape(45, 67, "444") == (45, 67)


# ---- the reader -----------------------------------------------------------------------------------------------------------------------

def _clip(h, w, layout, n, seed=0):
    return [yuv_ref.noise_planes(h, w, layout, seed + i) for i in range(n)]


def _same_planes(frame, planes):
    return all((a == b).all() for a, b in zip((frame.y, frame.u, frame.v), planes))


@pytest.mark.parametrize("w,h,n", [(64, 48, 5), (67, 45, 4), (1, 1, 3), (1920, 1080, 1)])
@pytest.mark.parametrize("layout", ["420", "422", "444"])
def test_round_trip(tmp_path, w, h, n, layout):
    from pyannote_video_amd.y4m import Y4mVideo
    clip = _clip(h, w, layout, n)
    v = Y4mVideo(yuv_ref.write_y4m(str(tmp_path / "a.y4m"), clip, layout))
    assert v.size == (w, h) and v.frame_size == (w, h) and len(v) == n and v.frame_rate == 25.0 and v.layout == layout
    assert v.duration == n / 25.0 and (v.step, v.start, v.end) == (1 / 25.0, 0.0, v.duration)
    v.frame_size = (32.0, 24)
    assert v.frame_size == (32, 24) and v.size == (w, h)
    for _ in range(2):                                   # a second pass reads the same frames
        got = list(v)
        assert [t for t, _ in got] == [i / 25.0 for i in range(n)]
        for (t, f), planes in zip(got, clip):
            assert (f.height, f.width, f.layout, f.matrix, f.full_range) == (h, w, layout, "601", False)
            assert _same_planes(f, planes)
    assert _same_planes(v.frame(n - 1), clip[n - 1])
    f = v.frame(0)
    assert f.rgb().shape == (h, w, 3) and (f.rgb() == yuv_ref.to_rgb(*clip[0], layout=layout)).all()


@pytest.mark.parametrize("matrix", ["601", "709"])
@pytest.mark.parametrize("full", [False, True])
def test_rgb_of_a_frame_is_the_reference(tmp_path, matrix, full):
    from pyannote_video_amd.y4m import Y4mVideo
    for layout in ("420", "422", "444"):
        clip = _clip(45, 67, layout, 1, seed=9)
        v = Y4mVideo(yuv_ref.write_y4m(str(tmp_path / ("%s.y4m" % layout)), clip, layout), matrix=matrix, full_range=full)
        ref = yuv_ref.to_rgb(*clip[0], layout=layout, matrix=matrix, full_range=full)
        assert ref.min() == 0 and ref.max() == 255
        assert (v.frame(0).rgb() == ref).all()


@pytest.mark.parametrize("tag,layout", [("420", "420"), ("420jpeg", "420"), ("420mpeg2", "420"), ("420paldv", "420"), ("", "420"),
                                        ("422", "422"), ("444", "444")])
def test_accepted_chroma_tags(tmp_path, tag, layout):
    from pyannote_video_amd.y4m import Y4mVideo
    clip = _clip(6, 10, layout, 2)
    v = Y4mVideo(yuv_ref.write_y4m(str(tmp_path / "a.y4m"), clip, layout, tag=tag, extra=("Ip", "A1:1")))
    assert v.layout == layout and len(v) == 2 and _same_planes(v.frame(1), clip[1])


@pytest.mark.parametrize("extra,tag,name", [((), "mono", "Cmono"), ((), "420p10", "C420p10"), ((), "444p12", "C444p12"),
                                            (("It",), None, "It"), (("Ib",), None, "Ib"), (("Im",), None, "Im")])
def test_refused_tags_are_named(tmp_path, extra, tag, name):
    from pyannote_video_amd.y4m import Y4mVideo
    p = yuv_ref.write_y4m(str(tmp_path / "a.y4m"), _clip(6, 10, "420", 1), "420", tag=tag, extra=extra)
    with pytest.raises(IOError, match=name):
        Y4mVideo(p)


def test_rate_range_and_frame_parameters(tmp_path):
    from pyannote_video_amd.y4m import Y4mVideo
    clip = _clip(6, 10, "420", 4)
    v = Y4mVideo(yuv_ref.write_y4m(str(tmp_path / "a.y4m"), clip, rate="30000:1001", frame_params="Ip XFOO=1"), frame_rate=25.0)
    assert v.frame_rate == 30000 / 1001.0 and len(v) == 4 and all(_same_planes(f, c) for (t, f), c in zip(v, clip))
    assert [t for t, _ in v] == [i / v.frame_rate for i in range(4)]
    # --fps counts only where the header names no rate
    v = Y4mVideo(yuv_ref.write_y4m(str(tmp_path / "b.y4m"), clip, rate=None), frame_rate=12.5)
    assert v.frame_rate == 12.5
    with pytest.raises(IOError, match="frame rate"):
        Y4mVideo(str(tmp_path / "b.y4m"))
    assert Y4mVideo(yuv_ref.write_y4m(str(tmp_path / "c.y4m"), clip, extra=("XCOLORRANGE=FULL",))).full_range is True
    assert Y4mVideo(yuv_ref.write_y4m(str(tmp_path / "d.y4m"), clip, extra=("XCOLORRANGE=LIMITED",))).full_range is False
    assert Y4mVideo(str(tmp_path / "a.y4m")).full_range is False
    assert Y4mVideo(str(tmp_path / "c.y4m"), full_range=False).full_range is False            # the caller overrides the header
    assert Y4mVideo(str(tmp_path / "c.y4m"), matrix="709").frame(0).matrix == "709"
    with pytest.raises(IOError, match="XCOLORRANGE=WIDE"):
        Y4mVideo(yuv_ref.write_y4m(str(tmp_path / "e.y4m"), clip, extra=("XCOLORRANGE=WIDE",)))


def test_damaged_files_are_refused(tmp_path):
    from pyannote_video_amd.y4m import Y4mVideo
    clip = _clip(6, 10, "420", 3)
    with pytest.raises(IOError, match="frame 2 is truncated"):
        Y4mVideo(yuv_ref.write_y4m(str(tmp_path / "a.y4m"), clip, truncate=1))
    with open(str(tmp_path / "b.y4m"), "wb") as f:
        f.write(b"RIFF....AVI \n")
    with pytest.raises(IOError, match="not a YUV4MPEG2"):
        Y4mVideo(str(tmp_path / "b.y4m"))
    data = open(yuv_ref.write_y4m(str(tmp_path / "c.y4m"), clip), "rb").read()
    with open(str(tmp_path / "d.y4m"), "wb") as f:
        f.write(data.replace(b"FRAME", b"FRAMX"))
    with pytest.raises(IOError, match="FRAME"):
        Y4mVideo(str(tmp_path / "d.y4m"))


def test_time_to_frame_rule_is_npy_videos(tmp_path):
    from pyannote_video_amd.cli import NpyVideo
    from pyannote_video_amd.y4m import Y4mVideo
    n = 30
    clip = _clip(4, 6, "420", n)
    for rate, fps in (("25:1", 25.0), ("30000:1001", 30000 / 1001.0)):
        y = Y4mVideo(yuv_ref.write_y4m(str(tmp_path / "a.y4m"), clip, rate=rate))
        np.save(str(tmp_path / "a.npy"), np.stack([yuv_ref.to_rgb(*p) for p in clip]))
        v = NpyVideo(str(tmp_path / "a.npy"), fps)
        assert len(v) == len(y) and v.duration == y.duration and (v.step, v.start, v.end) == (y.step, y.start, y.end)
        times = [i / fps for i in range(n)] + [i / fps + 0.5 / fps for i in range(n)] + [0.0199999, 0.04 - 1e-6, 0.3333333, 1.0, n / fps - 1e-9]
        for t in times:
            try:
                want = v(t)
            except IOError:
                with pytest.raises(IOError):
                    y(t)
                continue
            assert (y(t).rgb() == want).all(), t
        for t in (-0.5, n / fps, 99.0):
            with pytest.raises(IOError):
                v(t)
            with pytest.raises(IOError):
                y(t)


def test_a_stream_is_read_once_and_has_no_length(tmp_path):
    from pyannote_video_amd.y4m import Y4mVideo
    clip = _clip(5, 7, "420", 3)
    data = open(yuv_ref.write_y4m(str(tmp_path / "a.y4m"), clip, frame_params="Ip"), "rb").read()
    v = Y4mVideo(io.BytesIO(data))
    assert v.size == (7, 5) and v.frame_rate == 25.0
    with pytest.raises(TypeError, match="no length"):
        len(v)
    got = list(v)
    assert [t for t, _ in got] == [0.0, 0.04, 0.08] and all(_same_planes(f, c) for (t, f), c in zip(got, clip))
    with pytest.raises(IOError, match="truncated"):
        list(Y4mVideo(io.BytesIO(data[:-3])))


# ---- open_video -----------------------------------------------------------------------------------------------------------------------

def test_open_video_picks_the_reader_by_suffix_and_by_magic(tmp_path):
    """(the test that fails without the feature: np.load cannot read a Y4M file)"""
    from pyannote_video_amd import cli
    from pyannote_video_amd.y4m import Y4mVideo
    clip = _clip(6, 10, "420", 2)
    by_suffix = cli.open_video(yuv_ref.write_y4m(str(tmp_path / "a.y4m"), clip, rate="30:1"), 25.0)
    assert isinstance(by_suffix, Y4mVideo) and by_suffix.frame_rate == 30.0 and len(by_suffix) == 2
    by_magic = cli.open_video(yuv_ref.write_y4m(str(tmp_path / "film.raw"), clip), 25.0, matrix="709", full_range=True)
    assert isinstance(by_magic, Y4mVideo) and (by_magic.matrix, by_magic.full_range) == ("709", True)
    assert _same_planes(by_magic.frame(1), clip[1])
    np.save(str(tmp_path / "a.npy"), np.zeros((2, 6, 10, 3), np.uint8))
    assert isinstance(cli.open_video(str(tmp_path / "a.npy"), 25.0), cli.NpyVideo)
    assert type(cli.open_video("synthetic:320x180x6:2:1:5", 25.0)).__name__ == "SyntheticVideo"


def test_cli_refuses_stdin_for_verbs_that_need_a_length(tmp_path, capsys):
    from pyannote_video_amd import cli
    with pytest.raises(SystemExit):
        cli.main(["shot", "-", str(tmp_path / "out.json")])
    assert "needs the length" in capsys.readouterr().err


# ---- the streaming source -------------------------------------------------------------------------------------------------------------

def test_stream_source_on_a_y4m_video_equals_the_npy_video(tmp_path):
    """the same frames as .y4m and as .npy through engine.StreamSource on the scripted context: same shot cuts, detection flags,
    tracks, and every staged frame released exactly once"""
    from pyannote_video_amd import engine
    from pyannote_video_amd.cli import NpyVideo
    from pyannote_video_amd.tracking_by_detection import TrackingByDetection, HipTrackers
    from pyannote_video_amd.y4m import Y4mVideo, YuvFrame
    from tests.test_engine import FakeContext, FakeDeviceFrame, make_video

    class OrderedRing(object):
        """frames arrive in video order: the k-th push is scenario frame k"""
        def __init__(self, ctx, kind, want):
            self.ctx, self.kind, self.want = ctx, kind, want
            ctx.rings.append(self)
            self.closed = False

        def push(self, frame):
            assert isinstance(frame, self.want)
            f = FakeDeviceFrame(self.ctx.script_of[len(self.ctx.pushed)])
            self.ctx.pushed.append(f)
            return f

        def close(self):
            self.closed = True

    class Ctx(FakeContext):
        def __init__(self, frames, dets):
            FakeContext.__init__(self, frames, dets)
            self.rings, self.pushed = [], []

        def ingest_ring(self, h, w, depth=8):
            return OrderedRing(self, ("rgb", h, w), np.ndarray)

        def ingest_ring_yuv(self, h, w, layout="420", matrix="601", full_range=False, depth=8):
            return OrderedRing(self, ("yuv", h, w, layout, matrix, full_range), YuvFrame)

    frames, dets, times, shots = make_video(5, n_shots=3, n=12)
    h, w = frames[0].shape[:2]
    clip = [yuv_ref.noise_planes(h, w, "420", i) for i in range(len(frames))]
    y4m = yuv_ref.write_y4m(str(tmp_path / "a.y4m"), clip)
    np.save(str(tmp_path / "a.npy"), np.stack([yuv_ref.to_rgb(*p) for p in clip]))

    def run(video, every):
        ctx = Ctx(frames, dets)
        tbd = TrackingByDetection(detect_func=None, track_min_overlap_ratio=0.5, track_max_gap=1.0, trackers=HipTrackers(ctx))
        job = engine.VideoJob(ctx, w, h, extract=False)
        seen = []

        class Tap(engine.StreamSource):
            def __iter__(self):
                for item in engine.StreamSource.__iter__(self):
                    if isinstance(item, engine.ShotInput):
                        seen.append((item.base, [t for t, _ in item.cache], list(item.flags), item.owned))
                    yield item
        src = Tap(ctx, [(job, video, shots, every, None)])
        try:
            engine.Engine(ctx, tbd, detect_batch_size=5).run(src, HipTrackers(ctx))
        finally:
            src.close()
        assert len(ctx.pushed) == len(frames) and all(f.released for f in ctx.pushed)
        assert len(ctx.rings) == 1 and ctx.rings[0].closed
        return seen, job.tracks, ctx.rings[0].kind

    for every in (1, 3):
        cuts_y, tracks_y, kind_y = run(Y4mVideo(y4m), every)
        cuts_n, tracks_n, kind_n = run(NpyVideo(str(tmp_path / "a.npy"), 25.0), every)
        assert kind_y == ("yuv", h, w, "420", "601", False) and kind_n == ("rgb", h, w)
        assert cuts_y == cuts_n and len(cuts_y) == 3 and all(c[3] for c in cuts_y)
        assert json.dumps(tracks_y, default=str) == json.dumps(tracks_n, default=str) and len(tracks_y) > 0
