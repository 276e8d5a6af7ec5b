"""GPU: csrc/shot.hip (shot_convert_k, shot_pair_k, the host's farneback_plan) equals the oracle on every entry of the edge-case table
(tests/shot_cases.py; tests/test_shot_edge_cases.py proves on the CPU what the table reaches) -- no entry skipped or filtered: gray bytes
equal, flows equal as BIT PATTERNS (uint32 views: a sign of zero or a NaN cannot hide), differences equal as float64.  Beyond the table:
more pairs in one call than the card has compute units, the optional outputs on and off, calls of one and two frames, the order of calls
on the shared scratch buffer, the chunks of structure.Shot, frames staged ahead or brought by the YUV ring, and what the call refuses.
Reference: pyannote/video/structure/shot.py:71-117."""
import numpy as np
import pytest

import shot_cases as sc

pytestmark = pytest.mark.gpu

CHUNK = 64                      # frames per call on the table's long cases (even: the table's pairs are frames (2 i, 2 i + 1))


@pytest.fixture(scope="module")
def tables():
    from pyannote_video_amd import structure
    return structure.shot_tables()


@pytest.fixture(scope="module")
def own(model_paths):
    """a second context: its scratch buffer starts empty and sees another order of calls than the session's"""
    from pyannote_video_amd.runtime import Context
    c = Context(device=0, landmarks=model_paths[0])
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_flow(got, want, what):
    bad = np.flatnonzero((_bits(got) != _bits(want)).reshape(len(got), -1).any(axis=1))
    assert bad.size == 0, (what, "pairs", bad[:8].tolist(), "of", len(got))


def _run_case(ctx, c, tables):
    """the library on one table entry -> (gray [2 p], flow [p], dfd [p]): the table's pairs out of calls of at most CHUNK frames"""
    frames = c.frames()
    gray, flow, dfd = [], [], []
    for i0 in range(0, len(frames), CHUNK):
        d, g, f = ctx.shot_dfd(frames[i0:i0 + CHUNK], c.ow, c.oh, tables, want_gray=True, want_flow=True)
        gray.append(g); flow.append(f[0::2]); dfd.append(d[0::2])
    return np.concatenate(gray), np.concatenate(flow), np.concatenate(dfd)


@pytest.mark.parametrize("case", sc.cases(), ids=repr)
def test_table_entry_equals_the_oracle_bit_for_bit(ctx, oracle, tables, case):
    ref = sc.oracle_results(case, oracle, tables)
    gray, flow, dfd = _run_case(ctx, case, tables)
    assert gray.shape == ref["gray"].shape and np.array_equal(gray, ref["gray"])
    assert flow.shape == ref["flow"].shape and flow.dtype == np.float32
    _same_flow(flow, ref["flow"], case)
    print(case, "pairs", len(dfd), "largest |flow|", float(np.abs(flow).max()), "dfd", float(dfd.min()), "..", float(dfd.max()))
    assert dfd.dtype == np.float64 and dfd.tolist() == ref["dfd"].tolist()


# ---- many pairs in one call: more workgroups than compute units, every pair different
def _many_frames(ow, oh, n):
    """n different frames: noise, every third one a diagonal stripe or ramp pattern of its own phase"""
    frames = []
    for i in range(n):
        if i % 3 == 2:
            g = (sc.diag_stripes if i % 2 else sc.diag_ramp)(1 - 2 * ((i // 3) % 2), 2 + i % 7)(ow, oh)
            g[:3, :3] = sc.noise(100 + i)(3, 3)                    # (patterns of one period coincide: a mark of its own)
        else:
            g = sc.noise(100 + i)(ow, oh)
        frames.append(sc.rgb_of(g))
    return frames


@pytest.fixture(scope="module")
def many(oracle, tables):
    """(frames, reference) per geometry: 12 x 12 (no coarser level) and 64 x 64 (one: both flow buffers and the full-size float image
    are in use, up to the last float of a pair's scratch)"""
    out = {}
    for ow, oh, n in ((12, 12, 321), (64, 64, 301)):
        frames = _many_frames(ow, oh, n)
        gray = np.stack([f[:, :, 0] for f in frames])
        assert len(set(g.tobytes() for g in gray)) == n
        flow = np.stack(sc.threaded(lambda i: oracle.farneback(gray[i], gray[i + 1], tables), range(n - 1)))
        dfd = np.array([oracle.shot_dfd_from_flow(gray[i], gray[i + 1], flow[i]) for i in range(n - 1)])
        out[(ow, oh)] = (frames, dict(gray=gray, flow=flow, dfd=dfd))
    return out


@pytest.mark.parametrize("size", [(12, 12), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_many_pairs_in_one_call(ctx, many, tables, size):
    frames, ref = many[size]
    ow, oh = size
    assert len(frames) - 1 >= 300
    dfd, gray, flow = ctx.shot_dfd(frames, ow, oh, tables, want_gray=True, want_flow=True)
    assert np.array_equal(gray, ref["gray"])
    _same_flow(flow, ref["flow"], size)
    assert dfd.tolist() == ref["dfd"].tolist()
    assert len(set(dfd.tolist())) > 250                             # (the pairs differ: a pair reading its neighbour's scratch shows)
    # the same call without the optional outputs, each on its own
    d = ctx.shot_dfd(frames, ow, oh, tables)
    assert isinstance(d, np.ndarray) and d.tolist() == ref["dfd"].tolist()
    d, g = ctx.shot_dfd(frames, ow, oh, tables, want_gray=True)
    assert d.tolist() == ref["dfd"].tolist() and np.array_equal(g, ref["gray"])
    d, f = ctx.shot_dfd(frames, ow, oh, tables, want_flow=True)
    assert d.tolist() == ref["dfd"].tolist()
    _same_flow(f, ref["flow"], size)


def test_calls_of_one_and_two_frames(ctx, oracle, tables):
    c = sc.case("convert_down_noninteger")
    ref = sc.oracle_results(c, oracle, tables)
    frames = c.frames()
    for want_flow in (False, True):                                  # n = 1: gray only; there is no pair, no difference, no flow
        out = ctx.shot_dfd(frames[:1], c.ow, c.oh, tables, want_gray=True, want_flow=want_flow)
        assert out[0].shape == (0,) and np.array_equal(out[1], ref["gray"][:1])
        assert not want_flow or out[2].shape == (0, c.oh, c.ow, 2)
    assert ctx.shot_dfd(frames[:1], c.ow, c.oh, tables).shape == (0,)
    dfd, gray, flow = ctx.shot_dfd(frames[:2], c.ow, c.oh, tables, want_gray=True, want_flow=True)
    assert np.array_equal(gray, ref["gray"][:2]) and dfd.tolist() == ref["dfd"][:1].tolist()
    _same_flow(flow, ref["flow"][:1], "n = 2")
    assert ctx.shot_dfd(frames[:2], c.ow, c.oh, tables).tolist() == ref["dfd"][:1].tolist()


def _bytes_of(ctx, c, tables):
    gray, flow, dfd = _run_case(ctx, c, tables)
    return gray.tobytes() + flow.tobytes() + dfd.tobytes()


def test_results_do_not_depend_on_what_ran_before(ctx, own, oracle, tables, small_video, model_paths):
    """`s_misc` is one scratch buffer, carved anew by every call and shared with other subsystems: the kernels read nothing they have
    not written.  Largest geometry, smallest, largest again; the other order on a context of its own; then after detector, tracker and
    landmark work (the landmarks carve the same buffer)."""
    big, small = sc.case("content_257x259"), sc.case("content_12x12")
    a = [_bytes_of(ctx, c, tables) for c in (big, small, big)]
    b = [_bytes_of(own, c, tables) for c in (small, big, small)]
    assert a[0] == a[2] == b[1] and a[1] == b[0] == b[2]
    frame, nxt = small_video.frame(0), small_video.frame(1)
    boxes = [tuple(float(v) for v in bx[1:]) for bx in small_video.face_boxes(0)]
    assert ctx.detect(frame) is not None
    trks = ctx.tracker_create_many(len(boxes))
    ctx.tracker_start_many(trks, [frame] * len(boxes), boxes)
    ctx.tracker_update_many(trks, [nxt] * len(boxes))
    ctx.tracker_destroy_many(trks)
    ctx.landmarks([frame] * len(boxes), [tuple(int(v) for v in bx) for bx in boxes])
    assert _bytes_of(ctx, small, tables) == a[1] and _bytes_of(ctx, big, tables) == a[0]
    # (and the bytes are the oracle's)
    ref = sc.oracle_results(big, oracle, tables)
    assert a[0] == ref["gray"].tobytes() + ref["flow"].tobytes() + ref["dfd"].tobytes()


class _Clip(object):
    """the slice of the reference's Video that Shot touches"""

    def __init__(self, frames, fps=25.0):
        self.frames, self.frame_rate = frames, fps
        self._size = (frames[0].shape[1], frames[0].shape[0])
        self.step = 1.0 / fps
        self.start, self.end = 0.0, len(frames) / fps

    def __iter__(self):
        for i, f in enumerate(self.frames):
            yield i / self.frame_rate, f


def _striped_clip(side=64):
    """three shots of four square frames (Shot(height=side) keeps them as they are; one coarser level): a moving texture, diagonal
    stripes against black and against each other (the flow leaves the image by thousands of pixels), noise"""
    shots = [[sc.texture(dx=2 * i, dy=i)(side, side) for i in range(4)],
             [sc.diag_stripes(-1, 3)(side, side), sc.const(0)(side, side), sc.diag_stripes(-1, 6)(side, side), sc.diag_stripes(-1, 3)(side, side)],
             [sc.noise(40 + i)(side, side) for i in range(4)]]
    return [sc.rgb_of(g) for shot in shots for g in shot]


def test_chunks_of_shot_equal_one_call(ctx, oracle, tables):
    from pyannote_video_amd import structure
    frames = _striped_clip()
    n = len(frames)
    ow, oh = 64, 64
    whole = ctx.shot_dfd(frames, ow, oh, tables)
    small = [oracle.shot_convert(f, ow, oh) for f in frames]
    flows = [oracle.farneback(small[i], small[i + 1], tables) for i in range(n - 1)]
    assert whole.tolist() == [oracle.shot_dfd_from_flow(small[i], small[i + 1], flows[i]) for i in range(n - 1)]
    assert max(float(np.abs(f).max()) for f in flows[4:7]) > 1000      # the striped shot: flows far beyond the image
    for chunk in (2, 3, n - 1, n, n + 1):
        shot = structure.Shot(_Clip(frames), height=64, context=0.2, threshold=1.0, ctx=ctx, chunk=chunk)
        assert shot._resize == (ow, oh)
        pairs = list(shot.iter_dfd())
        assert [t for t, _ in pairs] == [i / 25.0 for i in range(1, n)], chunk
        assert [d for _, d in pairs] == whole.tolist(), chunk


def test_frames_staged_ahead_and_from_the_yuv_ring(ctx, tables):
    import yuv_ref
    from pyannote_video_amd.y4m import YuvFrame
    w, h, ow, oh = 70, 46, 33, 21
    clip = [yuv_ref.from_rgb(sc.colour_frame(w, h, 20 + i, smooth=i % 2 == 0), "420") for i in range(5)]
    frames = [np.ascontiguousarray(yuv_ref.to_rgb(*p)) for p in clip]
    want = ctx.shot_dfd(frames, ow, oh, tables, want_gray=True, want_flow=True)

    def same(got):
        return all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    uploaded = [ctx.upload(f) for f in frames]                        # frames in HBM before the call
    assert same(ctx.shot_dfd(uploaded, ow, oh, tables, want_gray=True, want_flow=True))
    staged = [ctx.stage(f) for f in frames]                           # ... staged through the cache ...
    assert same(ctx.shot_dfd(staged, ow, oh, tables, want_gray=True, want_flow=True))
    assert same(ctx.shot_dfd(ctx.frame_handles(staged), ow, oh, tables, want_gray=True, want_flow=True))     # ... or named by handle
    ring = ctx.ingest_ring_yuv(h, w, layout="420", depth=8)
    try:
        ringed = [ring.push(YuvFrame(*p, layout="420")) for p in clip]
        assert same(ctx.shot_dfd(ringed, ow, oh, tables, want_gray=True, want_flow=True))
        assert same(ctx.shot_dfd([YuvFrame(*p, layout="420") for p in clip], ow, oh, tables, want_gray=True, want_flow=True))
    finally:
        ring.close()
    for f in uploaded:
        f.release()


def test_refused_calls_raise_and_the_context_goes_on(ctx, oracle, tables):
    from pyannote_video_amd._lib import PvfError
    c = sc.case("convert_identity")
    frames = c.frames()[:2]
    for ow, oh in ((11, 12), (12, 11), (11, 11)):
        with pytest.raises(PvfError):
            ctx.shot_dfd(frames, ow, oh, tables)
    with pytest.raises(PvfError):                                    # frames of two sizes
        ctx.shot_dfd([frames[0], np.ascontiguousarray(frames[1][:-1])], c.ow, c.oh, tables)
    with pytest.raises(PvfError):                                    # no frame at all
        ctx.shot_dfd([], c.ow, c.oh, tables)
    for bad in (tables[:21], np.concatenate([tables, tables[:1]]), np.zeros((2, 11), np.float32), np.zeros(0, np.float32)):
        with pytest.raises(ValueError):
            ctx.shot_dfd(frames, c.ow, c.oh, bad)
    ref = sc.oracle_results(c, oracle, tables)
    dfd, gray, flow = ctx.shot_dfd(frames, c.ow, c.oh, tables, want_gray=True, want_flow=True)
    assert np.array_equal(gray, ref["gray"][:2]) and dfd.tolist() == ref["dfd"][:1].tolist()
    _same_flow(flow, ref["flow"][:1], "after the refusals")
