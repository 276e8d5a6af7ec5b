"""Shot threading, CPU side: the ORB restatement (tests/orb_ref.py), the host logic of structure.Thread (pairs, union-find, Tarjan,
labels, smoothing, scenes), the `thread` verb's arguments, and the reference's own thread.py run verbatim where a checkout is named
(PVF_REFERENCE) -- its results on the clip of tests/thread_clip.py are recorded in tests/golden/reference_thread_pins.json."""
import json
import os

import numpy as np
import pytest

import orb_ref
import refhost_thread
import thread_clip

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_thread_pins.json")


@pytest.fixture(scope="module")
def pins():
    with open(PINS) as f:
        return json.load(f)


def _smooth_noise(seed, n=201):
    from scipy.ndimage import gaussian_filter
    img = gaussian_filter(np.random.default_rng(seed).random((n, n)), 2.5)
    return ((img - img.min()) / (img.max() - img.min()) * 255).astype(np.uint8)


def test_finds_square_corners():
    # flat squares tie their corner scores with the diagonal neighbour (strict suppression drops both): a little noise separates them
    g = np.full((355, 200), 40, np.int32)
    corners = set()
    for y, x in ((60, 50), (60, 120), (160, 60), (250, 110)):
        g[y:y + 30, x:x + 30] = 220
        corners |= {(y, x), (y, x + 29), (y + 29, x), (y + 29, x + 29)}
    g = (g + np.random.default_rng(0).integers(-6, 7, g.shape)).astype(np.uint8)
    kp, desc = orb_ref.orb_gray(g)
    lv0 = kp[kp[:, 2] == 0]
    assert len(lv0) >= len(corners)
    for y, x in corners:
        assert np.min(np.abs(lv0[:, 1] - y) + np.abs(lv0[:, 0] - x)) <= 2, (y, x)
    assert desc.shape == (len(kp), 32)


def test_rotated_patch_angle_and_descriptor():
    img = _smooth_noise(2)
    c = 100
    a0 = orb_ref.ic_angle(img, c, c)
    rot = np.rot90(img)                                      # a quarter turn: the centroid direction turns by exactly 90 degrees
    a1 = orb_ref.ic_angle(rot, c, c)
    assert abs(((a0 - a1) % 360) - 90) < 0.05
    d0 = orb_ref.descriptor(orb_ref.blur(img), c, c, a0)
    d1 = orb_ref.descriptor(orb_ref.blur(np.ascontiguousarray(rot)), c, c, a1)
    assert orb_ref.hamming(d0[None], d1[None])[0, 0] <= 8
    # an arbitrary angle through bilinear rotation: the angle follows, the descriptor stays close
    from scipy.ndimage import rotate
    r30 = np.clip(rotate(img.astype(np.float64), 30, reshape=False, order=1), 0, 255).round().astype(np.uint8)
    a2 = orb_ref.ic_angle(r30, c, c)
    assert abs(((a0 - a2) % 360) - 30) < 3
    d2 = orb_ref.descriptor(orb_ref.blur(r30), c, c, a2)
    assert orb_ref.hamming(d0[None], d2[None])[0, 0] <= 40


def test_level_quota_and_sizes():
    q = orb_ref.level_quota()
    assert sum(q) == 500 and q == sorted(q, reverse=True) and len(q) == 8
    assert orb_ref.level_sizes(200, 355)[:3] == [(200, 355), (167, 296), (139, 247)]
    assert orb_ref.thread_size(1920, 1080) == (200, 355)
    assert orb_ref.gaussian7() == [18, 34, 48, 56, 48, 34, 18] and sum(orb_ref.gaussian7()) == 256
    assert orb_ref.umax() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]


def test_retain_best_keeps_ties():
    r = np.array([5, 4, 4, 4, 1, 4], np.float32)
    assert orb_ref.retain_best(r, 2).tolist() == [True, True, True, True, False, True]
    assert orb_ref.retain_best(r, 6).all() and orb_ref.retain_best(r, 1).tolist() == [True] + [False] * 5


def test_lookahead_pairs(pins):
    from pyannote_video_amd.structure import lookahead_pairs
    for key, want in pins["product_lookahead"].items():
        n, la = (int(v) for v in key.split(","))
        assert sorted(lookahead_pairs(n, la)) == sorted(tuple(p) for p in want), key
    for n in range(0, 40, 3):
        for la in (1, 2, 5, 24, 50):
            assert set(lookahead_pairs(n, la)) == {(i, k) for i in range(n) for k in range(n) if 1 <= k - i <= la}


def test_ratio_rule_integer_form():
    for d1 in range(257):
        for d2 in range(d1, 257):
            assert (10 * d1 < 7 * d2) == (d1 < 0.7 * d2)


def test_match_count_rule():
    a = np.zeros((3, 32), np.uint8)
    assert orb_ref.match_count(a[:1], a) == 0 and orb_ref.match_count(a, a[:1]) == 0 and orb_ref.match_count(None, a) == 0
    b = np.zeros((2, 32), np.uint8); b[1, :4] = 0xFF                 # distances 0 and 32 from every zero row
    assert orb_ref.match_count(a, b) == 3
    assert orb_ref.match_count(a, np.zeros((2, 32), np.uint8)) == 0      # d1 == d2: no match


def test_components_against_networkx():
    nx = pytest.importorskip("networkx")
    from pyannote_video_amd.structure import biconnected_components, connected_components
    rng = np.random.default_rng(0)
    for trial in range(60):
        n = int(rng.integers(1, 30))
        edges = [tuple(int(v) for v in rng.integers(0, n, 2)) for _ in range(int(rng.integers(0, 2 * n)))]
        edges = [(a, b) for a, b in edges if a != b]
        g = nx.Graph(); g.add_nodes_from(range(n)); g.add_edges_from(edges)
        assert connected_components(n, edges) == sorted(sorted(c) for c in nx.connected_components(g))
        assert sorted(sorted(c) for c in biconnected_components(edges)) == sorted(sorted(c) for c in nx.biconnected_components(g))


def _host_from_counts(shots, pairs, counts, min_match=20):
    from pyannote_video_amd import structure
    segs = [structure.Segment(a, b) for a, b in shots]
    threads = structure.thread_labels(segs, [p for p, c in zip(pairs, counts) if c > min_match])
    return threads, structure.thread_scenes(threads)


def _clip_counts(pins):
    from pyannote_video_amd.structure import lookahead_pairs
    frames, shots, fps = thread_clip.make_clip(**pins["clip"])
    collar = 10. / fps
    pairs = lookahead_pairs(len(shots), pins["lookahead"])
    orb = {}

    def desc(t):
        i = int(fps * t + 1e-5)
        if i not in orb:
            orb[i] = orb_ref.orb_frame(frames[i])[1]
        return orb[i]
    counts = [orb_ref.match_count(desc(shots[i][1] - collar), desc(shots[k][0] + collar)) for i, k in pairs]
    return frames, shots, fps, pairs, counts


def test_host_logic_reproduces_reference_pins(pins):
    _, shots, _, pairs, counts = _clip_counts(pins)
    assert [[i, k, c] for (i, k), c in zip(pairs, counts) if c > pins["min_match"]] == pins["edges"]
    threads, scenes = _host_from_counts(shots, pairs, counts, pins["min_match"])
    assert threads.for_json()["content"] == pins["threads"]["content"]
    assert scenes.for_json()["content"] == pins["scenes"]["content"]


@pytest.mark.skipif(not refhost_thread.have_reference(), reason="PVF_REFERENCE does not name a pyannote-video checkout")
def test_reference_verbatim_equals_host_logic(pins):
    frames, shots, fps, pairs, counts = _clip_counts(pins)
    threads, scenes, edges = refhost_thread.run_reference(thread_clip.ClipVideo(frames, fps), shots)
    mine_t, mine_s = _host_from_counts(shots, pairs, counts)
    assert threads.for_json() == mine_t.for_json() and scenes.for_json() == mine_s.for_json()
    assert edges == {p: c for p, c in zip(pairs, counts) if c > 20}


def test_scenes_merge_intertwined_threads():
    from pyannote_video_amd import structure
    segs = [structure.Segment(i, i + 1) for i in range(7)]
    # A B A B C D C: the A/B run becomes one scene, C/D another
    threads = structure.thread_labels(segs, [(0, 2), (1, 3), (4, 6)])
    assert [l for _, _, l in threads.itertracks(yield_label=True)] == list("ABABCDC")
    scenes = structure.thread_scenes(threads)
    assert [l for _, _, l in scenes.itertracks(yield_label=True)] == list("AAAACCC")


def test_annotation_smooth_and_json():
    from pyannote_video_amd._core import Annotation, Segment
    a = Annotation()
    for i, l in enumerate("AABAA"):
        a[Segment(i, i + 1)] = l
    s = a.smooth()
    assert [(seg.start, seg.end, l) for seg, _, l in s.itertracks(yield_label=True)] == [(0, 2, "A"), (2, 3, "B"), (3, 5, "A")]
    assert Annotation.from_json(json.loads(json.dumps(s.for_json()))) == s
    assert s.subset(["B"]).labels() == ["B"] and len(s.subset(["A"])) == 2


def test_cli_thread_arguments(monkeypatch):
    from pyannote_video_amd import cli
    seen = {}
    monkeypatch.setattr(cli, "thread", lambda video, shot, output, **kw: seen.update(shot=shot, output=output, **kw))
    monkeypatch.setattr(cli, "open_video", lambda spec, fps: spec)
    assert cli.main(["thread", "v.npy", "s.json", "o.json"]) == 0
    assert seen == {"shot": "s.json", "output": "o.json", "min_match": 20, "lookahead": 24, "ctx": None}
    cli.main(["thread", "--min-match", "7", "--lookahead", "3", "v.npy", "s.json", "o.json"])
    assert seen["min_match"] == 7 and seen["lookahead"] == 3


def test_thread_frame_index_rule():
    from pyannote_video_amd import structure
    frames, shots, fps = thread_clip.make_clip(frames_per_shot=2, setups="AB")
    th = structure.Thread.__new__(structure.Thread)
    th.video = thread_clip.ClipVideo(frames, fps)
    assert th._frame_index(0.0) == 0 and th._frame_index(3 / fps) == 3 and th._frame_index(4 / fps) is None
    assert th._frame_index(-0.5 / fps) == 0 and th._frame_index(-1.5 / fps) is None
    assert th._frame_index(0.12) == 3                       # 25 * 0.12 = 2.9999999999999996: + 1e-5 then truncation


# ---- the resize both device copies of INTER_LINEAR implement (ingest.hip's pvf_frame_resize, orb.hip's level 0): orb_ref's
# restatement == the oracle's, byte for byte, over the GPU tests' geometry table (upscales, odd sizes, one axis up and one down)
RESIZE_CASES = [((1440, 1080), (200, 266)), ((1080, 1920), (200, 112)), ((160, 120), (200, 266)), ((200, 200), (200, 200)),
                ((853, 479), (200, 356)), ((3000, 500), (200, 1200)), ((4095, 200), (200, 4095)), ((63, 200), (200, 63)),
                ((1920, 1080), (300, 533)), ((640, 360), (800, 450)), ((640, 360), (1280, 720)), ((640, 360), (641, 359)),
                ((640, 360), (700, 300)), ((97, 55), (640, 360)), ((1, 1), (5, 3)), ((2, 3), (7, 9)), ((3, 2), (200, 100))]


@pytest.mark.parametrize("src,dst", RESIZE_CASES, ids=["%dx%d-%dx%d" % (s + d) for s, d in RESIZE_CASES])
def test_resize_restatements_agree(oracle, src, dst):
    img = np.random.default_rng(src[0] * 7 + dst[1]).integers(0, 256, (src[1], src[0], 3), dtype=np.uint8)
    got = orb_ref.resize_linear_rgb(img, *dst)
    assert got.shape == (dst[1], dst[0], 3)
    np.testing.assert_array_equal(got, oracle.cv_resize(img, *dst))


# ---- structure.Thread over a CPU stand-in of the library: Context.orb_extract's cap handling and Thread's chunks
def _dot_grid(spacing, size=200):
    g = np.full((size, size, 3), 40, np.uint8)
    g[::spacing, ::spacing] = 220
    return g


class _OrbStandIn(object):
    """stands in for libpvface's two ORB entry points on the CPU (orb_ref): Context._orb_extract raises as pvf_orb_extract does when a
    frame has more keypoints than the cap (OrbCapError carrying the cap that fits), and orb_match_counts matches the resident sets of
    the last successful call or the host descriptors it is given.  Context's own orb_extract runs on top of it."""

    def __new__(cls):
        from pyannote_video_amd.runtime import Context
        stand_in = type("OrbStandInContext", (Context,), {k: v for k, v in vars(cls).items() if k.startswith(("_orb", "orb"))})
        obj = Context.__new__(stand_in)
        obj._h, obj.caps, obj.matched, obj._resident, obj._memo = None, [], [], None, {}
        return obj

    def _orb_extract(self, frames, width, height, cap):
        from pyannote_video_amd._lib import OrbCapError
        self.caps.append(cap)
        self._resident = None
        refs = []
        for f in frames:
            key = (f.tobytes(), width, height)
            if key not in self._memo:
                self._memo[key] = orb_ref.orb_gray(orb_ref.gray(orb_ref.resize_linear_rgb(f, width, height)))
            refs.append(self._memo[key])
        counts = np.array([len(k) for k, _ in refs], np.int32)
        if counts.max() > cap:
            raise OrbCapError("orb: frame %d has %d keypoints, more than cap = %d" % (counts.argmax(), counts.max(), cap), counts.max())
        kp = np.zeros((len(frames), cap, 6), np.float32)
        desc = np.zeros((len(frames), cap, 32), np.uint8)
        for i, (k, d) in enumerate(refs):
            kp[i, :len(k)] = k
            desc[i, :len(d)] = d
        self._resident = (desc, counts)
        return counts, kp, desc

    def orb_match_counts(self, pairs, descriptors=None, rows=None):
        if descriptors is None:
            descriptors, rows = self._resident
        self.matched.append((descriptors, rows))
        return np.array([orb_ref.match_count(descriptors[a, :rows[a]], descriptors[b, :rows[b]]) for a, b in pairs], np.int32)


def _grid_clip(fps=25.0, per=12):
    """200 x 200 shots A B G A C, G a dot grid: its frames need more than the default 1024 rows"""
    tex, _, _ = thread_clip.make_clip(width=200, height=200, frames_per_shot=per, setups="ABAC", frame_rate=fps)
    frames = np.concatenate([tex[:2 * per], np.stack([_dot_grid(4)] * per), tex[2 * per:]])
    return frames, [(i * per / fps, (i + 1) * per / fps) for i in range(5)], fps


def test_thread_chunks_with_different_caps():
    from pyannote_video_amd import structure
    frames, shots, fps = _grid_clip()
    video = thread_clip.ClipVideo(frames, fps)
    segs = [structure.Segment(a, b) for a, b in shots]
    grid_rows = len(orb_ref.orb_gray(orb_ref.gray(_dot_grid(4)))[0])
    assert grid_rows > 1024
    one = _OrbStandIn()
    _, pairs, counts = structure.Thread(video, shot=segs, lookahead=24, ctx=one).match_counts()
    assert one.caps == [1024, grid_rows]                                  # the default cap, then once more with the cap that fits
    # needed frames 2 14 | 22 26 | 34 38 | 46 58 in chunks of 2, the grid's at 26 and 34: caps 1024, 1024 then more, 1024 then more, 1024
    chunked = _OrbStandIn()
    chunked._memo = one._memo
    _, _, got = structure.Thread(video, shot=segs, lookahead=24, ctx=chunked, chunk=2).match_counts()
    assert chunked.caps == [1024, 1024, grid_rows, 1024, grid_rows, 1024]
    np.testing.assert_array_equal(got, counts)
    desc, rows = chunked.matched[-1]
    assert desc.shape[1] == grid_rows                                      # every set padded to the widest chunk
    needed = [2, 14, 22, 26, 34, 38, 46, 58]
    for j, f in enumerate(needed):
        _, d = one._memo[(np.ascontiguousarray(frames[f]).tobytes(), 200, 200)]
        assert rows[j] == len(d)
        np.testing.assert_array_equal(desc[j, :rows[j]], d)
        assert not desc[j, rows[j]:].any()
    # both equal the restatement of thread.py's pairs
    collar = 10. / fps
    ref = [orb_ref.match_count(one._memo[(np.ascontiguousarray(frames[int(fps * (shots[i][1] - collar) + 1e-5)]).tobytes(), 200, 200)][1],
                               one._memo[(np.ascontiguousarray(frames[int(fps * (shots[k][0] + collar) + 1e-5)]).tobytes(), 200, 200)][1])
           for i, k in pairs]
    np.testing.assert_array_equal(counts, ref)


def test_orb_cap_explicit_is_strict_and_limit_is_clear():
    from pyannote_video_amd import structure
    from pyannote_video_amd._lib import OrbCapError
    frames, shots, fps = _grid_clip()
    video = thread_clip.ClipVideo(frames, fps)
    segs = [structure.Segment(a, b) for a, b in shots]
    ctx = _OrbStandIn()
    with pytest.raises(OrbCapError, match="more than cap = 1024"):
        structure.Thread(video, shot=segs, lookahead=24, ctx=ctx, cap=1024).match_counts()
    assert ctx.caps == [1024]                                              # a given cap: no second call
    grid = _dot_grid(4)
    n = ctx.orb_extract([grid], 200, 200)[0][0]
    with pytest.raises(OrbCapError) as e:
        ctx.orb_extract([grid, grid], 200, 200, cap=n - 1)
    assert e.value.needed == n
    ctx.ORB_CAP_MAX = n - 1                                                # a frame past the library's limit: one clear error
    ctx.caps = []
    with pytest.raises(OrbCapError, match="%d keypoints .* more than the %d rows" % (n, n - 1)):
        ctx.orb_extract([grid], 200, 200)
    assert ctx.caps == [1024]
