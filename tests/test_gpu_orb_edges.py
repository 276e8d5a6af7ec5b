"""Shot threading on the GPU (csrc/orb.hip) at the edges the thread_clip geometry never reaches: pyramids of 0 to 8 levels, upscaling at
level 0, the largest side the candidate packing admits, content that stresses the selection (noise, saturated dots, Harris ties past the
quota and past the default cap, no corners, corners on the image border), batches longer than one launch chunk, the matcher's query and
train blocks, and the keypoint cap.  Extraction is compared with tests/orb_ref.py bit for bit (tests/orb_check.py), matching with
orb_ref.match_count."""
import json

import numpy as np
import pytest

import orb_check
import orb_ref
import thread_clip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gctx():
    from pyannote_video_amd.runtime import Context
    c = Context(device=0)
    yield c
    c.close()


def _textured(w, h, seed):
    f, _, _ = thread_clip.make_clip(width=w, height=h, frames_per_shot=1, setups="A", seed=seed)
    return f[0]


def _rgb(g):
    return np.ascontiguousarray(np.repeat(np.asarray(g, np.uint8)[:, :, None], 3, 2))


def _dot_grid(spacing, size=200, lo=40, hi=220):
    """one-pixel dots every `spacing` pixels: every dot at a level has the same Harris response"""
    g = np.full((size, size), lo, np.uint8)
    g[::spacing, ::spacing] = hi
    return _rgb(g)


def _levels_seen(counts, kp):
    return max((int(kp[i, :counts[i], 2].max()) + 1 for i in range(len(counts)) if counts[i]), default=0)


# ---- a. geometry: (input w, h, small-image height argument, small image, levels, levels that the two frames' keypoints reach)
GEOMETRY = [
    (1440, 1080, 200, (200, 266), 7, 7),         # 4:3
    (1080, 1920, 200, (200, 112), 4, 4),         # portrait: fewer levels
    (160, 120, 200, (200, 266), 7, 7),           # upscale on both axes: the clamp branches of the INTER_LINEAR table
    (200, 200, 200, (200, 200), 7, 6),           # identity level 0 (zero fractions)
    (853, 479, 200, (200, 356), 7, 7),           # odd sizes
    (3000, 500, 200, (200, 1200), 7, 7),         # tall small image
    (4095, 200, 200, (200, 4095), 7, 7),         # the largest side the 12-bit candidate packing admits
    (63, 200, 200, (200, 63), 1, 1),             # one interior row
    (62, 200, 200, (200, 62), 0, 0),             # no level at all
    (1920, 1080, 300, (300, 533), 8, 8),         # all 8 levels: level 7 takes the rest of the 500 (31)
]


@pytest.mark.parametrize("w,h,height,small,nlev,seen", GEOMETRY, ids=["%dx%d@%d" % g[:3] for g in GEOMETRY])
def test_extract_geometry(gctx, w, h, height, small, nlev, seen):
    assert orb_ref.thread_size(w, h, height) == small
    assert orb_check.levels(*small) == nlev
    frames = [_textured(w, h, seed=3), _textured(w, h, seed=4)]
    counts, kp, _, refs = orb_check.check_frames(gctx, frames, height=height)
    assert _levels_seen(counts, kp) == seen
    assert max((int(rk[:, 2].max()) + 1 for rk, _ in refs if len(rk)), default=0) == seen
    if nlev == 0:
        assert counts.tolist() == [0, 0]
        np.testing.assert_array_equal(gctx.orb_match_counts([(0, 1), (1, 0), (0, 0)]), [0, 0, 0])
    if nlev == 1:
        assert counts.max() >= 1
        for i in range(len(frames)):
            assert np.all(kp[i, :counts[i], 1] == 31)                   # the single interior row
    if nlev == 8:
        q = orb_ref.level_quota()
        assert q[7] == 31 and sum(q) == 500
        assert 0 < np.count_nonzero(kp[0, :counts[0], 2] == 7) <= q[7]


def test_extract_4096_refused(gctx):
    frames = [_textured(4096, 200, seed=3)]
    assert orb_ref.thread_size(4096, 200) == (200, 4096)
    from pyannote_video_amd._lib import PvfError
    gctx.orb_extract([_textured(480, 270, seed=1)], 200, 355)         # a valid result first: the refused call must drop it
    with pytest.raises(PvfError, match="4095"):
        gctx.orb_extract(frames, 200, 4096)
    with pytest.raises(PvfError, match="4095"):
        gctx.orb_extract(frames, 4096, 200)
    with pytest.raises(PvfError, match="no pvf_orb_extract result"):
        gctx.orb_match_counts([(0, 0)])


# ---- b. content
def test_noise_1080p(gctx):
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(2)]
    counts, _, _, _ = orb_check.check_frames(gctx, frames)
    ow, oh = orb_ref.thread_size(1920, 1080)
    lv0 = orb_ref.gray(orb_ref.resize_linear_rgb(frames[0], ow, oh))
    assert len(orb_ref.nms_candidates(orb_ref.fast_scores(lv0, lo=orb_ref.EDGE - 1), ow, oh)) > 3000    # thousands of candidates
    assert counts.min() > 300


def test_saturated_dots_reach_score_254(gctx):
    g = np.zeros((200, 200), np.uint8)
    g[:, 100:] = 255
    rng = np.random.default_rng(5)
    for _ in range(60):
        y, x = rng.integers(35, 165, 2)
        g[y, x] = 0 if g[y, x] else 255                                 # white dots on black, black dots on white
    counts, kp, _, _ = orb_check.check_frames(gctx, [_rgb(g)])
    assert counts[0] > 20 and kp[0, :counts[0], 3].max() == 254


@pytest.mark.parametrize("spacing", [5, 6])
def test_dot_grid_ties_past_the_quota(gctx, spacing):
    frame = _dot_grid(spacing)
    counts, kp, _, refs = orb_check.check_frames(gctx, [frame])
    lv0 = int(np.count_nonzero(refs[0][0][:, 2] == 0))
    assert lv0 > orb_ref.level_quota()[0] and counts[0] <= 1024         # ties kept, under the default cap
    assert kp.shape[1] == 1024


def test_dot_grid_past_the_default_cap(gctx):
    """the default call returns every tied keypoint of a frame that needs more than 1024 rows, bit for bit"""
    frame = _dot_grid(4)
    counts, kp, desc, refs = orb_check.check_frames(gctx, [frame])
    assert len(refs[0][0]) > 1024 and counts[0] == len(refs[0][0]) and kp.shape[1] == desc.shape[1] == counts[0]


def test_gradient_ramp_has_no_corners(gctx):
    ramp = np.tile(np.linspace(0, 255, 200).astype(np.uint8), (200, 1))
    counts, _, _, _ = orb_check.check_frames(gctx, [_rgb(ramp), _rgb(ramp.T.copy())])
    assert counts.tolist() == [0, 0]


def test_corners_on_the_image_border(gctx):
    """single-pixel corners on the 31-pixel border (kept) and one pixel past it (dropped), on all four sides"""
    g = np.full((200, 200), 60, np.uint8)
    kept = [(31, 100), (100, 31), (168, 60), (60, 168)]                  # (y, x): 31 <= x, y < 200 - 31
    dropped = [(30, 140), (140, 30), (169, 120), (120, 169)]
    for y, x in kept + dropped:
        g[y, x] = 230
    counts, kp, _, _ = orb_check.check_frames(gctx, [_rgb(g)])
    lv0 = {(int(y), int(x)) for x, y in kp[0, :counts[0], :2][kp[0, :counts[0], 2] == 0]}
    assert lv0 == set(kept)


# ---- c. batches
def _crops(n, w=480, h=270, pad=11, seed=21):
    """n distinct jittered crops of one scene"""
    scene = np.clip(thread_clip._scene(seed, h + 2 * pad, w + 2 * pad), 0, 255).astype(np.uint8)
    offs = [(dy, dx) for dy in range(2 * pad + 1) for dx in range(2 * pad + 1)]
    order = np.random.default_rng(seed).permutation(len(offs))[:n]
    return [np.ascontiguousarray(scene[offs[k][0]:offs[k][0] + h, offs[k][1]:offs[k][1] + w]) for k in order]


def test_batch_spans_two_chunks(gctx):
    ow, oh = orb_ref.thread_size(480, 270)
    chunk = orb_check.chunk_frames(ow, oh, 1024)
    frames = _crops(chunk + 30)
    assert chunk == 378 and len(frames) > chunk
    counts, kp, desc = gctx.orb_extract(frames, ow, oh)
    assert kp.shape[1] == 1024 and counts.min() > 100
    pairs = [(chunk - 1, chunk), (chunk, chunk - 1), (0, len(frames) - 1), (chunk - 2, chunk + 1), (chunk, chunk), (5, chunk + 7)]
    resident = gctx.orb_match_counts(pairs)                           # before the one-frame calls below replace the resident set
    host = gctx.orb_match_counts(pairs, desc, counts)
    np.testing.assert_array_equal(resident, host)
    np.testing.assert_array_equal(resident, [orb_ref.match_count(desc[a, :counts[a]], desc[b, :counts[b]]) for a, b in pairs])
    for i in (0, chunk - 1, chunk, len(frames) - 1):                  # both sides of the boundary and the last frame: orb_ref
        orb_check.assert_equal(counts[i:i + 1], kp[i:i + 1], desc[i:i + 1], [orb_check.reference(frames[i], ow, oh)])
    for i, f in enumerate(frames):                                   # every frame: its own one-frame extraction
        c1, k1, d1 = gctx.orb_extract([f], ow, oh)
        assert c1[0] == counts[i], i
        np.testing.assert_array_equal(k1[0, :c1[0]], kp[i, :counts[i]], err_msg=str(i))
        np.testing.assert_array_equal(d1[0, :c1[0]], desc[i, :counts[i]], err_msg=str(i))


def test_mixed_batch_packing(gctx):
    """a flat frame between textured ones and a frame past the default cap among them: every frame's rows at its own offset"""
    flat = np.full((200, 200, 3), 97, np.uint8)
    frames = [_textured(200, 200, seed=3), flat, _dot_grid(4), _textured(200, 200, seed=4), flat, _dot_grid(6)]
    counts, kp, desc, refs = orb_check.check_frames(gctx, frames)
    assert counts[1] == counts[4] == 0 and counts[2] > 1024 and kp.shape[1] == counts[2]
    pairs = [(a, b) for a in range(len(frames)) for b in range(len(frames))]
    got = gctx.orb_match_counts(pairs)
    np.testing.assert_array_equal(got, gctx.orb_match_counts(pairs, desc, counts))
    np.testing.assert_array_equal(got, [orb_ref.match_count(refs[a][1], refs[b][1]) for a, b in pairs])


# ---- d. the two device copies of INTER_LINEAR (pvf_frame_resize and orb.hip's level 0) agree
@pytest.mark.parametrize("w,h,size", [(1920, 1080, None), (160, 120, None), (853, 479, None), (640, 360, (211, 97))])
def test_level0_equals_device_resize(gctx, w, h, size):
    frame = _textured(w, h, seed=6)
    ow, oh = size or orb_ref.thread_size(w, h)
    small = gctx.resize(gctx.upload(frame), ow, oh)
    a = gctx.orb_extract([small], ow, oh)
    b = gctx.orb_extract([frame], ow, oh)
    assert a[0][0] == b[0][0] and a[0][0] > 0
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ---- e. matching edges: the 256-query blocks and the 1024-row train chunks
def _match_check(gctx, desc, rows, pairs):
    got = gctx.orb_match_counts(pairs, desc, rows)
    want = [orb_ref.match_count(desc[a, :rows[a]], desc[b, :rows[b]]) for a, b in pairs]
    np.testing.assert_array_equal(got, want)
    return got


def test_match_block_edges(gctx):
    rng = np.random.default_rng(3)
    na_list, nb_list = [0, 1, 2, 255, 256, 257], [1, 2, 1023, 1024, 1025, 2049]
    rows = np.array(na_list + nb_list, np.int32)
    cap = 2049
    desc = rng.integers(0, 256, (len(rows), cap, 32), dtype=np.uint8)
    desc[:len(na_list)] = desc[len(na_list) - 1]                     # every query set: the first na rows of one set
    q = desc[0, :257]
    for j, nb in enumerate(nb_list, len(na_list)):                   # near copies of the queries, spread over every train chunk
        at = rng.choice(nb, min(nb, 257), replace=False)
        desc[j, at] = q[:len(at)] ^ (rng.random((len(at), 32)) < 0.04).astype(np.uint8) * rng.integers(1, 256, (len(at), 32), dtype=np.uint8)
    pairs = [(a, b) for a in range(len(na_list)) for b in range(len(na_list), len(rows))]
    got = _match_check(gctx, desc, rows, pairs)
    assert got.max() > 200


def test_match_special_sets(gctx):
    rng = np.random.default_rng(4)
    cap = 300
    a = rng.integers(0, 256, (cap, 32), dtype=np.uint8)
    same = np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), cap, 0)
    eight = np.zeros((cap, 32), np.uint8)                             # every row 8 bits from the zero row
    eight[np.arange(cap), np.arange(cap) % 32] = 0xFF
    ones = np.full((cap, 32), 0xFF, np.uint8)
    sets = [a, ~a, same, np.zeros((cap, 32), np.uint8), eight, ones]
    desc = np.stack(sets)
    rows = np.full(len(sets), cap, np.int32)
    pairs = [(0, 1), (0, 0), (1, 1), (0, 2), (3, 4), (3, 5), (5, 3), (2, 2)]
    got = _match_check(gctx, desc, rows, pairs)
    assert got[1] == cap and got[2] == cap                            # a set matched with itself: every row, at distance 0
    assert got[3:].tolist() == [0] * 5                                # every distance ties (d1 == d2): no match
    assert int(orb_ref.hamming(a[:1], (~a)[:1])[0, 0]) == 256


# ---- f. the cap
def test_explicit_cap_is_strict(gctx):
    from pyannote_video_amd._lib import OrbCapError, PvfError
    frame = _textured(1920, 1080, seed=3)
    n = len(orb_ref.orb_frame(frame)[0])
    with pytest.raises(OrbCapError, match="%d keypoints" % n) as e:
        gctx.orb_extract([frame, frame], 200, 355, cap=n - 1)
    assert e.value.needed == n
    with pytest.raises(PvfError, match="no pvf_orb_extract result"):
        gctx.orb_match_counts([(0, 1)])                               # nothing was kept: no truncated set to match
    grid = _dot_grid(4)
    g = len(orb_ref.orb_frame(grid)[0])
    with pytest.raises(OrbCapError) as e:
        gctx.orb_extract([_textured(200, 200, seed=3), grid], 200, 200, cap=1024)
    assert e.value.needed == g
    counts, _, _, _ = orb_check.check_frames(gctx, [grid], cap=g)     # exactly the rows it needs
    assert counts[0] == g


def _grid_clip(fps=25.0, per=12):
    """200 x 200 shots A B G A G C, G a dot grid (more keypoints than the default cap)"""
    tex, _, _ = thread_clip.make_clip(width=200, height=200, frames_per_shot=per, setups="ABAC", frame_rate=fps)
    grid = np.stack([_dot_grid(4)] * per)
    frames = np.concatenate([tex[:2 * per], grid, tex[2 * per:3 * per], grid, tex[3 * per:]])
    shots = [(i * per / fps, (i + 1) * per / fps) for i in range(6)]
    return frames, shots, fps


def _restated_counts(frames, shots, fps, pairs):
    """thread.py's match count of every pair, from orb_ref (as test_gpu_thread.py::test_thread_equals_restatement)"""
    collar = 10. / fps
    orb = {}

    def desc(t):
        i = int(fps * t + 1e-5)
        if i not in orb:
            orb[i] = orb_ref.orb_frame(frames[i])[1]
        return orb[i]
    return [orb_ref.match_count(desc(shots[i][1] - collar), desc(shots[k][0] + collar)) for i, k in pairs]


def test_thread_and_cli_on_a_dot_grid_shot(gctx, tmp_path):
    from pyannote_video_amd import cli, structure
    frames, shots, fps = _grid_clip()
    video = thread_clip.ClipVideo(frames, fps)
    segs = [structure.Segment(a, b) for a, b in shots]
    _, pairs, counts = structure.Thread(video, shot=segs, lookahead=24, ctx=gctx).match_counts()
    ref = _restated_counts(frames, shots, fps, pairs)
    np.testing.assert_array_equal(counts, ref)
    _, _, chunked = structure.Thread(video, shot=segs, lookahead=24, ctx=gctx, chunk=3).match_counts()    # caps 1024, more, 1024
    np.testing.assert_array_equal(chunked, ref)
    clip = str(tmp_path / "clip.npy")
    np.save(clip, frames)
    shot_json = str(tmp_path / "shots.json")
    with open(shot_json, "w") as f:
        json.dump({"pyannote": "Timeline", "content": [{"start": a, "end": b} for a, b in shots]}, f)
    out = str(tmp_path / "threads.json")
    assert cli.main(["--fps", str(fps), "thread", clip, shot_json, out]) == 0
    with open(out) as f:
        got = json.load(f)
    want = structure.thread_labels(segs, [p for p, c in zip(pairs, ref) if c > 20])
    assert got["content"] == want.for_json()["content"]
