"""Shot threading on the GPU (csrc/orb.hip): ORB extraction bit-exact against tests/orb_ref.py, the matcher exact against numpy brute
force, and the `thread` verb end to end against what the reference's own thread.py produced on the same clip
(tests/golden/reference_thread_pins.json, tests/golden/make_reference_thread_pins.py)."""
import json
import os

import numpy as np
import pytest

import orb_check
import orb_ref
import thread_clip

pytestmark = pytest.mark.gpu
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_thread_pins.json")


@pytest.fixture(scope="module")
def gctx():
    from pyannote_video_amd.runtime import Context
    c = Context(device=0)
    yield c
    c.close()


def _textured(h, w, seed):
    f, _, _ = thread_clip.make_clip(width=w, height=h, frames_per_shot=1, setups="A", seed=seed)
    return f[0]


def _check_frames(gctx, frames):
    return orb_check.check_frames(gctx, frames)[0]        # count, keypoint rows and descriptors against orb_ref, bit for bit


@pytest.mark.parametrize("h,w", [(720, 1280), (1080, 1920), (2160, 3840)])
def test_orb_extract_bit_exact(gctx, h, w):
    counts = _check_frames(gctx, [_textured(h, w, seed=3), _textured(h, w, seed=4)])
    assert counts.min() > 100


def test_orb_extract_no_corners(gctx):
    flat = np.full((1080, 1920, 3), 97, np.uint8)
    counts = _check_frames(gctx, [flat, _textured(1080, 1920, seed=5)])
    assert counts[0] == 0 and counts[1] > 0


def _brute(desc, rows, pairs):
    return np.array([orb_ref.match_count(desc[a, :rows[a]], desc[b, :rows[b]]) for a, b in pairs], np.int64)


def test_match_counts_exact(gctx):
    rng = np.random.default_rng(0)
    rows = np.array([0, 1, 2, 3, 500, 480, 1500, 300, 64, 257], np.int32)
    cap = 1536
    desc = rng.integers(0, 256, (len(rows), cap, 32), dtype=np.uint8)
    # tie-heavy sets: a few distinct rows repeated, and rows one or two bits apart
    base = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    desc[8, :64] = base[rng.integers(0, 4, 64)]
    desc[9, :257] = base[rng.integers(0, 4, 257)]
    desc[9, ::3, 0] ^= 1
    desc[7, :300] = desc[4, :300] ^ (rng.random((300, 32)) < 0.05).astype(np.uint8)
    pairs = [(a, b) for a in range(len(rows)) for b in range(len(rows))]
    got = gctx.orb_match_counts(pairs, desc, rows)
    np.testing.assert_array_equal(got, _brute(desc, rows, pairs))
    assert got[pairs.index((4, 7))] > 200                # near copies pass the ratio test


def test_match_counts_batch_10000(gctx):
    rng = np.random.default_rng(1)
    n_sets, cap = 48, 80
    rows = rng.integers(0, cap + 1, n_sets).astype(np.int32)
    desc = rng.integers(0, 256, (n_sets, cap, 32), dtype=np.uint8)
    desc[rng.integers(0, n_sets, 10)] >>= 6                                     # many equal distances
    pairs = rng.integers(0, n_sets, (12000, 2))
    got = gctx.orb_match_counts(pairs, desc, rows)
    table = np.array([[orb_ref.match_count(desc[a, :rows[a]], desc[b, :rows[b]]) for b in range(n_sets)] for a in range(n_sets)])
    np.testing.assert_array_equal(got, table[pairs[:, 0], pairs[:, 1]])


def test_match_counts_resident_equals_host(gctx):
    frames = [_textured(270, 480, seed=s) for s in (1, 1, 2)]
    counts, _, desc = gctx.orb_extract(frames, 200, 112)
    pairs = [(0, 1), (1, 0), (0, 2), (2, 2)]
    np.testing.assert_array_equal(gctx.orb_match_counts(pairs), gctx.orb_match_counts(pairs, desc, counts))


def test_thread_equals_restatement(gctx):
    from pyannote_video_amd import structure
    frames, shots, fps = thread_clip.make_clip()
    video = thread_clip.ClipVideo(frames, fps)
    th = structure.Thread(video, shot=[structure.Segment(a, b) for a, b in shots], lookahead=24, ctx=gctx)
    _, pairs, counts = th.match_counts()
    collar = 10. / fps
    ref = []
    for i, k in pairs:
        a = orb_ref.orb_frame(frames[int(fps * (shots[i][1] - collar) + 1e-5)])[1]
        b = orb_ref.orb_frame(frames[int(fps * (shots[k][0] + collar) + 1e-5)])[1]
        ref.append(orb_ref.match_count(a, b))
    np.testing.assert_array_equal(counts, ref)


def test_cli_thread_matches_reference_pins(gctx, tmp_path):
    from pyannote_video_amd import cli, structure
    from pyannote_video_amd._core import Annotation
    with open(PINS) as f:
        pins = json.load(f)
    frames, shots, fps = thread_clip.make_clip(**pins["clip"])
    clip = str(tmp_path / "clip.npy")
    np.save(clip, frames)
    shot_json = str(tmp_path / "shots.json")
    with open(shot_json, "w") as f:
        json.dump({"pyannote": "Timeline", "content": [{"start": a, "end": b} for a, b in shots]}, f)
    out = str(tmp_path / "threads.json")
    assert cli.main(["--fps", str(fps), "thread", clip, shot_json, out]) == 0
    with open(out) as f:
        got = json.load(f)
    assert got["content"] == pins["threads"]["content"]
    scenes = structure.thread_scenes(Annotation.from_json(got))
    assert scenes.for_json()["content"] == pins["scenes"]["content"]
