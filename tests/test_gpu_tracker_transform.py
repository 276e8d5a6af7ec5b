"""GPU: the fused tracker kernels (csrc/dsst.hip start_fused_k, update_fused_k) and the 256-thread transform under the commit
(trans_planes_fft_k, peak_k) against oracle.Tracker, after the 64 x 64 transform's twiddle factors moved from LDS / vector registers
into scalar registers (fft2d_lds).  The move changes no butterfly, operand order or value, so everything is compared bit for bit:
no tolerance anywhere.

96 x 80 frames; 1, 3 and 65 trackers per call (65: more than one block per wave slot of a small grid, and every wave number b = 0..7
of the transform's second phase in many blocks at once).  Each tracker goes start_many -> update_many(defer=True) -> commit_many; the
oracle's start_track / update is the reference (a deferred update and its commit equal dlib's update()).  Among the first three:
an ordinary box, a box half off the frame, and an update on an all-black frame; the rest mix boxes inside, across and beyond the
frame's edges with starts and updates on picture and black frames.

PSR and boxes compare as 64-bit patterns (so -0.0 is not 0.0).  A NaN must meet a NaN in the same place, but all NaNs count as one
pattern: the PSR of an all-zero response is 0/0, whose sign bit the x86 of the oracle sets and the GPU does not
(tests/test_gpu_tracker_edges.py).  The filter state (pvf_debug_tracker_state: A, B; and the scale filters) compares as bytes after
the start and after the commit.
Reference: pyannote/video/tracking.py:203,231,250-251."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 96, 80
N_MAX = 65


def _picture(seed):
    """blobs of 8 x 8 pixels under a little noise: something a correlation filter can hold on to"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 256, (H // 8, W // 8, 3)).astype(np.int64)
    img = np.kron(coarse, np.ones((8, 8, 1), np.int64)) + rng.integers(-12, 13, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _moved(frame, dx, dy):
    out = np.zeros_like(frame)
    out[dy:, dx:] = frame[:H - dy, :W - dx]
    return out


def _cases():
    """-> (start frame, update frame, box) per tracker; the first one, and the first three, are the small batches"""
    pic = _picture(5)
    nxt = _moved(pic, 3, 2)
    black = np.zeros((H, W, 3), np.uint8)
    cases = [(pic, nxt, (30.0, 22.0, 66.0, 58.0)),                     # ordinary
             (pic, nxt, (-20.0, 10.0, 20.0, 50.0)),                    # half off the frame (left)
             (pic, black, (40.0, 30.0, 70.0, 60.0)),                   # all-black update: zero response, PSR 0/0
             (black, pic, (20.0, 20.0, 60.0, 60.0)),                   # started on black: zero filters
             (black, black, (10.0, 10.0, 50.0, 40.0)),
             (pic, nxt, (70.0, 50.0, 118.0, 106.0)),                   # across the bottom right corner
             (pic, nxt, (10.0, -15.0, 40.0, 15.0)),                    # half off the top
             (pic, nxt, (0.0, 0.0, 96.0, 80.0)),                       # the whole frame
             (pic, nxt, (-40.0, -30.0, 136.0, 110.0)),                 # larger than the frame
             (pic, nxt, (120.0, 20.0, 150.0, 50.0)),                   # wholly outside
             (pic, nxt, (44.5, 31.25, 56.75, 47.5))]                   # small, fractional corners
    rng = np.random.default_rng(17)
    while len(cases) < N_MAX:
        w, h = float(rng.integers(10, 60)), float(rng.integers(10, 60))
        x, y = float(rng.integers(-20, W - 10)), float(rng.integers(-20, H - 10))
        k = len(cases) % 9
        f0, f1 = (black, pic) if k == 7 else (pic, black) if k == 8 else (pic, nxt)
        cases.append((f0, f1, (x, y, x + w, y + h)))
    return cases


def _bits(a):
    """float64 -> uint64 patterns, every NaN as one pattern (see the module's docstring)"""
    a = np.ascontiguousarray(a, np.float64).copy()
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def _ref_state(r):
    A, B = r.debug_state()
    As, Bs = r.debug_scale_state()
    return tuple(x.tobytes() for x in (A, B, As, Bs))


def _gpu_state(ctx, h):
    _, A, B = ctx.tracker_state(h)
    As, Bs = ctx.tracker_scale_state(h)
    return tuple(x.tobytes() for x in (A, B, As, Bs))


@pytest.fixture(scope="module")
def reference(oracle):
    """the oracle's answers for all 65 trackers, computed once: trackers do not see each other, so a smaller batch is a prefix"""
    from pyannote_video_amd import models
    tables = models.dsst_tables()
    cases = _cases()
    ref = []
    for f0, f1, box in cases:
        r = oracle.Tracker(tables)
        r.start_track(f0, box)
        started = _ref_state(r)
        psr = r.update(f1)
        ref.append(dict(started=started, psr=psr, pos=r.get_position(), committed=_ref_state(r)))
    return cases, ref


def test_the_cases_hold_what_they_are_meant_to(reference):
    cases, ref = reference
    assert len(cases) == N_MAX
    x0, _, x1, _ = cases[1][2]
    assert x0 < 0 < x1 and -x0 == x1                                   # half of the box lies left of the frame
    assert not cases[2][1].any() and np.isnan(ref[2]["psr"])           # the all-black update ends in 0/0
    assert np.isfinite(ref[0]["psr"]) and ref[0]["pos"] != cases[0][2]  # the ordinary tracker followed the picture
    assert sum(bool(np.isnan(r["psr"])) for r in ref) < N_MAX // 2


@pytest.mark.parametrize("n", [1, 3, N_MAX])
def test_start_deferred_update_and_commit_equal_the_oracle(ctx, reference, n):
    cases, ref = reference
    cases, ref = cases[:n], ref[:n]
    f0, f1 = [c[0] for c in cases], [c[1] for c in cases]           # three distinct arrays: staged once each, by identity
    trk = ctx.tracker_create_many(n)
    try:
        ctx.tracker_start_many(trk, f0, [c[2] for c in cases])
        bad = [(k, "state after the start") for k in range(n) if _gpu_state(ctx, trk[k]) != ref[k]["started"]]
        psr, boxes = ctx.tracker_update_many(trk, f1, defer=True)
        bad += [(k, "the deferred update wrote the filters") for k in range(n) if _gpu_state(ctx, trk[k]) != ref[k]["started"]]
        want_psr, want_box = _bits([r["psr"] for r in ref]), _bits([r["pos"] for r in ref])
        print("n", n, "psr", np.asarray(psr)[:4], "oracle", [r["psr"] for r in ref[:4]])
        bad += [(k, "psr", float(psr[k]), ref[k]["psr"]) for k in np.flatnonzero(_bits(psr) != want_psr)]
        bad += [(k, "box", boxes[k].tolist(), ref[k]["pos"]) for k in np.flatnonzero((_bits(boxes) != want_box).any(axis=1))]
        ctx.tracker_commit_many(trk, f1)
        bad += [(k, "state after the commit") for k in range(n) if _gpu_state(ctx, trk[k]) != ref[k]["committed"]]
        bad += [(k, "position after the commit") for k in range(n)
                if not np.array_equal(_bits(ctx.tracker_position(trk[k])), _bits(ref[k]["pos"]))]
        assert not bad, bad[:20]
    finally:
        ctx.tracker_destroy_many(trk)
