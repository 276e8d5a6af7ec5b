"""Test infrastructure: csrc/orb.hip's extraction held bit for bit equal to tests/orb_ref.py -- count, x, y, level, FAST score, Harris
response, angle and all 32 descriptor bytes of every keypoint of every frame."""
import numpy as np

import orb_ref


def levels(ow, oh):
    """pyramid levels with an interior (both sides > 2 * 31) of a small image ow x oh: the levels orb.hip runs"""
    return sum(1 for lw, lh in orb_ref.level_sizes(ow, oh) if lw > 2 * orb_ref.EDGE and lh > 2 * orb_ref.EDGE)


def chunk_frames(ow, oh, cap):
    """frames per launch chunk of orb_extract (csrc/orb.hip): 1 GiB over the per-frame scratch of the levels, candidates and slots"""
    al = lambda n: (n + 255) // 256 * 256
    P = C = 0
    for lw, lh in orb_ref.level_sizes(ow, oh)[:levels(ow, oh)]:
        P += al(lw * lh)
        C += al(lw * lh // 2 + 64)
    return (1 << 30) // (P * 5 + C * 12 + orb_ref.NLEVELS * cap * (24 + 32))


def reference(frame, ow, oh):
    """orb_ref of one RGB frame at the small image ow x oh (orb_ref.orb_frame for the thread_size geometry)"""
    return orb_ref.orb_gray(orb_ref.gray(orb_ref.resize_linear_rgb(frame, ow, oh)))


def assert_equal(counts, kp, desc, refs):
    """the GPU's rows of every frame == the restatement's keypoints and descriptors, bit for bit"""
    assert len(counts) == len(refs)
    for i, (rk, rd) in enumerate(refs):
        n = counts[i]
        assert n == len(rk), (i, n, len(rk))
        np.testing.assert_array_equal(kp[i, :n, :4], rk[:, :4].astype(np.float32))
        np.testing.assert_array_equal(kp[i, :n, 4], rk[:, 4].astype(np.float32))       # Harris response, bit for bit
        np.testing.assert_array_equal(kp[i, :n, 5], rk[:, 5].astype(np.float32))       # angle, bit for bit
        np.testing.assert_array_equal(desc[i, :n], rd)


def check_frames(ctx, frames, height=200, size=None, cap=None):
    """ctx.orb_extract of the frames at `size` (default: thread_size at `height`) == orb_ref of each frame.
    Returns (counts, keypoints, descriptors, [(reference keypoints, reference descriptors)] per frame)."""
    ow, oh = size or orb_ref.thread_size(frames[0].shape[1], frames[0].shape[0], height)
    counts, kp, desc = ctx.orb_extract(frames, ow, oh, cap)
    refs = [reference(f, ow, oh) for f in frames]
    assert_equal(counts, kp, desc, refs)
    return counts, kp, desc, refs
