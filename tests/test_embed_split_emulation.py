"""CPU restatement of the embedder's split path (csrc/resnet.hip: conv_tile_k with ConvSplit, conv_wsplit_k) on the synthetic embedder, the two chips of
tests/golden/hotpath_small.npz and two random-byte chips: every convolution outside the 32-channel stage as hi.hi + hi.lo + lo.hi of f16
halves of the scaled operands (activations x 2^8, weights x 2^w_exp with the largest |w| in [2^14, 2^15)), products and sums in f64 so
that only the split's error is measured; the first layer and the 32-channel stage stay fp32 as in the kernels.  Descriptors are
compared with tests/torch_ref.py's f64 forward."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pyannote_video_amd import models  # noqa: E402
import torch_ref  # noqa: E402

A_EXP = 8                                   # EMB_A_SCALE_EXP
F16_MIN_NORMAL = 2.0 ** -14


def w_exp_of(w):
    """ctx.hip load_embedder: the power of two that puts the largest |w| in [2^14, 2^15)"""
    m = float(np.abs(w).max())
    return 15 - int(np.frexp(np.float32(m))[1]) if m > 0 else 0


def halves(v32, flush):
    """hi = f16(v), lo = f16(v - hi) (the difference in fp32), as f64 tensors"""
    hi = v32.to(torch.float16)
    lo = (v32 - hi.to(torch.float32)).to(torch.float16)
    hi, lo = hi.double(), lo.double()
    if flush:
        hi = torch.where(hi.abs() < F16_MIN_NORMAL, torch.zeros_like(hi), hi)
        lo = torch.where(lo.abs() < F16_MIN_NORMAL, torch.zeros_like(lo), lo)
    return hi, lo


def forward(chip_u8, params, mode, flush=False):
    """mode "fp32": every convolution in float32 (the exact kernels' rounding, another order); "split": as the kernels run by default"""
    units = models.RESNET_UNITS
    t32 = lambda k: torch.from_numpy(np.ascontiguousarray(params[k])).float()

    def conv(x32, name, stride, pad, split):
        w32 = t32(name + ".w")
        if not split:
            return F.conv2d(x32, w32, None, stride=stride, padding=pad)
        e = w_exp_of(params[name + ".w"])
        xh, xl = halves(x32 * 2.0 ** A_EXP, flush)
        wh, wl = halves(w32 * 2.0 ** e, flush)
        c = lambda a, b: F.conv2d(a, b, None, stride=stride, padding=pad)
        acc = c(xh, wh) + c(xh, wl) + c(xl, wh)
        return (acc.float() * 2.0 ** -(A_EXP + e))

    avg = torch.tensor([122.782, 117.001, 104.298], dtype=torch.float32)
    x = ((torch.from_numpy(chip_u8.astype(np.float32)) - avg) / 256.0).permute(2, 0, 1)[None]
    x = F.conv2d(x, t32("conv1.w"), None, stride=2, padding=0)
    x = F.relu((x + t32("conv1.b")[None, :, None, None]) * t32("aff1.g")[None, :, None, None] + t32("aff1.b")[None, :, None, None])
    x = F.max_pool2d(x, 3, 2, 0)
    for u, (cin, n, down) in enumerate(units):
        split = mode == "split" and not (cin == 32 and n == 32)
        p = "u%d." % u
        a = conv(x, p + "a", 2 if down else 1, 0 if down else 1, split)
        a = F.relu((a + t32(p + "a.b")[None, :, None, None]) * t32(p + "a.g")[None, :, None, None] + t32(p + "a.beta")[None, :, None, None])
        b = conv(a, p + "b", 1, 1, split)
        b = (b + t32(p + "b.b")[None, :, None, None]) * t32(p + "b.g")[None, :, None, None] + t32(p + "b.beta")[None, :, None, None]
        s = F.avg_pool2d(x, 2, 2, 0) if down else x
        oh, ow = max(b.shape[2], s.shape[2]), max(b.shape[3], s.shape[3])
        out = torch.zeros(x.shape[0], n, oh, ow, dtype=torch.float32)
        out[:, :, :b.shape[2], :b.shape[3]] += b
        out[:, :s.shape[1], :s.shape[2], :s.shape[3]] += s
        x = F.relu(out)
    feat = x.double().mean(dim=(2, 3))
    return (feat @ torch.from_numpy(np.ascontiguousarray(params["fc.w"])).double()).numpy()


@pytest.fixture(scope="module")
def setup():
    params = models.split_resnet_blob(models.make_embedder()["emb.blob"])
    g = np.load(os.path.join(ROOT, "tests", "golden", "hotpath_small.npz"))
    rnd = np.random.default_rng(11).integers(0, 256, (2, 150, 150, 3), dtype=np.uint8)
    chips = np.concatenate([g["chips"], rnd])
    ref = np.stack([torch_ref.forward(c, params, models.RESNET_UNITS) for c in chips])
    return params, chips, ref


def _err(params, chips, ref, mode, flush=False):
    out = np.concatenate([forward(c, params, mode, flush) for c in chips])
    return np.linalg.norm(out - ref, axis=1), out


def test_split_no_worse_than_fp32(setup):
    params, chips, ref = setup
    e32, _ = _err(params, chips, ref, "fp32")
    es, _ = _err(params, chips, ref, "split")
    assert es.max() <= e32.max(), (es, e32)
    assert es.max() < 1e-5


def test_split_with_flushed_subnormals(setup):
    params, chips, ref = setup
    e32, _ = _err(params, chips, ref, "fp32")
    ef, _ = _err(params, chips, ref, "split", flush=True)
    assert ef.max() <= e32.max(), (ef, e32)


def test_scales_depend_on_weights_only(setup):
    """w_exp follows from the layer's weights alone (ctx.hip), the activation scale is the constant 2^8"""
    params, chips, _ = setup
    for u in range(len(models.RESNET_UNITS)):
        for ab in "ab":
            w = params["u%d.%s.w" % (u, ab)]
            e = w_exp_of(w)
            assert 2.0 ** 14 <= np.abs(w).max() * 2.0 ** e < 2.0 ** 15
            assert w_exp_of(w * np.float32(4.0)) == e - 2 and w_exp_of(-w) == e
    # the activation scale is a constant: the same chip gives the same descriptor whatever was embedded before it
    a = forward(chips[0], params, "split")
    forward(chips[2], params, "split")
    assert np.array_equal(forward(chips[0], params, "split"), a)
