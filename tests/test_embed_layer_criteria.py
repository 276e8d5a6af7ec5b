"""That the per-layer criteria of tests/embed_ref.py bite, shown on the CPU before any GPU run: the fp32 and split restatements of the
embedder pass A and B at every layer with three weight sets, and each of ten deliberate defects, put into the restatement where a
kernel could have it, fails A or B at its own layer.  Beside each the change of the final descriptor is printed with the suite's
descriptor gates (1e-4 against the oracle, 2e-5 split against exact); the table (pytest -s) is the one in DESIGN.md section 4."""
import hashlib
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
import embed_ref as R  # noqa: E402
import torch_ref  # noqa: E402

DEFAULT_BLOB_SHA256 = "787b430b490d7781dc5e65662d2d2d495f67ad37906b610235eedb8e8e54d890"

WEIGHT_SETS = {
    "default": dict(),
    "seed1": dict(seed=1),
    "signs": dict(seed=2, gamma_signs=True, beta_sigma=0.5),
}


def weight_set(name):
    return models.split_resnet_blob(models.make_embedder(**WEIGHT_SETS[name])["emb.blob"])


@pytest.fixture(scope="module")
def chips():
    g = np.load(os.path.join(ROOT, "tests", "golden", "hotpath_small.npz"))
    rnd = np.random.default_rng(11).integers(0, 256, (2, 150, 150, 3), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([g["chips"][:1], rnd]))


emulate = R.emulate


def test_default_weights_unchanged():
    """make_embedder()'s keyword arguments leave its default output byte for byte what it was"""
    assert hashlib.sha256(models.make_embedder()["emb.blob"].tobytes()).hexdigest() == DEFAULT_BLOB_SHA256
    a, b = models.make_embedder(seed=2)["emb.blob"], models.make_embedder(seed=2, gamma_signs=True, beta_sigma=0.5)["emb.blob"]
    pa, pb = models.split_resnet_blob(a), models.split_resnet_blob(b)
    assert np.array_equal(pa["u5.a.w"], pb["u5.a.w"]) and np.array_equal(np.abs(pa["u5.a.g"]), np.abs(pb["u5.a.g"]))
    assert (pb["u5.a.g"] < 0).any() and (pb["u5.a.g"] > 0).any()
    assert np.allclose(pb["u5.a.beta"], pa["u5.a.beta"] * 10.0)


def test_stages_end_in_the_reference_descriptor(chips, oracle):
    params = weight_set("default")
    st = R.stages(chips, params)
    assert len(st) == 30 and st[0].shape == (3, 72, 72, 32) and st[1].shape == (3, 35, 35, 32) and st[-1].shape == (3, 2, 2, 256)
    assert st[22].shape == (3, 3, 3, 256) and st[23].shape == (3, 4, 4, 256) and st[28].shape == (3, 1, 1, 256)
    d = R.descriptor(st[-1], params)
    ref = np.stack([torch_ref.forward(c, params, models.RESNET_UNITS) for c in chips])
    assert np.abs(d - ref).max() <= 1e-12
    emb = oracle.Embedder(models.make_embedder())
    for c, row in zip(chips, d):
        assert np.linalg.norm(emb.forward(c) - row) < 1e-4 * max(1.0, np.linalg.norm(row))
    # row 3 / column 3 of unit 10's output is the averaged skip alone, and only in the skip's 128 channels
    assert np.all(st[23][:, 3, :, 128:] == 0) and np.all(st[23][:, :, 3, 128:] == 0) and np.any(st[23][:, 3, :, :128] != 0)


@pytest.mark.parametrize("wset", sorted(WEIGHT_SETS))
@pytest.mark.parametrize("split", [False, True])
def test_restatements_pass(chips, wset, split):
    params = weight_set(wset)
    outs, table, desc = emulate(chips, params, split)
    ref = R.descriptor(R.stages(chips, params)[-1], params)
    print("\n%s %s: descriptor L2 against f64 %s" % (wset, "split" if split else "fp32", np.linalg.norm(desc - ref, axis=1)))
    for i, name, j in table:
        print("  %2d %-6s A worst %.4f  rms %.3e" % (i, name, j["a_worst"], j["rms_cpu"]))
        assert j["a_ok"] and j["b_ok"], (wset, split, name, j)
    assert all(np.isfinite(o).all() for o in outs.values())


# ---- the ten defects ------------------------------------------------------------------------------------------------------------
def _stage(name):
    specs = R.layer_specs(weight_set("default"), models.RESNET_UNITS)
    return [n for n, _, _ in specs].index(name)


def _pad_row_as_neighbour(acc, x, w):
    """tap row 0 of output row 0 reads input row 0 (its neighbour) where the padding row's zeros belong"""
    acc = acc.clone()
    acc[:, :, 0, :] += F.conv2d(x[:, :, 0:1, :], w[:, :, 0:1, :].to(x.dtype), None, stride=1, padding=(0, 1))[:, :, 0, :]
    return acc


def _zero_corner(y, clean):
    c = int(np.argmax(clean[0, 16, 16, :]))
    assert y.shape[1:3] == (17, 17) and clean[0, 16, 16, c] > 0
    y[:, 16, 16, c] = 0.0
    return y


def _drop_last_skip_channel(x, kw):
    s = np.array(kw["skip"], copy=True)
    s[..., -1] = 0.0
    kw["skip"] = s
    return x, kw


def _avg_3_of_4(s):
    h, w = s.shape[2] // 2, s.shape[3] // 2
    q = lambda dy, dx: s[:, :, dy:2 * h:2, dx:2 * w:2]
    return ((q(0, 0) + q(0, 1)) + q(1, 0)) * 0.25


def _column_148_zero(x, kw):
    x = np.array(x, copy=True)
    x[:, :, 148, :] = (np.float32(0.0) - np.array(R.MEAN, np.float32)) / np.float32(256.0)       # a zero byte, as a read past the buffer gives
    return x, kw


def _neighbours_pixel(x, kw):
    x = np.array(x, copy=True)
    x[-1, 0, 0, :] = x[-2, 0, 0, :]
    return x, kw


MUTANTS = [
    # (what, stage name, split forward?, fault)
    ("lo.hi term dropped", "u9.a", True, {"fault": {"terms": (1, 1, 0)}}),
    ("hi.lo term dropped", "u9.a", True, {"fault": {"terms": (1, 0, 1)}}),
    ("w_exp off by one, out_scale not", "u5.b", True, {"fault": {"conv": lambda acc, x, w: acc * 2.0}}),
    ("padding row read as its neighbour (one tap row)", "u1.a", False, {"fault": {"conv": _pad_row_as_neighbour}}),
    ("corner pixel of a 17 x 17 map zero in one channel", "u4.b", False, {"post": _zero_corner}),
    ("last skip channel (XC - 1) missing in unit 3", "u3.b", True, {"inputs": _drop_last_skip_channel}),
    ("2 x 2 average taken as 3 of 4", "u7.b", True, {"fault": {"avg": _avg_3_of_4}}),
    ("row 3 of unit 10's 4 x 4 output not zero-extended", "u10.b", True, {"fault": {"extend": lambda b, g, bt: (b * g) + bt}}),
    ("column 148 of the chip read as zero", "stem", False, {"inputs": _column_148_zero}),
    ("last face reads its neighbour's pixel", "u8.a", True, {"inputs": _neighbours_pixel}),
]


def test_mutants_are_caught_at_their_layer(chips):
    params = weight_set("default")
    clean = {s: emulate(chips, params, s) for s in (False, True)}
    for s in clean:
        assert all(j["a_ok"] and j["b_ok"] for _, _, j in clean[s][1])
    rows, caught = [], 0
    for what, stage, split, f in MUTANTS:
        k = _stage(stage)
        outs, table, desc = emulate(chips, params, split, {k: f})
        at = {i: j for i, _, j in table}
        for i, name, j in table:
            if i < k:
                assert j["a_ok"] and j["b_ok"], (what, name)        # nothing before the defect is touched
        a_fail, b_fail = not at[k]["a_ok"], not at[k]["b_ok"]
        later = [name for i, name, j in table if i > k and not (j["a_ok"] and j["b_ok"])]
        assert not later, (what, later)                           # every later layer is judged on its own input: the defect does not spread
        dl2 = float(np.linalg.norm(desc - clean[split][2], axis=1).max())
        caught += a_fail or b_fail
        rows.append((what, stage, "split" if split else "fp32", a_fail, b_fail, at[k]["a_worst"], at[k]["ratio"], dl2))
    print("\n%-52s %-6s %-5s %-5s %-5s %10s %10s %12s %6s %6s" % ("defect", "layer", "path", "A", "B", "err/bound", "rms ratio", "descr. L2", "<1e-4", "<2e-5"))
    for what, stage, path, a_fail, b_fail, aw, ratio, dl2 in rows:
        print("%-52s %-6s %-5s %-5s %-5s %10.3g %10.3g %12.3e %6s %6s" % (what, stage, path, "FAILS" if a_fail else "ok", "FAILS" if b_fail else "ok", aw, ratio, dl2,
                                                                         "yes" if dl2 < 1e-4 else "no", "yes" if dl2 < 2e-5 else "no"))
    missed = [r[0] for r in rows if not (r[3] or r[4])]
    assert caught >= 9, missed
