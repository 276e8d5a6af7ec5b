"""The embedder's split path (csrc/resnet.hip: conv_tile_k with ConvSplit, the default) against its exact fp32 kernels on the same chips: the error
bound, batch independence, the range guard with its per-face exact fallback, and the switch."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))

from pyannote_video_amd import models  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def embedder_path(tmp_path_factory):
    return models.ensure_synthetic_models(str(tmp_path_factory.mktemp("emb_split")), small=True)[1]


@pytest.fixture(scope="module")
def chips():
    """random-byte chips and the two chips of the hot-path fixture"""
    rng = np.random.default_rng(7)
    c = rng.integers(0, 256, (64, 150, 150, 3), dtype=np.uint8)
    g = np.load(os.path.join(ROOT, "tests", "golden", "hotpath_small.npz"))
    extra = [g[k] for k in g.files if g[k].dtype == np.uint8 and g[k].shape[-3:] == (150, 150, 3)]
    if extra:
        c = np.concatenate([np.concatenate([e.reshape(-1, 150, 150, 3) for e in extra]), c])
    return np.ascontiguousarray(c)


def _ctx(path, split):
    from pyannote_video_amd.runtime import Context
    ctx = Context(0)
    ctx.load_embedder(path)
    ctx.embedder_split(split)
    return ctx


def test_split_against_exact(embedder_path, chips):
    exact = _ctx(embedder_path, False).embed_chips(chips)
    ctx = _ctx(embedder_path, True)
    split = ctx.embed_chips(chips)
    l2 = np.linalg.norm(split.astype(np.float64) - exact, axis=1)
    assert l2.max() <= 2e-5, l2.max()
    assert not np.array_equal(split, exact)            # the split path did run
    st = ctx.embedder_split_stats()
    assert st["faces"] == len(chips) and st["reruns"] == 0
    assert 0.0 <= st["pipe_err"] <= 2304 * 2.0 ** -22


def test_split_batch_independent(embedder_path, chips):
    ctx = _ctx(embedder_path, True)
    rng = np.random.default_rng(3)
    big = np.concatenate([chips, rng.integers(0, 256, (4096 - len(chips), 150, 150, 3), dtype=np.uint8)])
    e_big = ctx.embed_chips(big)
    perm = rng.permutation(len(big))
    e_perm = ctx.embed_chips(np.ascontiguousarray(big[perm]))
    assert np.array_equal(e_perm, e_big[perm])
    assert np.array_equal(ctx.embed_chips(big[:7]), e_big[:7])
    for i in (0, 5, 4095):
        assert np.array_equal(ctx.embed_chips(big[i:i + 1]), e_big[i:i + 1])


def test_range_guard_reruns_exact(embedder_path, chips, tmp_path):
    m = models.load_container(embedder_path)
    blob = np.array(m["emb.blob"], np.float32)
    o = 0
    for name, shape in models.resnet_param_layout():
        n = int(np.prod(shape))
        if name == "u4.a.w":                           # its outputs feed u4.b, a split layer: far above 65504 / 2^8 there
            blob[o:o + n] *= np.float32(2.0 ** 12)
        o += n
    m["emb.blob"] = blob
    path = str(tmp_path / "scaled.pvfm")
    models.save_container(path, m)
    exact = _ctx(path, False).embed_chips(chips)
    ctx = _ctx(path, True)
    split = ctx.embed_chips(chips)
    st = ctx.embedder_split_stats()
    assert st["reruns"] > 0
    assert st["reruns"] == len(chips)                  # every face goes over the range with these weights
    assert np.array_equal(split, exact)


def test_switch_off_is_exact_path(embedder_path, chips, monkeypatch):
    a = _ctx(embedder_path, False).embed_chips(chips)
    monkeypatch.setenv("PVF_EMBEDDER_SPLIT", "0")
    from pyannote_video_amd.runtime import Context
    ctx = Context(0)
    ctx.load_embedder(embedder_path)
    b = ctx.embed_chips(chips)
    assert np.array_equal(a, b)
    assert ctx.embedder_split_stats() == {"faces": 0, "reruns": 0, "pipe_err": -1.0}
