"""The face embedder (csrc/resnet.hip) layer by layer against an f64 reference: every stage of the forward (pvf_debug_embed_stage) and
single layers at the shapes where such kernels go wrong (pvf_debug_conv), each judged ALONE -- the reference gets the GPU's own input of
that layer -- under the two criteria of tests/embed_ref.py: A, a derived per-element bound; B, the layer's RMS error against f64 within
4 x that of a CPU restatement of the same arithmetic on the same input.  tests/test_embed_layer_criteria.py shows on the CPU that the
criteria see ten kinds of defect.  Kernels reached: stem_conv_k, maxpool3s2_k, conv3x3_c32_k, conv_tile_k<4,1> / <2,2> with
ConvExact and with ConvSplit, conv_wsplit_k, conv_frag_k, head_k."""
import json
import os
import sys
import time
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pyannote-video_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pyannote_video_amd import models  # noqa: E402
import embed_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

WEIGHT_SETS = {"seed1": dict(seed=1), "signs": dict(seed=2, gamma_signs=True, beta_sigma=0.5)}


# ---- chips --------------------------------------------------------------------------------------------------------------------------
def structured_chips():
    """all 0, all 255, 0 except row / column 148, 0 except row / column 149 (which no 7-tap stride-2 window on 150 reads)"""
    z = np.zeros((150, 150, 3), np.uint8)
    c148, c149 = z.copy(), z.copy()
    c148[148, :, :] = 255
    c148[:, 148, :] = 255
    c149[149, :, :] = 255
    c149[:, 149, :] = 255
    return [z, np.full_like(z, 255), c148, c149]


def batch(n):
    """n chips: the two of the hot-path fixture, random bytes, the structured ones; the batch always ENDS in a structured chip"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "hotpath_small.npz"))
    fix = [c for c in g["chips"][:2]]
    z, w, c148, c149 = structured_chips()
    if n == 1:
        return np.ascontiguousarray(np.stack([c148]))
    rnd = np.random.default_rng(5).integers(0, 256, (max(n - 6, 1), 150, 150, 3), dtype=np.uint8)
    chips = fix + [r for r in rnd] + [z, w, c149, c148]
    assert len(chips) == n
    return np.ascontiguousarray(np.stack(chips))


def judge_net(ctx, chips, params, split, label):
    """every stage of the GPU forward under A and B (the max-pool: equality); returns the per-layer table"""
    n = len(chips)
    specs = R.layer_specs(params, models.RESNET_UNITS)
    gpu = {-1: R.stem_input(chips)}
    flags = None
    for i in range(len(specs)):
        gpu[i], flags = ctx.embed_stage(chips, i, split)
        assert not flags.any(), (label, i, np.nonzero(flags))
    table, bad = [], []
    for i, spec in enumerate(specs):
        name, kind, a = spec
        if kind == "pool":
            assert np.array_equal(gpu[i], R.maxpool(gpu[0]).astype(np.float32)), (label, "max-pool")
            continue
        x, par, kw = R.stage_kwargs(spec, gpu)
        use_split = split and R.is_split_layer(a["w"])
        r = R.layer(x, *par, **kw)
        assert gpu[i].shape == r["y"].shape, (label, name, gpu[i].shape, r["y"].shape)
        cpu = (R.layer_split if use_split else R.layer_fp32)(x, *par, **kw)
        j = R.judge(gpu[i], r, cpu, use_split)
        table.append((name, "split" if use_split else "fp32", j))
        print("%-22s %-6s %-5s A worst %.4f  rms gpu %.3e cpu %.3e  ratio %.3f" % (label, name, "split" if use_split else "fp32", j["a_worst"], j["rms_y"],
                                                                                  j["rms_cpu"], j["ratio"]))
        if not (j["a_ok"] and j["b_ok"]):
            bad.append((name, j))
    assert not bad, (label, bad)
    return gpu, table


@pytest.fixture(scope="module")
def params():
    return models.split_resnet_blob(models.make_embedder()["emb.blob"])


# ---- a. the whole net, every stage -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("n", [1, 7, 128])
def test_every_stage(ctx, params, n, split):
    chips = batch(n)
    t0 = time.time()
    gpu, _ = judge_net(ctx, chips, params, split, "n=%d %s" % (n, "split" if split else "exact"))
    print("n=%d split=%d: %.1f s" % (n, split, time.time() - t0))
    if n >= 7:
        # row / column 149 is under no window: the first layer sees that chip as the all-zero one
        assert np.array_equal(gpu[0][n - 2], gpu[0][n - 4])
        assert not np.array_equal(gpu[0][n - 1], gpu[0][n - 4])


def test_stage_access_leaves_the_descriptors_alone(ctx, params):
    chips = batch(7)
    for split in (False, True):
        ctx.embedder_split(split)
        before = ctx.embed_chips(chips)
        ctx.embed_stage(chips, 11, split)
        assert np.array_equal(ctx.embed_chips(chips), before)
    ctx.embedder_split(True)
    with pytest.raises(Exception):
        ctx.embed_stage(chips, 30, False)
    assert np.array_equal(ctx.embed_chips(chips), before)


# ---- b. the dedicated 35 x 35 x 32 kernel against the generic one -----------------------------------------------------------------
def layer_params(rng, cin, cout, k=3, gamma="pos", beta=0.05):
    w = rng.normal(0, np.sqrt(2.0 / (cin * k * k)), (cout, cin, k, k)).astype(np.float32)
    bias = rng.normal(0, 0.1, cout).astype(np.float32)
    g = (1.0 + rng.normal(0, 0.05, cout)).astype(np.float32)
    if gamma == "neg":
        g = -g
    elif gamma == "mixed":
        g = g * rng.choice([-1.0, 1.0], cout).astype(np.float32)
    elif gamma == "zero":
        g = np.zeros(cout, np.float32)
    bt = (np.full(cout, float(beta)) if abs(beta) >= 1 else rng.normal(0, beta, cout)).astype(np.float32)
    return w, bias, g, bt


def relu_like(rng, shape):
    """N(0, 1) with about half the values zeroed"""
    x = rng.normal(0, 1, shape)
    return (x * (rng.random(shape) < 0.5)).astype(np.float32)


@pytest.mark.parametrize("B", [1, 128])
@pytest.mark.parametrize("with_skip", [False, True])
def test_c32_kernel_equals_generic(ctx, B, with_skip):
    rng = np.random.default_rng(100 + B + with_skip)
    x = relu_like(rng, (B, 35, 35, 32))
    w, bias, g, bt = layer_params(rng, 32, 32)
    skip = relu_like(rng, (B, 35, 35, 32)) if with_skip else None
    kw = dict(skip=skip, skip_mode=1 if with_skip else 0)
    own, _ = ctx.debug_conv(x, w, bias, g, bt, **kw)
    gen, _ = ctx.debug_conv(x, w, bias, g, bt, force_generic=True, **kw)
    assert np.array_equal(own, gen)
    r = R.layer(x, w, bias, g, bt, **kw)
    j = R.judge(gen, r, R.layer_fp32(x, w, bias, g, bt, **kw), False)
    print("c32 B=%d skip=%d: A worst %.4f ratio %.3f" % (B, with_skip, j["a_worst"], j["ratio"]))
    assert j["a_ok"] and j["b_ok"], j


# ---- c. the shape sweep ------------------------------------------------------------------------------------------------------------
def sweep_cases():
    """(id, dict): B, H, W, cin, cout, stride, pad, skip ("none" | "same" | ("avg", XH, XW, XC)), generic, gamma, beta"""
    cases = []

    def add(tag, **kw):
        d = dict(B=1, H=4, W=4, cin=64, cout=64, stride=1, pad=1, skip="none", generic=False, gamma="pos", beta=0.05)
        d.update(kw)
        cases.append(("%s-B%d-%dx%d-%d-%d" % (tag, d["B"], d["H"], d["W"], d["cin"], d["cout"]), d))

    # output maps of 1 .. 1225 pixels; M = B OH OW below one row tile, one tile and a bit, and with a prime number of faces.
    # Row tiles: 128 (Cout a multiple of 64: conv_tile_k<2,2>), 256 (Cout 32: <4,1>)
    for side in (1, 2, 3, 4, 8, 17, 35):
        hw = side * side
        for cout, tile in ((64, 128), (32, 256)):
            if side == 35 and cout == 32:
                continue                                 # (that shape: the generic-kernel cases below)
            below, past = max(1, (tile - 1) // hw), (tile + hw) // hw
            for B in sorted({below, past, 7 if hw > 16 else 131}):
                add("map", B=B, H=side, W=side, cin=32 if side >= 17 else 64, cout=cout, skip="same" if (B + side) % 2 else "none")
    # tiles that straddle 2, 3, 32 and 128 faces
    add("straddle2", B=5, H=8, W=8)
    add("straddle3", B=11, H=7, W=7)
    add("straddle32", B=96, H=2, W=2, skip="same")
    add("straddle32", B=96, H=2, W=2, cin=256, cout=256, skip="same")
    add("straddle128", B=300, H=1, W=1, skip="same")
    add("straddle64", B=200, H=2, W=2, cin=32, cout=32, skip="same")
    # the down-sampling units: the stride-2 `a` layer, then the `b` layer with the averaged, zero-extended skip (AH < OH for 8 and 4)
    for H, B in ((35, 3), (17, 5), (8, 9), (4, 37), (3, 50)):
        ah, sh = 1 + (H - 3) // 2, H // 2
        for cin, cout in ((32, 64), (64, 128), (128, 256), (64, 64)):
            if H == 35 and cin > 64:
                continue
            add("down-a", B=B, H=H, W=H, cin=cin, cout=cout, stride=2, pad=0)
            add("down-b", B=B, H=ah, W=ah, cin=cout, cout=cout, skip=("avg", H, H, cin))
        add("down-ab", B=B, H=H, W=H, cin=64, cout=128, stride=2, pad=0, skip=("avg", H, H, 64))     # both in one layer
    add("down-b32", B=9, H=3, W=3, cin=32, cout=32, skip=("avg", 8, 8, 32))
    # channel counts, Cout == 32 off the 35 x 35 shape and on it through the generic kernel
    for cin in (32, 64, 128, 256):
        for cout in (32, 64, 128, 256):
            add("chan", B=3, H=9, W=9, cin=cin, cout=cout, skip="same" if cin == cout else "none")
    add("generic35", B=2, H=35, W=35, cin=32, cout=32, generic=True, skip="same")
    add("generic35", B=1, H=35, W=35, cin=32, cout=32, generic=True)
    add("c32own", B=3, H=35, W=35, cin=32, cout=32, skip="same")
    add("c32own", B=103, H=35, W=35, cin=32, cout=32)
    # maps that are not square
    add("column", B=7, H=9, W=1)
    add("row", B=7, H=1, W=9, skip="same")
    add("column", B=40, H=5, W=1, cin=32, cout=32)
    add("oblong", B=3, H=5, W=12, cin=128, cout=64, stride=2, pad=0)
    # the affine map
    for gamma, beta in (("neg", 0.05), ("zero", 0.05), ("mixed", 3), ("pos", -3), ("neg", 3)):
        add("affine-%s-%s" % (gamma, beta), B=5, H=8, W=8, gamma=gamma, beta=beta, skip="same")
        add("affine32-%s-%s" % (gamma, beta), B=5, H=8, W=8, cin=32, cout=32, gamma=gamma, beta=beta)
    return cases


SWEEP = sweep_cases()


def case_inputs(d, seed):
    """a case's tensors: (x, w, bias, gamma, beta), debug_conv's keywords"""
    rng = np.random.default_rng(seed)
    x = relu_like(rng, (d["B"], d["H"], d["W"], d["cin"]))
    w, bias, g, bt = layer_params(rng, d["cin"], d["cout"], 3, d["gamma"], d["beta"])
    kw = dict(stride=d["stride"], pad=d["pad"])
    ah, aw = 1 + (d["H"] + 2 * d["pad"] - 3) // d["stride"], 1 + (d["W"] + 2 * d["pad"] - 3) // d["stride"]
    if d["skip"] == "same":
        kw.update(skip=relu_like(rng, (d["B"], ah, aw, d["cout"])), skip_mode=1)
    elif d["skip"] != "none":
        _, xh, xw, xc = d["skip"]
        kw.update(skip=relu_like(rng, (d["B"], xh, xw, xc)), skip_mode=2)
    return (x, w, bias, g, bt), kw


def run_case(ctx, d, split, seed):
    (x, w, bias, g, bt), kw = case_inputs(d, seed)
    y, flags = ctx.debug_conv(x, w, bias, g, bt, split=split, force_generic=d["generic"], **kw)
    r = R.layer(x, w, bias, g, bt, **kw)
    assert y.shape == r["y"].shape
    # conv3x3_c32_k's shape keeps its exact kernel in the product whatever `split` says
    own = d["cin"] == 32 and d["cout"] == 32 and not d["generic"]
    use_split = split and not own
    cpu = (R.layer_split if use_split else R.layer_fp32)(x, w, bias, g, bt, **kw)
    return R.judge(y, r, cpu, use_split), flags


def sweep_crcs(ctx, split):
    """"<k>-<case id>" (five ids occur twice) -> [crc32 of the output's bytes, crc32 of the flags' bytes] (hex) over SWEEP, with
    test_shape_sweep's inputs"""
    out = {}
    for k, (cid, d) in enumerate(SWEEP):
        par, kw = case_inputs(d, 1000 + k)
        y, flags = ctx.debug_conv(*par, split=split, force_generic=d["generic"], **kw)
        out["%03d-%s" % (k, cid)] = ["%08x" % zlib.crc32(y.tobytes()), "%08x" % zlib.crc32(flags.tobytes())]
    return out


@pytest.mark.parametrize("split", [False, True])
def test_shape_sweep(ctx, split):
    bad = []
    for k, (cid, d) in enumerate(SWEEP):
        j, flags = run_case(ctx, d, split, 1000 + k)
        print("%-34s %-5s A worst %.4f  rms gpu %.3e cpu %.3e ratio %.3f" % (cid, "split" if split else "exact", j["a_worst"], j["rms_y"], j["rms_cpu"], j["ratio"]))
        if not (j["a_ok"] and j["b_ok"]) or flags.any():
            bad.append((cid, j, flags.nonzero()))
    assert not bad, bad


@pytest.mark.parametrize("split", [False, True])
def test_sweep_bits_are_the_parents(ctx, split):
    """every bit the sweep's layers write, against tests/golden/conv_sweep_crc32.json: recorded once on the MI355X from the commit its
    _meta entry names, with these inputs (the generator's stream belongs to the numpy version named there)"""
    with open(os.path.join(ROOT, "tests", "golden", "conv_sweep_crc32.json")) as f:
        golden = json.load(f)
    want = golden["split" if split else "exact"]
    got = sweep_crcs(ctx, split)
    assert sorted(want) == sorted(got)
    differ = [key for key in sorted(got) if got[key] != want[key]]
    assert not differ, (golden["_meta"], "numpy here: " + np.__version__, differ)


def test_sweep_covers_what_it_says():
    """a condition on the case list itself (no GPU work): the tile geometries the sweep is there for are in it"""
    def tiles(d):
        tile = 256 if d["cout"] == 32 else 128
        ah, aw = 1 + (d["H"] + 2 * d["pad"] - 3) // d["stride"], 1 + (d["W"] + 2 * d["pad"] - 3) // d["stride"]
        oh, ow = (max(ah, d["skip"][1] // 2), max(aw, d["skip"][2] // 2)) if isinstance(d["skip"], tuple) else (ah, aw)
        return tile, oh * ow, d["B"] * oh * ow, (ah, oh)
    t = [tiles(d) for _, d in SWEEP]
    assert {hw for _, hw, _, _ in t} >= {1, 4, 9, 16, 64, 289, 1225}
    assert any(M < tile for tile, _, M, _ in t) and any(tile < M < 2 * tile and M % tile for tile, _, M, _ in t)
    assert any(tile // hw >= 32 and M > tile for tile, hw, M, _ in t)
    assert any(ah < oh for _, _, _, (ah, oh) in t) and any(ah == oh and isinstance(d["skip"], tuple) for (_, d), (_, _, _, (ah, oh)) in zip(SWEEP, t))
    assert any(d["cout"] == 32 and d["generic"] for _, d in SWEEP) and any(d["cout"] == 32 and d["H"] != 35 for _, d in SWEEP)
    assert any(isinstance(d["skip"], tuple) and d["skip"][3] < d["cout"] for _, d in SWEEP) and any(isinstance(d["skip"], tuple) and d["skip"][3] == d["cout"] for _, d in SWEEP)


def test_refused_shape_is_an_error_and_the_context_goes_on(ctx):
    rng = np.random.default_rng(9)
    for cin, cout in ((48, 64), (64, 96), (64, 48)):
        x = relu_like(rng, (2, 4, 4, cin))
        w, bias, g, bt = layer_params(rng, cin, cout)
        with pytest.raises(Exception, match="conv"):
            ctx.debug_conv(x, w, bias, g, bt)
    j, _ = run_case(ctx, dict(B=2, H=4, W=4, cin=64, cout=64, stride=1, pad=1, skip="none", generic=False, gamma="pos", beta=0.05), False, 3)
    assert j["a_ok"] and j["b_ok"]


# ---- d. head_k ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [1, 4])
def test_head(ctx, params, hw):
    """feat = fl(sum over HW) / HW: (HW + 1) u mean|x|; the 256-long product: (256 + 4) u sum |feat||fc| plus what feat's error carries"""
    rng = np.random.default_rng(40 + hw)
    x = relu_like(rng, (37, hw, 256))
    x[-1] = 0.0
    x[-1, hw - 1, 255] = 3.0
    out = ctx.embed_head(x)
    fc = np.asarray(params["fc.w"], np.float64)
    feat = x.astype(np.float64).mean(axis=1)
    ef = (hw + 1) * R.U * np.abs(x.astype(np.float64)).mean(axis=1)
    bound = ef @ np.abs(fc) + (256 + 4) * R.U * (np.abs(feat) @ np.abs(fc)) + 2.0 ** -124
    err = np.abs(out - feat @ fc)
    print("head hw=%d: worst err / bound %.4f" % (hw, (err / bound).max()))
    assert np.all(err <= bound)
    assert np.abs(out[-1]).max() > 0


# ---- e. the range guard marks the right face ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,B", [(64, 64, 96), (256, 256, 96), (64, 32, 200)])
def test_range_flag_goes_to_its_face(ctx, cin, cout, B):
    """2 x 2 maps: a 128-row tile holds 32 faces (a 256-row tile of the Cout = 32 kernel 64)"""
    rng = np.random.default_rng(77)
    x0 = relu_like(rng, (B, 2, 2, cin))
    w, bias, g, bt = layer_params(rng, cin, cout)
    faces = [0, 31, 32, 95] + ([63, 64, 199] if B > 96 else [])
    for j in faces:
        for value, want in ((256.0, {j}), (float("nan"), {j}), (-256.0, {j}), (255.8, set())):
            x = x0.copy()
            x[j, (j // 2) % 2, j % 2, (7 * j + 5) % cin] = value
            _, flags = ctx.debug_conv(x, w, bias, g, bt, split=True)
            assert set(np.nonzero(flags)[0].tolist()) == want, (j, value, np.nonzero(flags)[0])
    x = x0.copy()
    x[5, 1, 1, 3] = 300.0
    x[B - 1, 0, 0, 0] = 1e6
    _, flags = ctx.debug_conv(x, w, bias, g, bt, split=True)
    assert set(np.nonzero(flags)[0].tolist()) == {5, B - 1}
    _, flags = ctx.debug_conv(x, w, bias, g, bt, split=False)
    assert not flags.any()


def guard_chips():
    rng = np.random.default_rng(21)
    base = rng.integers(0, 256, (16, 150, 150, 3)).astype(np.float64)
    amp = np.where(np.arange(16) % 2 == 0, 1.0, 1.0 / 32)       # every other chip has next to no contrast
    return np.clip(np.rint(118.0 + (base - 118.0) * amp[:, None, None, None]), 0, 255).astype(np.uint8)


def test_range_guard_reruns_the_flagged_faces_only(tmp_path):
    """u4.a's weights are scaled, by a power of two chosen HERE from the f64 stages, so that some of 16 chips leave the split layers'
    range (an input of 65504 / 2^8 or more) and the others stay inside, every chip by a factor 2 at least"""
    from pyannote_video_amd.runtime import Context
    chips = guard_chips()
    m = models.make_embedder()
    limit = R.F16_LIMIT / 2.0 ** R.A_EXP
    chosen = None
    for e in (8, 7, 9, 6, 10):
        params = models.split_resnet_blob(m["emb.blob"].copy())
        params["u4.a.w"] = params["u4.a.w"] * np.float32(2.0 ** e)
        st = R.stages(chips, params)
        specs = R.layer_specs(params, models.RESNET_UNITS)
        mx = np.zeros(len(chips))
        for name, kind, a in specs:
            if kind == "conv" and R.is_split_layer(a["w"]):
                mx = np.maximum(mx, np.abs(st[a["input"]]).reshape(len(chips), -1).max(axis=1))
        over, under = mx >= 2 * limit, mx <= limit / 2
        if np.all(over | under) and 0 < over.sum() < len(chips):
            chosen = (e, over)
            break
    assert chosen is not None, "no scale separates the chips by a factor 2 on both sides"
    e, over = chosen
    blob = np.array(m["emb.blob"], np.float32)
    o = 0
    for name, shape in models.resnet_param_layout():
        n = int(np.prod(shape))
        if name == "u4.a.w":
            blob[o:o + n] *= np.float32(2.0 ** e)
        o += n
    m["emb.blob"] = blob
    path = str(tmp_path / "scaled.pvfm")
    models.save_container(path, m)

    def make(split):
        c = Context(0)
        c.load_embedder(path)
        c.embedder_split(split)
        return c
    cx, cs = make(False), make(True)
    exact = cx.embed_chips(chips)
    split = cs.embed_chips(chips)
    st = cs.embedder_split_stats()
    print("scale 2^%d: %d of %d chips over the range" % (e, int(over.sum()), len(chips)))
    assert st["reruns"] == int(over.sum()) and st["faces"] == len(chips)
    _, flags = cs.embed_stage(chips, 29, True)
    assert np.array_equal(flags != 0, over)
    for i in range(len(chips)):
        assert np.array_equal(split[i], exact[i]) == bool(over[i]), i
    cx.close()
    cs.close()


# ---- f. denormals and big values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_denormals_and_big_values(ctx, split):
    rng = np.random.default_rng(61)
    B, cin, cout = 5, 64, 64
    w, bias, g, bt = layer_params(rng, cin, cout)
    x = relu_like(rng, (B, 8, 8, cin))
    cases = {
        "subnormal inputs": (np.where(x != 0, np.float32(1e-40), np.float32(0.0)).astype(np.float32), w),
        "subnormal products": (np.where(x != 0, np.float32(1e-40), np.float32(0.0)).astype(np.float32), (np.sign(w) * np.float32(1e-30)).astype(np.float32)),
        "tiny weights": (x, (np.sign(w) * np.float32(1e-30)).astype(np.float32)),
        "activations of 200": (np.where(x != 0, np.float32(200.0), np.float32(0.0)).astype(np.float32), w),
        "mixed magnitudes": ((np.sign(x) * np.float32(200.0) * (rng.random(x.shape) < 0.1) + x * np.float32(1e-6)).astype(np.float32), w),
    }
    for what, (xx, ww) in cases.items():
        for zero_affine in (False, True):
            b2, bt2 = (np.zeros_like(bias), np.zeros_like(bt)) if zero_affine else (bias, bt)
            y, flags = ctx.debug_conv(xx, ww, b2, g, bt2, split=split)
            r = R.layer(xx, ww, b2, g, bt2)
            cpu = (R.layer_split if split else R.layer_fp32)(xx, ww, b2, g, bt2)
            j = R.judge(y, r, cpu, split)
            print("%-20s affine %d %-5s A worst %.4f rms gpu %.3e cpu %.3e" % (what, not zero_affine, "split" if split else "exact", j["a_worst"], j["rms_y"], j["rms_cpu"]))
            assert j["a_ok"], (what, j)
            assert not flags.any(), what


# ---- g. other weight sets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wset", sorted(WEIGHT_SETS))
@pytest.mark.parametrize("split", [False, True])
def test_every_stage_other_weights(tmp_path, wset, split):
    from pyannote_video_amd.runtime import Context
    m = models.make_embedder(**WEIGHT_SETS[wset])
    path = str(tmp_path / (wset + ".pvfm"))
    models.save_container(path, m)
    c = Context(0)
    try:
        c.load_embedder(path)
        judge_net(c, batch(7), models.split_resnet_blob(m["emb.blob"]), split, "%s %s" % (wset, "split" if split else "exact"))
    finally:
        c.close()


# ---- h. the descriptor against f64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_descriptor_against_f64(ctx, params, split):
    chips = batch(7)
    ctx.embedder_split(split)
    try:
        gpu = ctx.embed_chips(chips).astype(np.float64)
    finally:
        ctx.embedder_split(True)
    ref = R.descriptor(R.stages(chips, params)[-1], params)
    _, _, cpu = R.emulate(chips, params, split)
    l2_gpu, l2_cpu = np.linalg.norm(gpu - ref, axis=1), np.linalg.norm(cpu - ref, axis=1)
    print("descriptor L2 against f64 (%s): gpu %s\n cpu %s" % ("split" if split else "exact", l2_gpu, l2_cpu))
    assert R.rms(l2_gpu) <= R.B_FACTOR * R.rms(l2_cpu)
    assert l2_gpu.max() <= 1e-4
