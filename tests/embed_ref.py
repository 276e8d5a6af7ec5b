"""The face embedder (csrc/resnet.hip) layer by layer on the CPU: an f64 reference of every stage, ONE layer in f64 with the sums the
error bounds need, the same layer in the arithmetic the kernels intend (fp32; f16 split operands), and the two criteria a layer's
output is held to.  NHWC numpy arrays in and out; torch does the convolutions.

Criterion A (per element, derived; u = 2^-24, K = taps x input channels, S = sum |x||w| of the output's products, z the f64 value
before the ReLU, which is 1-Lipschitz and so passes every bound through):

  exact kernels   acc = fl(sum of K fp32 products), every product rounded once and carried through at most K - 1 additions:
                  |acc - sum| <= K u S to first order.  Then t1 = fl(acc + bias), t2 = fl(t1 g), t3 = fl(t2 + beta), t4 = fl(t3 + skip):
                  the first two roundings are relative to (S + |bias|)|g| at most, which with the second-order terms gives
                  (K + 4) u (S + |bias|) |g|; the last two are relative to |t3| <= |z| + |skip| and |t4| ~ |z|: 2 u (|z| + |skip|).
                  The averaged skip (((q0 + q1) + q2) + q3) / 4 rounds three times: 3 u mean|q| (4 u with the second order).
  split kernels   DESIGN.md section 4: a product as hi.hi + hi.lo + lo.hi of f16 halves misses at most 3 2^-22 |xw| (+ the
                  subnormal term), the 3K terms' accumulation in the matrix pipe at most 3K 2^-22 of their magnitudes (<= S (1 + 2^-10)):
                  (3 + 3K) 2^-22 S (1 + 2^-10); the power-of-two scales are exact.  Subnormal term, f16 subnormals flushed at worst:
                  2^-14 on each scaled operand, i.e. per product 2^-14 (|x| 2^-e + |w| 2^-8) after the scales are undone.
                  The epilogue is the exact kernels': 4 u (S + |bias|) |g| + 2 u (|z| + |skip|) (+ the averaged skip's 4 u mean|q|).
  fp32 subnormals an operand, a product or a result below 2^-126 may read or come out as zero: K 2^-126 (1 + max|w| + max|x|) |g| + 2^-124.

Criterion B (per layer): rms(y - y_f64) <= 4 rms(y_same_arithmetic_on_the_CPU - y_f64) on the same input; the factor covers another
accumulation order, nothing else."""
import numpy as np
import torch
import torch.nn.functional as F

A_EXP = 8                                   # EMB_A_SCALE_EXP
F16_LIMIT = 65504.0
U = 2.0 ** -24
MEAN = (122.782, 117.001, 104.298)
B_FACTOR = 4.0

torch.set_flush_denormal(False)


def w_exp_of(w):
    """conv_layer_upload: the power of two that puts the largest |w| in [2^14, 2^15)"""
    m = float(np.abs(np.asarray(w, np.float32)).max())
    return 15 - int(np.frexp(np.float32(m))[1]) if m > 0 and np.isfinite(m) else 0


def _nchw(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dt).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _avg4(s):
    """(((q0 + q1) + q2) + q3) / 4 over 2 x 2 windows, stride 2, in the tensor's own type (the kernel's order)"""
    h, w = s.shape[2] // 2, s.shape[3] // 2
    q = lambda dy, dx: s[:, :, dy:2 * h:2, dx:2 * w:2]
    return (((q(0, 0) + q(0, 1)) + q(1, 0)) + q(1, 1)) * 0.25


def _conv(x, w, stride, pad, arith, terms=(1, 1, 1)):
    """x NCHW tensor (f64 for "f64", else fp32), w OIHW fp32 tensor -> the convolution sums in `arith`, as that type's tensor"""
    if arith == "f64":
        return F.conv2d(x, w.double(), None, stride=stride, padding=pad)
    if arith == "fp32":
        return F.conv2d(x, w, None, stride=stride, padding=pad)
    assert arith == "split"
    e = w_exp_of(w.numpy())

    def halves(v):
        hi = v.to(torch.float16)
        lo = (v - hi.float()).to(torch.float16)
        return hi.float(), lo.float()
    xh, xl = halves(x * 2.0 ** A_EXP)
    wh, wl = halves(w * 2.0 ** e)
    c = lambda a, b: F.conv2d(a, b, None, stride=stride, padding=pad)      # f16 x f16 products are exact in fp32; fp32 accumulation
    acc = c(xh, wh) * float(terms[0])
    acc = acc + c(xh, wl) * float(terms[1])
    acc = acc + c(xl, wh) * float(terms[2])
    return acc * np.float32(2.0 ** -(A_EXP + e))


def _layer(x, w, bias, g, beta, stride, pad, skip, skip_mode, out_hw, arith, fault=None):
    """fault (tests/test_embed_layer_criteria.py: deliberate defects, to show that the criteria see them): a dict with any of `terms`
    (which of the three split terms are kept), `conv` (acc -> acc), `avg` (replaces the 2 x 2 average), `extend` (value written where
    the output is zero-extended: a function of (bias, g, beta) tensors)"""
    fault = fault or {}
    dt = torch.float64 if arith == "f64" else torch.float32
    xt, wt = _nchw(x, dt), torch.from_numpy(np.ascontiguousarray(w, np.float32))      # (an f64 input stays f64 in the f64 layer)
    v = lambda p: torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dt)[None, :, None, None]
    acc = _conv(xt, wt, stride, pad, arith, fault.get("terms", (1, 1, 1)))
    if "conv" in fault:
        acc = fault["conv"](acc, xt, wt)
    t = ((acc + v(bias)) * v(g)) + v(beta)
    B, cout, ah, aw = t.shape
    s = None
    if skip_mode == 1:
        s = _nchw(skip, dt)
    elif skip_mode == 2:
        s = fault.get("avg", _avg4)(_nchw(skip, dt))
    oh, ow = out_hw if out_hw is not None else ((max(ah, s.shape[2]), max(aw, s.shape[3])) if s is not None else (ah, aw))
    z = torch.zeros(B, cout, oh, ow, dtype=dt)
    if "extend" in fault:
        z = z + fault["extend"](v(bias), v(g), v(beta))
    z[:, :, :ah, :aw] = t
    sk = torch.zeros(B, cout, oh, ow, dtype=dt)
    if s is not None:
        sk[:, :s.shape[1], :s.shape[2], :s.shape[3]] = s
        z = z + sk
    return z, sk, (ah, aw)


def layer(x, w, bias, g, beta, stride=1, pad=1, skip=None, skip_mode=0, out_hw=None):
    """ONE layer in f64 on the given input.  Returns a dict: y (after the ReLU), z (before it), S (sum |x||w| per output, zero where
    the output is zero-extended), skip (the value added), skip_abs (mean |q| of an averaged skip, else zero), sx (sum of |x| under the
    window), all [B, OH, OW, Cout] f64; K, w_exp, sw (sum |w| per channel), xmax, wmax."""
    z, sk, (ah, aw) = _layer(x, w, bias, g, beta, stride, pad, skip, skip_mode, out_hw, "f64")
    xa, wa = _nchw(np.abs(np.asarray(x, np.float64)), torch.float64), torch.from_numpy(np.abs(np.asarray(w, np.float64)))
    S = torch.zeros_like(z)
    S[:, :, :ah, :aw] = F.conv2d(xa, wa, None, stride=stride, padding=pad)
    sx = torch.zeros_like(z)
    sx[:, :, :ah, :aw] = F.conv2d(xa, torch.ones(1, wa.shape[1], wa.shape[2], wa.shape[3], dtype=torch.float64), None, stride=stride, padding=pad)
    sa = torch.zeros_like(z)
    if skip_mode == 2:
        q = F.avg_pool2d(_nchw(np.abs(np.asarray(skip, np.float64)), torch.float64), 2, 2, 0)
        sa[:, :q.shape[1], :q.shape[2], :q.shape[3]] = q
    valid = torch.zeros_like(z)
    valid[:, :, :ah, :aw] = 1.0
    w32 = np.asarray(w, np.float32)
    return {"y": _nhwc(F.relu(z)), "z": _nhwc(z), "S": _nhwc(S), "skip": _nhwc(sk), "skip_abs": _nhwc(sa), "sx": _nhwc(sx), "valid": _nhwc(valid),
            "K": int(w32.shape[1] * w32.shape[2] * w32.shape[3]), "w_exp": w_exp_of(w32), "sw": np.abs(w32.astype(np.float64)).sum(axis=(1, 2, 3)),
            "bias": np.asarray(bias, np.float64), "g": np.asarray(g, np.float64),
            "xmax": float(np.abs(np.asarray(x, np.float64)).max()), "wmax": float(np.abs(w32).max())}


def layer_fp32(x, w, bias, g, beta, stride=1, pad=1, skip=None, skip_mode=0, out_hw=None, fault=None):
    """the same layer with fp32 products, accumulation and epilogue (the exact kernels' arithmetic, torch's order): y, f64 array"""
    z, _, _ = _layer(x, w, bias, g, beta, stride, pad, skip, skip_mode, out_hw, "fp32", fault)
    return _nhwc(F.relu(z)).astype(np.float64)


def layer_split(x, w, bias, g, beta, stride=1, pad=1, skip=None, skip_mode=0, out_hw=None, fault=None):
    """the same layer as conv_tile_k<.., ConvSplit> intends it: hi.hi + hi.lo + lo.hi of the f16 halves of 2^8 x and 2^w_exp w, fp32 accumulation, the
    exact power-of-two scale back, the fp32 epilogue"""
    z, _, _ = _layer(x, w, bias, g, beta, stride, pad, skip, skip_mode, out_hw, "split", fault)
    return _nhwc(F.relu(z)).astype(np.float64)


def bound_a(r, split):
    """criterion A's per-element bound for the layer described by r = layer(...)"""
    K = r["K"]
    g, bias = np.abs(r["g"]), np.abs(r["bias"])
    sb = (r["S"] + bias * r["valid"]) * g
    tail = 2 * U * (np.abs(r["z"]) + np.abs(r["skip"])) + 4 * U * r["skip_abs"]
    sub = (K * 2.0 ** -126 * (1.0 + r["wmax"] + r["xmax"])) * g + 2.0 ** -124
    if not split:
        return (K + 4) * U * sb + tail + sub
    sub16 = 2.0 ** -14 * (2.0 ** -r["w_exp"] * r["sx"] + 2.0 ** -A_EXP * r["sw"] * r["valid"])
    return ((3 + 3 * K) * 2.0 ** -22 * (1 + 2.0 ** -10) * r["S"] + sub16) * g + 4 * U * sb + tail + sub


def rms(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def judge(y, r, y_cpu, split):
    """y against the f64 layer r under both criteria: dict with a_ok, a_worst (largest |error| / bound), b_ok, rms_y, rms_cpu, ratio"""
    y = np.asarray(y, np.float64)
    err = np.abs(y - r["y"])
    bound = bound_a(r, split)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(err > 0, err / bound, 0.0)
    a_ok = bool(np.all(np.isfinite(y)) and np.all(err <= bound))
    e_y, e_c = rms(y - r["y"]), rms(y_cpu - r["y"])
    return {"a_ok": a_ok, "a_worst": float(np.nanmax(rel)) if rel.size else 0.0, "b_ok": bool(e_y <= B_FACTOR * e_c), "rms_y": e_y, "rms_cpu": e_c,
            "ratio": (e_y / e_c) if e_c > 0 else (0.0 if e_y == 0 else float("inf"))}


# ---- the whole network --------------------------------------------------------------------------------------------------------
def stem_input(chips_u8):
    """(byte - mean) / 256 in fp32, as stem_conv_k converts: [n, 150, 150, 3] float32"""
    return ((np.asarray(chips_u8, np.uint8).reshape(-1, 150, 150, 3).astype(np.float32) - np.array(MEAN, np.float32)) / np.float32(256.0)).astype(np.float32)


def maxpool(x):
    """3 x 3 stride 2, no padding; exact in any type"""
    return _nhwc(F.max_pool2d(_nchw(x, torch.float64), 3, 2, 0))


def layer_specs(params, units):
    """the 30 stages in order: (name, kind, arguments): kind "stem" | "pool" | "conv" with the keyword arguments of layer() (skip: the
    index of the stage whose output is the skip tensor, or None) and `input`: the index of the stage it reads (-1: the chips)"""
    specs = [("stem", "stem", dict(w=params["conv1.w"], bias=params["conv1.b"], g=params["aff1.g"], beta=params["aff1.b"], stride=2, pad=0, input=-1)),
             ("pool", "pool", dict(input=0))]
    prev = 1
    for u, (cin, n, down) in enumerate(units):
        p = "u%d." % u
        ia, ib = 2 + 2 * u, 3 + 2 * u
        specs.append((p + "a", "conv", dict(w=params[p + "a.w"], bias=params[p + "a.b"], g=params[p + "a.g"], beta=params[p + "a.beta"],
                                            stride=2 if down else 1, pad=0 if down else 1, skip_from=None, skip_mode=0, input=prev)))
        specs.append((p + "b", "conv", dict(w=params[p + "b.w"], bias=params[p + "b.b"], g=params[p + "b.g"], beta=params[p + "b.beta"],
                                            stride=1, pad=1, skip_from=prev, skip_mode=2 if down else 1, input=ia)))
        prev = ib
    return specs


def is_split_layer(w):
    """whether the product runs this layer on conv_tile_k<.., ConvSplit> when the split path is on (everything but the first layer and the 32 -> 32 stage)"""
    return not (w.shape[0] == 32 and w.shape[1] in (3, 32))


def stage_kwargs(spec, inputs):
    """(x, positional parameters, keyword arguments) of layer() / layer_fp32() / layer_split() for a "stem" or "conv" stage"""
    name, kind, a = spec
    kw = dict(stride=a["stride"], pad=a["pad"])
    if kind == "conv" and a["skip_from"] is not None:
        kw.update(skip=inputs[a["skip_from"]], skip_mode=a["skip_mode"])
    return inputs[a["input"]], (a["w"], a["bias"], a["g"], a["beta"]), kw


def run_stage(spec, inputs, arith="f64"):
    """one stage of layer_specs on the given stage outputs (inputs[i]: stage i, inputs[-1]: stem_input of the chips): its y"""
    name, kind, a = spec
    x = inputs[a["input"]]
    if kind == "pool":
        return maxpool(x)
    kw = dict(stride=a["stride"], pad=a["pad"])
    if kind == "conv" and a["skip_from"] is not None:
        kw.update(skip=inputs[a["skip_from"]], skip_mode=a["skip_mode"])
    fn = {"f64": lambda *p, **k: layer(*p, **k)["y"], "fp32": layer_fp32, "split": layer_split}[arith]
    return fn(x, a["w"], a["bias"], a["g"], a["beta"], **kw)


def stages(chip_u8, params, units=None):
    """every stage of the network in f64 on one chip (or a batch): list of 30 arrays [n, H, W, C]; descriptor(stages[-1], params) ends it"""
    if units is None:
        from pyannote_video_amd import models
        units = models.RESNET_UNITS
    outs = {-1: stem_input(chip_u8)}
    specs = layer_specs(params, units)
    for i, spec in enumerate(specs):
        outs[i] = run_stage(spec, outs, "f64")
    return [outs[i] for i in range(len(specs))]


def descriptor(last, params):
    """average over the last map, then the 256 -> 128 product, f64"""
    feat = np.asarray(last, np.float64).mean(axis=(1, 2))
    return feat @ np.asarray(params["fc.w"], np.float64)


def emulate(chips, params, split, faults=None, units=None):
    """The forward as the kernels intend it (fp32, or split where the product splits), every layer on the previous layer's fp32 output
    and judged ALONE against the f64 layer on that same input -- what tests/test_gpu_embed_layers.py does with the GPU's stages.
    faults: {stage index: {"fault": embed_ref fault, "inputs": (x, kw) -> (x, kw), "post": (y, clean) -> y}}.
    Returns (stage outputs, [(stage, name, judgement)], descriptors)."""
    faults = faults or {}
    if units is None:
        from pyannote_video_amd import models
        units = models.RESNET_UNITS
    specs = layer_specs(params, units)
    outs = {-1: stem_input(chips)}
    table = []
    for i, spec in enumerate(specs):
        name, kind, a = spec
        if kind == "pool":
            outs[i] = maxpool(outs[a["input"]]).astype(np.float32)
            continue
        x, par, kw = stage_kwargs(spec, outs)
        use_split = split and is_split_layer(a["w"])
        fn = layer_split if use_split else layer_fp32
        clean = fn(x, *par, **kw)
        y = clean
        f = faults.get(i)
        if f is not None:
            xin, kwin = f["inputs"](x, dict(kw)) if "inputs" in f else (x, kw)
            y = fn(xin, *par, fault=f.get("fault"), **kwin)
            if "post" in f:
                y = f["post"](y.copy(), clean)
        table.append((i, name, judge(y, layer(x, *par, **kw), clean, use_split)))
        outs[i] = y.astype(np.float32)
    return outs, table, descriptor(outs[len(specs) - 1], params)
