"""num_jitters restated (JITTER.md): the plan of the J transforms in Python integers and math.cos / math.sin, the jittered chip as the
oracle's extract_chip followed by the mirror, and the fp32 mean of the J descriptors."""
import math
import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def mix(x):
    z = x & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def u(seed, j, k):
    return float(mix((seed + (5 * j + k + 1) * GOLD) & M64) >> 11) * 2.0 ** -53


def plan_row(seed, j):
    """{"rect": (l, t, r, b), "cs", "sn", "flip", and the raw draws "tx", "ty", "s", "box", "angle"} of jitter j"""
    tx = (-0.02 + u(seed, j, 0) * 0.04) * 144.0
    ty = (-0.02 + u(seed, j, 1) * 0.04) * 144.0
    s = 0.97 + u(seed, j, 2) * (0.99999 - 0.97)
    box = 144.0 / s
    angle = (-3.0 + u(seed, j, 3) * 6.0) * math.pi / 180.0
    flip = u(seed, j, 4) > 0.5
    rect = (75 + tx - box / 2, 75 + ty - box / 2, 75 + tx + box / 2, 75 + ty + box / 2)
    return {"rect": rect, "cs": math.cos(angle), "sn": math.sin(angle), "flip": bool(flip), "tx": tx, "ty": ty, "s": s, "box": box, "angle": angle}


def plan(J, seed=0):
    return [plan_row(seed, j) for j in range(J)]


def row_of_library(row):
    """a row of _lib.jitter_plan (l t r b cs sn flip m[4] b[2] bx0 by0 sw sh) in the form jitter() takes"""
    return {"rect": tuple(float(v) for v in row[:4]), "cs": float(row[4]), "sn": float(row[5]), "flip": bool(row[6] != 0.0)}


def jitter(oracle, chip, row):
    """oracle.extract_chip(chip, rect, cs, sn, 150, 150), then the mirror: output column c takes extracted column 149 - c"""
    chip = np.ascontiguousarray(chip, np.uint8).reshape(150, 150, 3)
    out = oracle.extract_chip(chip, row["rect"], row["cs"], row["sn"], 150, 150)
    return np.ascontiguousarray(out[:, ::-1]) if row["flip"] else out


def mean32(d):
    """acc = 0; for j ascending: acc += d[j]; acc / float32(J) -- in fp32, over axis -2 of [..., J, 128]"""
    d = np.asarray(d, np.float32)
    acc = np.zeros(d.shape[:-2] + d.shape[-1:], np.float32)
    for j in range(d.shape[-2]):
        acc = acc + d[..., j, :]
    return acc / np.float32(d.shape[-2])


def ulps(a, b):
    """distance of two float64 in units of the last place"""
    ia = np.asarray(a, np.float64).view(np.int64).astype(object)
    ib = np.asarray(b, np.float64).view(np.int64).astype(object)
    fix = np.vectorize(lambda v: v if v >= 0 else -(v & 0x7FFFFFFFFFFFFFFF), otypes=[object])
    return np.abs(fix(ia) - fix(ib)).astype(np.float64)
