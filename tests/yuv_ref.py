"""The project's YUV -> RGB conversion restated in numpy ("YUV to RGB"), independent of the package, plus
what the YUV tests need to make input: an RGB -> YUV formula (any will do: it only makes input) and a YUV4MPEG2 writer.

    limited range:  C = 76309 * (Y - 16) + 32768            76309 = (65536 * 255) // 219
    full range:     C = 65536 * Y + 32768
    R = clip8((C + crv * (V - 128)) >> 16)
    G = clip8((C - cgu * (U - 128) - cgv * (V - 128)) >> 16)
    B = clip8((C + cbu * (U - 128)) >> 16)

`>>` floors; pixel (x, y) takes the chroma sample (x >> sx, y >> sy)."""
import numpy as np

SHIFTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
LIMITED = {"601": (104597, 132201, 25675, 53279), "709": (117504, 138453, 13954, 34903)}        # (crv, cbu, cgu, cgv)


def constants(matrix, full_range):
    c = LIMITED[str(matrix)]
    return tuple((v * 224) // 255 for v in c) if full_range else c


def accumulators(Y, U, V, matrix="601", full_range=False):
    """the three int64 values before the shift, for arrays of equal shape"""
    crv, cbu, cgu, cgv = constants(matrix, full_range)
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    C = 65536 * Y + 32768 if full_range else 76309 * (Y - 16) + 32768
    return C + crv * (V - 128), C - cgu * (U - 128) - cgv * (V - 128), C + cbu * (U - 128)


def chroma_shape(h, w, layout):
    sx, sy = SHIFTS[layout]
    return -(-h // (1 << sy)), -(-w // (1 << sx))


def to_rgb(Y, U, V, layout="420", matrix="601", full_range=False):
    """Y [H, W], U and V [ceil(H / 2^sy), ceil(W / 2^sx)] uint8 -> uint8 [H, W, 3]"""
    sx, sy = SHIFTS[layout]
    h, w = Y.shape
    assert U.shape == V.shape == chroma_shape(h, w, layout), (U.shape, V.shape, chroma_shape(h, w, layout))
    iy, ix = np.arange(h) >> sy, np.arange(w) >> sx
    acc = accumulators(Y, np.asarray(U)[iy][:, ix], np.asarray(V)[iy][:, ix], matrix, full_range)
    return np.stack([np.clip(a >> 16, 0, 255) for a in acc], axis=-1).astype(np.uint8)


def from_rgb(rgb, layout="420"):
    """input maker: BT.601 limited-range float arithmetic, chroma averaged over each block.  Not the inverse of anything."""
    sx, sy = SHIFTS[layout]
    r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
    y = 16 + (65.481 * r + 128.553 * g + 24.966 * b) / 255
    u = 128 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255
    v = 128 + (112.0 * r - 93.786 * g - 18.214 * b) / 255
    h, w = y.shape
    ch, cw = chroma_shape(h, w, layout)

    def down(p):
        q = np.pad(p, ((0, (ch << sy) - h), (0, (cw << sx) - w)), mode="edge")
        return q.reshape(ch, 1 << sy, cw, 1 << sx).mean(axis=(1, 3))
    q8 = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)
    return q8(y), q8(down(u)), q8(down(v))


def noise_planes(h, w, layout, seed):
    """uniform noise over all of 0..255 in every plane: all three clamps fire on both sides"""
    rng = np.random.RandomState(seed)
    ch, cw = chroma_shape(h, w, layout)
    return (rng.randint(0, 256, (h, w)).astype(np.uint8), rng.randint(0, 256, (ch, cw)).astype(np.uint8),
            rng.randint(0, 256, (ch, cw)).astype(np.uint8))


def constant_planes(h, w, layout, yuv):
    ch, cw = chroma_shape(h, w, layout)
    return (np.full((h, w), yuv[0], np.uint8), np.full((ch, cw), yuv[1], np.uint8), np.full((ch, cw), yuv[2], np.uint8))


def write_y4m(path, frames, layout="420", rate="25:1", tag=None, extra=(), frame_params=None, truncate=0):
    """frames: [(Y, U, V)].  tag: the C tag's value (default: the layout; None with layout 420 and tag "" writes no C tag at all);
    extra: more header tokens (e.g. "XCOLORRANGE=FULL", "Ip", "A1:1"); frame_params: text after FRAME on every frame line;
    truncate: bytes cut off the end of the file"""
    h, w = frames[0][0].shape
    tok = ["YUV4MPEG2", "W%d" % w, "H%d" % h]
    if rate is not None:
        tok.append("F" + rate)
    tag = layout if tag is None else tag
    if tag:
        tok.append("C" + tag)
    tok += list(extra)
    data = bytearray(" ".join(tok).encode() + b"\n")
    for planes in frames:
        data += b"FRAME" + ((" " + frame_params).encode() if frame_params else b"") + b"\n"
        for p in planes:
            data += np.ascontiguousarray(p).tobytes()
    with open(path, "wb") as f:
        f.write(bytes(data[:len(data) - truncate]))
    return path
