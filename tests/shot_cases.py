"""The shot detector's edge-case table, shared by tests/test_shot_edge_cases.py (CPU: the table reaches what it claims, on the oracle and
tests/shot_ref.py alone) and tests/test_gpu_shot_edges.py (GPU: csrc/shot.hip equals the oracle bit for bit on every entry).
Deterministic builders only, integer arithmetic in numpy: small-image geometries on the seams of Farneback's level rule and of the
256-lane stride, source frames that are reduced, kept and enlarged, and content from flat to rank-one (diagonal stripes and ramps, on
which the 2 x 2 solve divides by rounding noise and the flow leaves the image by thousands of pixels).
Reference: pyannote/video/structure/shot.py:71-99; the arithmetic is oracle/pvo_shot.c's."""
import numpy as np

# ---- small-image geometries (ow, oh): ow is Shot(height=...), oh = int(frame_w * ow / frame_h)
GEOMETRIES = [
    (12, 12), (12, 13), (13, 12),                       # the library's minimum
    (16, 16), (17, 15),                                 # 256 and 255 pixels
    (19, 27),                                           # 513 = 2 * 256 + 1 pixels (257 itself is prime: no image of 12 x 12 or more has it)
    (50, 88),                                           # the default from 1080p
    (63, 64), (64, 63),                                 # just below the first coarser level
    (64, 64), (65, 65), (67, 66),                       # one level; level sides 32.5 -> 32 and 33.5 -> 34 (ties to even)
    (127, 128), (128, 128), (129, 131),                 # around the second level
    (255, 256), (256, 256), (257, 259),                 # around the third
    (64, 400), (300, 33),                               # one side alone holds the level count down
]
FULL_CONTENT = [(50, 88), (64, 64), (128, 128), (256, 256)]     # the whole content set: one geometry per level count 0 .. 3


def _xy(ow, oh):
    y, x = np.mgrid[0:oh, 0:ow].astype(np.int64)
    return x, y


def const(v):
    return lambda ow, oh: np.full((oh, ow), v, np.uint8)


def checker(p):
    def f(ow, oh):
        x, y = _xy(ow, oh)
        return (((x // p + y // p) & 1) * 255).astype(np.uint8)
    return f


def vstripes(p):
    def f(ow, oh):
        x, _ = _xy(ow, oh)
        return (((x // p) & 1) * 255).astype(np.uint8)
    return f


def hstripes(p):
    def f(ow, oh):
        _, y = _xy(ow, oh)
        return (((y // p) & 1) * 255).astype(np.uint8)
    return f


def diag_stripes(sign, p):
    """saturated stripes of width p along x + y (sign +1) or x - y (sign -1): a rank-one structure tensor everywhere"""
    def f(ow, oh):
        x, y = _xy(ow, oh)
        return ((((x + sign * y + 4096) // p) & 1) * 255).astype(np.uint8)
    return f


def diag_ramp(sign, k):
    """a sawtooth of slope k grey levels per pixel along x + y or x - y"""
    def f(ow, oh):
        x, y = _xy(ow, oh)
        return (((x + sign * y + 4096) * k) % 256).astype(np.uint8)
    return f


def noise(seed):
    """uniform bytes from an integer hash of (x, y, seed): the same on every numpy"""
    def f(ow, oh):
        x, y = _xy(ow, oh)
        v = (x * 73856093) ^ (y * 19349663) ^ (seed * 83492791 + 12345)
        v = (v * 1103515245 + 12345) & 0x7FFFFFFF
        v = (v ^ (v >> 13)) * 1274126177 & 0x7FFFFFFF
        return ((v >> 11) & 255).astype(np.uint8)
    return f


def texture(dx=0, dy=0, add=0):
    """a smooth textured image (integer sum of four triangle waves of co-prime periods), translated by (dx, dy), brightness + add"""
    def tri(t, p):
        t = t % (2 * p)
        return np.where(t < p, t, 2 * p - t) * 255 // p

    def f(ow, oh):
        x, y = _xy(ow, oh)
        x, y = x + dx + 1000, y + dy + 1000
        v = (tri(3 * x + y, 23) + tri(x - 2 * y, 17) + tri(x + 4 * y, 31) + tri(5 * x - 3 * y, 41)) // 4
        return np.clip(v * 200 // 255 + 20 + add, 0, 255).astype(np.uint8)
    return f


def bright_pixel(ow, oh):
    img = np.zeros((oh, ow), np.uint8)
    img[oh // 2, ow // 2] = 255
    return img


def vstep(ow, oh):
    img = np.zeros((oh, ow), np.uint8)
    img[:, ow // 2:] = 255
    return img


# the nine diagonal patterns: stripes and ramps along x + y and x - y
DIAGONALS = [("ds+2", diag_stripes(+1, 2)), ("ds-3", diag_stripes(-1, 3)), ("ds+4", diag_stripes(+1, 4)), ("ds-6", diag_stripes(-1, 6)),
             ("ds+8", diag_stripes(+1, 8)), ("dr+16", diag_ramp(+1, 16)), ("dr-32", diag_ramp(-1, 32)), ("dr+64", diag_ramp(+1, 64)),
             ("dr-8", diag_ramp(-1, 8))]
OTHERS = [("black", const(0)), ("white", const(255)), ("noise1", noise(1))]


def full_pairs():
    """every content pair of the issue: (name, first image builder, second image builder)"""
    P = [("black_black", const(0), const(0)), ("grey_grey", const(128), const(128)), ("black_white", const(0), const(255)),
         ("white_black", const(255), const(0)),
         ("checker1_black", checker(1), const(0)), ("checker1_checker8", checker(1), checker(8)), ("checker8_noise", checker(8), noise(2)),
         ("vstripes_hstripes", vstripes(3), hstripes(5)), ("hstripes_vstripes", hstripes(2), vstripes(7)),
         ("noise_noise", noise(3), noise(4)), ("noise_itself", noise(3), noise(3)),
         ("pixel_black", bright_pixel, const(0)), ("black_pixel", const(0), bright_pixel), ("vstep_texture", vstep, texture()),
         ("texture_vstep", texture(), vstep),
         ("fade_up", texture(), texture(add=1)), ("fade_down", texture(), texture(add=-1))]
    P += [("shift%d" % s, texture(), texture(dx=s, dy=s if s % 2 else 0)) for s in range(1, 6)]
    for i, (na, a) in enumerate(DIAGONALS):
        for nb, b in OTHERS:
            P += [("%s_%s" % (na, nb), a, b), ("%s_%s" % (nb, na), b, a)]
        for nb, b in DIAGONALS[i + 1:]:
            P += [("%s_%s" % (na, nb), a, b), ("%s_%s" % (nb, na), b, a)]
    return P


# what every geometry gets: the constants, one noise pair, a small motion, a fade, and the rank-one pairs whose flows are the largest
# (a diagonal pattern FIRST, against a constant or another diagonal pattern: thousands of pixels from 50 x 88 on)
SUBSET = ["black_black", "black_white", "white_black", "noise_noise", "checker1_checker8", "shift3", "fade_up",
          "ds-3_black", "black_ds-3", "ds-3_white", "ds+4_black", "ds-6_white", "ds-6_ds-3", "ds-3_ds-6", "ds-3_dr-32", "dr-32_ds-3",
          "dr+64_ds+4", "ds+4_dr+64", "ds+8_ds+4", "noise1_ds-3", "ds-3_noise1"]


class Case(object):
    """pairs of RGB frames reduced to ow x oh small images: pairs[i] = (name, first frame, second frame)"""

    def __init__(self, name, ow, oh, pairs):
        self.name, self.ow, self.oh, self.pairs = name, ow, oh, pairs

    def __repr__(self):
        return self.name

    def frames(self):
        """all frames in one list: the pairs of the table are the consecutive pairs (2 i, 2 i + 1)"""
        return [f for _, a, b in self.pairs for f in (a, b)]


def rgb_of(gray):
    """a frame of the small image's own size whose conversion is the identity: R = G = B"""
    return np.ascontiguousarray(np.repeat(gray[:, :, None], 3, axis=2))


def colour_frame(w, h, seed, smooth=True):
    """an RGB source frame: three smooth textures (or three noise planes) of different phase"""
    if smooth:
        planes = [texture(dx=7 * c + seed, dy=3 * c + 2 * seed)(w, h) for c in range(3)]
    else:
        planes = [noise(10 * seed + c)(w, h) for c in range(3)]
    return np.ascontiguousarray(np.stack(planes, axis=2))


# ---- source frames for the conversion: (name, frame width, frame height, ow, oh)
CONVERSIONS = [
    ("down_noninteger", 77, 131, 50, 88),               # scale 1.54 x 1.4886...; 231 bytes per row (not a multiple of 4)
    ("down_to_minimum", 37, 41, 12, 13),
    ("identity", 50, 88, 50, 88),
    ("up_x_down_y", 20, 90, 60, 45),                    # enlarged horizontally, reduced vertically
    ("down_x_up_y", 90, 20, 45, 60),
    ("up_both", 20, 30, 60, 45),
    ("up_both_levels", 33, 41, 65, 67),                 # enlarged onto a geometry with a coarser level; 99 bytes per row
    ("odd_row_bytes", 71, 90, 64, 81),                  # 213 bytes per row
]

_CACHE = {}


def cases():
    """the whole table: one content case per geometry, then the conversion cases"""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    allp = full_pairs()
    by_name = {n: (a, b) for n, a, b in allp}
    assert len(by_name) == len(allp)
    out = []
    for ow, oh in GEOMETRIES:
        names = [n for n, _, _ in allp] if (ow, oh) in FULL_CONTENT else SUBSET
        out.append(Case("content_%dx%d" % (ow, oh), ow, oh, [(n, rgb_of(by_name[n][0](ow, oh)), rgb_of(by_name[n][1](ow, oh))) for n in names]))
    for name, fw, fh, ow, oh in CONVERSIONS:
        pairs = [("smooth", colour_frame(fw, fh, 1), colour_frame(fw, fh, 2)), ("noise", colour_frame(fw, fh, 3, False), colour_frame(fw, fh, 4, False)),
                 ("stripes", rgb_of(diag_stripes(+1, 3)(fw, fh)), rgb_of(diag_ramp(-1, 16)(fw, fh)))]
        c = Case("convert_" + name, ow, oh, pairs)
        c.frame_size = (fw, fh)
        out.append(c)
    _CACHE["cases"] = out
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


def threaded(fn, items):
    """[fn(item)] with the oracle's calls side by side (ctypes releases the interpreter lock; pvo_farneback itself is one thread)"""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle
    with ThreadPoolExecutor(max(1, min(16, oracle.usable_cpus()))) as pool:
        return list(pool.map(fn, items))


def oracle_results(c, oracle, tables):
    """the oracle on one case, computed once per process and shared read-only: dict(gray uint8 [2 p, oh, ow], flow float32 [p, oh, ow, 2],
    dfd float64 [p]); dfd = pvo_shot_dfd_from_flow on the oracle's flow, which is what pvo_shot_dfd computes"""
    key = ("oracle", c.name)
    if key not in _CACHE:
        gray = np.stack([oracle.shot_convert(f, c.ow, c.oh) for f in c.frames()])
        pairs = range(len(c.pairs))
        flow = np.stack(threaded(lambda i: oracle.farneback(gray[2 * i], gray[2 * i + 1], tables), pairs))
        dfd = np.array([oracle.shot_dfd_from_flow(gray[2 * i], gray[2 * i + 1], flow[i]) for i in pairs], np.float64)
        for a in (gray, flow, dfd):
            a.setflags(write=False)
        _CACHE[key] = dict(gray=gray, flow=flow, dfd=dfd)
    return _CACHE[key]


def off_image_sides(flow):
    """the sides on which the displaced lookup of shot.py:89-99 (`dy, dx = flow[y, x]`: component 0 is added to y, component 1 to x)
    leaves an image with this flow, from the flow alone"""
    h, w = flow.shape[:2]
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    fx, fy = x + flow[..., 1], y + flow[..., 0]
    sides = set()
    if (fx < 0).any():
        sides.add("left")
    if (fx > np.float32(w - 1)).any():
        sides.add("right")
    if (fy < 0).any():
        sides.add("top")
    if (fy > np.float32(h - 1)).any():
        sides.add("bottom")
    return sides
