"""CPU: the shot detector's edge-case table (tests/shot_cases.py) reaches what it claims -- on the oracle and tests/shot_ref.py alone.
tests/test_gpu_shot_edges.py holds csrc/shot.hip to the SAME table, no entry left out, so what is proven here is what is tested there:
every level count of Farneback's pyramid and level sides on a rounding tie, pixel counts 0, 1 and 255 modulo the 256-lane stride,
conversions that enlarge in either direction, flows that leave the image on all four sides (the off-image branch of the matrix update
and the four clamps of the displaced lookup), all-zero flows, and differences of exactly 0 and exactly 255.  Conditions, not tolerances.
Reference: pyannote/video/structure/shot.py:71-99.

Largest |flow| component the oracle returns on the table, per number of coarser levels (all finite, all below 2^24 = 1.68e7, so every
`(int)floorf(...)` of the oracle's C is defined): 0 levels 6.70e4 (64 x 63), 1 level 6.53e5 (127 x 128), 2 levels 1.82e6 (129 x 131),
3 levels 3.03e6 (257 x 259).  The smooth textures of tests/test_shot.py stay below 10 pixels."""
import numpy as np
import pytest

import shot_cases as sc
import shot_ref

CONTENT = [c for c in sc.cases() if c.name.startswith("content_")]
CONVERT = [c for c in sc.cases() if c.name.startswith("convert_")]


@pytest.fixture(scope="module")
def tables():
    from pyannote_video_amd import structure
    return structure.shot_tables()


def test_table_has_every_geometry_once_and_a_diagonal_pair_everywhere():
    assert [(c.ow, c.oh) for c in CONTENT] == sc.GEOMETRIES and len(set(sc.GEOMETRIES)) == len(sc.GEOMETRIES) >= 20
    assert len(set(c.name for c in sc.cases())) == len(sc.cases())
    full = [n for n, _, _ in sc.full_pairs()]
    assert set(sc.SUBSET) <= set(full) and len(set(full)) == len(full)
    diagonal = set(n for n, _ in sc.DIAGONALS)
    for c in CONTENT:
        names = [n for n, _, _ in c.pairs]
        assert names == (full if (c.ow, c.oh) in sc.FULL_CONTENT else sc.SUBSET)
        assert any(set(n.split("_")) & diagonal for n in names)
        for _, a, b in c.pairs:                                    # identity conversion: the small image IS the content
            assert a.shape == b.shape == (c.oh, c.ow, 3) and a.dtype == np.uint8
    # every diagonal pattern meets black, white, noise and every other diagonal pattern, in both orders
    for a in diagonal:
        for b in (diagonal - {a}) | set(n for n, _ in sc.OTHERS):
            assert "%s_%s" % (a, b) in full and "%s_%s" % (b, a) in full


def test_table_has_every_level_count_and_a_rounding_tie():
    counts = {}
    for c in CONTENT:
        counts.setdefault(shot_ref.levels(c.oh, c.ow), []).append((c.ow, c.oh))
    assert sorted(counts) == [0, 1, 2, 3]
    assert sorted(shot_ref.levels(oh, ow) for ow, oh in sc.FULL_CONTENT) == [0, 1, 2, 3]        # the whole content set at each count
    # the seams: one pixel less on either side and the level is gone
    for (ow, oh), k in (((63, 64), 0), ((64, 63), 0), ((64, 64), 1), ((127, 128), 1), ((128, 128), 2), ((255, 256), 2), ((256, 256), 3),
                        ((64, 400), 1), ((300, 33), 0)):
        assert (ow, oh) in sc.GEOMETRIES and shot_ref.levels(oh, ow) == k, (ow, oh)
    # level sides exactly between two integers, rounding down to even and up to even
    ties = {}
    for ow, oh in sc.GEOMETRIES:
        for k in range(1, shot_ref.levels(oh, ow) + 1):
            for side in (ow, oh):
                v = side * 0.5 ** k
                if v - np.floor(v) == 0.5:
                    ties[v] = shot_ref.cv_round(v)
    assert ties[32.5] == 32 and ties[33.5] == 34 and ties[64.5] == 64 and ties[65.5] == 66 and ties[128.5] == 128 and ties[129.5] == 130
    assert any(r < v for v, r in ties.items()) and any(r > v for v, r in ties.items())


def test_table_has_the_pixel_count_classes_of_the_256_lane_stride():
    classes = set((c.ow * c.oh) % 256 for c in sc.cases())
    assert {0, 1, 255} <= classes, sorted(classes)
    assert min(c.ow * c.oh for c in sc.cases()) == 144 < 256 and (16, 16) in sc.GEOMETRIES        # less than one stride, exactly one
    assert all(c.ow >= 12 and c.oh >= 12 for c in sc.cases())


def test_table_has_an_upscaling_conversion_in_each_direction():
    kinds = set()
    for c in CONVERT:
        fw, fh = c.frame_size
        assert all(a.shape == b.shape == (fh, fw, 3) for _, a, b in c.pairs)
        kinds.add(("up" if c.ow > fw else "same" if c.ow == fw else "down", "up" if c.oh > fh else "same" if c.oh == fh else "down"))
        if c.ow > fw:                                               # enlarged: both ends of the coefficient table clamp
            s, c0, c1 = shot_ref.resize_coeffs(fw, c.ow)
            assert s[0] == 0 and c1[0] == 0 and s[-1] == fw - 1 and c1[-1] == 0 and (c1[1:-1] > 0).any()
    assert {("up", "up"), ("up", "down"), ("down", "up"), ("down", "down"), ("same", "same")} <= kinds
    assert any((c.frame_size[0] * 3) % 4 for c in CONVERT)          # a row length in bytes that is no multiple of 4
    assert any(c.frame_size[0] / c.ow != c.frame_size[0] // c.ow and c.ow < c.frame_size[0] for c in CONVERT)     # a non-integer reduction


def test_convert_restatement_equals_the_oracle(oracle):
    for c in sc.cases():
        for f in c.frames():
            assert np.array_equal(shot_ref.convert(f, c.ow, c.oh), oracle.shot_convert(f, c.ow, c.oh)), c
    for c in CONTENT:                                               # R = G = B at the small image's size: the conversion changes nothing
        f = c.frames()[-1]
        assert np.array_equal(oracle.shot_convert(f, c.ow, c.oh), f[:, :, 0])


def test_level_plan_restatement_equals_the_oracle(oracle):
    sizes = [(c.oh, c.ow) for c in sc.cases()] + [(88, 50), (1000, 1000), (32, 4000), (511, 513)]
    for h, w in sizes:
        mine, theirs = shot_ref.level_plan(h, w), oracle.farneback_plan(h, w)
        assert len(mine) - 1 == oracle.farneback_levels(h, w) == shot_ref.levels(h, w) == len(theirs) - 1
        for a, b in zip(mine, theirs):
            assert a[:3] == b[:3], (h, w, a[:3], b[:3])
            assert a[3].dtype == b[3].dtype == np.float32 and np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32)), (h, w)
    assert [p[2] for p in shot_ref.level_plan(256, 256)] == [3, 3, 9, 19]         # 2.5 -> 2, 7.5 -> 8, 17.5 -> 18, each | 1


def test_dfd_restatement_equals_the_oracle(oracle, tables):
    """pvo_shot_dfd_from_flow, alone and through pvo_shot_dfd, on the whole table"""
    for c in sc.cases():
        r = sc.oracle_results(c, oracle, tables)
        mine = [shot_ref.dfd_from_flow(r["gray"][2 * i], r["gray"][2 * i + 1], r["flow"][i]) for i in range(len(c.pairs))]
        assert mine == r["dfd"].tolist(), c
        whole = sc.threaded(lambda i: oracle.shot_dfd(r["gray"][2 * i], r["gray"][2 * i + 1], tables), range(len(c.pairs)))
        assert whole == mine, c


def test_every_flow_is_finite_and_below_2_to_24(oracle, tables):
    worst = {}
    for c in sc.cases():
        flow = sc.oracle_results(c, oracle, tables)["flow"]
        assert np.isfinite(flow).all(), c
        k = shot_ref.levels(c.oh, c.ow)
        worst[k] = max(worst.get(k, 0.0), float(np.abs(flow).max()))
    print("largest |flow| per level count:", worst)
    assert all(v < 2.0 ** 24 for v in worst.values()), worst
    assert all(worst[k] > 1e4 for k in range(4)), worst               # the flows the smooth textures never give


def test_every_geometry_leaves_the_image_on_all_four_sides_and_has_a_zero_flow(oracle, tables):
    for c in CONTENT:
        flow = sc.oracle_results(c, oracle, tables)["flow"]
        sides, zero, matrix_off = set(), 0, False
        for i in range(len(c.pairs)):
            sides |= sc.off_image_sides(flow[i])
            zero += not flow[i].any()
            # the final flow also fails the matrix update's own test (x + flow_x, y + flow_y inside [0, side - 1)): its off-image branch
            y, x = np.mgrid[0:c.oh, 0:c.ow].astype(np.float32)
            x1, y1 = np.floor(x + flow[i, ..., 0]), np.floor(y + flow[i, ..., 1])
            matrix_off = matrix_off or bool(((x1 < 0) | (x1 >= c.ow - 1) | (y1 < 0) | (y1 >= c.oh - 1)).any())
        assert sides == {"left", "right", "top", "bottom"}, (c, sides)
        assert zero >= 1 and matrix_off, c


def test_differences_include_exactly_0_and_exactly_255(oracle, tables):
    for c in CONTENT:
        dfd = sc.oracle_results(c, oracle, tables)["dfd"].tolist()
        names = [n for n, _, _ in c.pairs]
        assert dfd[names.index("black_black")] == 0.0 and dfd[names.index("black_white")] == 255.0 and dfd[names.index("white_black")] == 255.0
        assert all(0.0 <= d <= 255.0 for d in dfd)
