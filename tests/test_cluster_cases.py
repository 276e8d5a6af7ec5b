"""CPU: csrc/group_blocks.h (the check of a group table, the 16-row blocking, the cut into column ranges) through its stand-alone program
under ASan + UBSan, and the plans of the layouts in tests/cluster_cases.py -- a layout that stops reaching its path fails here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import cluster_cases as cc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("group_blocks") / "group_blocks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(HERE, "..", "pyannote-video_amd", "csrc"), "-o", exe,
                           os.path.join(HERE, "csrc", "group_blocks_check.cpp")])
    return exe


def _plan(exe, sizes, wanted, floor):
    out = subprocess.run([exe, "plan", str(wanted), str(floor)], input=" ".join(str(int(s)) for s in sizes), capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 0, (out.stdout[-800:], out.stderr[-800:])
    head, ranges, big = out.stdout.splitlines()
    f = head.split()
    return dict(N=int(f[1]), nb=int(f[3]), parts=int(f[5]), range_b0=[int(v) for v in ranges.split()[1:]], big=[int(v) for v in big.split()[1:]])


def test_group_blocks_invariants_and_refusals(checker):
    """every row in exactly one segment, segments numbered in row order, blk_cont / blk_clean at the seams only, parts of a spanning group
    consecutive, ranges cut at clean blocks, over the named layouts and 3000 random size lists; the bad tables (decreasing, empty group,
    end != N, first != 0, an entry above N) refused with their messages before anything is indexed"""
    out = subprocess.run([checker], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-800:], out.stderr[-800:])
    assert out.stdout.strip().endswith("0 failures")


@pytest.mark.parametrize("name", sorted(cc.LAYOUTS))
def test_layout_plans_the_ranges_it_is_meant_to_reach(checker, name):
    sizes, N, nb, ranges = cc.LAYOUTS[name]
    assert sum(sizes) == N and (N + 15) // 16 == nb
    plan = _plan(checker, sizes, *cc.k10_wanted(nb))
    assert (plan["N"], plan["nb"], plan["range_b0"]) == (N, nb, ranges)
    assert len(ranges) > 2                                       # more than one range: what the layouts are for
    rs = cc.starts(sizes)
    span = np.flatnonzero((rs[1:] - 1) // 16 > rs[:-1] // 16)
    assert plan["big"] == span.tolist()
    assert plan["parts"] == int(((rs[1:] - 1) // 16 - rs[:-1] // 16 + 1)[span].sum())


def test_layout_details(checker):
    """what the table of layouts says beyond the ranges"""
    p = {name: _plan(checker, cc.LAYOUTS[name][0], *cc.k10_wanted(cc.LAYOUTS[name][2])) for name in cc.LAYOUTS}
    assert p["aligned16"]["big"] == [] and p["singletons"]["big"] == []
    assert len(p["cut_moved"]["big"]) == 25 and 36 in p["cut_moved"]["big"]
    assert 35 // 2 == 17 and p["cut_moved"]["range_b0"][1] == 22      # the even cut (block 17) moved
    assert cc.k10_wanted(50)[0] >= 3 and 50 // 16 == 3 and len(p["one_cut_dropped"]["range_b0"]) == 3   # three wanted, two planned
    assert cc.LAYOUTS["tail1"][1] % 16 == 1 and cc.LAYOUTS["singletons"][1] % 16 == 9
    assert len(p["tail1"]["big"]) in (25, 26)                    # every second track spans
    # the tables carry what they say they plant
    for name in cc.LAYOUTS:
        X, rs, planted = cc.table(name)
        assert X.shape == (cc.LAYOUTS[name][1], 128) and rs[-1] == len(X)
        cut = planted["cut_row"]
        if name == "singletons":
            for i, j in planted["zero_pairs"]:
                assert i < j and np.array_equal(X[i], X[j])
            assert any(i < cut <= j for i, j in planted["zero_pairs"])
        else:
            assert np.array_equal(X[cut], X[3]) and np.abs(X[cut + 2] - X[cut - 3] - 1e-5).max() < 1e-15
        for cuts in cc.share_cut_lists(name):
            assert cuts[0] == 0 and cuts[-1] == len(rs) - 1 and all(a <= b for a, b in zip(cuts, cuts[1:]))
            assert any(a == b for a, b in zip(cuts, cuts[1:])) and (len(rs) - 2, len(rs) - 1) in list(zip(cuts, cuts[1:]))


def test_the_all_block_shapes_test_plans_one_range(checker):
    """test_pair_mean_dist_matrix_core_kernel_all_block_shapes (tests/test_gpu_parity.py): N = 501, 32 blocks, two ranges wanted, and the
    250-row track covers every block from the proposed cut to the end -- one range, so that test never crosses a range cut"""
    sizes = cc.ALL_BLOCK_SHAPES_SIZES
    assert sum(sizes) == 501
    wanted, floor = cc.k10_wanted(32)
    assert min(wanted, 32 // 16) == 2
    assert _plan(checker, sizes, wanted, floor)["range_b0"] == [0, 32]


def test_python_wrappers_refuse_a_short_order_and_a_short_table():
    """runtime.py refuses, before the C call, an `order` whose length is not row_start[-1] (the library reads order[k] for every k < N) and
    a table with fewer rows than row_start[-1]"""
    from pyannote_video_amd.runtime import Context

    class Never(object):
        def __getattr__(self, name):
            def called(*args):
                raise AssertionError("the library was called: " + name)
            return called

    c = Context.__new__(Context)
    c._l, c._h = Never(), 1
    E = np.zeros((20, 128), np.float32)
    rs = np.array([0, 8, 20], np.int32)
    for order in (np.arange(19), np.arange(21) % 20, np.zeros((20, 1), np.int64)):
        with pytest.raises(ValueError, match="order"):
            c.cluster_tracks_f32(E, order, rs, 0.6)
        with pytest.raises(ValueError, match="order"):
            c.pair_upper_rows_f32(E, order, rs, 0, 2)
    with pytest.raises(ValueError, match="rows"):
        c.cluster_tracks_f32(E[:19], None, rs, 0.6)
    with pytest.raises(ValueError, match="rows"):
        c.pair_upper_rows_f32(E[:19], None, rs, 0, 2)
    X = np.zeros((19, 128))
    with pytest.raises(ValueError, match="rows"):
        c.pair_upper_rows(X, rs, 0, 2)
    with pytest.raises(ValueError, match="rows"):
        c.pair_mean_dist_rows(X, rs, 0, 2)
    c._h = None
