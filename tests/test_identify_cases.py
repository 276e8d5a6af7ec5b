"""CPU: the cases of tests/identify_cases.py are what they say -- every layout plans the column ranges it states (through the stand-alone
program of csrc/group_blocks.h, tests/csrc/group_blocks_check.cpp, with identify.hip's two numbers on 256 compute units), every rung of
the ladder lies on the side of every switch that it names, the vectorised reference equals the loop of tests/identify_ref.py -- and the
float64 emulation of the Gram form on the ladder, printed per rung: the prediction the GPU figures of DESIGN.md are compared with."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import cluster_cases as cc
from tests import identify_cases as ic
from tests import identify_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("identify_cases") / "group_blocks_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(HERE, "..", "pyannote-video_amd", "csrc"), "-o", exe,
                           os.path.join(HERE, "csrc", "group_blocks_check.cpp")])
    return exe


def _ranges(exe, sizes, wanted, floor):
    out = subprocess.run([exe, "plan", str(wanted), str(floor)], input=" ".join(str(int(s)) for s in sizes), capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 0, (out.stdout[-800:], out.stderr[-800:])
    head, ranges, big = out.stdout.splitlines()
    f = head.split()
    return int(f[1]), int(f[3]), [int(v) for v in ranges.split()[1:]]


@pytest.fixture(scope="module")
def ladders():
    return {scale: ic.ladder(scale) for scale in (None, 0.55)}


# ---- plans -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", sorted(ic.GALLERIES))
def test_gallery_plans_the_ranges_it_states_under_every_query_layout(checker, gname):
    sizes, M, nb, ranges = ic.GALLERIES[gname]
    assert sum(sizes) == M and (M + 15) // 16 == nb
    assert len(ranges) > 2                                       # more than one range: what the galleries are for
    for qname, q_sizes in ic.QUERIES.items():
        nbq = (sum(q_sizes) + 15) // 16
        assert _ranges(checker, sizes, *ic.identify_wanted(nbq, nb)) == (M, nb, ranges), qname
    if gname in cc.LAYOUTS:
        assert ranges == cc.LAYOUTS[gname][3]                    # the plan K10 makes of the same sizes
    for row in ic.plant_rows(gname):
        assert 0 <= row < M
    inside, cut, last = ic.plant_rows(gname)
    assert inside < cut == ranges[1] * 16 and last // 16 == nb - 1


def test_layout_details(checker):
    """what the tables say beyond the ranges"""
    sizes, M, nb, ranges = ic.GALLERIES["long"]
    assert len(ranges) - 1 >= 5 and max(sizes) >= 300 and 2000 <= M <= 2500
    assert nb // 16 == len(ic.LONG_EVEN_CUTS) + 1 and ic.LONG_EVEN_CUTS == [nb * k // 8 for k in range(1, 8)]
    moved = [b for b in ranges[1:-1] if b not in ic.LONG_EVEN_CUTS]
    assert len(moved) >= 1 and len(ranges) - 2 < len(ic.LONG_EVEN_CUTS)             # moved cuts, and dropped ones
    assert len(ic.GALLERIES["singletons"][0]) == 521 > 256       # K beyond one x-block of cross_norm_k / cross_chunks_k
    assert ic.GALLERIES["tail1"][1] % 16 == 1                    # a gallery tail of one row
    blocks = {q: (sum(s) + 15) // 16 for q, s in ic.QUERIES.items()}
    assert blocks == {"main": 20, "singletons70": 5, "one100": 7, "tail1": 33}
    assert sum(ic.QUERIES["tail1"]) % 16 == 1
    # the ladder's tables: two gallery ranges, and two ranges of the concatenated table under K10's numbers
    nq, ng = ic.LADDER_QUERY_ROWS, ic.LADDER_GALLERY_ROWS
    assert _ranges(checker, [1] * ng, *ic.identify_wanted((nq + 15) // 16, (ng + 15) // 16))[2] == ic.LADDER_GALLERY_RANGES
    assert _ranges(checker, [1] * (nq + ng), *cc.k10_wanted((nq + ng + 15) // 16))[2] == ic.LADDER_K10_RANGES
    # the huge case
    nbq = (sum(ic.HUGE_QUERY_SIZES) + 15) // 16
    for name, g_sizes in ic.HUGE_GALLERIES.items():
        nbg = (sum(g_sizes) + 15) // 16
        assert _ranges(checker, g_sizes, *ic.identify_wanted(nbq, nbg))[2] == ic.HUGE_GALLERY_RANGES[name]
    assert len(ic.HUGE_GALLERIES["three_hundred"]) == 300 and set(ic.HUGE_GALLERIES["three_hundred"]) == {1, 2, 3}
    rs = ref.starts(ic.HUGE_QUERY_SIZES)
    assert len(ic.HUGE_QUERY_SIZES) > 65535 + 40
    for what, t in ic.HUGE_NAMED.items():
        assert ("%d-row" % ic.HUGE_QUERY_SIZES[t]) in what or what == "group 65535", what
    spanning = [t for t in ic.HUGE_NAMED.values() if (rs[t + 1] - 1) // 16 > rs[t] // 16]
    assert min(spanning) < 65535 < max(spanning) and len(spanning) == 3


def test_query_tables_carry_their_plants():
    for gname in sorted(ic.GALLERIES):
        G, gs = ic.gallery_table(gname)
        assert G.shape == (ic.GALLERIES[gname][1], 128) and gs[-1] == len(G)
        for qname in sorted(ic.QUERIES):
            X, rs, planted = ic.query_table(qname, gname, G)
            assert X.shape == (sum(ic.QUERIES[qname]), 128) and rs[-1] == len(X)
            assert [g for _, g in planted["copies"]] == ic.plant_rows(gname) == [g for _, g in planted["near"]]
            for q, g in planted["copies"]:
                assert np.array_equal(X[q], G[g])
            for q, g in planted["near"]:
                assert np.abs(X[q] - G[g] - 1e-5).max() < 1e-15
            assert len({q for q, _ in planted["copies"] + planted["near"]}) == 6
            for t, k in planted["zero"]:
                assert rs[t + 1] - rs[t] == 1 and gs[k + 1] - gs[k] == 1
        # one-row groups against one-row identities: every copy makes a whole entry zero
        if gname == "singletons":
            assert len(ic.query_table("singletons70", gname, G)[2]["zero"]) == 3
            assert len(ic.query_table("main", gname, G)[2]["zero"]) == 2


# ---- the ladder ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [None, 0.55])
def test_every_rung_lies_on_the_side_it_names(ladders, scale):
    """rho from exact differences: below every switch for the copies, on the named side of 1e-5 for the rungs around it, within 1 % of the
    target for the rungs that bracket a switch (0.99 | 1.01 times 1e-5, 1e-4, 1e-3, 1e-2), after the rounding to 5 decimals"""
    L = ladders[scale]
    E = ic.fixture_rows()
    nrm = np.sqrt((E * E).sum(-1))
    targets = dict(ic.RUNGS)
    assert [name for name, _ in ic.RUNGS[:9]] == ["copy", "quantum", "0.5e-5", "0.99e-5", "1.01e-5", "2e-5", "1e-4", "1e-3", "1e-2"]
    assert len(L["pairs"]) == 3 * len(ic.RUNGS) and len({q for _, _, q, _ in L["pairs"]}) == len(L["pairs"]) == len({g for _, _, _, g in L["pairs"]})
    norms = set()
    for name, base, q, g in L["pairs"]:
        a, b = L["X"][q], L["G"][g]
        assert np.array_equal(a, np.round(a, 5)) and np.array_equal(b, np.round(b, 5))
        norms.add(round(float(np.sqrt(a @ a)), 3))
        r = ic.rho(a, b)
        if name == "copy":
            assert r == 0.0 and np.array_equal(a, b)
        elif name == "quantum":
            assert (a != b).sum() == 1 and abs(np.abs(a - b).max() - 1e-5) < 1e-15 and 0 < r < 1e-8
        else:
            for s in ic.SWITCHES:
                if targets[name] != s:                           # (the rung AT a power of ten names no side of it)
                    assert (r < s) == (targets[name] < s), (name, base, r, s)
            tol = 0.01 if name in ic.BRACKETS else 0.1
            assert abs(r / targets[name] - 1) < tol, (name, base, r)
    if scale is None:                                            # base rows near the fixture's smallest, mean and largest norm
        assert len(norms) == 3 and min(norms) == round(float(nrm.min()), 3) and max(norms) == round(float(nrm.max()), 3) and 6.0 < nrm.min() and nrm.max() < 12.0
        assert min(abs(n - nrm.mean()) for n in norms) < 0.01
    else:
        assert max(abs(n - scale) for n in norms) < 1e-4
    # the rows are scattered: first and last rows of blocks, the last blocks, both sides of the cuts
    qs, gs = {q for _, _, q, _ in L["pairs"]}, {g for _, _, _, g in L["pairs"]}
    cut, k10 = ic.LADDER_GALLERY_RANGES[1] * 16, ic.LADDER_K10_RANGES[1] * 16 - ic.LADDER_QUERY_ROWS
    assert {0, 15, 16, 64, 68} <= qs and {0, 15, cut - 1, cut, k10 - 1, k10, 640, 648} <= gs


@pytest.mark.parametrize("scale", [None, 0.55])
def test_gram_form_emulated_in_float64_on_the_ladder(ladders, scale):
    """numpy float64 in place of the f64 MFMAs (another order of additions, the same magnitudes): the worst relative error per rung if every
    pair took the Gram form.  Printed (pytest -s); required to be finite."""
    L = ladders[scale]
    Dr = ic.dist_ld(L["X"], L["G"])
    D = Dr.copy()
    for name, base, q, g in L["pairs"]:
        D[q, g] = ic.gram_emulation(L["X"][q], L["G"][g])
    errs = ic.ladder_errors(D, Dr, L["pairs"])
    ic.print_ladder_errors("emulated Gram form, scale %s:" % scale, errs)
    for name, (rel, ab) in errs.items():
        assert np.isfinite(ab) and (np.isfinite(rel) or name in ("copy",)), name


# ---- references ----------------------------------------------------------------------------------------------------------------------------
def test_vectorised_reference_equals_the_loop():
    """mean_dist_fast against identify_ref.mean_dist (both metrics): the main case, a layout pair with its plants (copies, near-copies),
    chunks that cut the group table, and the longdouble pair reference against both on one-row groups"""
    cases = [ref.main_case()]
    G, gs = ic.gallery_table("mixed3")
    X, rs, _ = ic.query_table("main", "mixed3", G)
    cases.append((X, rs, G, gs))
    X, rs, _ = ic.query_table("tail1", "mixed3", G)
    cases.append((X[:203], np.r_[rs[:21], 203].astype(np.int32), G[:118], gs[:10]))
    assert gs[9] == 118
    for X, rs, G, gs in cases:
        for metric in (0, 1):
            want = ref.mean_dist(X, rs, G, gs, metric)
            for chunk in (8192, 33, 1):
                got = ic.mean_dist_fast(X, rs, G, gs, metric, chunk=chunk)
                assert got.shape == want.shape and np.allclose(got, want, rtol=1e-14, atol=1e-15), (metric, chunk, np.abs(got - want).max())
    L = ic.ladder()
    for metric in (0, 1):
        ld = ic.dist_ld(L["X"][:20], L["G"][:60], metric)
        assert np.allclose(ld, ref.mean_dist(L["X"][:20], L["rs"][:21], L["G"][:60], L["gs"][:61], metric), rtol=1e-14, atol=1e-15)
        assert np.allclose(ld, ic.mean_dist_fast(L["X"][:20], L["rs"][:21], L["G"][:60], L["gs"][:61], metric), rtol=1e-14, atol=1e-15)
