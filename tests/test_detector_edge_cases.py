"""CPU: the detector's edge-case table (tests/detector_cases.py) reaches what it claims -- shown on the oracle and on plan_dims() alone,
without a GPU.  Every seam of the kernels' fixed-width pieces is hit by a level of a case, the frame byte lengths cover all four
remainders modulo 4 and odd pitches, the level counts are the oracle's, the `complete` cases really return every (window, filter) pair at
the all-pass threshold (so the GPU comparison covers the whole score map of every level), the sampled ones hold candidates on every level
and on each level's first and last scanned row and column, and no run of the GPU test reaches the oracle's candidate cap.
tests/test_gpu_detector_edges.py then holds the library to the oracle on the same table.
Reference: pyannote/video/face/face.py:54,66."""
import numpy as np
import pytest

import detector_cases as dc


@pytest.fixture(scope="module")
def det(oracle):
    from pyannote_video_amd import models
    return oracle.Detector(models.load_container(models.DEFAULT_DETECTOR))


_raw_cache = {}


def _raw(det, g, content, seed, adj):
    key = (g.name, content, seed, adj)
    if key not in _raw_cache:
        _raw_cache[key] = det.detect_raw(dc.case_frame(g, content, seed), g.up, adj)
    return _raw_cache[key]


def test_every_named_seam_is_hit_by_a_level_of_a_case():
    for name, hit in dc.SEAMS:
        assert any(hit(g) for g in dc.GEOMETRY), name
    assert len(set(g.name for g in dc.GEOMETRY)) == len(dc.GEOMETRY)


def test_the_issues_table_is_in_the_table():
    want = {"251x60_up1": ([(61, 13), (51, 11), (42, 8), (34, 7)], 9640), "255x100_up1": ([(62, 23), (51, 19)], 20205),
            "500x61_up1": ([(123, 13), (102, 11), (85, 9), (70, 7)], 19880), "385x97_up1": ([(95, 22), (78, 18), (65, 15)], 30165),
            "769x50_up1": ([(191, 11), (158, 9), (132, 7)], 22235), "1543x41_up1": ([(384, 8), (320, 7)], 26560),
            "2049x41_up0": ([(254, 3)], 3810), "127x127_up1": ([(30, 30)], 12960), "161x121_up2": ([], 72360), "97x55_up1": ([], 3240),
            "41x39_up1": ([], 570), "79x79_up0": ([], 500), "80x80_up0": ([], 500), "40x40_up0": ([(3, 3)], 45), "7x5_up0": ([], 0),
            "1x1_up1": ([], 0)}
    for name, (cells, pairs) in want.items():
        g = dc.by_name(name)
        assert [(d[2], d[3]) for d in g.lv][:len(cells)] == cells and g.pairs == pairs, name
    assert dc.upsampled(161, 121, 2) == (650, 487) and dc.upsampled(1, 1, 1) == (4, 3) and dc.upsampled(251, 60, 1) == (504, 121)
    for name in ("641x361_up1", "643x363_up1", "642x361_up1", "457x257_up1", "1000x90_up1", "90x1000_up1"):
        assert dc.by_name(name).pairs > dc.ORACLE_CAP and not dc.by_name(name).complete
    assert dc.by_name("641x361_up0").complete and all(dc.by_name(n).complete for n in dc.CONTENT_SIZES + dc.CHUNK_SIZES + (dc.BATCH_SIZE,))
    assert dc.by_name("7x5_up0").degenerate and dc.by_name("1x1_up1").degenerate


def test_frame_byte_remainders_and_odd_pitches_occur():
    live = [g for g in dc.GEOMETRY if not g.degenerate]
    assert set(g.w * g.h * 3 % 4 for g in live) == {0, 1, 2, 3}
    # ... also among the frames resize_rows_k reads through its descriptor (upsampling reads the frame itself)
    assert set(g.w * g.h * 3 % 4 for g in live if g.up >= 1) == {0, 1, 2, 3}
    assert any(g.w % 2 == 1 and g.up >= 1 for g in live) and any(g.w % 2 == 1 and g.up == 0 for g in live)
    assert set(g.w * 3 % 4 for g in live) == {0, 1, 2, 3}
    for n in dc.STACKED_ODD:                        # stacked frames of these sizes start at three or more different address remainders
        g = dc.by_name(n)
        assert n in dc.ADDRESS_SIZES and len(set(i * g.w * g.h * 3 % 4 for i in range(5))) >= 3, n


def test_level_counts_and_level_sizes_are_the_oracles(det):
    for g in dc.GEOMETRY:
        uw, uh = dc.upsampled(g.w, g.h, g.up)
        assert det.levels(uh, uw) == g.levels, g
        f = dc.case_frame(g, "noise")
        for l in sorted(set((0, 1, g.levels - 1)) & set(range(g.levels))):
            img = det.pyramid_level(f, g.up, l)
            assert img.shape == (g.lv[l][1], g.lv[l][0], 3), (g, l)
            if not g.degenerate:
                assert _hog(img.shape) == (g.lv[l][3], g.lv[l][2]), (g, l)


def _hog(shape):
    return (int(shape[0] / 8.0 + 0.5) - 2, int(shape[1] / 8.0 + 0.5) - 2)


def test_feature_map_sizes_are_the_plans(oracle, det):
    """the oracle's feature map of a level is the plan's cells plus the filter's border: fh = hog_nr + 9, fw = hog_nc + 9"""
    for g in dc.GEOMETRY:
        if g.degenerate or g.pairs > 25000:
            continue
        f = dc.case_frame(g, "noise")
        for l, d in dc.scored(g.lv):
            feat = oracle.fhog(det.pyramid_level(f, g.up, l), 8, dc.FILTER, dc.FILTER)
            assert feat.shape == (d[3] + dc.FILTER - 1, d[2] + dc.FILTER - 1, 32), (g, l)


def test_complete_cases_return_every_window_at_the_all_pass_threshold(det):
    n_cases = 0
    for g, content, seed, adj in dc.all_runs():
        if not g.complete or adj != dc.ALL_PASS:
            continue
        raw = _raw(det, g, content, seed, adj)
        assert len(raw) == g.pairs, (g, content, len(raw), g.pairs)
        for l, d in dc.scored(g.lv):
            at = set((r[1], r[3], r[4]) for r in raw if r[2] == l)
            assert at == set((f, dc.FIRST + y, dc.FIRST + x) for f in range(5) for y in range(d[3]) for x in range(d[2])), (g, content, l)
        n_cases += 1
    assert n_cases >= 2 * sum(1 for g in dc.GEOMETRY if g.complete and not g.degenerate)
    # the count has stopped growing well above ALL_PASS on the contents with the lowest scores
    for content in ("noise", "black", "checker2", "white"):
        g = dc.by_name("255x100_up1")
        assert len(det.detect_raw(dc.case_frame(g, content), g.up, -20.0)) == g.pairs, content


def test_degenerate_cases_have_nothing_to_score(det):
    for g in dc.GEOMETRY:
        if g.degenerate:
            f = dc.case_frame(g, "noise")
            assert det.detect_raw(f, g.up, dc.ALL_PASS) == [] and det.detect(f, g.up, dc.ALL_PASS) == []


def test_sampled_cases_hold_candidates_on_every_level_and_border(det):
    n_cases = 0
    for g, content, seed, adj in dc.geometry_runs():
        if g.complete or adj == 0.0:
            continue
        assert adj == dc.ADJUST[(g.name, content)]
        raw = _raw(det, g, content, seed, adj)
        assert 2000 < len(raw) < 60000, (g, content, len(raw))
        for l, d in dc.scored(g.lv):
            rows = set(r[3] for r in raw if r[2] == l)
            cols = set(r[4] for r in raw if r[2] == l)
            assert rows and cols, (g, content, l)
            assert (min(rows), max(rows)) == (dc.FIRST, dc.FIRST + d[3] - 1), (g, content, l, min(rows), max(rows))
            assert (min(cols), max(cols)) == (dc.FIRST, dc.FIRST + d[2] - 1), (g, content, l, min(cols), max(cols))
        assert len(dc.scored(g.lv)) == g.levels
        n_cases += 1
    assert n_cases == 2 * sum(1 for g in dc.GEOMETRY if not g.complete) == len(dc.ADJUST)


def test_no_run_of_the_gpu_test_reaches_the_oracles_candidate_cap(det):
    runs = dc.all_runs()
    assert len(runs) > 150
    for g, content, seed, adj in runs:
        n = len(_raw(det, g, content, seed, adj))
        assert n < dc.ORACLE_CAP, (g, content, seed, adj, n)
        assert n <= g.pairs
    # ... and why the thresholds of the large cases are bisected and not simply lowered: noise at 641 x 361 fills the buffer at -1.0
    g = dc.by_name("641x361_up1")
    assert len(det.detect_raw(dc.case_frame(g, "noise"), g.up, -1.0)) == dc.ORACLE_CAP


def test_content_reaches_the_ends_of_the_feature_range(oracle, det):
    """The screening pass's error bound assumes orientation planes (0 .. 26) <= 0.4 and texture planes (27 .. 30) <= 0.849 (tests/
    screen_bound.py: LIM_LO, LIM_HI; the kernel checks what it reads and gives a call up otherwise).  On the oracle's level-0 features of
    every content: constant frames give all-zero maps (and so does a period-1 checkerboard that is not upsampled); the largest value of
    the orientation planes is their clip (four terms clipped at 0.2, times 0.5: 0.4 + one float32 step), the saturated checkerboards
    reach it like most contents, and nothing passes it; the texture planes peak on the renderer's faces (0.52 to 0.55, measured),
    far below their limit."""
    import screen_bound as sb
    clip = float(np.float32(0.5) * (np.float32(0.2) + np.float32(0.2) + np.float32(0.2) + np.float32(0.2)))
    for name in dc.CONTENT_SIZES:
        g = dc.by_name(name)
        lo, hi = {}, {}
        for content, _ in dc.CONTENT:
            f = dc.case_frame(g, content)
            feat = oracle.fhog(det.pyramid_level(f, g.up, 0), 8, dc.FILTER, dc.FILTER)
            assert np.isfinite(feat).all() and feat.min() >= 0.0 and not feat[:, :, 31].any(), (name, content)
            lo[content], hi[content] = float(feat[:, :, :27].max()), float(feat[:, :, 27:31].max())
            # (a period-1 board has equal neighbours two pixels apart: its centred differences vanish unless the level is upsampled)
            flat = content in dc.CONSTANT or (g.up == 0 and content.startswith("checker1"))
            assert flat == (not feat.any()), (name, content)
        print(name, "orientation planes", sorted(lo.items(), key=lambda kv: -kv[1])[:4], "texture planes", sorted(hi.items(), key=lambda kv: -kv[1])[:4])
        assert max(lo[c] for c in dc.SATURATED) == max(lo.values()) and max(lo.values()) <= clip * (1 + 2.0 ** -22) < sb.LIM_LO, (name, lo)
        assert max(hi.values()) < 0.6 < sb.LIM_HI, (name, hi)


def test_content_generators_are_what_they_say():
    h, w = 37, 53
    for content, _ in dc.CONTENT:
        f = dc.frame(content, h, w, 3)
        assert f.dtype == np.uint8 and f.shape == (h, w, 3) and f.flags["C_CONTIGUOUS"]
        assert np.array_equal(f, dc.frame(content, h, w, 3)), content                      # seeded
    for p in (1, 2):
        f = dc.frame("checker%d" % p, h, w)
        assert set(np.unique(f)) == {0, 255} and (f[0, 0] == 0).all() and (f[0, p] == 255).all() and (f[p, p] == 0).all()
    for k, c in enumerate("rgb"):
        f = dc.frame("checker1_" + c, h, w)
        assert f[:, :, k].any() and not np.delete(f, k, 2).any()
    f = dc.frame("grey_noise", h, w)
    assert np.array_equal(f[:, :, 0], f[:, :, 1]) and np.array_equal(f[:, :, 0], f[:, :, 2]) and len(np.unique(f)) > 100
    f = dc.frame("ramp_x", h, w)
    assert f[0, 0, 0] == 0 and f[-1, -1, 2] == 255 and (np.diff(f[5, :, 1].astype(int)) >= 0).all() and (f[0] == f[-1]).all()
    f = dc.frame("ramp_y", h, w)
    assert f[0, 0, 0] == 0 and f[-1, -1, 2] == 255 and (f[:, 0] == f[:, -1]).all()
    f = dc.frame("noise_tail", h, w)
    assert (f[-1] == 255).all() and (f[:, -1] == 255).all() and f[:-1, :-1].max() < 128
    assert np.array_equal(dc.frame("renderer", 16, 16, 5), dc.frame("noise", 16, 16, 5))    # too small for the renderer's face grid
    assert len(np.unique(dc.frame("renderer", 100, 255, 1))) > 50
