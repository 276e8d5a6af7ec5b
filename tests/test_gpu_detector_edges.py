"""GPU: the detector (csrc/detect.hip: resize_rows_k, fhog_split_ml_k, score_roll_k; csrc/screen.hip) against oracle.Detector on the
edge-case table of tests/detector_cases.py -- frame geometries on the seams of the kernels' fixed-width pieces, frames whose byte length
and row pitch are not multiples of 4, frames at device addresses that are not multiples of 4, batches of mixed content, the plan knobs
PVF_FHOG_CHUNK and PVF_SCORE_SEG, the screening pass on and off, and content the synthetic renderer never makes (saturated
checkerboards, constant and grey frames, single-channel gradients, ramps, noise).  tests/test_detector_edge_cases.py proves on the oracle
alone that the table contains those conditions.  Everything is compared bit for bit: pyramid bytes, feature bits, raw candidates (score
bits, filter, level, row, column, box) and final boxes.  No tolerances.
Reference: pyannote/video/face/face.py:54,66 (dlib.get_frontal_face_detector()(rgb, 1))."""
import contextlib

import numpy as np
import pytest
import torch          # first, as in bench.py: the process then runs on the HIP runtime torch ships

import detector_cases as dc

pytestmark = pytest.mark.gpu


_dumps = [0]


def _dump(name, **arrays):
    """both sides of a mismatch where test_gpu_parity.py leaves its own (the first few of a run and nothing large: the assertion
    message names the rest)"""
    import test_gpu_parity
    _dumps[0] += 1
    if _dumps[0] <= 6 and sum(a.nbytes for a in arrays.values()) <= (4 << 20):
        test_gpu_parity._dump(name, **arrays)


@pytest.fixture(scope="module")
def det(oracle):
    from pyannote_video_amd import models
    return oracle.Detector(models.load_container(models.DEFAULT_DETECTOR))


_ref = {}     # the oracle's results of this module's runs: several tests meet the same (frame, threshold)


def _ref_raw(det, g, content, seed, adj, up=None):
    up = g.up if up is None else up
    key = ("raw", g.name, content, seed, adj, up)
    if key not in _ref:
        _ref[key] = det.detect_raw(dc.case_frame(g, content, seed), up, adj)
        assert len(_ref[key]) < dc.ORACLE_CAP
    return _ref[key]


def _ref_level(det, g, content, seed, l, up=None):
    up = g.up if up is None else up
    key = ("pyr", g.name, content, seed, l, up)
    if key not in _ref:
        _ref[key] = det.pyramid_level(dc.case_frame(g, content, seed), up, l)
    return _ref[key]


def _first_diff(a, b):
    at = np.argwhere(a != b)[0]
    return tuple(int(v) for v in at)


def _same_level(tag, l, a, b):
    """pyramid bytes of one level; -> list of what differed"""
    if a.shape != b.shape:
        return [(tag, "pyramid level %d" % l, "shape", a.shape, b.shape)]
    if not np.array_equal(a, b):
        _dump("det_edges_pyr_%s_l%d" % (tag, l), gpu=a, cpu=b)
        y, x, ch = _first_diff(a, b)
        return [(tag, "pyramid level %d" % l, "first differing (row, column, channel)", (y, x, ch), "gpu", int(a[y, x, ch]), "oracle", int(b[y, x, ch]),
                 "%d bytes differ" % int((a != b).sum()))]
    return []


def _pyramid(c, det, fr, g, content, seed, tag):
    bad = []
    for l in range(g.levels):
        bad += _same_level(tag, l, c.pyramid_level(fr, g.up, l), _ref_level(det, g, content, seed, l))
    return bad


def _features(c, oracle, det, fr, g, content, seed, tag):
    bad = []
    for l in range(g.levels):
        a = c.level_features(fr, g.up, l)
        d = g.lv[l]
        if d[2] <= 0 or d[3] <= 0:
            if a.size:
                bad.append((tag, "level %d has no feature map in the plan" % l, a.shape))
            continue
        b = oracle.fhog(_ref_level(det, g, content, seed, l), 8, dc.FILTER, dc.FILTER)
        if a.shape != b.shape:
            bad.append((tag, "features of level %d" % l, "shape", a.shape, b.shape))
        elif not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            _dump("det_edges_feat_%s_l%d" % (tag, l), gpu=a, cpu=b)
            y, x, p = _first_diff(a.view(np.uint32), b.view(np.uint32))
            bad.append((tag, "features of level %d" % l, "first differing (row, column, plane)", (y, x, p), "gpu", float(a[y, x, p]), "oracle",
                        float(b[y, x, p]), "%d floats differ" % int((a.view(np.uint32) != b.view(np.uint32)).sum())))
    return bad


def _table(raw):
    """raw candidates as an array [n, 9]: level, filter, row, column, score bits, box"""
    t = np.zeros((len(raw), 9), np.int64)
    for i, r in enumerate(raw):
        t[i] = (r[2], r[1], r[3], r[4], int(np.float32(r[0]).view(np.uint32)), r[5][0], r[5][1], r[5][2], r[5][3])
    return t


def _same_raw(tag, got, want):
    if got == want:
        return []
    a, b = _table(got), _table(want)
    _dump("det_edges_raw_%s" % tag, gpu=a, cpu=b)
    # the first window, in scan order, that one side has and the other has not (or scores differently)
    sa, sb = set(map(tuple, a.tolist())), set(map(tuple, b.tolist()))
    odd = sorted(sa ^ sb, key=lambda t: (t[0], t[2], t[3], t[1]))
    if not odd:
        return [(tag, "raw candidates: the same %d candidates in another order" % len(want))]
    at = odd[0]
    return [(tag, "raw candidates: gpu %d, oracle %d, %d differ" % (len(got), len(want), len(odd)),
             "first differing level %d (row, column) (%d, %d) filter %d" % (at[0], at[2], at[3], at[1]),
             "gpu", [t for t in sa if t[:4] == at[:4]], "oracle", [t for t in sb if t[:4] == at[:4]])]


def _same_boxes(tag, c, det, fr, fnp, up, adj):
    boxes, scores = c.detect(fr, up, adj)
    fin = det.detect(fnp, up, adj)
    assert len(fin) < 4096                                       # (the oracle's buffer for final boxes)
    if boxes != [d[5] for d in fin] or not np.array_equal(scores, np.array([d[0] for d in fin], np.float32)):
        return [(tag, "final boxes at %r" % adj, boxes[:5], [d[5] for d in fin][:5])]
    return []


LIST_CAP = 1 << 20        # csrc/pvf_internal.h: screen_list_cap, the pairs a batch may list by default (what tests put back)


@contextlib.contextmanager
def _uploaded(c, fnp):
    """the frame on the device for the block; released whether or not the block raises"""
    fr = c.upload(fnp)
    try:
        yield fr
    finally:
        fr.release()


class _Screening(object):
    """with _Screening(ctx, on): the screening pass switched for the block and back on (its default) afterwards"""

    def __init__(self, c, on, list_cap=0):
        self.c, self.on, self.list_cap = c, on, list_cap

    def __enter__(self):
        self.c.detector_screening(self.on, self.list_cap)
        return self

    def __exit__(self, *exc):
        self.c.detector_screening(True, LIST_CAP)


def _dense_and_screened(c, det, fr, g, content, seed, adj, tag, up=None):
    """raw candidates on the dense kernel and through the screening pass, both against the oracle; the screened call must have been
    screened (`batches` grew) and must not have been repeated on the dense kernel (`retries` did not grow)"""
    up = g.up if up is None else up
    want = _ref_raw(det, g, content, seed, adj, up)
    bad = []
    with _Screening(c, False):
        bad += _same_raw(tag + "_dense_%r" % adj, c.detect_raw(fr, up, adj), want)       # (first: it also grows the candidate slots to what the frame needs)
    with _Screening(c, True):
        s0 = c.detector_screening_stats()
        got = c.detect_raw(fr, up, adj)
        s1 = c.detector_screening_stats()
    bad += _same_raw(tag + "_screened_%r" % adj, got, want)
    if not g.degenerate:
        if s1["batches"] - s0["batches"] != 1:
            bad.append((tag, adj, "the screened call ran %d screened batches" % (s1["batches"] - s0["batches"])))
        if s1["retries"] != s0["retries"]:
            bad.append((tag, adj, "the screening pass gave the call up: a feature above the bound its error analysis assumes"))
    return bad


# ---- a, f: every geometry, renderer and noise content: pyramid, features, raw candidates dense and screened, final boxes ---------------
@pytest.mark.parametrize("g", dc.GEOMETRY, ids=lambda g: g.name)
def test_every_geometry_equals_the_oracle(ctx, oracle, det, g):
    bad = []
    for content in ("renderer", "noise"):
        fnp = dc.case_frame(g, content)
        tag = "%s_%s" % (g.name, content)
        with _uploaded(ctx, fnp) as fr:
            bad += _pyramid(ctx, det, fr, g, content, 0, tag)
            bad += _features(ctx, oracle, det, fr, g, content, 0, tag)
            for adj in dc.thresholds(g, content):
                bad += _dense_and_screened(ctx, det, fr, g, content, 0, adj, tag)
                bad += _same_boxes(tag, ctx, det, fr, fnp, g.up, adj)
                if g.degenerate:
                    assert ctx.detect_raw(fr, g.up, adj) == [] and ctx.detect(fr, g.up, adj)[0] == []
                elif adj == dc.ALL_PASS:
                    assert len(_ref_raw(det, g, content, 0, adj)) == g.pairs      # the whole score map of every level was compared
    assert not bad, bad[:10]


def test_list_overflow_on_the_complete_cases_is_counted_and_exact(ctx, det):
    """at the all-pass threshold with a list of 16 pairs the screening pass overflows: the call is repeated on the dense kernel, counted,
    and still exact"""
    bad = []
    for name in ("40x40_up0", "251x60_up1", "1543x41_up1", "777x45_up1", "391x99_up0"):
        g = dc.by_name(name)
        with _uploaded(ctx, dc.case_frame(g, "noise")) as fr:
            with _Screening(ctx, True, 16):
                s0 = ctx.detector_screening_stats()
                got = ctx.detect_raw(fr, g.up, dc.ALL_PASS)
                s1 = ctx.detector_screening_stats()
            bad += _same_raw(name + "_overflow", got, _ref_raw(det, g, "noise", 0, dc.ALL_PASS))
            assert g.pairs > 16 and s1["retries"] == s0["retries"] + 1, (name, s0, s1)
    assert not bad, bad[:10]


# ---- b: both coordinate generations on the odd-sized cases ------------------------------------------------------------------------------
def test_pyramid_of_the_odd_sizes_under_accumulated_coordinates(oracle, det, monkeypatch):
    """... and the switch took effect on both sides: on most levels the oracle's bytes under `accumulate` differ from its bytes under
    `mul`, and the library equals the former"""
    from pyannote_video_amd import models
    from pyannote_video_amd.runtime import Context
    odd = [g for g in dc.GEOMETRY if g.odd and not g.degenerate]
    assert len(odd) >= 12
    monkeypatch.delenv("PVO_RESIZE_COORDS", raising=False)
    monkeypatch.delenv("PVF_RESIZE_COORDS", raising=False)
    mul = {(g.name, content, l): _ref_level(det, g, content, 0, l) for g in odd for content in ("renderer", "noise") for l in range(g.levels)}
    monkeypatch.setenv("PVO_RESIZE_COORDS", "accumulate")
    monkeypatch.setenv("PVF_RESIZE_COORDS", "accumulate")
    c = Context(device=0, detector=models.DEFAULT_DETECTOR)          # (a context of its own: the tables belong to a context's plans)
    bad, moved, moved_cases = [], 0, set()
    try:
        for g in odd:
            for content in ("renderer", "noise"):
                fnp = dc.case_frame(g, content)
                with _uploaded(c, fnp) as fr:
                    for l in range(g.levels):
                        b = det.pyramid_level(fnp, g.up, l)          # (not through the cache: these are the other mode's bytes)
                        bad += _same_level("%s_%s_accumulate" % (g.name, content), l, c.pyramid_level(fr, g.up, l), b)
                        if b.shape == mul[(g.name, content, l)].shape and not np.array_equal(b, mul[(g.name, content, l)]):
                            moved += 1
                            moved_cases.add(g.name)
    finally:
        c.close()
    assert not bad, bad[:10]
    print("levels whose bytes differ between the two coordinate generations: %d of %d" % (moved, len(mul)))
    assert moved > 0 and len(moved_cases) >= len(odd) // 2, (moved, sorted(moved_cases))


# ---- suspect 1: the last 1 .. 3 bytes of a frame whose length is not a multiple of 4 ------------------------------------------------------
def test_the_last_bytes_of_a_frame_of_odd_length_arrive(ctx, det):
    """resize_rows_k reads the frame as dwords behind a descriptor of exactly h * w * 3 bytes: the dword that holds the frame's last pixel
    straddles the descriptor's end when that length is not a multiple of 4.  With the last row and column at 255 over dark noise the
    upsampled level's bottom-right corner shows whether those bytes arrived; the whole level must equal the oracle's"""
    bad, seen = [], set()
    for name in ("385x97_up1", "769x50_up1", "1543x41_up1", "641x361_up1", "457x257_up1"):
        g = dc.by_name(name)
        fnp = dc.case_frame(g, "noise_tail")
        want = _ref_level(det, g, "noise_tail", 0, 0)
        assert (want[-1, -1] == 255).all() and (fnp[-1, -1] == 255).all()
        seen.add(fnp.size % 4)
        t = torch.from_numpy(fnp).cuda()                                # an allocation of exactly the frame
        for how, fr in (("upload", ctx.upload(fnp)), ("wrap", ctx.wrap_torch(t))):
            got = ctx.pyramid_level(fr, 1, 0)
            print(name, how, "frame bytes %% 4 = %d, bottom-right pixel of level 0: gpu %s oracle %s" % (fnp.size % 4, got[-1, -1].tolist(), want[-1, -1].tolist()))
            bad += _same_level("%s_tail_%s" % (name, how), 0, got, want)
            fr.release()
    assert seen == {1, 2, 3}
    assert not bad, bad[:10]


# ---- c: frames at device addresses that are not multiples of 4 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.ADDRESS_SIZES)
def test_frames_at_unaligned_addresses(ctx, det, name):
    g = dc.by_name(name)
    h, w, n = g.h, g.w, g.h * g.w * 3
    frames = [dc.case_frame(g, "noise", s) for s in dc.ADDRESS_SEEDS]
    adj = dc.thresholds(g, "noise")[1]
    bad = []

    def check(fr, seed, how):
        out = []
        tag = "%s_%s_seed%d" % (name, how, seed)
        out += _same_level(tag + "_up1", 0, ctx.pyramid_level(fr, 1, 0), _ref_level(det, g, "noise", seed, 0, 1))
        out += _same_level(tag + "_up0", 0, ctx.pyramid_level(fr, 0, 0), frames[seed])
        out += _same_raw(tag, ctx.detect_raw(fr, g.up, adj), _ref_raw(det, g, "noise", seed, adj))
        return out

    # the uploaded frame: what the others must equal (and itself the oracle's)
    for s, f in enumerate(frames):
        fr = ctx.upload(f)
        bad += check(fr, s, "upload")
        fr.release()
    # five frames in one contiguous tensor: frame i starts i * h * w * 3 bytes in
    stack = torch.from_numpy(np.stack(frames)).cuda()
    rem = [stack[i].data_ptr() % 4 for i in range(5)]
    if name in dc.STACKED_ODD:
        assert len(set(rem)) >= 3, rem
    for s in range(5):
        fr = ctx.wrap_torch(stack[s])
        bad += check(fr, s, "stack%d" % rem[s])
        fr.release()
    # a frame 1, 2 and 3 bytes into a larger byte buffer
    for off in (1, 2, 3):
        buf = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
        view = buf[off:off + n].view(h, w, 3)
        view.copy_(torch.from_numpy(frames[off]))
        torch.cuda.synchronize()
        assert view.data_ptr() % 4 == off and view.is_contiguous()
        fr = ctx.wrap_torch(view)
        bad += check(fr, off, "offset%d" % off)
        fr.release()
    # the same frames through the ingest ring
    ring = ctx.ingest_ring(h, w, depth=8)
    try:
        held = [ring.push(f) for f in frames]
        ring.wait()
        for s, fr in enumerate(held):
            bad += check(fr, s, "ring")
            fr.release()
    finally:
        ring.close()
    assert not bad, bad[:10]


# ---- d: batches ---------------------------------------------------------------------------------------------------------------------------
def _rows(raw):
    """a detect_raw list as detect_raw_many's table: level, filter, row, column, score bits"""
    return np.array([(r[2], r[1], r[3], r[4], int(np.float32(r[0]).view(np.int32))) for r in raw], np.int32).reshape(-1, 5)


@pytest.mark.parametrize("name", [dc.BATCH_SIZE, dc.TINY_BATCH_SIZE, "7x5_up0"])
def test_batches_of_mixed_content_equal_single_calls_and_the_oracle(ctx, det, name):
    g = dc.by_name(name)
    frames = [dc.case_frame(g, c, s) for c, s in dc.BATCH_FRAMES]
    assert g.degenerate or len(set(f.tobytes() for f in frames)) == 7
    dev = [ctx.upload(f) for f in frames]
    bad = []
    try:
        for adj in ((0.0, dc.ALL_PASS) if name == dc.BATCH_SIZE else (dc.ALL_PASS,)):
            want = [det.detect_raw(f, g.up, adj) if g.degenerate else _ref_raw(det, g, c, s, adj) for f, (c, s) in zip(frames, dc.BATCH_FRAMES)]
            fin = [det.detect(f, g.up, adj) for f in frames]
            single = [ctx.detect_raw(fr, g.up, adj) for fr in dev]
            for k in range(7):
                bad += _same_raw("%s_single%d_%r" % (name, k, adj), single[k], want[k])
            for batch in (1, 3, 7):
                many = ctx.detect_raw_many(dev, batch, g.up, adj)
                for k in range(7):
                    if not np.array_equal(many[k], _rows(want[k])):
                        _dump("det_edges_many_%s_b%d_f%d" % (name, batch, k), gpu=many[k], cpu=_rows(want[k]))
                        bad.append((name, adj, "detect_raw_many, batches of %d, frame %d: %d candidates, oracle %d" % (batch, k, len(many[k]), len(want[k]))))
                res = ctx.detect_many(dev, batch, g.up, adj)
                for k in range(7):
                    if res[k][0] != [d[5] for d in fin[k]] or not np.array_equal(res[k][1], np.array([d[0] for d in fin[k]], np.float32)):
                        bad.append((name, adj, "detect_many, batches of %d, frame %d" % (batch, k), res[k][0][:4], [d[5] for d in fin[k]][:4]))
            if g.degenerate:
                assert all(len(m) == 0 for m in many) and all(r[0] == [] for r in res)
    finally:
        for fr in dev:
            fr.release()
    assert not bad, bad[:10]


# ---- e: the FHOG row chunks and the scoring kernel's row pieces, other than the ones the device's size chooses --------------------------
def _ceil(a, b):
    return (a + b - 1) // b


@pytest.mark.parametrize("knob,value", [("PVF_FHOG_CHUNK", v) for v in (1, 2, 3, 16)] + [("PVF_SCORE_SEG", v) for v in (2, 3, 16)])
def test_chunk_and_piece_seams(ctx, oracle, det, monkeypatch, knob, value):
    """every value is accepted (ml_plan refuses none) and must be exact; pvf_debug_level_plan shows that the knob cut the levels
    differently from the session context's plan, and only the pieces it is about"""
    from pyannote_video_amd import models
    from pyannote_video_amd.runtime import Context
    monkeypatch.setenv(knob, str(value))                             # (read in ml_plan when a context builds the plan of a size)
    c = Context(device=0, detector=models.DEFAULT_DETECTOR)
    bad, compared, changed = [], 0, 0
    try:
        for name in dc.CHUNK_SIZES:
            g = dc.by_name(name)
            fnp = dc.case_frame(g, "noise")
            tag = "%s_%s%d" % (name, knob, value)
            with _uploaded(c, fnp) as fr, _uploaded(ctx, fnp) as fr0:
                for l, d in dc.scored(g.lv):
                    p, p0 = c.level_plan(fr, g.up, l), ctx.level_plan(fr0, g.up, l)
                    assert (p["w"], p["h"], p["hog_nc"], p["hog_nr"]) == d == (p0["w"], p0["h"], p0["hog_nc"], p0["hog_nr"]), (tag, l, p, p0)
                    assert p["chunks"] == _ceil(d[3], p["chunk_rows"]) and p["roll_nseg"] == _ceil(d[3], p["roll_rows"]), (tag, l, p)
                    if knob == "PVF_FHOG_CHUNK":                     # chunks of about `value` rows, never fewer than two per level
                        assert 1 <= p["chunk_rows"] <= max(value, _ceil(d[3], 2)), (tag, l, p)
                        assert (p["roll_rows"], p["roll_nseg"]) == (p0["roll_rows"], p0["roll_nseg"]), (tag, l, p, p0)
                        changed += int((p["chunk_rows"], p["chunks"]) != (p0["chunk_rows"], p0["chunks"]))
                    else:                                            # pieces of at most `value` rows, rounded up to an even height
                        assert 2 <= p["roll_rows"] <= (max(2, value) + 1) // 2 * 2 and p["roll_rows"] % 2 == 0, (tag, l, p)
                        assert (p["chunk_rows"], p["chunks"]) == (p0["chunk_rows"], p0["chunks"]), (tag, l, p, p0)
                        changed += int((p["roll_rows"], p["roll_nseg"]) != (p0["roll_rows"], p0["roll_nseg"]))
                bad += _features(c, oracle, det, fr, g, "noise", 0, tag)
                with _Screening(c, False):                           # the dense kernel: the one PVF_SCORE_SEG cuts into pieces
                    for adj in (0.0, dc.ALL_PASS):
                        bad += _same_raw(tag + "_%r" % adj, c.detect_raw(fr, g.up, adj), _ref_raw(det, g, "noise", 0, adj))
                        compared += 1
                bad += _same_raw(tag + "_screened", c.detect_raw(fr, g.up, dc.ALL_PASS), _ref_raw(det, g, "noise", 0, dc.ALL_PASS))
                compared += 1
                assert len(_ref_raw(det, g, "noise", 0, dc.ALL_PASS)) == g.pairs
    finally:
        c.close()
    assert not bad, bad[:10]
    assert compared == 3 * len(dc.CHUNK_SIZES) and changed > 0, (compared, changed)


# ---- g: content the renderer never makes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.CONTENT_SIZES)
def test_every_content_equals_the_oracle(ctx, oracle, det, name):
    """... and no content, the saturated checkerboards least of all, drives the screening pass into a retry: a retry here (the list holds
    2^20 pairs, these frames have at most 60 000) would be a feature above the bound the error analysis assumes"""
    g = dc.by_name(name)
    bad = []
    for content, _ in dc.CONTENT:
        tag = "%s_%s" % (name, content)
        with _uploaded(ctx, dc.case_frame(g, content)) as fr:
            bad += _pyramid(ctx, det, fr, g, content, 0, tag)
            bad += _features(ctx, oracle, det, fr, g, content, 0, tag)
            bad += _dense_and_screened(ctx, det, fr, g, content, 0, dc.ALL_PASS, tag)
            assert len(_ref_raw(det, g, content, 0, dc.ALL_PASS)) == g.pairs
    assert not bad, bad[:10]


# ---- h: after other work on the same context ---------------------------------------------------------------------------------------------
def test_odd_sizes_after_tracker_work_and_after_each_other(ctx, det, small_video):
    """plans of different sizes take turns on the pyramid and feature scratch (and the tracker uses the feature scratch too): every
    window of an odd-sized frame, the zero border's included, after tracker work and after a detector call at another size"""
    f0, f1 = small_video.frame(0), small_video.frame(1)
    boxes = ctx.detect(f0, 1)[0]
    dbox = [tuple(float(v) for v in b) for b in boxes]
    assert dbox
    trk = ctx.tracker_create_many(len(dbox))
    ctx.tracker_start_many(trk, [f0] * len(dbox), dbox)
    ctx.tracker_update_many(trk, [f1] * len(dbox))
    bad = []
    order = [dc.by_name(n) for n in dc.AFTER_OTHER_WORK]
    try:
        for k, g in enumerate(order + order[::-1]):
            want = _ref_raw(det, g, "noise", 0, dc.ALL_PASS)
            assert len(want) == g.pairs and min(r[3] for r in want) == dc.FIRST and min(r[4] for r in want) == dc.FIRST
            with _uploaded(ctx, dc.case_frame(g, "noise")) as fr:
                for on in (False, True):
                    with _Screening(ctx, on):
                        bad += _same_raw("%s_after_%d_%s" % (g.name, k, "screened" if on else "dense"), ctx.detect_raw(fr, g.up, dc.ALL_PASS), want)
                ctx.tracker_update_many(trk, [f0] * len(dbox))        # tracker work between the sizes as well
    finally:
        ctx.tracker_destroy_many(trk)
    assert not bad, bad[:10]
