"""Who shares which scratch arena of a context (the `DevBuf s_*` members of Ctx, csrc/pvf_internal.h; the table in csrc/ctx.hip says which
of them are call-local), and two steps per sharer for tests/test_gpu_scratch_sharers.py.

SHARERS restates the `ensure` calls of csrc/*.hip as data: {arena: [user, ...]}.  A user is one verb (kernel family) with the entries it
runs here (USERS says which).  The GPU test holds the table against the library: after a user's `small` step on a fresh context
exactly the call-local arenas listed for it have grown.

A step is a function (ctx) -> [arrays].  It makes the call(s), compares the result with the verb's own reference under the equality the
verb's own GPU test uses (np.array_equal against tests/*_ref.py or the oracle; the distance tables' rtol / atol of test_gpu_identify.py;
the embedder bit for bit against the same call on a fresh context and to 1e-4 against the hot-path fixture), and returns what it
compared, so that a caller can also hold two runs of one step against each other bit for bit.  Inputs and references are made once per
process and shared read-only.

`small` is the smallest input of the verb's own case table.  `large` is the smallest input that grows every arena the user shares past
every sharer's `small`, with content that is neither 0 nor a plausible count.  Two smalls are larger than they look and set the sizes of
the others: one window of pvf_frame_hist takes a round of 2^18 pieces (8 MiB of s_act0) whatever its size, and ORB's smallest image with
a level takes ~170 KB of s_misc at 64 keypoint rows.  Hence 20 chips for the embedder, but 1400 for `talk`; 560 planes of 16384 pixels,
1200 text frames and a 2000 x 1500 sheet; and for s_misc 2300 tracks for the agglomeration, 320 boxes and 7500 query groups.  The GPU
test asserts from Context.scratch() that each large really left the arena larger than the small that follows it needs.

configure(model_paths, ref_ctx) must be called before a step runs: the synthetic models' paths, and the context the reference distance
matrices of the agglomeration are computed on (the session context: its buffers are not under test)."""
import collections
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "pyannote-video_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# ---- the table ------------------------------------------------------------------------------------------------------------------------
SHARERS = {
    "s_act0": ["embed", "blend", "motion", "text", "prints", "clothes", "thumbs", "talk", "faces"],
    "s_act1": ["embed"],
    "s_act2": ["embed"],
    "s_emb_flags": ["embed"],
    "s_trk0": ["tracker", "embed", "jitter", "chip", "thumbs", "talk", "faces"],
    "s_trk1": ["tracker"],
    "s_trk2": ["tracker"],
    "s_trkfeat": ["tracker"],
    "s_jit": ["jitter"],
    "s_clu0": ["pair_dist", "hac", "identify", "search", "cast", "runs"],
    "s_clu1": ["pair_dist", "hac", "identify", "search", "cast", "runs"],
    "s_misc": ["landmarks", "hac", "orb", "shot", "identify"],
    "s_chip": ["chip", "jitter", "tracker"],    # (the tracker cuts its 64 x 64 windows with chip.hip's chip_extract_batch)
    "s_chip_pyr": ["chip", "tracker"],
    "s_orb_set": ["orb"],                    # holds state (the resident descriptor sets): reported, never filled
    "s_orb_work": ["orb"],
}
# the arenas more than one user carves, as the pair test walks them (the two clustering buffers have the same users: one walk)
SHARED = [("s_act0",), ("s_trk0",), ("s_clu0", "s_clu1"), ("s_misc",), ("s_chip",), ("s_chip_pyr",)]
FILLS = (0x00, 0xFF, 0xA5)
TOL = {0: dict(rtol=1e-12, atol=1e-13), 1: dict(rtol=1e-10, atol=1e-12)}      # pair and gallery mean distances: Euclidean, cosine

_CFG = {}


def configure(model_paths, ref_ctx):
    _CFG["models"], _CFG["ref_ctx"] = tuple(model_paths), ref_ctx


def open_context(kinds=()):
    """a fresh context: a detector, and the landmark model / the embedder where a step of `kinds` needs it"""
    from pyannote_video_amd.runtime import Context
    lp, ep = _CFG["models"]
    return Context(device=0, landmarks=lp if "landmarks" in kinds else None, embedding=ep if "embedder" in kinds else None)


def arenas_of(user):
    return sorted(a for a, users in SHARERS.items() if user in users)


def _oracle():
    from oracle import oracle as o
    o.lib()
    return o


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError((what, "%d differ, first at %s: %s against %s" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])))


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


class _uploaded(object):
    """the frames on the device for a block; an array that appears more than once in the list is uploaded once"""

    def __init__(self, ctx, frames):
        self.ctx, self.frames = ctx, frames

    def __enter__(self):
        self.known = {}
        for f in self.frames:
            if id(f) not in self.known:
                self.known[id(f)] = self.ctx.upload(f)
        return [self.known[id(f)] for f in self.frames]

    def __exit__(self, *a):
        for d in self.known.values():
            d.release()


@functools.lru_cache(maxsize=None)
def _video():
    from pyannote_video_amd import synth
    return synth.SyntheticVideo(width=640, height=360, n_frames=12, n_shots=2, faces=3, min_face=50, max_face=110, seed=7)   # conftest's small_video


@functools.lru_cache(maxsize=None)
def _noise_chips(n, seed):
    c = np.random.default_rng(seed).integers(0, 256, (n, 150, 150, 3), dtype=np.uint8)
    c.setflags(write=False)
    return c


# ---- embedder -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gold():
    g = np.load(os.path.join(HERE, "golden", "hotpath_small.npz"))
    return _frozen(np.ascontiguousarray(g["chips"]), np.ascontiguousarray(g["embeddings"]))


@functools.lru_cache(maxsize=None)
def _embed_case(size):
    chips, emb = _gold()
    if size == "small":
        return _frozen(np.ascontiguousarray(chips[:1]), emb[:1])
    return _frozen(np.ascontiguousarray(np.concatenate([chips, _noise_chips(20 - len(chips), 31)])), emb)


@functools.lru_cache(maxsize=None)
def _embed_fresh(size):
    """the same call on a context that has done nothing else"""
    c = open_context(("embedder",))
    try:
        return _frozen(c.embed_chips(_embed_case(size)[0]))[0]
    finally:
        c.close()


def _embed(size, ctx):
    chips, gold = _embed_case(size)
    got = ctx.embed_chips(chips)
    _same(got.view(np.uint32), _embed_fresh(size).view(np.uint32), ("embed", size, "against a fresh context"))
    err = float(np.linalg.norm(got[:len(gold)] - gold, axis=1).max())
    assert err <= 1e-4, ("embed", size, "against the oracle's descriptors", err)
    return [got]


# ---- blend (pvf_blend_measure, pvf_frame_blend) ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _blend_case(size):
    from tests import blend_cases as bc, blend_ref as br
    N, P, (w, h, tw, th), n = (1, 1, bc.FRAME_SIZES[0], 1) if size == "small" else (560, 16384, bc.FRAME_SIZES[6], 40)
    y = bc.planes("random", N, P)
    frames = bc.frames_of(w, h, n)
    rows, luma = br.frame_rows(frames, tw, th)
    return _frozen(y, br.rows_of(y)) + (frames, tw, th) + _frozen(rows, luma)


def _blend(size, ctx):
    y, want, frames, tw, th, rows, luma = _blend_case(size)
    got = ctx.blend_measure(y)
    _same(got, want, ("blend_measure", size))
    with _uploaded(ctx, frames) as devs:
        r, l = ctx.frame_blend(devs, tw, th)
    _same(l, luma, ("frame_blend luma", size))
    _same(r, rows, ("frame_blend", size))
    return [got, r, l]


# ---- motion (pvf_flow_motion) ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _motion_case(size):
    from tests import motion_cases as mc
    if size == "small":
        f, r = mc.reference("translation", 12, 12)
        return _frozen(f[None].copy(), r[None].copy())
    refs = [mc.reference(c, 128, 128) for c in ("noise", "planted37", "worst_pp", "nonfinite")]        # a row depends on its own flow only
    pick = [(5 * k + 1) % 4 for k in range(72)]
    return _frozen(np.stack([refs[p][0] for p in pick]), np.stack([refs[p][1] for p in pick]))


def _motion(size, ctx):
    flows, want = _motion_case(size)
    got = ctx.flow_motion(flows)
    _same(got, want, ("flow_motion", size))
    return [got]


# ---- text (pvf_frame_text) ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _text_case(size):
    from tests import text_cases as tc, text_ref as tr
    if size == "small":
        frames = tc.frames_of("noise", 1, 1, n=1)
        return (frames,) + _frozen(*tr.rows_of(frames))
    five = tc.frames_of("noise", 641, 359, n=5)
    n = 1200
    frames = [five[i % 5] for i in range(n)]
    rows, counts = tr.rows_of(frames[:11])                           # a row depends on its frame and the one before: from frame 1 on the rows repeat
    assert np.array_equal(rows[6:11], rows[1:6]) and np.array_equal(counts[6:11], counts[1:6]) and int(rows[1:6, 2:5].min()) > 0
    at = np.array([0] + [1 + (i - 1) % 5 for i in range(1, n)])
    return (frames,) + _frozen(rows[at], counts[at])


def _text(size, ctx):
    frames, rows, counts = _text_case(size)
    with _uploaded(ctx, frames) as devs:
        r, c = ctx.frame_text(devs, want_counts=True)
    _same(c, counts, ("frame_text counts", size))
    _same(r, rows, ("frame_text", size))
    return [r, c]


# ---- prints (pvf_frame_prints) --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _prints_case(size):
    from tests import repeat_cases as rc, repeat_ref as rr
    if size == "small":
        frames = [rc.make_frame(1, 1, "noise")]
        return (frames,) + _frozen(rr.prints(frames))
    some = [rc.make_frame(300, 37, "noise", seed=s) for s in range(4)] + [rc.make_frame(641, 359, "noise")]
    pick = [(3 * k + 2) % 5 for k in range(620)]
    return ([some[p] for p in pick],) + _frozen(rr.prints(some)[pick])


def _prints(size, ctx):
    frames, want = _prints_case(size)
    with _uploaded(ctx, frames) as devs:
        got = ctx.frame_prints(devs)
    _same(got, want, ("frame_prints", size))
    return [got]


# ---- clothes (pvf_frame_hist) ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _clothes_case(size):
    from tests import clothes_cases as cc, clothes_ref as cr
    if size == "small":
        f, wins, group, G, B = cc.frame_of("noise", 1, 1), np.array([(0, 0, 1, 1)], np.int32), np.zeros(1, np.int32), 1, 1
    else:
        f = cc.frame_of("noise", 641, 359)
        wins = cc.windows_for(641, 359)
        # a few hundred groups, three in four of them empty: 1.2 MB of rows behind the pieces, more than the slack the smallest call's buffer has
        group, G, B = (4 * np.arange(len(wins)) + 1).astype(np.int32), 4 * len(wins) + 4, 4
    return (f,) + _frozen(wins, group) + (G, B) + _frozen(cr.hist_of([f] * len(wins), wins, group, G, B))


def _clothes(size, ctx):
    f, wins, group, G, B, want = _clothes_case(size)
    with _uploaded(ctx, [f]) as devs:
        got = ctx.frame_hist(devs * len(wins), wins, group, G, bands=B)
    _same(got, want, ("frame_hist", size))
    return [got]


# ---- thumbs (pvf_thumb_sheet) ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _thumbs_case(size):
    from tests import storyboard_ref as sr
    from tests.test_gpu_storyboard import PRIMS, tiles
    if size == "small":
        t, xy, W, H, prims = tiles(1, 1, 1), [(0, 0)], 1, 1, ()
    else:
        th, tw, W, H = 113, 200, 2000, 1500
        t = tiles(24, th, tw)
        xy = [(-tw // 2, -th // 2), (W - tw // 2, 40), (300, H - th // 3), (W - 1, H - 1)] + [(37 + 241 * (k % 8), 211 + 389 * (k // 8)) for k in range(20)]
        prims = PRIMS
    return _frozen(t) + (xy, W, H, prims) + _frozen(sr.sheet(t, xy, W, H, (10, 20, 30), prims))


def _thumbs(size, ctx):
    from tests import storyboard_ref as sr
    t, xy, W, H, prims, want = _thumbs_case(size)
    got = ctx.thumb_sheet(t, xy, W, H, (10, 20, 30), prims)
    bad = sr.mismatch(got, want)
    assert bad is None, ("thumb_sheet", size, bad)
    return [got]


# ---- talk (pvf_chip_motion) -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _talk_case(size):
    from tests import talk_ref as tr
    distinct = tr.named_cases()["chain"][0] + [tr.smooth_chip(), tr.smooth_chip(-1, 2)]
    n = 2 if size == "small" else 1400
    chips = [distinct[(i * 5 + 3) % len(distinct)] for i in range(n)]
    prev = np.full(n, -1, np.int32)
    prev[1::3] = np.arange(n)[1::3] - 1                              # every third face follows its neighbour
    for i, p in ((n - 1, 0), (n // 2, 3), (n - 2, n // 2)):          # and a few follow faces far in front of them
        if 0 <= p < i:
            prev[i] = p
    return _frozen(np.stack(chips), prev, tr.motion(chips, prev))


def _talk(size, ctx):
    chips, prev, want = _talk_case(size)
    got = ctx.chip_motion(chips, prev)
    _same(got, want, ("chip_motion", size))
    return [got]


# ---- faces (pvf_chip_quality, pvf_chip_sheet) -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _faces_case(size):
    from tests import faces_ref as fr
    from tests.test_gpu_faces import _prims, batch
    if size == "small":
        _, chips, sums = batch(1)
        xy, S, W, H, prims = [(-20, -30)], 48, 1, 1, ()
    else:
        _, chips, sums = batch(20)
        S, W, H = 150, 2000, 1500
        xy = [(-S // 3, 20), (W - S // 2, 3), (S // 2, -S // 4), (S + 9, H - S // 3)] + [(41 + 283 * (k % 7), 199 + 401 * (k // 7)) for k in range(16)]
        prims = _prims(W, H)
    chips = np.ascontiguousarray(chips)
    return _frozen(chips, sums) + (xy, S, W, H, prims) + _frozen(fr.sheet(chips, xy, S, W, H, (10, 20, 30), prims))


def _faces(size, ctx):
    chips, sums, xy, S, W, H, prims, want = _faces_case(size)
    q = ctx.chip_quality(chips)
    _same(q, sums, ("chip_quality", size))
    sheet = ctx.chip_sheet(chips, xy, S, W, H, (10, 20, 30), prims)
    _same(sheet, want, ("chip_sheet", size))
    return [q, sheet]


# ---- tracker (pvf_tracker_start_many, pvf_tracker_update_many) ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tracker_case(size):
    import tracker_cases as tc
    from pyannote_video_amd import models
    v = _video()
    pics = [v.frame(i) for i in range(3)]
    boxes = tc.face_boxes(v, 0)[:1] if size == "small" else [b for _, b in tc.small_boxes()]          # one tracker; 30, one per box class
    case = tc.Case("scratch_" + size, pics, boxes)
    return case, tc.run_oracle(case, _oracle(), models.dsst_tables())


def _tracker(size, ctx):
    case, ref = _tracker_case(size)
    n = len(case.boxes)
    out = []
    trk = ctx.tracker_create_many(n)
    try:
        with _uploaded(ctx, case.frames) as devs:
            ctx.tracker_start_many(trk, [devs[0]] * n, case.boxes)
            for i in range(1, len(devs)):
                psr, pos = ctx.tracker_update_many(trk, [devs[i]] * n)
                want_psr = np.array([r["psr"][i - 1] for r in ref], np.float64)
                want_pos = np.stack([r["pos"][i - 1] for r in ref])
                assert np.array_equal(psr, want_psr, equal_nan=True), ("tracker confidence", size, i, psr.tolist(), want_psr.tolist())
                _same(pos, want_pos, ("tracker position", size, i))
                out += [psr, pos]
            for k, r in enumerate(ref):                              # the filters after the last update, bit for bit
                _, A, B = ctx.tracker_state(trk[k])
                As, Bs = ctx.tracker_scale_state(trk[k])
                for name, g, w in (("A", A, r["A"]), ("B", B, r["B"]), ("As", As, r["As"]), ("Bs", Bs, r["Bs"])):
                    _same(g, w, ("tracker state", size, k, name))
                out += [B, Bs]
    finally:
        ctx.tracker_destroy_many(trk)
    return out


# ---- jitter (pvf_debug_jitter_chips) and chip (pvf_debug_extract_chip) ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _jitter_case(size):
    from pyannote_video_amd import _lib
    from tests import jitter_ref as ref
    from tests.test_gpu_faces import batch
    n, J = (1, 1) if size == "small" else (20, 8)
    chips = np.ascontiguousarray(batch(n)[1])
    rows = [ref.row_of_library(r) for r in _lib.jitter_plan(J, 0)]
    o = _oracle()
    return _frozen(chips) + (J,) + _frozen(np.stack([np.stack([ref.jitter(o, c, r) for r in rows]) for c in chips]))


def _jitter(size, ctx):
    chips, J, want = _jitter_case(size)
    got = ctx.jitter_chips(chips, J)
    _same(got, want, ("jitter_chips", size))
    return [got]


@functools.lru_cache(maxsize=None)
def _chip_case(size):
    f = _video().frame(2)
    if size == "small":
        cases = [((100.5, 60.25, 108.5, 68.25), 1.0, 0.0, 8, 8)]
    else:                                        # the chips of test_gpu_parity.py, a four-level pyramid and one large chip
        cases = [((100.5, 60.25, 180.75, 140.0), 1.0, 0.0, 64, 64), ((50.0, 30.0, 450.0, 330.0), 1.0, 0.0, 64, 64),
                 ((200.0, 100.0, 330.0, 230.0), 0.9659258262890683, 0.25881904510252074, 150, 150), ((-40.0, -30.0, 120.0, 130.0), 1.0, 0.0, 64, 64),
                 ((300.0, 200.0, 320.0, 220.0), 0.8, 0.6, 150, 150), ((1000.0, 1000.0, 1100.0, 1100.0), 1.0, 0.0, 64, 64),
                 ((-60.0, -200.0, 700.0, 560.0), 1.0, 0.0, 16, 16), ((20.0, 10.0, 620.0, 350.0), 1.0, 0.0, 300, 300)]
    o = _oracle()
    return f, cases, _frozen(*[o.extract_chip(f, *c) for c in cases])


def _chip(size, ctx):
    f, cases, want = _chip_case(size)
    out = []
    with _uploaded(ctx, [f]) as devs:
        for c, w in zip(cases, want):
            got = ctx.extract_chip(devs[0], *c)
            _same(got, w, ("extract_chip", size, c))
            out.append(got)
    return out


# ---- the distance tables and what runs on them ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair_case(size):
    from tests import cluster_cases as cc
    from tests.test_gpu_scratch_regrow import _tracks
    if size == "small":
        X, rs = _tracks(2, [1, 1], 128)
    else:
        sizes = np.random.default_rng(1).integers(10, 25, 64)        # 64 tracks: a matrix in s_clu1 that is larger than the search's smallest arena
        sizes[7] = 40                            # spans three blocks of 16 rows
        X, rs = _tracks(3, sizes, 128)
    return _frozen(X, rs, _oracle().pair_mean_dist(X, rs), cc.cosine_mean_dist(X, rs))


def _pair_dist(size, ctx):
    X, rs, D0, D1 = _pair_case(size)
    out = []
    for metric, want in ((0, D0), (1, D1)):
        D = ctx.pair_mean_dist(X, rs, metric=metric)
        assert D.shape == want.shape and np.allclose(D, want, **TOL[metric]), ("pair_mean_dist", size, metric, float(np.abs(D - want).max()))
        out.append(D)
    return out


@functools.lru_cache(maxsize=None)
def _hac_case(size):
    """tracks with extents; the agglomeration's reference runs on the matrix the DEVICE computes (the reference context's), bit for bit:
    tests/cooccur_ref.py where it is quick enough, and the oracle's unchanged agglomeration on the stamped matrix (cooccur_ref.stamp:
    the second reference of test_gpu_cooccur.py) for the 2300 tracks that s_misc needs"""
    from tests import cooccur_ref as R
    T = 3 if size == "small" else 2300
    X, rs, ext = R.make(T, seed=11 if size == "small" else 12, identities=None if size == "small" else 2000, span=None if size == "small" else 3000.0)
    D = _CFG["ref_ctx"].pair_mean_dist(X, rs)
    if size == "small":
        labels, log = R.hac(D, np.diff(rs), 0.6, R.cooccur(ext))
    else:
        labels, log = _oracle().hac(R.stamp(D, ext), np.diff(rs), 0.6)
    return _frozen(X, rs, ext, labels, log) + (R.n_blocked(ext),)


def _hac(size, ctx):
    X, rs, ext, labels, log, blocked = _hac_case(size)
    got = ctx.cluster_tracks_cooccur(X, rs, 0.6, extent=ext)
    _same(got[0], labels, ("cluster_tracks_cooccur labels", size))
    _same(got[1], log, ("cluster_tracks_cooccur log", size))
    assert got[2] == blocked, ("cluster_tracks_cooccur blocked pairs", size, got[2], blocked)
    return [got[0], got[1]]


@functools.lru_cache(maxsize=None)
def _identify_case(size):
    from tests import identify_ref as ref
    from tests.test_gpu_identify import _blobs
    if size == "small":
        X, rs, G, gs = _blobs(3, [1], [1])
    else:                                        # the main case's 20 groups, and 7480 one-row groups behind them: s_misc holds four values a group
        X, rs, G, gs = ref.main_case()
        more = np.round(np.concatenate([X, G])[np.random.default_rng(9).integers(0, len(X) + len(G), 7480)] + 1e-3, 5)
        X, rs = np.concatenate([X, more]), np.concatenate([rs, rs[-1] + 1 + np.arange(len(more))]).astype(np.int32)
    from tests import identify_cases as ic
    mean = ref.mean_dist if size == "small" else ic.mean_dist_fast   # (the vectorised reference test_gpu_identify_layouts.py uses for long tables)
    return _frozen(X, rs, G, gs, mean(X, rs, G, gs, 0), mean(X, rs, G, gs, 1))


def _identify(size, ctx):
    from tests import identify_ref as ref
    X, rs, G, gs, D0, D1 = _identify_case(size)
    out = []
    for metric, threshold, want in ((0, 0.6, D0), (1, 0.3, D1)):
        best, bd, second, sd, D = ctx.identify(X, rs, G, gs, threshold, metric=metric, return_dist=True)
        assert D.shape == want.shape and np.allclose(D, want, **TOL[metric]), ("identify distances", size, metric, float(np.abs(D - want).max()))
        assert ref.same_picks((best, bd, second, sd), ref.pick(D, threshold)), ("identify decision on its own matrix", size, metric)
        out += [best, bd, second, sd, D]
    return out


@functools.lru_cache(maxsize=None)
def _search_case(size):
    from tests import search_cases as cases, search_ref as ref
    Q, X, k = (cases.blobs(3, 1), cases.blobs(2, 1), 1) if size == "small" else (cases.blobs(5, 20), cases.blobs(1, 600), 10)
    return _frozen(Q, X) + (k,) + _frozen(*ref.search(Q, X, k))


def _search(size, ctx):
    Q, X, k, idx, d2, count = _search_case(size)
    got = ctx.search(Q, X, k)
    for g, w, name in zip(got, (idx, d2, count), ("idx", "d2", "count")):
        _same(g, w, ("search", size, name))
    return list(got)


@functools.lru_cache(maxsize=None)
def _cast_case(size):
    from tests import cast_cases as cases, cast_ref as ref, search_cases
    N, k = (1, 1) if size == "small" else (300, 20)
    X, group = search_cases.blobs(4, N), (None if size == "small" else cases.groups_in_runs(N))
    idx, d2, count = ref.lists(X, k, -1, group)
    labels, comps = ref.cast(X, k, -1, 2000, 1000, group)
    return _frozen(X, group) + (k,) + _frozen(idx, d2, count, labels) + (comps,)


def _cast(size, ctx):
    X, group, k, idx, d2, count, labels, comps = _cast_case(size)
    got = ctx.cast_lists(X, k, -1, group)
    for g, w, name in zip(got, (idx, d2, count), ("idx", "d2", "count")):
        _same(g, w, ("cast_lists", size, name))
    lab, n = ctx.cast(X, k, -1, 2000, 1000, group)
    _same(lab, labels, ("cast labels", size))
    assert n == comps, ("cast components", size, n, comps)
    return list(got) + [lab]


@functools.lru_cache(maxsize=None)
def _runs_case(size):
    from tests import repeat_cases as rc, repeat_ref as rr
    case = rc.size_case(1, 1) if size == "small" else rc.size_case(1025, 1023)      # (2048 rows: 40 KB of s_clu0, more than the search's smallest tables)
    kws = [dict(tau=rc.TAU_RANDOM)] + ([] if size == "small" else [dict(tau=128, min_len=3)])          # the planted run; every pair matches
    return case, kws, _frozen(*[rr.runs(case.A, case.ua, case.B, case.ub, strip=rc.S, **kw) for kw in kws])


def _runs(size, ctx):
    case, kws, want = _runs_case(size)
    out = []
    for kw, w in zip(kws, want):
        got = ctx.print_runs(case.A, case.ua, case.B, case.ub, **kw)
        _same(got, w, ("print_runs", size, kw))
        out.append(got)
    return out


# ---- the other users of s_misc --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _landmarks_case(size):
    from pyannote_video_amd import models
    sp = _oracle().ShapePredictor(models.load_container(_CFG["models"][0]))
    frame = _video().frame(0)
    if size == "small":
        boxes = [(40, 30, 130, 120)]
    else:                                        # 320 boxes over the frame, some of them leaving it
        boxes = [(-20 + 31 * (k % 20), -10 + 19 * (k // 20), 70 + 31 * (k % 20) + 3 * (k % 7), 80 + 19 * (k // 20) + 5 * (k % 5)) for k in range(320)]
    return frame, boxes, _frozen(np.stack([sp(frame, b) for b in boxes]))[0]


def _landmarks(size, ctx):
    frame, boxes, want = _landmarks_case(size)
    with _uploaded(ctx, [frame]) as devs:
        got = np.asarray(ctx.landmarks(devs * len(boxes), boxes))
    _same(got.astype(want.dtype), want, ("landmarks", size))
    return [got]


ORB_SMALL_CAP = 64          # keypoint rows of the small step: s_misc holds 8 levels x cap slots per frame, 448 KB of them at the default cap


@functools.lru_cache(maxsize=None)
def _orb_case(size):
    import orb_check
    import orb_ref
    import thread_clip
    w, h, n, cap = (63, 200, 1, ORB_SMALL_CAP) if size == "small" else (160, 120, 3, None)       # test_gpu_scratch_regrow.py's geometries
    frames = [thread_clip.make_clip(width=w, height=h, frames_per_shot=1, setups="A", seed=3 + k)[0][0] for k in range(n)]
    ow, oh = orb_ref.thread_size(w, h, 200)
    refs = [orb_check.reference(f, ow, oh) for f in frames]
    pairs = [(a, b) for a in range(n) for b in range(n)]
    return frames, ow, oh, cap, refs, pairs, [orb_ref.match_count(refs[a][1], refs[b][1]) for a, b in pairs]


def _orb(size, ctx):
    import orb_check
    frames, ow, oh, cap, refs, pairs, want = _orb_case(size)
    with _uploaded(ctx, frames) as devs:
        counts, kp, desc = ctx.orb_extract(devs, ow, oh, cap)
    orb_check.assert_equal(counts, kp, desc, refs)
    matched = ctx.orb_match_counts(pairs)                            # the resident sets
    _same(matched, np.array(want, np.int32), ("orb_match_counts", size))
    return [counts, np.concatenate([desc[i, :counts[i]] for i in range(len(counts))]), matched]


@functools.lru_cache(maxsize=None)
def _shot_case(size):
    o = _oracle()
    v = _video()
    n, side = (2, 12) if size == "small" else (6, 64)                # 64 x 64: one coarser pyramid level, 508 KB of s_misc a pair
    frames = [v.frame(i)[40:200, 60:300].copy() for i in range(n)]
    tables = o.shot_tables()
    small = [o.shot_convert(f, side, side) for f in frames]
    flows = [o.farneback(small[i - 1], small[i], tables) for i in range(1, n)]
    dfd = np.array([o.shot_dfd(small[i - 1], small[i], tables) for i in range(1, n)], np.float64)
    return frames, side, _frozen(tables, np.stack(flows), dfd)


def _shot(size, ctx):
    frames, side, (tables, flows, dfd) = _shot_case(size)
    with _uploaded(ctx, frames) as devs:
        got_dfd, got_flow = ctx.shot_dfd(devs, side, side, tables, want_flow=True)
    _same(got_flow, flows, ("shot flow", size))
    _same(got_dfd, dfd, ("shot dfd", size))
    return [got_dfd, got_flow]


# ---- the users ------------------------------------------------------------------------------------------------------------------------
# kind: what the context must hold beside the detector.  exact: integers or oracle bits (a repeated step returns the same bits whatever
# lies in the arenas; the distance tables are held to their tolerance alone).  rounds: the knobs that cut the user's calls into rounds, at
# their smallest setting -- a later round then runs on the leftovers of the first.
User = collections.namedtuple("User", "name kind exact rounds run")
USERS = collections.OrderedDict((u.name, u) for u in (
    User("embed", "embedder", True, {}, _embed),
    User("blend", None, True, {"PVF_THUMB_ROUND": "1"}, _blend),
    User("motion", None, True, {}, _motion),
    User("text", None, True, {"PVF_TEXT_ROUND": "1"}, _text),
    User("prints", None, True, {}, _prints),
    User("clothes", None, True, {"PVF_HIST_ROUND": "1"}, _clothes),
    User("thumbs", None, True, {"PVF_THUMB_ROUND": "1"}, _thumbs),
    User("talk", None, True, {}, _talk),
    User("faces", None, True, {}, _faces),
    User("tracker", None, True, {}, _tracker),
    User("jitter", None, True, {"PVF_JITTER_CHUNK": "1"}, _jitter),
    User("chip", None, True, {}, _chip),
    User("pair_dist", None, False, {}, _pair_dist),
    User("hac", None, True, {}, _hac),
    User("identify", None, False, {}, _identify),
    User("search", None, True, {"PVF_SEARCH_CHUNK": "16"}, _search),
    User("cast", None, True, {"PVF_CAST_QBLOCK": "16", "PVF_SEARCH_CHUNK": "16"}, _cast),
    User("runs", None, True, {}, _runs),
    User("landmarks", "landmarks", True, {}, _landmarks),
    User("orb", None, True, {}, _orb),
    User("shot", None, True, {}, _shot),
))


def step(user, size):
    """(ctx) -> [arrays] of user's `small` or `large` step"""
    assert size in ("small", "large")
    return functools.partial(USERS[user].run, size)


def kinds_of(*users):
    return tuple(sorted(set(USERS[u].kind for u in users if USERS[u].kind)))
