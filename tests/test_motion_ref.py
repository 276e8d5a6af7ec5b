"""CPU: MOTION.md's worked values on the restatement (tests/motion_ref.py), the proof that no intermediate reaches 2^63 at the caps, planted
defects shown to be seen by the comparison the GPU tests make on the inputs of tests/motion_cases.py, the sign and axis of the oracle's
flow, the camera rules on hand-made rows, the `motion` verb on a scripted context against a plain loop, and `transition --motion` on the
clip whose soft pan `transition` alone takes for a dissolve."""
import json

import numpy as np
import pytest

from pyannote_video_amd import blend, cli, motion, runtime
from tests import blend_ref as br, motion_cases as mc, motion_ref as mr


def fields(content, w=96, h=54):
    return mr.unpack(mc.reference(content, w, h)[1])


# ---- the row: hand cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", mc.SIZES)
def test_exact_models_come_back_exactly(w, h):
    P = w * h
    f = fields("translation", w, h)
    assert (f["TX16"], f["TY16"], f["A16"], f["B16"], f["m"]) == (96 << 16, -(40 << 16), 0, 0, 0)
    assert (f["n_valid"], f["n_in"], f["mag"], f["w"], f["h"], f["dfd_bits"], f["ms"], f["index"]) == (P, P, 136 * P, w, h, 0, 0, 0)
    f = fields("zoom", w, h)                                         # u = 3 X, v = 3 Y
    assert (f["TX16"], f["TY16"], f["A16"], f["B16"], f["m"], f["n_in"]) == (0, 0, 3 << 16, 0, 0, P)
    f = fields("roll", w, h)                                         # u = -2 Y, v = 2 X
    assert (f["TX16"], f["TY16"], f["A16"], f["B16"], f["m"], f["n_in"]) == (0, 0, 0, 2 << 16, 0, P)


@pytest.mark.parametrize("share,background", ((18, 4224), (37, 3264)))
def test_a_planted_foreground_is_trimmed_completely(share, background):
    flow, count = mc.planted(96, 54, share)
    assert count == background
    f = mr.unpack(mr.row_of(flow))
    tx, ty, a, b = mc.BACKGROUND
    assert (f["TX16"], f["TY16"], f["A16"], f["B16"], f["m"]) == (tx << 16, ty << 16, a << 16, b << 16, 0)
    assert (f["n_valid"], f["n_in"]) == (96 * 54, background)
    untrimmed = mr.unpack(mr.row_of(flow, defect="no_trimming"))
    assert untrimmed["TX16"] != tx << 16 and untrimmed["n_in"] == 96 * 54


def test_validity_clipping_and_the_smallest_sets():
    flow = mc.flow_of("nonfinite", 13, 17)
    bad = ~np.isfinite(flow).all(axis=2)
    assert bad.sum() > 20 and fields("nonfinite", 13, 17)["n_valid"] == 13 * 17 - bad.sum()
    for kill in (np.nan, np.inf, -np.inf):                          # a non-finite component invalidates its pixel, whichever it is
        for c in (0, 1):
            f = mc.flow_of("translation", 12, 12).copy()
            f[5, 7, c] = kill
            r = mr.unpack(mr.row_of(f))
            assert (r["n_valid"], r["n_in"], r["TX16"], r["TY16"], r["mag"]) == (143, 143, 96 << 16, -(40 << 16), 136 * 143)
    valid, u, v = mr.quantise(mc.flow_of("clip", 12, 12))           # +-3e6 pixels clip to +-2^20 sixty-fourths
    assert valid.all() and set(np.unique(u)) == set(np.unique(v)) == {-(1 << 20), 1 << 20}
    assert fields("clip", 12, 12)["mag"] == 2 * 144 << 20
    _, u, _ = mr.quantise(np.array([[[0.5 / 64, 0], [1.5 / 64, 0], [2.5 / 64, 0], [-0.5 / 64, 0], [-1.5 / 64, 0], [3e38, 0]]], np.float32))
    assert u.tolist() == [[0, 2, 2, 0, -2, 1 << 20]]                # half to even; 64 f overflows float32 and still clips
    f = fields("one_valid", 12, 12)                                 # den = 0: the translation is the pixel's flow
    assert (f["n_valid"], f["n_in"], f["TX16"], f["TY16"], f["A16"], f["B16"], f["m"]) == (1, 1, 80 << 16, 0, 0, 0, 0)
    f = fields("two_valid", 12, 12)                                 # two pixels fix the four parameters: the residual is the flooring's
    assert (f["n_valid"], f["n_in"]) == (2, 2) and f["m"] < 8 and (f["A16"], f["B16"]) != (0, 0)
    assert fields("three_valid", 12, 12)["n_in"] == 3
    row = mc.reference("none_valid", 12, 12)[1]
    assert not row[:9].any() and row[9] == 12 | 12 << 16


def test_both_number_systems_agree_on_every_case():
    for w, h in mc.SIZES[:4]:
        for content in mc.CONTENTS:
            flow, row = mc.reference(content, w, h)
            assert np.array_equal(mr.row_of(flow, ints=True), row), (content, w, h)
    rows = mr.rows_of(np.stack([mc.flow_of(c, 13, 17) for c in ("noise", "zoom")]), dfd=np.array([1.5, 0.0]))
    assert rows.shape == (2, 10) and rows[0, 7] == np.float64(1.5).view(np.int64) and rows[1, 7] == 0
    assert mr.rows_of(np.zeros((0, 12, 12, 2), np.float32)).shape == (0, 10)
    with pytest.raises(AssertionError):
        mr.row_of(np.zeros((129, 128, 2), np.float32))              # beyond the cap nothing is promised


# ---- the overflow proof --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", mc.CAP_SIZES)
def test_no_intermediate_reaches_2_63_at_the_caps(w, h):
    most = {}
    for content in mc.WORST + ("clip", "halves"):
        flow, row = mc.reference(content, w, h)
        track = mr.Track()
        assert np.array_equal(mr.row_of(flow, ints=True, track=track), row), content       # Python ints cannot wrap: int64 did not either
        for name, value in track.most.items():
            most[name] = max(most.get(name, 0), value)
    print(w, h, {k: "2^%.1f" % np.log2(max(v, 1)) for k, v in sorted(most.items(), key=lambda kv: -kv[1])[:8]})
    assert max(most.values()) < 1 << 63
    # MOTION.md "Bounds"
    assert most["n*Pp"] <= 1.4e17 and most["SX*Su"] <= 1 << 56 and most["numA"] < 1 << 59
    assert most["A16.rem<<16"] <= 4.1e17 and most["den"] << 16 <= 4.1e17
    assert most["numTX"] < 1 << 62 and most["numTY"] < 1 << 62 and most["sum ru+rv"] < 1 << 62
    if (w, h) == (256, 64):
        full = mr.Track()
        mr.row_of(mc.flow_of("zoom", w, h), ints=True, track=full)
        assert full.most["den"] == 16384 * (64 * 256 * (256 ** 2 - 1) // 3 + 256 * 64 * (64 ** 2 - 1) // 3) and 4.0e17 < full.most["den"] << 16 <= 4.1e17


# ---- planted defects ------------------------------------------------------------------------------------------------------------------
def seen(defect, content, w, h):
    flow, row = mc.reference(content, w, h)
    return not np.array_equal(mr.row_of(flow, defect=defect), row)


def test_the_comparison_sees_every_planted_defect():
    assert set(mr.DEFECTS) == {"components_swapped", "x_not_centred", "truncating_division", "no_trimming", "tau_without_floor",
                               "round_half_up", "one_round_fewer", "n_in_from_next_set"}
    for w, h in ((12, 12), (96, 54)):
        assert seen("components_swapped", "translation", w, h) and seen("components_swapped", "roll", w, h)
        assert seen("x_not_centred", "zoom", w, h) and not seen("x_not_centred", "translation", w, h)
        assert seen("truncating_division", "translation", w, h)      # TY16 < 0 ...
        assert seen("truncating_division", "noise", w, h)            # ... and negative A16
        assert seen("no_trimming", "planted18", w, h) and seen("no_trimming", "noise", w, h)
        assert seen("round_half_up", "ties", w, h) and not seen("round_half_up", "noise", w, h)
        assert seen("one_round_fewer", "planted37", w, h)            # 37 % of foreground takes all four fits to shed
        assert seen("n_in_from_next_set", "ties", w, h) and seen("n_in_from_next_set", "clip", w, h)
    # tau = floor(sum / n) against 2 floor(sum / 2 n): they differ by one, and by a pixel only where a residual sits on the odd value
    assert seen("tau_without_floor", "tau_edge", 12, 12)
    assert not any(seen("tau_without_floor", c, 12, 12) for c in mc.CONTENTS if c != "tau_edge")
    f = fields("tau_edge", 12, 12)
    assert (f["n_in"], f["TX16"], f["m"]) == (48, 17 << 16, 0)


# ---- the oracle's flow: sign and axis -------------------------------------------------------------------------------------------------
def test_component_0_is_horizontal_and_positive_to_the_right():
    from oracle import oracle
    from tests import blend_cases as bc
    big = bc._texture(np.random.default_rng(9), 80, 120)[:, :, 0]    # smoothed noise
    prev = np.rint(big[10:64, 10:106]).astype(np.uint8)
    cur = np.rint(big[7:61, 8:104]).astype(np.uint8)                 # the content moved right by 2 and down by 3
    for a, b, sx, sy in ((prev, cur, 1, 1), (cur, prev, -1, -1)):
        f = mr.unpack(mr.row_of(oracle.farneback(a, b)))
        tx, ty = f["TX16"] / float(1 << 22), f["TY16"] / float(1 << 22)
        print("translation in pixels", tx, ty, "inliers", f["n_in"], "zoom, roll", f["A16"], f["B16"])
        assert sx * tx > 0 and sy * ty > 0 and abs(tx) < abs(ty)                      # right and down; the larger one is vertical
    only_x = mr.unpack(mr.row_of(oracle.farneback(prev, np.rint(big[10:64, 8:104]).astype(np.uint8))))
    assert only_x["TX16"] > 0 and abs(only_x["TY16"]) < abs(only_x["TX16"]) / 4
    only_y = mr.unpack(mr.row_of(oracle.farneback(prev, np.rint(big[7:61, 10:106]).astype(np.uint8))))
    assert only_y["TY16"] > 0 and abs(only_y["TX16"]) < abs(only_y["TY16"]) / 4


# ---- the camera rules on hand-made rows ---------------------------------------------------------------------------------------------
def make_rows(specs, fps=25.0, w=96, h=54, first=0):
    """specs: per frame (tx, ty, a) in pixels, pixels, scale per frame -- or None for a pair without enough inliers"""
    rows = np.zeros((len(specs), 10), np.int64)
    for k, s in enumerate(specs):
        rows[k, 9] = w | h << 16
        if k == 0:
            continue
        if s is None:
            rows[k, 0] = 5184 | 100 << 32
            continue
        rows[k, 0] = 5184 | 5000 << 32
        rows[k, 1], rows[k, 2], rows[k, 3] = int(round(s[0] * (1 << 22))), int(round(s[1] * (1 << 22))), int(round(s[2] * (1 << 21)))
    return mr.stamp(rows, fps, first)


def kinds(found):
    return [(k, s, e) for k, s, e, _ in found]


def test_every_label_and_its_name():
    # 1 pixel of 96 a frame at 25 frames a second is 260 thousandths of the width a second; thresholds: 50 (pan, tilt) and 30 (zoom)
    for spec, kind, rate in (((1.0, 0, 0), "pan-left", 250), ((-1.0, 0, 0), "pan-right", -250), ((0, 0.54, 0), "tilt-up", 250),
                             ((0, -0.54, 0), "tilt-down", -250), ((0, 0, 0.01), "zoom-in", 250), ((0, 0, -0.01), "zoom-out", -250),
                             ((0.1, 0.05, 0.0005), "static", 0)):
        rows = make_rows([spec] * 30)
        assert mr.frame_rates(rows[5])[:3] == tuple(int(np.floor(1000 * v / s + 0.5)) for v, s in zip(spec, (96, 54, 1)))
        found = mr.camera(rows)
        assert found == [(kind, 1, 29, rate)], (spec, found)
        assert motion.analyse(rows) == found
        assert mr.camera_report(rows) == motion.report(rows, found) == [{"kind": kind, "start": 0.04, "end": 1.16, "first": 1, "last": 29, "rate": rate}]
    # the largest |rate| / threshold names the row: a zoom of 5 % a second beats a pan of 7.5 % (5 / 3 against 7.5 / 5), not one of 10 %
    assert kinds(mr.camera(make_rows([(0.288, 0, 0.002)] * 30))) == [("zoom-in", 1, 29)]
    assert kinds(mr.camera(make_rows([(0.384, 0, 0.002)] * 30))) == [("pan-left", 1, 29)]
    assert kinds(mr.camera(make_rows([(0.288, 0, 0.002)] * 30), zoom=6.0)) == [("pan-left", 1, 29)]
    # the rates are whole thousandths a frame: 0.27 pixels of 96 are 2.8 and count as 3
    assert mr.frame_rates(make_rows([(0.27, 0, 0.0016)] * 2)[1]) == (3, 0, 2, 0)


def test_bridging_dropping_shots_and_unreliable_rows():
    pan, still = (1.0, 0, 0), (0, 0, 0)
    # a gap of 4 unreliable rows (0.2 s between its neighbours) is bridged, one of 6 is not
    rows = make_rows([pan] * 20 + [None] * 4 + [pan] * 20)
    assert kinds(mr.camera(rows)) == [("pan-left", 1, 43)]
    rows = make_rows([pan] * 20 + [None] * 6 + [pan] * 20)
    assert kinds(mr.camera(rows)) == [("pan-left", 1, 19), ("pan-left", 26, 45)]
    assert kinds(mr.camera(rows, max_gap=0.3)) == [("pan-left", 1, 45)]
    assert kinds(mr.camera(rows, min_inliers=1)) == [("pan-left", 1, 45)]             # 100 of 5184 pixels are 1.9 %
    assert kinds(mr.camera(rows, min_duration=0.75)) == [("pan-left", 26, 45)]        # 18 frames are 0.72 s
    assert mr.camera(make_rows([pan] * 10)) == []                                      # 0.32 s
    assert mr.camera(make_rows([None] * 40)) == [] and mr.camera(np.zeros((0, 10), np.int64)) == []
    # the window: the label turns where the window's mean crosses the threshold, within half a window of the change
    rows = make_rows([still] * 30 + [pan] * 30)
    found = kinds(mr.camera(rows))
    assert [k for k, _, _ in found] == ["static", "pan-left"] and found[0][2] + 1 == found[1][1] and 30 - 7 <= found[1][1] <= 30
    assert kinds(mr.camera(rows, window=0.0)) == [("static", 1, 29), ("pan-left", 30, 59)]
    # shots: the pair across a boundary does not count, windows and spans stay inside their shot
    rows = make_rows([pan] * 30 + [still] * 30)
    shots = [(0.0, 1.2), (1.2, 2.4)]
    assert kinds(mr.camera(rows, shots=shots)) == [("pan-left", 1, 29), ("static", 31, 59)]
    rows = make_rows([pan] * 60)
    assert kinds(mr.camera(rows, shots=shots)) == [("pan-left", 1, 29), ("pan-left", 31, 59)]
    assert kinds(mr.camera(rows, shots=[(0.0, 1.2)])) == [("pan-left", 1, 29)]        # frames outside every shot have no label
    for kw in (dict(), dict(shots=shots), dict(window=0.2, max_gap=0.0), dict(pan=30.0, zoom=0.5), dict(min_inliers=97)):
        rows = make_rows([pan] * 12 + [None] * 3 + [(0, 0, 0.004)] * 20 + [still] * 9 + [(0, -0.4, 0)] * 25)
        assert motion.analyse(rows, **kw) == mr.camera(rows, **kw), kw                  # the package against the restatement
    with pytest.raises(ValueError, match="above 0"):
        motion.analyse(rows, pan=0.0)


# ---- the verbs --------------------------------------------------------------------------------------------------------------------------
class Dev(object):
    def __init__(self, rgb):
        self.rgb, self.released = rgb, False

    def release(self):
        assert not self.released
        self.released = True


class Ring(object):
    def __init__(self, ctx):
        self.ctx = ctx

    def push(self, rgb):
        d = Dev(rgb)
        self.ctx.live.append(d)
        return d

    def close(self):
        pass


class ScriptContext(object):
    """shot_motion is the oracle's flow and the restatement's rows, one pair at a time; given: every frame an earlier call was given --
    its last is carried as the first of the next, no other"""

    def __init__(self):
        self.live, self.calls, self.known, self.given = [], [], {}, []

    def ingest_ring(self, h, w, depth=16):
        return Ring(self)

    def shot_motion(self, frames, width, height, tables, want_dfd=True):
        from oracle import oracle
        assert all(not f.released for f in frames), "a row asked of a released frame"
        assert all(f.released for f in self.given if f is not frames[0]), "a frame of an earlier call, not the carried one, is still resident"
        self.given.extend(frames)
        self.calls.append(len(frames))
        rows = []
        for a, b in zip(frames[:-1], frames[1:]):
            key = (id(a.rgb), id(b.rgb), width, height)
            if key not in self.known:
                ga, gb = oracle.shot_convert(a.rgb, width, height), oracle.shot_convert(b.rgb, width, height)
                flow = oracle.farneback(ga, gb)
                self.known[key] = mr.row_of(flow, int(np.float64(oracle.shot_dfd_from_flow(ga, gb, flow)).view(np.int64)))
            rows.append(self.known[key])
        return (np.stack(rows) if rows else np.zeros((0, 10), np.int64)), None

    def mem_info(self):
        return 0, 0


class ClipVideo(object):
    def __init__(self, frames, fps):
        self.frames, self.frame_rate = frames, fps
        self.frame_size = self.size = (frames[0].shape[1], frames[0].shape[0])

    def __len__(self):
        return len(self.frames)

    def frame(self, i):
        return self.frames[i]

    def __iter__(self):
        for i, f in enumerate(self.frames):
            yield i / self.frame_rate, f


@pytest.fixture(scope="module")
def clip():
    c = mc.camera_clip()
    tw, th = mr.tile_size(mc.CLIP_WIDTH, mc.CLIP_W, mc.CLIP_H)
    return c, mc.oracle_rows(c.frames, tw, th)


def check_labels(found, parts, slack=7):
    """the planted parts in order, every change within half a window (0.25 s: 6 frames, and one for the pair) of where it was planted"""
    assert [f["kind"] for f in found] == [p[0] for p in parts], found
    for f, (_, first, last) in zip(found, parts):
        assert abs(f["first"] - max(first, 1)) <= slack and abs(f["last"] - last) <= slack, (f, first, last)


def test_the_restatement_alone_labels_the_clip(clip):
    c, rows = clip
    assert rows.shape == (len(c.frames), 10) and (rows[:, 9] == (96 | 54 << 16)).all() and rows[0, 0] == 0 and (rows[1:, 0] & 0xFFFFFFFF == 5184).all()
    found = mr.camera_report(rows)
    print(found)
    check_labels(found, c.parts)
    assert found[1]["rate"] < -150 and found[2]["rate"] > 150       # 260 and 250 were planted; Farneback's flow falls short, see MOTION.md
    assert motion.report(rows, motion.analyse(rows)) == found


def test_motion_through_main_equals_the_plain_loop_at_every_batch(tmp_path, monkeypatch, clip):
    c, want = clip
    ctx = ScriptContext()
    monkeypatch.setattr(runtime, "default_context", lambda: ctx)
    monkeypatch.setattr(cli, "open_video", lambda spec, fps, **kw: ClipVideo(c.frames, mc.FPS))
    n, files = len(c.frames), {}
    for batch in (1, 7, 256):
        ctx.calls[:] = []
        files[batch] = str(tmp_path / ("motion%d.npy" % batch))
        assert cli.main(["motion", "--batch", str(batch), "film", files[batch]]) == 0
        sizes = [batch] * (n // batch) + ([n % batch] if n % batch else [])
        assert ctx.calls == [sizes[0]] + [s + 1 for s in sizes[1:]]                 # every later call starts with the frame kept from the one before
        assert all(f.released for f in ctx.live)
        got = np.load(files[batch])
        assert got.dtype == np.int64 and np.array_equal(got, want), batch
    assert open(files[1], "rb").read() == open(files[7], "rb").read() == open(files[256], "rb").read()
    out = str(tmp_path / "camera.json")
    assert cli.main(["camera", files[7], out]) == 0
    assert json.load(open(out)) == mr.camera_report(want)
    assert cli.main(["camera", "--pan", "50", "--window", "0.2", files[7], "-"]) == 0
    # a range of the video: the first row of the range has no pair
    assert cli.main(["motion", "--from", "0.4", "--until", "2.0", "film", files[1]]) == 0
    part = np.load(files[1])
    assert len(part) == 40 and part[0, 0] == 0 and part[0, 8] == 400 | 10 << 32 and np.array_equal(part[1:], want[11:50])
    a = cli.parse_args(["motion", "-", "motion.npy"])
    assert (a.video, a.output, a.width, a.t_from, a.t_until, a.batch) == ("-", "motion.npy", 96, 0.0, None, 256)
    a = cli.parse_args(["camera", "motion.npy", "out.json"])
    assert (a.pan, a.zoom, a.window, a.min_inliers, a.min_duration, a.max_gap, a.shots) == (5.0, 3.0, 0.5, 50, 0.5, 0.2, None)
    # refusals
    bad = str(tmp_path / "bad.npy")
    np.save(bad, np.zeros((3, 10), np.int32))
    for args in (["camera", bad, out], ["camera", "--pan", "0", files[7], out], ["motion", "--width", "8", "film", bad],
                 ["motion", "--width", "300", "film", bad], ["transition", "--motion", bad, bad, out]):
        with pytest.raises(SystemExit):
            cli.main(args)


def test_the_carrier_hands_back_all_but_the_frame_it_carries(clip):
    """measure -> (rows, the frames the caller may release now): the one held from before and all but the last of the call's;
    ScriptContext checks at every call that no other is left"""
    c, want = clip
    ctx = ScriptContext()
    carry = motion.Pairs(ctx, 96, 54)
    frames = [Dev(f) for f in c.frames[:7]]
    parts, held = [], []
    for part in (frames[:3], frames[3:6], frames[6:]):
        rows, done = carry.measure(part)
        assert len(rows) == len(part) and sorted(map(id, done)) == sorted(map(id, held + part[:-1]))
        parts.append(rows)
        for f in done:
            f.release()
        held = part[-1:]
    assert ctx.calls == [3, 4, 2] and [f.released for f in frames] == [True] * 6 + [False] and carry.held is frames[6]
    assert np.array_equal(np.concatenate(parts)[:, :8], want[:7, :8])                # (word 8 is the verb's stamp)


def test_transition_with_motion_takes_the_soft_pan_out_of_the_dissolves(tmp_path):
    c = mc.soft_pan_clip()
    parts = {kind: (a, b) for kind, a, b in c.parts if kind in ("dissolve", "pan")}
    blend_rows = br.video_rows(c.frames, 32, 18, 25.0)
    alone = br.report(blend_rows)
    assert [f["kind"] for f in alone] == ["dissolve", "dissolve"]                   # BLEND.md's limit: the pan is the second one
    assert parts["pan"][0] <= alone[1]["first"] and alone[1]["last"] <= parts["pan"][1] + 1
    motion_rows = mc.oracle_rows(c.frames, 96, 54)
    moves = [f for f in mr.camera_report(motion_rows) if f["kind"] in mr.MOVING]
    assert [f["kind"] for f in moves] == ["pan-right"] and abs(moves[0]["first"] - parts["pan"][0]) <= 7
    assert motion.moving_frames(motion_rows) == mr.frames_in_motion(motion_rows)
    b, m, out, out2, shots, refined = (str(tmp_path / n) for n in ("b.npy", "m.npy", "out.json", "out2.json", "shots.json", "refined.json"))
    np.save(b, blend_rows)
    np.save(m, motion_rows)
    json.dump({"pyannote": "Timeline", "content": [{"start": 0.0, "end": 1.7}, {"start": 1.7, "end": 3.48}]}, open(shots, "w"))
    assert cli.main(["transition", "--motion", m, "--shots", shots, "--refined", refined, b, out]) == 0
    found = json.load(open(out))
    assert [f["kind"] for f in found] == ["dissolve", "camera"]
    assert found[0] == alone[0] and {k: found[1][k] for k in ("start", "end", "first", "last")} == {k: alone[1][k] for k in ("start", "end", "first", "last")}
    cut = (alone[0]["first"] + alone[0]["last"]) // 2 / 25.0
    assert [(s.start, s.end) for s in cli.load_shots(refined)] == [(0.0, cut), (cut, 1.7), (1.7, 3.48)]     # the pan cuts nothing
    # without the flag every byte is what it was
    assert cli.main(["transition", b, out2]) == 0
    assert json.load(open(out2)) == alone and open(out2).read() == json.dumps(alone, indent=1) + "\n"
    assert blend.analyse(blend_rows) == br.transitions(blend_rows)
