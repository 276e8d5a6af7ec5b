"""CPU: num_jitters without a device (JITTER.md) -- the library's plan of the J transforms (pvf_jitter_plan, host only) against its
restatement in tests/jitter_ref.py; what the oracle makes of those transforms on an all-255 chip (black corners, blended values: where
a wrong box or a reordered blend would show); and the argument carried through the `extract` / `enroll` verbs and the dlib-like shim, on
the scripted contexts of tests/test_cli_host.py and tests/test_identify_ref.py."""
import numpy as np
import pytest

from pyannote_video_amd import _lib, cli, formats, runtime, shim
from tests import jitter_ref as ref
from tests.test_cli_host import ScriptContext as ExtractContext, ScriptVideo, make_tracks
from tests.test_identify_ref import ScriptContext as EnrollContext, _Frames


@pytest.mark.parametrize("J,seed", [(8, 0), (8, 1), (8, 2), (1, 0), (100, 0), (100, 2)])
def test_plan_equals_the_restatement(J, seed):
    rows = _lib.jitter_plan(J, seed)
    assert rows.shape == (J, _lib.JITTER_ROW)
    want = ref.plan(J, seed)
    for j in range(J):
        row, w = rows[j], want[j]
        assert bool(row[6]) == w["flip"] and row[6] in (0.0, 1.0)
        # the libm of the library and of Python may differ in the last place of cos / sin: 4 ulp
        assert ref.ulps(row[:4], w["rect"]).max() <= 4
        assert ref.ulps(row[4], w["cs"]) <= 4 and ref.ulps(row[5], w["sn"]) <= 4
        # inside the stated ranges
        l, t, r, b = row[:4]
        box = r - l
        assert 144.0 / 0.99999 - 1e-9 <= box <= 144.0 / 0.97 + 1e-9 and box < 150 and abs((b - t) - box) < 1e-9
        assert abs((l + r) / 2 - 75) <= 0.02 * 144 + 1e-9 and abs((t + b) / 2 - 75) <= 0.02 * 144 + 1e-9
        assert abs(np.degrees(np.arctan2(row[5], row[4]))) <= 3.0 + 1e-9 and abs(row[4] ** 2 + row[5] ** 2 - 1) < 1e-12
        # the chip_plan part: a box inside the 150 x 150 chip, integers
        bx0, by0, sw, sh = row[13:17]
        assert all(float(v).is_integer() for v in (bx0, by0, sw, sh))
        assert bx0 >= 0 and by0 >= 0 and sw >= 2 and sh >= 2 and bx0 + sw <= 150 and by0 + sh <= 150


def test_plan_of_a_jitter_does_not_depend_on_J():
    for seed in (0, 1, 2, 2 ** 64 - 1):
        big = _lib.jitter_plan(100, seed)
        for J in (1, 8, 13):
            assert np.array_equal(_lib.jitter_plan(J, seed), big[:J])
    assert not np.array_equal(_lib.jitter_plan(8, 0), _lib.jitter_plan(8, 1))
    assert _lib.jitter_plan(0, 0).shape == (0, _lib.JITTER_ROW)


def test_plan_refusals():
    for J in (-1, 4097):
        with pytest.raises(_lib.PvfError, match="jitters|negative"):
            _lib.jitter_plan(J, 0)
    assert _lib.jitter_plan(4096, 0).shape == (4096, _lib.JITTER_ROW)


def test_seed_0_J_8_covers_both_flips_both_signs_black_and_blended_pixels(oracle):
    rows = _lib.jitter_plan(8, 0)
    assert [int(r[6]) for r in rows] == [0, 1, 1, 1, 1, 1, 1, 0]
    assert [int(r[5] > 0) for r in rows] == [1, 0, 1, 0, 0, 1, 0, 0]
    white = np.full((150, 150, 3), 255, np.uint8)
    chips = [ref.jitter(oracle, white, ref.row_of_library(r)) for r in rows]
    black = [int((c == 0).all(axis=2).sum()) for c in chips]
    assert min(black) >= 50 and max(black) <= 782, black                 # the sampled box leaves the chip at a corner or an edge
    blended = [j for j, c in enumerate(chips) if ((c != 0) & (c != 255)).any()]
    assert blended == [1, 3, 6, 7], blended                              # 255 blended with 255 that does not come back as 255
    # the mirror is the last step: a mirrored row's chip is the unmirrored extraction read right to left
    j = 1
    plain = dict(ref.row_of_library(rows[j]), flip=False)
    assert np.array_equal(chips[j], ref.jitter(oracle, white, plain)[:, ::-1])


def test_mean32_is_the_ascending_fp32_sum():
    rng = np.random.default_rng(0)
    d = rng.standard_normal((3, 7, 128)).astype(np.float32)
    got = ref.mean32(d)
    assert got.dtype == np.float32 and got.shape == (3, 128)
    acc = np.float32(0)
    for j in range(7):
        acc = np.float32(acc + d[2, j, 5])
    assert got[2, 5] == np.float32(acc / np.float32(7))
    assert np.array_equal(ref.mean32(d[:, :1]), d[:, 0])


# ---- the verbs and the shim on scripted contexts ---------------------------------------------------------------------------------------
class _RecordingExtract(ExtractContext):
    def landmarks_embed(self, frames, boxes, num_jitters=0, seed=0):
        self.jitter = getattr(self, "jitter", []) + [(num_jitters, seed)]
        return ExtractContext.landmarks_embed(self, frames, boxes)


class _RecordingEnroll(EnrollContext):
    def landmarks_embed(self, frames, boxes, num_jitters=0, seed=0):
        self.jitter = getattr(self, "jitter", []) + [(num_jitters, seed)]
        return EnrollContext.landmarks_embed(self, frames, boxes)


def test_extract_verb_carries_the_jitter_options(tmp_path, monkeypatch):
    tp = str(tmp_path / "track.txt")
    formats.write_tracks(tp, make_tracks(60))
    monkeypatch.setattr(cli, "open_video", lambda spec, fps, **kw: ScriptVideo(60))
    files = {}
    for name, opts, want in (("plain", [], (0, 0)), ("jit", ["--jitters", "5", "--jitter-seed", "3"], (5, 3))):
        ctx = _RecordingExtract()
        monkeypatch.setattr(runtime, "default_context", lambda ctx=ctx: ctx)
        lp, ep = str(tmp_path / (name + "_l.txt")), str(tmp_path / (name + "_e.txt"))
        assert cli.main(["extract"] + opts + ["v", tp, "unused", "unused", lp, ep]) == 0
        assert ctx.jitter and set(ctx.jitter) == {want}
        files[name] = (open(lp, "rb").read(), open(ep, "rb").read())
    # the scripted descriptors ignore the jitters: the files are the same, and they are what a context without the arguments writes
    old = ExtractContext()
    lp, ep = str(tmp_path / "old_l.txt"), str(tmp_path / "old_e.txt")
    cli.extract(ScriptVideo(60), "unused", "unused", tp, lp, ep, ctx=old)
    assert files["plain"] == files["jit"] == (open(lp, "rb").read(), open(ep, "rb").read())
    with pytest.raises(ValueError, match="negative"):
        cli.extract(ScriptVideo(60), "unused", "unused", tp, lp, ep, ctx=old, num_jitters=-1)


def test_enroll_verb_carries_the_jitter_options(tmp_path, monkeypatch):
    faces = {i: [(i, 0, i + 9, 9)] for i in range(20)}
    monkeypatch.setattr(cli, "open_video", lambda spec, fps, **kw: _Frames(20))
    for name, opts, want in (("plain", [], (0, 0)), ("jit", ["--jitters", "5", "--jitter-seed", "3"], (5, 3))):
        ctx = _RecordingEnroll(faces)
        monkeypatch.setattr(runtime, "default_context", lambda ctx=ctx: ctx)
        gal = str(tmp_path / (name + ".txt"))
        assert cli.main(["enroll"] + opts + ["v", "unused", "unused", "dora", gal]) == 0
        assert len(ctx.jitter) == 2 and set(ctx.jitter) == {want}                  # two batches of 16
        assert formats.read_gallery(gal)[1].tolist() == [0, 20]
    # the Python functions take num_jitters / jitter_seed; a context whose landmarks_embed knows no jitters still serves the default
    gal = str(tmp_path / "api.txt")
    ctx = _RecordingEnroll(faces)
    cli.enroll(_Frames(20), "unused", "unused", "dora", gal, ctx=ctx, num_jitters=7, jitter_seed=11)
    assert set(ctx.jitter) == {(7, 11)}
    assert cli.enroll(_Frames(20), "unused", "unused", "dora", str(tmp_path / "old.txt"), ctx=EnrollContext(faces))["faces"] == 20


class _ShimContext(object):
    def __init__(self):
        self.calls = []

    def load_embedder(self, path):
        pass

    def embed(self, frames, pts, num_jitters=0, seed=0):
        self.calls.append((num_jitters, seed))
        return np.full((len(pts), 128), 0.25, np.float32)


def test_shim_compute_face_descriptor_takes_num_jitters():
    from pyannote_video_amd.face import Face
    ctx = _ShimContext()
    model = shim.face_recognition_model_v1("unused", ctx)
    shape = shim.full_object_detection(shim.rectangle(0, 0, 10, 10), np.zeros((68, 2), np.int32))
    rgb = np.zeros((8, 8, 3), np.uint8)
    v = model.compute_face_descriptor(rgb, shape, num_jitters=4)
    assert len(v) == 128 and v[0] == 0.25
    model.compute_face_descriptor(rgb, shape)
    model.compute_face_descriptor(rgb, shape, 1)
    assert ctx.calls == [(4, 0), (0, 0), (0, 0)]
    face = Face.__new__(Face)
    face.face_recognition_ = model
    face.get_embedding(rgb, shape, num_jitters=10)
    face.get_embedding(rgb, shape)
    assert ctx.calls[3:] == [(10, 0), (0, 0)]
