"""CPU: identification against a gallery without a device -- the decision rules of tests/identify_ref.py on hand-made matrices, the gallery
file, the refusals, and the `identify` / `enroll-track` / `enroll` verbs through cli.main on a scripted context whose device calls are
identify_ref's; plus the margins of the inputs tests/test_gpu_identify.py decides on."""
import numpy as np
import pytest

from pyannote_video_amd import cli, formats, identification, runtime
from tests import identify_ref as ref


class ScriptContext(object):
    """the device side of FaceIdentification and of `enroll`, scripted"""

    def __init__(self, faces=None):
        self.calls, self.faces, self.released = [], faces or {}, 0

    def identify(self, X, row_start, G, gal_start, threshold, metric=0, return_dist=False):
        self.calls.append((np.array(X), np.array(row_start), np.array(G), np.array(gal_start), threshold, metric))
        D = ref.mean_dist(X, row_start, G, gal_start, metric)
        out = ref.pick(D, threshold)
        return out + (D,) if return_dist else out

    # `enroll`: frame i carries its index in its first pixel; faces = {frame: [box, ...]}
    def load_shape_predictor(self, path):
        pass

    def load_embedder(self, path):
        pass

    def upload(self, rgb):
        ctx = self

        class Dev(object):
            i = int(rgb[0, 0, 0])

            def release(self):
                ctx.released += 1
        return Dev()

    def detect_batch(self, frames, upsample=1):
        assert upsample == 1
        return [(list(self.faces.get(f.i, [])), [1.0] * len(self.faces.get(f.i, []))) for f in frames]

    def landmarks_embed(self, frames, boxes):
        emb = np.array([np.float32(0.001) * (100 * f.i + b[0]) + np.float32(0.01) * np.arange(128, dtype=np.float32) for f, b in zip(frames, boxes)], np.float32)
        return np.zeros((len(boxes), 68, 2), np.int32), emb.reshape(-1, 128)


@pytest.fixture
def script(monkeypatch):
    ctx = ScriptContext()
    monkeypatch.setattr(runtime, "default_context", lambda: ctx)
    return ctx


# ---- the decision --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.HAND_MADE, ids=[c[0] for c in ref.HAND_MADE])
def test_pick_on_hand_made_matrices(case):
    _, D, threshold, *want = case
    assert ref.same_picks(ref.pick(D, threshold), ref.as_picks(*want))


def test_one_ulp_above_the_threshold_is_the_next_double():
    assert ref.ULP_ABOVE > 0.6 and np.nextafter(ref.ULP_ABOVE, 0.0) == 0.6


def test_mean_dist_is_the_plain_block_mean():
    X, rs, G, gs = ref.main_case()
    D = ref.mean_dist(X, rs, G, gs, 0)
    t, k = 7, 4
    want = np.mean([np.linalg.norm(x - g) for x in X[rs[t]:rs[t + 1]] for g in G[gs[k]:gs[k + 1]]])
    assert abs(D[t, k] - want) < 1e-14
    Dc = ref.mean_dist(np.r_[X[:2], np.zeros((1, 128))], [0, 3], G[:2], [0, 2], 1)
    cos = [1 - x @ g / np.linalg.norm(x) / np.linalg.norm(g) for x in X[:2] for g in G[:2]] + [0.0, 0.0]
    assert abs(Dc[0, 0] - np.mean(cos)) < 1e-14


def test_margins_of_the_gpu_test_inputs():
    """the end-to-end GPU test asserts best and second of EVERY group: the inputs carry the condition that no decision is a near tie"""
    X, rs, G, gs = ref.main_case()
    assert len(X) == 320 and len(G) == 201 and len(rs) == 21 and len(gs) == 18
    for metric, threshold in ((0, 0.6), (1, 0.3)):
        D = ref.mean_dist(X, rs, G, gs, metric)
        best, bd, second, sd = ref.pick(D, threshold)
        assert np.array_equal(best, ref.main_case_truth()) and (best >= 0).sum() == 15 and (best < 0).sum() == 5
        srt = np.sort(D, axis=1)
        gap12, gap23 = (srt[:, 1] - srt[:, 0]).min(), (srt[:, 2] - srt[:, 1]).min()
        edge = np.abs(D - threshold).min()
        print("metric %d: smallest runner-up gap %.3g, second-to-third gap %.3g, smallest distance from the threshold %.3g" % (metric, gap12, gap23, edge))
        assert gap12 >= 1e-6 and gap23 >= 1e-6 and edge >= 1e-6


# ---- the gallery file ----------------------------------------------------------------------------------------------------------------
def test_gallery_round_trip_groups_by_name_in_order_of_first_appearance(tmp_path):
    rng = np.random.default_rng(1)
    E = rng.standard_normal((7, 128)) * 0.1
    order = ["bob", "alice", "bob", "carol", "alice", "bob", "carol"]
    path = str(tmp_path / "gallery.txt")
    with open(path, "w") as f:
        for name, e in zip(order, E):
            f.write(formats.gallery_line(name, e))
        f.write("\n")
    names, start, G = formats.read_gallery(path)
    assert names == ["bob", "alice", "carol"] and start.tolist() == [0, 3, 5, 7] and start.dtype == np.int32
    rows = [0, 2, 5, 1, 4, 3, 6]                                                    # stable inside a name
    assert np.array_equal(G, np.array([formats.quantise_embedding(E[r]) for r in rows]))
    assert open(path).readline().split()[1:] == formats.embedding_line(0.0, 0, E[0]).split()[2:]      # the values as embedding.txt writes them
    # FaceGallery: the same grouping, float32 descriptors rounded as the clustering rounds them, save -> load unchanged
    g = identification.FaceGallery()
    for name, e in zip(order, E):
        g.add(name, e.astype(np.float32))
    n2, s2, G2 = g.arrays()
    assert n2 == names and np.array_equal(s2, start)
    assert np.array_equal(G2, np.round(E.astype(np.float32).astype(np.float64), 5)[rows])
    p2 = str(tmp_path / "g2.txt")
    g.save(p2)
    n3, s3, G3 = identification.FaceGallery.load(p2).arrays()
    assert n3 == names and np.array_equal(s3, start) and np.array_equal(G3, G2)


def test_refusals(tmp_path):
    e = np.zeros(128)
    for bad in ("", "two words", " lead", "tab\tbed", "line\n", None, 3):
        with pytest.raises(ValueError, match="one token"):
            formats.gallery_line(bad, e)
        with pytest.raises(ValueError, match="one token"):
            identification.FaceGallery().add(bad, e)
    with pytest.raises(ValueError, match="128 values"):
        formats.gallery_line("a", e[:127])
    ragged = str(tmp_path / "ragged.txt")
    with open(ragged, "w") as f:
        f.write(formats.gallery_line("a", e))
        f.write("b " + " ".join(["0.00000"] * 127) + "\n")
    with pytest.raises(ValueError, match="ragged.txt:2: expected a name and 128 values"):
        formats.read_gallery(ragged)
    with open(ragged, "w") as f:
        f.write("a " + " ".join(["0.00000"] * 127) + " x\n")
    with pytest.raises(ValueError, match="not a number"):
        formats.read_gallery(ragged)
    # an existing file without --append
    path = str(tmp_path / "gallery.txt")
    g = identification.FaceGallery().add("a", e)
    g.save(path)
    before = open(path).read()
    with pytest.raises(FileExistsError, match="--append"):
        g.save(path)
    assert open(path).read() == before
    g.save(path, append=True)
    assert open(path).read() == before * 2
    with pytest.raises(ValueError, match="empty"):
        identification.FaceIdentification(identification.FaceGallery())
    with pytest.raises(ValueError, match="metric"):
        identification.FaceIdentification(g, metric="manhattan")


# ---- the verbs on a scripted context ---------------------------------------------------------------------------------------------------
def _clip(tmp_path):
    """five tracks around three people (track 3: nobody enrolled; track 9: a single row), rows interleaved in time as `extract` writes
    them; a gallery of alice and bob with carol's rows absent -> (embedding path, gallery path, {track: person})"""
    rng = np.random.default_rng(3)
    centre = {p: 0.7 * rng.standard_normal(128) / np.sqrt(128) for p in ("alice", "bob", "carol")}
    who = {0: "alice", 1: "bob", 3: "carol", 4: "alice", 9: "bob"}
    n_rows = {0: 5, 1: 17, 3: 4, 4: 20, 9: 1}
    rows = [(0.04 * i, t) for t in who for i in range(n_rows[t])]
    rows.sort()
    emb = str(tmp_path / "embedding.txt")
    with open(emb, "w") as f:
        for t_, trk in rows:
            f.write(formats.embedding_line(t_, trk, centre[who[trk]] + 0.15 / np.sqrt(128) * rng.standard_normal(128)))
    gal = str(tmp_path / "gallery.txt")
    with open(gal, "w") as f:
        for name, n in (("bob", 3), ("alice", 18)):
            for _ in range(n):
                f.write(formats.gallery_line(name, centre[name] + 0.15 / np.sqrt(128) * rng.standard_normal(128)))
    return emb, gal, who


def _lines(path):
    return [l.split() for l in open(path).read().splitlines()]


def test_identify_verb_per_track(tmp_path, script):
    emb, gal, who = _clip(tmp_path)
    out, sc = str(tmp_path / "names.txt"), str(tmp_path / "scores.txt")
    assert cli.main(["identify", "--scores", sc, emb, gal, out]) == 0
    assert _lines(out) == [["0", "alice"], ["1", "bob"], ["4", "alice"], ["9", "bob"]]          # track 3 matches nobody: left out
    # what the device was given: rows sorted by (track, time), one group per track, the gallery grouped by name in file order
    X, rs, G, gs, threshold, metric = script.calls[0]
    time, track, Xf = formats.read_embeddings(emb)
    order = np.lexsort((time, track))
    assert np.array_equal(X, Xf[order]) and rs.tolist() == [0, 5, 22, 26, 46, 47] and gs.tolist() == [0, 3, 21] and (threshold, metric) == (0.6, 0)
    D = ref.mean_dist(X, rs, G, gs, 0)
    rows = _lines(sc)
    assert [r[0] for r in rows] == ["0", "1", "3", "4", "9"]
    for r, d in zip(rows, D):
        k = int(np.argmin(d))
        assert r[1] == ["bob", "alice"][k] and r[3] == ["bob", "alice"][1 - k]                  # the nearest identity even above the threshold
        assert r[2] == "%.6f" % d[k] and r[4] == "%.6f" % d[1 - k]
    assert D[2].min() > 0.6 and rows[2][1] in ("alice", "bob")
    # --unknown names the rest; --threshold and --metric reach the device
    assert cli.main(["identify", "--unknown", "somebody", "--threshold", "0.3", "--metric", "cosine", emb, gal, out]) == 0
    assert _lines(out) == [["0", "alice"], ["1", "bob"], ["3", "somebody"], ["4", "alice"], ["9", "bob"]]
    assert script.calls[1][4:] == (0.3, 1)
    # the API form: the same decision
    got = identification.FaceIdentification(gal, ctx=script).identify(emb)
    assert {t: v[0] for t, v in got.items()} == {0: "alice", 1: "bob", 3: None, 4: "alice", 9: "bob"}
    assert all(v[2] in ("alice", "bob") for v in got.values())


def test_identify_verb_per_cluster(tmp_path, script):
    emb, gal, who = _clip(tmp_path)
    lab = str(tmp_path / "labels.txt")
    with open(lab, "w") as f:
        f.write("0 0\n1 1\n3 3\n4 0\n9 9\n")                                            # what `cluster` writes: tracks 0 and 4 are one cluster
    out, sc = str(tmp_path / "names.txt"), str(tmp_path / "scores.txt")
    assert cli.main(["identify", "--labels", lab, "--scores", sc, emb, gal, out]) == 0
    assert _lines(out) == [["0", "alice"], ["1", "bob"], ["3", "3"], ["4", "alice"], ["9", "bob"]]      # a complete replacement
    X, rs, G, gs, _, _ = script.calls[0]
    time, track, Xf = formats.read_embeddings(emb)
    group = np.where(track == 4, 0, track)
    assert np.array_equal(X, Xf[np.lexsort((time, track, group))]) and rs.tolist() == [0, 25, 42, 46, 47]      # (group, track, time)
    assert [r[0] for r in _lines(sc)] == ["0", "1", "3", "9"]
    assert cli.main(["identify", "--labels", lab, "--unknown", "nobody", emb, gal, out]) == 0
    assert _lines(out)[2] == ["3", "nobody"]
    # labels that are names already, and a track the map does not mention (its own group)
    got = identification.FaceIdentification(gal, ctx=script).identify(emb, labels={0: "x", 4: "x", 1: 7})
    assert {g: v[0] for g, v in got.items()} == {3: None, 7: "bob", 9: "bob", "x": "alice"}
    assert list(got) == [3, 7, 9, "x"]                                                  # numbers first, in order, then text
    from pyannote_video_amd import render
    assert render.read_labels(out) == {0: "alice", 1: "bob", 3: "nobody", 4: "alice", 9: "bob"}      # the file `demo --label` reads


def test_identify_arrays_rounds_float32_descriptors_like_the_clustering(script):
    rng = np.random.default_rng(5)
    E = (rng.standard_normal(128) * 0.1 + rng.standard_normal((6, 128)) * 0.01).astype(np.float32)          # one person
    g = identification.FaceGallery().add("a", E[:2])
    got = identification.FaceIdentification(g, ctx=script).identify_arrays([2, 2, 1, 1, 1, 2], E)
    X, rs, G, gs, _, _ = script.calls[0]
    want = np.round(E.astype(np.float64), 5)
    assert np.array_equal(X, want[[2, 3, 4, 0, 1, 5]]) and rs.tolist() == [0, 3, 6] and np.array_equal(G, want[:2])
    assert sorted(got) == [1, 2] and got[2][0] == "a" and got[2][2] is None and got[2][3] == np.inf      # K = 1: no runner-up


def test_enroll_track_verb(tmp_path, script):
    emb, gal, who = _clip(tmp_path)
    new = str(tmp_path / "new.txt")
    assert cli.main(["enroll-track", emb, "3", "carol", new]) == 0
    names, start, G = formats.read_gallery(new)
    time, track, X = formats.read_embeddings(emb)
    assert names == ["carol"] and start.tolist() == [0, 4] and np.array_equal(G, X[track == 3])
    with pytest.raises(FileExistsError):
        cli.main(["enroll-track", emb, "1", "bob", new])
    assert cli.main(["enroll-track", "--append", emb, "1", "bob", new]) == 0
    assert formats.read_gallery(new)[0] == ["carol", "bob"] and formats.read_gallery(new)[1].tolist() == [0, 4, 21]
    with pytest.raises(ValueError, match="no row of track 5"):
        cli.main(["enroll-track", "--append", emb, "5", "eve", new])
    with pytest.raises(ValueError, match="one token"):
        cli.main(["enroll-track", "--append", emb, "1", "bob b", new])
    # enrolled from the video itself, track 3 is now known
    out = str(tmp_path / "names.txt")
    assert cli.main(["identify", emb, new, out]) == 0
    assert ["3", "carol"] in _lines(out)


class _Frames(object):
    frame_rate, size, frame_size = 25.0, (8, 8), (8, 8)

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __iter__(self):
        for i in range(self.n):
            a = np.zeros((8, 8, 3), np.uint8)
            a[0, 0, 0] = i
            yield i / 25.0, a


def test_enroll_takes_the_largest_face_of_every_frame(tmp_path):
    faces = {0: [(10, 10, 20, 20), (30, 30, 50, 50)],            # the second is larger
             2: [(1, 1, 11, 11), (2, 2, 12, 12)],                # equal areas: the first in detector order
             3: [(5, 5, 6, 6)]}
    faces.update({i: [(i, 0, i + 9, 9)] for i in range(4, 37)})   # more than two batches
    ctx = ScriptContext(faces)
    gal = str(tmp_path / "gallery.txt")
    res = cli.enroll(_Frames(38), "unused", "unused", "dora", gal, ctx=ctx)
    assert res == {"faces": 36, "skipped": 2} and ctx.released == 38             # frames 1 and 37 carry no face
    names, start, G = formats.read_gallery(gal)
    boxes = [faces[0][1], faces[2][0], faces[3][0]] + [faces[i][0] for i in range(4, 37)]
    frames = [type("F", (), {"i": i}) for i in [0, 2, 3] + list(range(4, 37))]
    assert names == ["dora"] and np.array_equal(G, np.round(ctx.landmarks_embed(frames, boxes)[1].astype(np.float64), 5))
    with pytest.raises(FileExistsError):
        cli.enroll(_Frames(3), "unused", "unused", "dora", gal, ctx=ctx)
    res = cli.enroll(_Frames(3), "unused", "unused", "erin", gal, append=True, ctx=ctx)
    assert res == {"faces": 2, "skipped": 1} and formats.read_gallery(gal)[1].tolist() == [0, 36, 38]
    with pytest.raises(ValueError, match="no face was found"):
        cli.enroll(_Frames(2), "unused", "unused", "fay", str(tmp_path / "none.txt"), ctx=ScriptContext({}))
    assert not (tmp_path / "none.txt").exists()


def test_process_needs_labels_for_a_gallery(tmp_path):
    with pytest.raises(ValueError, match="needs --labels"):
        cli.process(_Frames(2), [], "unused", "unused", "t", "l", "e", None, gallery="g", ctx=ScriptContext())
