"""CPU: the rules of SEARCH.md without a device -- the numpy restatement (tests/search_ref.py) on cases whose answer is found by
inspection, the quantisation round trip, planted defects that the comparison must see, the host merge of a multi-row query, the margins
of the inputs tests/test_gpu_search.py runs, and the `search` verb through cli.main on a scripted context whose device call is the
restatement."""
import numpy as np
import pytest

from pyannote_video_amd import cli, formats, identification, runtime
from pyannote_video_amd import search as face_search
from tests import search_cases as cases
from tests import search_ref as ref


# ---- by inspection ---------------------------------------------------------------------------------------------------------------------
def test_rows_of_one_non_zero_component():
    X = np.zeros((4, 128))
    X[0, 3], X[1, 3], X[2, 90], X[3, 3] = 0.00003, -0.00004, 0.00005, 0.00003
    q = np.zeros((1, 128))
    idx, d2, count = ref.search(q, X, 4)
    assert list(idx[0]) == [0, 3, 1, 2] and list(d2[0]) == [9, 9, 16, 25] and count[0] == 4
    idx, d2, _ = ref.search(X[:1], X, 4)                          # (3 - -4)^2 = 49; 3^2 + 5^2 = 34
    assert list(idx[0]) == [0, 3, 2, 1] and list(d2[0]) == [0, 0, 34, 49]


def test_a_row_against_itself_and_the_extreme():
    X = cases.blobs(1, 5)
    assert list(ref.search(X, X, 1)[1][:, 0]) == [0] * 5
    Qr, T = cases.extreme()
    assert (ref.search(Qr, T, 3)[1] == 1 << 49).all() and 128 * (1 << 21) ** 2 == 1 << 49
    assert ref.d2_matrix(Qr, T).dtype == np.int64


def test_quantisation_round_trip_of_the_five_decimal_text():
    """for every integer n (a sample of |n| <= 2^20 and the ends): the double the text n / 10^5 parses to gives rint(v * 100000.0) == n"""
    rng = np.random.default_rng(0)
    n = np.concatenate([rng.integers(-(1 << 20), (1 << 20) + 1, 20000), [-(1 << 20), (1 << 20), 0, 1, -1, 50000, 99999]])
    v = np.array([float("%d.%05d" % divmod(abs(int(i)), 100000)) * (1 if i >= 0 else -1) for i in n])
    assert np.array_equal(ref.quantise(v[None])[0], n)
    assert np.array_equal(np.array([float("{x:.5f}".format(x=float(x))) for x in v]), v)      # and the text of that double is the same text


def test_quantisation_round_trip_of_float32_descriptors():
    e = (np.random.default_rng(1).standard_normal((50, 128)) / np.sqrt(128.0)).astype(np.float32)
    rounded = np.round(e.astype(np.float64), 5)
    text = np.array([formats.quantise_embedding(r) for r in e])
    assert np.array_equal(rounded, text)
    q = ref.quantise(rounded)
    assert np.array_equal(q, np.rint(e.astype(np.float64) * 1e5).astype(np.int64)) and np.array_equal(q / 1e5, rounded)


def test_refusals_of_the_restatement():
    X = cases.blobs(2, 20)
    for bad in (10.48577, -10.48577, np.nan, np.inf):
        Y = X.copy()
        Y[7, 5] = bad
        Y[9, 0] = bad
        with pytest.raises(ref.Refused, match=r"X\[7\]\[5\]"):
            ref.search(X[:2], Y, 3)
        with pytest.raises(ref.Refused, match=r"Qrows\[7\]\[5\]"):
            ref.search(Y, X, 3)
    Y = X.copy()
    Y[0, 0] = 10.48576                                            # 2^20 units: the last value taken
    assert ref.quantise(Y)[0, 0] == 1 << 20
    for kw, what in ((dict(k=0), "k"), (dict(k=1025), "k"), (dict(k=3, max_d2=-2), "max_d2"), (dict(k=3, row_group=np.zeros(20, np.int32)), "groups")):
        with pytest.raises(ref.Refused, match=what):
            ref.search(X[:2], X, **kw)
    with pytest.raises(ref.Refused):
        ref.search(X[:0], X, 3)
    with pytest.raises(ref.Refused):
        ref.search(X[:2, :64], X[:, :64], 3)


# ---- planted defects: each one is seen by the comparison on the inputs the GPU test runs ----------------------------------------------
def _defective(defect, Qr, X, k, max_d2=-1, query_group=None, row_group=None):
    D = ref.d2_matrix(Qr, X)
    if defect == "float32 accumulation":
        qa, qb = ref.quantise(Qr).astype(np.float32), ref.quantise(X).astype(np.float32)
        D = np.array([((qb - a) ** 2).sum(1, dtype=np.float32) for a in qa]).astype(np.int64)
    kk = k - 1 if defect == "k off by one" else k
    fill = 0 if defect == "tail of 0" else -1
    idx, d2, count = np.full((len(D), k), fill, np.int32), np.full((len(D), k), fill, np.int64), np.zeros(len(D), np.int32)
    for q in range(len(D)):
        keep = np.ones(D.shape[1], bool)
        if query_group is not None and defect != "exclusion ignored":
            if query_group[q] >= 0 or defect == "exclusion of group -1":
                keep &= np.asarray(row_group) != query_group[q]
        if max_d2 >= 0:
            keep &= (D[q] < max_d2) if defect == "cut as <" else (D[q] <= max_d2)
        i = np.arange(D.shape[1])[keep]
        order = np.lexsort((-i if defect == "ties to the higher index" else i, D[q][i]))[:kk]
        idx[q, :len(order)], d2[q, :len(order)], count[q] = i[order], D[q][i][order], len(order)
    return idx, d2, count


def _differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


def test_planted_defects_are_seen():
    X = cases.ties(9, 3000)
    zero = np.zeros((1, 128))
    table = cases.blobs(1, 600)
    rg = cases.groups_across_seams(600)
    qrows = np.array([0, 15, 16, 17, 207, 208, 209, 300, 415, 416, 599])
    qg = rg[qrows].copy()
    qg[::2] = -1
    kth = int(ref.search(table[:6], table, 30)[1][:, 29].min())
    wide = cases.blobs(8, 2500) * 30.0                            # d2 far above 2^24: float32 sums round
    seen = {
        "no defect": _differs(_defective(None, zero, X, 100), ref.search(zero, X, 100)),
        "ties to the higher index": _differs(_defective("ties to the higher index", zero, X, 100), ref.search(zero, X, 100)),
        "k off by one": _differs(_defective("k off by one", zero, X, 100), ref.search(zero, X, 100)),
        "cut as <": _differs(_defective("cut as <", table[:6], table, 30, max_d2=kth), ref.search(table[:6], table, 30, max_d2=kth)),
        "exclusion ignored": _differs(_defective("exclusion ignored", table[qrows], table, 20, query_group=qg, row_group=rg),
                                      ref.search(table[qrows], table, 20, query_group=qg, row_group=rg)),
        "exclusion of group -1": _differs(_defective("exclusion of group -1", table[qrows], table, 20, query_group=qg, row_group=rg),
                                          ref.search(table[qrows], table, 20, query_group=qg, row_group=rg)),
        "float32 accumulation": _differs(_defective("float32 accumulation", np.round(wide[:2], 5), np.round(wide, 5), 1024),
                                         ref.search(np.round(wide[:2], 5), np.round(wide, 5), 1024)),
        "tail of 0": _differs(_defective("tail of 0", table[:3], table[:300], 301), ref.search(table[:3], table[:300], 301)),
    }
    assert seen.pop("no defect") is False
    assert all(seen.values()), seen


def test_a_merge_that_keeps_duplicates_is_seen():
    files = cases.two_files()
    X = np.concatenate([f[2] for f in files])
    Qr = files[0][2][files[0][1] == 0]
    idx, d2, count = ref.search(Qr, X, 12)
    good = ref.merge_min(idx, d2, count, 12)
    dup = sorted((int(d2[q, j]), int(idx[q, j])) for q in range(len(count)) for j in range(count[q]))[:12]
    assert len(set(i for _, i in good)) == 12 and len(set(i for _, i in dup)) < 12 and good != dup


# ---- the host merge ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 12, 40, 100])
def test_merge_by_the_minimum_equals_brute_force(k):
    files = cases.two_files()
    X = np.concatenate([f[2] for f in files])
    for Qr in (files[0][2][files[0][1] == 0], files[1][2][files[1][1] == 5], X[:1]):
        idx, d2, count = ref.search(Qr, X, k)
        want = ref.merge_brute(Qr, X, k)
        assert ref.merge_min(idx, d2, count, k) == want
        assert face_search.merge_min(idx, d2, count, k) == want


def test_max_distance_becomes_an_integer_cut():
    assert face_search.max_d2_of(None) == -1 and face_search.max_d2_of(0.6) == 60000 ** 2 and face_search.max_d2_of(0) == 0
    assert face_search.max_d2_of(0.123456) == 12346 ** 2
    with pytest.raises(ValueError):
        face_search.max_d2_of(-0.1)


# ---- margins of the GPU inputs ----------------------------------------------------------------------------------------------------------
def test_margins_of_the_gpu_test_inputs():
    zero = np.zeros((1, 128))
    # ties at the k-th place: the k-th and the (k + 1)-th hit share their d2
    X = cases.ties(9, 3000)
    D = np.sort(ref.d2_matrix(zero, X)[0])
    assert D[99] == D[100] and len(np.unique(D)) < 40
    D = ref.d2_matrix(X[:17], X)
    assert all(np.sort(r)[49] == np.sort(r)[50] for r in D)
    assert (ref.d2_matrix(cases.identical(700)[:2], cases.identical(700)) == 0).all()
    # order of arrival: descending, every row passes -- at least two compactions in every range; ascending, only the first k pass
    p = ref.plan(1, 2000, 100)
    assert p["n_ranges"] == 8 and p["range_blocks"] == 16 and p["pending"] == 128
    rows = p["range_blocks"] * 16
    for order, least, most in (("descending", 2, 99), ("ascending", 0, 1), ("shuffled", 1, 99)):
        d = ref.d2_matrix(zero, cases.ladder(2000, order))[0]
        n = [ref.compactions(d, 100, r0, min(r0 + rows, 2000), p["pending"]) for r0 in range(0, 2000, rows)]
        assert least <= min(n) and max(n) <= most, (order, n)
    # the seams
    assert ref.plan(20, 600, 10) == dict(chunk_rows=608, n_chunks=1, n_ranges=3, range_blocks=13, pending=64, arena_bytes=32 * 3 * 128 * 12)
    assert [ref.plan(21, 600, 70, c)["n_chunks"] for c in (16, 100, 257)] == [38, 6, 3]
    rg = cases.groups_across_seams(600)
    assert (rg == -1).any() and any(rg[b - 1] == rg[b] >= 0 for b in (16, 208, 416))      # a group across a block seam and both range seams
    # exact values
    Qr, T = cases.extreme()
    assert ref.quantise(Qr).max() == 1 << 20 and ref.quantise(T).min() == -(1 << 20)
    edge = (1 << 20) * 1e-5
    for v in (edge + 1e-5, -edge - 1e-5):
        with pytest.raises(ref.Refused):
            ref.quantise(np.full((1, 128), v))
    # the cut: at the k-th d2 the k-th hit is kept, one below it is not
    table = cases.blobs(1, 600)
    _, d2, _ = ref.search(table[:6], table, 30)
    kth = int(d2[:, 29].min())
    assert ref.search(table[:6], table, 30, max_d2=kth)[2].max() == 30 and ref.search(table[:6], table, 30, max_d2=kth - 1)[2].max() == 29


# ---- the verb on a scripted context -----------------------------------------------------------------------------------------------------
class ScriptContext(object):
    """the device side of FaceSearch, scripted: the restatement"""

    def __init__(self):
        self.calls = []

    def search(self, Qrows, X, k, max_d2=-1, query_group=None, row_group=None):
        self.calls.append(dict(Q=len(Qrows), N=len(X), k=k, max_d2=max_d2, query_group=query_group, row_group=row_group))
        return ref.search(Qrows, X, k, max_d2=max_d2, query_group=query_group, row_group=row_group)


@pytest.fixture
def script(monkeypatch):
    ctx = ScriptContext()
    monkeypatch.setattr(runtime, "default_context", lambda: ctx)
    return ctx


@pytest.fixture
def clip(tmp_path):
    files = cases.two_files()
    paths = [str(tmp_path / n) for n in ("a.txt", "b.txt")]
    for p, (t, track, X) in zip(paths, files):
        with open(p, "w") as f:
            for i in range(len(t)):
                f.write(formats.embedding_line(t[i], int(track[i]), X[i]))
    X = np.concatenate([f[2] for f in files])
    owner = [(p, int(k)) for p, f in zip(paths, files) for k in f[1]]
    times = np.concatenate([f[0] for f in files])
    gal = str(tmp_path / "gallery.txt")
    identification.FaceGallery().add("ann", files[1][2][files[1][1] == 5]).add("bob", files[0][2][:2]).save(gal)
    return paths, files, X, owner, times, gal


def _want(hits, owner, times):
    return "".join(ref.line(r, d, owner[i][0], owner[i][1], times[i]) for r, (d, i) in enumerate(hits))


def test_search_verb_from_a_track(tmp_path, script, clip, capsys):
    paths, files, X, owner, times, _ = clip
    out = str(tmp_path / "hits.txt")
    Qr = files[0][2][files[0][1] == 0]
    skip = [o == (paths[0], 0) for o in owner]
    assert cli.main(["search", "-k", "12", "--rows", "--from", paths[0], "--track", "0", out] + paths) == 0
    hits = ref.merge_brute(Qr, X, 12, skip=skip)
    assert open(out).read() == _want(hits, owner, times) and len(hits) == 12
    assert script.calls[-1]["Q"] == 7 and script.calls[-1]["N"] == len(X) and (script.calls[-1]["query_group"] == 0).all()
    # collapsed (the default): the tracks that own those faces, nearest first -- the same person's other tracks in both files lead
    assert cli.main(["search", "-k", "12", "--from", paths[0], "--track", "0", out] + paths) == 0
    lines = open(out).read()
    assert lines == _want(ref.collapse(hits, owner), owner, times)
    first = [l.split()[2:4] for l in lines.splitlines()][:2]
    assert sorted(first) == sorted([[paths[0], "2"], [paths[1], "5"]]) and len(lines.splitlines()) < 12
    # the own track is found with --include-self, and when its file is not among the searched ones nothing is excluded
    assert cli.main(["search", "-k", "12", "--rows", "--include-self", "--from", paths[0], "--track", "0", out] + paths) == 0
    assert open(out).read() == _want(ref.merge_brute(Qr, X, 12), owner, times) and script.calls[-1]["query_group"] is None
    assert cli.main(["search", "-k", "5", "--rows", "--from", paths[0], "--track", "0", "-", paths[1]]) == 0
    n0 = len(files[0][0])
    hits = ref.merge_brute(Qr, files[1][2], 5)
    assert capsys.readouterr().out == _want(hits, owner[n0:], times[n0:]) and script.calls[-1]["query_group"] is None


def test_search_verb_from_a_gallery_with_a_cut(tmp_path, script, clip):
    paths, files, X, owner, times, gal = clip
    out = str(tmp_path / "hits.txt")
    Qr = files[1][2][files[1][1] == 5]
    assert cli.main(["search", "-k", "100", "--rows", "--max-distance", "0.3", "--gallery", gal, "--name", "ann", out] + paths) == 0
    hits = ref.merge_brute(Qr, X, 100, max_d2=30000 ** 2)
    assert open(out).read() == _want(hits, owner, times) and 8 <= len(hits) < len(X)
    assert script.calls[-1]["max_d2"] == 30000 ** 2 and script.calls[-1]["query_group"] is None


def test_an_array_query_rounds_float32_like_the_clustering(script, clip):
    paths, files, X, owner, times, _ = clip
    e = files[0][2][:3].astype(np.float32) + np.float32(3e-6)
    fs = face_search.FaceSearch().add(paths[0]).add(paths[1]).add(paths[0])
    assert len(fs) == len(X) and fs.paths == paths
    got = fs.search(fs.rows_of_array(e), k=6, collapse=False)
    want = ref.merge_brute(np.round(e.astype(np.float64), 5), X, 6)
    assert [(h.d2, h.row) for h in got] == want and got[0].path == paths[0] and abs(got[0].distance - np.sqrt(want[0][0]) / 1e5) < 1e-15


def test_search_verb_refusals(tmp_path, script, clip, capsys):
    paths, _, _, _, _, gal = clip
    out = str(tmp_path / "hits.txt")
    empty = str(tmp_path / "empty.txt")
    open(empty, "w").close()

    def refused(argv, message):
        with pytest.raises(SystemExit):
            cli.main(["search"] + argv)
        assert message in capsys.readouterr().err, message
    refused(["--from", paths[0], "--track", "9", out] + paths, "has no row of track 9")
    refused(["--gallery", gal, "--name", "zoe", out] + paths, "the gallery has no 'zoe'")
    refused(["--from", paths[0], "--track", "0", out, empty], "the table is empty")
    refused(["-k", "0", "--from", paths[0], "--track", "0", out] + paths, "k must lie in 1 .. 1024")
    refused(["-k", "1025", "--from", paths[0], "--track", "0", out] + paths, "k must lie in 1 .. 1024")
    refused([out] + paths, "the query is")
    refused(["--gallery", gal, "--name", "ann", "--from", paths[0], "--track", "0", out] + paths, "the query is")
    assert script.calls == []
