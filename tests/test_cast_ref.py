"""CPU: the rules of CAST.md without a device -- the restatement (tests/cast_ref.py) on cases worked out by hand, its lists against
tests/search_ref.py, the paths and the planted identities tests/test_gpu_cast.py runs, planted defects that the comparison must see,
the mean rule of the track nodes, the `cast` verb through cli.main on a scripted context whose device call is the restatement, and the
compiler's resource report for the kernels of csrc/cast.hip."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from pyannote_video_amd import cast as face_cast
from pyannote_video_amd import cli, formats, runtime
from tests import cast_cases as cases
from tests import cast_ref as ref
from tests import search_cases, search_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402


def line_points(*units):
    X = np.zeros((len(units), 128))
    X[:, 0] = np.round(np.array(units) * cases.UNIT, 5)
    return X


# ---- by hand ---------------------------------------------------------------------------------------------------------------------------
def test_one_row():
    X = search_cases.blobs(1, 1)
    idx, d2, count = ref.lists(X, 3)
    assert list(count) == [0] and (idx == -1).all() and (d2 == -1).all()
    lab, n = ref.cast(X, 3)
    assert list(lab) == [0] and n == 1 and lab.dtype == np.int32


def test_two_identical_rows():
    X = search_cases.identical(2)
    idx, d2, count = ref.lists(X, 3)
    assert idx.tolist() == [[1, -1, -1], [0, -1, -1]] and d2.tolist() == [[0, -1, -1], [0, -1, -1]] and list(count) == [1, 1]
    m, r, linked = ref.links(idx, count, 0, 1)
    assert m.tolist() == [[0, -1, -1], [0, -1, -1]] and r.tolist() == [[1, -1, -1], [1, -1, -1]] and linked.tolist() == [[1, 0, 0], [1, 0, 0]]
    assert ref.cast(X, 3, num=0, den=1)[0].tolist() == [0, 0]


def test_a_one_sided_neighbour():
    """rows at 0, 10 and 13 units, k = 1: L_0 = [1], L_1 = [2], L_2 = [1] -- 1 is in L_0 but 0 is not in L_1.
    pair (0, 1): miss(0 -> 1): p = O_0(1) = 1, L_0[0:1] = {1} less 1 itself: 0.  miss(1 -> 0): 0 is not in L_1, p = c_1 = 1, L_1[0:1] = {2},
    2 is not in L_0: 1.  m = 1, r = O_0(1) = 1 (O_1(0) does not exist): linked when den <= num.
    pairs (1, 2) and (2, 1): both misses 0, r = 1: linked at every threshold."""
    X = line_points(0, 10, 13)
    idx, d2, count = ref.lists(X, 1)
    assert idx.tolist() == [[1], [2], [1]] and d2.tolist() == [[100], [9], [9]] and list(count) == [1, 1, 1]
    m, r, linked = ref.links(idx, count, 1, 1)
    assert m.tolist() == [[1], [0], [0]] and r.tolist() == [[1], [1], [1]] and linked.tolist() == [[1], [1], [1]]
    assert ref.links(idx, count, 999, 1000)[2].tolist() == [[0], [1], [1]]
    assert ref.cast(X, 1, num=1, den=1) [0].tolist() == [0, 0, 0] and ref.cast(X, 1, num=0, den=1)[0].tolist() == [0, 1, 1]


def test_a_list_that_is_empty_under_the_cut():
    X = line_points(0, 10, 1000)
    idx, d2, count = ref.lists(X, 2, max_d2=225)
    assert idx.tolist() == [[1, -1], [0, -1], [-1, -1]] and list(count) == [1, 1, 0]
    assert ref.links(idx, count, 2000, 1000)[2].tolist() == [[1, 0], [1, 0], [0, 0]]
    lab, n = ref.cast(X, 2, max_d2=225)
    assert lab.tolist() == [0, 0, 2] and n == 2
    assert ref.lists(X, 2, max_d2=100)[2].tolist() == [1, 1, 0] and ref.lists(X, 2, max_d2=99)[2].tolist() == [0, 0, 0]       # d2 <= max_d2


def test_num_zero_links_only_pairs_that_miss_nothing():
    X = search_cases.blobs(3, 80)
    idx, _, count = ref.lists(X, 6)
    m, r, linked = ref.links(idx, count, 0, 1)
    inside = np.arange(6)[None, :] < count[:, None]
    assert np.array_equal(linked.astype(bool), inside & (m == 0)) and (m[inside] > 0).any() and (m[inside] == 0).any()


def test_the_link_rule_is_symmetric():
    X = search_cases.blobs(4, 120)
    idx, _, count = ref.lists(X, 9, max_d2=cases.DEFAULT_MAX_D2)
    m, r, linked = ref.links(idx, count, 2000, 1000)
    both = 0
    for a in range(120):
        for s in range(count[a]):
            b = idx[a, s]
            back = np.nonzero(idx[b, :count[b]] == a)[0]
            if len(back):
                both += 1
                assert (m[a, s], r[a, s], linked[a, s]) == (m[b, back[0]], r[b, back[0]], linked[b, back[0]])
    assert both > 100


# ---- the lists against search_ref ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blobs", "ties", "identical", "ladder", "extreme"])
def test_lists_equal_search_ref_row_by_row(name):
    if name == "extreme":
        a, b = search_cases.extreme()
        X = np.concatenate([a, b, search_cases.blobs(5, 20)])
    else:
        X = {"blobs": lambda: search_cases.blobs(5, 90), "ties": lambda: search_cases.ties(6, 90), "identical": lambda: search_cases.identical(40),
             "ladder": lambda: search_cases.ladder(90, "shuffled")}[name]()
    N = len(X)
    assert np.array_equal(ref.d2_matrix(X), search_ref.d2_matrix(X, X))
    group = cases.groups_in_runs(N)
    for g, cut, k in ((None, -1, 7), (group, -1, 7), (group, int(np.median(ref.d2_matrix(X))), 100)):
        idx, d2, count = ref.lists(X, k, cut, g)
        for a in range(N):                                           # plain groups: every row its own, or its group's, on both sides
            eff = np.arange(N, dtype=np.int32) + N if g is None else np.where(g >= 0, g, np.arange(N) + N).astype(np.int32)
            w = search_ref.search(X[a:a + 1], X, k, max_d2=cut, query_group=eff[a:a + 1], row_group=eff)
            assert np.array_equal(idx[a], w[0][0]) and np.array_equal(d2[a], w[1][0]) and count[a] == w[2][0], (name, a)


# ---- paths and planted identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", cases.PATHS)
def test_a_path_is_one_component_of_diameter_n_less_one(n, k):
    X = cases.path(n)
    idx, _, count = ref.lists(X, k)
    lab, comps = ref.cast(X, k, num=1, den=1)
    assert comps == 1 and (lab == 0).all()
    # no list reaches further than k rows along the line, so the graph's diameter grows with n: a label that moved one link a round
    # would need n / k rounds.  In rows the path is n - 1 long.
    reach = np.abs(idx - np.arange(n)[:, None])
    assert reach.max() == k and reach[k:-k].max() == k // 2 and (count == k).all()          # k rows at the two ends, k / 2 inside
    assert int(np.abs(np.diff(np.round(X[:, 0] / (100 * cases.UNIT)))).sum()) == n - 1
    across = cases.links_across(idx, count)                               # breadth first from row 0 to the far end, over every list entry
    assert cases.path_links_across(n, k) <= across <= (n - 1) // (k // 2) and across >= n // k


@pytest.mark.parametrize("n,identities,k", cases.PLANTED)
def test_planted_identities_come_back_pure_and_complete(n, identities, k):
    X, who = cases.planted(1, n, identities)
    lab, comps = ref.cast(X, k, max_d2=cases.DEFAULT_MAX_D2, num=2000, den=1000)
    assert comps == identities and cases.pure_and_complete(lab, who)
    assert not cases.pure_and_complete(np.zeros(n, np.int32), who)


# ---- planted defects ---------------------------------------------------------------------------------------------------------------------
def _defective(defect, X, k, max_d2=-1, num=2000, den=1000, group=None):
    """the rules with one of them broken -> (idx, count, m, r, linked, labels)"""
    N = len(X)
    D = ref.d2_matrix(X)
    L = []
    for a in range(N):
        rows = [i for i in range(N) if (i != a or defect == "self kept") and (max_d2 < 0 or D[a, i] <= max_d2)
                and not (defect != "group row kept" and group is not None and i != a and group[i] >= 0 and group[i] == group[a])]
        sign = -1 if defect == "tie to the higher index" else 1
        L.append(sorted(rows, key=lambda i: (D[a, i], sign * i))[:k])
    idx, count = np.full((N, k), -1, np.int32), np.array([len(l) for l in L], np.int32)
    for a in range(N):
        idx[a, :len(L[a])] = L[a]

    def miss(x, y):
        p = L[x].index(y) + 1 if y in L[x] else len(L[x])
        return len([z for z in L[x][:p] if (z != y or defect == "z != y dropped") and z not in L[y]])
    m, r, linked = np.full((N, k), -1, np.int32), np.full((N, k), -1, np.int32), np.zeros((N, k), np.uint8)
    for a in range(N):
        for s, b in enumerate(L[a]):
            ranks = [s + 1] + ([L[b].index(a) + 1] if a in L[b] else [])
            mm, rr = miss(a, b) + miss(b, a), (max if defect == "r as the maximum" else min)(ranks)
            m[a, s], r[a, s] = mm, rr
            linked[a, s] = int(mm * den < num * rr) if defect == "< for <=" else int(mm * den <= num * rr)
    lab, _ = ref.labels(idx, linked, None if defect == "group edges forgotten" else group)
    if defect == "label is the maximum":
        lab = np.array([np.nonzero(lab == l)[0].max() for l in lab], np.int32)
    return idx, count, m, r, linked, lab


def _truth(X, k, max_d2=-1, num=2000, den=1000, group=None):
    idx, _, count = ref.lists(X, k, max_d2, group)
    m, r, linked = ref.links(idx, count, num, den)
    return idx, count, m, r, linked, ref.labels(idx, linked, group)[0]


def _differs(a, b):
    return not all(np.array_equal(x, y) for x, y in zip(a, b))


def test_planted_defects_are_seen():
    """(`p = c_x` replaced by k cannot be planted: y outside L_x while x is in L_y means L_x is full -- the cut and the groups are
    symmetric -- so c_x = k wherever that branch is taken.)"""
    blobs, group = search_cases.blobs(7, 60), cases.groups_in_runs(60)
    ties, one_sided = search_cases.ties(8, 60), line_points(0, 10, 13)
    everyone = np.zeros(20, np.int32)
    seen = {
        "no defect": _differs(_defective(None, blobs, 5, group=group), _truth(blobs, 5, group=group))
        or _differs(_defective(None, ties, 5), _truth(ties, 5)) or _differs(_defective(None, one_sided, 1, num=1, den=1), _truth(one_sided, 1, num=1, den=1)),
        "self kept": _differs(_defective("self kept", blobs, 5), _truth(blobs, 5)),
        "group row kept": _differs(_defective("group row kept", blobs, 5, group=group), _truth(blobs, 5, group=group)),
        "tie to the higher index": _differs(_defective("tie to the higher index", ties, 5), _truth(ties, 5)),
        "z != y dropped": _differs(_defective("z != y dropped", blobs, 5), _truth(blobs, 5)),
        "r as the maximum": _differs(_defective("r as the maximum", blobs, 5), _truth(blobs, 5)),
        "< for <=": _differs(_defective("< for <=", one_sided, 1, num=1, den=1), _truth(one_sided, 1, num=1, den=1)),
        "label is the maximum": _differs(_defective("label is the maximum", blobs, 5), _truth(blobs, 5)),
        "group edges forgotten": _differs(_defective("group edges forgotten", blobs[:20], 5, group=everyone), _truth(blobs[:20], 5, group=everyone)),
    }
    assert seen == {name: name != "no defect" for name in seen} and len(seen) == 9


def test_one_group_of_everyone_is_one_component_with_empty_lists():
    X, g = search_cases.blobs(9, 20), np.full(20, 13, np.int32)
    assert ref.lists(X, 5, group=g)[2].tolist() == [0] * 20 and ref.cast(X, 5, group=g)[0].tolist() == [0] * 20


def test_limits():
    X = search_cases.blobs(1, 4)
    for kw, what in ((dict(k=0), "k"), (dict(k=257), "k"), (dict(max_d2=-2), "max_d2"), (dict(num=-1), "num"), (dict(num=(1 << 20) + 1), "num"),
                     (dict(den=0), "den"), (dict(den=(1 << 20) + 1), "den"), (dict(group=np.array([0, 1, 4, -3], np.int32)), "group")):
        with pytest.raises(ref.Refused, match=what):
            ref.cast(X, **dict(dict(k=2), **kw))
    with pytest.raises(ref.Refused, match="dim"):
        ref.cast(X[:, :64], 2)
    Y = X.copy()
    Y[2, 5] = np.nan
    with pytest.raises(ref.Refused, match=r"X\[2\]\[5\]"):
        ref.cast(Y, 2)
    assert ref.cast(X, 256, num=1 << 20, den=1 << 20, group=np.array([3, -1, 3, -9], np.int32))[0].tolist()[2] == 0


# ---- the mean rule -----------------------------------------------------------------------------------------------------------------------
def test_the_mean_rule():
    col = lambda *v: np.array(v, np.int64)[:, None]           # noqa: E731
    for rows, want in ((col(-1, -2), -1), (col(1, 2), 2), (col(-1, 0, 0), 0), (col(-1, -1, 0), -1), (col(-3, -4), -3), (col(5), 5), (col(-5), -5),
                       (col(1, 1, 2, 2), 2), (col(-1, -1, -2, -2), -1), (col(1 << 20, 1 << 20), 1 << 20), (col(-(1 << 20), -(1 << 20)), -(1 << 20))):
        assert face_cast.track_mean(rows)[0] == want == ref.track_mean(rows)[0], rows.ravel()
        s, n = int(rows.sum()), len(rows)
        assert want == int(np.floor(s / n + 0.5))             # round half up (small integers: the float is exact)
    q = np.random.default_rng(0).integers(-(1 << 20), (1 << 20) + 1, (9, 128))
    assert np.array_equal(face_cast.track_mean(q), ref.track_mean(q)) and face_cast.track_mean(q).dtype == np.int64


def test_a_mean_survives_the_division_by_1e5():
    m = np.concatenate([np.arange(-(1 << 20), -(1 << 20) + 3000), np.arange(-3000, 3000), np.arange((1 << 20) - 3000, (1 << 20) + 1),
                        np.random.default_rng(1).integers(-(1 << 20), 1 << 20, 200000)])
    assert np.array_equal(np.rint((m / 1e5) * 100000.0).astype(np.int64), m)
    assert np.array_equal(search_ref.quantise((m[:1280] / 1e5).reshape(10, 128)).ravel(), m[:1280])


def test_threshold_and_distance():
    assert face_cast.threshold_fraction(2.0) == (2000, 1000) and face_cast.threshold_fraction(0) == (0, 1000)
    assert face_cast.threshold_fraction(0.0005) == (0, 1000) and face_cast.threshold_fraction(1.2345) == (1234, 1000)
    with pytest.raises(ValueError, match="threshold"):
        face_cast.threshold_fraction(-0.1)
    with pytest.raises(ValueError, match="threshold"):
        face_cast.threshold_fraction(float("nan"))


# ---- the verb on a scripted context ----------------------------------------------------------------------------------------------------
class ScriptContext(object):
    """the device side of FaceCast, scripted: the restatement"""

    def __init__(self):
        self.calls = []

    def cast(self, X, k, max_d2=-1, num=2000, den=1000, group=None):
        self.calls.append(dict(N=len(X), k=k, max_d2=max_d2, num=num, den=den, group=group))
        return ref.cast(X, k, max_d2, num, den, group)

    def cast_lists(self, X, k, max_d2=-1, group=None):
        return ref.lists(X, k, max_d2, group)


@pytest.fixture
def script(monkeypatch):
    ctx = ScriptContext()
    monkeypatch.setattr(runtime, "default_context", lambda: ctx)
    return ctx


@pytest.fixture
def clip(tmp_path):
    files = search_cases.two_files()
    paths = [str(tmp_path / n) for n in ("a.txt", "b.txt")]
    for p, (t, track, X) in zip(paths, files):
        with open(p, "w") as f:
            for i in range(len(t)):
                f.write(formats.embedding_line(t[i], int(track[i]), X[i]))
    return paths, files


PERSON = {("a.txt", 0): 0, ("a.txt", 1): 1, ("a.txt", 2): 0, ("a.txt", 3): 2, ("b.txt", 0): 1, ("b.txt", 1): 3, ("b.txt", 5): 0, ("b.txt", 7): 4}


def _text(lines):
    return "".join("%s %d %d\n" % l for l in lines)


@pytest.mark.parametrize("by", ["track", "face"])
def test_cast_verb(tmp_path, script, clip, capsys, by):
    paths, files = clip
    out = str(tmp_path / "cast.txt")
    table = [(p, f[1], f[2]) for p, f in zip(paths, files)]
    want = ref.verb(table, 64, cases.DEFAULT_MAX_D2, 2000, 1000, by)
    assert cli.main(["cast", "--by", by, out] + paths + paths[:1]) == 0                  # (a file given twice is read once)
    assert open(out).read() == _text(want) and len(want) == 8
    call = script.calls[-1]
    assert (call["k"], call["max_d2"], call["num"], call["den"]) == (64, 60000 ** 2, 2000, 1000)
    assert (call["N"], call["group"] is None) == ((8, True) if by == "track" else (44, False))
    # the tracks of one planted person share a `person`, across the two files, and nobody else does
    got = {(os.path.basename(p), t): person for p, t, person in want}
    assert all((got[a] == got[b]) == (PERSON[a] == PERSON[b]) for a in PERSON for b in PERSON)
    assert [l[2] for l in want][:2] == [0, 1] and sorted(set(l[2] for l in want)) == list(range(5))      # numbered by ascending label
    # other settings reach the call; stdout; --labels and --graph
    graph = str(tmp_path / "graph.npz")
    assert cli.main(["cast", "--by", by, "-k", "3", "--max-distance", "0.3", "--threshold", "0.5", "--labels", ".persons", "--graph", graph, "-"] + paths) == 0
    call = script.calls[-1]
    assert (call["k"], call["max_d2"], call["num"], call["den"]) == (3, 30000 ** 2, 500, 1000)
    want = ref.verb(table, 3, 30000 ** 2, 500, 1000, by)
    assert capsys.readouterr().out == _text(want)
    for p in paths:
        assert open(p + ".persons").read() == "".join("%d %d\n" % (t, person) for q, t, person in want if q == p)
    from pyannote_video_amd import identification
    assert identification.read_label_map(paths[1] + ".persons") == {t: person for q, t, person in want if q == paths[1]}
    g = np.load(graph)
    assert g["idx"].shape == (call["N"], 3) and g["d2"].dtype == np.int64 and len(g["count"]) == len(g["X"]) == len(g["owner"]) == call["N"]


def test_track_nodes_are_the_integer_means(script, clip):
    paths, files = clip
    fc = face_cast.FaceCast().add(paths[0]).add(paths[1]).add(paths[0])
    assert len(fc) == 44 and fc.paths == paths and fc.keys == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 5), (1, 7)]
    X, group, owner = fc.nodes("track")
    assert group is None and X.shape == (8, 128) and list(owner) == list(range(8))
    t, track, rows = files[1]
    q = search_ref.quantise(rows[track == 5])
    assert np.array_equal(search_ref.quantise(X[6:7])[0], (2 * q.sum(0) + len(q)) // (2 * len(q)))
    X, group, owner = fc.nodes("face")
    assert X.shape == (44, 128) and np.array_equal(group, owner) and group.dtype == np.int32 and group.max() == 7


def test_cast_verb_refusals(tmp_path, script, clip, capsys):
    paths, _ = clip
    out = str(tmp_path / "cast.txt")
    empty = str(tmp_path / "empty.txt")
    open(empty, "w").close()

    def refused(argv, message):
        with pytest.raises(SystemExit):
            cli.main(["cast"] + argv)
        assert message in capsys.readouterr().err, message
    refused([out, empty], "the table is empty")
    refused(["-k", "0", out] + paths, "k must lie in 1 .. 256")
    refused(["-k", "257", out] + paths, "k must lie in 1 .. 256")
    refused(["--threshold", "-1", out] + paths, "a threshold is not negative")
    refused(["--max-distance", "-0.5", out] + paths, "a distance is not negative")
    refused(["--by", "film", out] + paths, "--by is track or face")
    assert script.calls == [] and not os.path.exists(out)


# ---- the kernels' resources -------------------------------------------------------------------------------------------------------------
SOURCE = os.path.join("pyannote-video_amd", "csrc", "cast.hip")


@pytest.fixture(scope="module")
def report():
    if kernel_resources.hipcc() is None:
        pytest.skip("no hipcc")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), os.path.join(ROOT, SOURCE)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return {k["kernel"]: k for k in json.loads(out.stdout)[SOURCE]}


@pytest.mark.parametrize("kernel", ["cast_prep_k", "cast_first_k", "cast_links_k", "cast_hook_k", "cast_jump_k"])
def test_no_spills_and_no_scratch(report, kernel):
    k = report[kernel]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch_bytes_per_lane"] == 0, k
    assert k["occupancy_waves_per_simd"] == 8, k
