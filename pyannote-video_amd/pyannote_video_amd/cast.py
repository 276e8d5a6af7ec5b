"""WHO the people of many films are: rank-order clustering on the exact k-NN graph of the tracks (or faces) of any number of embedding
files (the `cast` verb; CAST.md states every rule).

No reference call -- the reference clusters one film through a T x T matrix.  The nodes' table goes to the GPU once (csrc/cast.hip;
pvf_cast): the exact k nearest nodes of every node by (d2, row), the rank-order link rule of Otto, Wang and Jain (2016) on those lists in
integers, connected components.  Only the labels come back.  No accuracy is claimed for the defaults: they are untuned."""
import os
import numpy as np
from . import formats
from .search import max_d2_of

MAX_K = 256
DEN = 1000
BY = ("track", "face")


def quantise(X):
    """q(v) = rint(v * 100000.0) -> int64 (SEARCH.md section 1); a value that is not finite or beyond 2^20 is refused"""
    X = np.asarray(X, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.rint(X * 100000.0)
        bad = ~(np.isfinite(X) & (np.abs(q) <= 1 << 20))
    if bad.any():
        r, c = np.argwhere(bad)[0]
        raise ValueError("cast: X[%d][%d] is not finite or lies beyond 2^20 units of 1e-5: refused, nothing is clamped" % (r, c))
    return q.astype(np.int64)


def track_mean(q):
    """the integer mean of a track's quantised rows, per column: (2 S + n) // (2 n) with S the int64 sum -- halves go up"""
    q = np.asarray(q, np.int64)
    n = len(q)
    return (2 * q.sum(0) + n) // (2 * n)


def threshold_fraction(threshold):
    """--threshold t -> (num, den) = (rint(t * 1000), 1000)"""
    t = float(threshold)
    if not t >= 0:
        raise ValueError("cast: a threshold is not negative")
    return int(np.rint(t * DEN)), DEN


class FaceCast(object):
    """the rows of one or more embedding files; every (file, track) is a group, numbered in the order of first appearance"""

    def __init__(self, ctx=None):
        self.ctx = ctx
        self.paths, self.keys, self._key = [], [], {}
        self._track, self._X, self._group = [], [], []

    def add(self, path):
        """an embedding file given twice is read once"""
        real = os.path.realpath(path)
        if any(os.path.realpath(p) == real for p in self.paths):
            return self
        _, track, X = formats.read_embeddings(path)
        f = len(self.paths)
        self.paths.append(path)
        for t in sorted(set(int(t) for t in track)):
            self._key[(f, t)] = len(self.keys)
            self.keys.append((f, t))
        self._track.append(track); self._X.append(X)
        self._group.append(np.array([self._key[(f, int(t))] for t in track], np.int32))
        return self

    def __len__(self):
        return int(sum(len(t) for t in self._track))

    def nodes(self, by="track"):
        """-> (X float64 [N, 128], group int32 [N] or None, owner int [N]: the (file, track) number of every node)"""
        if by not in BY:
            raise ValueError("cast: --by is track or face")
        if len(self) == 0:
            raise ValueError("cast: the table is empty (no row in %s)" % (", ".join(self.paths) or "no file"))
        X = np.ascontiguousarray(np.concatenate(self._X), np.float64)
        group = np.concatenate(self._group)
        if by == "face":
            return X, group, group
        q = quantise(X)
        means = np.array([track_mean(q[group == g]) for g in range(len(self.keys))], np.int64)
        return means / 1e5, None, np.arange(len(self.keys), dtype=np.int32)

    def run(self, k=64, max_distance=0.6, threshold=2.0, by="track", graph=None):
        """-> [(path, track, person)] by file, then track; persons are numbered 0, 1, ... by ascending label.  graph: a path that gets
        the lists (idx, d2, count) and the node table as an .npz"""
        from . import runtime
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("cast: k must lie in 1 .. %d" % MAX_K)
        num, den = threshold_fraction(threshold)
        max_d2 = max_d2_of(max_distance)
        X, group, owner = self.nodes(by)
        ctx = self.ctx or runtime.default_context()
        labels, _ = ctx.cast(X, k, max_d2=max_d2, num=num, den=den, group=group)
        if graph is not None:
            idx, d2, count = ctx.cast_lists(X, k, max_d2=max_d2, group=group)
            np.savez(graph, idx=idx, d2=d2, count=count, X=X, owner=owner, labels=labels)
        first = np.full(len(self.keys), -1, np.int64)
        first[owner[::-1]] = np.arange(len(owner))[::-1]          # a row of every (file, track): its rows share one label
        node_label = labels[first]
        person = {int(l): i for i, l in enumerate(np.unique(node_label))}
        return [(self.paths[f], t, person[int(node_label[g])]) for g, (f, t) in enumerate(self.keys)]


def write_cast(output, lines):
    """one line per (file, track): `path track person`; output: a path, or - for stdout"""
    import sys
    f = sys.stdout if output == "-" else open(output, "w")
    try:
        for path, track, person in lines:
            f.write("%s %d %d\n" % (path, track, person))
    finally:
        if output != "-":
            f.close()
        else:
            f.flush()


def write_label_files(lines, suffix):
    """<embeddings><suffix> beside each file: the `identifier label` lines that demo / faces / redact --label and identify --labels read"""
    by_path = {}
    for path, track, person in lines:
        by_path.setdefault(path, []).append((track, person))
    for path, rows in by_path.items():
        with open(path + suffix, "w") as f:
            for track, person in rows:
                f.write("%d %d\n" % (track, person))
