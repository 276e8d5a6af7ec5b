"""WHERE ELSE a face appears: the exact k nearest faces across embedding files (the `search` verb; SEARCH.md states every rule).

No reference call -- the reference stops at cluster numbers.  A query is a set of rows: a track of an embedding file, a person of a
gallery, or an array of descriptors.  Every query row is searched on the GPU in one call (csrc/search.hip; pvf_search: exact integer
distances on the 5-decimal values, ranked by (d2, row)); the lists of a multi-row query are merged on the host by the MINIMUM over its
rows -- for every table row its smallest d2 over the query rows, then (d2, row) and the first k.  The merge is exact: a row among the k
best by the minimum is among the k best of the query row that attains it, so it is in that row's list."""
import os
import numpy as np
from . import formats, identification

MAX_K = 1024


class Hit(object):
    """one line of the result: row of the table, squared distance in units of 1e-5, and where the face is"""
    __slots__ = ("row", "d2", "path", "track", "time")

    def __init__(self, row, d2, path, track, time):
        self.row, self.d2, self.path, self.track, self.time = int(row), int(d2), path, int(track), float(time)

    @property
    def distance(self):
        return float(np.sqrt(float(self.d2)) / 1e5)

    def __repr__(self):
        return "Hit(row=%d, distance=%.5f, %s track %d at %.3f)" % (self.row, self.distance, self.path, self.track, self.time)


def max_d2_of(distance):
    """--max-distance D -> r = rint(D * 1e5), max_d2 = r * r (None: no cut, -1)"""
    if distance is None:
        return -1
    r = int(np.rint(float(distance) * 1e5))
    if r < 0:
        raise ValueError("search: a distance is not negative")
    return r * r


def merge_min(idx, d2, count, k):
    """the lists of the rows of one query -> [(d2, row)], by the minimum over the query rows, in (d2, row) order, the first k"""
    n = np.asarray(count, np.int64)
    take = np.arange(idx.shape[1])[None, :] < n[:, None]
    rows, dist = idx[take].astype(np.int64), d2[take].astype(np.int64)
    order = np.lexsort((dist, rows))                     # by row, the smallest d2 of a row first
    rows, dist = rows[order], dist[order]
    first = np.ones(len(rows), bool)
    first[1:] = rows[1:] != rows[:-1]
    rows, dist = rows[first], dist[first]
    order = np.lexsort((rows, dist))[:k]
    return [(int(dist[i]), int(rows[i])) for i in order]


class FaceSearch(object):
    """the table: the rows of one or more embedding files, each with its (path, time, track); every (file, track) is a group"""

    def __init__(self, ctx=None):
        self.ctx = ctx
        self.paths, self._key = [], {}
        self._T, self._track, self._file, self._X, self._group = [], [], [], [], []

    def add(self, path):
        """an embedding file given twice is read once"""
        real = os.path.realpath(path)
        if any(os.path.realpath(p) == real for p in self.paths):
            return self
        T, track, X = formats.read_embeddings(path)
        f = len(self.paths)
        self.paths.append(path)
        for t in track:
            self._key.setdefault((f, int(t)), len(self._key))
        self._T.append(T); self._track.append(track); self._X.append(X)
        self._file.append(np.full(len(T), f, np.int64))
        self._group.append(np.array([self._key[(f, int(t))] for t in track], np.int32))
        return self

    def __len__(self):
        return int(sum(len(t) for t in self._T))

    def _table(self):
        if len(self) == 0:
            raise ValueError("search: the table is empty (no row in %s)" % (", ".join(self.paths) or "no file"))
        return (np.concatenate(self._T), np.concatenate(self._track), np.concatenate(self._file),
                np.ascontiguousarray(np.concatenate(self._X), np.float64), np.concatenate(self._group))

    def group_of(self, path, track):
        """the group number of a (file, track) of the table, or -1"""
        real = os.path.realpath(path)
        for f, p in enumerate(self.paths):
            if os.path.realpath(p) == real:
                return self._key.get((f, int(track)), -1)
        return -1

    # ---- the three sources of a query
    @staticmethod
    def rows_of_track(path, track):
        _, ids, X = formats.read_embeddings(path)
        rows = X[ids == int(track)]
        if len(rows) == 0:
            raise ValueError("search: %s has no row of track %d" % (path, int(track)))
        return rows

    @staticmethod
    def rows_of_person(gallery, name):
        g = identification.FaceGallery.load(gallery) if isinstance(gallery, str) else gallery
        names, start, G = g.arrays()
        if name not in names:
            raise ValueError("search: the gallery has no %r (it has: %s)" % (name, ", ".join(names) or "nobody"))
        i = names.index(name)
        return G[start[i]:start[i + 1]]

    @staticmethod
    def rows_of_array(embeddings):
        """float32 descriptors round as the clustering rounds them (identification._quantised)"""
        return identification._quantised(embeddings)

    def search(self, rows, k=100, max_distance=None, exclude_group=-1, collapse=True):
        """-> [Hit] nearest first: the k nearest faces of the table to the query rows, and with `collapse` the best hit of each
        (file, track) among those k -- the tracks that own the k nearest faces, in the order of their nearest face (fewer than k lines
        may come out).  exclude_group: a group of the table the query does not find (its own track)."""
        from . import runtime
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("search: k must lie in 1 .. %d" % MAX_K)
        T, track, file, X, group = self._table()
        rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 128)
        if len(rows) == 0:
            raise ValueError("search: the query has no row")
        ctx = self.ctx or runtime.default_context()
        kw = {}
        if exclude_group >= 0:
            kw = dict(query_group=np.full(len(rows), exclude_group, np.int32), row_group=group)
        idx, d2, count = ctx.search(rows, X, k, max_d2=max_d2_of(max_distance), **kw)
        hits = merge_min(idx, d2, count, k)
        if collapse:
            seen, kept = set(), []
            for d, i in hits:
                if group[i] not in seen:
                    seen.add(group[i])
                    kept.append((d, i))
            hits = kept
        return [Hit(i, d, self.paths[file[i]], track[i], T[i]) for d, i in hits]


def write_hits(output, hits):
    """one line per hit: `rank distance path track T`; output: a path, or - for stdout"""
    import sys
    f = sys.stdout if output == "-" else open(output, "w")
    try:
        for rank, h in enumerate(hits):
            f.write("%d %.5f %s %d %.3f\n" % (rank, h.distance, h.path, h.track, h.time))
    finally:
        if output != "-":
            f.close()
        else:
            f.flush()
