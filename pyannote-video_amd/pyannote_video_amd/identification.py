"""WHO a face is: tracks or clusters named against a gallery of enrolled faces (the `enroll`, `enroll-track` and `identify` verbs).

No reference call -- the reference stops at cluster numbers -- but the standard use of its embedder: "is the distance to a known face
below 0.6?".  The measure is the one `cluster` merges by: a group (a track, or a cluster: all rows of all its tracks) belongs to a person
when the MEAN PAIRWISE DISTANCE between its descriptors and the person's enrolled descriptors is at most the threshold -- one more
average-linkage step against fixed, named clusters, with FaceClustering's metric, `<=` and default of 0.6.  The T x K block means and the
decision per group run on the GPU (csrc/identify.hip; include/pvface.h states the rules: first minimum, lowest index on ties)."""
import os
import numpy as np
from . import _lib, formats

METRICS = {"euclidean": 0, "cosine": 1}


def _quantised(embeddings):
    """float64 [n, 128] as the 5-decimal text gives them back: float32 descriptors through np.round(float64, 5) (pvf_round_rows, what the
    in-memory clustering uses), anything else through the text itself"""
    E = np.asarray(embeddings)
    if E.ndim == 1:
        E = E[None]
    if E.ndim != 2 or E.shape[1] != 128:
        raise ValueError("faces are rows of 128 values")
    if E.dtype == np.float32:
        return _lib.round_rows(E, 5)
    return np.array([formats.quantise_embedding(row) for row in E], np.float64).reshape(-1, 128)


class FaceGallery(object):
    """named, enrolled descriptors; names keep the order in which they were first added"""

    def __init__(self):
        self._faces = {}

    def add(self, name, embeddings):
        formats.check_gallery_name(name)
        E = _quantised(embeddings)
        if len(E):
            self._faces.setdefault(name, []).append(E)
        return self

    @property
    def names(self):
        return list(self._faces)

    def __len__(self):
        return len(self._faces)

    def arrays(self):
        """(names[K], gal_start int32 [K+1], G float64 [M, 128])"""
        names = self.names
        blocks = [np.concatenate(self._faces[n]) for n in names]
        G = np.concatenate(blocks) if blocks else np.zeros((0, 128))
        return names, np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int32), np.ascontiguousarray(G, np.float64)

    def save(self, path, append=False):
        """without `append` an existing file is refused, not overwritten"""
        if not append and os.path.exists(path):
            raise FileExistsError("%s exists: --append adds to it" % path)
        names, start, G = self.arrays()
        with open(path, 'a' if append else 'w') as f:
            for k, name in enumerate(names):
                for row in G[start[k]:start[k + 1]]:
                    f.write(formats.gallery_line(name, row))

    @classmethod
    def load(cls, path):
        g = cls()
        names, start, G = formats.read_gallery(path)
        for k, name in enumerate(names):
            g._faces[name] = [G[start[k]:start[k + 1]]]
        return g


def _group_key(g):
    """groups sort as numbers where they are numbers (cluster labels, track identifiers), as text otherwise"""
    return (0, int(g), "") if isinstance(g, (int, np.integer)) else (1, 0, str(g))


def read_label_map(labels):
    """a {track: label} map, or the path of a `cluster` output (`identifier label` lines) -> {int track: label}"""
    if isinstance(labels, str):
        from . import render
        labels = render.read_labels(labels)

    def plain(v):          # "12" and 12 are one label
        try:
            return int(v) if str(int(v)) == str(v) else v
        except (TypeError, ValueError):
            return v
    return {int(k): plain(v) for k, v in labels.items()}


class FaceIdentification(object):
    """gallery: a FaceGallery or the path of a gallery file"""

    def __init__(self, gallery, threshold=0.6, metric="euclidean", ctx=None):
        if metric not in METRICS:
            raise ValueError("metric: euclidean or cosine")
        self.gallery = FaceGallery.load(gallery) if isinstance(gallery, str) else gallery
        if len(self.gallery) == 0:
            raise ValueError("the gallery is empty")
        self.threshold = float(threshold)
        self.metric = metric
        self.ctx = ctx

    def scores_arrays(self, track, X, groups=None, time=None):
        """-> [(group, nearest name or None, best_dist, second name or None, second_dist, matched)] in group order: the nearest identity
        even where its distance is above the threshold (`matched` False).  X: float64 rows as formats.read_embeddings returns them, or
        float32 descriptors (rounded to 5 decimals: the values `cluster` sees); groups: a {track: label} map, default one group per
        track; rows are sorted by (group, track, time) on the host -- without `time`, a track's rows keep their order."""
        from . import runtime
        track = np.asarray(track, np.int64)
        X = np.asarray(X)
        X = _lib.round_rows(X, 5) if X.dtype == np.float32 else np.ascontiguousarray(X, np.float64)
        if X.ndim != 2 or len(X) != len(track):
            raise ValueError("one row of X per entry of track")
        if len(track) == 0:
            return []
        tracks = np.unique(track)
        label = {int(t): int(t) for t in tracks}
        if groups is not None:
            label.update({t: g for t, g in read_label_map(groups).items() if t in label})
        ordered = sorted(set(label.values()), key=_group_key)
        rank = {g: i for i, g in enumerate(ordered)}
        row_group = np.array([rank[label[int(t)]] for t in tracks], np.int64)[np.searchsorted(tracks, track)]
        keys = (track, row_group) if time is None else (np.asarray(time, np.float64), track, row_group)
        order = np.lexsort(keys)                                    # stable: (group, track, time)
        row_start = np.concatenate([[0], np.cumsum(np.bincount(row_group, minlength=len(ordered)))]).astype(np.int32)
        names, gal_start, G = self.gallery.arrays()
        ctx = self.ctx or runtime.default_context()
        best, bd, second, sd, D = ctx.identify(np.ascontiguousarray(X[order]), row_start, G, gal_start, self.threshold,
                                               metric=METRICS[self.metric], return_dist=True)
        out = []
        for i, g in enumerate(ordered):
            near = int(best[i])
            if near < 0 and bd[i] < np.inf:                         # refused by the threshold: the entry the measured value was taken from
                near = int(np.flatnonzero(D[i] == bd[i])[0])
            out.append((g, names[near] if near >= 0 else None, float(bd[i]), names[second[i]] if second[i] >= 0 else None, float(sd[i]),
                        bool(best[i] >= 0)))
        return out

    def identify_arrays(self, track, X, groups=None, time=None):
        """-> {group: (name or None, best_dist, second_name or None, second_dist)}; a group is a track, or with `groups` a cluster"""
        return {g: (name if matched else None, bd, second, sd) for g, name, bd, second, sd, matched in self.scores_arrays(track, X, groups, time)}

    def identify(self, embedding_path, labels=None):
        time, track, X = formats.read_embeddings(embedding_path)
        return self.identify_arrays(track, X, labels, time)


def write_identification(output, scores, tracks, label, unknown=None, per_cluster=False, scores_output=None):
    """the `identifier name` file of `identify` (and of `process --gallery`), and the --scores file.  scores: scores_arrays' list; tracks:
    the identifiers to write, label: {track: group}.  Per track (per_cluster False) a track nobody matches is left out, or gets
    `unknown`; per cluster it keeps its cluster label (or gets `unknown`), so the file replaces `cluster`'s."""
    name_of = {g: name for g, name, _, _, _, matched in scores if matched}
    with open(output, 'w') as f:
        for t in sorted(int(t) for t in tracks):
            g = label.get(t, t)
            name = name_of.get(g, unknown if unknown is not None else (str(g) if per_cluster else None))
            if name is not None:
                f.write('{identifier:d} {name:s}\n'.format(identifier=t, name=name))
    if scores_output is not None:
        with open(scores_output, 'w') as f:
            for g, name, bd, second, sd, _ in scores:
                f.write('{g} {a} {bd:.6f} {b} {sd:.6f}\n'.format(g=g, a=name or '-', bd=bd, b=second or '-', sd=sd))
