"""Minimal stand-ins for the two pyannote.core types the face path and the shot threading touch (pyannote.core is not a dependency).

Reference usage: `Segment(start, end)` with truthiness = non-empty (clustering.py:55-57,78), and
`Annotation(modality='face')` filled as `annotation[segment, track] = label` (clustering.py:76-80)."""


class Segment(object):
    __slots__ = ("start", "end")

    def __init__(self, start=0.0, end=0.0):
        self.start, self.end = float(start), float(end)

    def __bool__(self):
        # pyannote.core.Segment: empty when end - start is below its precision (1e-6)
        return (self.end - self.start) > 1e-6

    __nonzero__ = __bool__

    @property
    def duration(self):
        return self.end - self.start if self else 0.0

    def __iter__(self):
        return iter((self.start, self.end))

    def __eq__(self, o):
        return isinstance(o, Segment) and (self.start, self.end) == (o.start, o.end)

    def __hash__(self):
        return hash((self.start, self.end))

    def __lt__(self, o):
        return (self.start, self.end) < (o.start, o.end)

    def __repr__(self):
        return "<Segment(%g, %g)>" % (self.start, self.end)


class Annotation(object):
    """ordered {(segment, track): label}"""

    def __init__(self, uri=None, modality=None):
        self.uri, self.modality = uri, modality
        self._d = {}

    def __setitem__(self, key, label):
        # a bare segment is track '_' (pyannote.core: `annotation[segment] = label`, structure/thread.py:201)
        segment, track = (key, "_") if isinstance(key, Segment) else key
        self._d[(segment, track)] = label

    def __getitem__(self, key):
        return self._d[(key, "_") if isinstance(key, Segment) else tuple(key)]

    def __len__(self):
        return len(self._d)

    def itertracks(self, yield_label=False):
        for (segment, track), label in sorted(self._d.items(), key=lambda kv: (kv[0][0].start, kv[0][0].end, str(kv[0][1]))):
            yield (segment, track, label) if yield_label else (segment, track)

    def labels(self):
        return sorted(set(self._d.values()))

    def get_timeline(self):
        return sorted(set(s for s, _ in self._d))

    def copy(self):
        a = Annotation(self.uri, self.modality)
        a._d = dict(self._d)
        return a

    def rename_labels(self, mapping):
        a = self.copy()
        for k, v in a._d.items():
            a._d[k] = mapping.get(v, v)
        return a

    def __eq__(self, o):
        return isinstance(o, Annotation) and self._d == o._d

    # ---- what shot threading uses (structure/thread.py:203-226)
    def subset(self, labels):
        """the tracks whose label is in `labels`"""
        keep = set(labels)
        a = Annotation(self.uri, self.modality)
        a._d = dict((k, v) for k, v in self._d.items() if v in keep)
        return a

    def smooth(self, collar=0.):
        """pyannote.core's Annotation.smooth: per label (sorted), the union of its segments where they touch or overlap (gaps
        shorter than `collar` bridged), one new track per merged segment named by string_generator()"""
        names = string_generator()
        out = Annotation(self.uri, self.modality)
        for label in self.labels():
            segs = sorted(s for (s, _), l in self._d.items() if l == label)
            merged = []
            for s in segs:
                if merged:
                    gap = Segment(min(merged[-1].end, s.end), max(merged[-1].start, s.start))     # Segment ^ Segment
                    if not gap or gap.duration < collar:
                        merged[-1] = Segment(min(merged[-1].start, s.start), max(merged[-1].end, s.end))
                        continue
                merged.append(s)
            for s in merged:
                out[s, next(names)] = label
        return out

    def for_json(self):
        """pyannote.core.json's form: {"pyannote": "Annotation", "content": [{"segment": {start, end}, "track", "label"}], uri, modality}"""
        data = {"pyannote": "Annotation",
                "content": [{"segment": {"start": s.start, "end": s.end}, "track": t, "label": l} for s, t, l in self.itertracks(yield_label=True)]}
        if self.uri:
            data["uri"] = self.uri
        if self.modality:
            data["modality"] = self.modality
        return data

    @classmethod
    def from_json(cls, data):
        a = cls(data.get("uri"), data.get("modality"))
        for item in data["content"]:
            a[Segment(item["segment"]["start"], item["segment"]["end"]), item["track"]] = item["label"]
        return a


def string_generator():
    """pyannote.core.utils.generators.string_generator: A, B, ..., Z, AA, AB, ..."""
    import itertools
    import string
    r = 1
    while True:
        for c in itertools.product(string.ascii_uppercase, repeat=r):
            yield "".join(c)
        r += 1
