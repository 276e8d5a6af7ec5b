"""Shot boundary detection: the reference's `Shot` (pyannote/video/structure/shot.py) with the displaced
frame differences computed on the GPU -- the producer of the shot file that `track` reads and that multi-GPU jobs are cut along.

The reference converts every frame to a 50-pixel-wide gray image, runs OpenCV's Farneback optical flow between consecutive images, and
walks every pixel in Python to build the displaced frame (shot.py:75-99).  Here the frames already staged in HBM are reduced to the small
gray images in one launch and every consecutive pair is one workgroup (csrc/shot.hip).  What happens to the differences afterwards --
median filtering, the threshold on the normalised difference, "first of a run of consecutive frames" -- is the reference's code path
(shot.py:119-147), kept in Python.  OpenCV's arithmetic is restated, not linked: PARITY UNPINNED (see oracle/pvo_shot.c).
"""
import numpy as np

try:                                    # the reference's own segment type where it is installed (structure/shot.py:33) ...
    from pyannote.core import Segment, Annotation
except ImportError:                     # ... a stand-in with the same constructor and truthiness where it is not
    from ._core import Segment, Annotation


def shot_tables(poly_n=5, poly_sigma=1.1):
    """the 22 floats both the kernels and the oracle work from: the normalised Gaussian g[x], x g[x], x^2 g[x] for x = 0..5 and the four
    entries (1,1), (0,3), (3,3), (5,5) of the inverse moment matrix of the polynomial expansion (Farneback 2003; computed in double)"""
    if poly_n != 5:
        raise ValueError("the kernels are written for poly_n = 5 (the reference's value, shot.py:80-84)")
    n = poly_n
    x = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-x * x / (2.0 * poly_sigma * poly_sigma))
    g = (g * (1.0 / g.sum())).astype(np.float32)
    t = np.zeros(22, np.float32)
    k = np.arange(0, n + 1)
    t[0:6] = g[n:]
    t[6:12] = (k * g[n:]).astype(np.float32)
    t[12:18] = (k * k * g[n:]).astype(np.float32)
    gd = g.astype(np.float64)
    w = np.outer(gd, gd)                               # w[y, x]
    X, Y = np.meshgrid(x, x)
    G = np.zeros((6, 6))
    G[0, 0] = w.sum(); G[1, 1] = (w * X * X).sum(); G[3, 3] = (w * X ** 4).sum(); G[5, 5] = (w * X * X * Y * Y).sum()
    G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G[1, 1]
    G[4, 4] = G[3, 3]
    G[3, 4] = G[4, 3] = G[5, 5]
    inv = np.linalg.inv(G)
    t[18], t[19], t[20], t[21] = inv[1, 1], inv[0, 3], inv[3, 3], inv[5, 5]
    return t


def boundaries(times, dfd, start, end, kernel_size, threshold):
    """The reference's decision rule (shot.py:119-147) on the displaced frame differences dfd[i] taken at times[i]: a frame is a
    candidate when its difference exceeds the median-filtered one by more than `threshold` times that median; of a run of candidates at
    consecutive indices only the first counts -- where "consecutive" is judged against the previous candidate, or against index 0 for the
    first one (so a candidate at index 1 never counts: the reference's loop starts from `_i = 0`).  Segments run from cut to cut; the
    last one is kept if it is not empty.  Array form of that loop; tests/test_shot.py holds it equal to the reference class run verbatim."""
    import scipy.signal
    y = np.asarray(dfd, np.float64)
    base = scipy.signal.medfilt(y, kernel_size=kernel_size)
    with np.errstate(divide="ignore", invalid="ignore"):
        excess = (y - base) / base
    candidates = np.flatnonzero(excess > threshold)
    before = np.concatenate(([0], candidates[:-1]))
    cuts = candidates[candidates != before + 1]
    edges = [start] + [times[int(i)] for i in cuts] + [end]
    segments = [Segment(a, b) for a, b in zip(edges[:-1], edges[1:])]
    return segments[:-1] + ([segments[-1]] if segments[-1] else [])


class Shot(object):
    """Shot boundary detection based on displaced frame difference (shot.py:40-69)

    Parameters
    ----------
    video : iterable of (t, rgb) with `_size` (width, height), `step`, `start`, `end` like the reference's Video
    height : int, optional      the small image is this many pixels WIDE (the reference hands (height, int(w * height / h)) to cv2.resize as
                                (width, height)).  Defaults to 50 (one pyramid level of the optical flow; a side of 64 pixels or more brings
                                OpenCV's coarser levels, computed in the same kernel).
    context : float, optional   median filtering context in seconds.  Defaults to 2.
    threshold : float, optional Defaults to 1.
    ctx : runtime.Context
    chunk : frames reduced and compared per call (consecutive chunks overlap by one frame)
    """

    def __init__(self, video, height=50, context=2.0, threshold=1.0, ctx=None, chunk=1024):
        self.video = video
        self.height = height
        self.threshold = threshold
        self.context = context
        frame_w, frame_h = self.video._size
        # (shot.py:62) handed to cv2.resize as dsize, i.e. (width, height) of the small image
        self._resize = (self.height, int(frame_w * self.height / frame_h))
        # (shot.py:65-67) median window in frames: odd, at least 3
        self._kernel_size = max(3, int(np.ceil(self.context / self.video.step) // 2 * 2 + 1))
        if ctx is None:
            from .runtime import Context
            ctx = Context(0)
        self.ctx = ctx
        self.chunk = int(chunk)
        self._tables = shot_tables()

    def iter_dfd(self):
        """Pairwise displaced frame difference: (t of the later frame, dfd), like shot.py:101-117"""
        ow, oh = self._resize
        pending_t, pending_f = [], []
        for t, rgb in self.video:
            pending_t.append(t)
            pending_f.append(rgb)
            if len(pending_f) == self.chunk:
                for item in self._flush(pending_t, pending_f, ow, oh):
                    yield item
                pending_t, pending_f = pending_t[-1:], pending_f[-1:]       # the next chunk starts with this chunk's last frame
        if len(pending_f) > 1:
            for item in self._flush(pending_t, pending_f, ow, oh):
                yield item

    def _flush(self, ts, frames, ow, oh):
        dfd = self.ctx.shot_dfd(frames, ow, oh, self._tables)
        return list(zip(ts[1:], dfd.tolist()))

    def __iter__(self):
        pairs = list(self.iter_dfd())
        if not pairs:
            last = Segment(self.video.start, self.video.end)
            if last:
                yield last
            return
        t, y = zip(*pairs)
        for segment in boundaries(t, y, self.video.start, self.video.end, self._kernel_size, self.threshold):
            yield segment


# ---- shot threading: the reference's `Thread` (pyannote/video/structure/thread.py) --------------------------------
# ORB extraction and the 2-nearest-neighbour Hamming matching run on the GPU (csrc/orb.hip, two launches for a whole video); the graph
# work around them -- which pairs, connected components, labels, smoothing, biconnected components for the scenes -- is plain Python
# here (union-find and Tarjan instead of networkx, which is not a dependency).

def lookahead_pairs(n, lookahead):
    """the pairs (i, k) of thread.py's product_lookahead over n items: exactly 1 <= k - i <= lookahead (in the reference's order)"""
    return [(i, k) for i in range(n) for k in range(i + 1, min(n, i + lookahead + 1))]


def connected_components(n, edges):
    """union-find: the components of the graph on nodes 0..n-1, each a sorted list, ordered by their first node"""
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a, b in edges:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    groups = {}
    for i in range(n):
        groups.setdefault(find(i), []).append(i)
    return sorted(groups.values())


def biconnected_components(edges):
    """Tarjan (iterative): the node sets of the biconnected components of an undirected graph given by its edges (nodes hashable)"""
    adj = {}
    for a, b in edges:
        if a == b:
            continue
        adj.setdefault(a, set()).add(b)
        adj.setdefault(b, set()).add(a)
    disc, low, out = {}, {}, []
    counter = 0
    for root in adj:
        if root in disc:
            continue
        disc[root] = low[root] = counter; counter += 1
        stack = [(root, None, iter(adj[root]))]
        estack = []
        while stack:
            u, parent, it = stack[-1]
            advanced = False
            for v in it:
                if v == parent:
                    continue
                if v not in disc:
                    disc[v] = low[v] = counter; counter += 1
                    estack.append((u, v))
                    stack.append((v, u, iter(adj[v])))
                    advanced = True
                    break
                if disc[v] < disc[u]:
                    low[u] = min(low[u], disc[v])
                    estack.append((u, v))
            if advanced:
                continue
            stack.pop()
            if parent is not None:
                low[parent] = min(low[parent], low[u])
                if low[u] >= disc[parent]:
                    comp = set()
                    while True:
                        e = estack.pop()
                        comp.update(e)
                        if e == (parent, u):
                            break
                    out.append(comp)
    return out


def thread_labels(shots, edges):
    """thread.py:193-205: threads = connected components (each sorted), ordered by their first shot, labelled A, B, ..., smoothed"""
    from ._core import string_generator
    order = sorted(range(len(shots)), key=lambda i: shots[i])
    rank = {i: r for r, i in enumerate(order)}
    comps = connected_components(len(shots), [(rank[a], rank[b]) for a, b in edges])
    annotation = Annotation()
    names = string_generator()
    for comp in comps:
        label = next(names)
        for r in comp:
            annotation[shots[order[r]]] = label
    return annotation.smooth()


def thread_scenes(threads):
    """thread.py:207-232: adjacent shots and consecutive shots of one thread linked; every biconnected component of 3 or more shots
    takes the (current) label of its first shot, components visited in sorted order"""
    tracks = list(threads.itertracks())
    edges = list(zip(tracks[:-1], tracks[1:]))
    for label in threads.labels():
        sub = list(threads.subset([label]).itertracks())
        edges += list(zip(sub[:-1], sub[1:]))
    scenes = threads.copy()
    for shots in sorted(sorted(bc) for bc in biconnected_components(edges)):
        if len(shots) < 3:
            continue
        common = scenes[shots[0]]
        for shot in shots:
            scenes[shot] = common
    return scenes


class Thread(object):
    """Shot threading based on ORB features (thread.py:85-232)

    Parameters
    ----------
    video : frames by index (`frame(i)`, or the reference's `video(t)`), `frame_rate`, `_size` (width, height)
    shot : iterable of segments, optional   Defaults to the product's Shot(video) (as the reference does)
    height : int, optional      the small image is this many pixels WIDE (cv2.resize gets (height, int(w * height / h)) as dsize)
    min_match : int, optional   shots are linked when MORE than this many descriptors pass the ratio test.  Defaults to 20.
    lookahead : int, optional   each shot is compared with the next `lookahead` shots.  Defaults to 5 (the CLI passes 24).
    ctx : runtime.Context
    cap : keypoints a frame may keep (500 plus the ties retainBest keeps); None: as many as the frames have (Context.orb_extract)
    chunk : frames extracted per call
    """

    def __init__(self, video, shot=None, height=200, min_match=20, lookahead=5, verbose=False, ctx=None, cap=None, chunk=512):
        self.video = video
        self.height = height
        w, h = self.video._size
        self._resize = (int(self.height), int(w * self.height / h))
        self.lookahead = lookahead
        if ctx is None:
            from .runtime import Context
            ctx = Context(0)
        self.ctx = ctx
        if shot is None:
            shot = Shot(video, ctx=ctx)
        self.shot = shot
        self.verbose = verbose
        self.min_match = min_match
        self.cap, self.chunk = None if cap is None else int(cap), int(chunk)

    def _frame_index(self, t):
        """video(t) reads frame int(fps * t + 1e-5) (video.py:486, truncation toward zero); None where there is no such frame"""
        i = int(self.video.frame_rate * t + 0.00001)
        return i if 0 <= i < len(self.video) else None

    def _read(self, i):
        if hasattr(self.video, "frame"):
            return self.video.frame(i)
        return self.video(i / self.video.frame_rate)

    def match_counts(self):
        """(shots, pairs (i, k), n_matches per pair) -- thread.py:172-191 with every needed frame read once, ORB on all of them in one
        pass and all pairs matched in one launch"""
        import warnings
        shots = [s if isinstance(s, Segment) else Segment(s.start, s.end) for s in self.shot]
        pairs = lookahead_pairs(len(shots), self.lookahead)
        collar = 10. / self.video.frame_rate
        last = [self._frame_index(s.end - collar) for s in shots]
        first = [self._frame_index(s.start + collar) for s in shots]
        for s, a, b in zip(shots, last, first):
            for t, i in ((s.end - collar, a), (s.start + collar, b)):
                if i is None:
                    warnings.warn("unable to reach t = {t:.3f}".format(t=t))
        needed = sorted(set(last[i] for i, _ in pairs if last[i] is not None) | set(first[k] for _, k in pairs if first[k] is not None))
        pos = {f: j for j, f in enumerate(needed)}
        valid = [p for p, (i, k) in enumerate(pairs) if last[i] is not None and first[k] is not None]
        counts = np.zeros(len(pairs), np.int64)
        if not valid:
            return shots, pairs, counts
        set_pairs = [(pos[last[pairs[p][0]]], pos[first[pairs[p][1]]]) for p in valid]
        ow, oh = self._resize
        if len(needed) <= self.chunk:
            self.ctx.orb_extract([self._read(f) for f in needed], ow, oh, self.cap)
            got = self.ctx.orb_match_counts(set_pairs)
        else:
            rows = np.zeros(len(needed), np.int32)
            desc = np.zeros((len(needed), 0, 32), np.uint8)
            for j0 in range(0, len(needed), self.chunk):
                part = needed[j0:j0 + self.chunk]
                n, _, d = self.ctx.orb_extract([self._read(f) for f in part], ow, oh, self.cap)
                if d.shape[1] > desc.shape[1]:          # the first chunk, or one whose frames needed a larger cap: widen every set
                    desc = np.pad(desc, ((0, 0), (0, d.shape[1] - desc.shape[1]), (0, 0)))
                rows[j0:j0 + len(part)] = n
                desc[j0:j0 + len(part), :d.shape[1]] = d
            got = self.ctx.orb_match_counts(set_pairs, desc, rows)
        counts[valid] = got
        return shots, pairs, counts

    def __call__(self):
        shots, pairs, counts = self.match_counts()
        edges = [p for p, c in zip(pairs, counts) if c > self.min_match]
        return thread_labels(shots, edges)

    def scenes(self, threads):
        return thread_scenes(threads)
