"""Test infrastructure: the REFERENCE'S shot threading (pyannote/video/structure/thread.py), executed verbatim from the checkout named by
PVF_REFERENCE (tests/refhost.py's mechanism), on top of stand-in modules:
    cv2                 resize / cvtColor / ORB_create from tests/orb_ref.py; FlannBasedMatcher as the exact 2-nearest-neighbour search
    pyannote.core       the product's Annotation stand-in (_core.Annotation) and pyannote.core.utils.generators
    tqdm, pyannote.video.structure.shot   empty stand-ins (shots are given; no progress bar)
    networkx            the real package
"""
import os
import sys
import types

import numpy as np

import orb_ref
from refhost import REFERENCE, _load


def have_reference():
    return bool(REFERENCE) and os.path.isfile(os.path.join(REFERENCE, "pyannote", "video", "structure", "thread.py"))


class _KeyPoint(object):
    def __init__(self, row):
        self.pt = (float(row[0]), float(row[1]))
        self.octave, self.response, self.angle = int(row[2]), float(row[4]), float(row[5])


class _ORB(object):
    def detectAndCompute(self, gray, mask):
        kp, desc = orb_ref.orb_gray(gray)
        return [_KeyPoint(r) for r in kp], (desc if len(desc) else None)


class _DMatch(object):
    def __init__(self, q, t, d):
        self.queryIdx, self.trainIdx, self.distance = q, t, float(d)


class _Flann(object):
    def __init__(self, index_params, search_params):
        pass

    def knnMatch(self, query, train, k=2):
        d = orb_ref.hamming(query, train)
        order = np.argsort(d, axis=1, kind="stable")[:, :k]
        return [[_DMatch(q, int(t), d[q, t]) for t in order[q]] for q in range(len(query))]


def _stubs():
    from pyannote_video_amd import _core
    cv2 = types.ModuleType("cv2")
    cv2.__version__ = "3.4.2"
    cv2.COLOR_RGB2GRAY = 7
    cv2.resize = lambda img, dsize: orb_ref.resize_linear_rgb(img, dsize[0], dsize[1])
    cv2.cvtColor = lambda img, code: orb_ref.gray(img)
    cv2.ORB_create = _ORB
    cv2.FlannBasedMatcher = _Flann
    core = types.ModuleType("pyannote.core")
    core.Annotation, core.Segment = _core.Annotation, _core.Segment
    utils = types.ModuleType("pyannote.core.utils")
    gens = types.ModuleType("pyannote.core.utils.generators")
    gens.string_generator = _core.string_generator
    gens.pairwise = lambda it: (lambda l: zip(l[:-1], l[1:]))(list(it))
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda iterable=None, **kw: iterable
    mods = {"cv2": cv2, "pyannote.core": core, "pyannote.core.utils": utils, "pyannote.core.utils.generators": gens, "tqdm": tqdm}
    for name in ("pyannote", "pyannote.video", "pyannote.video.structure"):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REFERENCE, *name.split("."))]
        mods[name] = m
    shot = types.ModuleType("pyannote.video.structure.shot")
    shot.Shot = None
    mods["pyannote.video.structure.shot"] = shot
    return mods


def reference_thread_module():
    """thread.py loaded from the reference checkout with the stand-ins above in sys.modules (restored afterwards)"""
    mods = _stubs()
    saved = {k: sys.modules.get(k) for k in list(mods) + ["pyannote.video.structure.thread"]}
    sys.modules.update(mods)
    try:
        return _load("pyannote.video.structure.thread", os.path.join(REFERENCE, "pyannote", "video", "structure", "thread.py"))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def run_reference(video, shots, min_match=20, lookahead=24):
    """(threads, scenes, edges {(i, k): n_matches}) from the reference's Thread as scripts/pyannote-structure.py:72-80 calls it"""
    from pyannote_video_amd._core import Segment
    mod = reference_thread_module()
    segs = [Segment(a, b) for a, b in shots]
    th = mod.Thread(video, shot=segs, lookahead=lookahead, min_match=min_match)
    graph = th._threads_graph()
    edges = {(segs.index(u), segs.index(v)): d["n_matches"] for u, v, d in graph.edges(data=True)}
    threads = th()
    return threads, th.scenes(threads), edges
