"""Test infrastructure: runs the REFERENCE'S OWN Python, verbatim, from a checkout of pyannote-video named by PVF_REFERENCE, on top
of a dlib look-alike.

The reference is pure Python; everything it computes goes through `dlib`, `munkres`, `networkx`, numpy and pandas
(pyannote/video/tracking.py:31-35, face/face.py:30-32, scripts/pyannote-face.py:92-109).  None of its files is copied:
they are executed where they lie, with
    sys.modules['dlib']     = the module under test (pyannote_video_amd.shim on a GPU, tests/oracle_dlib.py on CPU)
    sys.modules['munkres']  = the real package (importable, or its munkres.py named by PVF_MUNKRES)
    `pyannote`, `pyannote.video`, `pyannote.video.face`, `pyannote.core`, `docopt`, `cv2` = empty / minimal stand-in modules,
      because pyannote/video/__init__.py would pull in ffmpeg / OpenCV code that is out of scope.
This is exactly the "edit" INTEGRATION.md describes: the reference's host code stays, only `import dlib` is re-pointed.

The reference is not part of this repository.  What its code returns on the tests' seeded inputs is recorded where it is available
(tests/golden/make_reference_golden.py, tests/golden/make_reference_pins.py) and travels as committed fixtures under tests/golden/,
which the tests compare the product and the oracle with (`recorded`).
"""
import contextlib
import gzip
import importlib.util
import json
import os
import sys
import types

REFERENCE = os.environ.get("PVF_REFERENCE", "")
MUNKRES_PY = os.environ.get("PVF_MUNKRES", "")
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_pins.json.gz")


def have_reference():
    return bool(REFERENCE) and os.path.isfile(os.path.join(REFERENCE, "pyannote", "video", "tracking.py"))


def have_munkres():
    return importlib.util.find_spec("munkres") is not None or os.path.isfile(MUNKRES_PY)


_pins = None


def recorded(name):
    """what the reference's code (or the real munkres package) returned for one test's seeded inputs: tests/golden/reference_pins.json.gz,
    written by tests/golden/make_reference_pins.py"""
    global _pins
    if _pins is None:
        with gzip.open(PINS, "rt") as f:
            _pins = json.load(f)
    return _pins[name]


def _load(name, path, register=True):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    if register:
        sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


_munkres = None


def real_munkres():
    """the munkres package itself (1.1.4): the installed one, else loaded from its source file"""
    global _munkres
    if _munkres is None:
        if importlib.util.find_spec("munkres") is not None:
            _munkres = importlib.import_module("munkres")
        else:
            spec = importlib.util.spec_from_file_location("_real_munkres", MUNKRES_PY)
            _munkres = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(_munkres)
    return _munkres


class _Segment(object):
    """what pyannote.core.json.load gives `track` for a shot file: objects with .end (tracking.py:48)"""

    def __init__(self, start, end):
        self.start, self.end = float(start), float(end)


@contextlib.contextmanager
def reference_modules(dlib_module, video_cls=None):
    """Context manager yielding a namespace with the reference's modules executed against `dlib_module`:
         .tracking       pyannote/video/tracking.py          (TrackingByDetection)
         .face           pyannote/video/face/face.py         (Face)
         .face_tracking  pyannote/video/face/tracking.py     (FaceTracking, get_face_detect)
         .cli            scripts/pyannote-face.py            (track, extract, getFaceGenerator, FACE_TEMPLATE)
    sys.modules is restored on exit."""
    saved = dict(sys.modules)
    try:
        sys.modules["dlib"] = dlib_module
        sys.modules["munkres"] = real_munkres()
        sys.modules["cv2"] = types.ModuleType("cv2")
        for pkg in ("pyannote", "pyannote.video", "pyannote.video.face"):
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
        ns = types.SimpleNamespace()
        base = os.path.join(REFERENCE, "pyannote", "video")
        ns.tracking = _load("pyannote.video.tracking", os.path.join(base, "tracking.py"))
        ns.face = _load("pyannote.video.face.face", os.path.join(base, "face", "face.py"))
        ns.face_tracking = _load("pyannote.video.face.tracking", os.path.join(base, "face", "tracking.py"))
        # what `from pyannote.video import ...` resolves in the CLI script (pyannote/video/__init__.py:33-44)
        pv = sys.modules["pyannote.video"]
        pv.__version__ = "reference"
        pv.Video = video_cls if video_cls is not None else object
        pv.Face = ns.face.Face
        pv.FaceTracking = ns.face_tracking.FaceTracking
        core = types.ModuleType("pyannote.core")
        core.__path__ = []

        class Annotation(object):       # only used in an isinstance() test (pyannote-face.py:256)
            pass
        core.Annotation = Annotation
        core_json = types.ModuleType("pyannote.core.json")

        def load(fp):
            import json
            return [_Segment(a, b) for a, b in json.load(fp)]
        core_json.load = load
        core.json = core_json
        sys.modules["pyannote.core"] = core
        sys.modules["pyannote.core.json"] = core_json
        sys.modules["pyannote"].core = core        # `import pyannote.core.json` then `pyannote.core.json.load(fp)` (pyannote-face.py:96,254)
        sys.modules["pyannote"].video = pv
        docopt = types.ModuleType("docopt")
        docopt.docopt = lambda *a, **k: {}
        sys.modules["docopt"] = docopt
        ns.cli = _load("_reference_pyannote_face_cli", os.path.join(REFERENCE, "scripts", "pyannote-face.py"))
        ns.Segment = _Segment
        yield ns
    finally:
        for k in list(sys.modules):
            if k not in saved:
                del sys.modules[k]
        sys.modules.update(saved)


@contextlib.contextmanager
def reference_shot_module(cv2_module, segment_cls):
    """pyannote/video/structure/shot.py executed verbatim with `cv2` = cv2_module (the CPU oracle's restatements of cvtColor / resize /
    calcOpticalFlowFarneback behind OpenCV's names) and `pyannote.core.Segment` = segment_cls.  Yields the module (its `Shot` class)."""
    saved = dict(sys.modules)
    try:
        sys.modules["cv2"] = cv2_module
        for pkg in ("pyannote", "pyannote.video", "pyannote.video.structure"):
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
        vid = types.ModuleType("pyannote.video.video")
        vid.Video = object                       # shot.py:32 imports the name only
        sys.modules["pyannote.video.video"] = vid
        core = types.ModuleType("pyannote.core")
        core.Segment = segment_cls
        sys.modules["pyannote.core"] = core
        yield _load("pyannote.video.structure.shot", os.path.join(REFERENCE, "pyannote", "video", "structure", "shot.py"))
    finally:
        for k in list(sys.modules):
            if k not in saved:
                del sys.modules[k]
        sys.modules.update(saved)


@contextlib.contextmanager
def reference_clustering_module(segment_cls, annotation_cls):
    """pyannote/video/face/clustering.py executed verbatim.  Its third-party bases are absent here, so they are stand-ins that do nothing of
    their own: `HACModel` (keeps the per-cluster models the reference's methods fill and read), `ValueSortedDict` (a dict),
    `HierarchicalAgglomerativeClustering` / `DistanceThreshold` (constructors only -- the agglomeration loop itself is
    pyannote.algorithms code and stays unpinned).  pandas >= 2 dropped `Series.iteritems` (clustering.py:77): the alias is restored while
    the module is in use.  Yields the module (`_Model`, `FaceClustering`)."""
    import pandas
    saved = dict(sys.modules)
    had_iteritems = hasattr(pandas.Series, "iteritems")
    try:
        if not had_iteritems:
            pandas.Series.iteritems = pandas.Series.items
        sc = types.ModuleType("sortedcollections")

        class ValueSortedDict(dict):
            pass
        sc.ValueSortedDict = ValueSortedDict
        sys.modules["sortedcollections"] = sc
        for pkg in ("pyannote", "pyannote.video", "pyannote.video.face", "pyannote.algorithms", "pyannote.algorithms.clustering",
                    "pyannote.algorithms.clustering.hac"):
            m = types.ModuleType(pkg)
            m.__path__ = []
            sys.modules[pkg] = m
        core = types.ModuleType("pyannote.core")
        core.Segment, core.Annotation = segment_cls, annotation_cls
        sys.modules["pyannote.core"] = core

        class HACModel(object):
            def __init__(self, is_symmetric=False):
                self.is_symmetric = is_symmetric
                self._models = {}

            def __getitem__(self, cluster):
                return self._models[cluster]

        class HierarchicalAgglomerativeClustering(object):
            def __init__(self, model, stopping_criterion=None, constraint=None, logger=None):
                self.model, self.stopping_criterion, self.constraint = model, stopping_criterion, constraint

        class DistanceThreshold(object):
            def __init__(self, threshold=1.0, force=False):
                self.threshold, self.force = threshold, force
        hac = sys.modules["pyannote.algorithms.clustering.hac"]
        hac.HierarchicalAgglomerativeClustering = HierarchicalAgglomerativeClustering
        model = types.ModuleType("pyannote.algorithms.clustering.hac.model")
        model.HACModel = HACModel
        stop = types.ModuleType("pyannote.algorithms.clustering.hac.stop")
        stop.DistanceThreshold = DistanceThreshold
        sys.modules["pyannote.algorithms.clustering.hac.model"] = model
        sys.modules["pyannote.algorithms.clustering.hac.stop"] = stop
        yield _load("pyannote.video.face.clustering", os.path.join(REFERENCE, "pyannote", "video", "face", "clustering.py"))
    finally:
        if not had_iteritems:
            del pandas.Series.iteritems
        for k in list(sys.modules):
            if k not in saved:
                del sys.modules[k]
        sys.modules.update(saved)
