"""`Context`: one GPU, one HIP stream, the loaded models and the frames staged in HBM.  Thin Python over the C ABI."""
import contextlib
import ctypes as C
import threading
import itertools
import operator
import numpy as np
from . import _lib
from ._lib import check, ptr, handles
from . import models as _models
from .y4m import YuvFrame, chroma_shape


class DeviceFrame(object):
    """A frame resident in HBM (uint8 RGB HWC).  `keep` pins whatever owns the memory (e.g. a torch tensor)."""
    __slots__ = ("ctx", "handle", "height", "width", "keep", "transient", "__weakref__")

    def __init__(self, ctx, handle, height, width, keep=None, transient=False):
        self.ctx, self.handle, self.height, self.width, self.keep = ctx, handle, height, width, keep
        self.transient = transient      # a streaming source made it for one pass: the engine releases it when `extract` has passed it

    @property
    def shape(self):
        return (self.height, self.width, 3)

    def release(self):
        if self.handle is not None and self.ctx._h is not None:
            _lib.lib().pvf_frame_release(self.ctx._h, self.handle)
        self.handle = None
        self.keep = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class IngestRing(object):
    """Pinned host slots of one frame size + a copy stream (pvf_ingest_*).  `slot()` hands out the next slot as a numpy view for the
    decoder to write into; `submit()` queues its upload and returns a DeviceFrame at once -- kernels that read the frame wait for
    the copy on the device, so uploads run beside the compute stream."""

    def __init__(self, ctx, height, width, depth=8):
        self.ctx, self.h, self.w, self.depth = ctx, int(height), int(width), int(depth)
        r = C.c_uint64(0)
        check(ctx._l.pvf_ingest_create(ctx._h, self.h, self.w, self.depth, C.byref(r)))
        self._r = r.value
        self._cur = None

    def slot(self):
        s, p = C.c_int32(0), C.c_void_p(0)
        check(self.ctx._l.pvf_ingest_acquire(self.ctx._h, self._r, C.byref(s), C.byref(p)))
        self._cur = s.value
        buf = (C.c_uint8 * (self.h * self.w * 3)).from_address(p.value)
        return np.frombuffer(buf, np.uint8).reshape(self.h, self.w, 3)

    def submit(self):
        h = C.c_uint64(0)
        check(self.ctx._l.pvf_ingest_submit(self.ctx._h, self._r, self._cur, C.byref(h)))
        return DeviceFrame(self.ctx, h.value, self.h, self.w)

    def wait(self):
        check(self.ctx._l.pvf_ingest_wait(self.ctx._h, self._r))

    def push(self, rgb):
        """copy a decoded frame into the next slot and queue its upload (a decoder would write into slot() directly)"""
        np.copyto(self.slot(), rgb)
        return self.submit()

    def close(self):
        if self._r is not None and self.ctx._h is not None:
            self.ctx._l.pvf_ingest_destroy(self.ctx._h, self._r)
        self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_YUV_LAYOUTS = {"420": 420, "422": 422, "444": 444}


def _yuv_flags(matrix, full_range):
    if str(matrix) not in ("601", "709"):
        raise ValueError("matrix must be '601' or '709', not %r" % (matrix,))
    return (1 if str(matrix) == "709" else 0) | (2 if full_range else 0)       # PVF_YUV_BT709, PVF_YUV_FULL_RANGE


def _yuv_layout(layout):
    if str(layout) not in _YUV_LAYOUTS:
        raise ValueError("layout must be '420', '422' or '444', not %r" % (layout,))
    return _YUV_LAYOUTS[str(layout)]


class YuvIngestRing(IngestRing):
    """An ingest ring whose pinned slots hold the planes a decoder writes (pvf_ingest_create_yuv): `slot()` hands out the (Y, U, V) views
    of the next slot, `submit()` queues one copy of the planes and the conversion kernel on the copy stream and returns the RGB
    DeviceFrame at once.  4:2:0 crosses PCIe with half the bytes of RGB."""

    def __init__(self, ctx, height, width, layout="420", matrix="601", full_range=False, depth=8):
        self.ctx, self.h, self.w, self.depth = ctx, int(height), int(width), int(depth)
        self.layout, self.matrix, self.full_range = str(layout), str(matrix), bool(full_range)
        self._r = None
        code, flags = _yuv_layout(layout), _yuv_flags(matrix, full_range)
        r = C.c_uint64(0)
        check(ctx._l.pvf_ingest_create_yuv(ctx._h, self.h, self.w, self.depth, code, flags, C.byref(r)))
        self._r = r.value
        self._cur = None
        self._ch, self._cw = chroma_shape(self.h, self.w, self.layout)

    def slot(self):
        s, p = C.c_int32(0), C.c_void_p(0)
        check(self.ctx._l.pvf_ingest_acquire(self.ctx._h, self._r, C.byref(s), C.byref(p)))
        self._cur = s.value
        ny, nc = self.h * self.w, self._ch * self._cw
        a = np.frombuffer((C.c_uint8 * (ny + 2 * nc)).from_address(p.value), np.uint8)
        return (a[:ny].reshape(self.h, self.w), a[ny:ny + nc].reshape(self._ch, self._cw), a[ny + nc:].reshape(self._ch, self._cw))

    def push(self, frame):
        """copy a YuvFrame's planes into the next slot and queue upload + conversion"""
        if (frame.height, frame.width, frame.layout, frame.matrix, frame.full_range) != (self.h, self.w, self.layout, self.matrix, self.full_range):
            raise ValueError("this ring was made for %dx%d %s frames (matrix %s, %s range)" % (
                self.w, self.h, self.layout, self.matrix, "full" if self.full_range else "limited"))
        y, u, v = self.slot()
        np.copyto(y, frame.y)
        np.copyto(u, frame.u)
        np.copyto(v, frame.v)
        return self.submit()


class EgressRing(object):
    """Pinned host slots of one planar YUV 4:2:0 output frame + a copy stream (pvf_egress_*): the way annotated frames leave the GPU,
    the mirror image of IngestRing.  `submit(frame, prims)` renders the next slot (resize, drawing and colour conversion in one kernel on
    the context's stream, the copy to the host queued behind it) and returns its number at once; `wait(slot)` blocks until the planes
    are in host memory and returns them as a numpy view; `release(slot)` gives the slot back.  At most `depth` frames are in flight:
    submit raises when the next slot has not been given back.  wait / release may run in another thread than submit."""

    def __init__(self, ctx, width, height, matrix="601", full_range=False, depth=8):
        self.ctx, self.w, self.h, self.depth = ctx, int(width), int(height), int(depth)
        self.matrix, self.full_range = str(matrix), bool(full_range)
        self._r = None
        r = C.c_uint64(0)
        check(ctx._l.pvf_egress_create(ctx._h, self.w, self.h, self.depth, _yuv_flags(matrix, full_range), C.byref(r)))
        self._r = r.value
        self.frame_bytes = self.w * self.h + 2 * ((self.w + 1) // 2) * ((self.h + 1) // 2)

    def submit(self, frame, prims=()):
        """frame: a DeviceFrame (or anything Context.stage takes); prims: one frame's primitive list (render.py)"""
        from . import render as _render
        _, p, text = _render.pack_primitives([prims])
        s = C.c_int32(0)
        check(self.ctx._l.pvf_egress_submit(self.ctx._h, self._r, self.ctx.stage(frame).handle, ptr(p), len(p), ptr(text), len(text), C.byref(s)))
        return s.value

    def wait(self, slot):
        p = C.c_void_p(0)
        check(self.ctx._l.pvf_egress_wait(self.ctx._h, self._r, int(slot), C.byref(p)))
        return np.frombuffer((C.c_uint8 * self.frame_bytes).from_address(p.value), np.uint8)

    def release(self, slot):
        check(self.ctx._l.pvf_egress_release(self.ctx._h, self._r, int(slot)))

    def close(self):
        if self._r is not None and self.ctx._h is not None:
            self.ctx._l.pvf_egress_destroy(self.ctx._h, self._r)
        self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostFrameStager(object):
    """What a reader thread does with the frames a video yields: numpy RGB frames go through a pinned RGB ring, YuvFrames through a YUV
    ring (made when the first such frame arrives, remade when the geometry changes); anything else -- a DeviceFrame -- is passed on
    as it is.  stage(frame) -> (frame for the engine, True if this object made it and the consumer has to release it)."""

    def __init__(self, ctx, depth):
        self.ctx, self.depth = ctx, int(depth)
        self._ring, self._key = None, None

    def stage(self, frame):
        if isinstance(frame, YuvFrame):
            key = ("yuv",) + frame.key
        elif isinstance(frame, np.ndarray):
            key = ("rgb",) + tuple(frame.shape[:2])
        else:
            return frame, False
        if key != self._key:
            self.close()
            if key[0] == "yuv":
                self._ring = self.ctx.ingest_ring_yuv(frame.height, frame.width, layout=frame.layout, matrix=frame.matrix,
                                                      full_range=frame.full_range, depth=self.depth)
            else:
                self._ring = self.ctx.ingest_ring(frame.shape[0], frame.shape[1], depth=self.depth)
            self._key = key
        return self._ring.push(frame), True

    def close(self):
        """waits for the last uploads"""
        if self._ring is not None:
            self._ring.close()
        self._ring, self._key = None, None


def _boxes_and_scores(out, scores, counts):
    """[( [(l, t, r, b) Python ints], float32 scores )] per frame.  One tolist() for the whole batch: indexing numpy rows element by
    element cost 3 ms per 250-frame shot, during which the GPU had nothing queued."""
    cnt = counts.tolist()
    rows = out[:, :max(cnt, default=0)].tolist()           # only the filled slots
    return [([tuple(b) for b in rows[i][:cnt[i]]], scores[i, :cnt[i]].copy()) for i in range(len(cnt))]


class DeviceRows(object):
    """rows in device memory handed to the library by address: n rows, `stride` bytes apart; `keep` = whatever owns the memory
    (a torch tensor, a buffer of another library), kept alive as long as this object"""

    def __init__(self, ptr, n, stride, keep=None):
        self.ptr, self.n, self.stride, self.keep = int(ptr), int(n), int(stride), keep

    @classmethod
    def of_tensor(cls, t):
        """a 2-D contiguous torch tensor on the device"""
        assert t.dim() == 2 and t.is_contiguous()
        return cls(t.data_ptr(), t.shape[0], t.shape[1] * t.element_size(), keep=t)


_handle_of = operator.attrgetter("handle")


def _rects(boxes, n):
    """pvf_rect_i32[n] from n boxes: int() of each coordinate.  Lists of integer 4-tuples (what `extract` hands over, thousands per call)
    go through one iterator pass -- a quarter of the time numpy takes to parse a list of tuples, on a thread the GPU is waiting for."""
    if not isinstance(boxes, np.ndarray):
        try:
            r = np.fromiter(itertools.chain.from_iterable(boxes), dtype=np.int64)
            if r.size == 4 * n:
                return r.astype(np.int32).reshape(n, 4)
        except (TypeError, ValueError):
            pass                                            # floats, arrays, ragged input: the general form below decides
    return np.ascontiguousarray(np.asarray(boxes).astype(np.int64).astype(np.int32)).reshape(n, 4)


class Context(object):
    _stage_mu = threading.RLock()      # (instances make their own in __init__; this one serves objects built without it, e.g. test doubles)

    def __init__(self, device=0, detector=_models.DEFAULT_DETECTOR, landmarks=None, embedding=None, priority=0):
        self._h = None
        l = _lib.lib()
        h = C.c_uint64(0)
        check(l.pvf_ctx_create_prio(int(device), int(priority), C.byref(h)))
        self._h = h.value
        self.device = int(device)
        self._l = l
        self._staged = {}      # (id, data ptr) -> DeviceFrame for numpy frames passed through the dlib-like API
        self._staged_order = []
        self.stage_capacity = 1024
        self._hold = 0         # > 0 while a call is collecting frame handles: nothing staged may be evicted until it has run
        self._stage_mu = threading.RLock()   # the staging cache is used from the detector thread and the tracker / extraction threads
        self._tables = False
        self._models = {}
        self._yuv_rings = {}   # YuvFrame.key -> YuvIngestRing of upload(): made on first use, closed with the context
        if detector:
            self.load_detector(detector)
        if landmarks:
            self.load_shape_predictor(landmarks)
        if embedding:
            self.load_embedder(embedding)

    def close(self):
        if self._h is not None:
            for f in list(self._staged.values()):
                f.release()
            self._staged.clear()
            for r in self.__dict__.pop("_yuv_rings", {}).values():
                r.close()
            self._l.pvf_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self._l.pvf_sync(self._h))

    # ---- models
    def load_detector(self, path):
        check(self._l.pvf_load_detector(self._h, str(path).encode()))

    def _model_key(self, path):
        import os
        try:
            st = os.stat(str(path))
        except OSError:
            return object()          # never equal: the loader reports the missing file
        return (os.path.abspath(str(path)), st.st_size, st.st_mtime_ns)

    def load_shape_predictor(self, path):
        """(a model file that is already loaded -- same path, size and modification time -- is not read again: every CLI verb and
        every FacePipeline names its models)"""
        key = self._model_key(path)
        if self._models.get("sp") != key:
            check(self._l.pvf_load_shape_predictor(self._h, str(path).encode()))
            self._models["sp"] = key

    def load_embedder(self, path):
        key = self._model_key(path)
        if self._models.get("emb") != key:
            check(self._l.pvf_load_embedder(self._h, str(path).encode()))
            self._models["emb"] = key

    def ensure_tracker_tables(self):
        if not self._tables:
            t = _models.dsst_tables()
            self._tab_keep = t
            check(self._l.pvf_set_tracker_tables(self._h, ptr(t["mask64"]), ptr(t["mask_scale"]), ptr(t["tw64"]), ptr(t["tw32"]),
                                                 t["alpha_pow_m16"], t["ln_alpha"]))
            self._tables = True

    # ---- frames
    def upload(self, rgb):
        """a host frame to HBM: a numpy RGB frame as it is, a YuvFrame (y4m.py) through a small YUV ring and the conversion kernel"""
        if isinstance(rgb, YuvFrame):
            with self._stage_mu:
                ring = self._yuv_rings.get(rgb.key)
                if ring is None:
                    ring = self._yuv_rings[rgb.key] = self.ingest_ring_yuv(rgb.height, rgb.width, rgb.layout, rgb.matrix, rgb.full_range, depth=4)
                return ring.push(rgb)
        rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
            raise TypeError("frames must be uint8 arrays of shape (H, W, 3)")   # dlib raises on unsupported arrays too
        if not rgb.flags["C_CONTIGUOUS"]:
            rgb = np.ascontiguousarray(rgb)
        h = C.c_uint64(0)
        check(self._l.pvf_frame_upload(self._h, ptr(rgb), rgb.shape[0], rgb.shape[1], rgb.strides[0], C.byref(h)))
        return DeviceFrame(self, h.value, rgb.shape[0], rgb.shape[1])

    def upload_device(self, data_ptr, height, width, transient=False):
        """copy of a frame that already lies in HBM (a decoder's output surface) into a buffer of the library's own"""
        h = C.c_uint64(0)
        check(self._l.pvf_frame_upload(self._h, C.c_void_p(int(data_ptr)), int(height), int(width), int(width) * 3, C.byref(h)))
        return DeviceFrame(self, h.value, int(height), int(width), transient=transient)

    def mem_info(self):
        """(free, total) bytes of device memory as the driver sees them"""
        f, t = C.c_int64(0), C.c_int64(0)
        check(self._l.pvf_mem_info(self._h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def pool_trim(self, keep_bytes=0):
        """give pooled frame buffers beyond keep_bytes back to the allocator; returns what the pool still holds"""
        n = C.c_int64(0)
        check(self._l.pvf_frame_pool_trim(self._h, int(keep_bytes), C.byref(n)))
        return n.value

    def wrap_device(self, data_ptr, height, width, keep=None):
        h = C.c_uint64(0)
        check(self._l.pvf_frame_wrap_device(self._h, C.c_void_p(int(data_ptr)), int(height), int(width), C.byref(h)))
        return DeviceFrame(self, h.value, int(height), int(width), keep)

    def share(self, frame):
        """DeviceFrame of THIS context for a frame staged in another context on the same GPU (no copy)"""
        if frame.ctx is self:
            return frame
        p = C.c_void_p(0)
        check(self._l.pvf_frame_device_ptr(frame.ctx._h, frame.handle, C.byref(p)))
        return self.wrap_device(p.value, frame.height, frame.width, keep=frame)

    def wrap_torch(self, t):
        """t: torch.uint8 CUDA tensor [H, W, 3], contiguous"""
        assert t.is_cuda and t.is_contiguous() and t.dim() == 3 and t.shape[2] == 3 and t.element_size() == 1
        return self.wrap_device(t.data_ptr(), t.shape[0], t.shape[1], keep=t)

    def resize(self, frame, width, height):
        """cv2.resize(frame, (width, height)) on the device (reference video.py:402-403): a new DeviceFrame; the source stays resident"""
        f = self.stage(frame)
        h = C.c_uint64(0)
        check(self._l.pvf_frame_resize(self._h, f.handle, int(width), int(height), C.byref(h)))
        return DeviceFrame(self, h.value, int(height), int(width))

    def ingest_ring(self, height, width, depth=8):
        return IngestRing(self, height, width, depth)

    def ingest_ring_yuv(self, height, width, layout="420", matrix="601", full_range=False, depth=8):
        return YuvIngestRing(self, height, width, layout, matrix, full_range, depth)

    def egress_ring(self, width, height, matrix="601", full_range=False, depth=8):
        return EgressRing(self, width, height, matrix, full_range, depth)

    def render(self, frames, prims, width, height, matrix="601", full_range=False, out_ptr=None):
        """the `demo` picture of n resident frames of one size (pvf_render_batch): resized to (width, height), frame i drawn over with
        prims[i] (render.py primitive lists, redactions included; None: nothing is drawn), converted to planar YUV 4:2:0.  Returns uint8 [n, frame bytes]
        (Y, U, V tight per frame); with out_ptr, a device address that holds as much, the planes stay in HBM and nothing is returned.
        prims may also be the packed (start, prims, text) arrays of render.pack_primitives."""
        from . import render as _render
        n = len(frames)
        if prims is None:
            start, p, text = None, None, np.zeros(0, np.uint8)
        elif isinstance(prims, tuple) and len(prims) == 3 and isinstance(prims[0], np.ndarray):
            start, p, text = prims
        else:
            if len(prims) != n:
                raise ValueError("%d primitive lists for %d frames" % (len(prims), n))
            start, p, text = _render.pack_primitives(prims)
        fb = int(width) * int(height) + 2 * ((int(width) + 1) // 2) * ((int(height) + 1) // 2)
        out = None if out_ptr is not None else np.empty((n, fb), np.uint8)
        with self._staging():
            hs = self._handles(frames)
            check(self._l.pvf_render_batch(self._h, ptr(hs), n, int(width), int(height), _yuv_flags(matrix, full_range), ptr(start), ptr(p),
                                           ptr(text), len(text), C.c_void_p(int(out_ptr)) if out_ptr is not None else ptr(out),
                                           1 if out_ptr is not None else 0))
        return out

    def render_rgb(self, frame, prims, width, height):
        """the drawn picture before colour conversion, uint8 [height, width, 3] (pvf_debug_render_rgb)"""
        from . import render as _render
        _, p, text = _render.pack_primitives([prims])
        out = np.empty((int(height), int(width), 3), np.uint8)
        check(self._l.pvf_debug_render_rgb(self._h, self.stage(frame).handle, int(width), int(height), ptr(p), len(p), ptr(text), len(text),
                                           ptr(out)))
        return out

    def redact_means(self, frame, prims, width, height):
        """the cell means the list's redactions are drawn from, uint8 [cells, 3]: the tables of its mosaic and smooth redactions in list
        order, a table's cells row-major (pvf_debug_redact_means).  Tells the reduction from the composition."""
        from . import render as _render
        _, p, _ = _render.pack_primitives([[q for q in prims if q[0] == _render.PRIM_REDACT]])
        n = sum(_render.redaction_cells(q) for q in prims if q[0] == _render.PRIM_REDACT)
        out = np.empty((n, 3), np.uint8)
        check(self._l.pvf_debug_redact_means(self._h, self.stage(frame).handle, int(width), int(height), ptr(p), len(p), ptr(out), out.nbytes))
        return out

    def frame_from_yuv_device(self, y_ptr, y_pitch, u_ptr, v_ptr, c_pitch, height, width, layout="420", matrix="601", full_range=False,
                              c_step=1):
        """RGB DeviceFrame from planes that already lie in HBM (a hardware decoder's surface): pitches in bytes, c_step 2 for
        interleaved chroma (NV12: v_ptr = u_ptr + 1).  The planes have been read when the call returns."""
        h = C.c_uint64(0)
        check(self._l.pvf_frame_from_yuv(self._h, C.c_void_p(int(y_ptr)), int(y_pitch), C.c_void_p(int(u_ptr)), C.c_void_p(int(v_ptr)),
                                         int(c_pitch), int(c_step), int(height), int(width), _yuv_layout(layout),
                                         _yuv_flags(matrix, full_range), C.byref(h)))
        return DeviceFrame(self, h.value, int(height), int(width))

    def frame_from_yuv_torch(self, y, u, v=None, layout="420", matrix="601", full_range=False):
        """y: torch.uint8 CUDA tensor [H, W]; u, v: the chroma planes [CH, CW], or u = interleaved [CH, CW, 2] and v = None (NV12).
        Rows may be strided (a view of a pitched surface); the samples of a row are contiguous.  The caller makes sure the tensors
        are written (torch.cuda.synchronize or a stream wait) before the call."""
        for t in (y, u) + (() if v is None else (v,)):
            assert t.is_cuda and t.element_size() == 1 and t.stride(-1) == 1
        if v is None:
            assert u.dim() == 3 and u.shape[2] == 2 and (u.shape[1] == 1 or u.stride(1) == 2)
            return self.frame_from_yuv_device(y.data_ptr(), y.stride(0), u.data_ptr(), u.data_ptr() + 1, u.stride(0), y.shape[0], y.shape[1],
                                              layout, matrix, full_range, c_step=2)
        assert u.dim() == 2 and v.dim() == 2 and u.shape == v.shape and u.stride(0) == v.stride(0)
        return self.frame_from_yuv_device(y.data_ptr(), y.stride(0), u.data_ptr(), v.data_ptr(), u.stride(0), y.shape[0], y.shape[1],
                                          layout, matrix, full_range)

    def stage(self, rgb):
        """DeviceFrame for whatever the caller holds: DeviceFrame (as is) or numpy array (uploaded once, cached by identity)."""
        if isinstance(rgb, DeviceFrame):
            return rgb
        key = (id(rgb), rgb.__array_interface__["data"][0] if hasattr(rgb, "__array_interface__") else 0)
        with self._stage_mu:
            f = self._staged.get(key)
            if f is None or f.keep is not rgb:
                f = self.upload(rgb)
                f.keep = rgb   # keeps the id stable while cached
                self._staged[key] = f
                self._staged_order.append(key)
                if not self._hold:
                    self._trim()
            return f

    def _trim(self):
        with self._stage_mu:
            while len(self._staged_order) > self.stage_capacity:
                old = self._staged_order.pop(0)
                g = self._staged.pop(old, None)
                if g is not None:
                    g.release()

    @contextlib.contextmanager
    def _staging(self):
        """Frames staged inside the block stay resident until the block ends: one call may reference more distinct numpy
        frames than the cache holds (a 4096-tracker batch of a long shot), and a handle released before the C call runs is
        an 'unknown frame handle'.  The cache is trimmed back to its capacity afterwards."""
        with self._stage_mu:
            self._hold += 1
        try:
            yield
        finally:
            with self._stage_mu:
                self._hold -= 1
                if not self._hold:
                    self._trim()

    def _handles(self, frames):
        if isinstance(frames, np.ndarray) and frames.dtype == np.uint64:     # handles the caller looked up before (frame_handles)
            return np.ascontiguousarray(frames)
        try:                                                # frames already on the device (the engine's case): one pass at C speed
            return np.fromiter(map(_handle_of, frames), dtype=np.uint64, count=len(frames))
        except AttributeError:
            return handles([self.stage(f).handle for f in frames])

    def frame_handles(self, frames):
        """uint64 array of the staged frames' handles: look them up once, index the array for every batched call"""
        return self._handles(frames)

    def unstage_all(self):
        for f in self._staged.values():
            f.release()
        self._staged.clear()
        self._staged_order = []

    # ---- S1
    def detect_batch(self, frames, upsample=1, adjust_threshold=0.0, cap=256):
        n = len(frames)
        out = np.zeros((n, cap, 4), np.int32)
        scores = np.zeros((n, cap), np.float32)
        counts = np.zeros(n, np.int32)
        with self._staging():
            hs = self._handles(frames)
            check(self._l.pvf_detect_batch(self._h, ptr(hs), n, int(upsample), float(adjust_threshold), ptr(out), ptr(scores), ptr(counts), cap))
        if int(counts.max(initial=0)) >= cap:     # a frame filled its slots: repeat with room for every detection (like detect_many)
            return self.detect_batch(frames, upsample, adjust_threshold, cap * 8)
        return _boxes_and_scores(out, scores, counts)

    def detect_many(self, frames, batch, upsample=1, adjust_threshold=0.0, cap=64, arrays=False):
        """any number of frames of one size, `batch` at a time, host post-processing overlapped with the next batch's kernels.
        arrays=True: (boxes int32 [n, slots, 4], scores float32 [n, slots], counts int32 [n]) instead of Python lists -- a caller that
        feeds the boxes straight back to the GPU converts them to Python objects when (and where) it has the time"""
        n = len(frames)
        out = np.zeros((n, cap, 4), np.int32)
        scores = np.zeros((n, cap), np.float32)
        counts = np.zeros(n, np.int32)
        with self._staging():
            hs = self._handles(frames)
            check(self._l.pvf_detect_many(self._h, ptr(hs), n, int(batch), int(upsample), float(adjust_threshold), ptr(out), ptr(scores), ptr(counts), cap))
        if int(counts.max(initial=0)) >= cap:     # a frame filled its slots: repeat with room for every detection
            return self.detect_many(frames, batch, upsample, adjust_threshold, cap * 8, arrays)
        if arrays:
            m = int(counts.max(initial=0))
            return out[:, :m], scores[:, :m], counts
        return _boxes_and_scores(out, scores, counts)

    def detect(self, frame, upsample=1, adjust_threshold=0.0):
        return self.detect_batch([frame], upsample, adjust_threshold)[0]

    def detect_raw(self, frame, upsample=1, adjust_threshold=0.0, cap=65536):
        f = self.stage(frame)
        scores = np.zeros(cap, np.float32)
        meta = np.zeros((cap, 8), np.int32)
        n = C.c_int32(0)
        check(self._l.pvf_debug_detect_raw(self._h, f.handle, int(upsample), float(adjust_threshold), ptr(scores), ptr(meta), cap, C.byref(n)))
        k = min(n.value, cap)
        return [(float(scores[i]), int(meta[i, 0]), int(meta[i, 1]), int(meta[i, 2]), int(meta[i, 3]),
                 tuple(int(v) for v in meta[i, 4:8])) for i in range(k)]

    def detect_raw_many(self, frames, batch, upsample=1, adjust_threshold=0.0, cap=1 << 16):
        """the scanner's candidates BEFORE non-maximum suppression through the batched path (screening pass included): per frame an int32
        [n, 5] table (level, filter, row, column, score bits) in the detector's canonical order"""
        n = len(frames)
        counts = np.zeros(n, np.int32)
        total = C.c_int64(0)
        with self._staging():
            hs = self._handles(frames)
            while True:
                rows = np.zeros((cap, 5), np.int32)
                check(self._l.pvf_debug_detect_raw_many(self._h, ptr(hs), n, int(batch), int(upsample), float(adjust_threshold), ptr(counts), ptr(rows), cap, C.byref(total)))
                if total.value <= cap:
                    break
                cap = int(total.value)
        off = np.concatenate([[0], np.cumsum(counts)])
        return [rows[off[i]:off[i + 1]] for i in range(n)]

    def pyramid_batch(self, frames, upsample=1):
        """the image pyramids of a batch and nothing else (measurement: the detector's resize chain alone)"""
        with self._staging():
            hs = self._handles(frames)
            check(self._l.pvf_debug_pyramid_batch(self._h, ptr(hs), len(frames), int(upsample)))

    def pyramid_level(self, frame, upsample, level):
        f = self.stage(frame)
        oh, ow = C.c_int32(0), C.c_int32(0)
        check(self._l.pvf_debug_pyramid_level(self._h, f.handle, upsample, level, None, C.byref(oh), C.byref(ow)))
        out = np.zeros((oh.value, ow.value, 3), np.uint8)
        check(self._l.pvf_debug_pyramid_level(self._h, f.handle, upsample, level, ptr(out), C.byref(oh), C.byref(ow)))
        return out

    def level_features(self, frame, upsample, level):
        """FHOG features [fh][fw][32] of one pyramid level as the batched detector computes them (parity tests)."""
        f = self.stage(frame)
        fh, fw = C.c_int32(0), C.c_int32(0)
        check(self._l.pvf_debug_level_features(self._h, f.handle, upsample, level, None, C.byref(fh), C.byref(fw)))
        out = np.zeros((fh.value, fw.value, 32), np.float32)
        if out.size:
            check(self._l.pvf_debug_level_features(self._h, f.handle, upsample, level, ptr(out), C.byref(fh), C.byref(fw)))
        return out

    def level_plan(self, frame, upsample, level):
        """how the plan of the frame's size cuts one pyramid level into pieces (tests of the plan knobs)"""
        f = self.stage(frame)
        out = np.zeros(8, np.int32)
        check(self._l.pvf_debug_level_plan(self._h, f.handle, int(upsample), int(level), ptr(out)))
        return dict(zip(("h", "w", "hog_nr", "hog_nc", "chunk_rows", "chunks", "roll_rows", "roll_nseg"), (int(v) for v in out)))

    def fhog(self, img, cell, pad_r, pad_c):
        img = np.ascontiguousarray(img, np.uint8)
        fh, fw = C.c_int32(0), C.c_int32(0)
        check(self._l.pvf_debug_fhog(self._h, ptr(img), img.shape[0], img.shape[1], cell, pad_r, pad_c, None, C.byref(fh), C.byref(fw)))
        out = np.zeros((fh.value, fw.value, 32), np.float32)
        check(self._l.pvf_debug_fhog(self._h, ptr(img), img.shape[0], img.shape[1], cell, pad_r, pad_c, ptr(out), C.byref(fh), C.byref(fw)))
        return out

    # ---- S2
    def tracker_create(self):
        self.ensure_tracker_tables()
        h = C.c_uint64(0)
        check(self._l.pvf_tracker_create(self._h, C.byref(h)))
        return h.value

    def tracker_create_many(self, n, as_array=False):
        self.ensure_tracker_tables()
        out = np.zeros(int(n), np.uint64)
        if n:
            check(self._l.pvf_tracker_create_many(self._h, int(n), ptr(out)))
        return out if as_array else out.tolist()

    def tracker_clone_many(self, trks, as_array=False):
        out = np.zeros(len(trks), np.uint64)
        if len(trks):
            check(self._l.pvf_tracker_clone_many(self._h, ptr(handles(trks)), len(trks), ptr(out)))
        return out if as_array else out.tolist()

    def tracker_destroy_many(self, trks):
        if self._h is not None and len(trks):
            check(self._l.pvf_tracker_destroy_many(self._h, ptr(handles(trks)), len(trks)))

    def tracker_destroy(self, trk):
        if self._h is not None:
            check(self._l.pvf_tracker_destroy(self._h, trk))

    def tracker_start_many(self, trks, frames, boxes):
        if not len(trks):
            return
        b = np.ascontiguousarray(boxes, np.float64).reshape(-1, 4)
        with self._staging():
            check(self._l.pvf_tracker_start_many(self._h, ptr(handles(trks)), ptr(self._handles(frames)), ptr(b), len(trks)))

    def tracker_update_many(self, trks, frames, defer=False):
        """defer=True: confidence and position only, the filter update is left to tracker_commit_many (same frames)"""
        n = len(trks)
        if not n:
            return np.zeros(0), np.zeros((0, 4))
        psr = np.zeros(n, np.float64)
        boxes = np.zeros((n, 4), np.float64)
        fn = self._l.pvf_tracker_update_many_deferred if defer else self._l.pvf_tracker_update_many
        with self._staging():
            check(fn(self._h, ptr(handles(trks)), ptr(self._handles(frames)), n, ptr(psr), ptr(boxes)))
        return psr, boxes

    def tracker_commit_many(self, trks, frames):
        n = len(trks)
        if n:
            with self._staging():
                check(self._l.pvf_tracker_commit_many(self._h, ptr(handles(trks)), ptr(self._handles(frames)), n))

    def tracker_position(self, trk):
        b = np.zeros(4, np.float64)
        check(self._l.pvf_tracker_position(self._h, trk, ptr(b)))
        return tuple(b.tolist())

    def tracker_state(self, trk):
        F = np.zeros((32, 64, 64, 2), np.float64)
        A = np.zeros((32, 64, 64, 2), np.float64)
        B = np.zeros((64, 64), np.float64)
        check(self._l.pvf_debug_tracker_state(self._h, trk, ptr(F), ptr(A), ptr(B)))
        return F, A, B

    def tracker_scale_state(self, trk):
        As = np.zeros((512, 32, 2), np.float64)
        Bs = np.zeros(32, np.float64)
        check(self._l.pvf_debug_tracker_scale_state(self._h, trk, ptr(As), ptr(Bs)))
        return As, Bs

    # ---- S4
    def landmarks(self, frames, boxes):
        n = len(boxes)
        pts = np.zeros((n, 68, 2), np.int32)
        if n == 0:
            return pts
        r = _rects(boxes, n)
        with self._staging():
            check(self._l.pvf_landmarks(self._h, ptr(self._handles(frames)), ptr(r), n, ptr(pts)))
        return pts

    def landmarks_shape(self, frames, boxes):
        """(int32 [n, 68, 2], float32 [n, 68, 2]): landmarks() and the float shape of the last cascade, in normalised box coordinates,
        that they are rounded from (pvf_debug_landmarks_shape)"""
        n = len(boxes)
        pts = np.zeros((n, 68, 2), np.int32)
        shape = np.zeros((n, 68, 2), np.float32)
        if n == 0:
            return pts, shape
        r = _rects(boxes, n)
        with self._staging():
            check(self._l.pvf_debug_landmarks_shape(self._h, ptr(self._handles(frames)), ptr(r), n, ptr(pts), ptr(shape)))
        return pts, shape

    def embed(self, frames, pts, num_jitters=0, seed=0):
        """descriptors of the faces; num_jitters > 1: dlib's compute_face_descriptor(img, shape, num_jitters) -- the fp32 mean over
        that many jittered chips per face (JITTER.md), a function of the face, num_jitters and the seed"""
        pts = np.ascontiguousarray(pts, np.int32).reshape(-1, 68, 2)
        n = len(pts)
        out = np.zeros((n, 128), np.float32)
        if n == 0:
            return out
        with self._staging():
            if num_jitters:
                check(self._l.pvf_embed_jitter(self._h, ptr(self._handles(frames)), ptr(pts), n, int(num_jitters), _seed64(seed), ptr(out)))
            else:
                check(self._l.pvf_embed(self._h, ptr(self._handles(frames)), ptr(pts), n, ptr(out)))
        return out

    def landmarks_embed(self, frames, boxes, num_jitters=0, seed=0):
        """landmarks() then embed() of the same faces in one library call: (int32 [n, 68, 2], float32 [n, 128])"""
        n = len(boxes)
        pts = np.zeros((n, 68, 2), np.int32)
        out = np.zeros((n, 128), np.float32)
        if n == 0:
            return pts, out
        r = _rects(boxes, n)
        with self._staging():
            if num_jitters:
                check(self._l.pvf_landmarks_embed_jitter(self._h, ptr(self._handles(frames)), ptr(r), n, int(num_jitters), _seed64(seed),
                                                         ptr(pts), ptr(out)))
            else:
                check(self._l.pvf_landmarks_embed(self._h, ptr(self._handles(frames)), ptr(r), n, ptr(pts), ptr(out)))
        return pts, out

    def face_chips(self, frames, pts):
        pts = np.ascontiguousarray(pts, np.int32).reshape(-1, 68, 2)
        n = len(pts)
        out = np.zeros((n, 150, 150, 3), np.uint8)
        with self._staging():
            check(self._l.pvf_face_chips(self._h, ptr(self._handles(frames)), ptr(pts), n, ptr(out)))
        return out

    # ---- the faces verb (FACES.md)
    def chip_quality(self, chips):
        """int64 [n, 5] = S1, S2, SY, ND, NB of uint8 [n, 150, 150, 3] chips (pvf_chip_quality): the sums faces.score reads"""
        chips = np.ascontiguousarray(chips, np.uint8).reshape(-1, 150, 150, 3)
        out = np.zeros((len(chips), 5), np.int64)
        check(self._l.pvf_chip_quality(self._h, ptr(chips), len(chips), ptr(out)))
        return out

    def face_quality(self, frames, pts):
        """the same five sums for faces given by frame and landmarks: the chips are made and reduced on the device (pvf_face_quality);
        needs no embedder"""
        pts = np.ascontiguousarray(pts, np.int32).reshape(-1, 68, 2)
        out = np.zeros((len(pts), 5), np.int64)
        with self._staging():
            check(self._l.pvf_face_quality(self._h, ptr(self._handles(frames)), ptr(pts), len(pts), ptr(out)))
        return out

    # ---- the talk verb (TALK.md)
    def chip_motion(self, chips, prev):
        """int32 [n, 8] = DM0, DMmin, kM, DC0, DCmin, kC, SM, NZ of uint8 [n, 150, 150, 3] chips (pvf_chip_motion); prev[i] is -1 or
        the index < i of the chip that chip i is compared with"""
        chips = np.ascontiguousarray(chips, np.uint8).reshape(-1, 150, 150, 3)
        prev = np.ascontiguousarray(prev, np.int32).reshape(-1)
        if len(prev) != len(chips):
            raise ValueError("chip_motion: one predecessor per chip")
        out = np.zeros((len(chips), 8), np.int32)
        check(self._l.pvf_chip_motion(self._h, ptr(chips), len(chips), ptr(prev), ptr(out)))
        return out

    def face_motion(self, frames, pts, prev):
        """the same eight values for faces given by frame and landmarks: the chips are made and reduced on the device
        (pvf_face_motion); needs no embedder"""
        pts = np.ascontiguousarray(pts, np.int32).reshape(-1, 68, 2)
        prev = np.ascontiguousarray(prev, np.int32).reshape(-1)
        if len(prev) != len(pts) or len(frames) != len(pts):
            raise ValueError("face_motion: one frame and one predecessor per face")
        out = np.zeros((len(pts), 8), np.int32)
        with self._staging():
            check(self._l.pvf_face_motion(self._h, ptr(self._handles(frames)), ptr(pts), len(pts), ptr(prev), ptr(out)))
        return out

    # ---- the tube verb (TUBE.md)
    def frame_crops(self, frames, windows, size, layout="rgb", matrix="601", full_range=False, out_ptr=None):
        """the windows (X0, Y0, L), in sixteenths of a pixel, of resident frames as size x size pictures (pvf_frame_crops): uint8
        [n, size, size, 3] for layout "rgb", [n, picture bytes] (Y, U, V tight) for "yuv420".  With out_ptr, a device address that holds
        as much, the pictures stay in HBM and nothing is returned."""
        return self._frame_pictures("frame_crops", self._l.pvf_frame_crops, 3, frames, windows, size, layout, matrix, full_range, out_ptr)

    def frame_warps(self, frames, windows, size, layout="rgb", matrix="601", full_range=False, out_ptr=None):
        """the oriented windows (CX, CY, BX, BY, K) of resident frames (TUBE.md "Oriented window", pvf_frame_warps) as size x size
        pictures: what frame_crops returns, through windows that need not be axis-aligned"""
        return self._frame_pictures("frame_warps", self._l.pvf_frame_warps, 5, frames, windows, size, layout, matrix, full_range, out_ptr)

    def _frame_pictures(self, name, call, per_window, frames, windows, size, layout, matrix, full_range, out_ptr):
        if str(layout) not in ("rgb", "yuv420"):
            raise ValueError("layout must be 'rgb' or 'yuv420', not %r" % (layout,))
        windows = np.ascontiguousarray(windows, np.int32).reshape(-1, per_window)
        n, size = len(windows), int(size)
        if len(frames) != n:
            raise ValueError("%s: one frame per window" % name)
        flags = _yuv_flags(matrix, full_range) | (4 if layout == "yuv420" else 0)      # PVF_CROP_YUV420
        shape = (n, size, size, 3) if layout == "rgb" else (n, size * size + 2 * ((size + 1) // 2) ** 2)
        out = None if out_ptr is not None else np.empty(shape if size > 0 else (n, 0), np.uint8)
        with self._staging():
            check(call(self._h, ptr(self._handles(frames)), ptr(windows), n, size, flags,
                       C.c_void_p(int(out_ptr)) if out_ptr is not None else ptr(out), 1 if out_ptr is not None else 0))
        return out

    @staticmethod
    def _sheet_args(n, xy, background, prims):
        from . import render as _render
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        if len(xy) != n:
            raise ValueError("%d tile corners for %d chips" % (len(xy), n))
        _, p, text = _render.pack_primitives([list(prims)])
        r, g, b = (int(v) for v in background)
        return xy, r | g << 8 | b << 16, p, text

    @staticmethod
    def _sheet_out(width, height):
        """the picture's memory, or None for a size the library refuses (it says why)"""
        w, h = int(width), int(height)
        return np.empty((h, w, 3), np.uint8) if 0 < w <= 16384 and 0 < h <= 16384 and w * h <= 1 << 26 else None

    def chip_sheet(self, chips, xy, S, width, height, background=(0, 0, 0), prims=()):
        """uint8 [height, width, 3]: the chips resampled to S x S at the corners xy (later over earlier), the primitives over them
        (pvf_chip_sheet; FACES.md "Sheet")"""
        chips = np.ascontiguousarray(chips, np.uint8).reshape(-1, 150, 150, 3)
        xy, bg, p, text = self._sheet_args(len(chips), xy, background, prims)
        out = self._sheet_out(width, height)
        check(self._l.pvf_chip_sheet(self._h, ptr(chips), len(chips), ptr(xy), int(S), int(width), int(height), bg, ptr(p), len(p), ptr(text),
                                     len(text), ptr(out)))
        return out

    def face_sheet(self, frames, pts, xy, S, width, height, background=(0, 0, 0), prims=()):
        """chip_sheet with the chips made on the device from frames and landmarks (pvf_face_sheet)"""
        pts = np.ascontiguousarray(pts, np.int32).reshape(-1, 68, 2)
        xy, bg, p, text = self._sheet_args(len(pts), xy, background, prims)
        out = self._sheet_out(width, height)
        with self._staging():
            check(self._l.pvf_face_sheet(self._h, ptr(self._handles(frames)), ptr(pts), len(pts), ptr(xy), int(S), int(width), int(height), bg,
                                         ptr(p), len(p), ptr(text), len(text), ptr(out)))
        return out

    # ---- the storyboard verb (STORYBOARD.md)
    def frame_thumbs(self, frames, tw, th, out_ptr=None):
        """resident frames of one size, whole, as tw x th pictures (pvf_frame_thumbs: the exact area average): uint8 [n, th, tw, 3].
        With out_ptr, a device address that holds as much, the pictures stay in HBM and nothing is returned."""
        n, tw, th = len(frames), int(tw), int(th)
        out = None if out_ptr is not None else np.empty((n, th, tw, 3) if 0 < tw <= 1024 and 0 < th <= 1024 else (n, 0), np.uint8)
        with self._staging():
            check(self._l.pvf_frame_thumbs(self._h, ptr(self._handles(frames)), n, tw, th, 0,
                                           C.c_void_p(int(out_ptr)) if out_ptr is not None else ptr(out), 1 if out_ptr is not None else 0))
        return out

    def thumb_sheet(self, thumbs, xy, width, height, background=(0, 0, 0), prims=()):
        """uint8 [height, width, 3]: the thumbnails uint8 [n, th, tw, 3] copied to the corners xy (later over earlier), the primitives
        over them (pvf_thumb_sheet; STORYBOARD.md "Sheet")"""
        thumbs = np.ascontiguousarray(thumbs, np.uint8)
        if thumbs.ndim != 4 or thumbs.shape[3] != 3:
            raise ValueError("thumbnails are uint8 [n, th, tw, 3]")
        xy, bg, p, text = self._sheet_args(len(thumbs), xy, background, prims)
        out = self._sheet_out(width, height)
        check(self._l.pvf_thumb_sheet(self._h, ptr(thumbs), len(thumbs), ptr(xy), int(thumbs.shape[2]), int(thumbs.shape[1]), int(width),
                                      int(height), bg, ptr(p), len(p), ptr(text), len(text), ptr(out)))
        return out

    def embed_chips(self, chips, num_jitters=0, seed=0):
        chips = np.ascontiguousarray(chips, np.uint8).reshape(-1, 150, 150, 3)
        out = np.zeros((len(chips), 128), np.float32)
        if num_jitters:
            check(self._l.pvf_embed_chips_jitter(self._h, ptr(chips), len(chips), int(num_jitters), _seed64(seed), ptr(out)))
        else:
            check(self._l.pvf_embed_chips(self._h, ptr(chips), len(chips), ptr(out)))
        return out

    def jitter_chips(self, chips, J, seed=0, via_transform=False, copy_out=True):
        """the J jittered copies of every chip, uint8 [n, J, 150, 150, 3] (pvf_debug_jitter_chips; JITTER.md).  via_transform: the
        measurement switch of tools/bench_jitter.py -- transform_k over n * J jobs, mirrored jitters left unmirrored; with copy_out off
        the kernels run and nothing comes back (None)"""
        chips = np.ascontiguousarray(chips, np.uint8).reshape(-1, 150, 150, 3)
        out = np.zeros((len(chips), max(int(J), 0), 150, 150, 3), np.uint8) if copy_out or not via_transform else None
        fn = self._l.pvf_debug_jitter_chips_transform if via_transform else self._l.pvf_debug_jitter_chips
        check(fn(self._h, ptr(chips), len(chips), int(J), _seed64(seed), ptr(out)))
        return out

    def extract_chip(self, frame, rect, cs, sn, rows, cols):
        f = self.stage(frame)
        r = np.asarray(rect, np.float64)
        out = np.zeros((rows, cols, 3), np.uint8)
        check(self._l.pvf_debug_extract_chip(self._h, f.handle, ptr(r), float(cs), float(sn), rows, cols, ptr(out)))
        return out

    EMBED_STAGES = 30

    def embed_stage(self, chips, stage, split):
        """the embedder's activation after `stage` (0 first layer, 1 max-pool, 2 + 2u / 3 + 2u the `a` layer / the output of unit u),
        float32 [n, H, W, C], and the per-face range flags of a split run (int32 [n]; zeros without split)"""
        chips = np.ascontiguousarray(chips, np.uint8).reshape(-1, 150, 150, 3)
        n = len(chips)
        dims = np.zeros(3, np.int32)
        check(self._l.pvf_debug_embed_stage(self._h, None, n, 1 if split else 0, int(stage), None, ptr(dims), None))
        out = np.zeros((n,) + tuple(int(d) for d in dims), np.float32)
        flags = np.zeros(n, np.int32)
        check(self._l.pvf_debug_embed_stage(self._h, ptr(chips), n, 1 if split else 0, int(stage), ptr(out), ptr(dims), ptr(flags)))
        return out, flags

    def debug_conv(self, x, w, bias, gamma, beta, stride=1, pad=1, skip=None, skip_mode=0, out_hw=None, split=False, force_generic=False):
        """one convolution layer through the embedder's launcher: x [B, H, W, Cin], w [Cout, Cin, k, k]; skip_mode 1: skip
        [B, OH, OW, Cout]; 2: skip [B, XH, XW, XC], averaged 2 x 2 and zero-extended.  out_hw: the output map (default: the larger of
        the convolution's and the averaged skip's).  Returns (float32 [B, OH, OW, Cout], flags int32 [B])."""
        x = np.ascontiguousarray(x, np.float32)
        w = np.ascontiguousarray(w, np.float32)
        B, H, W, cin = x.shape
        cout, wc, k, k2 = w.shape
        if wc != cin or k != k2:
            raise ValueError("debug_conv: weights do not fit the input")
        ah, aw = 1 + (H + 2 * pad - k) // stride, 1 + (W + 2 * pad - k) // stride
        xh = xw = xc = sh = sw = 0
        if skip is not None:
            skip = np.ascontiguousarray(skip, np.float32)
        if skip_mode == 2:
            _, xh, xw, xc = skip.shape
            sh, sw = xh // 2, xw // 2
        oh, ow = out_hw if out_hw is not None else (max(ah, sh), max(aw, sw))
        if skip_mode == 1 and skip.shape != (B, oh, ow, cout):
            raise ValueError("debug_conv: the skip tensor must have the output's shape")
        if skip_mode == 2 and skip.shape[0] != B:
            raise ValueError("debug_conv: one skip map per face")
        par = [np.ascontiguousarray(v, np.float32).reshape(-1) for v in (bias, gamma, beta)]
        if any(v.size != cout for v in par):
            raise ValueError("debug_conv: bias, gamma and beta have one value per output channel")
        geom = np.array([B, H, W, cin, oh, ow, cout, ah, aw, k, stride, pad, skip_mode, xh, xw, xc, sh, sw], np.int32)
        out = np.zeros((B, max(oh, 0), max(ow, 0), cout), np.float32)
        flags = np.zeros(B, np.int32)
        check(self._l.pvf_debug_conv(self._h, ptr(geom), ptr(x), ptr(w), ptr(par[0]), ptr(par[1]), ptr(par[2]),
                                     ptr(skip) if skip is not None else None, 1 if split else 0, 1 if force_generic else 0, ptr(out), ptr(flags)))
        return out, flags

    def embed_head(self, x):
        """head_k (average over the map, 256 -> 128 product with the loaded model's matrix): x [n, HW, 256] -> float32 [n, 128]"""
        x = np.ascontiguousarray(x, np.float32)
        n, hw, ch = x.shape
        if ch != 256:
            raise ValueError("embed_head: 256 channels")
        out = np.zeros((n, 128), np.float32)
        check(self._l.pvf_debug_embed_head(self._h, ptr(x), n, hw, ptr(out)))
        return out

    def scratch(self, fill=None, state=False):
        """{arena: capacity in bytes} of the context's scratch arenas (pvf_debug_scratch).  fill = 0..255: first set every byte of every
        arena that holds no state across calls to that value (tests: what a call finds under its layout is then another family's
        leftovers, not a fresh allocation's zeros).  state=True: (sizes, the set of arenas that hold state and are never filled)."""
        need = C.c_int64(0)
        check(self._l.pvf_debug_scratch(self._h, -1 if fill is None else int(fill), None, 0, C.byref(need)))
        while True:
            buf = np.zeros(need.value, np.uint8)
            check(self._l.pvf_debug_scratch(self._h, -1, ptr(buf), buf.nbytes, C.byref(need)))
            if need.value <= buf.nbytes:
                break
        sizes, held = {}, set()
        for line in buf.tobytes().split(b"\0")[0].decode().splitlines():
            tok = line.split()
            sizes[tok[0]] = int(tok[1])
            if tok[2:] == ["state"]:
                held.add(tok[0])
        return (sizes, held) if state else sizes

    # ---- f4: shot boundary detection
    def shot_dfd(self, frames, width, height, tables, want_gray=False, want_flow=False):
        """displaced frame differences of consecutive frames (structure/shot.py:71-99): float64 [n - 1]
        (+ the small gray images uint8 [n, height, width] and the flows float32 [n - 1, height, width, 2] on request)"""
        n = len(frames)
        t = np.ascontiguousarray(tables, np.float32)
        if t.shape != (22,):
            raise ValueError("shot tables: 22 floats (structure.shot_tables())")
        dfd = np.zeros(max(n - 1, 0), np.float64)
        gray = np.zeros((n, height, width), np.uint8) if want_gray else None
        flow = np.zeros((max(n - 1, 0), height, width, 2), np.float32) if want_flow else None
        with self._staging():
            check(self._l.pvf_shot_dfd(self._h, ptr(self._handles(frames)), n, int(width), int(height), ptr(t), ptr(dfd) if n > 1 else None,
                                       ptr(gray) if want_gray else None, ptr(flow) if want_flow and n > 1 else None))
        out = (dfd,)
        if want_gray:
            out += (gray,)
        if want_flow:
            out += (flow,)
        return out if len(out) > 1 else dfd

    # ---- shot threading (csrc/orb.hip)
    ORB_CAP, ORB_CAP_MAX = 1024, 65536     # keypoint rows per frame: the first try of orb_extract, the library's limit

    def orb_extract(self, frames, width, height, cap=None):
        """ORB of the reference's shot threading (structure/thread.py:139-150) on every frame: the frame resized to width x height,
        gray, cv2.ORB_create() defaults.  Returns (counts int32 [n], keypoints float32 [n, cap, 6] = (x, y, level, FAST score, Harris
        response, angle) in level / y / x order, descriptors uint8 [n, cap, 32]); rows past counts[i] are unused.  The descriptors
        stay on the device for orb_match_counts(pairs).
        cap None: ORB_CAP rows, and when a frame has more keypoints (retainBest keeps every point tied with the last one, so a level
        can exceed its quota) the call is repeated once with the cap the largest frame needs.  A given cap is strict: a frame with
        more keypoints raises OrbCapError; nothing is truncated."""
        if cap is not None:
            return self._orb_extract(frames, width, height, int(cap))
        try:
            return self._orb_extract(frames, width, height, self.ORB_CAP)
        except _lib.OrbCapError as e:
            if e.needed > self.ORB_CAP_MAX:
                raise _lib.OrbCapError("orb: a frame has %d keypoints (ties of retainBest included), more than the %d rows per frame the "
                                       "library can return" % (e.needed, self.ORB_CAP_MAX), e.needed)
            return self._orb_extract(frames, width, height, e.needed)

    def _orb_extract(self, frames, width, height, cap):
        """one pvf_orb_extract call; OrbCapError (with the cap every frame fits in) when a frame has more than `cap` keypoints"""
        n = len(frames)
        counts = np.zeros(n, np.int32)
        kp = np.zeros((n, cap, 6), np.float32)
        desc = np.zeros((n, cap, 32), np.uint8)
        with self._staging():
            rc = self._l.pvf_orb_extract(self._h, ptr(self._handles(frames)), n, int(width), int(height), int(cap), ptr(counts), ptr(kp),
                                         ptr(desc))
        if rc != 0:
            msg = self._l.pvf_last_error().decode("utf-8", "replace")
            if n and counts.min() < 0:                    # -needed for the frames that did not fit (include/pvface.h)
                raise _lib.OrbCapError(msg, -int(counts.min()))
            raise _lib.PvfError(msg)
        return counts, kp, desc

    def orb_match_counts(self, pairs, descriptors=None, rows=None):
        """counts[p] = rows of set pairs[p][0] whose two nearest rows of set pairs[p][1] (Hamming) pass the ratio test 10 d1 < 7 d2
        (thread.py:152-170 with an exact 2-NN); 0 when either set has fewer than 2 rows.  descriptors uint8 [n_sets, cap, 32] with
        rows[n_sets] used rows each; None: the sets of the last orb_extract on this context."""
        pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        out = np.zeros(len(pr), np.int32)
        if descriptors is None:
            check(self._l.pvf_orb_match_counts(self._h, None, None, 0, 0, ptr(pr), len(pr), ptr(out)))
        else:
            d = np.ascontiguousarray(descriptors, np.uint8)
            if d.ndim != 3 or d.shape[2] != 32:
                raise ValueError("descriptors: uint8 [n_sets, cap, 32]")
            r = np.ascontiguousarray(rows, np.int32)
            check(self._l.pvf_orb_match_counts(self._h, ptr(d), ptr(r), d.shape[0], d.shape[1], ptr(pr), len(pr), ptr(out)))
        return out

    # ---- S5
    def pair_mean_dist(self, X, row_start, metric=0):
        """T x T matrix of mean pair distances between the rows of two tracks; metric 0 = Euclidean (reference), 1 = cosine"""
        X = np.ascontiguousarray(X, np.float64)
        rs = np.ascontiguousarray(row_start, np.int32)
        T = len(rs) - 1
        D = np.zeros((T, T), np.float64)
        check(self._l.pvf_pair_mean_dist_metric(self._h, ptr(X), X.shape[0], X.shape[1], ptr(rs), T, int(metric), ptr(D)))
        return D

    # ---- identification against a gallery (pvf_gallery_mean_dist / pvf_identify_dist / pvf_identify; include/pvface.h states the rules)
    @staticmethod
    def _identify_tables(X, row_start, G, gal_start):
        X = np.ascontiguousarray(X, np.float64)
        G = np.ascontiguousarray(G, np.float64)
        if X.ndim != 2 or G.ndim != 2 or X.shape[1] != G.shape[1]:
            raise ValueError("identify: X [N, dim] and G [M, dim] are expected")
        return X, np.ascontiguousarray(row_start, np.int32), G, np.ascontiguousarray(gal_start, np.int32)

    def gallery_mean_dist(self, X, row_start, G, gal_start, metric=0):
        """T x K matrix of the mean pair distances between the rows of query group t and the rows of identity k"""
        X, rs, G, gs = self._identify_tables(X, row_start, G, gal_start)
        T, K = len(rs) - 1, len(gs) - 1
        D = np.zeros((max(T, 0), max(K, 0)), np.float64)
        check(self._l.pvf_gallery_mean_dist(self._h, ptr(X), X.shape[0], ptr(rs), T, ptr(G), G.shape[0], ptr(gs), K, X.shape[1], int(metric), ptr(D)))
        return D

    @staticmethod
    def _picks(T):
        T = max(T, 0)
        return np.full(T, -1, np.int32), np.full(T, np.inf, np.float64), np.full(T, -1, np.int32), np.full(T, np.inf, np.float64)

    def identify_dist(self, D, threshold):
        """the decision per row of a T x K matrix -> (best, best_dist, second, second_dist)"""
        D = np.ascontiguousarray(D, np.float64)
        if D.ndim != 2:
            raise ValueError("identify_dist: a T x K matrix is expected")
        out = self._picks(D.shape[0])
        check(self._l.pvf_identify_dist(self._h, ptr(D), D.shape[0], D.shape[1], float(threshold), *[ptr(o) for o in out]))
        return out

    def identify(self, X, row_start, G, gal_start, threshold, metric=0, return_dist=False):
        """distances and decision in one call -> (best, best_dist, second, second_dist), with return_dist also D [T, K]"""
        X, rs, G, gs = self._identify_tables(X, row_start, G, gal_start)
        T, K = len(rs) - 1, len(gs) - 1
        out = self._picks(T)
        D = np.zeros((max(T, 0), max(K, 0)), np.float64) if return_dist else None
        check(self._l.pvf_identify(self._h, ptr(X), X.shape[0], ptr(rs), T, ptr(G), G.shape[0], ptr(gs), K, X.shape[1], int(metric), float(threshold),
                                   *([ptr(o) for o in out] + [None if D is None else ptr(D)])))
        return out + (D,) if return_dist else out

    # ---- search: the exact k nearest rows of a table (pvf_search; SEARCH.md states the rules in integers)
    def search(self, Qrows, X, k, max_d2=-1, query_group=None, row_group=None):
        """-> (idx int32 [Q, k], d2 int64 [Q, k], count int32 [Q]): per query row the k nearest rows of X by (d2, index), -1 past count"""
        Qrows = np.ascontiguousarray(Qrows, np.float64)
        X = np.ascontiguousarray(X, np.float64)
        if Qrows.ndim != 2 or X.ndim != 2 or Qrows.shape[1] != X.shape[1]:
            raise ValueError("search: Qrows [Q, dim] and X [N, dim] are expected")
        if (query_group is None) != (row_group is None):
            raise ValueError("search: query_group and row_group are given together or not at all")
        qg = rg = None
        if query_group is not None:
            qg = np.ascontiguousarray(query_group, np.int32)
            rg = np.ascontiguousarray(row_group, np.int32)
            if qg.shape != (Qrows.shape[0],) or rg.shape != (X.shape[0],):
                raise ValueError("search: one query_group per query row and one row_group per table row")
        Q, k = Qrows.shape[0], int(k)
        kk = min(max(k, 0), 1024)                      # (a k out of range is refused by the library, before it writes anything)
        idx, d2, count = np.full((Q, kk), -1, np.int32), np.full((Q, kk), -1, np.int64), np.zeros(Q, np.int32)
        check(self._l.pvf_search(self._h, ptr(Qrows), Q, ptr(X), X.shape[0], X.shape[1], k, int(max_d2), ptr(qg), ptr(rg), ptr(idx), ptr(d2),
                                 ptr(count)))
        return idx, d2, count

    @staticmethod
    def search_plan(Q, N, k):
        """how pvf_search cuts a call of these sizes -> dict(chunk_rows, n_chunks, n_ranges, range_blocks, pending, arena_bytes)"""
        out = np.zeros(6, np.int64)
        check(_lib.lib().pvf_search_plan(int(Q), int(N), int(k), ptr(out)))
        return dict(zip(("chunk_rows", "n_chunks", "n_ranges", "range_blocks", "pending", "arena_bytes"), (int(v) for v in out)))

    # ---- cast: rank-order clustering on the exact k-NN graph (pvf_cast; CAST.md states the rules in integers)
    @staticmethod
    def _cast_table(X, group):
        X = np.ascontiguousarray(X, np.float64)
        if X.ndim != 2:
            raise ValueError("cast: X [N, dim] is expected")
        g = None
        if group is not None:
            g = np.ascontiguousarray(group, np.int32)
            if g.shape != (X.shape[0],):
                raise ValueError("cast: one group per row")
        return X, g

    def cast(self, X, k, max_d2=-1, num=2000, den=1000, group=None):
        """-> (labels int32 [N], n_components): the smallest row of every row's component under the links of CAST.md"""
        X, g = self._cast_table(X, group)
        labels, n = np.full(X.shape[0], -1, np.int32), C.c_int32(0)
        check(self._l.pvf_cast(self._h, ptr(X), X.shape[0], X.shape[1], int(k), int(max_d2), int(num), int(den), ptr(g), ptr(labels), C.byref(n)))
        return labels, n.value

    def cast_lists(self, X, k, max_d2=-1, group=None):
        """-> (idx int32 [N, k], d2 int64 [N, k], count int32 [N]): the list of every row, -1 past count"""
        X, g = self._cast_table(X, group)
        N, kk = X.shape[0], min(max(int(k), 0), 256)
        idx, d2, count = np.full((N, kk), -1, np.int32), np.full((N, kk), -1, np.int64), np.zeros(N, np.int32)
        check(self._l.pvf_debug_cast_lists(self._h, ptr(X), N, X.shape[1], int(k), int(max_d2), ptr(g), ptr(idx), ptr(d2), ptr(count)))
        return idx, d2, count

    def cast_links(self, X, k, max_d2=-1, num=2000, den=1000, group=None):
        """-> (m int32 [N, k], r int32 [N, k], linked uint8 [N, k]) per (row, slot of its list); -1, -1, 0 past the list"""
        X, g = self._cast_table(X, group)
        N, kk = X.shape[0], min(max(int(k), 0), 256)
        m, r, linked = np.full((N, kk), -1, np.int32), np.full((N, kk), -1, np.int32), np.zeros((N, kk), np.uint8)
        check(self._l.pvf_debug_cast_links(self._h, ptr(X), N, X.shape[1], int(k), int(max_d2), int(num), int(den), ptr(g), ptr(m), ptr(r), ptr(linked)))
        return m, r, linked

    @staticmethod
    def cast_plan(N, k):
        """how pvf_cast cuts a call of these sizes -> dict(qblock, n_batches, chunk_rows, n_chunks, n_ranges, device_bytes)"""
        out = np.zeros(6, np.int64)
        check(_lib.lib().pvf_cast_plan(int(N), int(k), ptr(out)))
        return dict(zip(("qblock", "n_batches", "chunk_rows", "n_chunks", "n_ranges", "device_bytes"), (int(v) for v in out)))

    # ---- the fingerprint and repeat verbs (REPEAT.md)
    def frame_prints(self, frames, out_ptr=None):
        """resident frames, of any sizes, as prints (pvf_frame_prints): uint64 [n, 4] = H, V, SY | RANGE << 32, 0.  With out_ptr, a
        device address that holds as much, the prints stay in HBM and nothing is returned."""
        n = len(frames)
        out = None if out_ptr is not None else np.zeros((n, 4), np.uint64)
        with self._staging():
            check(self._l.pvf_frame_prints(self._h, ptr(self._handles(frames)), n, C.c_void_p(int(out_ptr)) if out_ptr is not None else ptr(out),
                                           1 if out_ptr is not None else 0))
        return out

    RUNS_FIRST_CAP = 65536

    def print_runs(self, A, usable_a, B=None, usable_b=None, tau=10, min_len=1, min_gap=1, cap=None):
        """-> int32 [found, 3]: the runs (i, j, len) of matching prints of A uint64 [NA, 2 or 4] against B, or against A itself from
        diagonal min_gap on when B is None, ordered by (j - i, i) (pvf_print_runs).  The call is made again with room for every run when
        the first cap (65 536 runs) is too small."""
        def table(P, u, what):
            P = np.asarray(P)
            if P.dtype != np.uint64 or P.ndim != 2 or P.shape[1] not in (2, 4):
                raise ValueError("print_runs: %s is uint64 [n, 2] or [n, 4]" % what)
            u = np.ascontiguousarray(u, np.uint8)
            if u.shape != (len(P),):
                raise ValueError("print_runs: one usable byte per row of %s" % what)
            return np.ascontiguousarray(P[:, :2]), u
        A, ua = table(A, usable_a, "A")
        if B is not None:
            B, ub = table(B, usable_b, "B")
        cap = self.RUNS_FIRST_CAP if cap is None else int(cap)
        found = C.c_int64(0)
        while True:
            runs = np.zeros((max(cap, 0), 3), np.int32)
            check(self._l.pvf_print_runs(self._h, ptr(A), ptr(ua), len(A), ptr(B) if B is not None else None, ptr(ub) if B is not None else None,
                                         len(B) if B is not None else 0, int(tau), int(min_len), int(min_gap), ptr(runs), cap, C.byref(found)))
            if found.value <= cap:
                return runs[:found.value]
            cap = found.value

    # ---- the blend and transition verbs (BLEND.md)
    def frame_blend(self, frames, tw, th, hist=None, want_luma=True):
        """resident frames of one size as blend records (pvf_frame_blend): (rows uint32 [n, 16], luma uint8 [n, tw * th] or None).
        hist: the luma planes of the up to 32 frames in front of frames[0], oldest first, uint8 [nh, tw * th] -- what an earlier call
        returned as luma; the call keeps nothing."""
        n, tw, th = len(frames), int(tw), int(th)
        P = tw * th if tw > 0 and th > 0 else 0
        hist = np.zeros((0, P), np.uint8) if hist is None else np.ascontiguousarray(hist, np.uint8)
        if hist.ndim != 2 or hist.shape[1] != P:
            raise ValueError("frame_blend: the history is uint8 [nh, tw * th]")
        rows = np.zeros((n, 16), np.uint32)
        luma = np.zeros((n, P), np.uint8) if want_luma else None
        with self._staging():
            check(self._l.pvf_frame_blend(self._h, ptr(self._handles(frames)), n, tw, th, ptr(hist) if len(hist) else None, len(hist), ptr(rows),
                                          ptr(luma) if want_luma else None))
        return rows, luma

    def blend_measure(self, luma, first=0):
        """-> uint32 [N - first, 16]: the blend records of rows first .. N - 1 of the caller's own luma planes uint8 [N, P], the rows in
        front of them as history (pvf_blend_measure); S1 and S2 come from the planes, the size word is 0"""
        luma = np.ascontiguousarray(luma, np.uint8)
        if luma.ndim != 2:
            raise ValueError("blend_measure: the planes are uint8 [N, P]")
        N, P = luma.shape
        rows = np.zeros((max(N - int(first), 0), 16), np.uint32)
        check(self._l.pvf_blend_measure(self._h, ptr(luma) if luma.size else None, N, P, int(first), ptr(rows) if rows.size else None))
        return rows

    def flow_motion(self, flow):
        """-> int64 [n, 10]: the motion rows (MOTION.md) of the caller's own flows float32 [n, h, w, 2] (pvf_flow_motion); word 7 is 0"""
        flow = np.ascontiguousarray(flow, np.float32)
        if flow.ndim != 4 or flow.shape[3] != 2:
            raise ValueError("flow_motion: the flows are float32 [n, h, w, 2]")
        n, h, w = flow.shape[:3]
        rows = np.zeros((n, 10), np.int64)
        check(self._l.pvf_flow_motion(self._h, ptr(flow) if flow.size else None, n, h, w, ptr(rows) if n else None))
        return rows

    def shot_motion(self, frames, width, height, tables, want_dfd=True):
        """resident frames of one size -> (rows int64 [n - 1, 10], dfd float64 [n - 1] or None): the motion rows of the flows
        pvf_shot_dfd computes between consecutive frames, fitted on the device (pvf_shot_motion); word 7 holds the bits of dfd"""
        n = len(frames)
        t = np.ascontiguousarray(tables, np.float32)
        if t.shape != (22,):
            raise ValueError("shot tables: 22 floats (structure.shot_tables())")
        rows = np.zeros((max(n - 1, 0), 10), np.int64)
        dfd = np.zeros(max(n - 1, 0), np.float64) if want_dfd else None
        with self._staging():
            check(self._l.pvf_shot_motion(self._h, ptr(self._handles(frames)) if n else None, n, int(width), int(height), ptr(t),
                                          ptr(rows) if n > 1 else None, ptr(dfd) if want_dfd and n > 1 else None))
        return rows, dfd

    def frame_text(self, frames, prev=None, edge=48, still=8, on=24, want_counts=False, size=None):
        """resident frames of one size as text records (pvf_frame_text; CAPTION.md): (rows uint32 [n, 8 + ch * wpr], counts uint16
        [n, ch, cw, 4] = E, S, M, NP or None).  prev: the resident frame in front of frames[0] -- the last frame of the call before;
        the call keeps nothing.  size: (w, h), needed only where `frames` are bare handles (frame_handles)."""
        n = len(frames)
        if n == 0:
            return np.zeros((0, 8), np.uint32), (np.zeros((0, 0, 0, 4), np.uint16) if want_counts else None)
        w, h = size if size is not None else (frames[0].shape[1], frames[0].shape[0])
        cw, ch = (w + 15) // 16, (h + 15) // 16
        rows = np.zeros((n, 8 + ch * ((cw + 31) // 32)), np.uint32)
        counts = np.zeros((n, ch, cw, 4), np.uint16) if want_counts else None
        with self._staging():
            check(self._l.pvf_frame_text(self._h, ptr(self._handles(frames)), n, int(getattr(prev, "handle", prev)) if prev is not None else 0, int(edge), int(still),
                                         int(on), ptr(rows), ptr(counts) if want_counts else None))
        return rows, counts

    def frame_hist(self, frames, windows, group, G, bands=2, out_ptr=None):
        """the colour histograms of windows of resident frames, of any sizes (pvf_frame_hist; CLOTHES.md): uint32 [G, bands, 256], the
        pixels of the windows (x0, y0, x1, y1) -- int32 pixels, half-open, clipped to their frame -- of every group, per band.  With
        out_ptr, a device address that holds as much, the counts stay in HBM and nothing is returned."""
        n = len(frames)
        windows = np.ascontiguousarray(windows, np.int32).reshape(-1, 4)
        group = np.ascontiguousarray(group, np.int32).reshape(-1)
        if len(windows) != n or len(group) != n:
            raise ValueError("frame_hist: one window (x0, y0, x1, y1) and one group per frame")
        G, bands = int(G), int(bands)
        out = None if out_ptr is not None else np.empty((G, bands, 256) if G >= 1 and 1 <= bands <= 4 and G * bands <= 65536 else (0,), np.uint32)
        with self._staging():
            check(self._l.pvf_frame_hist(self._h, ptr(self._handles(frames)) if n else None, ptr(windows) if n else None, ptr(group) if n else None, n,
                                         G, bands, C.c_void_p(int(out_ptr)) if out_ptr is not None else ptr(out), 1 if out_ptr is not None else 0))
        return out

    # The four agglomerating calls have a `_cooccur` sibling that takes `extent` (float64 [T, 2]: start and end of every track, seconds):
    # the do-not-cooccur constraint (clustering.py:142-143; pvf_cluster_*_cooccur) -- tracks whose extents intersect never share a
    # cluster.  They return (labels, merge log, n_blocked = the co-occurring pairs); `flags` bit 0 is the library's test switch
    # (launch-per-merge path).
    @staticmethod
    def _extent(extent, T):
        e = np.ascontiguousarray(extent, np.float64)
        if e.shape != (T, 2):
            raise ValueError("extent: float64 [T, 2] (start, end) is expected")
        return e

    def _cluster_tracks(self, X, row_start, threshold, extent=None, flags=0):
        X = np.ascontiguousarray(X, np.float64)
        rs = np.ascontiguousarray(row_start, np.int32)
        T = len(rs) - 1
        labels = np.zeros(T, np.int32)
        log = np.zeros((max(T - 1, 1), 4), np.float64)
        n, nb = C.c_int32(0), C.c_int32(0)
        if extent is not None:
            e = self._extent(extent, T)
            check(self._l.pvf_cluster_tracks_cooccur(self._h, ptr(X), X.shape[0], X.shape[1], ptr(rs), T, float(threshold), ptr(labels), ptr(log),
                                                     C.byref(n), ptr(e), C.byref(nb), int(flags)))
        else:
            check(self._l.pvf_cluster_tracks(self._h, ptr(X), X.shape[0], X.shape[1], ptr(rs), T, float(threshold), ptr(labels), ptr(log), C.byref(n)))
        return labels, log[:n.value], nb.value

    def cluster_tracks(self, X, row_start, threshold):
        return self._cluster_tracks(X, row_start, threshold)[:2]

    def cluster_tracks_cooccur(self, X, row_start, threshold, extent, flags=0):
        return self._cluster_tracks(X, row_start, threshold, self._extent(extent, len(row_start) - 1), flags)

    @staticmethod
    def _f32_rows(emb):
        """(address, row stride in bytes, rows, on device?, keep-alive) of float32 descriptor rows: a numpy array or a DeviceRows"""
        if isinstance(emb, DeviceRows):
            return C.c_void_p(emb.ptr), emb.stride, emb.n, 1, emb
        a = np.asarray(emb)
        if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != 128 or a.strides[1] != 4 or a.strides[0] < 512:
            a = np.ascontiguousarray(a, np.float32).reshape(-1, 128)
        return ptr(a), int(a.strides[0]) if len(a) else 512, len(a), 0, a

    @staticmethod
    def _f32_order(name, order, rs, n_src):
        """`order` as int32, after the checks the library cannot make (it reads order[k] for every k < row_start[-1])"""
        if rs.ndim != 1 or len(rs) < 2:
            raise ValueError("%s: row_start holds T + 1 entries, T >= 1" % name)
        N = int(rs[-1])
        if order is None:
            if n_src < N:
                raise ValueError("%s: %d rows, row_start ends at %d" % (name, n_src, N))
            return None
        order = np.ascontiguousarray(order, np.int32)
        if order.ndim != 1 or len(order) != N:
            raise ValueError("%s: `order` holds %d entries, row_start ends at %d" % (name, order.size, N))
        return order

    def _cluster_tracks_f32(self, emb, order, row_start, threshold, decimals=5, metric=0, extent=None, flags=0):
        """the in-memory clustering (pvf_cluster_tracks_f32): float32 descriptors (numpy [n, 128] or DeviceRows), rows of the table =
        round(emb[order], decimals) made on the device, upper-triangle pair means, mirror, agglomeration -> (labels, merge log)"""
        p, stride, n_src, on_dev, keep = self._f32_rows(emb)
        rs = np.ascontiguousarray(row_start, np.int32)
        T = len(rs) - 1
        order = self._f32_order("cluster_tracks_f32", order, rs, n_src)
        N = int(rs[-1])
        labels = np.zeros(T, np.int32)
        log = np.zeros((max(T - 1, 1), 4), np.float64)
        n, nb = C.c_int32(0), C.c_int32(0)
        if extent is not None:
            e = self._extent(extent, T)
            check(self._l.pvf_cluster_tracks_f32_cooccur(self._h, p, stride, n_src, on_dev, None if order is None else ptr(order), N, int(decimals),
                                                         ptr(rs), T, int(metric), float(threshold), ptr(labels), ptr(log), C.byref(n),
                                                         ptr(e), C.byref(nb), int(flags)))
        else:
            check(self._l.pvf_cluster_tracks_f32(self._h, p, stride, n_src, on_dev, None if order is None else ptr(order), N, int(decimals), ptr(rs), T,
                                                 int(metric), float(threshold), ptr(labels), ptr(log), C.byref(n)))
        return labels, log[:n.value], nb.value

    def cluster_tracks_f32(self, emb, order, row_start, threshold, decimals=5, metric=0):
        return self._cluster_tracks_f32(emb, order, row_start, threshold, decimals, metric)[:2]

    def cluster_tracks_f32_cooccur(self, emb, order, row_start, threshold, decimals=5, metric=0, *, extent, flags=0):
        return self._cluster_tracks_f32(emb, order, row_start, threshold, decimals, metric, self._extent(extent, len(row_start) - 1), flags)

    def pair_upper_rows_f32(self, emb, order, row_start, track0, track1, decimals=5, out=None):
        """the upper-triangle entries of rows [track0, track1) of the track-pair matrix, compact [(track1 - track0), T]: into `out`
        (a DeviceRows of T * 8-byte rows: stays in HBM for the all-gather) or returned as a numpy array"""
        p, stride, n_src, on_dev, keep = self._f32_rows(emb)
        rs = np.ascontiguousarray(row_start, np.int32)
        T = len(rs) - 1
        order = self._f32_order("pair_upper_rows_f32", order, rs, n_src)
        m = int(track1) - int(track0)
        if out is None:
            res = np.zeros((max(m, 0), T), np.float64)
            op, odev = ptr(res), 0
        else:
            if out.n < m or out.stride != T * 8:
                raise ValueError("pair_upper_rows_f32: `out` must hold (track1 - track0) rows of T float64 values")
            res, op, odev = out, C.c_void_p(out.ptr), 1
        check(self._l.pvf_pair_upper_rows_f32(self._h, p, stride, n_src, on_dev, None if order is None else ptr(order), int(rs[-1]), int(decimals),
                                              ptr(rs), T, int(track0), int(track1), op, odev))
        return res

    def _cluster_upper(self, U, row_start, threshold, extent=None, flags=0):
        """mirror + agglomeration of an assembled upper triangle: U numpy [T, T] or a DeviceRows of T rows of T float64"""
        rs = np.ascontiguousarray(row_start, np.int32)
        T = len(rs) - 1
        if isinstance(U, DeviceRows):
            if U.n != T or U.stride != T * 8:
                raise ValueError("cluster_upper: a T x T matrix is expected")
            p, on_dev = C.c_void_p(U.ptr), 1
        else:
            U = np.ascontiguousarray(U, np.float64)
            p, on_dev = ptr(U), 0
        labels = np.zeros(T, np.int32)
        log = np.zeros((max(T - 1, 1), 4), np.float64)
        n, nb = C.c_int32(0), C.c_int32(0)
        if extent is not None:
            e = self._extent(extent, T)
            check(self._l.pvf_cluster_upper_cooccur(self._h, p, on_dev, ptr(rs), T, float(threshold), ptr(labels), ptr(log), C.byref(n),
                                                    ptr(e), C.byref(nb), int(flags)))
        else:
            check(self._l.pvf_cluster_upper(self._h, p, on_dev, ptr(rs), T, float(threshold), ptr(labels), ptr(log), C.byref(n)))
        return labels, log[:n.value], nb.value

    def cluster_upper(self, U, row_start, threshold):
        return self._cluster_upper(U, row_start, threshold)[:2]

    def cluster_upper_cooccur(self, U, row_start, threshold, extent, flags=0):
        return self._cluster_upper(U, row_start, threshold, self._extent(extent, len(row_start) - 1), flags)

    def pair_mean_dist_rows(self, X, row_start, track0, track1):
        """the complete rows [track0, track1) of the T x T track-pair mean-distance matrix (other rows zero): j > i computed, j < i mirrored"""
        return self._pair_rows(self._l.pvf_pair_mean_dist_rows, X, row_start, track0, track1)

    def pair_upper_rows(self, X, row_start, track0, track1):
        """upper-triangle entries (j > i) of rows [track0, track1) of that matrix (everything else zero): a rank's share of a split clustering"""
        return self._pair_rows(self._l.pvf_pair_upper_rows, X, row_start, track0, track1)

    def _pair_rows(self, fn, X, row_start, track0, track1):
        X = np.ascontiguousarray(X, np.float64)
        rs = np.ascontiguousarray(row_start, np.int32)
        T = len(rs) - 1
        if X.ndim != 2 or rs.ndim != 1 or T < 1 or X.shape[0] < int(rs[-1]):
            raise ValueError("pair rows: X [N, dim] with N = row_start[-1] = %s rows is expected, got %s" % (rs[-1] if rs.size else None, X.shape))
        D = np.zeros((T, T), np.float64)
        check(fn(self._h, ptr(X), X.shape[0], X.shape[1], ptr(rs), T, int(track0), int(track1), ptr(D)))
        return D

    def _cluster_dist(self, D, row_start, threshold, extent=None, flags=0):
        D = np.ascontiguousarray(D, np.float64)
        rs = np.ascontiguousarray(row_start, np.int32)
        T = len(rs) - 1
        labels = np.zeros(T, np.int32)
        log = np.zeros((max(T - 1, 1), 4), np.float64)
        n, nb = C.c_int32(0), C.c_int32(0)
        if extent is not None:
            e = self._extent(extent, T)
            check(self._l.pvf_cluster_dist_cooccur(self._h, ptr(D), ptr(rs), T, float(threshold), ptr(labels), ptr(log), C.byref(n),
                                                   ptr(e), C.byref(nb), int(flags)))
        else:
            check(self._l.pvf_cluster_dist(self._h, ptr(D), ptr(rs), T, float(threshold), ptr(labels), ptr(log), C.byref(n)))
        return labels, log[:n.value], nb.value

    def cluster_dist(self, D, row_start, threshold):
        return self._cluster_dist(D, row_start, threshold)[:2]

    def cluster_dist_cooccur(self, D, row_start, threshold, extent, flags=0):
        return self._cluster_dist(D, row_start, threshold, self._extent(extent, len(row_start) - 1), flags)

    # ---- measurement
    def detector_screening(self, on=True, list_cap=0):
        """the detector's screening pass (csrc/screen.hip): windows are first scored on the f16 matrix cores with a proven error bound and
        only those within the bound of the threshold go through the exact fp32 chain -- same rectangles, order and scores, bit for bit"""
        check(self._l.pvf_detector_screening(self._h, 1 if on else 0, int(list_cap)))

    def detector_screening_stats(self):
        """{"batches", "listed", "retries", "bounds", "pipe_err"}: batches screened, (window, filter) pairs that went through the exact
        chain, calls repeated on the dense kernel, the error bound per filter (score units), the accumulation error the context measured
        on its matrix pipe (relative to the sum of magnitudes; -1 before the first screened batch)"""
        b, n, r, pe = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(-1.0)
        bounds = np.zeros(8, np.float64)
        check(self._l.pvf_detector_screening_stats(self._h, C.byref(b), C.byref(n), C.byref(r), ptr(bounds), C.byref(pe)))
        return {"batches": b.value, "listed": n.value, "retries": r.value, "bounds": bounds[:5].tolist(), "pipe_err": pe.value}

    def embedder_split(self, on=True):
        """the embedder's convolutions on the f16 matrix cores with split operands (csrc/resnet.hip: conv_tile_k with ConvSplit; on by default): three
        f16 products of scaled hi / lo halves per product, descriptors within the bound of DESIGN.md section 4; a face whose activations
        leave the f16 range is embedded again on the exact fp32 kernels.  off: the exact kernels only"""
        check(self._l.pvf_embedder_split(self._h, 1 if on else 0))

    def embedder_split_stats(self):
        """{"faces", "reruns", "pipe_err"}: faces embedded with the split on, faces of those embedded again on the exact kernels, the
        accumulation error the context measured on its f16 matrix pipe (relative to the sum of magnitudes; -1 before the first split
        forward)"""
        f, r, pe = C.c_int64(0), C.c_int64(0), C.c_double(-1.0)
        check(self._l.pvf_embedder_split_stats(self._h, C.byref(f), C.byref(r), C.byref(pe)))
        return {"faces": f.value, "reruns": r.value, "pipe_err": pe.value}

    def prof_enable(self, on=True):
        check(self._l.pvf_prof_enable(self._h, 1 if on else 0))

    def prof_reset(self):
        check(self._l.pvf_prof_reset(self._h))

    def prof_get(self, family):
        ms, n = C.c_double(0), C.c_int64(0)
        check(self._l.pvf_prof_get(self._h, family.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


def _seed64(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


_default = None


def default_context():
    """Process-wide context on the GPU of this rank (LOCAL_RANK) -- what the dlib-like shim objects use."""
    global _default
    if _default is None:
        import os
        _default = Context(device=int(os.environ.get("LOCAL_RANK", "0")))
    return _default
