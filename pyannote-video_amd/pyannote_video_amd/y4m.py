"""YUV4MPEG2 (`.y4m`) video: what `ffmpeg -f yuv4mpegpipe` writes, read without decoding anything.

    ffmpeg -i film.mkv -pix_fmt yuv420p -f yuv4mpegpipe film.y4m

The reference asks ffmpeg for `-pix_fmt rgb24` and reads RGB from a pipe (video.py:332-358,368-401); here the planes a decoder
produces stay as they are -- 1.5 bytes per pixel for 4:2:0 -- until they are in HBM, where one kernel makes the RGB frame
(csrc/ingest.hip: yuv_to_rgb_k; the arithmetic is stated in INTEGRATION.md section 1, "YUV to RGB", and restated in `to_rgb` below).

`Y4mVideo` has the contract of `cli.NpyVideo`; it yields `(t, YuvFrame)`.  A regular file is memory mapped: its length is known,
any frame can be read, a second pass costs nothing, and the only host copy of a frame is the one into the pinned ingest slot.
A stream (a pipe, stdin) is read once, front to back, and has no length."""
import mmap
import numpy as np

MAGIC = b"YUV4MPEG2"
LAYOUTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}      # (sx, sy): chroma plane = ceil(w / 2^sx) x ceil(h / 2^sy)
# C tags: 4:2:0 differs between its variants in where the chroma samples sit, not in the plane layout (chroma is replicated here)
_C_TAGS = {"420": "420", "420jpeg": "420", "420mpeg2": "420", "420paldv": "420", "422": "422", "444": "444"}
# (crv, cbu, cgu, cgv), 16.16 fixed point
MATRICES = {"601": (104597, 132201, 25675, 53279), "709": (117504, 138453, 13954, 34903)}


def coefficients(matrix="601", full_range=False):
    """(ymul, yoff, crv, cgu, cgv, cbu) of  C = ymul * Y + yoff,  R = (C + crv * (V - 128)) >> 16, ..."""
    if str(matrix) not in MATRICES:
        raise ValueError("matrix must be '601' or '709', not %r" % (matrix,))
    crv, cbu, cgu, cgv = MATRICES[str(matrix)]
    if full_range:
        crv, cbu, cgu, cgv = ((c * 224) // 255 for c in (crv, cbu, cgu, cgv))
        return 65536, 32768, crv, cgu, cgv, cbu
    return 76309, 32768 - 16 * 76309, crv, cgu, cgv, cbu


def chroma_shape(height, width, layout):
    sx, sy = LAYOUTS[layout]
    return (height + (1 << sy) - 1) >> sy, (width + (1 << sx) - 1) >> sx


def to_rgb(y, u, v, layout="420", matrix="601", full_range=False):
    """the conversion of csrc/ingest.hip on the host (numpy, int32 like the kernel): uint8 [H, W, 3]"""
    sx, sy = LAYOUTS[layout]
    h, w = y.shape
    ymul, yoff, crv, cgu, cgv, cbu = coefficients(matrix, full_range)
    iy, ix = np.arange(h) >> sy, np.arange(w) >> sx
    c = ymul * np.asarray(y, np.int32) + yoff
    uu = np.asarray(u, np.int32)[iy][:, ix] - 128
    vv = np.asarray(v, np.int32)[iy][:, ix] - 128
    out = np.empty((h, w, 3), np.uint8)
    out[..., 0] = np.clip((c + crv * vv) >> 16, 0, 255)
    out[..., 1] = np.clip((c - cgu * uu - cgv * vv) >> 16, 0, 255)
    out[..., 2] = np.clip((c + cbu * uu) >> 16, 0, 255)
    return out


class YuvFrame(object):
    """one 8-bit frame as planes: y [H, W], u and v [ceil(H / 2^sy), ceil(W / 2^sx)] (views; rows may be strided)"""
    __slots__ = ("y", "u", "v", "height", "width", "layout", "matrix", "full_range", "__weakref__")

    def __init__(self, y, u, v, layout="420", matrix="601", full_range=False):
        if layout not in LAYOUTS:
            raise ValueError("layout must be one of %s, not %r" % (sorted(LAYOUTS), layout))
        if str(matrix) not in MATRICES:
            raise ValueError("matrix must be '601' or '709', not %r" % (matrix,))
        for p in (y, u, v):
            if p.dtype != np.uint8 or p.ndim != 2:
                raise TypeError("YUV planes must be 2-D uint8 arrays")
        self.height, self.width = int(y.shape[0]), int(y.shape[1])
        if tuple(u.shape) != chroma_shape(self.height, self.width, layout) or u.shape != v.shape:
            raise ValueError("chroma planes of a %dx%d %s frame are %s, not %s / %s" % (
                self.width, self.height, layout, chroma_shape(self.height, self.width, layout), tuple(u.shape), tuple(v.shape)))
        self.y, self.u, self.v = y, u, v
        self.layout, self.matrix, self.full_range = layout, str(matrix), bool(full_range)

    @property
    def shape(self):
        return (self.height, self.width, 3)       # of the RGB frame it stands for

    @property
    def key(self):
        """what an ingest ring is made for"""
        return (self.height, self.width, self.layout, self.matrix, self.full_range)

    def rgb(self):
        return to_rgb(self.y, self.u, self.v, self.layout, self.matrix, self.full_range)


def _parse_header(line, name):
    tok = line.split()
    if not tok or tok[0] != MAGIC:
        raise IOError("%s: not a YUV4MPEG2 stream" % name)
    h = {"layout": "420", "rate": None, "full_range": None}
    for t in tok[1:]:
        t = t.decode("ascii", "replace")
        tag, val = t[:1], t[1:]
        if tag == "W":
            h["width"] = int(val)
        elif tag == "H":
            h["height"] = int(val)
        elif tag == "F":
            num, _, den = val.partition(":")
            if int(num) > 0 and int(den or 1) > 0:           # F0:0 = unknown
                h["rate"] = int(num) / float(int(den or 1))
                h["rate_tag"] = "%d:%d" % (int(num), int(den or 1))
        elif tag == "C":
            if val not in _C_TAGS:
                raise IOError("%s: chroma format C%s is not supported (8-bit C420*, C422 and C444 are)" % (name, val))
            h["layout"] = _C_TAGS[val]
        elif tag == "I":
            if val not in ("p", "?"):
                raise IOError("%s: interlaced material (I%s) is not supported" % (name, val))
        elif t.startswith("XCOLORRANGE="):
            r = t[len("XCOLORRANGE="):].upper()
            if r not in ("FULL", "LIMITED"):
                raise IOError("%s: unknown %s" % (name, t))
            h["full_range"] = r == "FULL"
        # A (pixel aspect) and other X comments carry nothing the frames depend on
    if h.get("width", 0) <= 0 or h.get("height", 0) <= 0:
        raise IOError("%s: the stream header has no frame size (W, H)" % name)
    return h


class Y4mVideo(object):
    """`path`: a file name, or a binary file object (a pipe: read once, no length).  frame_rate: used only when the header has no F
    tag; matrix / full_range: override the header (which cannot name a matrix: BT.601 unless told otherwise)."""

    def __init__(self, path, frame_rate=None, matrix=None, full_range=None):
        self._name = path if isinstance(path, str) else getattr(path, "name", "<stream>")
        self._map = self._file = None
        if isinstance(path, str):
            with open(path, "rb") as f:
                try:
                    self._map = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
                except (ValueError, OSError):            # empty, or not a regular file (a named pipe)
                    self._file = open(path, "rb")
        else:
            self._file = path
        if self._map is not None:
            end = self._map.find(b"\n", 0, 4096)
            line = self._map[:max(end, 0)]
            self._pos = end + 1
        else:
            line = self._file.readline(4096)
            end = len(line) - 1 if line.endswith(b"\n") else -1
            line = line[:-1]
        if end < 0:
            raise IOError("%s: not a YUV4MPEG2 stream" % self._name)
        hd = _parse_header(line, self._name)
        self.layout = hd["layout"]
        self.matrix = str(matrix) if matrix is not None else "601"
        if self.matrix not in MATRICES:
            raise ValueError("matrix must be '601' or '709', not %r" % (matrix,))
        self.full_range = bool(full_range) if full_range is not None else bool(hd["full_range"])
        rate = hd["rate"] if hd["rate"] is not None else frame_rate
        if rate is None:
            raise IOError("%s: the header names no frame rate; give one (--fps)" % self._name)
        self.frame_rate = float(rate)
        self.rate_tag = hd.get("rate_tag")              # the header's own F tag, for a writer that passes the rate on (render.Y4mWriter)
        w, h = hd["width"], hd["height"]
        self._size = (w, h)
        self._frame_size = self._size
        ch, cw = chroma_shape(h, w, self.layout)
        self._plane_bytes = (h * w, ch * cw)
        self._frame_bytes = h * w + 2 * ch * cw
        self._chroma = (ch, cw)
        self.step, self.start = 1.0 / self.frame_rate, 0.0
        self._offsets = None
        if self._map is not None:
            self._offsets = self._index()
            self.duration = len(self._offsets) / self.frame_rate
            self.end = self.duration
        else:
            self.duration = self.end = None              # a stream: not known before it has been read

    # ---- the file
    def _index(self):
        """byte offset of every frame's planes.  FRAME lines may carry parameters, so each is looked at: one short search per frame"""
        m, pos, n, out = self._map, self._pos, len(self._map), []
        while pos < n:
            if m[pos:pos + 5] != b"FRAME":
                raise IOError("%s: no FRAME marker at byte %d (frame %d)" % (self._name, pos, len(out)))
            end = m.find(b"\n", pos, pos + 256)
            if end < 0:
                raise IOError("%s: unterminated FRAME line at byte %d" % (self._name, pos))
            if end + 1 + self._frame_bytes > n:
                raise IOError("%s: frame %d is truncated (%d of %d bytes)" % (self._name, len(out), n - end - 1, self._frame_bytes))
            out.append(end + 1)
            pos = end + 1 + self._frame_bytes
        return out

    def _frame_of(self, buf, off):
        w, h = self._size
        ch, cw = self._chroma
        ny, nc = self._plane_bytes
        y = np.frombuffer(buf, np.uint8, ny, off).reshape(h, w)
        u = np.frombuffer(buf, np.uint8, nc, off + ny).reshape(ch, cw)
        v = np.frombuffer(buf, np.uint8, nc, off + ny + nc).reshape(ch, cw)
        return YuvFrame(y, u, v, self.layout, self.matrix, self.full_range)

    def close(self):
        # (frames handed out are views of the map: it is closed when the last of them is gone, not here)
        self._map = None
        if self._file is not None and hasattr(self._file, "close"):
            self._file.close()
        self._file = None

    # ---- the contract of cli.NpyVideo
    @property
    def size(self):
        return self._size

    @property
    def frame_size(self):
        return self._frame_size

    @frame_size.setter
    def frame_size(self, value):
        self._frame_size = tuple(int(v) for v in value)     # applied by the consumer on the device (FaceTracking: detect_min_size)

    def __len__(self):
        if self._offsets is None:
            raise TypeError("a Y4M stream has no length before it has been read; this needs a file")
        return len(self._offsets)

    def __iter__(self):
        if self._offsets is not None:
            for i in range(len(self._offsets)):
                yield i / self.frame_rate, self._frame_of(self._map, self._offsets[i])
            return
        if self._file is None:
            raise IOError("%s: a Y4M stream can be read once" % self._name)
        f, i = self._file, 0
        while True:
            line = f.readline(256)
            if not line:
                break
            if not line.startswith(b"FRAME") or not line.endswith(b"\n"):
                raise IOError("%s: no FRAME marker in front of frame %d" % (self._name, i))
            data = f.read(self._frame_bytes)
            while 0 < len(data) < self._frame_bytes:          # a pipe returns what it has
                more = f.read(self._frame_bytes - len(data))
                if not more:
                    break
                data += more
            if len(data) != self._frame_bytes:
                raise IOError("%s: frame %d is truncated (%d of %d bytes)" % (self._name, i, len(data), self._frame_bytes))
            yield i / self.frame_rate, self._frame_of(data, 0)
            i += 1
        self._file = None

    def frame(self, i):
        if self._offsets is None:
            raise TypeError("a Y4M stream cannot seek; this needs a file")
        return self._frame_of(self._map, self._offsets[i])

    def __call__(self, t):
        """the frame at time t: index int(fps * t + 1e-5), as the reference's Video reads it (video.py:466-486)"""
        i = int(self.frame_rate * t + 0.00001)
        if not 0 <= i < len(self):
            raise IOError("no frame at t = %.3f" % t)
        return self.frame(i)


def is_y4m(path):
    """by suffix, or by the first bytes of an existing file"""
    if str(path).lower().endswith(".y4m"):
        return True
    try:
        with open(path, "rb") as f:
            return f.read(len(MAGIC)) == MAGIC
    except (IOError, OSError):
        return False
