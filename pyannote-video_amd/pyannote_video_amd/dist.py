"""Multi-GPU: one process per GPU; a long video is cut into contiguous frame ranges at shot boundaries, every rank runs
detect -> track -> extract on its range with no data-path collective, then ONE exchange step: an all-gather of the
per-rank (128-D float32 embedding, time, track id) rows over RCCL/xGMI, followed by a single global clustering.

Track ids: the reference numbers tracks in yield order over the whole video (pyannote-face.py:261) and tracks never span
shots (tracking.py:359-362,410-417), so global id = local id + exclusive prefix sum of the per-rank track counts.

What travels (round 4): 528 bytes per face -- the 128 float32 values the embedder produced, the float64 time, the int32 track id --
instead of 130 float64 columns; the gathered rows STAY IN HBM: the clustering's float64 table (np.round(x, 5) of every row, in (track,
time) order) is made from them on the device (pvf_pair_upper_rows_f32), every rank computes the upper-triangle rows of the track-pair
matrix for a share of the tracks of equal triangle AREA, those rows are all-gathered device to device, mirrored and agglomerated
(pvf_cluster_upper).  Only the (time, track id) columns come back to the host, where the row order is decided.

ONE collective path: `libpvface_dist.so` (include/pvface_dist.h: RCCL behind a C ABI) whenever the job runs on GPUs over nccl; a
communicator that cannot be set up is an ERROR.  The torch.distributed collectives are used only when PVF_DIST_COLLECTIVE=torch asks
for them (CPU tests over gloo; `bench.py --oversubscribe`, where several ranks share one device and cannot form an RCCL communicator)."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DIST_LIB_PATH = os.path.join(_HERE, "libpvface_dist.so")
_DIST_SIGS = {
    "pvfd_last_error": (C.c_char_p, []),
    "pvfd_unique_id": (C.c_int32, [C.c_void_p]),
    "pvfd_comm_create": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "pvfd_comm_destroy": (C.c_int32, [C.c_uint64]),
    "pvfd_allgather_counts": (C.c_int32, [C.c_uint64, C.c_int64, C.c_void_p]),
    "pvfd_allgatherv_dev": (C.c_int32, [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pvfd_debug_stall": (C.c_int32, [C.c_uint64, C.c_int32]),
}
DIST_EXPORTS = sorted(_DIST_SIGS)
_dist_lib = None

ROW_BYTES = 528           # one face on the wire: float32[128] | float64 time | int32 local track id | int32 zero


def dist_lib():
    """libpvface_dist.so (include/pvface_dist.h): the RCCL all-gather behind a C ABI"""
    global _dist_lib
    if _dist_lib is None:
        l = C.CDLL(DIST_LIB_PATH)
        for name, (res, args) in _DIST_SIGS.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _dist_lib = l
    return _dist_lib


class RcclRows(object):
    """one communicator of libpvface_dist.so per process: all-gather of byte rows in device memory, a different count per rank"""
    name = "libpvface_dist"

    def __init__(self, device, rank, world, unique_id):
        self.l = dist_lib()
        self.rank, self.world, self.device = rank, world, int(device)
        h = C.c_uint64(0)
        idb = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._check(self.l.pvfd_comm_create(int(device), int(rank), int(world), idb, C.byref(h)))
        self.h = h.value

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError("libpvface_dist: " + self.l.pvfd_last_error().decode("utf-8", "replace"))

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        l = dist_lib()
        if l.pvfd_unique_id(buf) != 0:
            raise RuntimeError("libpvface_dist: " + l.pvfd_last_error().decode("utf-8", "replace"))
        return bytes(buf)

    def counts(self, n):
        out = np.zeros(self.world, np.int64)
        self._check(self.l.pvfd_allgather_counts(self.h, int(n), out.ctypes.data_as(C.c_void_p)))
        return [int(c) for c in out]

    def allgather(self, t):
        """t: torch uint8 [n, k] on this communicator's device (n may differ per rank, k must not) -> (all rows in rank order, a uint8
        [N, k] tensor on the device; the row count of every rank).  Device to device: nothing passes through host memory."""
        import torch
        assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2
        t = t.contiguous()
        n, k = int(t.shape[0]), int(t.shape[1])
        counts = self.counts(n)
        out = torch.empty((max(sum(counts), 1), k), dtype=torch.uint8, device=t.device)
        nbytes = np.asarray([c * k for c in counts], np.int64)
        torch.cuda.synchronize(t.device)                  # whoever produced t (another library's stream, torch's) is done
        self._check(self.l.pvfd_allgatherv_dev(self.h, C.c_void_p(t.data_ptr() if n else 0), nbytes.ctypes.data_as(C.c_void_p), C.c_void_p(out.data_ptr())))
        return out[:sum(counts)], counts

    def stall(self, milliseconds):
        """the watchdog's test entry: a spinning kernel in place of a collective (include/pvface_dist.h: pvfd_debug_stall)"""
        self._check(self.l.pvfd_debug_stall(self.h, int(milliseconds)))

    def close(self):
        if getattr(self, "h", None):
            self.l.pvfd_comm_destroy(self.h)
            self.h = None


class TorchRows(object):
    """the same exchange over torch.distributed (PVF_DIST_COLLECTIVE=torch only): gloo on CPU tensors (tensors on a device travel through
    host memory), nccl on device tensors"""
    name = "torch"

    def __init__(self):
        import torch.distributed as dist
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.on_host = dist.get_backend() != "nccl"

    def counts(self, n):
        import torch
        import torch.distributed as dist
        dev = "cpu" if self.on_host else "cuda"
        c = torch.tensor([int(n)], dtype=torch.int64, device=dev)
        allc = [torch.zeros_like(c) for _ in range(self.world)]
        dist.all_gather(allc, c)
        return [int(x[0]) for x in allc]

    def allgather(self, t):
        import torch
        import torch.distributed as dist
        home = t.device
        n, k = int(t.shape[0]), int(t.shape[1])
        counts = self.counts(n)
        cap = max(max(counts), 1)
        work = "cpu" if self.on_host else home
        pay = torch.zeros((cap, k), dtype=torch.uint8, device=work)
        if n:
            pay[:n] = t.to(work)
        parts = [torch.zeros_like(pay) for _ in range(self.world)]
        dist.all_gather(parts, pay)
        out = torch.cat([parts[r][:counts[r]] for r in range(self.world)]) if sum(counts) else torch.zeros((0, k), dtype=torch.uint8, device=work)
        return out.to(home), counts

    def close(self):
        pass


_exchange = {"tried": False, "comm": None}


def exchange():
    """The process's exchange step, or None for a single process.  Over nccl: the RCCL communicator of libpvface_dist.so -- if it
    cannot be set up on every rank the job FAILS (no silent change of collective).  PVF_DIST_COLLECTIVE=torch selects the
    torch.distributed collectives explicitly; a job on another backend than nccl (gloo) must say so."""
    import torch.distributed as dist
    if _exchange["tried"]:
        return _exchange["comm"]
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return None
    _exchange["tried"] = True
    want = os.environ.get("PVF_DIST_COLLECTIVE", "rccl")
    if want == "torch":
        _exchange["comm"] = TorchRows()
        return _exchange["comm"]
    if dist.get_backend() != "nccl":
        raise RuntimeError("pyannote_video_amd.dist: the job runs over the %r backend, where libpvface_dist.so's RCCL communicator cannot be used; "
                           "set PVF_DIST_COLLECTIVE=torch to ask for the torch.distributed collectives explicitly" % dist.get_backend())
    import torch
    rank, world = dist.get_rank(), dist.get_world_size()
    err = None
    try:
        box = [RcclRows.unique_id() if rank == 0 else None]
    except Exception as e:      # noqa: BLE001 -- reported below, on every rank
        box, err = [None], e
    dist.broadcast_object_list(box, src=0)
    comm = None
    try:
        if box[0] is None:
            raise RuntimeError("rank 0 could not create a communicator id")
        comm = RcclRows(torch.cuda.current_device(), rank, world, box[0])
    except Exception as e:      # noqa: BLE001
        err = err or e
    flag = torch.tensor([1 if comm is not None else 0], dtype=torch.int32, device="cuda")
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)           # every rank learns whether all of them have the communicator
    if int(flag.item()) != 1:
        if comm is not None:
            comm.close()
        raise RuntimeError("libpvface_dist.so: the RCCL communicator could not be set up on every rank (%s); "
                           "PVF_DIST_COLLECTIVE=torch selects the torch.distributed collectives explicitly" % (err if err is not None else "another rank failed"))
    _exchange["comm"] = comm
    return comm


def preflight(log=None, payload_bytes=1 << 20):
    """Make the first multi-GPU run diagnose itself BEFORE any video is rendered: the communicator, one exchange of counts, and one
    all-gather of about `payload_bytes` in UNEVEN shares (rank r sends r + 1 parts of world (world + 1) / 2) whose every byte is checked
    on arrival -- each step under the collectives' watchdog (PVF_DIST_TIMEOUT_S, 30 s here unless set), each reported per rank through
    `log` (a callable taking one string; default: stderr).  Returns the report as a dict; raises on the first failure, naming the step."""
    import sys
    import time
    import torch
    import torch.distributed as dist
    if log is None:
        def log(msg):
            sys.stderr.write(msg + "\n"); sys.stderr.flush()
    had = os.environ.get("PVF_DIST_TIMEOUT_S")
    if had is None:
        os.environ["PVF_DIST_TIMEOUT_S"] = "30"
    rep = {"world": 1, "rank": 0, "collective": "none"}
    try:
        t0 = time.perf_counter()
        ex = exchange()
        if ex is None:
            log("preflight: a single process, no exchange step")
            return rep
        rank, world = ex.rank, ex.world
        rep.update(world=world, rank=rank, collective=ex.name, communicator_s=round(time.perf_counter() - t0, 3))
        log("preflight rank %d/%d: communicator up (%s) in %.3f s" % (rank, world, ex.name, rep["communicator_s"]))
        t0 = time.perf_counter()
        counts = ex.counts(rank + 1)
        if counts != list(range(1, world + 1)):
            raise RuntimeError("preflight rank %d: the count exchange returned %r, expected %r" % (rank, counts, list(range(1, world + 1))))
        rep["counts_s"] = round(time.perf_counter() - t0, 4)
        log("preflight rank %d/%d: counts exchanged in %.4f s" % (rank, world, rep["counts_s"]))
        part = max(16, int(payload_bytes) // (world * (world + 1) // 2) // 16 * 16)
        on_gpu = dist.get_backend() == "nccl"
        dev = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
        mine = (torch.arange((rank + 1) * part // 16 * 16, dtype=torch.int64, device=dev) * 37 + rank * 101) % 251
        t0 = time.perf_counter()
        got, rows = ex.allgather(mine.to(torch.uint8).reshape(-1, 16))
        if on_gpu:
            torch.cuda.synchronize()
        rep["allgatherv_s"] = round(time.perf_counter() - t0, 4)
        want_rows = [(r + 1) * part // 16 for r in range(world)]
        if rows != want_rows:
            raise RuntimeError("preflight rank %d: share sizes %r arrived, expected %r" % (rank, rows, want_rows))
        got = got.reshape(-1).to(torch.int64)
        off = 0
        for r in range(world):
            n = want_rows[r] * 16
            want = (torch.arange(n, dtype=torch.int64, device=got.device) * 37 + r * 101) % 251
            if not bool(torch.equal(got[off:off + n], want)):
                bad = int((got[off:off + n] != want).nonzero()[0])
                raise RuntimeError("preflight rank %d: rank %d's share (%d bytes at offset %d) arrived damaged, first at byte %d" % (rank, r, n, off, bad))
            off += n
        rep["allgatherv_bytes"] = int(off)
        log("preflight rank %d/%d: %d bytes in uneven shares %r gathered and verified in %.4f s" % (rank, world, off, [w * 16 for w in want_rows], rep["allgatherv_s"]))
        return rep
    finally:
        if had is None:
            os.environ.pop("PVF_DIST_TIMEOUT_S", None)


def collective_name():
    """which exchange step a multi-GPU run uses: 'libpvface_dist' (RCCL behind the C ABI), 'torch' (asked for with
    PVF_DIST_COLLECTIVE=torch) or 'none' (a single process)"""
    ex = exchange()
    return "none" if ex is None else ex.name


def shard_shots(shot_ranges, world_size):
    """Contiguous groups of shots per rank, balancing frame counts greedily. shot_ranges: [(i0, i1)]. -> [(s0, s1)] per rank"""
    n = len(shot_ranges)
    total = sum(b - a for a, b in shot_ranges)
    out, s = [], 0
    acc = 0
    for r in range(world_size):
        if r == world_size - 1:
            out.append((s, n))
            break
        target = total * (r + 1) / float(world_size)
        e = s
        while e < n - (world_size - 1 - r) and (acc + (shot_ranges[e][1] - shot_ranges[e][0]) <= target or e == s):
            acc += shot_ranges[e][1] - shot_ranges[e][0]
            e += 1
        out.append((s, e))
        s = e
    return out


def shard_clips(n_clips, world_size, frames=None):
    """The clip farm (BASELINE.json configs[3]: independent videos, one result each, no exchange step): which clips every rank takes.
    Without `frames`: round robin (clips of one length).  With `frames` = frame count per clip: longest first onto the rank with the least
    work so far (ties: lowest rank), each rank's clips then in input order.  -> [[clip indices] per rank]; every clip exactly once."""
    out = [[] for _ in range(world_size)]
    if frames is None:
        for i in range(n_clips):
            out[i % world_size].append(i)
        return out
    if len(frames) != n_clips:
        raise ValueError("shard_clips: one frame count per clip")
    load = [0] * world_size
    for i in sorted(range(n_clips), key=lambda k: (-int(frames[k]), k)):
        r = min(range(world_size), key=lambda q: (load[q], q))
        out[r].append(i)
        load[r] += int(frames[i])
    return [sorted(c) for c in out]


class GatheredEmb(object):
    """the float32 descriptor rows of all ranks after the exchange: `rows` (numpy float32 [n, 128] on a CPU job, runtime.DeviceRows in HBM
    otherwise) and `index`: row k of the result is rows[index[k]] (the rows themselves are never moved: the clustering gathers on the
    device)"""

    def __init__(self, rows, index=None):
        self.rows, self.index = rows, index

    def __len__(self):
        return len(self.index) if self.index is not None else (self.rows.n if hasattr(self.rows, "n") else len(self.rows))

    def numpy(self):
        """float32 [N, 128] in result order (tests, debugging: downloads the rows)"""
        rows = self.rows
        if hasattr(rows, "keep") and rows.keep is not None:
            a = rows.keep[:, :512].contiguous().cpu().numpy().view(np.float32).reshape(-1, 128)
        else:
            a = np.asarray(rows, np.float32).reshape(-1, 128)
        return a if self.index is None else a[self.index]


def _wire_rows(face_T, face_id, emb):
    n = len(face_T)
    buf = np.zeros((n, ROW_BYTES), np.uint8)
    if n:
        buf[:, :512] = np.ascontiguousarray(emb, np.float32).reshape(n, 128).view(np.uint8)
        buf[:, 512:520] = np.ascontiguousarray(face_T, np.float64).reshape(n, 1).view(np.uint8)
        buf[:, 520:524] = np.ascontiguousarray(face_id, np.int32).reshape(n, 1).view(np.uint8)
    return buf


def gather_rows(face_T, face_id, emb, n_tracks, device=None, file_T=None, file_id=None):
    """All-gather variable-length rows from every rank.  emb: this rank's float32 descriptors [n, 128] (FacePipeline.run's
    "embeddings").  Returns (T, global track id, GatheredEmb) in rank order -- or in the reference's file order, below -- and the
    per-rank track offsets.

    device: where the gathered rows live (a torch device; None: the current CUDA device when the job runs on GPUs, host memory on a CPU
    job).  file_T / file_id: this rank's share of the track table in file order (FacePipeline.run(..., reorder=False)["file_T"/"file_id"]).
    When given, the shares are gathered too (16 bytes per row) and the rows are put into the order the reference's `extract` writes
    them for the WHOLE video (formats.file_order: pandas' unstable sort of the complete table decides the order of the faces of one
    frame), so a sharded run returns exactly the rows of a single-process run."""
    from . import formats
    ex = exchange()
    if ex is None:
        T, ids = np.asarray(face_T, np.float64), np.asarray(face_id, np.int64)
        X = GatheredEmb(np.ascontiguousarray(emb, np.float32).reshape(-1, 128))
        if file_T is not None and len(T):
            perm = formats.file_order(T, ids, file_T, file_id)
            T, ids, X.index = T[perm], ids[perm], np.asarray(perm, np.int64)
        return T, ids, X, [0]
    import torch
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    device = torch.device(device)
    # ---- who has how many tracks (global id = local id + the tracks of the ranks before)
    tracks = ex.counts(int(n_tracks))
    offsets = [0]
    for k in tracks[:-1]:
        offsets.append(offsets[-1] + k)
    # ---- the faces: one 528-byte row each, gathered into device memory, where the descriptors stay
    mine = torch.from_numpy(_wire_rows(face_T, face_id, emb)).to(device)
    G, counts = ex.allgather(mine)
    N = int(G.shape[0])
    meta = G[:, 512:ROW_BYTES].contiguous().cpu().numpy() if N else np.zeros((0, 16), np.uint8)
    T = meta[:, :8].copy().view(np.float64).reshape(-1)
    gid = meta[:, 8:12].copy().view(np.int32).reshape(-1).astype(np.int64)
    o = 0
    for r, c in enumerate(counts):
        gid[o:o + c] += offsets[r]
        o += c
    if G.is_cuda:
        from .runtime import DeviceRows
        X = GatheredEmb(DeviceRows(G.data_ptr(), N, ROW_BYTES, keep=G))
    else:
        X = GatheredEmb(G[:, :512].contiguous().numpy().view(np.float32).reshape(-1, 128))
    if file_T is not None:
        m = len(file_T)
        ft = np.zeros((m, 16), np.uint8)
        if m:
            ft[:, :8] = np.ascontiguousarray(file_T, np.float64).reshape(m, 1).view(np.uint8)
            ft[:, 8:12] = np.ascontiguousarray(file_id, np.int32).reshape(m, 1).view(np.uint8)
        F, fcounts = ex.allgather(torch.from_numpy(ft).to(device))
        F = F.cpu().numpy()
        fT = F[:, :8].copy().view(np.float64).reshape(-1)
        fid = F[:, 8:12].copy().view(np.int32).reshape(-1).astype(np.int64)
        o = 0
        for r, c in enumerate(fcounts):
            fid[o:o + c] += offsets[r]
            o += c
        if N:
            perm = np.asarray(formats.file_order(T, gid, fT, fid), np.int64)
            T, gid, X.index = T[perm], gid[perm], perm
    return T, gid, X, offsets


class DistanceShard(object):
    """Splits the pairwise distances of the global clustering over the ranks: every rank already holds all gathered rows and computes
    the upper-triangle entries D[i][j], j > i, of a contiguous share of the tracks i; one all-gather of those rows (T x T doubles in
    total, device to device) gives every rank the complete upper triangle, which is mirrored (clustering.py:111-112) and agglomerated
    identically everywhere.  Shares are cut by equal triangle AREA -- the pairs (row a, row b > a) a rank computes -- not by equal
    rows: the first rows have all the others to their right, the last ones almost nothing.  Without the split each rank would repeat
    the whole O(N^2) step, which grows with the square of the number of GPUs under weak scaling."""

    def __init__(self, rank, world, device=None):
        self.rank, self.world, self.device = rank, world, device

    def bounds(self, row_start):
        """track cuts [world + 1]: rank r takes the tracks [cuts[r], cuts[r + 1]).  The pairs above row a number a N - a^2 / 2 of the
        N^2 / 2 in total, so rank r's share ends at the row a = N (1 - sqrt(1 - r / world)), moved down to a track boundary."""
        n = int(row_start[-1])
        T = len(row_start) - 1
        cuts = [0]
        for r in range(1, self.world):
            target = n * (1.0 - np.sqrt(1.0 - r / float(self.world)))
            t = cuts[-1]
            while t < T and row_start[t + 1] <= target:
                t += 1
            cuts.append(t)
        cuts.append(T)
        return cuts

    def track_range(self, row_start):
        cuts = self.bounds(row_start)
        return cuts[self.rank], cuts[self.rank + 1]

    def assemble(self, U_mine, row_start):
        """U_mine: this rank's rows [(t1 - t0), T] (numpy) -> the assembled T x T upper triangle (numpy); the host form of cluster()"""
        import torch
        T = len(row_start) - 1
        ex = exchange()
        dev = self.device if self.device is not None else ("cpu" if (isinstance(ex, TorchRows) and ex.on_host) else "cuda")
        t = torch.from_numpy(np.ascontiguousarray(U_mine, np.float64).reshape(-1, T).view(np.uint8).reshape(-1, T * 8)).to(dev)
        G, counts = ex.allgather(t)
        cuts = self.bounds(row_start)
        assert counts == [cuts[r + 1] - cuts[r] for r in range(self.world)] and int(G.shape[0]) == T
        return G.cpu().numpy().view(np.float64).reshape(T, T)

    def _upper(self, ctx, emb, order, row_start, decimals):
        """this rank's rows of the upper triangle from the float32 rows (table made on the device), all-gathered: the assembled T x T
        upper triangle, numpy for rows in host memory, DeviceRows (device to device) otherwise"""
        import torch
        from .runtime import DeviceRows
        T = len(row_start) - 1
        t0, t1 = self.track_range(row_start)
        ex = exchange()
        if not isinstance(emb, DeviceRows):
            # rows in host memory (a CPU-resident gather): the host form
            return self.assemble(ctx.pair_upper_rows_f32(emb, order, row_start, t0, t1, decimals=decimals), row_start)
        dev = emb.keep.device if emb.keep is not None else torch.device("cuda", torch.cuda.current_device())
        mine = torch.empty((max(t1 - t0, 0), T), dtype=torch.float64, device=dev)
        if t1 > t0:
            ctx.pair_upper_rows_f32(emb, order, row_start, t0, t1, decimals=decimals, out=DeviceRows.of_tensor(mine))
        G, counts = ex.allgather(mine.view(torch.uint8).reshape(-1, T * 8))
        cuts = self.bounds(row_start)
        assert counts == [cuts[r + 1] - cuts[r] for r in range(self.world)] and int(G.shape[0]) == T
        return DeviceRows(G.data_ptr(), T, T * 8, keep=G)

    def cluster(self, ctx, emb, order, row_start, cut, decimals=5):
        """the split clustering with everything in HBM: upper-triangle rows, all-gather, mirror + agglomeration -> (labels, merge log)"""
        return ctx.cluster_upper(self._upper(ctx, emb, order, row_start, decimals), row_start, cut)

    def cluster_cooccur(self, ctx, emb, order, row_start, cut, decimals=5, *, extent):
        """the same with the do-not-cooccur constraint (extent: float64 [T, 2]): every rank stamps the assembled matrix itself
        (pvf_cluster_upper_cooccur), so all ranks still agglomerate one matrix -> (labels, merge log, n_blocked)"""
        return ctx.cluster_upper_cooccur(self._upper(ctx, emb, order, row_start, decimals), row_start, cut, extent)


def global_cluster(clustering, face_T, face_id, X):
    """single global clustering on the gathered rows (computed identically on every rank); X: what gather_rows returned (or float32
    rows [N, 128])"""
    if len(face_T) == 0:
        return {}
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and clustering.shard is None:
        clustering.shard = DistanceShard(dist.get_rank(), dist.get_world_size())
    if isinstance(X, GatheredEmb):
        return clustering.cluster_rows(face_T, face_id, X.rows, src_index=X.index)
    return clustering.cluster_rows(face_T, face_id, X)
