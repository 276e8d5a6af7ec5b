// ingest.hip -- frame staging: what the reference does per frame in Python -- `proc.stdout.read` into a fresh
// numpy array (video.py:368-401), an optional `cv2.resize` to the detection size (video.py:402-403, tracking.py:389-400), a second
// decode for `extract` (pyannote-face.py:261 vs :287) -- becomes:
//   - a ring of pinned host slots the decoder writes into (pvf_ingest_*); a slot goes to HBM with ONE asynchronous copy on a copy
//     stream of its own, so uploads run ahead of / beside the detector instead of in front of it;
//   - frames that carry a "ready" event: the compute stream waits for a frame's copy the first time a kernel is about to read it
//     (Ctx::frame), not when the copy is queued, so later frames keep streaming in while earlier ones are processed;
//   - the down-scaled detection frames made on the device from the staged frame (pvf_frame_resize: OpenCV's 8-bit bilinear,
//     restated), the full-size frame staying resident for `extract`: one decode, one upload, no host resize;
//   - slots that hold what a decoder really writes -- 8-bit YUV 4:2:0 / 4:2:2 / 4:4:4 planes (pvf_ingest_create_yuv) or a surface
//     already in HBM (pvf_frame_from_yuv, planar or NV12) -- and ONE kernel, yuv_to_rgb_k, that turns them into the RGB frame every
//     other kernel reads: half the bytes of RGB cross PCIe, the conversion the reference leaves to `ffmpeg -pix_fmt rgb24` on the CPU
//     (video.py:332-358) runs on the copy stream behind the frame's own upload.
#include "pvf_internal.h"
#include <cmath>

struct IngestRing {
    int h = 0, w = 0, depth = 0;
    uint8_t* host = nullptr;                 // depth * h * w * 3 bytes, pinned
    hipStream_t copy = nullptr;
    std::vector<hipEvent_t> done;            // last upload of each slot
    std::vector<char> busy;
    int next = 0;
    size_t slot_bytes = 0;                   // host bytes from one slot to the next
    // YUV rings (pvf_ingest_create_yuv): a slot holds the Y, U and V planes, tight; `stage` is its copy in HBM, one per slot, which
    // yuv_to_rgb_k reads on the copy stream (done[slot] is recorded behind the kernel, so both are free when acquire returns the slot)
    bool yuv = false;
    int layout = 0, flags = 0;
    uint8_t* stage = nullptr;                // depth * slot_bytes, device
};

// ---------------------------------------------------------------------------------------------------
// YUV -> RGB ("YUV to RGB"): 16.16 fixed point, chroma replicated.
//   C = ymul * Y + yoff                       (limited: 76309 * (Y - 16) + 32768; full: 65536 * Y + 32768)
//   R = clip8((C + crv * (V - 128)) >> 16)    G = clip8((C - cgu * (U - 128) - cgv * (V - 128)) >> 16)    B = clip8((C + cbu * (U - 128)) >> 16)
// |accumulator| < 2^26 for every input, so int32 holds it.  The constants are chosen on the host and passed by value.
struct YuvCoef { int32_t ymul, yoff, crv, cgu, cgv, cbu; };

static YuvCoef yuv_coef(int flags)
{
    const bool full = (flags & PVF_YUV_FULL_RANGE) != 0;
    int32_t m[4] = {104597, 132201, 25675, 53279};                      // crv, cbu, cgu, cgv: BT.601
    if (flags & PVF_YUV_BT709) { m[0] = 117504; m[1] = 138453; m[2] = 13954; m[3] = 34903; }
    if (full) for (int32_t& v : m) v = (v * 224) / 255;
    YuvCoef k;
    k.ymul = full ? 65536 : 76309;
    k.yoff = 32768 - (full ? 0 : 16 * 76309);
    k.crv = m[0]; k.cbu = m[1]; k.cgu = m[2]; k.cgv = m[3];
    return k;
}

template <int N> struct alignas(N) ByteVec { uint8_t b[N]; };          // N = 4, 8, 16: one dword / dwordx2 / dwordx4 access
struct alignas(4) Rgb8 { uint32_t d[6]; };                             // 8 RGB pixels

// clip8(v >> 16), written as clamp first, shift second: the same value ((v >> 16) floors, so it is monotonic in v), and not the
// shift-then-clamp form, which hipcc 7 fuses pairwise into v_ashr_pk_u8_i32 and then ORs the neighbouring bytes into -- on the
// MI355X that came back with bits above the two packed bytes set (B of pixel 0 and R of pixel 1 of every block read too high).
__device__ __forceinline__ uint32_t yuv_clip8(int v) { return (uint32_t)min(max(v, 0), 0xFFFFFF) >> 16; }

// One lane = 8 pixels of a row, times the 1 << SY rows that share its chroma samples.  Lanes of a wave take consecutive 8-pixel blocks,
// so a wave instruction reads 512 contiguous bytes of Y and writes 1536 contiguous bytes of RGB.
//   WIDE: every plane row and every RGB row starts on the boundary its vector access needs (checked on the host, yuv_launch): a block
//         that lies inside the row loads Y as one dwordx2, its chroma as one dword / dwordx2 / dwordx4 and stores six dwords of RGB per
//         row -- no byte access to global memory.  The row tail (w % 8 pixels) takes the byte path below.
//   otherwise (odd widths, tight RGB rows that start off a dword, unaligned surfaces): bytes throughout.
// CSTEP = 2: interleaved chroma (NV12), `u` and `v` one byte apart.
template <int SX, int SY, int CSTEP, bool WIDE>
__global__ void __launch_bounds__(256) yuv_to_rgb_k(const uint8_t* __restrict__ yp, int64_t y_pitch, const uint8_t* up, const uint8_t* vp,
                                                    int64_t c_pitch, uint8_t* __restrict__ out, int h, int w, int nbx, int n_lanes, YuvCoef k)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= n_lanes) return;
    const int cy = id / nbx, bx = id - cy * nbx;
    const int x0 = bx * 8, y0 = cy << SY;
    constexpr int NC = 8 >> SX;                                         // chroma samples of the block
    const uint8_t* urow = up + (int64_t)cy * c_pitch + (int64_t)(x0 >> SX) * CSTEP;
    const uint8_t* vrow = vp + (int64_t)cy * c_pitch + (int64_t)(x0 >> SX) * CSTEP;
    if (WIDE && x0 + 8 <= w) {
        int rv[NC], gg[NC], bu[NC];
        if (CSTEP == 1) {
            const ByteVec<NC> U = *reinterpret_cast<const ByteVec<NC>*>(urow);
            const ByteVec<NC> V = *reinterpret_cast<const ByteVec<NC>*>(vrow);
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const int u = (int)U.b[i] - 128, v = (int)V.b[i] - 128;
                rv[i] = k.crv * v; gg[i] = -k.cgu * u - k.cgv * v; bu[i] = k.cbu * u;
            }
        } else {
            const ByteVec<2 * NC> UV = *reinterpret_cast<const ByteVec<2 * NC>*>(urow);     // (WIDE and CSTEP == 2: v == u + 1)
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const int u = (int)UV.b[2 * i] - 128, v = (int)UV.b[2 * i + 1] - 128;
                rv[i] = k.crv * v; gg[i] = -k.cgu * u - k.cgv * v; bu[i] = k.cbu * u;
            }
        }
#pragma unroll
        for (int r = 0; r < (1 << SY); ++r) {
            const int y = y0 + r;
            if (y >= h) break;
            const ByteVec<8> Y = *reinterpret_cast<const ByteVec<8>*>(yp + (int64_t)y * y_pitch + x0);
            uint32_t px[24];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = k.ymul * (int)Y.b[i] + k.yoff, j = i >> SX;
                px[3 * i] = yuv_clip8(c + rv[j]);
                px[3 * i + 1] = yuv_clip8(c + gg[j]);
                px[3 * i + 2] = yuv_clip8(c + bu[j]);
            }
            Rgb8 o;
#pragma unroll
            for (int i = 0; i < 6; ++i) o.d[i] = px[4 * i] | (px[4 * i + 1] << 8) | (px[4 * i + 2] << 16) | (px[4 * i + 3] << 24);
            *reinterpret_cast<Rgb8*>(out + ((int64_t)y * w + x0) * 3) = o;
        }
        return;
    }
    const int n = min(8, w - x0);
    for (int r = 0; r < (1 << SY); ++r) {
        const int y = y0 + r;
        if (y >= h) break;
        const uint8_t* yrow = yp + (int64_t)y * y_pitch + x0;
        uint8_t* o = out + ((int64_t)y * w + x0) * 3;
        for (int i = 0; i < n; ++i) {
            const int j = (i >> SX) * CSTEP;
            const int u = (int)urow[j] - 128, v = (int)vrow[j] - 128;
            const int c = k.ymul * (int)yrow[i] + k.yoff;
            o[3 * i] = (uint8_t)yuv_clip8(c + k.crv * v);
            o[3 * i + 1] = (uint8_t)yuv_clip8(c - k.cgu * u - k.cgv * v);
            o[3 * i + 2] = (uint8_t)yuv_clip8(c + k.cbu * u);
        }
    }
}

static bool yuv_layout_shifts(int layout, int* sx, int* sy)
{
    switch (layout) {
        case 420: *sx = 1; *sy = 1; return true;
        case 422: *sx = 1; *sy = 0; return true;
        case 444: *sx = 0; *sy = 0; return true;
    }
    return false;
}

template <int SX, int SY, int CSTEP>
static void yuv_launch_as(bool wide, dim3 grid, hipStream_t s, const uint8_t* y, int64_t y_pitch, const uint8_t* u, const uint8_t* v, int64_t c_pitch,
                          uint8_t* out, int h, int w, int nbx, int n_lanes, const YuvCoef& k)
{
    if (wide) hipLaunchKernelGGL((yuv_to_rgb_k<SX, SY, CSTEP, true>), grid, dim3(256), 0, s, y, y_pitch, u, v, c_pitch, out, h, w, nbx, n_lanes, k);
    else hipLaunchKernelGGL((yuv_to_rgb_k<SX, SY, CSTEP, false>), grid, dim3(256), 0, s, y, y_pitch, u, v, c_pitch, out, h, w, nbx, n_lanes, k);
}

// planes and `out` (tight h * w * 3) in device memory; arguments already checked
static void yuv_launch(hipStream_t s, const uint8_t* y, int64_t y_pitch, const uint8_t* u, const uint8_t* v, int64_t c_pitch, int c_step,
                       uint8_t* out, int h, int w, int layout, int flags)
{
    int sx = 0, sy = 0;
    yuv_layout_shifts(layout, &sx, &sy);
    const int nbx = (w + 7) / 8, rows = (h + (1 << sy) - 1) >> sy;
    const int64_t lanes = (int64_t)nbx * rows;
    PVF_REQUIRE(lanes < ((int64_t)1 << 31), "yuv_to_rgb: frame too large for one launch");
    // the vector path: Y blocks on 8 bytes, the chroma bytes of a block on their own size, RGB rows on a dword
    const int64_t ca = (int64_t)(8 >> sx) * c_step;
    auto on = [](const void* p, int64_t a) { return (uintptr_t)p % (uintptr_t)a == 0; };
    const bool wide = on(y, 8) && y_pitch % 8 == 0 && on(u, ca) && c_pitch % ca == 0 && (c_step == 2 ? v == u + 1 : on(v, ca)) &&
                      on(out, 4) && ((int64_t)w * 3) % 4 == 0;
    const YuvCoef k = yuv_coef(flags);
    const dim3 grid((unsigned)((lanes + 255) / 256));
    const int key = layout * 10 + c_step;
    switch (key) {
        case 4201: yuv_launch_as<1, 1, 1>(wide, grid, s, y, y_pitch, u, v, c_pitch, out, h, w, nbx, (int)lanes, k); break;
        case 4202: yuv_launch_as<1, 1, 2>(wide, grid, s, y, y_pitch, u, v, c_pitch, out, h, w, nbx, (int)lanes, k); break;
        case 4221: yuv_launch_as<1, 0, 1>(wide, grid, s, y, y_pitch, u, v, c_pitch, out, h, w, nbx, (int)lanes, k); break;
        case 4222: yuv_launch_as<1, 0, 2>(wide, grid, s, y, y_pitch, u, v, c_pitch, out, h, w, nbx, (int)lanes, k); break;
        case 4441: yuv_launch_as<0, 0, 1>(wide, grid, s, y, y_pitch, u, v, c_pitch, out, h, w, nbx, (int)lanes, k); break;
        case 4442: yuv_launch_as<0, 0, 2>(wide, grid, s, y, y_pitch, u, v, c_pitch, out, h, w, nbx, (int)lanes, k); break;
        default: throw PvfError("yuv_to_rgb: unknown layout");
    }
    HIP_CHECK(hipGetLastError());
}

// what every YUV entry point refuses: sizes the tight RGB frame (int32 offsets in the kernels that read it) cannot hold
static void yuv_require_size(int h, int w, int layout, int flags, const char* who)
{
    int sx, sy;
    PVF_REQUIRE(h > 0 && w > 0, std::string(who) + ": bad frame size");
    PVF_REQUIRE(yuv_layout_shifts(layout, &sx, &sy), std::string(who) + ": layout must be 420, 422 or 444");
    PVF_REQUIRE((flags & ~(PVF_YUV_BT709 | PVF_YUV_FULL_RANGE)) == 0, std::string(who) + ": unknown flags");
    PVF_REQUIRE((int64_t)h * w * 3 <= (int64_t)INT32_MAX, std::string(who) + ": h * w * 3 exceeds what a frame can index");
}

static std::unordered_map<uint64_t, std::unique_ptr<IngestRing>>& rings(Ctx* c)
{
    return *reinterpret_cast<std::unordered_map<uint64_t, std::unique_ptr<IngestRing>>*>(c->ingest_rings);
}

void ingest_free_all(Ctx* c)
{
    if (!c->ingest_rings) return;
    auto* m = reinterpret_cast<std::unordered_map<uint64_t, std::unique_ptr<IngestRing>>*>(c->ingest_rings);
    for (auto& kv : *m) {
        IngestRing& r = *kv.second;
        if (r.copy) { (void)hipStreamSynchronize(r.copy); (void)hipStreamDestroy(r.copy); }
        for (auto e : r.done) if (e) (void)hipEventDestroy(e);
        if (r.host) (void)hipHostFree(r.host);
        if (r.stage) (void)hipFree(r.stage);
    }
    delete m;
    c->ingest_rings = nullptr;
}

#define API_BEGIN try {
#define API_END                                                        \
    return 0;                                                          \
    }                                                                  \
    catch (const std::exception& e) { pvf_set_error(e.what()); return -1; } \
    catch (...) { pvf_set_error("unknown error"); return -2; }

extern "C" int32_t pvf_ingest_create(pvf_handle h, int32_t fh, int32_t fw, int32_t depth, pvf_handle* ring)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    HIP_CHECK(hipSetDevice(c->device));
    PVF_REQUIRE(fh > 0 && fw > 0 && depth > 0 && ring, "pvf_ingest_create: bad arguments");
    std::unique_ptr<IngestRing> r(new IngestRing());
    r->h = fh; r->w = fw; r->depth = depth;
    r->slot_bytes = (size_t)fh * fw * 3;
    HIP_CHECK(hipHostMalloc((void**)&r->host, (size_t)depth * fh * fw * 3, hipHostMallocDefault));
    HIP_CHECK(hipStreamCreateWithFlags(&r->copy, hipStreamNonBlocking));
    r->done.assign(depth, nullptr);
    r->busy.assign(depth, 0);
    for (int i = 0; i < depth; ++i) HIP_CHECK(hipEventCreateWithFlags(&r->done[i], hipEventDisableTiming));
    const uint64_t id = c->next_id++;
    std::lock_guard<std::mutex> lk(c->frames_mu);
    if (!c->ingest_rings) c->ingest_rings = new std::unordered_map<uint64_t, std::unique_ptr<IngestRing>>();
    rings(c)[id] = std::move(r);
    *ring = id;
    API_END
}

extern "C" int32_t pvf_ingest_destroy(pvf_handle h, pvf_handle ring)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    HIP_CHECK(hipSetDevice(c->device));
    std::unique_ptr<IngestRing> own;
    {
        std::lock_guard<std::mutex> lk(c->frames_mu);
        PVF_REQUIRE(c->ingest_rings && rings(c).count(ring), "unknown ingest ring");
        own = std::move(rings(c)[ring]);
        rings(c).erase(ring);
    }
    IngestRing& r = *own;
    HIP_CHECK(hipStreamSynchronize(r.copy));
    (void)hipStreamDestroy(r.copy);
    for (auto e : r.done) (void)hipEventDestroy(e);
    (void)hipHostFree(r.host);
    if (r.stage) (void)hipFree(r.stage);
    API_END
}

// next slot in ring order; returns once the previous upload from that slot has left the host buffer
extern "C" int32_t pvf_ingest_acquire(pvf_handle h, pvf_handle ring, int32_t* slot, uint8_t** host_rgb)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    IngestRing* rp = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->frames_mu);
        PVF_REQUIRE(c->ingest_rings && rings(c).count(ring) && slot && host_rgb, "pvf_ingest_acquire: bad arguments");
        rp = rings(c)[ring].get();
    }
    IngestRing& r = *rp;                        // one producer per ring: its slot bookkeeping needs no lock
    const int s = r.next;
    r.next = (r.next + 1) % r.depth;
    if (r.busy[s]) { HIP_CHECK(hipEventSynchronize(r.done[s])); r.busy[s] = 0; }
    *slot = s;
    *host_rgb = r.host + (size_t)s * r.slot_bytes;
    API_END
}

// block until every upload queued on the ring's copy stream has finished (measurement / shutdown)
extern "C" int32_t pvf_ingest_wait(pvf_handle h, pvf_handle ring)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    hipStream_t copy = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->frames_mu);
        PVF_REQUIRE(c->ingest_rings && rings(c).count(ring), "unknown ingest ring");
        copy = rings(c)[ring]->copy;
    }
    HIP_CHECK(hipStreamSynchronize(copy));
    API_END
}

// queue the upload of a filled slot; the frame handle is valid at once (kernels that read it wait for the copy on the device)
extern "C" int32_t pvf_ingest_submit(pvf_handle h, pvf_handle ring, int32_t slot, pvf_handle* frame)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    HIP_CHECK(hipSetDevice(c->device));
    IngestRing* rp = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->frames_mu);
        PVF_REQUIRE(c->ingest_rings && rings(c).count(ring) && frame, "pvf_ingest_submit: bad arguments");
        rp = rings(c)[ring].get();
    }
    IngestRing& r = *rp;
    PVF_REQUIRE(slot >= 0 && slot < r.depth, "pvf_ingest_submit: slot out of range");
    const size_t bytes = (size_t)r.h * r.w * 3;
    uint8_t* d = c->take_frame_buffer(bytes, r.copy);   // a recycled buffer: the copy waits (on the device) for the kernels that still read it
    if (r.yuv) {
        // the planes as they are to the slot's staging buffer, then the conversion, both on the copy stream; `done` behind the kernel
        int sx = 0, sy = 0;
        yuv_layout_shifts(r.layout, &sx, &sy);
        const int64_t cw = (r.w + (1 << sx) - 1) >> sx, ch = (r.h + (1 << sy) - 1) >> sy;
        const size_t planes = (size_t)r.h * r.w + 2 * (size_t)(cw * ch);
        uint8_t* st = r.stage + (size_t)slot * r.slot_bytes;
        HIP_CHECK(hipMemcpyAsync(st, r.host + (size_t)slot * r.slot_bytes, planes, hipMemcpyHostToDevice, r.copy));
        const uint8_t* u = st + (size_t)r.h * r.w;
        yuv_launch(r.copy, st, r.w, u, u + cw * ch, cw, 1, d, r.h, r.w, r.layout, r.flags);
    } else {
        HIP_CHECK(hipMemcpyAsync(d, r.host + (size_t)slot * bytes, bytes, hipMemcpyHostToDevice, r.copy));
    }
    HIP_CHECK(hipEventRecord(r.done[slot], r.copy));
    r.busy[slot] = 1;
    Frame f; f.d = d; f.h = r.h; f.w = r.w; f.owned = true; f.pooled = true;
    HIP_CHECK(hipEventCreateWithFlags(&f.ready, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(f.ready, r.copy));
    *frame = c->add_frame(f);
    API_END
}

// A ring whose slots hold one planar 8-bit YUV frame: Y (h x w), then U, then V (ceil(w / 2^sx) x ceil(h / 2^sy) each), tight.  Slots
// are 256 bytes apart or a multiple, so that a plane's alignment does not depend on the slot.
extern "C" int32_t pvf_ingest_create_yuv(pvf_handle h, int32_t fh, int32_t fw, int32_t depth, int32_t layout, int32_t flags, pvf_handle* ring)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    HIP_CHECK(hipSetDevice(c->device));
    PVF_REQUIRE(depth > 0 && ring, "pvf_ingest_create_yuv: bad arguments");
    yuv_require_size(fh, fw, layout, flags, "pvf_ingest_create_yuv");
    int sx = 0, sy = 0;
    yuv_layout_shifts(layout, &sx, &sy);
    const size_t cw = ((size_t)fw + (1 << sx) - 1) >> sx, ch = ((size_t)fh + (1 << sy) - 1) >> sy;
    std::unique_ptr<IngestRing> r(new IngestRing());
    r->h = fh; r->w = fw; r->depth = depth;
    r->yuv = true; r->layout = layout; r->flags = flags;
    r->slot_bytes = ((size_t)fh * fw + 2 * cw * ch + 255) / 256 * 256;
    HIP_CHECK(hipHostMalloc((void**)&r->host, (size_t)depth * r->slot_bytes, hipHostMallocDefault));
    if (hipMalloc((void**)&r->stage, (size_t)depth * r->slot_bytes) != hipSuccess) {
        (void)hipHostFree(r->host);
        throw PvfError("pvf_ingest_create_yuv: out of device memory for the staging buffers");
    }
    HIP_CHECK(hipStreamCreateWithFlags(&r->copy, hipStreamNonBlocking));
    r->done.assign(depth, nullptr);
    r->busy.assign(depth, 0);
    for (int i = 0; i < depth; ++i) HIP_CHECK(hipEventCreateWithFlags(&r->done[i], hipEventDisableTiming));
    const uint64_t id = c->next_id++;
    std::lock_guard<std::mutex> lk(c->frames_mu);
    if (!c->ingest_rings) c->ingest_rings = new std::unordered_map<uint64_t, std::unique_ptr<IngestRing>>();
    rings(c)[id] = std::move(r);
    *ring = id;
    API_END
}

// Planes that already lie in HBM (a hardware decoder's surface).  The kernel runs where pvf_frame_resize runs, on the detector's
// stream under its lock, and the call returns when it has finished: the frame is complete for either stream (no `ready` event to wait
// for), and the caller may hand the surface back to its decoder at once -- the contract pvf_frame_upload has for a device source.
extern "C" int32_t pvf_frame_from_yuv(pvf_handle h, const uint8_t* y, int64_t y_pitch, const uint8_t* u, const uint8_t* v, int64_t c_pitch,
                                      int32_t c_step, int32_t fh, int32_t fw, int32_t layout, int32_t flags, pvf_handle* out)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    std::lock_guard<std::recursive_mutex> det_lock(c->det_mu);
    HIP_CHECK(hipSetDevice(c->device));
    PVF_REQUIRE(out && y && u && v, "pvf_frame_from_yuv: null plane or result pointer");
    yuv_require_size(fh, fw, layout, flags, "pvf_frame_from_yuv");
    PVF_REQUIRE(c_step == 1 || c_step == 2, "pvf_frame_from_yuv: c_step must be 1 (planar) or 2 (interleaved)");
    PVF_REQUIRE(c_step == 1 || v == u + 1 || u == v + 1, "pvf_frame_from_yuv: interleaved chroma wants u and v one byte apart");
    int sx = 0, sy = 0;
    yuv_layout_shifts(layout, &sx, &sy);
    const int64_t cw = ((int64_t)fw + (1 << sx) - 1) >> sx;
    PVF_REQUIRE(y_pitch >= fw, "pvf_frame_from_yuv: luma pitch smaller than a row");
    PVF_REQUIRE(c_pitch >= cw * c_step, "pvf_frame_from_yuv: chroma pitch smaller than a row");
    const size_t bytes = (size_t)fh * fw * 3;
    uint8_t* d = c->take_frame_buffer(bytes, c->det_stream);
    hipEvent_t ev = nullptr;
    try {
        yuv_launch(c->det_stream, y, y_pitch, u, v, c_pitch, c_step, d, fh, fw, layout, flags);
        HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(ev, c->det_stream));
        HIP_CHECK(hipEventSynchronize(ev));
    } catch (...) {
        if (ev) (void)hipEventDestroy(ev);
        (void)hipFree(d);
        throw;
    }
    (void)hipEventDestroy(ev);
    Frame f; f.d = d; f.h = fh; f.w = fw; f.owned = true; f.pooled = true;
    *out = c->add_frame(f);
    API_END
}

// ---------------------------------------------------------------------------------------------------
// cv2.resize(frame, (out_w, out_h)) with the default INTER_LINEAR on 8-bit images (reference video.py:402-403), [EXT] restated from
// OpenCV's resize.cpp: pixel-centre mapping fx = (dx + 0.5) * scale - 0.5, source index clamped to the image, 11-bit coefficients
// (cvRound(f * 2048) as int16), horizontal pass in int32, vertical pass
//   dst = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2
// The coefficient tables are built on the host (a few thousand entries), one lane = one output pixel (3 channels).
ResizeTab linear_table(int in, int out)
{
    ResizeTab t;
    t.idx.resize(out); t.coef.resize((size_t)out * 2);
    const double scale = (double)in / out;
    for (int d = 0; d < out; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= s;
        if (s < 0) { f = 0; s = 0; }
        if (s >= in - 1) { f = 0; s = in - 1; }
        t.idx[d] = s;
        auto cv_round = [](float v) { return (int)std::nearbyint(v); };     // round half to even, like cvRound
        t.coef[2 * d] = (int16_t)cv_round((1.f - f) * 2048.f);
        t.coef[2 * d + 1] = (int16_t)cv_round(f * 2048.f);
    }
    return t;
}

__global__ void __launch_bounds__(256) cv_resize_linear_k(const uint8_t* __restrict__ in, int ih, int iw, uint8_t* __restrict__ out, int oh, int ow,
                                                          const int32_t* __restrict__ xi, const int16_t* __restrict__ xc,
                                                          const int32_t* __restrict__ yi, const int16_t* __restrict__ yc)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= ow) return;
    const int sx = xi[x], sy = yi[y];
    const int sx1 = min(sx + 1, iw - 1), sy1 = min(sy + 1, ih - 1);
    const int a0 = xc[2 * x], a1 = xc[2 * x + 1], b0 = yc[2 * y], b1 = yc[2 * y + 1];
    const uint8_t* r0 = in + (size_t)sy * iw * 3;
    const uint8_t* r1 = in + (size_t)sy1 * iw * 3;
    uint8_t* o = out + ((size_t)y * ow + x) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int S0 = r0[3 * sx + k] * a0 + r0[3 * sx1 + k] * a1;
        const int S1 = r1[3 * sx + k] * a0 + r1[3 * sx1 + k] * a1;
        o[k] = (uint8_t)((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2);
    }
}

extern "C" int32_t pvf_frame_resize(pvf_handle h, pvf_handle frame, int32_t out_w, int32_t out_h, pvf_handle* out)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    std::lock_guard<std::recursive_mutex> det_lock(c->det_mu);       // the --min-size copies are made where the detector runs
    HIP_CHECK(hipSetDevice(c->device));
    PVF_REQUIRE(out && out_w > 0 && out_h > 0, "pvf_frame_resize: bad arguments");
    const Frame f = c->frame(frame);
    // coefficient tables: built and uploaded once per (source size, target size), in a buffer of their own (--min-size asks for the same
    // resize for every frame of a video)
    const std::vector<int> key{f.w, f.h, out_w, out_h};
    auto it = c->resize_tabs.find(key);
    if (it == c->resize_tabs.end()) {
        const ResizeTab tx = linear_table(f.w, out_w), ty = linear_table(f.h, out_h);
        std::unique_ptr<DevBuf> tab(new DevBuf());
        tab->ensure((size_t)(out_w + out_h) * (4 + 4));
        uint8_t* q = tab->as<uint8_t>();
        HIP_CHECK(hipMemcpy(q, tx.idx.data(), (size_t)out_w * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(q + (size_t)out_w * 4, ty.idx.data(), (size_t)out_h * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(q + (size_t)(out_w + out_h) * 4, tx.coef.data(), (size_t)out_w * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(q + (size_t)(out_w + out_h) * 4 + (size_t)out_w * 4, ty.coef.data(), (size_t)out_h * 4, hipMemcpyHostToDevice));
        it = c->resize_tabs.emplace(key, std::move(tab)).first;
    }
    uint8_t* p = it->second->as<uint8_t>();
    const int32_t* dxi = (const int32_t*)p; const int32_t* dyi = dxi + out_w;
    const int16_t* dxc = (const int16_t*)(dyi + out_h); const int16_t* dyc = dxc + 2 * out_w;
    const size_t bytes = (size_t)out_h * out_w * 3;
    uint8_t* d = c->take_frame_buffer(bytes, c->det_stream);
    hipLaunchKernelGGL(cv_resize_linear_k, dim3((out_w + 255) / 256, out_h), dim3(256), 0, c->det_stream, f.d, f.h, f.w, d, out_h, out_w, dxi, dxc, dyi, dyc);
    HIP_CHECK(hipGetLastError());
    Frame g; g.d = d; g.h = out_h; g.w = out_w; g.owned = true; g.pooled = true;
    // the copy is written on the detector stream; a consumer on the main stream (tracker start / update, landmarks, shot) must come
    // after it whoever calls in whatever order: Ctx::frame() makes both streams wait for `ready` on first use and destroys it
    HIP_CHECK(hipEventCreateWithFlags(&g.ready, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(g.ready, c->det_stream));
    *out = c->add_frame(g);
    API_END
}
