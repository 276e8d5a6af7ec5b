// render.hip -- the `demo` verb's pixels (DEMO.md): what the reference does per frame on the CPU -- cv2.resize to the demo height
// (video.py:402-403), cv2.putText / rectangle / line per face (pyannote-face.py:345-382), moviepy pushing RGB frames to ffmpeg
// (:405-413) -- becomes ONE kernel per batch of resident frames, render_k:
//   - OpenCV's 8-bit bilinear resize (the bytes of pvf_frame_resize), read straight from the resident RGB frame;
//   - the frame's primitives (rectangle outlines, lines, text in the project's 5 x 7 font) evaluated per pixel, in list order;
//   - RGB -> planar YUV 4:2:0 in 16.16 fixed point, a lane owning a 2 x 2 block so that chroma needs no second pass;
// The `redact` verb (REDACT.md) adds one thing that is not a per-pixel constant: a redacted pixel is the mean of its mosaic cell of
// the resized source picture.  redact_means_k reduces those cells into a table in front of render_k, on the same stream; render_k's
// REDACT instantiation takes a covered pixel's colour from the table.  A list without redactions runs the other instantiation, which
// is the kernel as it was, and launches no means kernel.
// and an egress ring (pvf_egress_*) that mirrors the ingest ring: pinned host slots of one planar output frame, the kernel on the
// context's stream, the device-to-host copy behind it on a copy stream of the ring's own, the host waiting per slot -- 1.5 bytes per
// output pixel cross PCIe, and rendering frame k + 1 overlaps the copy of frame k and the file write of frame k - 1.
#include "pvf_internal.h"
#include "render_font.h"
#include "render_prims.h"

static_assert(sizeof(pvf_prim) == 32, "pvf_prim is 8 x int32");

struct RenderArgs {
    const uint8_t* const* src;      // [n] resident RGB frames, ih x iw each
    int ih, iw, oh, ow;
    const int32_t* xi; const int16_t* xc; const int32_t* yi; const int16_t* yc;       // the resize tables of (iw, ih) -> (ow, oh)
    const int32_t* start;           // [n + 1]: frame f draws prims[start[f] .. start[f + 1])
    const pvf_prim* prims;
    const uint8_t* text;
    uint8_t* out;                   // [n] planar frames, out_stride bytes apart (Y, U, V tight), or null
    int64_t out_stride;
    uint8_t* rgb;                   // [n][oh][ow][3] the drawn picture before colour conversion, or null (pvf_debug_render_rgb)
    RenderCoef k;
    const uint32_t* table;          // cell means of the call's redactions (r | g << 8 | b << 16), a primitive's at its `reserved`
};

constexpr int R_TILE = 32;          // output pixels per block side: 16 x 16 lanes of 2 x 2 pixels
constexpr int R_CHUNK = 256;        // primitives culled and staged in LDS at a time

// one channel of one resized pixel: cv_resize_linear_k's arithmetic (DEMO.md "Resize").  r0, r1: the two source rows; o0, o1: the byte
// offsets of the two taps in a row; (a0, a1), (b0, b1): the column and row coefficients.  render_k and redact_means_k both call it.
__device__ __forceinline__ int resize_value(const uint8_t* __restrict__ r0, const uint8_t* __restrict__ r1, int o0, int o1, int a0, int a1, int b0, int b1)
{
    const int S0 = r0[o0] * a0 + r0[o1] * a1;
    const int S1 = r1[o0] * a0 + r1[o1] * a1;
    return ((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2) & 255;
}

// the colour of output pixel (X, Y), which the redaction covers (so it lies in the box and in the frame).  REDACT.md "Modes"
__device__ __forceinline__ uint32_t redact_colour(const pvf_prim& p, const uint32_t* __restrict__ table, int X, int Y, int ow, int oh)
{
    const int mode = (p.colour >> 24) & 6;
    if (mode == PVF_REDACT_FILL) return p.colour;
    const int cell = p.scale, nx = (p.c - p.a + cell) / cell;             // ceil(W / cell)
    const uint32_t* __restrict__ m = table + p.reserved;
    const int dx = X - p.a, dy = Y - p.b;
    if (mode == PVF_REDACT_MOSAIC) return m[(dy / cell) * nx + dx / cell];
    // smooth: bilinear between nominal cell centres, the neighbours clamped to the cells that hold a pixel of the frame
    const int ilo = (max(p.a, 0) - p.a) / cell, ihi = (min(p.c, ow - 1) - p.a) / cell;
    const int jlo = (max(p.b, 0) - p.b) / cell, jhi = (min(p.d, oh - 1) - p.b) / cell;
    const int ux = 2 * dx + 1 - cell, uy = 2 * dy + 1 - cell;            // >= 1 - cell
    const int i0 = (ux + 2 * cell) / (2 * cell) - 1, j0 = (uy + 2 * cell) / (2 * cell) - 1;          // floor(u / (2 cell)), u >= -2 cell
    const uint32_t fx = (uint32_t)(ux - 2 * cell * i0), fy = (uint32_t)(uy - 2 * cell * j0);
    const uint32_t wx0 = 2 * cell - fx, wy0 = 2 * cell - fy;
    const int ia = min(max(i0, ilo), ihi), ib = min(max(i0 + 1, ilo), ihi);
    const int ja = min(max(j0, jlo), jhi), jb = min(max(j0 + 1, jlo), jhi);
    const uint32_t m00 = m[ja * nx + ia], m01 = m[ja * nx + ib], m10 = m[jb * nx + ia], m11 = m[jb * nx + ib];
    const uint32_t w00 = wy0 * wx0, w01 = wy0 * fx, w10 = fy * wx0, w11 = fy * fx;                    // they sum to 4 cell^2 <= 2^24
    const uint32_t den = 4u * cell * cell, half = den >> 1;
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // uint32: at cell = 2048 the numerator reaches 255 * 2^24 + 2^23 = 4 286 578 688 < 2^32
        const uint32_t num = w00 * ((m00 >> (8 * k)) & 255) + w01 * ((m01 >> (8 * k)) & 255) + w10 * ((m10 >> (8 * k)) & 255) +
                             w11 * ((m11 >> (8 * k)) & 255) + half;
        out |= (num / den) << (8 * k);
    }
    return out;
}

// grid (ceil(ow / 32), ceil(oh / 32), n frames), 256 lanes: lane (tx, ty) owns output pixels (2 tx .. 2 tx + 1) x (2 ty .. 2 ty + 1) of the
// tile.  Lanes of a wave cover 32 x 8 output pixels: their source reads fall into a few rows of the frame, their Y stores into 8 rows of
// 32 contiguous bytes.  A pixel beyond the last column / row of an odd frame is its neighbour replicated (it only feeds the chroma).
// REDACT: the list holds redactions (the host sets it from the list); without it the kernel is what it was before they existed.
template <bool REDACT>
__global__ void __launch_bounds__(256) render_k(const RenderArgs a)
{
    __shared__ pvf_prim s_prim[R_CHUNK];
    __shared__ int s_wave[4];
    const int f = blockIdx.z, tid = threadIdx.x;
    const int X0 = blockIdx.x * R_TILE + 2 * (tid & 15), Y0 = blockIdx.y * R_TILE + 2 * (tid >> 4);
    const bool active = X0 < a.ow && Y0 < a.oh;
    int px[2], py[2];
    px[0] = min(X0, a.ow - 1); px[1] = min(X0 + 1, a.ow - 1);
    py[0] = min(Y0, a.oh - 1); py[1] = min(Y0 + 1, a.oh - 1);
    int R[4], G[4], B[4];                                                  // pixel 2 * j + i = (px[i], py[j])
    if (active) {
        const uint8_t* __restrict__ in = a.src[f];
        int sx[2], sx1[2], a0[2], a1[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            sx[i] = a.xi[px[i]]; sx1[i] = min(sx[i] + 1, a.iw - 1);
            a0[i] = a.xc[2 * px[i]]; a1[i] = a.xc[2 * px[i] + 1];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int sy = a.yi[py[j]], sy1 = min(sy + 1, a.ih - 1);
            const int b0 = a.yc[2 * py[j]], b1 = a.yc[2 * py[j] + 1];
            const uint8_t* r0 = in + (size_t)sy * a.iw * 3;
            const uint8_t* r1 = in + (size_t)sy1 * a.iw * 3;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int v[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) v[k] = resize_value(r0, r1, 3 * sx[i] + k, 3 * sx1[i] + k, a0[i], a1[i], b0, b1);
                R[2 * j + i] = v[0]; G[2 * j + i] = v[1]; B[2 * j + i] = v[2];
            }
        }
    }
    // the frame's primitives, R_CHUNK at a time: every lane tests one against the tile's bounding box, the survivors go to LDS in list
    // order (ballot + popcount ranks), then every lane walks the staged few for its four pixels.  Later primitives overwrite earlier ones.
    const int p0 = a.start[f], p1 = a.start[f + 1];
    const int64_t tx0 = (int64_t)blockIdx.x * R_TILE, ty0 = (int64_t)blockIdx.y * R_TILE;
    const int64_t tx1 = min(tx0 + R_TILE - 1, (int64_t)a.ow - 1), ty1 = min(ty0 + R_TILE - 1, (int64_t)a.oh - 1);
    for (int base = p0; base < p1; base += R_CHUNK) {
        const int i = base + tid;
        pvf_prim p;
        bool hit = false;
        if (i < p1) {
            const int4* q = reinterpret_cast<const int4*>(a.prims + i);
            const int4 lo = q[0], hi = q[1];
            p.type = lo.x; p.a = lo.y; p.b = lo.z; p.c = lo.w; p.d = hi.x; p.colour = (uint32_t)hi.y; p.scale = hi.z; p.reserved = REDACT ? hi.w : 0;
            hit = prim_meets<REDACT>(p, tx0, ty0, tx1, ty1);
        }
        const uint64_t m = __ballot(hit);
        const int lane = tid & 63, w = tid >> 6;
        if (lane == 0) s_wave[w] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { if (k < w) off += s_wave[k]; total += s_wave[k]; }
        if (hit) s_prim[off + __popcll(m & ((1ull << lane) - 1))] = p;
        __syncthreads();
        if (active) {
            for (int j = 0; j < total; ++j) {
                const pvf_prim q = s_prim[j];
                if constexpr (REDACT)
                    if (q.type == PVF_PRIM_REDACT) {                       // the colour is the pixel's own: its cell's mean
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (prim_covers<true>(q, a.text, px[e & 1], py[e >> 1])) {
                                const uint32_t c = redact_colour(q, a.table, px[e & 1], py[e >> 1], a.ow, a.oh);
                                R[e] = c & 255; G[e] = (c >> 8) & 255; B[e] = (c >> 16) & 255;
                            }
                        continue;
                    }
                const int cr = q.colour & 255, cg = (q.colour >> 8) & 255, cb = (q.colour >> 16) & 255;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (prim_covers<false>(q, a.text, px[e & 1], py[e >> 1])) { R[e] = cr; G[e] = cg; B[e] = cb; }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    const bool in_x1 = X0 + 1 < a.ow, in_y1 = Y0 + 1 < a.oh;
    if (a.rgb) {
        uint8_t* o = a.rgb + (size_t)f * a.oh * a.ow * 3;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (((e & 1) && !in_x1) || ((e >> 1) && !in_y1)) continue;
            uint8_t* q = o + ((size_t)py[e >> 1] * a.ow + px[e & 1]) * 3;
            q[0] = (uint8_t)R[e]; q[1] = (uint8_t)G[e]; q[2] = (uint8_t)B[e];
        }
    }
    if (!a.out) return;
    uint8_t* yp = a.out + (size_t)f * a.out_stride;
    const int cw = (a.ow + 1) >> 1, ch = (a.oh + 1) >> 1;
    uint8_t* up = yp + (size_t)a.oh * a.ow;
    uint8_t* vp = up + (size_t)cw * ch;
    int sr = 0, sg = 0, sb = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int y0v = yuv_luma(a.k, R[2 * j], G[2 * j], B[2 * j]);
        const int y1v = yuv_luma(a.k, R[2 * j + 1], G[2 * j + 1], B[2 * j + 1]);
        sr += R[2 * j] + R[2 * j + 1]; sg += G[2 * j] + G[2 * j + 1]; sb += B[2 * j] + B[2 * j + 1];
        if (j == 1 && !in_y1) continue;
        uint8_t* q = yp + (size_t)(Y0 + j) * a.ow + X0;
        if (in_x1 && ((uintptr_t)q & 1) == 0) *reinterpret_cast<uint16_t*>(q) = (uint16_t)(y0v | (y1v << 8));
        else { q[0] = (uint8_t)y0v; if (in_x1) q[1] = (uint8_t)y1v; }
    }
    const size_t ci = (size_t)(Y0 >> 1) * cw + (X0 >> 1);
    up[ci] = (uint8_t)yuv_chroma(a.k.u, sr, sg, sb);
    vp[ci] = (uint8_t)yuv_chroma(a.k.v, sr, sg, sb);
}

// ---- the cell means of a call's redactions (REDACT.md "Cells") --------------------------------------------------------------------
// One record per redaction that has a table, in list order over the frames of the call.  Blocks [block, next record's block) belong to
// it; `per` cells a block: 4 (a wave per cell) or 1 (the block per cell, for cells of more than R_WAVE_CELL pixels).
struct RedactRec { int32_t block, frame, prim, per; };
static_assert(sizeof(RedactRec) == 16, "RedactRec is read as one int4");
constexpr int R_WAVE_CELL = 4096;   // pixels of a cell up to which one wave sums it (64 pixels a lane)

struct MeansArgs {
    const uint8_t* const* src;
    int ih, iw, oh, ow;
    const int32_t* xi; const int16_t* xc; const int32_t* yi; const int16_t* yc;
    const pvf_prim* prims;          // the device copy of the list: `reserved` holds the table offset
    const RedactRec* recs;
    int n_recs;
    uint32_t* table;
};

// grid (sum of ceil(cells / per) over the records), 256 lanes.  A block finds its record by bisection on the block prefix, a wave (or the
// block) its cell; lanes walk the cell's pixels inside the frame row-major, take the resized value through resize_value and sum in
// uint32 (255 * 2048 * 2048 < 2^31); integer addition is exact in any order, so the reduction order is free.  A cell without a pixel
// in the frame reads 0.
__global__ void __launch_bounds__(256) redact_means_k(const MeansArgs a)
{
    __shared__ uint32_t s_sum[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lo = 0, hi = a.n_recs - 1;
    while (lo < hi) {                                                      // the last record whose first block is not beyond this one
        const int mid = (lo + hi + 1) >> 1;
        if (a.recs[mid].block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int4 rec = *reinterpret_cast<const int4*>(a.recs + lo);          // (block, frame, prim, per)
    const int4* pq = reinterpret_cast<const int4*>(a.prims + rec.z);
    const int4 plo = pq[0], phi = pq[1];
    const int l = plo.y, t = plo.z, r = plo.w, b = phi.x, cell = phi.z;
    const int nx = (r - l + cell) / cell, ny = (b - t + cell) / cell, cells = nx * ny;
    const bool whole = rec.w == 1;                                         // the block per cell
    const int c = ((int)blockIdx.x - rec.x) * rec.w + (whole ? 0 : wave);
    uint32_t sr = 0, sg = 0, sb = 0;
    int n = 0;
    if (c < cells) {
        const int j = c / nx, i = c - j * nx;
        const int xa = max(l + i * cell, 0), xb = min(min(l + (i + 1) * cell - 1, r), a.ow - 1);
        const int ya = max(t + j * cell, 0), yb = min(min(t + (j + 1) * cell - 1, b), a.oh - 1);
        const int cw = xb - xa + 1, chh = yb - ya + 1;
        if (cw > 0 && chh > 0) {
            n = cw * chh;
            const uint8_t* __restrict__ in = a.src[rec.y];
            for (int q = whole ? tid : lane; q < n; q += whole ? 256 : 64) {
                const int yy = q / cw, X = xa + (q - yy * cw), Y = ya + yy;
                const int sx = a.xi[X], sx1 = min(sx + 1, a.iw - 1), a0 = a.xc[2 * X], a1 = a.xc[2 * X + 1];
                const int sy = a.yi[Y], sy1 = min(sy + 1, a.ih - 1), b0 = a.yc[2 * Y], b1 = a.yc[2 * Y + 1];
                const uint8_t* r0 = in + (size_t)sy * a.iw * 3;
                const uint8_t* r1 = in + (size_t)sy1 * a.iw * 3;
                sr += resize_value(r0, r1, 3 * sx, 3 * sx1, a0, a1, b0, b1);
                sg += resize_value(r0, r1, 3 * sx + 1, 3 * sx1 + 1, a0, a1, b0, b1);
                sb += resize_value(r0, r1, 3 * sx + 2, 3 * sx1 + 2, a0, a1, b0, b1);
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { sr += __shfl_xor(sr, d); sg += __shfl_xor(sg, d); sb += __shfl_xor(sb, d); }
    if (lane == 0) { s_sum[wave][0] = sr; s_sum[wave][1] = sg; s_sum[wave][2] = sb; }
    __syncthreads();
    if (lane != 0 || c >= cells || (whole && wave != 0)) return;
    if (whole) {
        sr = s_sum[0][0] + s_sum[1][0] + s_sum[2][0] + s_sum[3][0];
        sg = s_sum[0][1] + s_sum[1][1] + s_sum[2][1] + s_sum[3][1];
        sb = s_sum[0][2] + s_sum[1][2] + s_sum[2][2] + s_sum[3][2];
    }
    uint32_t out = 0;
    if (n > 0) { const uint32_t h = (uint32_t)n >> 1, un = (uint32_t)n; out = (sr + h) / un | ((sg + h) / un) << 8 | ((sb + h) / un) << 16; }
    a.table[phi.w + c] = out;
}

// ---------------------------------------------------------------------------------------------------
struct RenderTabs { DevBuf buf; const int32_t* xi; const int32_t* yi; const int16_t* xc; const int16_t* yc; };

struct EgressRing {
    int w = 0, h = 0, depth = 0, flags = 0;
    size_t frame_bytes = 0, slot_bytes = 0;      // slots 256 bytes apart or a multiple
    uint8_t* host = nullptr;                     // depth * slot_bytes, pinned
    uint8_t* dev = nullptr;                      // depth * slot_bytes: what the kernel writes, the copy stream reads
    hipStream_t copy = nullptr;
    std::vector<hipEvent_t> rendered, done;      // kernel of the slot finished (context stream) / its copy reached the host (copy stream)
    std::vector<char> state;                     // 0 free, 1 in flight, 2 handed to the host
    std::vector<std::unique_ptr<DevBuf>> meta;   // the slot's frame pointer, list bounds, primitives and text on the device
    std::mutex mu;                               // `state`: a writer thread waits and gives back while another submits
    int next = 0;
};

struct RenderState {
    // by (in_w, in_h, out_w, out_h).  A cache of its own, not Ctx::resize_tabs: that one belongs to the detector side (det_mu), and a
    // render call must not queue behind a detector batch to look a table up
    std::map<std::vector<int>, std::unique_ptr<RenderTabs>> tabs;
    DevBuf meta, out;
    std::unordered_map<uint64_t, std::unique_ptr<EgressRing>> rings;
};

static RenderState& rstate(Ctx* c)
{
    static std::mutex mu;                // (made on first use, by whichever entry point comes first)
    std::lock_guard<std::mutex> lk(mu);
    if (!c->render_state) c->render_state = new RenderState();
    return *reinterpret_cast<RenderState*>(c->render_state);
}

static void egress_free(EgressRing& r)
{
    if (r.copy) { (void)hipStreamSynchronize(r.copy); (void)hipStreamDestroy(r.copy); }
    for (auto e : r.rendered) if (e) (void)hipEventDestroy(e);
    for (auto e : r.done) if (e) (void)hipEventDestroy(e);
    if (r.host) (void)hipHostFree(r.host);
    if (r.dev) (void)hipFree(r.dev);
}

void render_free_all(Ctx* c)
{
    if (!c->render_state) return;
    RenderState* s = reinterpret_cast<RenderState*>(c->render_state);
    for (auto& kv : s->rings) egress_free(*kv.second);
    delete s;
    c->render_state = nullptr;
}

static size_t up16(size_t v) { return (v + 15) / 16 * 16; }

static void render_require_output(int ow, int oh, int flags, const char* who)
{
    PVF_REQUIRE(ow >= 2 && oh >= 2, std::string(who) + ": the output is at least 2 x 2");
    PVF_REQUIRE((int64_t)ow * oh * 3 <= (int64_t)INT32_MAX, std::string(who) + ": output too large");
    PVF_REQUIRE((flags & ~(PVF_YUV_BT709 | PVF_YUV_FULL_RANGE)) == 0, std::string(who) + ": unknown flags");
}

// where render_launch left the call's cell means (device memory of `meta`, valid until its next use) and how many cells there are
struct RenderTable { const uint32_t* d; int64_t cells; };

// Checks the lists (nothing the kernel indexes with is taken on trust), uploads them behind the context's stream and launches.
// frames: one size; start: [n + 1] (null: no primitives at all); d_out / d_rgb: device memory or null.  api_mu held.
// means_only: the means kernel alone (pvf_debug_redact_means).
static RenderTable render_launch(Ctx* c, const std::vector<Frame>& frames, int ow, int oh, int flags, const int32_t* start, const pvf_prim* prims,
                          const uint8_t* text, int64_t text_bytes, DevBuf& meta, uint8_t* d_out, int64_t out_stride, uint8_t* d_rgb, const char* who,
                                 bool means_only = false)
{
    const std::string w(who);
    const int n = (int)frames.size();
    PVF_REQUIRE(n > 0, w + ": no frames");
    for (const Frame& f : frames) PVF_REQUIRE(f.h == frames[0].h && f.w == frames[0].w, w + ": the frames of one call have one size");
    PVF_REQUIRE(text_bytes >= 0 && text_bytes <= PVF_RENDER_MAX_TEXT, w + ": more text bytes than PVF_RENDER_MAX_TEXT");
    PVF_REQUIRE(text || text_bytes == 0, w + ": null text pool");
    int64_t total = 0;
    if (start) {
        PVF_REQUIRE(start[0] == 0, w + ": start[0] must be 0");
        for (int i = 0; i < n; ++i) {
            PVF_REQUIRE(start[i + 1] >= start[i], w + ": start must not decrease");
            PVF_REQUIRE(start[i + 1] - start[i] <= PVF_RENDER_MAX_PRIMS, w + ": more primitives on one frame than PVF_RENDER_MAX_PRIMS");
        }
        total = start[n];
    }
    PVF_REQUIRE(prims || total == 0, w + ": null primitive list");
    bool has_redact = false;
    for (int64_t i = 0; i < total; ++i) {
        const pvf_prim& p = prims[i];
        PVF_REQUIRE(p.type == PVF_PRIM_RECT || p.type == PVF_PRIM_LINE || p.type == PVF_PRIM_TEXT || p.type == PVF_PRIM_REDACT,
                    w + ": unknown primitive type");
        has_redact = has_redact || p.type == PVF_PRIM_REDACT;
        if (p.type != PVF_PRIM_TEXT) continue;
        PVF_REQUIRE(p.d >= 0 && p.d <= PVF_RENDER_MAX_RUN, w + ": a text run longer than PVF_RENDER_MAX_RUN bytes");
        PVF_REQUIRE(p.c >= 0 && (int64_t)p.c + p.d <= text_bytes, w + ": a text run outside the text pool");
        PVF_REQUIRE(p.scale >= 1 && p.scale <= PVF_RENDER_MAX_SCALE, w + ": text scale outside 1 .. PVF_RENDER_MAX_SCALE");
    }
    // the redactions (REDACT.md "Limits"): their table offsets, and the block prefix the means kernel finds its work by
    std::vector<RedactRec> recs;
    std::vector<std::pair<int64_t, int32_t>> offsets;          // (index into prims, table offset)
    int64_t cells_total = 0, blocks = 0;
    for (int f = 0; has_redact && f < n; ++f)
        for (int64_t i = start[f]; i < start[f + 1]; ++i) {
            const pvf_prim& p = prims[i];
            if (p.type != PVF_PRIM_REDACT) continue;
            const int64_t lim = PVF_REDACT_MAX_COORD;
            PVF_REQUIRE(p.a >= -lim && p.a <= lim && p.b >= -lim && p.b <= lim && p.c >= -lim && p.c <= lim && p.d >= -lim && p.d <= lim,
                        w + ": a redaction coordinate beyond PVF_REDACT_MAX_COORD");
            const uint32_t fl = p.colour >> 24;
            PVF_REQUIRE((fl & ~7u) == 0 && (fl & 6u) != 6u, w + ": unknown redaction flags");
            PVF_REQUIRE(p.scale >= 1 && p.scale <= PVF_REDACT_MAX_CELL, w + ": a redaction cell outside 1 .. PVF_REDACT_MAX_CELL");
            const int64_t W = (int64_t)p.c - p.a + 1, H = (int64_t)p.d - p.b + 1;
            if (W < 1 || H < 1) continue;                       // draws nothing
            PVF_REQUIRE(W <= PVF_REDACT_MAX_SIDE && H <= PVF_REDACT_MAX_SIDE, w + ": a redaction side beyond PVF_REDACT_MAX_SIDE");
            const int64_t cell = p.scale, cells = ((W + cell - 1) / cell) * ((H + cell - 1) / cell);
            PVF_REQUIRE(cells <= PVF_REDACT_MAX_CELLS, w + ": more cells in a redaction than PVF_REDACT_MAX_CELLS");
            if ((fl & 6u) == PVF_REDACT_FILL) continue;         // no table
            PVF_REQUIRE(cells_total + cells <= PVF_REDACT_MAX_TABLE, w + ": more redaction cells in one call than PVF_REDACT_MAX_TABLE");
            const int per = std::min(cell, W) * std::min(cell, H) > R_WAVE_CELL ? 1 : 4;
            recs.push_back(RedactRec{(int32_t)blocks, f, (int32_t)i, per});
            offsets.emplace_back(i, (int32_t)cells_total);
            cells_total += cells;
            blocks += (cells + per - 1) / per;
        }
    RenderState& st = rstate(c);
    const Frame& f0 = frames[0];
    const std::vector<int> key{f0.w, f0.h, ow, oh};
    auto it = st.tabs.find(key);
    if (it == st.tabs.end()) {
        const ResizeTab tx = linear_table(f0.w, ow), ty = linear_table(f0.h, oh);
        std::unique_ptr<RenderTabs> t(new RenderTabs());
        t->buf.ensure((size_t)(ow + oh) * 8);
        uint8_t* q = t->buf.as<uint8_t>();
        t->xi = (const int32_t*)q; t->yi = t->xi + ow;
        t->xc = (const int16_t*)(t->yi + oh); t->yc = t->xc + 2 * ow;
        HIP_CHECK(hipMemcpy((void*)t->xi, tx.idx.data(), (size_t)ow * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy((void*)t->yi, ty.idx.data(), (size_t)oh * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy((void*)t->xc, tx.coef.data(), (size_t)ow * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy((void*)t->yc, ty.coef.data(), (size_t)oh * 4, hipMemcpyHostToDevice));
        it = st.tabs.emplace(key, std::move(t)).first;
    }
    const RenderTabs& tab = *it->second;
    // one blob: frame pointers, list bounds, primitives (16-byte aligned: the kernel reads them as two dwordx4), text
    const size_t o_start = up16((size_t)n * 8), o_prims = o_start + up16((size_t)(n + 1) * 4);
    // ... the redaction records; behind what is uploaded, in the same buffer, the table the means kernel fills
    const size_t o_text = o_prims + (size_t)total * sizeof(pvf_prim), o_recs = up16(o_text + (size_t)text_bytes + 1);
    const size_t bytes = o_recs + recs.size() * sizeof(RedactRec), o_table = bytes;
    meta.ensure(o_table + (size_t)cells_total * 4);
    uint8_t* hb = (uint8_t*)c->stage.take(bytes);
    for (int i = 0; i < n; ++i) reinterpret_cast<const uint8_t**>(hb)[i] = frames[i].d;
    int32_t* hs = reinterpret_cast<int32_t*>(hb + o_start);
    for (int i = 0; i <= n; ++i) hs[i] = start ? start[i] : 0;
    if (total) memcpy(hb + o_prims, prims, (size_t)total * sizeof(pvf_prim));
    if (text_bytes) memcpy(hb + o_text, text, (size_t)text_bytes);
    for (int64_t i = 0; has_redact && i < total; ++i) {         // `reserved` is the library's: the table offset, 0 where there is no table
        pvf_prim& p = reinterpret_cast<pvf_prim*>(hb + o_prims)[i];
        if (p.type == PVF_PRIM_REDACT) p.reserved = 0;
    }
    for (const auto& o : offsets) reinterpret_cast<pvf_prim*>(hb + o_prims)[o.first].reserved = o.second;
    if (!recs.empty()) memcpy(hb + o_recs, recs.data(), recs.size() * sizeof(RedactRec));
    uint8_t* db = meta.as<uint8_t>();
    HIP_CHECK(hipMemcpyAsync(db, hb, bytes, hipMemcpyHostToDevice, c->stream));
    c->stage.sent(c->stream);
    RenderArgs a;
    a.src = reinterpret_cast<const uint8_t* const*>(db);
    a.ih = f0.h; a.iw = f0.w; a.oh = oh; a.ow = ow;
    a.xi = tab.xi; a.xc = tab.xc; a.yi = tab.yi; a.yc = tab.yc;
    a.start = reinterpret_cast<const int32_t*>(db + o_start);
    a.prims = reinterpret_cast<const pvf_prim*>(db + o_prims);
    a.text = db + o_text;
    a.out = d_out; a.out_stride = out_stride; a.rgb = d_rgb;
    a.k = render_coef(flags);
    a.table = reinterpret_cast<const uint32_t*>(db + o_table);
    const RenderTable made{a.table, cells_total};
    if (!recs.empty()) {
        MeansArgs m;
        m.src = a.src; m.ih = a.ih; m.iw = a.iw; m.oh = oh; m.ow = ow;
        m.xi = tab.xi; m.xc = tab.xc; m.yi = tab.yi; m.yc = tab.yc;
        m.prims = a.prims;
        m.recs = reinterpret_cast<const RedactRec*>(db + o_recs);
        m.n_recs = (int)recs.size();
        m.table = reinterpret_cast<uint32_t*>(db + o_table);
        ProfScope prof(c, "redact_means");
        hipLaunchKernelGGL(redact_means_k, dim3((unsigned)blocks), dim3(256), 0, c->stream, m);
        HIP_CHECK(hipGetLastError());
    }
    if (means_only) return made;
    ProfScope prof(c, "render");
    const dim3 grid((ow + R_TILE - 1) / R_TILE, (oh + R_TILE - 1) / R_TILE, n);
    if (has_redact) hipLaunchKernelGGL(render_k<true>, grid, dim3(256), 0, c->stream, a);
    else hipLaunchKernelGGL(render_k<false>, grid, dim3(256), 0, c->stream, a);
    HIP_CHECK(hipGetLastError());
    return made;
}

static size_t planar_bytes(int ow, int oh) { return (size_t)ow * oh + 2 * (size_t)((ow + 1) / 2) * ((oh + 1) / 2); }

#define API_BEGIN try {
#define API_END                                                        \
    return 0;                                                          \
    }                                                                  \
    catch (const std::exception& e) { pvf_set_error(e.what()); return -1; } \
    catch (...) { pvf_set_error("unknown error"); return -2; }

extern "C" int32_t pvf_render_batch(pvf_handle h, const pvf_handle* frames, int32_t n, int32_t out_w, int32_t out_h, int32_t flags,
                                    const int32_t* start, const pvf_prim* prims, const uint8_t* text, int64_t text_bytes,
                                    uint8_t* out, int32_t out_on_device)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    std::lock_guard<std::recursive_mutex> lock(c->api_mu);
    HIP_CHECK(hipSetDevice(c->device));
    PVF_REQUIRE(frames && n > 0 && n <= PVF_RENDER_MAX_BATCH && out, "pvf_render_batch: bad arguments");
    render_require_output(out_w, out_h, flags, "pvf_render_batch");
    std::vector<Frame> fs;
    for (int i = 0; i < n; ++i) fs.push_back(c->frame(frames[i]));
    RenderState& st = rstate(c);
    const size_t fb = planar_bytes(out_w, out_h);
    uint8_t* d = out;
    if (!out_on_device) { st.out.ensure(fb * n); d = st.out.as<uint8_t>(); }
    render_launch(c, fs, out_w, out_h, flags, start, prims, text, text_bytes, st.meta, d, (int64_t)fb, nullptr, "pvf_render_batch");
    if (!out_on_device) HIP_CHECK(hipMemcpyAsync(out, d, fb * n, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    API_END
}

extern "C" int32_t pvf_debug_render_rgb(pvf_handle h, pvf_handle frame, int32_t out_w, int32_t out_h, const pvf_prim* prims, int32_t n_prims,
                                        const uint8_t* text, int64_t text_bytes, uint8_t* rgb)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    std::lock_guard<std::recursive_mutex> lock(c->api_mu);
    HIP_CHECK(hipSetDevice(c->device));
    PVF_REQUIRE(rgb && n_prims >= 0, "pvf_debug_render_rgb: bad arguments");
    render_require_output(out_w, out_h, 0, "pvf_debug_render_rgb");
    std::vector<Frame> fs{c->frame(frame)};
    RenderState& st = rstate(c);
    const size_t bytes = (size_t)out_w * out_h * 3;
    st.out.ensure(bytes);
    const int32_t start[2] = {0, n_prims};
    render_launch(c, fs, out_w, out_h, 0, start, prims, text, text_bytes, st.meta, nullptr, 0, st.out.as<uint8_t>(), "pvf_debug_render_rgb");
    HIP_CHECK(hipMemcpyAsync(rgb, st.out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    API_END
}

extern "C" int32_t pvf_debug_redact_means(pvf_handle h, pvf_handle frame, int32_t out_w, int32_t out_h, const pvf_prim* prims, int32_t n_prims,
                                          uint8_t* means, int64_t capacity)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    std::lock_guard<std::recursive_mutex> lock(c->api_mu);
    HIP_CHECK(hipSetDevice(c->device));
    PVF_REQUIRE(n_prims >= 0 && capacity >= 0 && (means || capacity == 0), "pvf_debug_redact_means: bad arguments");
    render_require_output(out_w, out_h, 0, "pvf_debug_redact_means");
    std::vector<Frame> fs{c->frame(frame)};
    RenderState& st = rstate(c);
    PVF_REQUIRE(prims || n_prims == 0, "pvf_debug_redact_means: null primitive list");
    std::vector<pvf_prim> only;                                  // the list's redactions: the entry takes no text pool, so text stays out
    for (int32_t i = 0; i < n_prims; ++i) if (prims[i].type == PVF_PRIM_REDACT) only.push_back(prims[i]);
    const int32_t start[2] = {0, (int32_t)only.size()};
    const RenderTable tb = render_launch(c, fs, out_w, out_h, 0, start, only.data(), nullptr, 0, st.meta, nullptr, 0, nullptr,
                                         "pvf_debug_redact_means", true);
    PVF_REQUIRE(tb.cells * 3 <= capacity, "pvf_debug_redact_means: the tables need " + std::to_string(tb.cells * 3) + " bytes");
    std::vector<uint32_t> host((size_t)tb.cells);
    if (tb.cells) HIP_CHECK(hipMemcpyAsync(host.data(), tb.d, (size_t)tb.cells * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < tb.cells; ++i) {
        means[3 * i] = (uint8_t)(host[i] & 255); means[3 * i + 1] = (uint8_t)((host[i] >> 8) & 255); means[3 * i + 2] = (uint8_t)((host[i] >> 16) & 255);
    }
    API_END
}

static EgressRing* egress_find(Ctx* c, pvf_handle ring)
{
    std::lock_guard<std::mutex> lk(c->frames_mu);
    PVF_REQUIRE(c->render_state && rstate(c).rings.count(ring), "unknown egress ring");
    return rstate(c).rings[ring].get();
}

extern "C" int32_t pvf_egress_create(pvf_handle h, int32_t out_w, int32_t out_h, int32_t depth, int32_t flags, pvf_handle* ring)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    HIP_CHECK(hipSetDevice(c->device));
    PVF_REQUIRE(ring && depth > 0 && depth <= 1024, "pvf_egress_create: bad arguments");
    render_require_output(out_w, out_h, flags, "pvf_egress_create");
    std::unique_ptr<EgressRing> r(new EgressRing());
    r->w = out_w; r->h = out_h; r->depth = depth; r->flags = flags;
    r->frame_bytes = planar_bytes(out_w, out_h);
    r->slot_bytes = (r->frame_bytes + 255) / 256 * 256;
    try {
        HIP_CHECK(hipHostMalloc((void**)&r->host, (size_t)depth * r->slot_bytes, hipHostMallocDefault));
        HIP_CHECK(hipMalloc((void**)&r->dev, (size_t)depth * r->slot_bytes));
        HIP_CHECK(hipStreamCreateWithFlags(&r->copy, hipStreamNonBlocking));
        r->rendered.assign(depth, nullptr); r->done.assign(depth, nullptr); r->state.assign(depth, 0);
        for (int i = 0; i < depth; ++i) {
            HIP_CHECK(hipEventCreateWithFlags(&r->rendered[i], hipEventDisableTiming));
            HIP_CHECK(hipEventCreateWithFlags(&r->done[i], hipEventDisableTiming));
            r->meta.emplace_back(new DevBuf());
        }
    } catch (...) { egress_free(*r); throw; }
    const uint64_t id = c->next_id++;
    std::lock_guard<std::mutex> lk(c->frames_mu);
    rstate(c).rings[id] = std::move(r);
    *ring = id;
    API_END
}

extern "C" int32_t pvf_egress_destroy(pvf_handle h, pvf_handle ring)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    std::lock_guard<std::recursive_mutex> lock(c->api_mu);          // no submit of this context is half way
    HIP_CHECK(hipSetDevice(c->device));
    std::unique_ptr<EgressRing> own;
    {
        std::lock_guard<std::mutex> lk(c->frames_mu);
        PVF_REQUIRE(c->render_state && rstate(c).rings.count(ring), "unknown egress ring");
        own = std::move(rstate(c).rings[ring]);
        rstate(c).rings.erase(ring);
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));                     // kernels that still write its slots
    egress_free(*own);
    API_END
}

// the next slot in ring order; refuses (no wait) when the host has not given that slot back
extern "C" int32_t pvf_egress_submit(pvf_handle h, pvf_handle ring, pvf_handle frame, const pvf_prim* prims, int32_t n_prims,
                                     const uint8_t* text, int64_t text_bytes, int32_t* slot)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    std::lock_guard<std::recursive_mutex> lock(c->api_mu);
    HIP_CHECK(hipSetDevice(c->device));
    PVF_REQUIRE(slot && n_prims >= 0, "pvf_egress_submit: bad arguments");
    EgressRing& r = *egress_find(c, ring);
    std::vector<Frame> fs{c->frame(frame)};
    int s;
    {
        std::lock_guard<std::mutex> lk(r.mu);
        s = r.next;
        PVF_REQUIRE(r.state[s] == 0, "pvf_egress_submit: the ring is full (the next slot has not been given back)");
    }
    uint8_t* d = r.dev + (size_t)s * r.slot_bytes;
    const int32_t start[2] = {0, n_prims};
    render_launch(c, fs, r.w, r.h, r.flags, start, prims, text, text_bytes, *r.meta[s], d, (int64_t)r.slot_bytes, nullptr, "pvf_egress_submit");
    HIP_CHECK(hipEventRecord(r.rendered[s], c->stream));
    HIP_CHECK(hipStreamWaitEvent(r.copy, r.rendered[s], 0));
    HIP_CHECK(hipMemcpyAsync(r.host + (size_t)s * r.slot_bytes, d, r.frame_bytes, hipMemcpyDeviceToHost, r.copy));
    HIP_CHECK(hipEventRecord(r.done[s], r.copy));
    {
        std::lock_guard<std::mutex> lk(r.mu);
        r.state[s] = 1;
        r.next = (s + 1) % r.depth;
    }
    *slot = s;
    API_END
}

extern "C" int32_t pvf_egress_wait(pvf_handle h, pvf_handle ring, int32_t slot, const uint8_t** host_planes)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    HIP_CHECK(hipSetDevice(c->device));
    PVF_REQUIRE(host_planes, "pvf_egress_wait: bad arguments");
    EgressRing& r = *egress_find(c, ring);
    {
        std::lock_guard<std::mutex> lk(r.mu);
        PVF_REQUIRE(slot >= 0 && slot < r.depth && r.state[slot] == 1, "pvf_egress_wait: no frame in flight in this slot");
    }
    HIP_CHECK(hipEventSynchronize(r.done[slot]));
    {
        std::lock_guard<std::mutex> lk(r.mu);
        r.state[slot] = 2;
    }
    *host_planes = r.host + (size_t)slot * r.slot_bytes;
    API_END
}

extern "C" int32_t pvf_egress_release(pvf_handle h, pvf_handle ring, int32_t slot)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    HIP_CHECK(hipSetDevice(c->device));
    EgressRing& r = *egress_find(c, ring);
    std::lock_guard<std::mutex> lk(r.mu);
    PVF_REQUIRE(slot >= 0 && slot < r.depth && r.state[slot] == 2, "pvf_egress_release: the slot is not held by the host");
    r.state[slot] = 0;
    API_END
}
