// faces.hip -- the `faces` verb's device side (FACES.md): how good a face chip is, and the contact sheet of chosen chips.
//   chip_quality_k  five integer sums per 150 x 150 chip: the 4-neighbour Laplacian of the luma and its square over the interior (the
//                   numerator of the variance of the Laplacian, the sharpness), the luma sum, the counts of dark and bright pixels.
//                   A block per chip; the chip's 67.5 KB are read once, the luma plane lives in LDS, the Laplacian reads LDS only.
//   sheet_tiles_k   a sheet pixel finds the LAST tile that covers it and resamples that chip (integer bilinear), else background.
//   sheet_prims_k   the sheet's RECT / LINE / TEXT list over the tiles, through render.hip's own coverage code (render_prims.h).
// Everything is integer arithmetic (tests/faces_ref.py restates it; the kernels are held to it bit for bit).
#include "pvf_internal.h"
#include "render_prims.h"
#include <algorithm>

constexpr int Q_SIDE = 150, Q_PIX = Q_SIDE * Q_SIDE, Q_BYTES = Q_PIX * 3;
constexpr int Q_UNIT = 48;                       // bytes a lane takes at a time: three aligned 16-byte loads = 16 pixels
constexpr int Q_UNITS = (Q_BYTES - 12) / Q_UNIT; // 1406 whole units behind the head, whichever of 0 / 4 / 8 / 12 bytes the head is
constexpr int Q_FRONT = 160;                     // LDS bytes in front of the plane: the row above row 0 is read (and masked), never written
constexpr int Q_LDS = Q_FRONT + 16 + Q_PIX + 160;      // + the shift that aligns the unit stores + the row below the last
constexpr int Q_ROUND = 4096;                    // chips resident at a time, as pvf_embed's rounds
static_assert(Q_UNITS == 1406 && Q_LDS % 4 == 0, "chip_quality_k's layout");

__device__ __forceinline__ uint32_t luma8(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// the 16 pixels that START in a unit whose first pixel starts at byte S0 (the last may end in the dword behind it, w[12])
template <int S0>
__device__ __forceinline__ void unit_luma(const uint32_t (&w)[13], uint32_t (&y4)[4], uint32_t& sy, uint32_t& nd, uint32_t& nb)
{
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int o = S0 + 3 * e;
        const uint32_t r = (w[o >> 2] >> (8 * (o & 3))) & 255u, g = (w[(o + 1) >> 2] >> (8 * ((o + 1) & 3))) & 255u;
        const uint32_t b = (w[(o + 2) >> 2] >> (8 * ((o + 2) & 3))) & 255u;
        const uint32_t y = luma8(r, g, b);
        y4[e >> 2] |= y << (8 * (e & 3));
        sy += y; nd += y <= 16u; nb += y >= 239u;
    }
}

// grid (n chips), 256 lanes.  chips: [n][150][150][3], the first chip on a multiple of 4 bytes.  out: [n][5] = S1, S2, SY, ND, NB.
// A chip starts 67500 i bytes in: 4-byte aligned, 16-byte aligned for every fourth chip only.  So a chip is a head of hb = 0 / 4 / 8 / 12
// bytes up to the first 16-byte boundary, 1406 units of 48 bytes = 16 pixels (a pixel straddles a unit's end when hb is no multiple
// of 3: one more dword, inside the chip, completes it) and a tail; the four pixels that start in the head or the tail are read byte by
// byte.  Nothing outside [chip, chip + 67500) is read.  The luma plane is stored linearly, shifted so that a unit's 16 values are one
// aligned 16-byte LDS store; the Laplacian pass takes four pixels a lane from seven aligned LDS dwords (rows are 150 = 4 * 37 + 2 bytes
// apart: the row above and the row below come out of two dwords each).  Per lane S2 sums at most 88 squares below 1020^2: under
// 2^27; across lanes everything is 64-bit.  Integer sums, so the order is free.
__global__ void __launch_bounds__(256) chip_quality_k(const uint8_t* __restrict__ chips, int64_t* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_y[Q_LDS / 4];
    __shared__ int64_t s_red[4][5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* __restrict__ chip = chips + (size_t)blockIdx.x * Q_BYTES;
    const int hb = (16 - (int)(reinterpret_cast<uintptr_t>(chip) & 15)) & 15;
    const int s0 = (3 - hb % 3) % 3;             // where in a unit its first pixel starts
    const int nh = (hb + s0) / 3;                // pixels that start in the head: 0, 2, 3 or 4
    const int base = Q_FRONT + ((16 - nh) & 15); // LDS byte of pixel 0: pixel nh, the first of unit 0, lands on a multiple of 16
    uint8_t* s_yb = reinterpret_cast<uint8_t*>(s_y);
    uint32_t sy = 0, nd = 0, nb = 0;
    for (int u = tid; u < Q_UNITS; u += 256) {
        const uint8_t* p = chip + hb + (size_t)u * Q_UNIT;
        const uint4* q = reinterpret_cast<const uint4*>(p);
        const uint4 a = q[0], b = q[1], c = q[2];
        uint32_t w[13] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, 0u};
        if (s0) w[12] = *reinterpret_cast<const uint32_t*>(p + Q_UNIT);       // hb = 4 or 8: at least 4 bytes of the chip lie behind the last unit
        uint32_t y4[4] = {0u, 0u, 0u, 0u};
        if (s0 == 0) unit_luma<0>(w, y4, sy, nd, nb);
        else if (s0 == 1) unit_luma<1>(w, y4, sy, nd, nb);
        else unit_luma<2>(w, y4, sy, nd, nb);
        *reinterpret_cast<uint4*>(s_yb + base + nh + 16 * u) = make_uint4(y4[0], y4[1], y4[2], y4[3]);
    }
    if (tid >= 252) {                            // pixels 0 .. nh - 1 and nh + 22496 .. 22499: four, whatever hb is
        const int j = tid - 252, k = j < nh ? j : Q_PIX - 4 + j;
        const uint8_t* p = chip + 3 * k;
        const uint32_t y = luma8(p[0], p[1], p[2]);
        s_yb[base + k] = (uint8_t)y;
        sy += y; nd += y <= 16u; nb += y >= 239u;
    }
    __syncthreads();
    const int g0 = base & ~3, ng = (base + Q_PIX - g0 + 3) >> 2;      // groups of four LDS bytes that hold a pixel
    int32_t s1 = 0;
    uint32_t s2 = 0;
    for (int g = tid; g < ng; g += 256) {
        const int o = g0 + 4 * g, wi = o >> 2;
        const uint32_t own = s_y[wi], prv = s_y[wi - 1], nxt = s_y[wi + 1];
        const uint32_t ua = s_y[wi - 38], ub = s_y[wi - 37], da = s_y[wi + 37], db = s_y[wi + 38];       // bytes o -+ 152, o -+ 148
        const uint32_t up = (ua >> 16) | (ub << 16), dn = (da >> 16) | (db << 16);                       // bytes o - 150 .., o + 150 ..
        const uint32_t lf = (prv >> 24) | (own << 8), rt = (own >> 8) | (nxt << 24);
        const int k0 = o - base;                 // the group's first pixel; -3 .. -1 in the first group of a shifted plane
        const int r0 = k0 >= 0 ? k0 / Q_SIDE : -1, c0 = k0 - Q_SIDE * r0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int cc = c0 + e, rr = r0;
            if (cc >= Q_SIDE) { cc -= Q_SIDE; ++rr; }
            if (rr < 1 || rr > Q_SIDE - 2 || cc < 1 || cc > Q_SIDE - 2) continue;       // the border ring (and what is no pixel) has no Laplacian
            const int sh = 8 * e;
            const int L = 4 * (int)((own >> sh) & 255u) - (int)((up >> sh) & 255u) - (int)((dn >> sh) & 255u) - (int)((lf >> sh) & 255u) -
                          (int)((rt >> sh) & 255u);
            s1 += L; s2 += (uint32_t)(L * L);
        }
    }
    long long v[5] = {(long long)s1, (long long)s2, (long long)sy, (long long)nd, (long long)nb};
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
        for (int i = 0; i < 5; ++i) v[i] += __shfl_xor(v[i], d);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) s_red[wave][i] = v[i];
    }
    __syncthreads();
    if (tid == 0) {
        int64_t* o = out + (size_t)blockIdx.x * 5;
#pragma unroll
        for (int i = 0; i < 5; ++i) o[i] = s_red[0][i] + s_red[1][i] + s_red[2][i] + s_red[3][i];
    }
}

// ---- the sheet ----------------------------------------------------------------------------------------------------------------------
constexpr int SH_TW = 32, SH_TH = 8;             // sheet pixels per block: a lane per pixel, a wave two rows of 32
constexpr int SH_CHUNK = 256;                    // tiles / primitives culled and staged in LDS at a time

struct SheetTileArgs {
    const uint8_t* chips;           // [n][150][150][3]
    const int32_t* xy;              // [n][2] top-left corners, any int32
    int n, S, W, H;
    uint32_t background;
    int fill;                       // pixels no tile of this launch covers: 1 background, 0 left as they are (a later round of tiles)
    uint8_t* rgb;                   // [H][W][3]
};

// grid (ceil(W / 32), ceil(H / 8)), 256 lanes.  The tiles are walked from the LAST chunk of 256 to the first: every lane tests one
// against the block's rectangle, the survivors go to LDS in list order (ballot + popcount ranks, as render_k stages primitives), a pixel
// scans them from the back and keeps the first that covers it -- the last tile of the list, by index, not by launch order.  The walk
// ends as soon as every pixel of the block has its tile.  FACES.md "Tile" is the resampling.
__global__ void __launch_bounds__(256) sheet_tiles_k(const SheetTileArgs a)
{
    __shared__ int s_idx[SH_CHUNK], s_x[SH_CHUNK], s_ty[SH_CHUNK];
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int X = blockIdx.x * SH_TW + (tid & (SH_TW - 1)), Y = blockIdx.y * SH_TH + (tid >> 5);
    const bool inside = X < a.W && Y < a.H;
    const int64_t bx0 = (int64_t)blockIdx.x * SH_TW, by0 = (int64_t)blockIdx.y * SH_TH;
    const int64_t bx1 = min(bx0 + SH_TW - 1, (int64_t)a.W - 1), by1 = min(by0 + SH_TH - 1, (int64_t)a.H - 1);
    int best = -1, tx = 0, ty = 0;
    for (int top = a.n; top > 0; top -= SH_CHUNK) {
        const int lo = max(top - SH_CHUNK, 0), i = lo + tid;
        bool hit = false;
        int cx = 0, cy = 0;
        if (i < top) {
            cx = a.xy[2 * i]; cy = a.xy[2 * i + 1];
            hit = cx <= bx1 && (int64_t)cx + a.S - 1 >= bx0 && cy <= by1 && (int64_t)cy + a.S - 1 >= by0;
        }
        const uint64_t m = __ballot(hit);
        if (lane == 0) s_wave[wv] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { if (k < wv) off += s_wave[k]; total += s_wave[k]; }
        if (hit) { const int at = off + __popcll(m & ((1ull << lane) - 1)); s_idx[at] = i; s_x[at] = cx; s_ty[at] = cy; }
        __syncthreads();
        if (inside && best < 0)
            for (int j = total - 1; j >= 0; --j) {
                const int64_t dx = (int64_t)X - s_x[j], dy = (int64_t)Y - s_ty[j];
                if (dx >= 0 && dx < a.S && dy >= 0 && dy < a.S) { best = s_idx[j]; tx = (int)dx; ty = (int)dy; break; }
            }
        if (__syncthreads_and(!inside || best >= 0)) break;                   // (the barrier in front of the next chunk's stores, too)
    }
    if (!inside) return;
    uint8_t* o = a.rgb + ((size_t)Y * a.W + X) * 3;
    if (best < 0) {
        if (a.fill) { o[0] = (uint8_t)(a.background & 255u); o[1] = (uint8_t)((a.background >> 8) & 255u); o[2] = (uint8_t)((a.background >> 16) & 255u); }
        return;
    }
    const int S2 = 2 * a.S, umax = (Q_SIDE - 1) * S2;
    const int u = min(max((2 * tx + 1) * Q_SIDE - a.S, 0), umax), v = min(max((2 * ty + 1) * Q_SIDE - a.S, 0), umax);
    const int x0 = u / S2, y0 = v / S2;
    const uint32_t fx = (uint32_t)(u - x0 * S2), fy = (uint32_t)(v - y0 * S2);
    const int x1 = min(x0 + 1, Q_SIDE - 1), y1 = min(y0 + 1, Q_SIDE - 1);
    const uint32_t w00 = (S2 - fx) * (S2 - fy), w01 = fx * (S2 - fy), w10 = (S2 - fx) * fy, w11 = fx * fy;      // they sum to 4 S^2 <= 1 440 000
    const uint32_t den = 4u * a.S * a.S, half = den >> 1;
    const uint8_t* __restrict__ chip = a.chips + (size_t)best * Q_BYTES;
    const uint8_t* p00 = chip + (y0 * Q_SIDE + x0) * 3;
    const uint8_t* p01 = chip + (y0 * Q_SIDE + x1) * 3;
    const uint8_t* p10 = chip + (y1 * Q_SIDE + x0) * 3;
    const uint8_t* p11 = chip + (y1 * Q_SIDE + x1) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = (uint8_t)((w00 * p00[k] + w01 * p01[k] + w10 * p10[k] + w11 * p11[k] + half) / den);      // < 2^29
}

struct SheetPrimArgs { const pvf_prim* prims; int n; const uint8_t* text; int W, H; uint8_t* rgb; };

// grid as sheet_tiles_k.  render_k's walk over a frame's list, on a picture that is already there: chunks of 256 culled against the
// block's rectangle, the survivors in LDS in list order, a pixel takes the colour of the last primitive that covers it (prim_meets /
// prim_covers: the renderer's own) and stores only if one does.
__global__ void __launch_bounds__(256) sheet_prims_k(const SheetPrimArgs a)
{
    __shared__ pvf_prim s_prim[SH_CHUNK];
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int X = blockIdx.x * SH_TW + (tid & (SH_TW - 1)), Y = blockIdx.y * SH_TH + (tid >> 5);
    const bool inside = X < a.W && Y < a.H;
    const int64_t bx0 = (int64_t)blockIdx.x * SH_TW, by0 = (int64_t)blockIdx.y * SH_TH;
    const int64_t bx1 = min(bx0 + SH_TW - 1, (int64_t)a.W - 1), by1 = min(by0 + SH_TH - 1, (int64_t)a.H - 1);
    bool drawn = false;
    uint32_t colour = 0;
    for (int base = 0; base < a.n; base += SH_CHUNK) {
        const int i = base + tid;
        pvf_prim p;
        bool hit = false;
        if (i < a.n) {
            const int4* q = reinterpret_cast<const int4*>(a.prims + i);
            const int4 lo = q[0], hi = q[1];
            p.type = lo.x; p.a = lo.y; p.b = lo.z; p.c = lo.w; p.d = hi.x; p.colour = (uint32_t)hi.y; p.scale = hi.z; p.reserved = 0;
            hit = prim_meets<false>(p, bx0, by0, bx1, by1);
        }
        const uint64_t m = __ballot(hit);
        if (lane == 0) s_wave[wv] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { if (k < wv) off += s_wave[k]; total += s_wave[k]; }
        if (hit) s_prim[off + __popcll(m & ((1ull << lane) - 1))] = p;
        __syncthreads();
        if (inside)
            for (int j = 0; j < total; ++j) {
                const pvf_prim q = s_prim[j];
                if (prim_covers<false>(q, a.text, X, Y)) { drawn = true; colour = q.colour; }
            }
        __syncthreads();
    }
    if (!inside || !drawn) return;
    uint8_t* o = a.rgb + ((size_t)Y * a.W + X) * 3;
    o[0] = (uint8_t)(colour & 255u); o[1] = (uint8_t)((colour >> 8) & 255u); o[2] = (uint8_t)((colour >> 16) & 255u);
}

// ---------------------------------------------------------------------------------------------------
// the chip geometry: dlib's compiled-in mean face shape with EmbedModel's defaults (150, 0.25) -- what a dlib embedder file loads.  Not
// the loaded embedder's: the verb runs without one, and a face's quality must not depend on what else the context holds.
const EmbedModel& faces_geometry()
{
    static const EmbedModel dflt = [] {
        EmbedModel e;
        e.mean_shape.resize(102);
        dlib_mean_face_shape(e.mean_shape.data());
        return e;
    }();
    return dflt;
}

// the aligned chips of m faces into d_chips (the plan of api.hip's make_face_chips, without its need of a loaded embedder)
void faces_make_chips(Ctx* c, const pvf_handle* frames, const int32_t* pts, int m, uint8_t* d_chips)
{
    const EmbedModel& e = faces_geometry();
    static_assert(Q_SIDE == 150, "EmbedModel's default chip size");
    std::vector<ChipJob> jobs(m);
    for (int i = 0; i < m; ++i) {
        ChipDetails d;
        face_chip_details(e, pts + (size_t)i * 68 * 2, &d);
        jobs[i] = chip_plan(c->frame(frames[i]), d);
    }
    chip_extract_batch(c, jobs, d_chips);
}

static void quality_launch(Ctx* c, const uint8_t* d_chips, int m, int64_t* d_out)
{
    PVF_REQUIRE((reinterpret_cast<uintptr_t>(d_chips) & 3) == 0, "faces: the chips start on a multiple of 4 bytes");
    ProfScope prof(c, "chip_quality");
    hipLaunchKernelGGL(chip_quality_k, dim3((unsigned)m), dim3(256), 0, c->stream, d_chips, d_out);
    HIP_CHECK(hipGetLastError());
}

static void check_source(const ChipSource& src, int n, const std::string& w)
{
    PVF_REQUIRE(n >= 0 && n <= PVF_SHEET_MAX_TILES, w + ": n outside 0 .. PVF_SHEET_MAX_TILES");
    PVF_REQUIRE(n == 0 || src.host || (src.frames && src.pts), w + ": null chips, frames or landmarks");
}

// round [i0, i0 + m) of the source into d_chips, behind whatever still reads d_chips on the stream
void faces_source_round(Ctx* c, const ChipSource& src, int i0, int m, uint8_t* d_chips)
{
    if (src.host) HIP_CHECK(hipMemcpyAsync(d_chips, src.host + (size_t)i0 * Q_BYTES, (size_t)m * Q_BYTES, hipMemcpyHostToDevice, c->stream));
    else faces_make_chips(c, src.frames + i0, src.pts + (size_t)i0 * 136, m, d_chips);
}

static void quality_run(Ctx* c, const ChipSource& src, int n, int64_t* out, const char* who)
{
    check_source(src, n, who);
    if (n == 0) return;
    PVF_REQUIRE(out, std::string(who) + ": null output");
    ScratchLayout chips_lay, out_lay;
    const auto sChips = chips_lay.take<uint8_t>((size_t)std::min(n, Q_ROUND) * Q_BYTES);
    const auto sOut = out_lay.take<int64_t>((size_t)n * 5);
    c->s_trk0.ensure(chips_lay.bytes());
    c->s_act0.ensure(out_lay.bytes());
    for (int i0 = 0; i0 < n; i0 += Q_ROUND) {
        const int m = std::min(Q_ROUND, n - i0);
        faces_source_round(c, src, i0, m, sChips.in(c->s_trk0));
        quality_launch(c, sChips.in(c->s_trk0), m, sOut.in(c->s_act0) + (size_t)i0 * 5);
    }
    HIP_CHECK(hipMemcpyAsync(out, sOut.in(c->s_act0), sOut.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

void sheet_check(const std::string& w, int W, int H, uint32_t background, const pvf_prim* prims, int n_prims, const uint8_t* text,
                 int64_t text_bytes, const uint8_t* rgb)
{
    PVF_REQUIRE(W >= 1 && H >= 1 && W <= PVF_SHEET_MAX_SIDE && H <= PVF_SHEET_MAX_SIDE, w + ": sheet side outside 1 .. PVF_SHEET_MAX_SIDE");
    PVF_REQUIRE((int64_t)W * H <= PVF_SHEET_MAX_PIXELS, w + ": more sheet pixels than PVF_SHEET_MAX_PIXELS");
    PVF_REQUIRE(rgb, w + ": null output");
    PVF_REQUIRE(background <= 0xffffffu, w + ": the background is r | g << 8 | b << 16");
    PVF_REQUIRE(n_prims >= 0 && n_prims <= PVF_RENDER_MAX_PRIMS, w + ": more primitives than PVF_RENDER_MAX_PRIMS");
    PVF_REQUIRE(prims || n_prims == 0, w + ": null primitive list");
    PVF_REQUIRE(text_bytes >= 0 && text_bytes <= PVF_RENDER_MAX_TEXT, w + ": more text bytes than PVF_RENDER_MAX_TEXT");
    PVF_REQUIRE(text || text_bytes == 0, w + ": null text pool");
    for (int i = 0; i < n_prims; ++i) {          // nothing the kernel indexes with is taken on trust (render_launch's checks)
        const pvf_prim& p = prims[i];
        PVF_REQUIRE(p.type != PVF_PRIM_REDACT, w + ": a sheet takes no redactions");
        PVF_REQUIRE(p.type == PVF_PRIM_RECT || p.type == PVF_PRIM_LINE || p.type == PVF_PRIM_TEXT, w + ": unknown primitive type");
        if (p.type != PVF_PRIM_TEXT) continue;
        PVF_REQUIRE(p.d >= 0 && p.d <= PVF_RENDER_MAX_RUN, w + ": a text run longer than PVF_RENDER_MAX_RUN bytes");
        PVF_REQUIRE(p.c >= 0 && (int64_t)p.c + p.d <= text_bytes, w + ": a text run outside the text pool");
        PVF_REQUIRE(p.scale >= 1 && p.scale <= PVF_RENDER_MAX_SCALE, w + ": text scale outside 1 .. PVF_RENDER_MAX_SCALE");
    }
}

void sheet_prims_launch(Ctx* c, const pvf_prim* d_prims, int n_prims, const uint8_t* d_text, int W, int H, uint8_t* d_rgb)
{
    if (!n_prims) return;
    SheetPrimArgs a;
    a.prims = d_prims; a.n = n_prims; a.text = d_text; a.W = W; a.H = H; a.rgb = d_rgb;
    ProfScope prof(c, "sheet");
    hipLaunchKernelGGL(sheet_prims_k, dim3((W + SH_TW - 1) / SH_TW, (H + SH_TH - 1) / SH_TH), dim3(256), 0, c->stream, a);
    HIP_CHECK(hipGetLastError());
}

static void sheet_run(Ctx* c, const ChipSource& src, int n, const int32_t* xy, int S, int W, int H, uint32_t background, const pvf_prim* prims,
                      int n_prims, const uint8_t* text, int64_t text_bytes, uint8_t* rgb, const char* who)
{
    const std::string w(who);
    check_source(src, n, w);
    PVF_REQUIRE(n == 0 || xy, w + ": null tile corners");
    PVF_REQUIRE(S >= PVF_SHEET_MIN_TILE && S <= PVF_SHEET_MAX_TILE, w + ": tile side outside PVF_SHEET_MIN_TILE .. PVF_SHEET_MAX_TILE");
    sheet_check(w, W, H, background, prims, n_prims, text, text_bytes, rgb);
    ScratchLayout chips_lay, lay;
    const auto sChips = chips_lay.take<uint8_t>((size_t)std::min(n, Q_ROUND) * Q_BYTES);
    const auto sRgb = lay.take<uint8_t>((size_t)W * H * 3);
    const auto sXy = lay.take<int32_t>((size_t)n * 2);
    const auto sPrims = lay.take<pvf_prim>((size_t)n_prims);     // 256-byte aligned: the kernel reads a primitive as two dwordx4
    const auto sText = lay.take<uint8_t>((size_t)text_bytes + 1);
    c->s_trk0.ensure(chips_lay.bytes());
    c->s_act0.ensure(lay.bytes());
    if (n) HIP_CHECK(hipMemcpyAsync(sXy.in(c->s_act0), xy, sXy.bytes(), hipMemcpyHostToDevice, c->stream));
    if (n_prims) HIP_CHECK(hipMemcpyAsync(sPrims.in(c->s_act0), prims, sPrims.bytes(), hipMemcpyHostToDevice, c->stream));
    if (text_bytes) HIP_CHECK(hipMemcpyAsync(sText.in(c->s_act0), text, (size_t)text_bytes, hipMemcpyHostToDevice, c->stream));
    const dim3 grid((W + SH_TW - 1) / SH_TW, (H + SH_TH - 1) / SH_TH);
    // rounds in list order; a later round stores only where its own tiles are, so the last tile of the whole list wins
    for (int i0 = 0; i0 == 0 || i0 < n; i0 += Q_ROUND) {
        const int m = std::min(Q_ROUND, n - i0);
        if (m) faces_source_round(c, src, i0, m, sChips.in(c->s_trk0));
        SheetTileArgs a;
        a.chips = sChips.in(c->s_trk0); a.xy = sXy.in(c->s_act0) + (size_t)i0 * 2;
        a.n = m; a.S = S; a.W = W; a.H = H; a.background = background; a.fill = i0 == 0; a.rgb = sRgb.in(c->s_act0);
        ProfScope prof(c, "sheet");
        hipLaunchKernelGGL(sheet_tiles_k, grid, dim3(256), 0, c->stream, a);
        HIP_CHECK(hipGetLastError());
    }
    sheet_prims_launch(c, sPrims.in(c->s_act0), n_prims, sText.in(c->s_act0), W, H, sRgb.in(c->s_act0));
    HIP_CHECK(hipMemcpyAsync(rgb, sRgb.in(c->s_act0), sRgb.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

#define API_BEGIN try {
#define API_END                                                        \
    return 0;                                                          \
    }                                                                  \
    catch (const std::exception& e) { pvf_set_error(e.what()); return -1; } \
    catch (...) { pvf_set_error("unknown error"); return -2; }
#define ENTER(c, h)                                                \
    Ctx* c = pvf_ctx(h);                                           \
    std::lock_guard<std::recursive_mutex> _api_lock(c->api_mu);    \
    HIP_CHECK(hipSetDevice(c->device))

extern "C" int32_t pvf_chip_quality(pvf_handle h, const uint8_t* chips, int32_t n, int64_t* out)
{
    API_BEGIN
    ENTER(c, h);
    quality_run(c, ChipSource{chips, nullptr, nullptr}, n, out, "pvf_chip_quality");
    API_END
}

extern "C" int32_t pvf_face_quality(pvf_handle h, const pvf_handle* frames, const int32_t* pts, int32_t n, int64_t* out)
{
    API_BEGIN
    ENTER(c, h);
    quality_run(c, ChipSource{nullptr, frames, pts}, n, out, "pvf_face_quality");
    API_END
}

extern "C" int32_t pvf_chip_sheet(pvf_handle h, const uint8_t* chips, int32_t n, const int32_t* xy, int32_t S, int32_t W, int32_t H,
                                  uint32_t background, const pvf_prim* prims, int32_t n_prims, const uint8_t* text, int64_t text_bytes, uint8_t* rgb)
{
    API_BEGIN
    ENTER(c, h);
    sheet_run(c, ChipSource{chips, nullptr, nullptr}, n, xy, S, W, H, background, prims, n_prims, text, text_bytes, rgb, "pvf_chip_sheet");
    API_END
}

extern "C" int32_t pvf_face_sheet(pvf_handle h, const pvf_handle* frames, const int32_t* pts, int32_t n, const int32_t* xy, int32_t S, int32_t W,
                                  int32_t H, uint32_t background, const pvf_prim* prims, int32_t n_prims, const uint8_t* text, int64_t text_bytes,
                                  uint8_t* rgb)
{
    API_BEGIN
    ENTER(c, h);
    sheet_run(c, ChipSource{nullptr, frames, pts}, n, xy, S, W, H, background, prims, n_prims, text, text_bytes, rgb, "pvf_face_sheet");
    API_END
}
