// tube.hip -- the `tube` verb's device side (TUBE.md): square windows of resident RGB frames resampled to S x S pictures, n of them per call.
//   crop_k   a block per (crop, column piece of C_COLS output columns, row band of C_BAND output rows), a lane per output column.
//            The source rows of the band are staged in LDS as 16-byte loads through a buffer descriptor over the frame, each row once
//            per band; a lane reduces its own columns of a staged row to three 32-bit sums (horizontal first) and adds them, weighted,
//            to the 64-bit sums of the output row being made and of the one below it (a source row lies in at most two output rows when
//            reducing).  A finished row is divided by its exact quotient and leaves as RGB bytes or, converted with render_k's own
//            device code (render_prims.h), as planar YUV 4:2:0 -- a lane pair and two consecutive rows of a band make a chroma sample.
//   warp_k   the oriented window of `tube --align` (TUBE.md "Oriented window"): a block per (crop, W_SIDE x W_SIDE tile of output pixels), a
//            lane per output pixel.  The block bounds the source pixels its K x K sub-samples per pixel can touch from the tile's four
//            corner sub-samples, stages that box in LDS through crop_k's descriptor when it fits W_TILE bytes and takes its taps through
//            the descriptor one by one when it does not; a lane then sums its K^2 bilinear sub-samples in 32 bits.
// The two regimes of TUBE.md (area average at L >= 16 S, bilinear below) are the same separable weighted sum with other weights and
// another divisor, so they are one kernel; a block takes the regime of its crop.  Every sum is an integer sum: neither the pieces, the
// bands, the LDS tiles nor the rounds of a call change a bit (tests/tube_ref.py restates the arithmetic; the kernel is held to it).
#include "pvf_internal.h"
#include "render_prims.h"
#include <algorithm>
#include <cstdlib>

constexpr int C_COLS = 128;         // output columns of a block, a lane each: the column piece (even, so a lane pair shares a chroma sample)
constexpr int C_BAND = 16;          // output rows of a block: the row band (even: a chroma sample never straddles two bands)
constexpr int C_TILE = 16384;       // LDS bytes of staged source rows: the rows of a band of face-sized windows in one piece
constexpr int C_TILE_PX = 2720;     // source pixels of a staged row piece at most: 3 bytes of misalignment + 3 * 2720, rounded up to 16, is 8176
constexpr size_t C_ROUND_BYTES = (size_t)32 << 20;      // output bytes of a round, unless PVF_CROP_ROUND names the crops of a round
constexpr int C_ROUND_MAX = 4096;   // crops of a round at most (blockIdx.y)
static_assert(C_COLS % 2 == 0 && C_BAND % 2 == 0, "chroma samples stay inside a block");
static_assert((3 + 3 * C_TILE_PX + 15) / 16 * 16 <= C_TILE, "one staged row piece fits the tile");
static_assert((C_BAND + 1) * ((3 + 3 * (C_COLS + 1) + 15) / 16 * 16) <= C_TILE, "enlarging: a band's sample centres span less than C_BAND - 1 source rows and C_COLS - 1 columns, plus the two taps");
// the bounds TUBE.md "Caps" argues from
static_assert((int64_t)PVF_CROP_MAX_SIDE * 255 < ((int64_t)1 << 31), "a row's weighted sum of one channel fits 32 bits");
static_assert((int64_t)PVF_CROP_MAX_SIZE * 15 + (int64_t)PVF_CROP_MAX_SIZE * PVF_CROP_MAX_SIDE + 32 * PVF_CROP_MAX_SIZE < ((int64_t)1 << 31), "window-relative units fit int32");
static_assert((PVF_CROP_MAX_COORD >> 4) + (PVF_CROP_MAX_SIDE >> 4) * 2 < (1 << 30), "source indices fit int32");

struct CropJob { const uint8_t* img; int32_t h, w, X0, Y0, L, pad; };
static_assert(sizeof(CropJob) == 32, "CropJob is two 16-byte units");
struct CropArgs { const CropJob* jobs; uint8_t* out; int S, yuv; RenderCoef k; };

// num // den for num < 257 den, den < 2^37.  The estimate is made from the high 32 bits of num (sh, block-uniform, is chosen so that
// num >> sh fits them: a 64-bit integer has no conversion to float of its own) times rden_s = 2^sh / den: off from num / den by less
// than 2^-13 (three roundings of relative 2^-24 on a value below 257, and a truncation below 2^sh / den <= 2^-22), so its integer
// part is the quotient or one beside it, and the exact 64-bit residual says which (tests/csrc/crop_quotient_check.c).
__device__ __forceinline__ int exact_quotient(uint64_t num, uint64_t den, float rden_s, int sh)
{
    int q = (int)((float)(uint32_t)(num >> sh) * rden_s);
    int64_t r = (int64_t)num - (int64_t)((uint64_t)(uint32_t)q * den);
    if (r < 0) { --q; r += (int64_t)den; }
    if (r >= (int64_t)den) ++q;
    return q;
}

// grid (pieces * bands, crops of the round), C_COLS lanes.
// Units: 1 / (16 S) pixel when reducing, 1 / (32 S) when enlarging; U of them make a source pixel.  With bx = X0 >> 4 (less one when
// enlarging) an output column's left edge (its sample centre) is U bx + ox + j step, and ox + j step is a small non-negative int32: the
// window is reduced against the source grid before anything is multiplied by S, and floor() of a negative coordinate is the arithmetic
// shift alone.  Rows likewise.
__global__ void __launch_bounds__(C_COLS) crop_k(const CropArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[C_TILE];
    const int tid = threadIdx.x, S = a.S;
    const int pieces = (S + C_COLS - 1) / C_COLS;
    const int piece = blockIdx.x % pieces, band = blockIdx.x / pieces;
    const int4* jq = reinterpret_cast<const int4*>(a.jobs + blockIdx.y);
    const int4 j_lo = jq[0], j_hi = jq[1];
    const uint8_t* img = reinterpret_cast<const uint8_t*>(((uint64_t)(uint32_t)j_lo.y << 32) | (uint32_t)j_lo.x);
    const int h = j_lo.z, w = j_lo.w, X0 = j_hi.x, Y0 = j_hi.y, L = j_hi.z;
    const bool enl = L < 16 * S;
    const int U = enl ? 32 * S : 16 * S, step = enl ? 2 * L : L;
    const int bx = (X0 >> 4) - (enl ? 1 : 0), by = (Y0 >> 4) - (enl ? 1 : 0);
    const int ox = enl ? 2 * S * (X0 & 15) + L + 16 * S : S * (X0 & 15);
    const int oy = enl ? 2 * S * (Y0 & 15) + L + 16 * S : S * (Y0 & 15);

    // an output column's source columns p0 .. p1 with the weights of the first and the last; those between weigh U
    auto columns = [&](int j, int& p0, int& p1, int& wf, int& wl) {
        const int lo = ox + j * step;
        if (enl) { const int q = lo / U, f = lo - q * U; p0 = bx + q; p1 = p0 + 1; wf = U - f; wl = f; return; }
        const int hi = lo + L, q0 = lo / U, q1 = (hi - 1) / U;
        p0 = bx + q0; p1 = bx + q1;
        wf = min(hi, U * (q0 + 1)) - lo; wl = hi - U * q1;        // (q1 == q0: wf = L is the column's whole weight, wl is not used)
    };
    const int j0 = piece * C_COLS, j = j0 + tid, jl = min(j0 + C_COLS, S) - 1;
    int p0 = 1, p1 = 0, wf = 0, wl = 0;
    if (j < S) columns(j, p0, p1, wf, wl);
    int pA, pB, t0, t1;
    columns(j0, pA, t0, t1, t1);
    columns(jl, t0, pB, t1, t1);
    pA = max(pA, 0); pB = min(pB, w - 1);                           // the piece's source columns inside the frame; empty: everything reads black
    const int pitch = (3 + 3 * min(C_TILE_PX, max(pB - pA + 1, 1)) + 15) & ~15, n16 = pitch >> 4, TR = C_TILE / pitch;

    // the frame behind a descriptor whose base is 4-byte aligned; the range is rounded UP to whole dwords, because a dword load that
    // straddles the end of the range reads 0 for all four bytes on gfx950, and the aligned dword that holds the
    // frame's last byte lies in the page that byte lies in.  Bytes read beyond a row's wanted pixels are never looked at.
    const unsigned delta = (unsigned)((uintptr_t)img & 3u), rb = 3u * (unsigned)w;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)((uintptr_t)img - delta), 0, (int)((delta + (unsigned)h * rb + 3u) & ~3u), 0x00020000);

    const uint64_t den = enl ? (uint64_t)1024 * S * S : (uint64_t)L * L;
    const int sh = max(0, 64 - __clzll((long long)den) + 9 - 32);
    const float rden_s = (float)((uint64_t)1 << sh) / (float)den;
    const int r0 = band * C_BAND, r1 = min(r0 + C_BAND, S);
    const int cw = (S + 1) >> 1;
    const size_t crop_bytes = a.yuv ? (size_t)S * S + 2 * (size_t)cw * cw : (size_t)S * S * 3;
    uint8_t* out = a.out + (size_t)blockIdx.y * crop_bytes;
    uint64_t acc[3] = {0, 0, 0}, nxt[3] = {0, 0, 0};
    int top[3] = {0, 0, 0};

    // rows ty .. ty + nrow - 1 of the frame, from the aligned dword that holds pixel pc0 on, into the tile at `pitch` bytes a row
    auto stage = [&](int ty, int nrow, int pc0) {
        __syncthreads();                                            // (whoever still reads the tile's last content)
        for (int u = tid; u < nrow * n16; u += C_COLS) {
            const int i = u / n16, k = u - i * n16;
            const unsigned off = ((delta + (unsigned)(ty + i) * rb + 3u * (unsigned)pc0) & ~3u) + 16u * (unsigned)k;
            reinterpret_cast<uint4*>(s_tile)[u] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0));
        }
        __syncthreads();
    };
    // this lane's weighted sums over the pixels pc0 .. pc1 of tile row i, which holds frame row sy, times wc into acc and times wn into nxt
    auto add_row = [&](int i, int sy, int pc0, int pc1, int wc, int wn) {
        const int il = max(p0 + 1, pc0), ih = min(p1 - 1, pc1);
        const bool first_in = p0 >= pc0 && p0 <= pc1, last_in = p1 != p0 && p1 >= pc0 && p1 <= pc1;
        // the row's pixel p is at tile bytes at + 3 p ..: the staged row starts at the aligned dword that holds pixel pc0
        const int at = i * pitch + (int)((delta + (unsigned)sy * rb + 3u * (unsigned)pc0) & 3u) - 3 * pc0;
        const uint8_t* s = s_tile;
        uint32_t m0 = 0, m1 = 0, m2 = 0;
        for (int p = il; p <= ih; ++p) { m0 += s[at + 3 * p]; m1 += s[at + 3 * p + 1]; m2 += s[at + 3 * p + 2]; }
        uint32_t h0 = m0 * (uint32_t)U, h1 = m1 * (uint32_t)U, h2 = m2 * (uint32_t)U;
        if (first_in) { h0 += (uint32_t)wf * s[at + 3 * p0]; h1 += (uint32_t)wf * s[at + 3 * p0 + 1]; h2 += (uint32_t)wf * s[at + 3 * p0 + 2]; }
        if (last_in) { h0 += (uint32_t)wl * s[at + 3 * p1]; h1 += (uint32_t)wl * s[at + 3 * p1 + 1]; h2 += (uint32_t)wl * s[at + 3 * p1 + 2]; }
        acc[0] += (uint64_t)(uint32_t)wc * h0; acc[1] += (uint64_t)(uint32_t)wc * h1; acc[2] += (uint64_t)(uint32_t)wc * h2;
        nxt[0] += (uint64_t)(uint32_t)wn * h0; nxt[1] += (uint64_t)(uint32_t)wn * h1; nxt[2] += (uint64_t)(uint32_t)wn * h2;
    };
    // output row r is complete in acc: divide, store, and make nxt the sums of the row below
    auto finish = [&](int r) {
        int v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = exact_quotient(acc[c] + (den >> 1), den, rden_s, sh);
            acc[c] = nxt[c]; nxt[c] = 0;
        }
        if (!a.yuv) {
            if (j < S) { uint8_t* o = out + ((size_t)r * S + j) * 3; o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2]; }
            return;
        }
        if (j < S) out[(size_t)r * S + j] = (uint8_t)yuv_luma(a.k, v[0], v[1], v[2]);
        // chroma: the even lane of a pair adds its neighbour's pixel (its own again past an odd picture's last column), the odd row of a
        // pair of rows adds the even row's sums (an odd picture's last row counts twice)
        const bool has_right = j + 1 < S;
        int pair[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { const int o = __shfl_xor(v[c], 1); pair[c] = v[c] + (has_right ? o : v[c]); }
        if (!(r & 1)) {
            top[0] = pair[0]; top[1] = pair[1]; top[2] = pair[2];
            if (r + 1 < S) return;
        }
        if (j < S && !(j & 1)) {
            uint8_t* up = out + (size_t)S * S + (size_t)(r >> 1) * cw + (j >> 1);
            up[0] = (uint8_t)yuv_chroma(a.k.u, top[0] + pair[0], top[1] + pair[1], top[2] + pair[2]);
            up[(size_t)cw * cw] = (uint8_t)yuv_chroma(a.k.v, top[0] + pair[0], top[1] + pair[1], top[2] + pair[2]);
        }
    };

    // the band's source rows inside the frame
    const int lo_first = oy + r0 * step, lo_last = oy + (r1 - 1) * step;
    const int ya = max(by + lo_first / U, 0), yb = min(by + (enl ? lo_last / U + 1 : (lo_last + L - 1) / U), h - 1);
    const bool any = pA <= pB && ya <= yb;                          // else everything the band sees is black
    if (enl) {
        // at most 17 rows of at most 129 pixels (static_assert above): one tile, staged once; an output row reads its two rows from it
        if (any) stage(ya, yb - ya + 1, pA);
        for (int r = r0; r < r1; ++r) {
            const int lo = oy + r * step, q0 = lo / U, fy = lo - q0 * U;
            if (any) {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int sy = by + q0 + k;
                    if (sy >= ya && sy <= yb) add_row(sy - ya, sy, pA, pB, k ? fy : U - fy, 0);
                }
            }
            finish(r);
        }
        return;
    }
    // reducing: the source rows go by once, tile after tile; row q lies in the output row being made (weight wc) and perhaps in the one
    // below it (wn); an output row is finished when a source row beyond its last arrives, or when the rows have run out.  A row piece
    // wider than the tile is cut (more than C_TILE_PX source pixels under C_COLS output columns): then a tile holds one row, so that no
    // output row is finished between the pieces of a source row.
    int r = r0, lo = lo_first, hi = lo + L, qb = (hi - 1) / U;
    if (any) {
        const int rows_tile = pB - pA + 1 > C_TILE_PX ? 1 : TR;
        for (int ty = ya; ty <= yb; ty += rows_tile) {
            const int nrow = min(rows_tile, yb - ty + 1);
            for (int pc0 = pA; pc0 <= pB; pc0 += C_TILE_PX) {
                const int pc1 = min(pc0 + C_TILE_PX - 1, pB);
                stage(ty, nrow, pc0);
                for (int i = 0; i < nrow; ++i) {
                    const int sy = ty + i, q = sy - by;
                    if (pc0 == pA)
                        while (q > qb && r < r1 - 1) { finish(r); ++r; lo = hi; hi += L; qb = (hi - 1) / U; }
                    const int wc = max(0, min(hi, U * (q + 1)) - max(lo, U * q)), wn = max(0, min(hi + L, U * (q + 1)) - max(hi, U * q));
                    add_row(i, sy, pc0, pc1, wc, wn);
                }
            }
        }
    }
    for (; r < r1; ++r) finish(r);
}


// ---- the oriented window ---------------------------------------------------------------------------------------------------------------
constexpr int W_SIDE = 16;          // output pixels of a tile along each axis, a lane each (even: a 2 x 2 chroma sample never leaves a block)
constexpr int W_TILE = 24576;       // LDS bytes of a staged box: 6 blocks of 4 waves a CU (24 of its 32 waves, 144 of its 160 KiB).  A 16-pixel
                                    // tile of a face at 3.5 : 1, rolled 30 degrees, touches 78 x 78 source pixels: 19 KiB.  A larger box
                                    // goes to the direct path.
static_assert(W_SIDE % 2 == 0 && W_SIDE * W_SIDE % 64 == 0 && 64 % W_SIDE == 0, "a chroma sample's four lanes lie in one wave");
// the bounds TUBE.md "Oriented window" argues from: which quantities need 64 bits and which fit 32
static_assert((int64_t)8192 * PVF_CROP_MAX_COORD + (int64_t)2 * PVF_WARP_MAX_K * PVF_CROP_MAX_SIZE * PVF_WARP_MAX_STEP + 65536 >= ((int64_t)1 << 31),
              "PX and PY of a sub-sample are 64-bit");
static_assert((((int64_t)8192 * PVF_CROP_MAX_COORD + (int64_t)2 * PVF_WARP_MAX_K * PVF_CROP_MAX_SIZE * PVF_WARP_MAX_STEP + 65536) >> 17) + 1 < ((int64_t)1 << 30),
              "source indices fit int32");
static_assert(131071 + (int64_t)2 * 2 * W_SIDE * PVF_WARP_MAX_K * PVF_WARP_MAX_STEP < ((int64_t)1 << 31), "a sub-sample's position relative to its tile's first fits int32");
static_assert((uint64_t)65536 * PVF_WARP_MAX_K * PVF_WARP_MAX_K * 255 + (uint64_t)32768 * PVF_WARP_MAX_K * PVF_WARP_MAX_K < ((uint64_t)1 << 32),
              "a pixel's sum with its rounding term fits uint32");
static_assert((255 * 2 + 1) * PVF_WARP_MAX_K * PVF_WARP_MAX_K / 2 < 65536 && PVF_WARP_MAX_K * PVF_WARP_MAX_K <= 256, "the quotient's numerator is below 2^16, its divisor at most 256");

struct WarpJob { const uint8_t* img; int32_t h, w, CX, CY, BX, BY, K; uint32_t M; int32_t pad[2]; };      // M = 2^24 / K^2 + 1 (warp_quotient)
static_assert(sizeof(WarpJob) == 48, "WarpJob is three 16-byte units");
struct WarpArgs { const WarpJob* jobs; uint8_t* out; int S, yuv; RenderCoef k; };

// v / d for v < 2^16, d <= 256 with M = 2^24 / d + 1: v M / 2^24 = v / d + v e / (d 2^24) with e = M d - 2^24 in 1 .. d, and v e < 2^24, so
// the excess is below 1 / d, the least distance from v / d to the next integer (tests/csrc/warp_quotient_check.c runs every d and v)
__host__ __device__ __forceinline__ uint32_t warp_quotient(uint32_t v, uint32_t M) { return (uint32_t)(((uint64_t)v * M) >> 24); }

// grid (tiles across * tiles down, crops of the round), W_SIDE * W_SIDE lanes.
// Units: 1 / 131072 pixel.  O = (OX, OY), 64-bit, is the position of the tile's first sub-sample; split as 2^17 (O >> 17) + (O & 131071) it
// leaves every other sub-sample of the tile at a small int32 offset (static_assert above), and floor() is the arithmetic shift alone.
__global__ void __launch_bounds__(W_SIDE * W_SIDE) warp_k(const WarpArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[W_TILE];
    const int tid = threadIdx.x, S = a.S;
    const int across = (S + W_SIDE - 1) / W_SIDE;
    const int j0 = (int)(blockIdx.x % across) * W_SIDE, i0 = (int)(blockIdx.x / across) * W_SIDE;
    const int4* jq = reinterpret_cast<const int4*>(a.jobs + blockIdx.y);
    const int4 q0 = jq[0], q1 = jq[1], q2 = jq[2];
    const uint8_t* img = reinterpret_cast<const uint8_t*>(((uint64_t)(uint32_t)q0.y << 32) | (uint32_t)q0.x);
    const int h = q0.z, w = q0.w, CX = q1.x, CY = q1.y, BX = q1.z, BY = q1.w, K = q2.x;
    const uint32_t M = (uint32_t)q2.y;
    const int tw = min(W_SIDE, S - j0), th = min(W_SIDE, S - i0);   // the tile's pixels inside the picture
    const int64_t m0 = 2 * (int64_t)j0 * K + 1 - (int64_t)S * K, n0 = 2 * (int64_t)i0 * K + 1 - (int64_t)S * K;
    const int64_t OX = (int64_t)8192 * CX + m0 * BX - n0 * BY - 65536, OY = (int64_t)8192 * CY + m0 * BY + n0 * BX - 65536;
    const int ox = (int)(OX >> 17), oy = (int)(OY >> 17), rx = (int)(OX & 131071), ry = (int)(OY & 131071);

    // the source pixels the tile can touch: a sub-sample's position is affine in (dm, dn), so its first tap is least and greatest at a corner
    const int dmx = 2 * (tw * K - 1), dnx = 2 * (th * K - 1);
    int bx0, bx1, by0, by1;
    {
        const int xa = rx, xb = rx + dmx * BX, xc = rx - dnx * BY, xd = rx + dmx * BX - dnx * BY;
        const int ya = ry, yb = ry + dmx * BY, yc = ry + dnx * BX, yd = ry + dmx * BY + dnx * BX;
        bx0 = max(ox + (min(min(xa, xb), min(xc, xd)) >> 17), 0); bx1 = min(ox + (max(max(xa, xb), max(xc, xd)) >> 17) + 1, w - 1);
        by0 = max(oy + (min(min(ya, yb), min(yc, yd)) >> 17), 0); by1 = min(oy + (max(max(ya, yb), max(yc, yd)) >> 17) + 1, h - 1);
    }
    const bool any = bx0 <= bx1 && by0 <= by1;                      // else everything the tile sees is black: no loads
    const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
    const int pitch = any ? (3 + 3 * bw + 15) & ~15 : 16, n16 = pitch >> 4;
    const bool staged = any && (int64_t)bh * pitch <= W_TILE;

    // crop_k's descriptor: the base aligned down to 4 bytes, the range rounded up to whole dwords
    const unsigned delta = (unsigned)((uintptr_t)img & 3u), rb = 3u * (unsigned)w;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)((uintptr_t)img - delta), 0, (int)((delta + (unsigned)h * rb + 3u) & ~3u), 0x00020000);
    if (staged) {
        for (int u = tid; u < bh * n16; u += W_SIDE * W_SIDE) {     // (bh * n16 <= W_TILE / 16)
            const int i = u / n16, k = u - i * n16;
            const unsigned off = ((delta + (unsigned)(by0 + i) * rb + 3u * (unsigned)bx0) & ~3u) + 16u * (unsigned)k;
            reinterpret_cast<uint4*>(s_tile)[u] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0));
        }
    }
    __syncthreads();

    const int tx = tid % W_SIDE, ty = tid / W_SIDE, j = j0 + tx, i = i0 + ty;
    const bool live = tx < tw && ty < th;
    uint32_t sum[3] = {0, 0, 0};
    if (live && any) {
        // one tap: a pixel outside the box is outside the frame, or no sub-sample of the tile reaches it; it reads black, its weight counted
        auto tap = [&](int x, int y, uint32_t wgt) {
            if (x < bx0 || x > bx1 || y < by0 || y > by1 || wgt == 0) return;
            const unsigned at = delta + (unsigned)y * rb + 3u * (unsigned)x;
            if (staged) {
                const uint8_t* s = s_tile + (y - by0) * pitch + (int)((delta + (unsigned)y * rb + 3u * (unsigned)bx0) & 3u) + 3 * (x - bx0);
                sum[0] += wgt * s[0]; sum[1] += wgt * s[1]; sum[2] += wgt * s[2];
            } else {
                sum[0] += wgt * (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)at, 0, 0);
                sum[1] += wgt * (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)at + 1, 0, 0);
                sum[2] += wgt * (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)at + 2, 0, 0);
            }
        };
        const int px = rx + 2 * tx * K * BX - 2 * ty * K * BY, py = ry + 2 * tx * K * BY + 2 * ty * K * BX;       // sub-sample (0, 0) of this pixel
        for (int b = 0; b < K; ++b) {
            int sx = px - 2 * b * BY, sy = py + 2 * b * BX;
            for (int c = 0; c < K; ++c, sx += 2 * BX, sy += 2 * BY) {
                const int x0 = ox + (sx >> 17), y0 = oy + (sy >> 17);
                const uint32_t fx = (uint32_t)(sx & 131071) >> 9, fy = (uint32_t)(sy & 131071) >> 9;
                tap(x0, y0, (256u - fx) * (256u - fy)); tap(x0 + 1, y0, fx * (256u - fy));
                tap(x0, y0 + 1, (256u - fx) * fy); tap(x0 + 1, y0 + 1, fx * fy);
            }
        }
    }
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (int)warp_quotient((sum[c] + 32768u * (uint32_t)(K * K)) >> 16, M);

    const int cw = (S + 1) >> 1;
    const size_t crop_bytes = a.yuv ? (size_t)S * S + 2 * (size_t)cw * cw : (size_t)S * S * 3;
    uint8_t* out = a.out + (size_t)blockIdx.y * crop_bytes;
    if (!a.yuv) {
        if (live) { uint8_t* o = out + ((size_t)i * S + j) * 3; o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2]; }
        return;
    }
    if (live) out[(size_t)i * S + j] = (uint8_t)yuv_luma(a.k, v[0], v[1], v[2]);
    // chroma: the lane to the right (tid ^ 1) and the pair below (tid ^ W_SIDE) lie in this wave; a pixel past an odd picture's edge is its
    // neighbour counted again, as crop_k counts it
    int quad[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int right = __shfl_xor(v[c], 1);
        const int pair = v[c] + (j + 1 < S ? right : v[c]);
        const int below = __shfl_xor(pair, W_SIDE);
        quad[c] = pair + (i + 1 < S ? below : pair);
    }
    if (live && !(i & 1) && !(j & 1)) {
        uint8_t* up = out + (size_t)S * S + (size_t)(i >> 1) * cw + (j >> 1);
        up[0] = (uint8_t)yuv_chroma(a.k.u, quad[0], quad[1], quad[2]);
        up[(size_t)cw * cw] = (uint8_t)yuv_chroma(a.k.v, quad[0], quad[1], quad[2]);
    }
}

// ---- the call ------------------------------------------------------------------------------------------------------------------------
// what the context keeps for pvf_frame_crops: the two output buffers of the rounds, the job table, a copy stream and the events that
// order a round's copy behind its kernel and the kernel after next behind the copy
struct TubeState {
    hipStream_t copy = nullptr;
    DevBuf out[2], jobs;
    hipEvent_t made[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
};

static TubeState& tstate(Ctx* c)
{
    if (!c->tube_state) {
        std::unique_ptr<TubeState> s(new TubeState());
        HIP_CHECK(hipStreamCreateWithFlags(&s->copy, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            HIP_CHECK(hipEventCreateWithFlags(&s->made[k], hipEventDisableTiming));
            HIP_CHECK(hipEventCreateWithFlags(&s->copied[k], hipEventDisableTiming));
        }
        c->tube_state = s.release();
    }
    return *reinterpret_cast<TubeState*>(c->tube_state);
}

void tube_free_all(Ctx* c)
{
    if (!c->tube_state) return;
    TubeState* s = reinterpret_cast<TubeState*>(c->tube_state);
    if (s->copy) { (void)hipStreamSynchronize(s->copy); (void)hipStreamDestroy(s->copy); }
    for (int k = 0; k < 2; ++k) {
        if (s->made[k]) (void)hipEventDestroy(s->made[k]);
        if (s->copied[k]) (void)hipEventDestroy(s->copied[k]);
    }
    delete s;
    c->tube_state = nullptr;
}

// crops of a round: as many as C_ROUND_BYTES of output hold, or what PVF_CROP_ROUND says, read when the call is made (tests lower it)
static int crops_per_round(size_t crop_bytes)
{
    int m = (int)std::max<size_t>(1, C_ROUND_BYTES / crop_bytes);
    const char* e = getenv("PVF_CROP_ROUND");
    if (e && atoi(e) > 0) m = atoi(e);
    return std::min(m, C_ROUND_MAX);
}

static size_t picture_bytes(int S, bool yuv)
{
    const int cw = (S + 1) / 2;
    return yuv ? (size_t)S * S + 2 * (size_t)cw * cw : (size_t)S * S * 3;
}

// The rounds of a call, shared by pvf_frame_crops and pvf_frame_warps: the n jobs (in the staging arena) go to the device, then
// launch(jobs of the round on the device, their number, where their pictures go) is called once per round.
template <typename Job, typename Launch>
static void rounds_run(Ctx* c, TubeState& ts, const Job* jobs, int n, size_t crop_bytes, uint8_t* out, bool on_device, Launch launch)
{
    const int round = crops_per_round(crop_bytes);
    ScratchLayout jl, ol;
    const auto sJobs = jl.take<Job>((size_t)n);
    const auto sOut = ol.take<uint8_t>((size_t)std::min(n, round) * crop_bytes);
    ts.jobs.ensure(jl.bytes());
    HIP_CHECK(hipMemcpyAsync(sJobs.in(ts.jobs), jobs, sJobs.bytes(), hipMemcpyHostToDevice, c->stream));
    c->stage.sent(c->stream);
    if (!on_device) { ts.out[0].ensure(ol.bytes()); if (n > round) ts.out[1].ensure(ol.bytes()); }
    // round k's kernel writes buffer k & 1 on the context's stream; its copy to the host runs on the copy stream behind the kernel's event,
    // while round k + 1's kernel, launched before the copy is asked for, runs; round k + 2's kernel waits for the copy's event
    int k = 0, prev_i0 = -1, prev_m = 0;
    auto copy_out = [&](int slot, int i0, int m) {
        HIP_CHECK(hipStreamWaitEvent(ts.copy, ts.made[slot], 0));
        HIP_CHECK(hipMemcpyAsync(out + (size_t)i0 * crop_bytes, sOut.in(ts.out[slot]), (size_t)m * crop_bytes, hipMemcpyDeviceToHost, ts.copy));
        HIP_CHECK(hipEventRecord(ts.copied[slot], ts.copy));
    };
    for (int i0 = 0; i0 < n; i0 += round, ++k) {
        const int m = std::min(round, n - i0), slot = k & 1;
        if (!on_device && k >= 2) HIP_CHECK(hipStreamWaitEvent(c->stream, ts.copied[slot], 0));
        {
            ProfScope prof(c, "tube");
            launch(sJobs.in(ts.jobs) + i0, m, on_device ? out + (size_t)i0 * crop_bytes : sOut.in(ts.out[slot]));
            HIP_CHECK(hipGetLastError());
        }
        if (on_device) continue;
        HIP_CHECK(hipEventRecord(ts.made[slot], c->stream));
        if (prev_i0 >= 0) copy_out(slot ^ 1, prev_i0, prev_m);
        prev_i0 = i0; prev_m = m;
    }
    if (!on_device) { copy_out((k - 1) & 1, prev_i0, prev_m); HIP_CHECK(hipStreamSynchronize(ts.copy)); }
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

static void crops_run(Ctx* c, const pvf_handle* frames, const int32_t* windows, int n, int S, int flags, uint8_t* out, bool on_device)
{
    const std::string w("pvf_frame_crops");
    PVF_REQUIRE(n >= 0 && n <= PVF_CROP_MAX_CROPS, w + ": n outside 0 .. PVF_CROP_MAX_CROPS");
    if (n == 0) return;
    PVF_REQUIRE(frames && windows && out, w + ": null frames, windows or output");
    PVF_REQUIRE(S >= PVF_CROP_MIN_SIZE && S <= PVF_CROP_MAX_SIZE, w + ": S outside PVF_CROP_MIN_SIZE .. PVF_CROP_MAX_SIZE");
    PVF_REQUIRE((flags & ~(PVF_CROP_YUV420 | PVF_YUV_BT709 | PVF_YUV_FULL_RANGE)) == 0, w + ": unknown flags");
    for (int i = 0; i < n; ++i) {                // nothing the kernel computes with is taken on trust
        const int32_t* q = windows + (size_t)3 * i;
        PVF_REQUIRE(q[2] >= PVF_CROP_MIN_SIDE && q[2] <= PVF_CROP_MAX_SIDE, w + ": L outside PVF_CROP_MIN_SIDE .. PVF_CROP_MAX_SIDE");
        PVF_REQUIRE(q[0] >= -PVF_CROP_MAX_COORD && q[0] <= PVF_CROP_MAX_COORD && q[1] >= -PVF_CROP_MAX_COORD && q[1] <= PVF_CROP_MAX_COORD,
                    w + ": X0 or Y0 beyond PVF_CROP_MAX_COORD");
    }
    TubeState& ts = tstate(c);
    CropJob* jobs = reinterpret_cast<CropJob*>(c->stage.take((size_t)n * sizeof(CropJob)));
    for (int i = 0; i < n; ++i) {
        const Frame f = c->frame(frames[i]);
        PVF_REQUIRE(f.h >= 1 && f.w >= 1 && (int64_t)f.h * f.w * 3 + 6 < ((int64_t)1 << 31), w + ": a frame of 2 GiB or more");
        jobs[i] = CropJob{f.d, f.h, f.w, windows[3 * i], windows[3 * i + 1], windows[3 * i + 2], 0};
    }
    const bool yuv = flags & PVF_CROP_YUV420;
    const int pieces = (S + C_COLS - 1) / C_COLS, bands = (S + C_BAND - 1) / C_BAND;
    CropArgs a{nullptr, nullptr, S, yuv ? 1 : 0, render_coef(flags)};
    rounds_run(c, ts, jobs, n, picture_bytes(S, yuv), out, on_device, [&](const CropJob* dev_jobs, int m, uint8_t* dst) {
        a.jobs = dev_jobs; a.out = dst;
        hipLaunchKernelGGL(crop_k, dim3((unsigned)(pieces * bands), (unsigned)m), dim3(C_COLS), 0, c->stream, a);
    });
}

static void warps_run(Ctx* c, const pvf_handle* frames, const int32_t* windows, int n, int S, int flags, uint8_t* out, bool on_device)
{
    const std::string w("pvf_frame_warps");
    PVF_REQUIRE(n >= 0 && n <= PVF_CROP_MAX_CROPS, w + ": n outside 0 .. PVF_CROP_MAX_CROPS");
    if (n == 0) return;
    PVF_REQUIRE(frames && windows && out, w + ": null frames, windows or output");
    PVF_REQUIRE(S >= PVF_CROP_MIN_SIZE && S <= PVF_CROP_MAX_SIZE, w + ": S outside PVF_CROP_MIN_SIZE .. PVF_CROP_MAX_SIZE");
    PVF_REQUIRE((flags & ~(PVF_CROP_YUV420 | PVF_YUV_BT709 | PVF_YUV_FULL_RANGE)) == 0, w + ": unknown flags");
    for (int i = 0; i < n; ++i) {                // nothing the kernel computes with is taken on trust
        const int32_t* q = windows + (size_t)5 * i;
        PVF_REQUIRE(q[4] >= 1 && q[4] <= PVF_WARP_MAX_K, w + ": K outside 1 .. PVF_WARP_MAX_K");
        PVF_REQUIRE(q[2] >= -PVF_WARP_MAX_STEP && q[2] <= PVF_WARP_MAX_STEP && q[3] >= -PVF_WARP_MAX_STEP && q[3] <= PVF_WARP_MAX_STEP,
                    w + ": BX or BY beyond PVF_WARP_MAX_STEP");
        PVF_REQUIRE(q[0] >= -PVF_CROP_MAX_COORD && q[0] <= PVF_CROP_MAX_COORD && q[1] >= -PVF_CROP_MAX_COORD && q[1] <= PVF_CROP_MAX_COORD,
                    w + ": CX or CY beyond PVF_CROP_MAX_COORD");
    }
    TubeState& ts = tstate(c);
    WarpJob* jobs = reinterpret_cast<WarpJob*>(c->stage.take((size_t)n * sizeof(WarpJob)));
    for (int i = 0; i < n; ++i) {
        const Frame f = c->frame(frames[i]);
        PVF_REQUIRE(f.h >= 1 && f.w >= 1 && (int64_t)f.h * f.w * 3 + 6 < ((int64_t)1 << 31), w + ": a frame of 2 GiB or more");
        const int32_t* q = windows + (size_t)5 * i;
        jobs[i] = WarpJob{f.d, f.h, f.w, q[0], q[1], q[2], q[3], q[4], ((uint32_t)1 << 24) / (uint32_t)(q[4] * q[4]) + 1u, {0, 0}};
    }
    const bool yuv = flags & PVF_CROP_YUV420;
    const int tiles = (S + W_SIDE - 1) / W_SIDE;
    WarpArgs a{nullptr, nullptr, S, yuv ? 1 : 0, render_coef(flags)};
    rounds_run(c, ts, jobs, n, picture_bytes(S, yuv), out, on_device, [&](const WarpJob* dev_jobs, int m, uint8_t* dst) {
        a.jobs = dev_jobs; a.out = dst;
        hipLaunchKernelGGL(warp_k, dim3((unsigned)(tiles * tiles), (unsigned)m), dim3(W_SIDE * W_SIDE), 0, c->stream, a);
    });
}

#define API_BEGIN try {
#define API_END                                                        \
    return 0;                                                          \
    }                                                                  \
    catch (const std::exception& e) { pvf_set_error(e.what()); return -1; } \
    catch (...) { pvf_set_error("unknown error"); return -2; }

extern "C" int32_t pvf_frame_crops(pvf_handle h, const pvf_handle* frames, const int32_t* windows, int32_t n, int32_t S, int32_t flags, uint8_t* out,
                                   int32_t out_on_device)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    std::lock_guard<std::recursive_mutex> _api_lock(c->api_mu);
    HIP_CHECK(hipSetDevice(c->device));
    crops_run(c, frames, windows, n, S, flags, out, out_on_device != 0);
    API_END
}

extern "C" int32_t pvf_frame_warps(pvf_handle h, const pvf_handle* frames, const int32_t* windows, int32_t n, int32_t S, int32_t flags, uint8_t* out,
                                   int32_t out_on_device)
{
    API_BEGIN
    Ctx* c = pvf_ctx(h);
    std::lock_guard<std::recursive_mutex> _api_lock(c->api_mu);
    HIP_CHECK(hipSetDevice(c->device));
    warps_run(c, frames, windows, n, S, flags, out, out_on_device != 0);
    API_END
}
