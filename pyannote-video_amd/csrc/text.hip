// text.hip -- the `text` verb's device side (CAPTION.md): the text record of every frame, from which `caption` finds name straps and subtitles.
//   text_cells_k  per 16 x 16 cell of a full-resolution frame the counts E (stroke pixels), S (strokes that persist from the frame before),
//                 M (moved pixels) and NP, and the mask bit S >= on.  A workgroup owns 16 cells of one cell row (256 columns) and walks the
//                 frames of the call in order: a lane owns one pixel row of one cell and keeps the luma and the stroke bits of the frame
//                 before in registers, so a frame's bytes are fetched once, with the next frame's loads in flight during the arithmetic.
//   text_head_k   words 0 .. 7 of a frame's row: the sums of the counts and the number of set bits.  A block per frame.
// Everything is integer arithmetic and every cell is written once: no atomics (tests/text_ref.py restates it; held bit for bit).
#include "pvf_internal.h"
#include <algorithm>
#include <cstdlib>

constexpr int TX_CELL = PVF_TEXT_CELL, TX_HEAD = PVF_TEXT_HEAD_WORDS;
constexpr int TX_STRIP_CELLS = 16;                         // cells of a workgroup: half a mask word
constexpr int TX_STRIP = TX_STRIP_CELLS * TX_CELL;         // 256 columns, and one more on either side for the central difference
constexpr int TX_LANES = TX_STRIP_CELLS * TX_CELL;         // a lane per (cell, pixel row)
constexpr int TX_PITCH = (3 * (TX_STRIP + 2) + 30) & ~15;  // bytes of a staged row: 774 of the strip and up to 15 in front, in 16-byte chunks
constexpr int TX_N16 = TX_PITCH / 16;
constexpr int TX_PER_LANE = (TX_CELL * TX_N16 + TX_LANES - 1) / TX_LANES;      // 16-byte chunks a lane fetches of a frame
static_assert(TX_CELL == 16 && TX_HEAD == 8 && TX_LANES == 256 && TX_PITCH == 800 && TX_PER_LANE == 4, "text_cells_k's layout");

struct TextArgs {
    const uint8_t* const* frames;    // [n] device addresses of the frames, [h][w][3]
    const uint8_t* prev;             // the frame in front of frames[0], or null
    int n, h, w, cw, ch, wpr, edge, still, on;
    uint16_t* counts;                // [n][ch][cw][4] = E, S, M, NP
    uint32_t* rows;                  // [n][8 + ch wpr]
};

// the sum over the 16 lanes of a DPP row, in every lane of it
__device__ __forceinline__ uint32_t row16_sum(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128 /* row_ror:8 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124 /* row_ror:4 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122 /* row_ror:2 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121 /* row_ror:1 */, 0xf, 0xf, false);
    return v;
}

// The lane's 16-byte chunks of the strip's rows of one frame, into registers.  Chunk u = (row r, chunk k of the row): the row's bytes
// are [A, A + nbytes) with A = frame + off at any byte; chunk k is the aligned 16 bytes at (A & ~15) + 16 k, so chunk 0 starts up to 15
// bytes before A.  A chunk that lies inside [frame, frame + 3 w h) is one load; the frame's first or last chunk is read byte by byte, the
// frame's bytes alone; a chunk behind the row's last byte, or of a row below the frame (off = TX_NO_ROW), is not read: nothing reads its
// place in LDS.  off[j] and k16[j] = 16 k belong to the lane's chunk u = tid + 256 j and are the same for every frame (3 w h < 2^28).
constexpr uint32_t TX_NO_ROW = 0xFFFFFFFFu;
__device__ __forceinline__ void text_fetch(uint4 (&v)[TX_PER_LANE], const uint8_t* img, uint32_t frame_bytes, const uint32_t (&off)[TX_PER_LANE],
                                           const uint32_t (&k16)[TX_PER_LANE], uint32_t nbytes)
{
    const uintptr_t fb = reinterpret_cast<uintptr_t>(img), fe = fb + frame_bytes;
#pragma unroll
    for (int j = 0; j < TX_PER_LANE; ++j) {
        v[j] = make_uint4(0u, 0u, 0u, 0u);
        if (off[j] == TX_NO_ROW) continue;
        const uintptr_t A = fb + off[j];
        const uintptr_t q = (A & ~(uintptr_t)15) + k16[j];
        if (q >= A + nbytes) continue;
        if (q >= fb && q + 16 <= fe) v[j] = *reinterpret_cast<const uint4*>(q);
        else {
            uint32_t d[4] = {0u, 0u, 0u, 0u};
            for (int e = 0; e < 16; ++e)
                if (q + e >= fb && q + e < fe) d[e >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(q + e) << (8 * (e & 3));
            v[j] = make_uint4(d[0], d[1], d[2], d[3]);
        }
    }
}

// grid (ceil(cw / 16), ch), 256 lanes.  Block (sx, cr) owns the cells 16 sx .. 16 sx + 15 of cell row cr: pixel rows y0 = 16 cr .. and
// columns x0 = 256 sx ..; it stages the columns [pa, pb) = [max(x0 - 1, 0), min(x0 + 257, w)) of its nr = min(16, h - y0) rows.  Lane
// (cell, row) reads the 18 pixels xf - 1 .. xf + 16 of its row, xf = 16 c, with the column clamped to [0, w - 1], which lies inside
// [pa, pb): byte sh + 3 (x - pa) + {0, 1, 2} of the staged row, sh = the row's address & 15, at most 15 + 3 * 257 + 2 < TX_PITCH.  Lanes
// of rows below the frame or of cells right of it read nothing and add nothing.  The three sums of a cell are at most 256 each and travel
// in one word, 10 bits apart.  Writes: the cell's four counts (one 8-byte store by the cell's first lane, cells c < cw only) and the
// strip's 16 mask bits (one store by lane 0: half of mask word sx / 2, or the whole word when the strip is the row's last and even).
__global__ void __launch_bounds__(TX_LANES) text_cells_k(const TextArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[TX_CELL * TX_PITCH];
    __shared__ uint32_t s_bits[TX_LANES / 64];
    const int tid = threadIdx.x, sx = blockIdx.x, cr = blockIdx.y;
    const int w = a.w, h = a.h;
    const int x0 = sx * TX_STRIP, y0 = cr * TX_CELL;
    const int pa = max(x0 - 1, 0), pb = min(x0 + TX_STRIP + 1, w), nbytes = 3 * (pb - pa);
    const int nr = min(TX_CELL, h - y0);
    const uint32_t rowb = (uint32_t)w * 3u, frame_bytes = rowb * (uint32_t)h;
    const int cell = tid >> 4, row = tid & 15, c = sx * TX_STRIP_CELLS + cell, xf = c * TX_CELL;
    const bool live = row < nr && c < a.cw;
    const uint32_t inmask = live ? (1u << min(TX_CELL, w - xf)) - 1u : 0u;     // the lane's pixels inside the frame
    const uint32_t row_off = (uint32_t)(y0 + row) * rowb + (uint32_t)pa * 3u;  // (read by live lanes only)
    const int xl = 3 * (max(xf - 1, 0) - pa);
    uint32_t off[TX_PER_LANE], k16[TX_PER_LANE];
#pragma unroll
    for (int j = 0; j < TX_PER_LANE; ++j) {
        const int u = tid + TX_LANES * j, r = u / TX_N16;
        k16[j] = 16u * (uint32_t)(u - r * TX_N16);
        off[j] = r < nr ? (uint32_t)(y0 + r) * rowb + (uint32_t)pa * 3u : TX_NO_ROW;      // (nr <= 16: also the chunks past the 16 rows)
    }
    uint32_t py[4] = {0u, 0u, 0u, 0u}, pstroke = 0u;           // the frame before: the lane's 16 lumas and stroke bits
    int still = 255;                             // without a predecessor nothing has moved, and pstroke = 0: nothing persists
    uint4 v[TX_PER_LANE];
    int t = a.prev ? -1 : 0;
    text_fetch(v, t < 0 ? a.prev : a.frames[0], frame_bytes, off, k16, (uint32_t)nbytes);
    for (; t < a.n; ++t) {
        const uint8_t* img = t < 0 ? a.prev : a.frames[t];
#pragma unroll
        for (int j = 0; j < TX_PER_LANE; ++j) {
            const int u = tid + TX_LANES * j;
            if (u < TX_CELL * TX_N16) *reinterpret_cast<uint4*>(s_tile + 16 * u) = v[j];
        }
        __syncthreads();
        if (t + 1 < a.n) text_fetch(v, a.frames[t + 1], frame_bytes, off, k16, (uint32_t)nbytes);        // in flight during the arithmetic
        uint32_t cy[4] = {0u, 0u, 0u, 0u}, cstroke = 0u, acc = 0u;
        if (live) {
            const uint32_t sh = ((uint32_t)reinterpret_cast<uintptr_t>(img) + row_off) & 15u;
            const uint8_t* s = s_tile + row * TX_PITCH + sh;
            auto luma = [&](int b) { return (int)((77u * s[b] + 150u * s[b + 1] + 29u * s[b + 2] + 128u) >> 8); };
            const int b0 = 3 * (xf - pa), blast = 3 * (w - 1 - pa);
            int yl = luma(xl), yc = luma(b0);
            uint32_t moved = 0u;
#pragma unroll
            for (int i = 0; i < TX_CELL; ++i) {
                const int yr = luma(min(b0 + 3 * (i + 1), blast));
                const int yp = (int)((py[i >> 2] >> (8 * (i & 3))) & 255u);
                cstroke |= (abs(yr - yl) >= a.edge ? 1u : 0u) << i;
                moved |= (abs(yc - yp) > still ? 1u : 0u) << i;
                cy[i >> 2] |= (uint32_t)yc << (8 * (i & 3));
                yl = yc; yc = yr;
            }
            cstroke &= inmask; moved &= inmask;
            acc = (uint32_t)__popc(cstroke) | (uint32_t)__popc(cstroke & pstroke & ~moved) << 10 | (uint32_t)__popc(moved) << 20;
        }
        acc = row16_sum(acc);
        const uint32_t E = acc & 1023u, S = (acc >> 10) & 1023u, M = acc >> 20;
        const bool first_lane = row == 0 && c < a.cw;          // (row 0 lies inside the frame: nr >= 1)
        const unsigned long long m = __ballot(first_lane && S >= (uint32_t)a.on);
        if ((tid & 63) == 0) s_bits[tid >> 6] = (uint32_t)((m & 1u) | ((m >> 15) & 2u) | ((m >> 30) & 4u) | ((m >> 45) & 8u));
        if (t >= 0 && first_lane) {
            const uint32_t NP = (uint32_t)(nr * min(TX_CELL, w - xf));
            uint16_t* dst = a.counts + (((size_t)t * a.ch + cr) * a.cw + c) * 4;
            *reinterpret_cast<uint2*>(dst) = make_uint2(E | S << 16, M | NP << 16);
        }
        __syncthreads();                         // s_bits is complete; every lane is done with the staged rows
        if (t >= 0 && tid == 0) {
            const uint32_t bits = s_bits[0] | s_bits[1] << 4 | s_bits[2] << 8 | s_bits[3] << 12;
            uint32_t* word = a.rows + (size_t)t * (TX_HEAD + a.ch * a.wpr) + TX_HEAD + cr * a.wpr + (sx >> 1);
            if ((sx & 1) == 0 && (sx + 1) * TX_STRIP_CELLS >= a.cw) *word = bits;
            else reinterpret_cast<uint16_t*>(word)[sx & 1] = (uint16_t)bits;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) py[q] = cy[q];
        pstroke = cstroke;
        still = a.still;
    }
}

__device__ __forceinline__ uint32_t text_wave_sum(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// grid (n), 256 lanes, after text_cells_k.  Words 0 .. 7 of frame f's row: the sizes, the parameters with has_prev, the sums of E, S and
// M over the frame's ch cw cells (at most w h <= 2^26 each), the number of set mask bits, and the caller's two words as 0.  Reads
// counts [f][ch cw][4] and the row's ch wpr mask words, nothing else.
__global__ void __launch_bounds__(256) text_head_k(const TextArgs a)
{
    __shared__ uint32_t s_part[4][4];
    const int tid = threadIdx.x, f = blockIdx.x;
    const int cells = a.ch * a.cw, words = a.ch * a.wpr;
    const uint2* cnt = reinterpret_cast<const uint2*>(a.counts) + (size_t)f * cells;
    uint32_t* row = a.rows + (size_t)f * (TX_HEAD + words);
    uint32_t e = 0, s = 0, m = 0, b = 0;
    for (int i = tid; i < cells; i += 256) { const uint2 q = cnt[i]; e += q.x & 0xFFFFu; s += q.x >> 16; m += q.y & 0xFFFFu; }
    for (int i = tid; i < words; i += 256) b += (uint32_t)__popc(row[TX_HEAD + i]);
    e = text_wave_sum(e); s = text_wave_sum(s); m = text_wave_sum(m); b = text_wave_sum(b);
    if ((tid & 63) == 0) { s_part[0][tid >> 6] = e; s_part[1][tid >> 6] = s; s_part[2][tid >> 6] = m; s_part[3][tid >> 6] = b; }
    __syncthreads();
    if (tid == 0) {
        const uint32_t has_prev = (f > 0 || a.prev) ? 1u : 0u;
        row[0] = (uint32_t)a.w | (uint32_t)a.h << 16;
        row[1] = (uint32_t)a.edge | (uint32_t)a.still << 8 | (uint32_t)a.on << 16 | has_prev << 31;
        for (int k = 0; k < 4; ++k) row[2 + k] = s_part[k][0] + s_part[k][1] + s_part[k][2] + s_part[k][3];
        row[6] = 0u; row[7] = 0u;
    }
}

// frames of a round: what keeps the counts and the rows of a round within 64 MiB of scratch (PVF_TEXT_ROUND overrides, for the tests)
static int text_round(size_t frame_out_bytes)
{
    size_t m = std::max<size_t>(1, ((size_t)64 << 20) / frame_out_bytes);
    const char* e = getenv("PVF_TEXT_ROUND");
    if (e && atoi(e) > 0) m = (size_t)atoi(e);
    return (int)std::min<size_t>(m, PVF_TEXT_MAX_FRAMES);
}

static void frame_text_run(Ctx* c, const pvf_handle* frames, int n, pvf_handle prev, int edge, int still, int on, uint32_t* rows, uint16_t* counts)
{
    const std::string w("pvf_frame_text");
    PVF_REQUIRE(n >= 0 && n <= PVF_TEXT_MAX_FRAMES, w + ": n outside 0 .. PVF_TEXT_MAX_FRAMES");
    if (n == 0) return;
    PVF_REQUIRE(edge >= 1 && edge <= 255, w + ": edge outside 1 .. 255");
    PVF_REQUIRE(still >= 0 && still <= 254, w + ": still outside 0 .. 254");
    PVF_REQUIRE(on >= 1 && on <= 256, w + ": on outside 1 .. 256");
    PVF_REQUIRE(frames && rows, w + ": null frames or rows");
    const uint8_t** table = reinterpret_cast<const uint8_t**>(c->stage.take((size_t)n * sizeof(uint8_t*)));
    int h = 0, fw = 0;
    const uint8_t* d_prev = nullptr;
    for (int i = (prev ? -1 : 0); i < n; ++i) {
        const Frame f = c->frame(i < 0 ? prev : frames[i]);        // (orders the stream behind the frame's upload)
        PVF_REQUIRE(f.h >= 1 && f.w >= 1 && f.h <= PVF_TEXT_MAX_SIDE && f.w <= PVF_TEXT_MAX_SIDE, w + ": a frame side outside 1 .. PVF_TEXT_MAX_SIDE");
        if (h == 0) { h = f.h; fw = f.w; }
        PVF_REQUIRE(f.h == h && f.w == fw, w + ": frames of different sizes");
        if (i < 0) d_prev = f.d; else table[i] = f.d;
    }
    const int cw = (fw + TX_CELL - 1) / TX_CELL, ch = (h + TX_CELL - 1) / TX_CELL, wpr = (cw + 31) / 32;
    const size_t row_words = (size_t)TX_HEAD + (size_t)ch * wpr, cells = (size_t)ch * cw;
    const int round = std::min(n, text_round(row_words * 4 + cells * 8));
    ScratchLayout lay;
    const auto sTable = lay.take<const uint8_t*>((size_t)n);
    const auto sCounts = lay.take<uint16_t>((size_t)round * cells * 4);
    const auto sRows = lay.take<uint32_t>((size_t)round * row_words);
    c->s_act0.ensure(lay.bytes());
    HIP_CHECK(hipMemcpyAsync(sTable.in(c->s_act0), table, (size_t)n * sizeof(uint8_t*), hipMemcpyHostToDevice, c->stream));
    c->stage.sent(c->stream);
    // a later round's predecessor is the last frame of the round before; it writes the same scratch, behind this round's copies on the stream
    for (int i0 = 0; i0 < n; i0 += round) {
        const int m = std::min(round, n - i0);
        const TextArgs a{sTable.in(c->s_act0) + i0, i0 ? table[i0 - 1] : d_prev, m, h, fw, cw, ch, wpr, edge, still, on, sCounts.in(c->s_act0),
                         sRows.in(c->s_act0)};
        {
            ProfScope prof(c, "text");
            hipLaunchKernelGGL(text_cells_k, dim3((unsigned)((cw + TX_STRIP_CELLS - 1) / TX_STRIP_CELLS), (unsigned)ch), dim3(TX_LANES), 0, c->stream, a);
            HIP_CHECK(hipGetLastError());
        }
        {
            ProfScope prof(c, "text_head");
            hipLaunchKernelGGL(text_head_k, dim3((unsigned)m), dim3(256), 0, c->stream, a);
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipMemcpyAsync(rows + (size_t)i0 * row_words, a.rows, (size_t)m * row_words * 4, hipMemcpyDeviceToHost, c->stream));
        if (counts) HIP_CHECK(hipMemcpyAsync(counts + (size_t)i0 * cells * 4, a.counts, (size_t)m * cells * 8, hipMemcpyDeviceToHost, c->stream));
    }
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

extern "C" int32_t pvf_frame_text(pvf_handle h, const pvf_handle* frames, int32_t n, pvf_handle prev, int32_t edge, int32_t still, int32_t on,
                                  uint32_t* rows, uint16_t* counts)
{
    API_BEGIN
    ENTER(c, h);
    frame_text_run(c, frames, n, prev, edge, still, on, rows, counts);
    API_END
}
