// clothes.hip -- the `clothes` verb's device side (CLOTHES.md): colour histograms over windows of resident frames, summed per group and band.
//   hist_zero_k   the result, uint32 [G][B][256], set to zero.
//   box_hist_k    a workgroup per piece.  The host cuts every clipped window into pieces of at most 16 rows by 256 columns that lie in one
//                 band, so a piece has one destination row (group, band) and a window costs what it reads.  The piece's rows are staged in
//                 LDS as aligned 16-byte chunks at any byte alignment of the frame; a lane owns 16 consecutive pixels of one row, merges
//                 equal consecutive bins and adds the runs to its wave's 256-bin table with LDS atomic adds; after a barrier lane b adds
//                 the sum of the four tables' bin b, where non-zero, to the destination row with a global atomicAdd on uint32.
// Everything is integer arithmetic; sums of integers do not depend on the order of the adds (tests/clothes_ref.py restates it; held bit
// for bit).
#include "pvf_internal.h"
#include <algorithm>
#include <cstdlib>
#include <vector>

constexpr int BH_COLS = 256, BH_ROWS = 16;                 // the largest piece
constexpr int BH_LANES = 256, BH_RUN = 16;                 // a lane owns BH_RUN consecutive pixels of one row
constexpr int BH_PITCH = (3 * BH_COLS + 15 + 15) & ~15;    // bytes of a staged row: 768 of the piece and up to 15 in front, in 16-byte chunks
constexpr int BH_N16 = BH_PITCH / 16;
constexpr int BH_PER_LANE = (BH_ROWS * BH_N16 + BH_LANES - 1) / BH_LANES;      // 16-byte chunks a lane fetches
static_assert(BH_PITCH == 784 && BH_N16 == 49 && BH_PER_LANE == 4 && BH_ROWS * (BH_COLS / BH_RUN) == BH_LANES, "box_hist_k's layout");

struct HistPiece {
    const uint8_t* img;              // the frame, [h][w][3]
    uint32_t frame_bytes;            // 3 w h
    uint32_t off;                    // of the piece's first pixel in the frame, bytes
    uint32_t rowb;                   // 3 w
    uint16_t ncols, nrows;           // 1 .. 256, 1 .. 16
    uint32_t dest;                   // group * B + band
    uint32_t pad;
};
static_assert(sizeof(HistPiece) == 32, "HistPiece is uploaded as it is");

// CLOTHES.md "Bin of a pixel".  The shifts of c1 + 64, c2 + 64 and 2 B - R - G are arithmetic: they floor negative values.
__device__ __forceinline__ uint32_t hist_bin(int R, int G, int B)
{
    const int Y = (77 * R + 150 * G + 29 * B + 128) >> 8;
    const int c1 = R - G, c2 = (2 * B - R - G) >> 1;
    const int q1 = min(max((c1 + 64) >> 4, 0), 7), q2 = min(max((c2 + 64) >> 4, 0), 7);
    return (uint32_t)((Y >> 6) * 64 + q1 * 8 + q2);
}

__global__ void __launch_bounds__(256) hist_zero_k(uint32_t* out, size_t words)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) out[i] = 0u;
}

// grid (pieces), 256 lanes.  Row r of the piece is the bytes [A, A + 3 ncols), A = img + off + r rowb at any byte; its chunk k is the
// aligned 16 bytes at (A & ~15) + 16 k, so chunk 0 starts up to 15 bytes before A and the row's last byte lies below 15 + 768 <= BH_PITCH.
// A chunk inside [img, img + frame_bytes) is one load; the frame's first or last chunk is read byte by byte, the frame's bytes alone; a
// chunk behind the row's last byte or of a row r >= nrows is not read, and no lane reads its place in LDS for a pixel it counts.  Lane
// (row, seg) counts the pixels 16 seg .. 16 seg + 15 of its row that lie below ncols: it reads the 13 aligned words that hold their 48
// bytes (at most byte 784 of the row: inside s_tile) and takes the bytes out with alignbyte.
__global__ void __launch_bounds__(BH_LANES) box_hist_k(const HistPiece* __restrict__ pieces, uint32_t* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[BH_ROWS * BH_PITCH];
    __shared__ uint32_t s_tab[BH_LANES / 64][256];
    const int tid = threadIdx.x;
    const HistPiece p = pieces[blockIdx.x];
    const int ncols = p.ncols, nrows = p.nrows;
    const uintptr_t fb = reinterpret_cast<uintptr_t>(p.img), fe = fb + p.frame_bytes;
    const uint32_t nbytes = 3u * (uint32_t)ncols;
#pragma unroll
    for (int j = 0; j < BH_LANES / 64; ++j) s_tab[j][tid] = 0u;
#pragma unroll
    for (int j = 0; j < BH_PER_LANE; ++j) {
        const int u = tid + BH_LANES * j, r = u / BH_N16, k = u - r * BH_N16;
        if (r >= nrows) continue;                              // (also the chunks past the 16 rows)
        const uintptr_t A = fb + p.off + (uintptr_t)r * p.rowb;
        const uintptr_t q = (A & ~(uintptr_t)15) + 16u * (uint32_t)k;
        if (q >= A + nbytes) continue;
        uint4 v;
        if (q >= fb && q + 16 <= fe) v = *reinterpret_cast<const uint4*>(q);
        else {
            uint32_t d[4] = {0u, 0u, 0u, 0u};
            for (int e = 0; e < 16; ++e)
                if (q + e >= fb && q + e < fe) d[e >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(q + e) << (8 * (e & 3));
            v = make_uint4(d[0], d[1], d[2], d[3]);
        }
        *reinterpret_cast<uint4*>(s_tile + 16 * u) = v;
    }
    __syncthreads();
    const int row = tid >> 4, x0 = (tid & 15) * BH_RUN;
    if (row < nrows && x0 < ncols) {
        const int m = min(BH_RUN, ncols - x0);
        const uint32_t sh = (uint32_t)((fb + p.off + (uintptr_t)row * p.rowb) & 15u);
        const uint32_t start = (uint32_t)row * BH_PITCH + sh + 3u * (uint32_t)x0;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(s_tile + (start & ~3u));
        const uint32_t by = start & 3u;
        uint32_t a[3 * BH_RUN / 4 + 1], d[3 * BH_RUN / 4];
#pragma unroll
        for (int i = 0; i < 3 * BH_RUN / 4 + 1; ++i) a[i] = src[i];
#pragma unroll
        for (int i = 0; i < 3 * BH_RUN / 4; ++i) d[i] = __builtin_amdgcn_alignbyte(a[i + 1], a[i], by);
        uint32_t* tab = s_tab[tid >> 6];
        uint32_t cur = 0u, run = 0u;                           // a run of equal consecutive bins is one add
#pragma unroll
        for (int i = 0; i < BH_RUN; ++i) {
            if (i < m) {
                const int b0 = 3 * i, b1 = b0 + 1, b2 = b0 + 2;
                const int R = (int)((d[b0 >> 2] >> (8 * (b0 & 3))) & 255u), G = (int)((d[b1 >> 2] >> (8 * (b1 & 3))) & 255u),
                          B = (int)((d[b2 >> 2] >> (8 * (b2 & 3))) & 255u);
                const uint32_t bin = hist_bin(R, G, B);
                if (run && bin != cur) { atomicAdd(&tab[cur], run); run = 0u; }
                cur = bin; ++run;
            }
        }
        if (run) atomicAdd(&tab[cur], run);
    }
    __syncthreads();
    const uint32_t sum = s_tab[0][tid] + s_tab[1][tid] + s_tab[2][tid] + s_tab[3][tid];
    if (sum) atomicAdd(out + (size_t)p.dest * 256 + tid, sum);
}

// pieces of a round: what the staging buffer and the device list hold at a time (PVF_HIST_ROUND overrides, for the tests)
static size_t hist_round()
{
    size_t m = (size_t)1 << 18;                  // 8 MiB of pieces
    const char* e = getenv("PVF_HIST_ROUND");
    if (e && atoi(e) > 0) m = (size_t)atoi(e);
    return m;
}

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }           // a >= 0, b > 0

struct HistWin { const uint8_t* d; int h, w; int64_t y0, y1, cx0, cy0, cx1, cy1; };      // the window's rows and its clip, empty: cx1 <= cx0

static void frame_hist_run(Ctx* c, const pvf_handle* frames, const int32_t* windows, const int32_t* group, int n, int G, int B, uint32_t* out,
                           bool on_device)
{
    const std::string w("pvf_frame_hist");
    PVF_REQUIRE(n >= 0 && n <= PVF_HIST_MAX_WINDOWS, w + ": n outside 0 .. PVF_HIST_MAX_WINDOWS");
    PVF_REQUIRE(G >= 1, w + ": G below 1");
    PVF_REQUIRE(B >= 1 && B <= PVF_HIST_MAX_BANDS, w + ": B outside 1 .. 4");
    PVF_REQUIRE((int64_t)G * B <= PVF_HIST_MAX_ROWS, w + ": G * B beyond PVF_HIST_MAX_ROWS");
    PVF_REQUIRE(n == 0 || (frames && windows && group && out), w + ": null frames, windows, group or out");
    if (!out) return;
    for (int i = 0; i < n; ++i) PVF_REQUIRE(group[i] >= 0 && group[i] < G, w + ": a group outside 0 .. G - 1");
    std::vector<HistWin> win((size_t)n);
    std::vector<uint64_t> total((size_t)G, 0);
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const Frame f = c->frame(frames[i]);                   // (orders the stream behind the frame's upload)
        PVF_REQUIRE(f.h >= 1 && f.w >= 1 && (int64_t)f.h * f.w * 3 + 6 < ((int64_t)1 << 31), w + ": a frame of 2 GiB or more");
        HistWin& q = win[(size_t)i];
        q.d = f.d; q.h = f.h; q.w = f.w;
        const int64_t x0 = windows[4 * (size_t)i], x1 = windows[4 * (size_t)i + 2];         // 64 bits from here on: no difference wraps
        q.y0 = windows[4 * (size_t)i + 1]; q.y1 = windows[4 * (size_t)i + 3];
        q.cx0 = std::max<int64_t>(x0, 0); q.cy0 = std::max<int64_t>(q.y0, 0);
        q.cx1 = std::min<int64_t>(x1, f.w); q.cy1 = std::min<int64_t>(q.y1, f.h);
        if (q.cx1 <= q.cx0 || q.cy1 <= q.cy0) { q.cx1 = q.cx0; continue; }      // (an inverted window clips to nothing as well)
        any = true;
        total[(size_t)group[i]] += (uint64_t)((q.cx1 - q.cx0) * (q.cy1 - q.cy0));       // (65536 frames below 2^30 pixels: far inside 64 bits)
    }
    for (int g = 0; g < G; ++g) PVF_REQUIRE(total[(size_t)g] < ((uint64_t)1 << 32), w + ": a group of 2^32 pixels or more in one call");

    const size_t words = (size_t)G * B * 256, round = hist_round();
    ScratchLayout lay;
    const auto sPieces = lay.take<HistPiece>(any ? round : 0);
    const auto sOut = lay.take<uint32_t>(on_device ? 0 : words);
    c->s_act0.ensure(lay.bytes());
    uint32_t* d_out = on_device ? out : sOut.in(c->s_act0);
    {
        ProfScope prof(c, "hist_zero");
        hipLaunchKernelGGL(hist_zero_k, dim3((unsigned)std::min<size_t>((words + 255) / 256, 4096)), dim3(256), 0, c->stream, d_out, words);
        HIP_CHECK(hipGetLastError());
    }
    HistPiece* host = nullptr;
    size_t m = 0;
    auto flush = [&]() {
        if (!m) return;
        HIP_CHECK(hipMemcpyAsync(sPieces.in(c->s_act0), host, m * sizeof(HistPiece), hipMemcpyHostToDevice, c->stream));
        c->stage.sent(c->stream);
        {
            ProfScope prof(c, "hist");
            hipLaunchKernelGGL(box_hist_k, dim3((unsigned)m), dim3(BH_LANES), 0, c->stream, sPieces.in(c->s_act0), d_out);
            HIP_CHECK(hipGetLastError());
        }
        m = 0; host = nullptr;
    };
    for (int i = 0; i < n && any; ++i) {
        const HistWin& q = win[(size_t)i];
        if (q.cx1 <= q.cx0) continue;
        const int64_t H = q.y1 - q.y0;
        const uint32_t rowb = 3u * (uint32_t)q.w, frame_bytes = rowb * (uint32_t)q.h;
        for (int k = 0; k < B; ++k) {
            // band k holds the rows y with ((y - y0) B) // H == k: y - y0 in [ceil(k H / B), ceil((k + 1) H / B))
            const int64_t ya = std::max(q.y0 + ceil_div((int64_t)k * H, B), q.cy0), yb = std::min(q.y0 + ceil_div((int64_t)(k + 1) * H, B), q.cy1);
            for (int64_t y = ya; y < yb; y += BH_ROWS)
                for (int64_t x = q.cx0; x < q.cx1; x += BH_COLS) {
                    if (!host) host = reinterpret_cast<HistPiece*>(c->stage.take(round * sizeof(HistPiece)));
                    host[m++] = HistPiece{q.d, frame_bytes, (uint32_t)(y * rowb + 3 * x), rowb, (uint16_t)std::min<int64_t>(BH_COLS, q.cx1 - x),
                                          (uint16_t)std::min<int64_t>(BH_ROWS, yb - y), (uint32_t)(group[i] * B + k), 0u};
                    if (m == round) flush();
                }
        }
    }
    flush();
    if (!on_device) HIP_CHECK(hipMemcpyAsync(out, d_out, words * 4, hipMemcpyDeviceToHost, c->stream));
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

extern "C" int32_t pvf_frame_hist(pvf_handle h, const pvf_handle* frames, const int32_t* windows, const int32_t* group, int32_t n, int32_t G, int32_t B,
                                  uint32_t* out, int32_t out_on_device)
{
    API_BEGIN
    ENTER(c, h);
    frame_hist_run(c, frames, windows, group, n, G, B, out, out_on_device != 0);
    API_END
}
