// board.hip -- the `storyboard` verb's device side (STORYBOARD.md): whole resident frames as small pictures, and the sheet of them.
//   frame_thumbs_k  the exact area average of an h x w frame into th x tw: a block per (85 output columns, output row, frame) stages the
//                   source rows of its output row in LDS with 16-byte loads and every lane sums the source columns of its own output byte.
//   thumb_tiles_k   a sheet pixel finds the LAST tile that covers it and copies that thumbnail's pixel, else background.
//   sheet_prims_k   (faces.hip, through sheet_prims_launch) the RECT / LINE / TEXT list over the tiles.
// Everything is integer arithmetic (tests/storyboard_ref.py restates it; the kernels are held to it bit for bit).
#include "pvf_internal.h"
#include <algorithm>

constexpr int TB_LANES = 256;
constexpr int TB_SEG_PX = 85;                    // output columns of a block: 255 lanes, one per output byte
constexpr int TB_PIECE_COLS = 1024;              // source columns staged at a time; also the bound of a lane's 32-bit row sum (below)
constexpr int TB_LDS = 20480;                    // bytes of the staged rows: 6 rows of the widest piece (pitch 3088); 8 blocks a CU
constexpr size_t TB_ROUND_BYTES = (size_t)32 << 20;    // output of a round of pictures; tiles of a round of the sheet
constexpr int TB_ROUND_MAX = 32768;              // pictures of a launch (grid z)
static_assert(TB_SEG_PX * 3 <= TB_LANES && ((3 * TB_PIECE_COLS + 30) & ~15) * 6 <= TB_LDS, "frame_thumbs_k's layout");

struct ThumbCol { int32_t ja, jb; uint32_t wfirst, wlast; };     // an output column's source columns and the weights of the two outer ones
struct ThumbRow { int32_t i0, i1; };                           // an output row's source rows [i0, i1)
struct ThumbArgs {
    const uint8_t* const* frames;   // [n] device addresses of the frames, [h][w][3] each
    const ThumbCol* cols;           // [tw]
    const ThumbRow* rows;           // [th]
    int h, w, th, tw;
    uint8_t* out;                   // [n][th][tw][3]
};

// the tables of a call (host, 64-bit arithmetic; a few KB).  Lengths are in units of 1 / tw source pixel (x) and 1 / th (y): source
// column j is [j tw, (j + 1) tw), output column X is [X w, (X + 1) w); wx(X, j) is the length they share.  The source columns of X are
// ja = (X w) / tw .. jb = ((X + 1) w - 1) / tw: ja with wx = min((ja + 1) tw, (X + 1) w) - X w, jb (if jb > ja) with (X + 1) w - jb tw,
// every column between with tw -- one rule for every ratio, enlarging included (then ja = jb mostly).  Rows alike.
static void thumb_tables(int64_t h, int64_t w, int64_t th, int64_t tw, ThumbCol* cols, ThumbRow* rows)
{
    for (int64_t X = 0; X < tw; ++X) {
        const int64_t xa = X * w, xb = xa + w, ja = xa / tw, jb = (xb - 1) / tw;
        cols[X] = ThumbCol{(int32_t)ja, (int32_t)jb, (uint32_t)(std::min((ja + 1) * tw, xb) - xa), jb > ja ? (uint32_t)(xb - jb * tw) : 0u};
    }
    for (int64_t Y = 0; Y < th; ++Y) rows[Y] = ThumbRow{(int32_t)((Y * h) / th), (int32_t)(((Y + 1) * h + th - 1) / th)};
}

// grid (ceil(tw / 85), th, n), 256 lanes.  A lane owns one output byte (X, c); its columns and their weights come from the call's table
// (thumb_tables), the weight of a row from lane-invariant arithmetic.
// The block's source columns are cut into pieces of 1024; the piece's bytes of up to TB_LDS / pitch rows are staged with aligned 16-byte
// loads (a row starts at any byte: its chunk 0 starts up to 15 bytes before the piece, inside the frame or read byte by byte -- nothing
// outside [frame, frame + 3 w h) is read), the lane adds its columns of each staged row:
//   row sum <= 255 (tw 1022 + 2 tw) < 2^28 with tw <= 1024: 32-bit.  Times wy <= 1024 and over rows and pieces: 64-bit, <= 255 w h.
// The quotient (sum + w h / 2) / (w h) is below 256 and w h below 2^30: eight compare-and-subtract steps of a 64-bit long division,
// exact by construction.  No atomics, no float; integer sums, so the order is free.
__global__ void __launch_bounds__(TB_LANES) frame_thumbs_k(const ThumbArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[TB_LDS];
    const int tid = threadIdx.x;
    const int64_t h = a.h, w = a.w, th = a.th;
    const uint32_t tw = (uint32_t)a.tw;
    const int Y = blockIdx.y;
    const int X0 = blockIdx.x * TB_SEG_PX, X1 = min(X0 + TB_SEG_PX, a.tw);
    const uint8_t* __restrict__ img = a.frames[blockIdx.z];
    const uintptr_t fb = reinterpret_cast<uintptr_t>(img), fe = fb + (size_t)h * (size_t)w * 3;
    const ThumbRow yr = a.rows[Y];
    const int i0 = yr.i0, i1 = yr.i1;                          // source rows [i0, i1)
    const int J0 = a.cols[X0].ja, J1 = a.cols[X1 - 1].jb + 1;  // source columns [J0, J1)
    const int X = X0 + tid / 3, c = tid - 3 * (tid / 3);
    const bool live = X < X1;
    const ThumbCol xc = a.cols[live ? X : X0];
    const int ja = xc.ja, jb = xc.jb;
    const uint32_t wfirst = xc.wfirst, wlast = xc.wlast;
    const size_t rowb = (size_t)w * 3;
    uint64_t acc = 0;
    for (int p0 = J0; p0 < J1; p0 += TB_PIECE_COLS) {
        const int ncols = min(TB_PIECE_COLS, J1 - p0), p1 = p0 + ncols;
        const int pitch = (3 * ncols + 30) & ~15, n16 = pitch >> 4, R = TB_LDS / pitch;
        const int la = max(ja + 1, p0), lb = min(jb - 1, p1 - 1);            // the lane's columns of weight tw in this piece
        const bool hasf = ja >= p0 && ja < p1, hasl = jb > ja && jb >= p0 && jb < p1;
        for (int r0 = i0; r0 < i1; r0 += R) {
            const int nr = min(R, i1 - r0);
            __syncthreads();                     // the lanes are done with the rows staged before
            for (int u = tid; u < nr * n16; u += TB_LANES) {
                const int r = u / n16, k = u - r * n16;
                const uintptr_t A = fb + (size_t)(r0 + r) * rowb + (size_t)p0 * 3;       // the piece's first byte of this row
                const uintptr_t q = (A & ~(uintptr_t)15) + 16u * (unsigned)k;
                if (q >= A + 3u * (unsigned)ncols) continue;                  // behind the piece's last byte: nothing reads it
                uint4 v;
                if (q >= fb && q + 16 <= fe) v = *reinterpret_cast<const uint4*>(q);
                else {                           // the frame's first or last chunk: only the bytes of the frame
                    uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int e = 0; e < 16; ++e)
                        if (q + e >= fb && q + e < fe) d[e >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(q + e) << (8 * (e & 3));
                    v = make_uint4(d[0], d[1], d[2], d[3]);
                }
                *reinterpret_cast<uint4*>(s_tile + r * pitch + 16 * k) = v;
            }
            __syncthreads();
            if (!live) continue;
            for (int r = 0; r < nr; ++r) {
                const int64_t i = r0 + r;
                const uint32_t wy = (uint32_t)(min((i + 1) * th, (Y + 1) * h) - max(i * th, Y * h));
                const int sh = (int)((fb + (size_t)i * rowb + (size_t)p0 * 3) & 15);
                const uint8_t* s = s_tile + r * pitch + sh + c;               // column j of the piece: s[3 (j - p0)]
                uint32_t si = 0;
                for (int j = la; j <= lb; j += 4) {                           // four reads in flight; the index is clamped, the sum is not
                    const uint32_t b0 = s[3 * (j - p0)], b1 = s[3 * (min(j + 1, lb) - p0)], b2 = s[3 * (min(j + 2, lb) - p0)];
                    const uint32_t b3 = s[3 * (min(j + 3, lb) - p0)];
                    si += b0 + (j + 1 <= lb ? b1 : 0u) + (j + 2 <= lb ? b2 : 0u) + (j + 3 <= lb ? b3 : 0u);      // <= 255 x 1022 in all
                }
                uint32_t hs = tw * si;
                if (hasf) hs += wfirst * s[3 * (ja - p0)];
                if (hasl) hs += wlast * s[3 * (jb - p0)];
                acc += (uint64_t)wy * hs;
            }
        }
    }
    if (!live) return;
    const uint64_t den = (uint64_t)(w * h);
    uint64_t num = acc + den / 2;                // < 256 den
    uint32_t quo = 0;
#pragma unroll
    for (int k = 7; k >= 0; --k) {
        const uint64_t t = den << k;
        if (num >= t) { num -= t; quo |= 1u << k; }
    }
    a.out[(((size_t)blockIdx.z * a.th + Y) * a.tw + X) * 3 + c] = (uint8_t)quo;
}

// ---- the sheet ----------------------------------------------------------------------------------------------------------------------
constexpr int BS_TW = 32, BS_TH = 8;             // sheet pixels per block, as sheet_tiles_k
constexpr int BS_CHUNK = 256;

struct ThumbTileArgs {
    const uint8_t* thumbs;          // [n][th][tw][3]
    const int32_t* xy;              // [n][2] top-left corners, any int32
    int n, tw, th, W, H;
    uint32_t background;
    int fill;                       // pixels no tile of this launch covers: 1 background, 0 left as they are (a later round of tiles)
    uint8_t* rgb;                   // [H][W][3]
};

// grid (ceil(W / 32), ceil(H / 8)), 256 lanes.  sheet_tiles_k's walk (faces.hip) with rectangular tiles: the tiles from the LAST chunk of
// 256 to the first, culled against the block's rectangle, the survivors in LDS in list order; a pixel keeps the last of the list that
// covers it and copies that thumbnail's pixel.
__global__ void __launch_bounds__(256) thumb_tiles_k(const ThumbTileArgs a)
{
    __shared__ int s_idx[BS_CHUNK], s_x[BS_CHUNK], s_ty[BS_CHUNK];
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int X = blockIdx.x * BS_TW + (tid & (BS_TW - 1)), Y = blockIdx.y * BS_TH + (tid >> 5);
    const bool inside = X < a.W && Y < a.H;
    const int64_t bx0 = (int64_t)blockIdx.x * BS_TW, by0 = (int64_t)blockIdx.y * BS_TH;
    const int64_t bx1 = min(bx0 + BS_TW - 1, (int64_t)a.W - 1), by1 = min(by0 + BS_TH - 1, (int64_t)a.H - 1);
    int best = -1, tx = 0, ty = 0;
    for (int top = a.n; top > 0; top -= BS_CHUNK) {
        const int lo = max(top - BS_CHUNK, 0), i = lo + tid;
        bool hit = false;
        int cx = 0, cy = 0;
        if (i < top) {
            cx = a.xy[2 * i]; cy = a.xy[2 * i + 1];
            hit = cx <= bx1 && (int64_t)cx + a.tw - 1 >= bx0 && cy <= by1 && (int64_t)cy + a.th - 1 >= by0;
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
                if (dx >= 0 && dx < a.tw && dy >= 0 && dy < a.th) { best = s_idx[j]; tx = (int)dx; ty = (int)dy; break; }
            }
        if (__syncthreads_and(!inside || best >= 0)) break;                   // (the barrier in front of the next chunk's stores, too)
    }
    if (!inside) return;
    uint8_t* o = a.rgb + ((size_t)Y * a.W + X) * 3;
    if (best < 0) {
        if (a.fill) { o[0] = (uint8_t)(a.background & 255u); o[1] = (uint8_t)((a.background >> 8) & 255u); o[2] = (uint8_t)((a.background >> 16) & 255u); }
        return;
    }
    const uint8_t* __restrict__ p = a.thumbs + (((size_t)best * a.th + ty) * a.tw + tx) * 3;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

// ---- the calls -----------------------------------------------------------------------------------------------------------------------
// what the context keeps for pvf_frame_thumbs: the two output buffers of the rounds, the frame table, a copy stream and the events that
// order a round's copy behind its kernel and the kernel after next behind the copy (tube.hip's scheme)
struct BoardState {
    hipStream_t copy = nullptr;
    DevBuf out[2], table;
    hipEvent_t made[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
};

static BoardState& bstate(Ctx* c)
{
    if (!c->board_state) {
        std::unique_ptr<BoardState> s(new BoardState());
        HIP_CHECK(hipStreamCreateWithFlags(&s->copy, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            HIP_CHECK(hipEventCreateWithFlags(&s->made[k], hipEventDisableTiming));
            HIP_CHECK(hipEventCreateWithFlags(&s->copied[k], hipEventDisableTiming));
        }
        c->board_state = s.release();
    }
    return *reinterpret_cast<BoardState*>(c->board_state);
}

void board_free_all(Ctx* c)
{
    if (!c->board_state) return;
    BoardState* s = reinterpret_cast<BoardState*>(c->board_state);
    if (s->copy) { (void)hipStreamSynchronize(s->copy); (void)hipStreamDestroy(s->copy); }
    for (int k = 0; k < 2; ++k) {
        if (s->made[k]) (void)hipEventDestroy(s->made[k]);
        if (s->copied[k]) (void)hipEventDestroy(s->copied[k]);
    }
    delete s;
    c->board_state = nullptr;
}

// pictures of a round: as many as TB_ROUND_BYTES hold, or what PVF_THUMB_ROUND says, read when the call is made (tests lower it)
static int thumbs_per_round(size_t picture_bytes)
{
    int m = (int)std::max<size_t>(1, TB_ROUND_BYTES / picture_bytes);
    const char* e = getenv("PVF_THUMB_ROUND");
    if (e && atoi(e) > 0) m = atoi(e);
    return std::min(m, TB_ROUND_MAX);
}

static void check_tile(const std::string& w, int tw, int th)
{
    PVF_REQUIRE(tw >= 1 && tw <= PVF_THUMB_MAX_SIDE && th >= 1 && th <= PVF_THUMB_MAX_SIDE, w + ": tw or th outside 1 .. PVF_THUMB_MAX_SIDE");
}

static void thumbs_run(Ctx* c, const pvf_handle* frames, int n, int tw, int th, int flags, uint8_t* out, bool on_device)
{
    const std::string w("pvf_frame_thumbs");
    PVF_REQUIRE(n >= 0 && n <= PVF_THUMB_MAX_FRAMES, w + ": n outside 0 .. PVF_THUMB_MAX_FRAMES");
    if (n == 0) return;
    PVF_REQUIRE(frames && out, w + ": null frames or output");
    check_tile(w, tw, th);
    PVF_REQUIRE(flags == 0, w + ": unknown flags");
    BoardState& bs = bstate(c);
    // one staging block: the frames' addresses, then the column and the row table
    const size_t col_at = ((size_t)n * sizeof(uint8_t*) + 15) & ~(size_t)15, row_at = col_at + (size_t)tw * sizeof(ThumbCol);
    const size_t table_bytes = row_at + (size_t)th * sizeof(ThumbRow);
    uint8_t* staged = reinterpret_cast<uint8_t*>(c->stage.take(table_bytes));
    const uint8_t** table = reinterpret_cast<const uint8_t**>(staged);
    int h = 0, fw = 0;
    for (int i = 0; i < n; ++i) {
        const Frame f = c->frame(frames[i]);     // (orders the stream behind the frame's upload)
        PVF_REQUIRE(f.h >= 1 && f.w >= 1 && (int64_t)f.h * f.w * 3 <= INT32_MAX, w + ": a frame of 2 GiB or more");
        if (i == 0) { h = f.h; fw = f.w; }
        PVF_REQUIRE(f.h == h && f.w == fw, w + ": frames of different sizes");
        table[i] = f.d;
    }
    thumb_tables(h, fw, th, tw, reinterpret_cast<ThumbCol*>(staged + col_at), reinterpret_cast<ThumbRow*>(staged + row_at));
    const size_t pb = (size_t)th * tw * 3;
    const int round = thumbs_per_round(pb);
    ScratchLayout ol;
    const auto sOut = ol.take<uint8_t>((size_t)std::min(n, round) * pb);
    bs.table.ensure(table_bytes);
    uint8_t* d_table = bs.table.as<uint8_t>();
    HIP_CHECK(hipMemcpyAsync(d_table, staged, table_bytes, hipMemcpyHostToDevice, c->stream));
    c->stage.sent(c->stream);
    if (!on_device) { bs.out[0].ensure(ol.bytes()); if (n > round) bs.out[1].ensure(ol.bytes()); }
    // round k's kernel writes buffer k & 1 on the context's stream; its copy to the host runs on the copy stream behind the kernel's event,
    // while round k + 1's kernel, launched before the copy is asked for, runs; round k + 2's kernel waits for the copy's event
    int k = 0, prev_i0 = -1, prev_m = 0;
    auto copy_out = [&](int slot, int i0, int m) {
        HIP_CHECK(hipStreamWaitEvent(bs.copy, bs.made[slot], 0));
        HIP_CHECK(hipMemcpyAsync(out + (size_t)i0 * pb, sOut.in(bs.out[slot]), (size_t)m * pb, hipMemcpyDeviceToHost, bs.copy));
        HIP_CHECK(hipEventRecord(bs.copied[slot], bs.copy));
    };
    const unsigned segs = (unsigned)((tw + TB_SEG_PX - 1) / TB_SEG_PX);
    for (int i0 = 0; i0 < n; i0 += round, ++k) {
        const int m = std::min(round, n - i0), slot = k & 1;
        if (!on_device && k >= 2) HIP_CHECK(hipStreamWaitEvent(c->stream, bs.copied[slot], 0));
        {
            ProfScope prof(c, "thumbs");
            const ThumbArgs a{reinterpret_cast<const uint8_t* const*>(d_table) + i0, reinterpret_cast<const ThumbCol*>(d_table + col_at),
                              reinterpret_cast<const ThumbRow*>(d_table + row_at), h, fw, th, tw,
                              on_device ? out + (size_t)i0 * pb : sOut.in(bs.out[slot])};
            hipLaunchKernelGGL(frame_thumbs_k, dim3(segs, (unsigned)th, (unsigned)m), dim3(TB_LANES), 0, c->stream, a);
            HIP_CHECK(hipGetLastError());
        }
        if (on_device) continue;
        HIP_CHECK(hipEventRecord(bs.made[slot], c->stream));
        if (prev_i0 >= 0) copy_out(slot ^ 1, prev_i0, prev_m);
        prev_i0 = i0; prev_m = m;
    }
    if (!on_device) { copy_out((k - 1) & 1, prev_i0, prev_m); HIP_CHECK(hipStreamSynchronize(bs.copy)); }
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

// for blend.hip: the thumbnails of resident frames of one size into device memory, and the frames of a round at a picture size
void board_thumbs_device(Ctx* c, const pvf_handle* frames, int n, int tw, int th, uint8_t* d_out) { thumbs_run(c, frames, n, tw, th, 0, d_out, true); }
int board_thumbs_per_round(size_t picture_bytes) { return thumbs_per_round(picture_bytes); }

static void thumb_sheet_run(Ctx* c, const uint8_t* thumbs, int n, const int32_t* xy, int tw, int th, int W, int H, uint32_t background,
                            const pvf_prim* prims, int n_prims, const uint8_t* text, int64_t text_bytes, uint8_t* rgb)
{
    const std::string w("pvf_thumb_sheet");
    PVF_REQUIRE(n >= 0 && n <= PVF_SHEET_MAX_TILES, w + ": n outside 0 .. PVF_SHEET_MAX_TILES");
    PVF_REQUIRE(n == 0 || thumbs, w + ": null thumbnails");
    PVF_REQUIRE(n == 0 || xy, w + ": null tile corners");
    check_tile(w, tw, th);
    sheet_check(w, W, H, background, prims, n_prims, text, text_bytes, rgb);
    const size_t pb = (size_t)th * tw * 3;
    const int round = thumbs_per_round(pb);
    ScratchLayout tiles_lay, lay;
    const auto sTiles = tiles_lay.take<uint8_t>((size_t)std::min(n, round) * pb);
    const auto sRgb = lay.take<uint8_t>((size_t)W * H * 3);
    const auto sXy = lay.take<int32_t>((size_t)n * 2);
    const auto sPrims = lay.take<pvf_prim>((size_t)n_prims);     // 256-byte aligned: the kernel reads a primitive as two dwordx4
    const auto sText = lay.take<uint8_t>((size_t)text_bytes + 1);
    c->s_trk0.ensure(tiles_lay.bytes());
    c->s_act0.ensure(lay.bytes());
    if (n) HIP_CHECK(hipMemcpyAsync(sXy.in(c->s_act0), xy, sXy.bytes(), hipMemcpyHostToDevice, c->stream));
    if (n_prims) HIP_CHECK(hipMemcpyAsync(sPrims.in(c->s_act0), prims, sPrims.bytes(), hipMemcpyHostToDevice, c->stream));
    if (text_bytes) HIP_CHECK(hipMemcpyAsync(sText.in(c->s_act0), text, (size_t)text_bytes, hipMemcpyHostToDevice, c->stream));
    const dim3 grid((W + BS_TW - 1) / BS_TW, (H + BS_TH - 1) / BS_TH);
    // rounds in list order; a later round stores only where its own tiles are, so the last tile of the whole list wins
    for (int i0 = 0; i0 == 0 || i0 < n; i0 += round) {
        const int m = std::min(round, n - i0);
        if (m) HIP_CHECK(hipMemcpyAsync(sTiles.in(c->s_trk0), thumbs + (size_t)i0 * pb, (size_t)m * pb, hipMemcpyHostToDevice, c->stream));
        ThumbTileArgs a;
        a.thumbs = sTiles.in(c->s_trk0); a.xy = sXy.in(c->s_act0) + (size_t)i0 * 2;
        a.n = m; a.tw = tw; a.th = th; a.W = W; a.H = H; a.background = background; a.fill = i0 == 0; a.rgb = sRgb.in(c->s_act0);
        ProfScope prof(c, "sheet");
        hipLaunchKernelGGL(thumb_tiles_k, grid, dim3(256), 0, c->stream, a);
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

extern "C" int32_t pvf_frame_thumbs(pvf_handle h, const pvf_handle* frames, int32_t n, int32_t tw, int32_t th, int32_t flags, uint8_t* out,
                                    int32_t out_on_device)
{
    API_BEGIN
    ENTER(c, h);
    thumbs_run(c, frames, n, tw, th, flags, out, out_on_device != 0);
    API_END
}

extern "C" int32_t pvf_thumb_sheet(pvf_handle h, const uint8_t* thumbs, int32_t n, const int32_t* xy, int32_t tw, int32_t th, int32_t W, int32_t H,
                                   uint32_t background, const pvf_prim* prims, int32_t n_prims, const uint8_t* text, int64_t text_bytes, uint8_t* rgb)
{
    API_BEGIN
    ENTER(c, h);
    thumb_sheet_run(c, thumbs, n, xy, tw, th, W, H, background, prims, n_prims, text, text_bytes, rgb);
    API_END
}
