// blend.hip -- the `blend` verb's device side (BLEND.md): the blend record of every frame, from which `transition` finds fades and dissolves.
//   frame_thumbs_k   (board.hip, through board_thumbs_device) the tw x th thumbnail of every frame of a round, left in device memory.
//   blend_luma_k     the luma plane of a thumbnail and its sums S1 = sum Y, S2 = sum Y^2: a block per frame.
//   blend_measure_k  the sums of absolute differences of a plane against the planes 1, 4, 8, 16 and 32 frames before it, and of twice the
//                    middle plane against the two outer ones: a wave per (frame, lag), four pixels per 32-bit load.
// Everything is integer arithmetic (tests/blend_ref.py restates it; the kernels are held to it bit for bit).
#include "pvf_internal.h"
#include <algorithm>

constexpr int BL_WORDS = PVF_BLEND_ROW_WORDS;    // uint32 words of a row
constexpr int BL_HIST = PVF_BLEND_MAX_HISTORY;   // planes in front of a frame that a row can reach: the largest lag
constexpr int BL_TASKS = 5;                      // lag 1 (E1 alone), then 4, 8, 16, 32 (E and R)
constexpr uint32_t BL_ABSENT = 0xFFFFFFFFu;      // a sum whose earlier frame does not exist
static_assert(BL_WORDS == 16 && BL_HIST == 32, "the row of BLEND.md");

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// grid (m), 256 lanes.  thumbs [m][P][3] -> planes [m][P] with Y = (77 R + 150 G + 29 B + 128) >> 8, and words 0 .. 2 and 12 .. 15 of the
// frame's row: P, S1, S2, 0, 0, size, 0.  Pixel p of frame f is read at thumbs + 3 (f P + p) + {0, 1, 2} with p < P and written at
// planes + f P + p: nothing outside the two arrays.  S1 <= 255 P and S2 <= 65025 P fit 32 bits with P <= 16384; a lane's share too.
__global__ void __launch_bounds__(256) blend_luma_k(const uint8_t* __restrict__ thumbs, int P, uint32_t size_word, uint8_t* __restrict__ planes,
                                                    uint32_t* __restrict__ rows)
{
    __shared__ uint32_t s_part[2][4];
    const int tid = threadIdx.x, f = blockIdx.x;
    const uint8_t* __restrict__ src = thumbs + (size_t)f * P * 3;
    uint8_t* __restrict__ dst = planes + (size_t)f * P;
    uint32_t s1 = 0, s2 = 0;
    for (int p = tid; p < P; p += 256) {
        const uint32_t y = (77u * src[3 * p] + 150u * src[3 * p + 1] + 29u * src[3 * p + 2] + 128u) >> 8;
        dst[p] = (uint8_t)y;
        s1 += y; s2 += y * y;
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    if ((tid & 63) == 0) { s_part[0][tid >> 6] = s1; s_part[1][tid >> 6] = s2; }
    __syncthreads();
    if (tid == 0) {
        uint32_t* row = rows + (size_t)f * BL_WORDS;
        row[0] = (uint32_t)P;
        row[1] = s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3];
        row[2] = s_part[1][0] + s_part[1][1] + s_part[1][2] + s_part[1][3];
        row[12] = 0u; row[13] = 0u; row[14] = size_word; row[15] = 0u;
    }
}

// four bytes at any byte address: the planes are tight, so with P no multiple of 4 a plane starts between two dwords.  gfx950 under HSA
// runs with unaligned access on; the copy of four bytes is one global_load_dword.
__device__ __forceinline__ uint32_t load4(const uint8_t* p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// grid (BL_TASKS + sums, m), 64 lanes.  planes [first + m][P]: row i of the launch is plane g = first + i, its history the planes in front.
// Task 0 is lag 1 and writes E1 (word 3); task k = 1 .. 4 is lag L = 2 << k and writes E_L and R_L (words 2 + 2 k, 3 + 2 k), with
// a = g - L and mid = g - L / 2; both are BL_ABSENT when g < L.  Task 5 exists only with sums = 1 (pvf_blend_measure): it writes the words
// blend_luma_k writes otherwise, S1 and S2 from the plane and a size word of 0.  A lane takes the dwords lane, lane + 64, ... of the
// P / 4 whole dwords of each plane and lanes 0 .. 2 the P % 4 bytes behind them: every byte read lies in planes g, a or mid, below
// (first + m) P.  E through the byte SAD; R through the 16-bit SAD of 2 Y_mid against Y_a + Y_t, even and odd bytes apart (at most 510
// a half).  A lane's sums stay below 510 P <= 2^23; integer sums, so the order is free.
__global__ void __launch_bounds__(64) blend_measure_k(const uint8_t* __restrict__ planes, int P, int first, int sums, uint32_t* __restrict__ rows)
{
    const int lane = threadIdx.x, task = blockIdx.x, g = first + (int)blockIdx.y;
    uint32_t* row = rows + (size_t)blockIdx.y * BL_WORDS;
    const uint8_t* __restrict__ pt = planes + (size_t)g * P;
    const int nd = P >> 2;
    if (task == BL_TASKS) {
        if (!sums) return;
        uint32_t s1 = 0, s2 = 0;
        for (int d = lane; d < nd; d += 64) {
            const uint32_t v = load4(pt + 4 * d);
            const uint32_t b0 = v & 255u, b1 = (v >> 8) & 255u, b2 = (v >> 16) & 255u, b3 = v >> 24;
            s1 = __builtin_amdgcn_sad_u8(v, 0u, s1);
            s2 += b0 * b0 + b1 * b1 + b2 * b2 + b3 * b3;
        }
        if (4 * nd + lane < P) { const uint32_t y = pt[4 * nd + lane]; s1 += y; s2 += y * y; }
        s1 = wave_sum(s1); s2 = wave_sum(s2);
        if (lane == 0) { row[0] = (uint32_t)P; row[1] = s1; row[2] = s2; row[12] = 0u; row[13] = 0u; row[14] = 0u; row[15] = 0u; }
        return;
    }
    const int L = task == 0 ? 1 : 2 << task;
    uint32_t* out = task == 0 ? row + 3 : row + 2 + 2 * task;
    if (g < L) {                                 // (uniform over the block)
        if (lane == 0) { out[0] = BL_ABSENT; if (task) out[1] = BL_ABSENT; }
        return;
    }
    const uint8_t* __restrict__ pa = planes + (size_t)(g - L) * P;
    uint32_t E = 0, R = 0;
    if (task == 0) {
        for (int d = lane; d < nd; d += 64) E = __builtin_amdgcn_sad_u8(load4(pt + 4 * d), load4(pa + 4 * d), E);
        if (4 * nd + lane < P) { const int yt = pt[4 * nd + lane], ya = pa[4 * nd + lane]; E += (uint32_t)abs(yt - ya); }
        E = wave_sum(E);
        if (lane == 0) out[0] = E;
        return;
    }
    const uint8_t* __restrict__ pm = planes + (size_t)(g - L / 2) * P;
    const uint32_t even = 0x00FF00FFu;
    for (int d = lane; d < nd; d += 64) {
        const uint32_t vt = load4(pt + 4 * d), va = load4(pa + 4 * d), vm = load4(pm + 4 * d);
        E = __builtin_amdgcn_sad_u8(vt, va, E);
        R = __builtin_amdgcn_sad_u16((vm & even) << 1, (vt & even) + (va & even), R);
        R = __builtin_amdgcn_sad_u16(((vm >> 8) & even) << 1, ((vt >> 8) & even) + ((va >> 8) & even), R);
    }
    if (4 * nd + lane < P) {
        const int yt = pt[4 * nd + lane], ya = pa[4 * nd + lane], ym = pm[4 * nd + lane];
        E += (uint32_t)abs(yt - ya);
        R += (uint32_t)abs(2 * ym - ya - yt);
    }
    E = wave_sum(E); R = wave_sum(R);
    if (lane == 0) { out[0] = E; out[1] = R; }
}

static void check_plane(const std::string& w, int64_t P)
{
    PVF_REQUIRE(P >= 1 && P <= PVF_BLEND_MAX_PIXELS, w + ": a plane outside 1 .. PVF_BLEND_MAX_PIXELS pixels");
}

// the planes of a call live in two buffers that take turns: a round's buffer holds the up to BL_HIST planes in front of the round's first
// frame, then the round's own; the next round copies its history out of it into the other one.  pvf_blend_measure uploads
// every round's history with the round and needs one buffer.
struct BlendArena {
    ScratchSlot<uint8_t> thumbs, plane[2];
    ScratchSlot<uint32_t> rows;
    BlendArena(ScratchLayout& lay, size_t round, size_t P, bool from_frames)
    {
        thumbs = lay.take<uint8_t>(from_frames ? round * P * 3 : 0);
        for (int k = 0; k < (from_frames ? 2 : 1); ++k) plane[k] = lay.take<uint8_t>((BL_HIST + round) * P);
        rows = lay.take<uint32_t>(round * BL_WORDS);
    }
};

static void frame_blend_run(Ctx* c, const pvf_handle* frames, int n, int tw, int th, const uint8_t* hist, int nh, uint32_t* rows, uint8_t* luma_out)
{
    const std::string w("pvf_frame_blend");
    PVF_REQUIRE(n >= 0 && n <= PVF_THUMB_MAX_FRAMES, w + ": n outside 0 .. PVF_THUMB_MAX_FRAMES");
    if (n == 0) return;
    PVF_REQUIRE(nh >= 0 && nh <= BL_HIST, w + ": nh outside 0 .. PVF_BLEND_MAX_HISTORY");
    PVF_REQUIRE(tw >= 1 && tw <= PVF_THUMB_MAX_SIDE && th >= 1 && th <= PVF_THUMB_MAX_SIDE, w + ": tw or th outside 1 .. PVF_THUMB_MAX_SIDE");
    const int64_t P = (int64_t)tw * th;
    check_plane(w, P);
    PVF_REQUIRE(frames && rows, w + ": null frames or rows");
    PVF_REQUIRE(nh == 0 || hist, w + ": null history");
    int h = 0, fw = 0;
    for (int i = 0; i < n; ++i) {
        const Frame f = c->frame(frames[i]);
        PVF_REQUIRE(f.h >= 1 && f.w >= 1 && (int64_t)f.h * f.w * 3 <= INT32_MAX, w + ": a frame of 2 GiB or more");
        if (i == 0) { h = f.h; fw = f.w; }
        PVF_REQUIRE(f.h == h && f.w == fw, w + ": frames of different sizes");
    }
    const int round = std::min(n, board_thumbs_per_round((size_t)P * 3));
    ScratchLayout lay;
    const BlendArena ar(lay, (size_t)round, (size_t)P, true);
    c->s_act0.ensure(lay.bytes());
    const uint32_t size_word = (uint32_t)tw | (uint32_t)th << 16;
    int have = nh, k = 0;                        // planes of history in front of the round's first frame
    if (nh) HIP_CHECK(hipMemcpyAsync(ar.plane[0].in(c->s_act0), hist, (size_t)nh * P, hipMemcpyHostToDevice, c->stream));
    for (int i0 = 0; i0 < n; i0 += round, ++k) {
        const int m = std::min(round, n - i0);
        uint8_t* planes = ar.plane[k & 1].in(c->s_act0);
        board_thumbs_device(c, frames + i0, m, tw, th, ar.thumbs.in(c->s_act0));
        {
            ProfScope prof(c, "blend");
            hipLaunchKernelGGL(blend_luma_k, dim3((unsigned)m), dim3(256), 0, c->stream, ar.thumbs.in(c->s_act0), (int)P, size_word,
                               planes + (size_t)have * P, ar.rows.in(c->s_act0));
            hipLaunchKernelGGL(blend_measure_k, dim3(BL_TASKS, (unsigned)m), dim3(64), 0, c->stream, planes, (int)P, have, 0, ar.rows.in(c->s_act0));
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipMemcpyAsync(rows + (size_t)i0 * BL_WORDS, ar.rows.in(c->s_act0), (size_t)m * BL_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
        if (luma_out) HIP_CHECK(hipMemcpyAsync(luma_out + (size_t)i0 * P, planes + (size_t)have * P, (size_t)m * P, hipMemcpyDeviceToHost, c->stream));
        if (i0 + m < n) {                        // the next round's history: the last planes of this buffer, to the front of the other
            const int keep = std::min(BL_HIST, have + m);
            HIP_CHECK(hipMemcpyAsync(ar.plane[(k + 1) & 1].in(c->s_act0), planes + (size_t)(have + m - keep) * P, (size_t)keep * P,
                                     hipMemcpyDeviceToDevice, c->stream));
            have = keep;
        }
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

static void blend_measure_check(const uint8_t* luma, int N, int P, int first, const uint32_t* rows)
{
    const std::string w("pvf_blend_measure");
    PVF_REQUIRE(N >= 0 && N <= PVF_BLEND_MAX_ROWS, w + ": N outside 0 .. PVF_BLEND_MAX_ROWS");
    PVF_REQUIRE(first >= 0 && first <= N, w + ": first outside 0 .. N");
    check_plane(w, P);
    PVF_REQUIRE(N == 0 || luma, w + ": null planes");
    PVF_REQUIRE(first == N || rows, w + ": null rows");
}

static void blend_measure_run(Ctx* c, const uint8_t* luma, int N, int P, int first, uint32_t* rows)
{
    if (first == N) return;
    const int round = std::min(N - first, board_thumbs_per_round((size_t)P * 3));
    ScratchLayout lay;
    const BlendArena ar(lay, (size_t)round, (size_t)P, false);
    c->s_act0.ensure(lay.bytes());
    uint8_t* planes = ar.plane[0].in(c->s_act0);
    for (int r0 = first; r0 < N; r0 += round) {  // every round uploads its own history: nothing is carried
        const int m = std::min(round, N - r0), have = std::min(BL_HIST, r0);
        HIP_CHECK(hipMemcpyAsync(planes, luma + (size_t)(r0 - have) * P, (size_t)(have + m) * P, hipMemcpyHostToDevice, c->stream));
        {
            ProfScope prof(c, "blend");
            hipLaunchKernelGGL(blend_measure_k, dim3(BL_TASKS + 1, (unsigned)m), dim3(64), 0, c->stream, planes, P, have, 1, ar.rows.in(c->s_act0));
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipMemcpyAsync(rows + (size_t)(r0 - first) * BL_WORDS, ar.rows.in(c->s_act0), (size_t)m * BL_WORDS * 4, hipMemcpyDeviceToHost, c->stream));
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

extern "C" int32_t pvf_frame_blend(pvf_handle h, const pvf_handle* frames, int32_t n, int32_t tw, int32_t th, const uint8_t* hist, int32_t nh,
                                   uint32_t* rows, uint8_t* luma_out)
{
    API_BEGIN
    ENTER(c, h);
    frame_blend_run(c, frames, n, tw, th, hist, nh, rows, luma_out);
    API_END
}

extern "C" int32_t pvf_blend_measure(pvf_handle h, const uint8_t* luma, int32_t N, int32_t P, int32_t first, uint32_t* rows)
{
    API_BEGIN
    blend_measure_check(luma, N, P, first, rows);
    ENTER(c, h);
    blend_measure_run(c, luma, N, P, first, rows);
    API_END
}
