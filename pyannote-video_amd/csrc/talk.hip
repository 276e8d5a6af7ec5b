// talk.hip -- the `talk` verb's device side (TALK.md): how much the mouth of an aligned face chip moved since the face before it.
//   mouth_patch_k   a block per chip of the resident round: the luma of rows 49 .. 136, columns 39 .. 108 -- the mouth window and the
//                   control window above it, each with the +-3 margin of the search -- as two uint8 patches of 46 x 70 (pitch 72) in
//                   an arena that outlives the round; SM and NZ are reduced in the same pass.
//   patch_motion_k  a block per linked face, after the last round: the 2 x 49 displaced absolute differences between the face's two
//                   windows and its predecessor's two patches (v_sad_u8 on packed dwords, v_alignbyte_b32 for the byte shifts), their
//                   minima and the shift of the minimum.
// Two stages, so that nothing depends on where a round of 4096 chips ends.  Everything is integer arithmetic (tests/talk_ref.py
// restates it; the kernels are held to it bit for bit).
#include "pvf_internal.h"
#include <algorithm>

constexpr int T_SIDE = 150, T_ROWB = T_SIDE * 3, T_BYTES = T_SIDE * T_ROWB;
constexpr int T_ROW0 = 49, T_ROWS = 88;          // chip rows 49 .. 136: both windows with their margins
constexpr int T_COL0 = 39, T_COLS = 70;          // chip columns 39 .. 108
constexpr int T_MARGIN = 3, T_SHIFTS = 2 * T_MARGIN + 1, T_NSHIFT = T_SHIFTS * T_SHIFTS;        // 49 shifts, k = 24 the zero shift
constexpr int T_WIN_ROWS = 40, T_WIN_COLS = 64, T_WIN_COL0 = 42;
constexpr int T_MOUTH0 = 94, T_CTRL0 = 52;       // first rows of the two windows
constexpr int T_PROWS = T_WIN_ROWS + 2 * T_MARGIN, T_PITCH = 72, T_PDW = T_PITCH / 4;           // a patch: 46 rows of 18 dwords
constexpr int T_PATCH = T_PROWS * T_PITCH, T_FACE = 2 * T_PATCH;                                // 3312 and 6624 bytes: mouth, then control
constexpr int T_SPAN = 240, T_SPAN16 = T_SPAN / 16;      // bytes staged of a chip row: 210 wanted, at most 15 in front of them
constexpr int T_ROUND = 4096;                    // chips resident at a time, as pvf_chip_quality's rounds
static_assert(T_PATCH % 16 == 0 && ((T_MOUTH0 - T_MARGIN - T_ROW0) * T_PITCH) % 16 == 0, "a patch is whole 16-byte units of the luma block");
static_assert(T_CTRL0 - T_MARGIN == T_ROW0 && T_MOUTH0 + T_WIN_ROWS + T_MARGIN == T_ROW0 + T_ROWS, "the rows read are the two patches");
static_assert(T_WIN_COL0 - T_MARGIN == T_COL0 && T_WIN_COLS + 2 * T_MARGIN == T_COLS && 15 + 3 * T_COLS <= T_SPAN, "the columns read");
static_assert((size_t)PVF_MOTION_MAX_FACES * T_FACE < ((size_t)1 << 31), "the patch arena");

// grid (m chips of the round), 256 lanes.  chips: [m][150][150][3], any alignment.  patches: [m][2][46][72], 16-byte aligned.
// out: [m][8]; the six motion values are set to -1 here, patch_motion_k overwrites them for linked faces.
// Of chip row 49 + r only bytes 117 .. 326 (columns 39 .. 108) are wanted: the 15 aligned 16-byte loads from the boundary at or below
// byte 117 cover them whatever the row's alignment is, and lie inside the chip (the first starts at least 22 152 bytes in, the last
// ends at most 61 557 bytes in), so the head and tail that are not wanted are simply not looked at.
__global__ void __launch_bounds__(256) mouth_patch_k(const uint8_t* __restrict__ chips, uint8_t* __restrict__ patches, int32_t* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_raw[T_ROWS * T_SPAN / 4];
    __shared__ __attribute__((aligned(16))) uint32_t s_y[T_ROWS * T_PDW];
    __shared__ uint32_t s_red[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* __restrict__ chip = chips + (size_t)blockIdx.x * T_BYTES;
    for (int u = tid; u < T_ROWS * T_SPAN16; u += 256) {
        const int r = u / T_SPAN16, j = u - r * T_SPAN16;
        const uint8_t* p = chip + (T_ROW0 + r) * T_ROWB + T_COL0 * 3;
        const uint4* a = reinterpret_cast<const uint4*>(p - (reinterpret_cast<uintptr_t>(p) & 15));
        reinterpret_cast<uint4*>(s_raw)[u] = a[j];
    }
    __syncthreads();
    uint32_t sm = 0, nz = 0;
    for (int u = tid; u < T_ROWS * T_PDW; u += 256) {             // four pixels a lane: one dword of the luma block
        const int r = u / T_PDW, q = u - r * T_PDW, row = T_ROW0 + r;
        const int head = (int)(reinterpret_cast<uintptr_t>(chip + row * T_ROWB + T_COL0 * 3) & 15);
        // the unit's 12 bytes start at LDS byte r * 240 + head + 12 q: four aligned dwords (all inside the 21 120 bytes
        // staged), funnelled down by the start's offset in its dword
        const int at = r * T_SPAN + head + 12 * q;
        const uint32_t* sw = s_raw + (at >> 2);
        const uint32_t w0 = sw[0], w1 = sw[1], w2 = sw[2], w3 = sw[3], sh = (uint32_t)(at & 3);
        const uint32_t x[3] = {__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh), __builtin_amdgcn_alignbyte(w3, w2, sh)};
        const bool mouth = row >= T_MOUTH0 && row < T_MOUTH0 + T_WIN_ROWS, ctrl = row >= T_CTRL0 && row < T_CTRL0 + T_WIN_ROWS;
        uint32_t y4 = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int cc = 4 * q + e;                             // column 39 + cc; 70 and 71 are the pitch's padding, stored as 0
            if (cc >= T_COLS) continue;
            const uint32_t rr = (x[(3 * e) >> 2] >> (8 * ((3 * e) & 3))) & 255u, gg = (x[(3 * e + 1) >> 2] >> (8 * ((3 * e + 1) & 3))) & 255u;
            const uint32_t bb = (x[(3 * e + 2) >> 2] >> (8 * ((3 * e + 2) & 3))) & 255u;
            const uint32_t y = (77u * rr + 150u * gg + 29u * bb + 128u) >> 8;
            y4 |= y << (8 * e);
            if (cc < T_MARGIN || cc >= T_MARGIN + T_WIN_COLS) continue;
            if (mouth) sm += y;
            if (mouth || ctrl) nz += y <= 16u;
        }
        s_y[u] = y4;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { sm += __shfl_xor(sm, d); nz += __shfl_xor(nz, d); }
    if (lane == 0) { s_red[wave][0] = sm; s_red[wave][1] = nz; }
    __syncthreads();
    // the mouth patch is rows 42 .. 87 of the luma block, the control patch rows 0 .. 45: 207 aligned 16-byte units each
    uint4* dst = reinterpret_cast<uint4*>(patches + (size_t)blockIdx.x * T_FACE);
    const uint4* s_y4 = reinterpret_cast<const uint4*>(s_y);
    constexpr int PU = T_PATCH / 16, MOUTH_U = (T_MOUTH0 - T_MARGIN - T_ROW0) * T_PITCH / 16;
    for (int u = tid; u < 2 * PU; u += 256) dst[u] = s_y4[u < PU ? MOUTH_U + u : u - PU];
    if (tid == 0) {
        int4* o = reinterpret_cast<int4*>(out + (size_t)blockIdx.x * 8);
        o[0] = make_int4(-1, -1, -1, -1);
        o[1] = make_int4(-1, -1, (int)(s_red[0][0] + s_red[1][0] + s_red[2][0] + s_red[3][0]), (int)(s_red[0][1] + s_red[1][1] + s_red[2][1] + s_red[3][1]));
    }
}

// One step of a wave's sum of 64 values per lane in 63 exchanges instead of 64 x 6: of 2H values a lane keeps the half its bit H names,
// sends the other half to lane ^ H and adds what comes back.  After the steps H = 32 .. 1, v[0] of lane l is the sum over the wave of
// what was v[l].
template <int H>
__device__ __forceinline__ void fold_half(uint32_t (&v)[64], int lane)
{
    const bool up = lane & H;
#pragma unroll
    for (int j = 0; j < H; ++j) {
        const uint32_t keep = up ? v[j + H] : v[j], send = up ? v[j] : v[j + H];
        v[j] = keep + __shfl_xor(send, H);
    }
}

// grid (linked faces), 256 lanes.  patches: the arena of the whole call; links: (face, predecessor), both inside it (the host checked).
// Lanes 0 .. 127 take the mouth window, 128 .. 255 the control window: 640 dwords of four window pixels, five a lane, kept in registers
// (a window dword is read by one lane only).  The predecessor's two patches are staged in LDS (6624 bytes).  For a window dword at
// row r, dword q and a row shift dy the predecessor's bytes for the seven dx are bytes 4q .. 4q + 9 of patch row r + 3 + dy: three
// LDS dwords, four v_alignbyte_b32, seven v_sad_u8.  A lane's 49 sums stay below 5 * 4 * 255; integer sums, so the reduction's
// shape is free: a halving butterfly inside the wave (fold_half), the two waves of a window added by the lane that picks the minimum.
__global__ void __launch_bounds__(256) patch_motion_k(const uint8_t* __restrict__ patches, const int2* __restrict__ links, int32_t* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_prev[T_FACE / 4];
    __shared__ uint32_t s_part[4][T_NSHIFT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, win = tid >> 7, g = tid & 127;
    const int2 link = links[blockIdx.x];
    const uint4* prev = reinterpret_cast<const uint4*>(patches + (size_t)link.y * T_FACE);
    for (int u = tid; u < T_FACE / 16; u += 256) reinterpret_cast<uint4*>(s_prev)[u] = prev[u];
    const uint32_t* cur = reinterpret_cast<const uint32_t*>(patches + (size_t)link.x * T_FACE + (size_t)win * T_PATCH);
    constexpr int UNITS = T_WIN_ROWS * T_WIN_COLS / 4 / 128;      // 5
    uint32_t cw[UNITS];
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
        const int u = g + 128 * k, r = u >> 4, q = u & 15;
        const uint32_t* s = cur + (r + T_MARGIN) * T_PDW + q;     // window column 4q is patch byte 4q + 3
        cw[k] = __builtin_amdgcn_alignbyte(s[1], s[0], 3);
    }
    __syncthreads();
    uint32_t acc[T_NSHIFT];
#pragma unroll
    for (int j = 0; j < T_NSHIFT; ++j) acc[j] = 0;
    const uint32_t* pw = s_prev + win * (T_PATCH / 4);
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
        const int u = g + 128 * k, r = u >> 4, q = u & 15;
#pragma unroll
        for (int dy = 0; dy < T_SHIFTS; ++dy) {                   // the shift is dy - 3: patch row r + 3 + (dy - 3)
            const uint32_t* s = pw + (r + dy) * T_PDW + q;        // at most dword 45 * 18 + 15 + 2 = 827, the patch's last
            const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
            uint32_t* a = acc + dy * T_SHIFTS;
            a[0] = __builtin_amdgcn_sad_u8(cw[k], w0, a[0]);
            a[1] = __builtin_amdgcn_sad_u8(cw[k], __builtin_amdgcn_alignbyte(w1, w0, 1), a[1]);
            a[2] = __builtin_amdgcn_sad_u8(cw[k], __builtin_amdgcn_alignbyte(w1, w0, 2), a[2]);
            a[3] = __builtin_amdgcn_sad_u8(cw[k], __builtin_amdgcn_alignbyte(w1, w0, 3), a[3]);
            a[4] = __builtin_amdgcn_sad_u8(cw[k], w1, a[4]);
            a[5] = __builtin_amdgcn_sad_u8(cw[k], __builtin_amdgcn_alignbyte(w2, w1, 1), a[5]);
            a[6] = __builtin_amdgcn_sad_u8(cw[k], __builtin_amdgcn_alignbyte(w2, w1, 2), a[6]);
        }
    }
    uint32_t v[64];                                               // 49 sums and 15 zeros: lane l ends with the wave's sum number l
#pragma unroll
    for (int j = 0; j < 64; ++j) v[j] = j < T_NSHIFT ? acc[j] : 0u;
    fold_half<32>(v, lane); fold_half<16>(v, lane); fold_half<8>(v, lane); fold_half<4>(v, lane); fold_half<2>(v, lane); fold_half<1>(v, lane);
    if (lane < T_NSHIFT) s_part[wave][lane] = v[0];
    __syncthreads();
    if (tid < 2) {                                                // lane 0 the mouth (waves 0, 1), lane 1 the control window (waves 2, 3)
        const uint32_t d0 = s_part[2 * tid][T_NSHIFT / 2] + s_part[2 * tid + 1][T_NSHIFT / 2];
        uint32_t dmin = 0xffffffffu;
        int kmin = 0;
        for (int j = 0; j < T_NSHIFT; ++j) {
            const uint32_t d = s_part[2 * tid][j] + s_part[2 * tid + 1][j];
            if (d < dmin) { dmin = d; kmin = j; }                 // the first minimum in row-major order
        }
        int32_t* o = out + (size_t)link.x * 8 + 3 * tid;
        o[0] = (int32_t)d0; o[1] = (int32_t)dmin; o[2] = d0 == dmin ? T_NSHIFT / 2 : kmin;
    }
}

// chips (host, or frames + landmarks) -> eight int32 per face.  s_trk0 holds the chips of a round, s_act0 the patches of the whole
// call, the list of linked faces and the outputs.
static void motion_run(Ctx* c, const ChipSource& src, int n, const int32_t* prev, int32_t* out, const char* who)
{
    const std::string w(who);
    PVF_REQUIRE(n >= 0 && n <= PVF_MOTION_MAX_FACES, w + ": n outside 0 .. PVF_MOTION_MAX_FACES");
    if (n == 0) return;
    PVF_REQUIRE(src.host || (src.frames && src.pts), w + ": null chips, frames or landmarks");
    PVF_REQUIRE(prev, w + ": null predecessor list");
    PVF_REQUIRE(out, w + ": null output");
    std::vector<int2> links;
    for (int i = 0; i < n; ++i) {                // nothing the kernel indexes with is taken on trust
        PVF_REQUIRE(prev[i] >= -1, w + ": a predecessor below -1");
        PVF_REQUIRE(prev[i] < i, w + ": a predecessor is an earlier face of the same call (prev[i] < i)");
        if (prev[i] >= 0) links.push_back(make_int2(i, prev[i]));
    }
    ScratchLayout chips_lay, lay;
    const auto sChips = chips_lay.take<uint8_t>((size_t)std::min(n, T_ROUND) * T_BYTES);
    const auto sPatch = lay.take<uint8_t>((size_t)n * T_FACE);
    const auto sLinks = lay.take<int2>(links.size());
    const auto sOut = lay.take<int32_t>((size_t)n * 8);
    c->s_trk0.ensure(chips_lay.bytes());
    c->s_act0.ensure(lay.bytes());
    if (!links.empty()) HIP_CHECK(hipMemcpyAsync(sLinks.in(c->s_act0), links.data(), sLinks.bytes(), hipMemcpyHostToDevice, c->stream));
    for (int i0 = 0; i0 < n; i0 += T_ROUND) {
        const int m = std::min(T_ROUND, n - i0);
        faces_source_round(c, src, i0, m, sChips.in(c->s_trk0));
        ProfScope prof(c, "talk");
        hipLaunchKernelGGL(mouth_patch_k, dim3((unsigned)m), dim3(256), 0, c->stream, sChips.in(c->s_trk0), sPatch.in(c->s_act0) + (size_t)i0 * T_FACE,
                           sOut.in(c->s_act0) + (size_t)i0 * 8);
        HIP_CHECK(hipGetLastError());
    }
    if (!links.empty()) {
        ProfScope prof(c, "talk");
        hipLaunchKernelGGL(patch_motion_k, dim3((unsigned)links.size()), dim3(256), 0, c->stream, sPatch.in(c->s_act0), sLinks.in(c->s_act0),
                           sOut.in(c->s_act0));
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipMemcpyAsync(out, sOut.in(c->s_act0), sOut.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));         // (links lives until here: its copy has been read)
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

extern "C" int32_t pvf_chip_motion(pvf_handle h, const uint8_t* chips, int32_t n, const int32_t* prev, int32_t* out)
{
    API_BEGIN
    ENTER(c, h);
    motion_run(c, ChipSource{chips, nullptr, nullptr}, n, prev, out, "pvf_chip_motion");
    API_END
}

extern "C" int32_t pvf_face_motion(pvf_handle h, const pvf_handle* frames, const int32_t* pts, int32_t n, const int32_t* prev, int32_t* out)
{
    API_BEGIN
    ENTER(c, h);
    motion_run(c, ChipSource{nullptr, frames, pts}, n, prev, out, "pvf_face_motion");
    API_END
}
