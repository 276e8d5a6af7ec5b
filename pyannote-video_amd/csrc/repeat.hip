// repeat.hip -- the `fingerprint` and `repeat` verbs' device side (REPEAT.md): a 128-bit print of every frame, and the runs of matching
// prints along the diagonals of two films (or of one film against itself).
//   frame_print_k   the weighted sums of the 9 x 9 area-average grid of a resident frame of any size: a block per (row chunk, grid row,
//                   frame), a lane per byte column, the frame read once, 64-bit sums per block left for
//   print_finish_k  which adds a frame's partial sums, divides (rounded half up), takes the luma and writes H, V, SY | RANGE << 32.
//   print_runs_k    a block per (256 diagonals, strip of PVF_RUNS_STRIP rows of A): B's prints of the tile in LDS, A's print of the row
//                   through the scalar cache, a lane walks its diagonal and reports the runs that start in its strip.
// Everything is integer arithmetic (tests/repeat_ref.py restates it; the kernels are held to it bit for bit).
#include "pvf_internal.h"
#include <algorithm>

// ---- prints --------------------------------------------------------------------------------------------------------------------------
constexpr int PP_G = 9;                          // the grid is 9 x 9
constexpr int PP_CHUNKS = 8;                     // blocks that share the source rows of one grid row
constexpr int PP_SLOTS = 16;                     // copies of a block's 27 sums in LDS: lanes of a wave spread over them
constexpr int PP_ROUND = 1024;                   // frames of a launch

struct PrintFrame { const uint8_t* d; int32_t h, w; };

// grid (PP_CHUNKS, 9, m), 256 lanes.  STORYBOARD.md's thumbnail with tw = th = 9, before the division: in units of 1/9 source pixel source
// column j is [9 j, 9 j + 9) and grid column X is [X w, (X + 1) w); rows alike with h.  Grid row Y takes the source rows
// [Y h / 9, ceil((Y + 1) h / 9)), cut into PP_CHUNKS runs of rows, one a block (a block without rows writes zeros).  A lane owns byte
// column b = 3 j + c of the row, b = tid, tid + 256, ...: it adds wy(Y, i) byte(i, b) over the block's rows (32-bit: at most 255 x 9 x h),
// then gives wx(X, j) times that to every grid column X its source column meets (two at most when w >= 9, up to nine below), as a 64-bit
// LDS add.  Every address is row i < h, byte b < 3 w of the frame.  Integer sums: the order is free.
__global__ void __launch_bounds__(256) frame_print_k(const PrintFrame* __restrict__ frames, unsigned long long* __restrict__ partial)
{
    __shared__ unsigned long long s_acc[PP_SLOTS][PP_G * 3];
    const int tid = threadIdx.x, Y = blockIdx.y, f = blockIdx.z;
    const PrintFrame fr = frames[f];
    const int h = fr.h, w = fr.w;
    const uint8_t* __restrict__ img = fr.d;
    for (int k = tid; k < PP_SLOTS * PP_G * 3; k += 256) (&s_acc[0][0])[k] = 0ull;
    __syncthreads();
    const int64_t ya = (int64_t)Y * h, yb = ya + h;              // grid row Y in units of 1/9 source row
    const int i0 = (int)(ya / PP_G), i1 = (int)((yb + PP_G - 1) / PP_G);
    const int per = (i1 - i0 + PP_CHUNKS - 1) / PP_CHUNKS;
    const int ra = i0 + (int)blockIdx.x * per, rb = min(ra + per, i1);
    const int rowb = 3 * w;
    auto wy = [&](int i) { return (uint32_t)(min((int64_t)(i + 1) * PP_G, yb) - max((int64_t)i * PP_G, ya)); };
    if (ra < rb)
        for (int b = tid; b < rowb; b += 256) {
            const uint8_t* p = img + (size_t)ra * rowb + b;
            uint32_t s = 0;
            int i = ra;
            for (; i + 4 <= rb; i += 4, p += (size_t)4 * rowb) {          // four loads in flight
                const uint32_t v0 = p[0], v1 = p[rowb], v2 = p[(size_t)2 * rowb], v3 = p[(size_t)3 * rowb];
                s += wy(i) * v0 + wy(i + 1) * v1 + wy(i + 2) * v2 + wy(i + 3) * v3;
            }
            for (; i < rb; ++i, p += rowb) s += wy(i) * (uint32_t)p[0];
            const int j = b / 3, c = b - 3 * j;
            const int64_t u0 = (int64_t)j * PP_G, u1 = u0 + PP_G;
            int Xa, Xb;                                                 // < 9: u1 - 1 < 9 w
            if (w < (1 << 27)) { Xa = (int)((uint32_t)u0 / (uint32_t)w); Xb = (int)((uint32_t)(u1 - 1) / (uint32_t)w); }      // (32-bit division)
            else { Xa = (int)(u0 / w); Xb = (int)((u1 - 1) / w); }
            for (int X = Xa; X <= Xb; ++X) {
                const uint32_t wx = (uint32_t)(min(u1, (int64_t)(X + 1) * w) - max(u0, (int64_t)X * w));
                atomicAdd(&s_acc[tid & (PP_SLOTS - 1)][X * 3 + c], (unsigned long long)wx * s);
            }
        }
    __syncthreads();
    if (tid < PP_G * 3) {
        unsigned long long t = 0;
#pragma unroll
        for (int k = 0; k < PP_SLOTS; ++k) t += s_acc[k][tid];
        partial[(((size_t)f * PP_G + Y) * PP_CHUNKS + blockIdx.x) * (PP_G * 3) + tid] = t;
    }
}

// grid (m), 128 lanes.  Lane t < 81 is grid cell (t / 9, t % 9): the sums of the chunks, (sum + w h / 2) / (w h) per channel (below 256),
// the luma (77 R + 150 G + 29 B + 128) >> 8.  Lane t < 64 then holds bit t = 8 r + c of H and of V; lane 0 adds SY and takes the range.
__global__ void __launch_bounds__(128) print_finish_k(const PrintFrame* __restrict__ frames, const unsigned long long* __restrict__ partial,
                                                      unsigned long long* __restrict__ out)
{
    __shared__ uint32_t s_y[PP_G * PP_G];
    const int t = threadIdx.x, f = blockIdx.x;
    const PrintFrame fr = frames[f];
    const unsigned long long den = (unsigned long long)fr.h * (unsigned long long)fr.w;
    if (t < PP_G * PP_G) {
        const int Y = t / PP_G, X = t - PP_G * Y;
        uint32_t px[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            unsigned long long s = 0;
            for (int k = 0; k < PP_CHUNKS; ++k) s += partial[(((size_t)f * PP_G + Y) * PP_CHUNKS + k) * (PP_G * 3) + X * 3 + c];
            px[c] = (uint32_t)((s + den / 2) / den);
        }
        s_y[t] = (77u * px[0] + 150u * px[1] + 29u * px[2] + 128u) >> 8;
    }
    __syncthreads();
    if (t >= 64) return;                         // wave 0, all of its lanes
    const int r = t >> 3, c = t & 7;
    const uint32_t y = s_y[PP_G * r + c];
    const unsigned long long H = __ballot(y < s_y[PP_G * r + c + 1]), V = __ballot(y < s_y[PP_G * (r + 1) + c]);
    if (t == 0) {
        uint32_t sy = 0, lo = 255u, hi = 0u;
        for (int k = 0; k < PP_G * PP_G; ++k) { const uint32_t v = s_y[k]; sy += v; lo = min(lo, v); hi = max(hi, v); }
        unsigned long long* o = out + (size_t)f * 4;
        o[0] = H; o[1] = V; o[2] = (unsigned long long)sy | (unsigned long long)(hi - lo) << 32; o[3] = 0ull;
    }
}

static void prints_run(Ctx* c, const pvf_handle* frames, int n, uint64_t* out, bool on_device)
{
    const std::string w("pvf_frame_prints");
    PVF_REQUIRE(n >= 0 && n <= PVF_PRINT_MAX_ROWS, w + ": n outside 0 .. PVF_PRINT_MAX_ROWS");
    if (n == 0) return;
    PVF_REQUIRE(frames && out, w + ": null frames or output");
    std::vector<PrintFrame> table((size_t)n);
    for (int i = 0; i < n; ++i) {
        const Frame f = c->frame(frames[i]);     // (orders the stream behind the frame's upload)
        PVF_REQUIRE(f.h >= 1 && f.w >= 1 && (int64_t)f.h * f.w * 3 <= INT32_MAX, w + ": a frame of 2 GiB or more");
        table[(size_t)i] = PrintFrame{f.d, f.h, f.w};
    }
    const int round = std::min(n, PP_ROUND);
    ScratchLayout lay;
    const auto sTab = lay.take<PrintFrame>((size_t)round);
    const auto sPart = lay.take<unsigned long long>((size_t)round * PP_G * PP_CHUNKS * PP_G * 3);
    const auto sOut = lay.take<unsigned long long>((size_t)round * 4);
    c->s_act0.ensure(lay.bytes());
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "a print is copied as it lies");
    for (int i0 = 0; i0 < n; i0 += round) {
        const int m = std::min(round, n - i0);
        PrintFrame* staged = reinterpret_cast<PrintFrame*>(c->stage.take((size_t)m * sizeof(PrintFrame)));
        std::copy(table.begin() + i0, table.begin() + i0 + m, staged);
        HIP_CHECK(hipMemcpyAsync(sTab.in(c->s_act0), staged, (size_t)m * sizeof(PrintFrame), hipMemcpyHostToDevice, c->stream));
        c->stage.sent(c->stream);
        unsigned long long* d_out = on_device ? reinterpret_cast<unsigned long long*>(out) + (size_t)i0 * 4 : sOut.in(c->s_act0);
        {
            ProfScope prof(c, "prints");
            hipLaunchKernelGGL(frame_print_k, dim3(PP_CHUNKS, PP_G, (unsigned)m), dim3(256), 0, c->stream, sTab.in(c->s_act0), sPart.in(c->s_act0));
            hipLaunchKernelGGL(print_finish_k, dim3((unsigned)m), dim3(128), 0, c->stream, sTab.in(c->s_act0), sPart.in(c->s_act0), d_out);
            HIP_CHECK(hipGetLastError());
        }
        if (!on_device) HIP_CHECK(hipMemcpyAsync(out + (size_t)i0 * 4, d_out, (size_t)m * 32, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

// ---- runs ----------------------------------------------------------------------------------------------------------------------------
constexpr int PR_S = PVF_RUNS_STRIP;             // rows of A a block walks
constexpr int PR_D = 256;                        // diagonals of a block: a lane each
constexpr int PR_E = PR_S + PR_D;                // B's entries of a tile: j = j0 .. j0 + PR_E - 1, the row before the strip included
constexpr uint32_t PR_NEVER = 255u;              // the penalty of an unusable or absent print: above every tau

struct RunsArgs {
    const uint4* A; const uint32_t* pa;          // [NA] prints (H lo, H hi, V lo, V hi) and penalties (0 usable, PR_NEVER not)
    const uint4* B; const uint32_t* pb;          // [NB]; A's own in self mode
    int NA, NB;
    int d0, ndiag;                               // diagonals d = j - i of the call: d0 .. d0 + ndiag - 1
    uint32_t tau; int min_len;
    int32_t* runs; unsigned long long cap;       // [cap][3]
    unsigned long long* count;
};

// popcount(x) + acc in one instruction: the count's add operand (the compiler adds apart)
__device__ __forceinline__ uint32_t popc_add(uint32_t x, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
    return r;
#else
    return (uint32_t)__builtin_popcount(x) + acc;
#endif
}

__device__ __forceinline__ uint32_t print_dist(const uint4 a, const uint4 b, uint32_t acc)
{
    return popc_add(a.x ^ b.x, popc_add(a.y ^ b.y, popc_add(a.z ^ b.z, popc_add(a.w ^ b.w, acc))));
}

// grid (ceil(ndiag / 256), ceil(NA / PR_S)), 256 lanes.  Lane tid walks diagonal d = d0 + 256 bx + tid over the rows i of the strip
// [s0, s0 + nrows), cell (i, i + d).  Entry e of the tile is B's print j = j0 + e with j0 = s0 - 1 + d0 + 256 bx, so the cell of row i
// is entry i - s0 + 1 + tid and the cell before the strip entry tid.  An entry outside [0, NB) is staged with the penalty PR_NEVER, which
// also ends every diagonal at the array's ends and silences the lanes past the last diagonal (their j is never below NB); nothing is
// read outside A[0, NA) and B[0, NB).  A's row is the same for every lane: it comes from the constant address space, as scalar loads.
// A lane reports the runs that START in its strip: it knows from the cell before the strip whether its first cell starts one, and it
// follows a run that is still open at the strip's end through global memory to the run's end (bounded by NA and NB).  A run that
// came in from the strip before is that strip's.  A reported run takes a slot from one counter; beyond cap it is counted, not written.
__global__ void __launch_bounds__(PR_D) print_runs_k(const RunsArgs a)
{
    __shared__ uint4 s_b[PR_E];
    __shared__ uint32_t s_pen[PR_E];
    const int tid = threadIdx.x;
    const int s0 = (int)blockIdx.y * PR_S, nrows = min(PR_S, a.NA - s0);
    const int dblock = a.d0 + (int)blockIdx.x * PR_D, j0 = s0 - 1 + dblock;
    if (j0 + nrows + PR_D - 1 < 0 || j0 + 1 >= a.NB) return;   // no cell of the tile's strip lies in B (entry 0 is the row before the strip)
    for (int e = tid; e < nrows + PR_D; e += PR_D) {
        const int j = j0 + e;
        const bool in = j >= 0 && j < a.NB;
        s_b[e] = in ? a.B[j] : make_uint4(0u, 0u, 0u, 0u);
        s_pen[e] = in ? a.pb[j] : PR_NEVER;
    }
    __syncthreads();
    const __attribute__((address_space(4))) uint32_t* cW = (const __attribute__((address_space(4))) uint32_t*)a.A;
    auto row_of_a = [&](int i) { return make_uint4(cW[4 * (size_t)i], cW[4 * (size_t)i + 1], cW[4 * (size_t)i + 2], cW[4 * (size_t)i + 3]); };
    const __attribute__((address_space(4))) uint32_t* cP = (const __attribute__((address_space(4))) uint32_t*)a.pa;
    const int d = dblock + tid;
    const uint32_t tau = a.tau;
    auto emit = [&](int start, int len) {
        const unsigned long long slot = atomicAdd(a.count, 1ull);
        if (slot < a.cap) { int32_t* o = a.runs + slot * 3; o[0] = start; o[1] = start + d; o[2] = len; }
    };
    // len: the matching cells that end at the row above; a run that came in from the strip before counts from far below zero, so it
    // never reaches min_len >= 1 here (NA <= 2^24 rows cannot lift it)
    int len = 0;
    if (s0 > 0 && cP[s0 - 1] == 0u) { const uint4 av = row_of_a(s0 - 1); if (print_dist(av, s_b[tid], s_pen[tid]) <= tau) len = -(1 << 30); }
    auto step = [&](int i, bool m) {
        if (!m && len >= a.min_len) emit(i - len, len);
        len = m ? len + 1 : 0;
    };
    int r = 0;
    for (; r + 4 <= nrows; r += 4) {             // the loads of four rows first, so that one wait covers them
        uint32_t pen[4];
        uint4 av[4], bv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { pen[k] = cP[s0 + r + k] | s_pen[r + k + 1 + tid]; av[k] = row_of_a(s0 + r + k); bv[k] = s_b[r + k + 1 + tid]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) step(s0 + r + k, print_dist(av[k], bv[k], pen[k]) <= tau);
    }
    for (; r < nrows; ++r) step(s0 + r, print_dist(row_of_a(s0 + r), s_b[r + 1 + tid], cP[s0 + r] | s_pen[r + 1 + tid]) <= tau);
    if (len <= 0) return;
    const int start = s0 + nrows - len;
    int i = s0 + nrows, j = i + d;               // the open run goes on below the strip (j >= 0: the run has cells above)
    while (i < a.NA && j < a.NB && a.pa[i] == 0u && print_dist(a.A[i], a.B[j], a.pb[j]) <= tau) { ++i; ++j; }
    if (i - start >= a.min_len) emit(start, i - start);
}

static void runs_check(const uint64_t* A, const uint8_t* ua, int NA, const uint64_t* B, const uint8_t* ub, int NB, int tau, int min_len,
                       int min_gap, const int32_t* runs, int64_t cap, const int64_t* found)
{
    const std::string w("pvf_print_runs");
    PVF_REQUIRE(NA >= 0 && NA <= PVF_PRINT_MAX_ROWS && (!B || (NB >= 0 && NB <= PVF_PRINT_MAX_ROWS)), w + ": NA or NB outside 0 .. PVF_PRINT_MAX_ROWS");
    PVF_REQUIRE(tau >= 0 && tau <= 128, w + ": tau outside 0 .. 128");
    PVF_REQUIRE(min_len >= 1, w + ": min_len below 1");
    PVF_REQUIRE(B || min_gap >= 1, w + ": self mode (B == NULL) needs min_gap >= 1");
    PVF_REQUIRE(cap >= 0, w + ": cap below 0");
    PVF_REQUIRE(found, w + ": null found");
    PVF_REQUIRE(NA == 0 || (A && ua), w + ": null A or usable_a");
    PVF_REQUIRE(!B || NB == 0 || ub, w + ": null usable_b");
    PVF_REQUIRE(cap == 0 || runs, w + ": null runs");
}

static void runs_dev(Ctx* c, const uint64_t* A, const uint8_t* ua, int NA, const uint64_t* B, const uint8_t* ub, int NB, int tau, int min_len,
                     int min_gap, int32_t* runs, int64_t cap, int64_t* found)
{
    const bool self = B == nullptr;
    if (self) NB = NA;
    *found = 0;
    if (NA == 0 || NB == 0) return;
    const int64_t d0 = self ? (int64_t)min_gap : -(int64_t)(NA - 1), d1 = NB - 1;      // diagonals d0 .. d1
    if (d0 > d1) return;
    const int64_t ndiag = d1 - d0 + 1;
    // a diagonal of L cells holds at most (L + 1) / (min_len + 1) runs; NA NB bounds every sum of them
    const int64_t dev_cap = std::min<int64_t>(cap, (int64_t)NA * NB);
    ScratchLayout lay, layR;
    const auto sA = lay.take<uint4>((size_t)NA), sB = lay.take<uint4>(self ? 0 : (size_t)NB);
    const auto sPa = lay.take<uint32_t>((size_t)NA), sPb = lay.take<uint32_t>(self ? 0 : (size_t)NB);
    const auto sCount = lay.take<unsigned long long>(1);
    const auto sRuns = layR.take<int32_t>((size_t)dev_cap * 3);
    c->s_clu0.ensure(lay.bytes());
    c->s_clu1.ensure(layR.bytes());
    std::vector<uint32_t> pen((size_t)std::max(NA, NB));
    auto upload = [&](const uint64_t* P, const uint8_t* u, int N, uint4* dP, uint32_t* dPen) {
        for (int i = 0; i < N; ++i) pen[(size_t)i] = u[i] ? 0u : PR_NEVER;
        HIP_CHECK(hipMemcpyAsync(dP, P, (size_t)N * 16, hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipMemcpyAsync(dPen, pen.data(), (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));            // (pen is filled again for B)
    };
    upload(A, ua, NA, sA.in(c->s_clu0), sPa.in(c->s_clu0));
    if (!self) upload(B, ub, NB, sB.in(c->s_clu0), sPb.in(c->s_clu0));
    HIP_CHECK(hipMemsetAsync(sCount.in(c->s_clu0), 0, 8, c->stream));
    RunsArgs a;
    a.A = sA.in(c->s_clu0); a.pa = sPa.in(c->s_clu0);
    a.B = self ? a.A : sB.in(c->s_clu0); a.pb = self ? a.pa : sPb.in(c->s_clu0);
    a.NA = NA; a.NB = NB; a.d0 = (int)d0; a.ndiag = (int)ndiag; a.tau = (uint32_t)tau; a.min_len = min_len;
    a.runs = sRuns.in(c->s_clu1); a.cap = (unsigned long long)dev_cap; a.count = sCount.in(c->s_clu0);
    {
        ProfScope prof(c, "runs");
        hipLaunchKernelGGL(print_runs_k, dim3((unsigned)((ndiag + PR_D - 1) / PR_D), (unsigned)((NA + PR_S - 1) / PR_S)), dim3(PR_D), 0, c->stream, a);
        HIP_CHECK(hipGetLastError());
    }
    unsigned long long count = 0;
    HIP_CHECK(hipMemcpyAsync(&count, a.count, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    *found = (int64_t)count;
    if ((int64_t)count > cap || count == 0) return;
    HIP_CHECK(hipMemcpyAsync(runs, a.runs, (size_t)count * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    struct Run { int32_t i, j, len; };
    static_assert(sizeof(Run) == 12, "a run is three int32");
    Run* r = reinterpret_cast<Run*>(runs);
    std::sort(r, r + count, [](const Run& x, const Run& y) { return x.j - x.i != y.j - y.i ? x.j - x.i < y.j - y.i : x.i < y.i; });
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

extern "C" int32_t pvf_frame_prints(pvf_handle h, const pvf_handle* frames, int32_t n, uint64_t* out, int32_t out_on_device)
{
    API_BEGIN
    ENTER(c, h);
    prints_run(c, frames, n, out, out_on_device != 0);
    API_END
}

extern "C" int32_t pvf_print_runs(pvf_handle h, const uint64_t* A, const uint8_t* usable_a, int32_t NA, const uint64_t* B, const uint8_t* usable_b,
                                  int32_t NB, int32_t tau, int32_t min_len, int32_t min_gap, int32_t* runs, int64_t cap, int64_t* found)
{
    API_BEGIN
    runs_check(A, usable_a, NA, B, usable_b, NB, tau, min_len, min_gap, runs, cap, found);
    ENTER(c, h);
    runs_dev(c, A, usable_a, NA, B, usable_b, NB, tau, min_len, min_gap, runs, cap, found);
    API_END
}
