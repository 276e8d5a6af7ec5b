// search.hip -- the EXACT k nearest rows of a table for every query row (pvf_search; SEARCH.md states the rules in integers).
//
// A descriptor of an embedding file is a 5-decimal number, i.e. an integer over 10^5: q(v) = rint(v * 100000.0), |q| <= 2^20.  On such
// integers the squared Euclidean distance is an integer of at most 128 * (2^21)^2 = 2^49 < 2^53: every product, every partial sum of the
// f64 matrix cores and the Gram form |a|^2 + |b|^2 - 2 a.b are exact in float64 in ANY order of additions.  So the ranking by
// (d2, row index) is a pure function of the inputs, and this file is held to a numpy restatement bit for bit (tests/search_ref.py).
//
//   search_quant_k   float64 rows -> quantised rows as float32 (exact below 2^24; 512 bytes a row) + |row|^2 as an exact double; the
//                    position of the first value that is not finite or lies beyond 2^20 goes into a flag (row-major minimum).  Once the
//                    flag is set the kernels below return at once: nothing is computed from a refused table.
//   search_tiles_k   the rectangular tile of cross_tiles_k (identify.hip) without its segment reductions: a wave keeps the 32 A fragments
//                    of a 16-row query block in registers, the workgroup stages 16-row table blocks through LDS (the next block is
//                    requested from HBM before the MFMAs of the current one and converted float32 -> float64 on its way into LDS), 32
//                    v_mfma_f64_16x16x4_f64 per tile, then d2 = na + nb - 2 dot.  No cancellation branch, no sqrt.  Grid: (query blocks /
//                    4, column ranges).  SELECTION: per (query row, range) a list of the k best so far, sorted by (d2, index), lives in
//                    a global arena beside a pending region of kp = max(64, k rounded up to a power of two) entries.  The list's k-th d2
//                    is the row's bound; an entry with d2 below the bound (an equal d2 loses: its index is higher than every listed one)
//                    is appended to the pending region, in column order (ballot prefix, no atomics).  When fewer than 16 free pending
//                    entries are left -- a tile adds at most 16 per row -- the wave sorts list + pending in LDS (bitonic, 64-bit keys
//                    d2 << 11 | position: positions follow the index order) and keeps the first k.  Lists persist from chunk to chunk.
//   search_merge_k   one workgroup per query: the lists of its ranges, each sorted, are merged one after the other into the k best in
//                    (d2, index) order (bitonic merge of an ascending and a reversed list), then idx / d2 / count are written.
// Device memory: O(chunk + Q * ranges * kp); Q x N exists only as work.
#include "pvf_internal.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>

typedef double f64x4 __attribute__((ext_vector_type(4)));
#define SR_PITCH 130                      // doubles per staged row, as in cross_tiles_k: distinct bank pairs for the B fragment reads
static constexpr unsigned long long SR_NONE = ~0ull;
static constexpr int SR_DIM = 128, SR_MAX_K = 1024, SR_MIN_BUF = 64, SR_RANGE_MIN_BLOCKS = 16, SR_TARGET_WG = 768;
static constexpr int64_t SR_DEFAULT_CHUNK = 1 << 18, SR_ARENA_MAX = (int64_t)1 << 30;
static constexpr double SR_Q_MAX = 1048576.0;        // 2^20

__global__ void __launch_bounds__(256) search_quant_k(const double* __restrict__ X, int n, long long row0, float* __restrict__ out,
                                                      double* __restrict__ nrm, unsigned long long* __restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;                              // (a whole wave)
    double s = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = lane + 64 * h;
        const double v = X[(size_t)row * SR_DIM + c];
        double q = __builtin_rint(v * 100000.0);       // ties to even
        if (!(__builtin_isfinite(v) && __builtin_fabs(q) <= SR_Q_MAX)) {
            atomicMin(flag, (unsigned long long)(row0 + row) * SR_DIM + c);
            q = 0.0;
        }
        out[(size_t)row * SR_DIM + c] = (float)q;
        s += q * q;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);      // integers below 2^47: exact in any order
    if (lane == 0) nrm[row] = s;
}

namespace {
// LDS traffic between the lanes of ONE wave: the wave's LDS instructions are served in order; this keeps the compiler from moving them
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// list (n entries, sorted) + pending (p entries, in index order) of one query row -> the min(k, n + p) smallest, sorted, back in the list.
// One wave; wk / wi: its 2 kp keys and indices in LDS.  The list goes into the lower half as it is (ascending, padded), the pending entries
// into the upper half, which is sorted DESCENDING; the two halves then form a bitonic sequence and one merge finishes.  A key is
// d2 << 11 | position: list before pending, each in index order, so equal distances keep the order of their indices.  The entries were
// stored by lanes of this wave through this CU's L1: a workgroup-scope fence orders them, nothing wider is needed.
// Returns the new length; *bound = the k-th d2, or +inf while the list is short.
__device__ __forceinline__ int sr_compact(const SrArgs& a, size_t base, int lane, unsigned long long* wk, int* wi, int n, int p, double* bound)
{
    const int kp = a.kp, W = 2 * kp;
    wave_sync();
    for (int s = lane; s < W; s += 64) {
        const bool ok = s < kp ? s < n : s - kp < p;
        wk[s] = ok ? (((unsigned long long)a.a_d2[base + s] << 11) | (unsigned)s) : SR_NONE;      // d2 <= 2^49, s < 2^11
        wi[s] = ok ? a.a_idx[base + s] : -1;
    }
    wave_sync();
    unsigned long long* up_half = wk + kp;
    for (int size = 2; size <= kp; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < kp / 2; t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                const bool down = (i & size) == 0;               // (the last pass, size == kp: all of it descending)
                const unsigned long long x = up_half[i], y = up_half[l];
                if ((x < y) == down) { up_half[i] = y; up_half[l] = x; }
            }
            wave_sync();
        }
    }
    for (int j = kp; j > 0; j >>= 1) {
        for (int t = lane; t < kp; t += 64) {
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
            const unsigned long long x = wk[i], y = wk[l];
            if (x > y) { wk[i] = y; wk[l] = x; }
        }
        wave_sync();
    }
    const int m = min(a.k, n + p);
    for (int s = lane; s < m; s += 64) {
        const unsigned long long key = wk[s];
        a.a_d2[base + s] = (long long)(key >> 11);
        a.a_idx[base + s] = wi[key & 2047];
    }
    *bound = (m == a.k) ? (double)(wk[a.k - 1] >> 11) : INFINITY;
    wave_sync();
    return m;
}
} // namespace

// grid (query blocks / 4, column ranges): a wave owns one query block and sweeps every table block of the workgroup's range.
// dynamic LDS: 4 waves x 2 kp x (8 + 4) bytes
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) search_tiles_k(SrArgs a)
{
    constexpr int KS = SR_DIM / 4;
    __shared__ __attribute__((aligned(16))) double Bs[2][16 * SR_PITCH];
    __shared__ double colNrm[2][16];                  // |x|^2 per staged column
    __shared__ int colGrp[2][16];                     // its group (-1: none), INT_MIN: padding past the chunk's last row
    __shared__ double s_bd[4][16];                    // per wave and query row: the bound
    __shared__ int s_n[4][16], s_p[4][16];            // length of the list, of the pending region
    extern __shared__ __attribute__((aligned(16))) unsigned char sr_dyn[];
    if (a.flag[0] != SR_NONE || a.flag[1] != SR_NONE) return;             // a refused value: nothing is computed (uniform)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long* wk = reinterpret_cast<unsigned long long*>(sr_dyn) + (size_t)wave * 2 * a.kp;
    int* wi = reinterpret_cast<int*>(sr_dyn + (size_t)4 * 2 * a.kp * 8) + (size_t)wave * 2 * a.kp;
    const int ab = blockIdx.x * 4 + wave;             // query block of this wave
    const bool have = ab < a.nbq;                     // (a wave without one still stages its share of every table block)
    const int nbc = (a.n + 15) / 16;
    const int cb0 = blockIdx.y * a.range_blocks, cb1 = min(cb0 + a.range_blocks, nbc);
    if (cb0 >= cb1) return;                           // (the last chunk may leave ranges empty: their lists stay as they are)
    const int ar0 = have ? ab * 16 : 0, anr = have ? min(16, a.Q - ab * 16) : 0;
    const int i16 = lane & 15, k4 = lane >> 4;
    double af[KS];
    {
        const float* xa = a.Qf + (size_t)(ar0 + i16) * SR_DIM + k4;      // (rows past Q are zeros)
#pragma unroll
        for (int s = 0; s < KS; ++s) af[s] = have ? (double)xa[4 * s] : 0.0;
    }
    double na4[4];
    int qg[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = k4 + 4 * r;                    // C-layout row of register r
        const bool ok = row < anr;
        na4[r] = ok ? a.nq[ar0 + row] : 0.0;
        qg[r] = ok ? a.qgrp[ar0 + row] : -1;
    }
    // this wave's lists: where they stand after the chunks before
    const size_t W = (size_t)2 * a.kp;
    if (lane < 16) {
        const size_t slot = (size_t)(ar0 + lane) * a.n_ranges + blockIdx.y;
        const int n = have ? a.a_cnt[slot] : 0;
        s_n[wave][lane] = n; s_p[wave][lane] = 0;
        s_bd[wave][lane] = (have && n == a.k) ? (double)a.a_d2[slot * W + a.k - 1] : INFINITY;
    }
    // staging: thread t carries 8 values of row t / 16 of the block from HBM to LDS, float32 -> float64; the block for step cb + 1 is
    // requested before the MFMAs of step cb and written after them
    float4 u0, u1;
    double pn = 0.0;
    int pg = 0;
    auto fetch = [&](int cb) {
        const int r = cb * 16 + (tid >> 4);
        const bool ok = r < a.n;
        const float4* p = reinterpret_cast<const float4*>(a.Xf + (size_t)(ok ? r : 0) * SR_DIM + (tid & 15) * 8);
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        u0 = ok ? p[0] : z; u1 = ok ? p[1] : z;
        if (tid < 16) {
            const int rr = cb * 16 + tid;
            const bool okk = rr < a.n;
            pn = okk ? a.nx[rr] : 0.0;
            pg = okk ? (a.rgrp ? max(a.rgrp[rr], -1) : -1) : (int)0x80000000;
        }
    };
    auto put = [&](int buf) {
        double* d = &Bs[buf][(tid >> 4) * SR_PITCH + (tid & 15) * 8];
        d[0] = u0.x; d[1] = u0.y; d[2] = u0.z; d[3] = u0.w; d[4] = u1.x; d[5] = u1.y; d[6] = u1.z; d[7] = u1.w;
        if (tid < 16) { colNrm[buf][tid] = pn; colGrp[buf][tid] = pg; }
    };
    fetch(cb0);
    put(0);
    __syncthreads();
    for (int cb = cb0; cb < cb1; ++cb) {
        const int buf = (cb - cb0) & 1;
        if (cb + 1 < cb1) fetch(cb + 1);
        if (have) {
            f64x4 acc = (f64x4){0.0, 0.0, 0.0, 0.0};
            const double* bp = &Bs[buf][i16 * SR_PITCH + k4];
#pragma unroll
            for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af[s], bp[4 * s], acc, 0, 0, 0);
            // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * reg
            const double nb = colNrm[buf][i16];
            const int cg = colGrp[buf][i16];
            const bool colok = cg != (int)0x80000000;
            double d2[4];
            bool v[4];
            bool any = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = k4 + 4 * r;
                d2[r] = (na4[r] + nb) - 2.0 * acc[r];              // three exact terms
                v[r] = colok && row < anr && !(qg[r] >= 0 && qg[r] == cg) && (a.cut < 0.0 || d2[r] <= a.cut) && d2[r] < s_bd[wave][row];
                any = any || v[r];
            }
            if (__builtin_amdgcn_ballot_w64(any) != 0) {           // some lane of the wave holds a candidate
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = k4 + 4 * r;
                    const unsigned bits = (unsigned)(__builtin_amdgcn_ballot_w64(v[r]) >> (k4 * 16)) & 0xffffu;      // the 16 columns of this row
                    if (bits) {
                        const int p0 = s_p[wave][row];
                        if (v[r]) {
                            const size_t dst = ((size_t)(ar0 + row) * a.n_ranges + blockIdx.y) * W + a.kp + p0 + __builtin_popcount(bits & ((1u << i16) - 1u));
                            a.a_d2[dst] = (long long)d2[r];
                            a.a_idx[dst] = a.row0 + cb * 16 + i16;
                        }
                        if (i16 == 0) s_p[wave][row] = p0 + __builtin_popcount(bits);
                    }
                }
                wave_sync();
#pragma unroll 1
                for (int row = 0; row < 16; ++row) {
                    const int p = __builtin_amdgcn_readfirstlane(s_p[wave][row]);
                    if (p + 16 > a.kp) {                           // the next tile may add 16
                        const int n = __builtin_amdgcn_readfirstlane(s_n[wave][row]);
                        double bd;
                        const int m = sr_compact(a, ((size_t)(ar0 + row) * a.n_ranges + blockIdx.y) * W, lane, wk, wi, n, p, &bd);
                        if (lane == 0) { s_n[wave][row] = m; s_p[wave][row] = 0; s_bd[wave][row] = bd; }
                        wave_sync();
                    }
                }
            }
        }
        if (cb + 1 < cb1) put(buf ^ 1);
        __syncthreads();
    }
    if (!have) return;
    wave_sync();
#pragma unroll 1
    for (int row = 0; row < 16; ++row) {
        const int p = __builtin_amdgcn_readfirstlane(s_p[wave][row]);
        if (p > 0) {
            const int n = __builtin_amdgcn_readfirstlane(s_n[wave][row]);
            double bd;
            const int m = sr_compact(a, ((size_t)(ar0 + row) * a.n_ranges + blockIdx.y) * W, lane, wk, wi, n, p, &bd);
            if (lane == 0) { s_n[wave][row] = m; s_p[wave][row] = 0; }
            wave_sync();
        }
    }
    if (lane < 16) a.a_cnt[(size_t)(ar0 + lane) * a.n_ranges + blockIdx.y] = s_n[wave][lane];
}

// one workgroup per query: the sorted lists of its ranges -> the k best in (d2, index) order.  Lists hold rows of several chunks each, so
// the index is compared too.  dynamic LDS: 2 kp x (8 + 4) bytes
__global__ void __launch_bounds__(256) search_merge_k(const long long* __restrict__ a_d2, const int* __restrict__ a_idx, const int* __restrict__ a_cnt,
                                                      int n_ranges, int k, int kp, const unsigned long long* __restrict__ flag,
                                                      int32_t* __restrict__ idx, long long* __restrict__ d2, int32_t* __restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_dyn[];
    __shared__ int n_hits;
    if (flag[0] != SR_NONE || flag[1] != SR_NONE) return;
    const int W = 2 * kp, tid = threadIdx.x, q = blockIdx.x;
    long long* md = reinterpret_cast<long long*>(sm_dyn);
    int* mi = reinterpret_cast<int*>(sm_dyn + (size_t)W * 8);
    const long long D_NONE = 0x7fffffffffffffffLL;
    for (int s = tid; s < kp; s += 256) { md[s] = D_NONE; mi[s] = 0x7fffffff; }
    if (tid == 0) n_hits = 0;
    for (int l = 0; l < n_ranges; ++l) {
        const size_t slot = (size_t)q * n_ranges + l;
        const int n = a_cnt[slot];
        if (n == 0) continue;                          // (uniform)
        __syncthreads();
        {   // a list whose first entry does not beat the k-th best so far adds nothing (uniform: every thread reads the same values)
            const long long f = a_d2[slot * W], b = md[k - 1];
            if (f > b || (f == b && a_idx[slot * W] > mi[k - 1])) continue;
        }
        for (int s = tid; s < kp; s += 256) {          // the list, reversed, into the upper half: ascending + descending = bitonic
            const bool ok = s < n;
            md[W - 1 - s] = ok ? a_d2[slot * W + s] : D_NONE;
            mi[W - 1 - s] = ok ? a_idx[slot * W + s] : 0x7fffffff;
        }
        __syncthreads();
        for (int j = kp; j > 0; j >>= 1) {
            for (int t = tid; t < kp; t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), m = i + j;
                const long long x = md[i], y = md[m];
                const int xi = mi[i], yi = mi[m];
                if (x > y || (x == y && xi > yi)) { md[i] = y; mi[i] = yi; md[m] = x; mi[m] = xi; }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int s = tid; s < k; s += 256) {
        const bool hit = md[s] != D_NONE;
        idx[(size_t)q * k + s] = hit ? mi[s] : -1;
        d2[(size_t)q * k + s] = hit ? md[s] : -1;
        if (hit) atomicAdd(&n_hits, 1);
    }
    __syncthreads();
    if (tid == 0) count[q] = n_hits;
}

namespace {

// every limit of a call, on the host, before any device work
void search_check(int Q, int64_t N, int dim, int k, int64_t max_d2, const int32_t* query_group, const int32_t* row_group)
{
    PVF_REQUIRE(dim == 128, "pvf_search: dim must be 128 (the descriptor of the embedder; the matrix-core kernel is built for it)");
    PVF_REQUIRE(Q >= 1 && N >= 1, "pvf_search: Q and N must be at least 1");
    PVF_REQUIRE(k >= 1 && k <= SR_MAX_K, "pvf_search: k must lie in 1 .. 1024");
    PVF_REQUIRE(N <= ((int64_t)1 << 30), "pvf_search: more than 2^30 rows (32-bit row indices)");
    PVF_REQUIRE(Q <= (1 << 24), "pvf_search: more than 2^24 queries");
    PVF_REQUIRE(max_d2 >= -1, "pvf_search: max_d2 must be at least -1 (-1: no cut)");
    PVF_REQUIRE((query_group == nullptr) == (row_group == nullptr), "pvf_search: query_group and row_group are given together or not at all");
}

// how a call is cut: rows per chunk (PVF_SEARCH_CHUNK, the test switch, read at every call; whole 16-row blocks), column ranges per chunk
// (the same number for every chunk: range r of every chunk feeds list r), the pending region
SrPlan search_plan(int Q, int64_t N, int k)
{
    SrPlan p;
    int64_t chunk = SR_DEFAULT_CHUNK;
    const char* e = getenv("PVF_SEARCH_CHUNK");
    if (e && atoll(e) > 0) chunk = std::min<int64_t>(atoll(e), (int64_t)1 << 22);
    chunk = (std::min(chunk, N) + 15) / 16 * 16;
    p.chunk_rows = chunk;
    p.n_chunks = (N + chunk - 1) / chunk;
    int kp = SR_MIN_BUF;
    while (kp < k) kp *= 2;
    p.kp = kp;
    const int64_t nbq = (Q + 15) / 16, row_groups = (nbq + 3) / 4, nb = chunk / 16;
    int64_t r = std::max<int64_t>(1, std::min<int64_t>(SR_TARGET_WG / row_groups, (nb + SR_RANGE_MIN_BLOCKS - 1) / SR_RANGE_MIN_BLOCKS));
    while (r > 1 && nbq * 16 * r * 2 * kp * 12 > SR_ARENA_MAX) r = (r + 1) / 2;
    p.range_blocks = (nb + r - 1) / r;
    p.n_ranges = (nb + p.range_blocks - 1) / p.range_blocks;
    p.arena_entries = nbq * 16 * p.n_ranges * 2 * kp;
    return p;
}

void search_dev(Ctx* c, const double* Qrows, int Q, const double* X, int64_t N, int k, int64_t max_d2, const int32_t* query_group,
                const int32_t* row_group, int32_t* idx, int64_t* d2, int32_t* count)
{
    const SrPlan pl = search_plan(Q, N, k);
    const int nbq = (Q + 15) / 16, Q16 = nbq * 16, row_groups = (nbq + 3) / 4, kp = (int)pl.kp, n_ranges = (int)pl.n_ranges;
    PVF_REQUIRE(n_ranges <= 65535, "pvf_search: too many column ranges");
    const size_t chunk = (size_t)pl.chunk_rows;
    // ---- device buffers: queries, one chunk and the flags in s_clu0; the arena and the results in s_clu1
    ScratchLayout lay;
    const auto sQd = lay.take<double>((size_t)Q * SR_DIM), sXd = lay.take<double>(chunk * SR_DIM);
    const auto sQf = lay.take<float>((size_t)Q16 * SR_DIM), sXf = lay.take<float>(chunk * SR_DIM);
    const auto sNQ = lay.take<double>(Q16), sNX = lay.take<double>(chunk);
    const auto sQG = lay.take<int>(Q16), sRG = lay.take<int>(chunk);
    const auto sFlag = lay.take<unsigned long long>(2);
    ScratchLayout layA;
    const auto sAD = layA.take<long long>((size_t)pl.arena_entries);
    const auto sAI = layA.take<int>((size_t)pl.arena_entries), sCnt = layA.take<int>((size_t)Q16 * n_ranges);
    const auto sOD = layA.take<long long>((size_t)Q * k);
    const auto sOI = layA.take<int32_t>((size_t)Q * k), sOC = layA.take<int32_t>(Q);
    c->s_clu0.ensure(lay.bytes());
    c->s_clu1.ensure(layA.bytes());
    double* dQd = sQd.in(c->s_clu0); double* dXd = sXd.in(c->s_clu0); float* dQf = sQf.in(c->s_clu0); float* dXf = sXf.in(c->s_clu0);
    double* dNQ = sNQ.in(c->s_clu0); double* dNX = sNX.in(c->s_clu0); int* dQG = sQG.in(c->s_clu0); int* dRG = sRG.in(c->s_clu0);
    unsigned long long* dFlag = sFlag.in(c->s_clu0);
    long long* dAD = sAD.in(c->s_clu1); int* dAI = sAI.in(c->s_clu1); int* dCnt = sCnt.in(c->s_clu1);
    long long* dOD = sOD.in(c->s_clu1); int32_t* dOI = sOI.in(c->s_clu1); int32_t* dOC = sOC.in(c->s_clu1);
    const size_t lds_tiles = (size_t)4 * 2 * kp * 12, lds_merge = (size_t)2 * kp * 12;
    if (lds_tiles + 36 * 1024 > 64 * 1024) {           // (above the default limit per workgroup; static LDS of the kernel: 34.5 KB)
        static std::atomic<unsigned> attr_on{0};
        const unsigned bit = 1u << (c->device & 31);
        if (!(attr_on.load() & bit)) {
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(search_tiles_k), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 2 * SR_MAX_K * 12));
            attr_on.fetch_or(bit);
        }
    }
    unsigned long long flag[2] = {SR_NONE, SR_NONE};
    auto refuse = [&](const char* what, unsigned long long pos) {
        char b[200];
        snprintf(b, sizeof b, "pvf_search: %s[%llu][%d] is not finite or lies beyond 2^20 units of 1e-5 (|v| above about 10.48): refused, nothing is clamped",
                 what, pos / SR_DIM, (int)(pos % SR_DIM));
        throw PvfError(b);
    };
    // ---- the queries
    HIP_CHECK(hipMemsetAsync(dFlag, 0xff, 16, c->stream));
    HIP_CHECK(hipMemsetAsync(dQf, 0, (size_t)Q16 * SR_DIM * 4, c->stream));
    HIP_CHECK(hipMemsetAsync(dNQ, 0, (size_t)Q16 * 8, c->stream));
    HIP_CHECK(hipMemsetAsync(dQG, 0xff, (size_t)Q16 * 4, c->stream));
    HIP_CHECK(hipMemsetAsync(dCnt, 0, (size_t)Q16 * n_ranges * 4, c->stream));
    HIP_CHECK(hipMemcpyAsync(dQd, Qrows, (size_t)Q * SR_DIM * 8, hipMemcpyHostToDevice, c->stream));
    if (query_group) HIP_CHECK(hipMemcpyAsync(dQG, query_group, (size_t)Q * 4, hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, "search");
        hipLaunchKernelGGL(search_quant_k, dim3((Q + 3) / 4), dim3(256), 0, c->stream, dQd, Q, 0LL, dQf, dNQ, dFlag);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(flag, dFlag, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (flag[0] != SR_NONE) refuse("Qrows", flag[0]);
    // ---- the table, chunk by chunk
    SrArgs a;
    a.Qf = dQf; a.nq = dNQ; a.qgrp = dQG; a.Xf = dXf; a.nx = dNX; a.rgrp = row_group ? dRG : nullptr;
    a.Q = Q; a.nbq = nbq; a.range_blocks = (int)pl.range_blocks; a.n_ranges = n_ranges; a.k = k; a.kp = kp;
    a.cut = (max_d2 < 0) ? -1.0 : (double)std::min<int64_t>(max_d2, (int64_t)1 << 50);      // (no d2 is above 2^49)
    a.a_d2 = dAD; a.a_idx = dAI; a.a_cnt = dCnt; a.flag = dFlag;
    for (int64_t r0 = 0; r0 < N; r0 += (int64_t)chunk) {
        const int n = (int)std::min<int64_t>((int64_t)chunk, N - r0);
        HIP_CHECK(hipMemcpyAsync(dXd, X + (size_t)r0 * SR_DIM, (size_t)n * SR_DIM * 8, hipMemcpyHostToDevice, c->stream));
        if (row_group) HIP_CHECK(hipMemcpyAsync(dRG, row_group + r0, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        a.n = n; a.row0 = (int)r0;
        ProfScope ps(c, "search");
        hipLaunchKernelGGL(search_quant_k, dim3((n + 3) / 4), dim3(256), 0, c->stream, dXd, n, (long long)r0, dXf, dNX, dFlag + 1);
        hipLaunchKernelGGL(search_tiles_k, dim3(row_groups, n_ranges), dim3(256), lds_tiles, c->stream, a);
    }
    {
        ProfScope ps(c, "search");
        hipLaunchKernelGGL(search_merge_k, dim3(Q), dim3(256), lds_merge, c->stream, dAD, dAI, dCnt, n_ranges, k, kp, dFlag, dOI, dOD, dOC);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(flag, dFlag, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (flag[1] != SR_NONE) refuse("X", flag[1]);
    static_assert(sizeof(long long) == sizeof(int64_t), "d2 is copied as it lies");
    HIP_CHECK(hipMemcpyAsync(idx, dOI, (size_t)Q * k * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(d2, dOD, (size_t)Q * k * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(count, dOC, (size_t)Q * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
} // namespace

// ---- what cast.hip runs of this file (declared in pvf_internal.h): the plan and the three kernels, on c->stream, unchanged
SrPlan search_plan_of(int Q, int64_t N, int k) { return search_plan(Q, N, k); }
void search_quant_launch(Ctx* c, const double* X, int n, long long row0, float* out, double* nrm, unsigned long long* flag)
{
    hipLaunchKernelGGL(search_quant_k, dim3((n + 3) / 4), dim3(256), 0, c->stream, X, n, row0, out, nrm, flag);
}
void search_tiles_launch(Ctx* c, const SrArgs& a)      // (a.kp <= 256: the dynamic LDS stays below the default limit)
{
    hipLaunchKernelGGL(search_tiles_k, dim3((a.nbq + 3) / 4, a.n_ranges), dim3(256), (size_t)4 * 2 * a.kp * 12, c->stream, a);
}
void search_merge_launch(Ctx* c, const SrArgs& a, int32_t* idx, long long* d2, int32_t* count)
{
    hipLaunchKernelGGL(search_merge_k, dim3(a.Q), dim3(256), (size_t)2 * a.kp * 12, c->stream, a.a_d2, a.a_idx, a.a_cnt, a.n_ranges, a.k, a.kp, a.flag,
                       idx, d2, count);
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

extern "C" int32_t pvf_search(pvf_handle h, const double* Qrows, int32_t Q, const double* X, int64_t N, int32_t dim, int32_t k, int64_t max_d2,
                              const int32_t* query_group, const int32_t* row_group, int32_t* idx, int64_t* d2, int32_t* count)
{
    API_BEGIN
    search_check(Q, N, dim, k, max_d2, query_group, row_group);
    PVF_REQUIRE(Qrows && X && idx && d2 && count, "pvf_search: bad arguments");
    ENTER(c, h);
    search_dev(c, Qrows, Q, X, N, k, max_d2, query_group, row_group, idx, d2, count);
    API_END
}

// host only: how pvf_search would cut a call of these sizes (what the tests restate)
extern "C" int32_t pvf_search_plan(int32_t Q, int64_t N, int32_t k, int64_t out[6])
{
    API_BEGIN
    search_check(Q, N, 128, k, -1, nullptr, nullptr);
    PVF_REQUIRE(out, "pvf_search_plan: bad arguments");
    const SrPlan p = search_plan(Q, N, k);
    out[0] = p.chunk_rows; out[1] = p.n_chunks; out[2] = p.n_ranges; out[3] = p.range_blocks; out[4] = p.kp; out[5] = p.arena_entries * 12;
    API_END
}
