// identify.hip -- face identification against a gallery of enrolled, named descriptors: D[t][k] = the mean pairwise distance between the
// rows of query group t (a track or a cluster) and the rows of identity k, and the decision per group (the nearest identity, if its mean
// distance is at most the threshold; the runner-up beside it).  No reference call: naming a 128-D descriptor by its distance to known
// faces is the use the embedder was trained for, and the measure is the one `cluster` merges by (face/clustering.py:116-119, :138-141) --
// identification is one more average-linkage step against fixed, named clusters.
//
// cross_tiles_k is the RECTANGULAR form of K10 (cluster.hip, pair_tiles_k), built the same way: 16-row blocks with segments on both sides,
// a wave keeps its query block's 32 A fragments in registers, the workgroup stages gallery blocks asynchronously through LDS, 32 f64 MFMAs
// per 16 x 16 tile, the Gram-form distance recomputed from differences where it cancels (a query row that IS a gallery row is the expected
// case here: a person enrolled from the same video), the two 0/1-matrix MFMA reductions to (row segment, column segment), the lane
// shuffle that carries a column segment into the next block, parts of row groups that span blocks summed in part order.  What differs:
//   * the row table (queries, N rows in T groups) and the column table (gallery, M rows in K identities) are different arrays, each with
//     its own blocking;
//   * EVERY column block is visited: no triangle, no i < j filter, no mirror;
//   * the output is T x K;
//   * column ranges are cut from the gallery's blocks only, at clean blocks.
// Neither N x M nor N x K is materialised.  An entry is defined up to the test tolerance, not bit for bit across inputs: the additions
// that form it depend on where the rows of its group and of its identity fall in their 16-row blocks (the same call gives the same bits).
#include "pvf_internal.h"
#include <algorithm>
#include <cmath>

typedef double f64x4 __attribute__((ext_vector_type(4)));
#define CT_PITCH 130                      // doubles per staged row, as in pair_tiles_k: distinct bank pairs for the B fragment reads

struct CtArgs {
    const double* X; const double* G;                  // queries [N][128], gallery [M][128]
    const double* nrm_x; const double* nrm_g;          // |row|^2
    int N, M, K;
    const int* q_segidx;                               // per query row: index of its segment inside its block
    const int* q_seg_group; const int* q_seg_part;     // [query block][16]: group of each segment (-1: none); its row in P (-1: the segment is its whole group)
    const int* g_segidx;                               // per gallery row: index of its segment inside its block
    const int* g_seg_id;                               // [gallery block][16]: identity of each segment (-1: none)
    const int* g_blk_cont;                             // per gallery block: the segment that goes on in the next block, or -1
    const int* range_b0;                               // column ranges: gallery block bounds [n_ranges + 1]
    double* D; double* P;                              // T x K sums; [parts][K] sums of the groups that span blocks
    int nbq, metric;
};

__global__ void __launch_bounds__(256) id_row_norms_k(const double* __restrict__ X, int N, int dim, double* __restrict__ nrm)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= N) return;
    double s = 0;
    for (int k = 0; k < dim; ++k) { const double v = X[(size_t)a * dim + k]; s += v * v; }
    nrm[a] = s;
}

namespace {
// sqrt of a squared distance (0, or far from the ends of the exponent range): the steps of cluster.hip's sqrt_nonneg, i.e. the device
// library's own without its rescaling and class checks
__device__ __forceinline__ double sqrt_nonneg(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    g = __builtin_fma(__builtin_fma(-g, g, x), h, g);
    g = __builtin_fma(__builtin_fma(-g, g, x), h, g);
    return x == 0.0 ? 0.0 : g;                       // (rsq(0) is infinite)
}
} // namespace

// grid (query blocks / 4, column ranges): a wave owns one query block and sweeps every gallery block of the workgroup's range
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) cross_tiles_k(CtArgs a)
{
    constexpr int DIM = 128, KS = DIM / 4;
    __shared__ __attribute__((aligned(16))) double Bs[2][16 * CT_PITCH];
    __shared__ int colSeg[2][16];                     // per staged column: segment index inside its block (-1: padding)
    __shared__ int colSegId[2][16];                   // per segment of the staged block: its identity (-1: none)
    __shared__ double colNrm[2][16];                  // |g|^2 per staged column
    __shared__ int colCont[2];                        // the staged block's segment that goes on in the next block (-1: none)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ab = blockIdx.x * 4 + wave;             // query block of this wave
    const bool have = ab < a.nbq;                     // (a wave without one still stages its share of every gallery block)
    const int cb0 = a.range_b0[blockIdx.y], cb1 = a.range_b0[blockIdx.y + 1];
    if (cb0 >= cb1) return;
    const int ar0 = have ? ab * 16 : 0, anr = have ? min(16, a.N - ab * 16) : 0;
    const int i16 = lane & 15, k4 = lane >> 4;
    double af[KS];
    {
        const bool ok = have && i16 < anr;
        const double* xa = a.X + (size_t)(ar0 + (ok ? i16 : 0)) * DIM + k4;
#pragma unroll
        for (int s = 0; s < KS; ++s) af[s] = ok ? xa[4 * s] : 0.0;
    }
    double na4[4], rb[4];
    int rt[4], rpart[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = k4 + 4 * r;                    // C-layout row of register r == K index of step r in the row reduction
        const bool ok = have && row < anr;
        na4[r] = ok ? a.nrm_x[ar0 + row] : 0.0;
        rb[r] = (ok && a.q_segidx[ar0 + row] == i16) ? 1.0 : 0.0;            // Rind^T[row][segment i16]
        // T2's C layout: register r of this lane holds row segment k4 + 4 r, column segment i16
        const int seg = k4 + 4 * r;
        rt[r] = have ? a.q_seg_group[ab * 16 + seg] : -1;
        rpart[r] = rt[r] >= 0 ? a.q_seg_part[ab * 16 + seg] : -1;
    }
    // staging as in pair_tiles_k: rows wave, wave + 4, ... of the gallery block go straight from HBM into LDS, the block for step cb + 1
    // requested before the MFMAs of step cb; rows past the block's last one are requested beyond the buffer's end, which returns zeros.
    // The descriptor covers this workgroup's column range only: 32-bit offsets whatever M is (the host refuses a range above 2^20 rows).
    const int range_rows = min(a.M - cb0 * 16, (cb1 - cb0) * 16);
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc((void*)(a.G + (size_t)cb0 * 16 * DIM), 0, range_rows * DIM * 8, 0x00020000);
    auto stage = [&](int cb, int buf) {
        const int r0 = cb * 16, nr = min(16, a.M - r0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = wave + 4 * q;
            const int voff = (r < nr) ? lane * 16 : 0x7ffffff0;                  // (wave-uniform choice; out of range -> zeros)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(grs, (__attribute__((address_space(3))) void*)&Bs[buf][r * CT_PITCH], 16, voff,
                                                     (r0 - cb0 * 16 + (r < nr ? r : 0)) * (DIM * 8), 0, 0);
        }
        if (tid < 16) {
            colSeg[buf][tid] = tid < nr ? a.g_segidx[r0 + tid] : -1;
            colSegId[buf][tid] = a.g_seg_id[cb * 16 + tid];
            colNrm[buf][tid] = tid < nr ? a.nrm_g[r0 + tid] : 0.0;
            if (tid == 0) colCont[buf] = a.g_blk_cont[cb];
        }
    };
    f64x4 t2 = (f64x4){0.0, 0.0, 0.0, 0.0};          // sums per (row segment, column segment), carried across the blocks of a long identity
    stage(cb0, 0);
    __builtin_amdgcn_s_waitcnt(0);                     // the rows requested above are in LDS
    __syncthreads();
    for (int cb = cb0; cb < cb1; ++cb) {
        const int buf = (cb - cb0) & 1;
        if (cb + 1 < cb1) stage(cb + 1, buf ^ 1);
        if (have) {
            const int br0 = cb * 16;
            f64x4 acc = (f64x4){0.0, 0.0, 0.0, 0.0};
            const double* bp = &Bs[buf][i16 * CT_PITCH + k4];
#pragma unroll
            for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af[s], bp[4 * s], acc, 0, 0, 0);
            // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * reg.  Rows past the block's last one and padding columns need
            // no masking: their distances are finite (their fragments are zeros) and the 0/1 matrices of the two reductions leave them out.
            const double nb = colNrm[buf][i16];
            double d[4];
            if (a.metric == 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double den = sqrt(na4[r] * nb);
                    d[r] = den > 0.0 ? 1.0 - acc[r] / den : 0.0;
                }
            } else {
                double d2[4];
                bool fix = false;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double sum = na4[r] + nb;
                    d2[r] = sum - 2.0 * acc[r];
                    // the Gram form cancels for close rows (relative error in d: C 2^-53 (|a|^2 + |b|^2) / d^2, C up to 4.5 measured, as in
                    // pair_tiles_k): pairs below GRAM_SWITCH (1e-3: closer than ~4.5e-2 |x|) -- a query row that is a copy of an enrolled
                    // one, or a neighbouring frame of it -- take the differences instead
                    fix = fix || (d2[r] < GRAM_SWITCH * sum && k4 + 4 * r < anr && colSeg[buf][i16] >= 0);
                }
                if (__builtin_amdgcn_ballot_w64(fix) != 0) {           // some lane of the wave holds such a pair
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = k4 + 4 * r;
                        if (d2[r] < GRAM_SWITCH * (na4[r] + nb) && row < anr && colSeg[buf][i16] >= 0) {      // (row < N and column < M)
                            const double* xa = a.X + (size_t)(ar0 + row) * DIM;
                            const double* xb = a.G + (size_t)(br0 + i16) * DIM;
                            double e = 0.0;
                            for (int k = 0; k < DIM; ++k) { const double t = xa[k] - xb[k]; e += t * t; }
                            d2[r] = e;
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) d[r] = sqrt_nonneg(d2[r] > 0.0 ? d2[r] : 0.0);
            }
            // rows of every query group: R'[column][row segment] = sum_row d[row][column] Rind[segment][row]; this lane's d[s] is element
            // (column i16, row 4 s + k4) of d^T, i.e. the A operand of step s
            f64x4 rp = (f64x4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 4; ++s) rp = __builtin_amdgcn_mfma_f64_16x16x4f64(d[s], rb[s], rp, 0, 0, 0);
            // columns of every identity: T2[row segment][column segment] += sum_col R'[col][row segment] Cind[col][column segment];
            // rp[q] is element (row segment i16, column 4 q + k4) of R'^T: the A operand of step q
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double cind = (colSeg[buf][4 * q + k4] == i16) ? 1.0 : 0.0;
                t2 = __builtin_amdgcn_mfma_f64_16x16x4f64(rp[q], cind, t2, 0, 0, 0);
            }
            // complete column segments are written (sums: cross_norm_k / cross_chunks_k divide); the one that goes on in the next block
            // (at most one, the block's last) hands its sums to segment 0 of the next tile
            const int cont = colCont[buf];                 // (uniform)
            const int j = colSegId[buf][i16];
            if (j >= 0 && i16 != cont) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = rt[q];
                    if (i < 0) continue;
                    if (rpart[q] >= 0) a.P[(size_t)rpart[q] * a.K + j] = t2[q];
                    else a.D[(size_t)i * a.K + j] = t2[q];
                }
            }
            f64x4 carry = (f64x4){0.0, 0.0, 0.0, 0.0};
            if (cont >= 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double v = __shfl(t2[q], (lane & 48) | cont, 64);
                    carry[q] = (i16 == 0) ? v : 0.0;
                }
            }
            t2 = carry;
        }
        __builtin_amdgcn_s_waitcnt(0);                 // this wave's share of the next block has arrived ...
        __syncthreads();                               // ... and so has everybody else's
    }
}

// groups that span several query blocks: D[i][k] = (P[c0][k] + P[c0 + 1][k] + ...) / (n_i m_k), parts in order
__global__ void __launch_bounds__(256) cross_chunks_k(const double* __restrict__ P, const int* __restrict__ big_group, const int* __restrict__ big_c0,
                                                      const int* __restrict__ big_nc, const int32_t* __restrict__ row_start,
                                                      const int32_t* __restrict__ gal_start, int K, double* __restrict__ D)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = big_group[blockIdx.y];
    if (k >= K) return;
    double s = 0.0;
    for (int c = 0; c < big_nc[blockIdx.y]; ++c) s += P[(size_t)(big_c0[blockIdx.y] + c) * K + k];
    const double cnt = (double)(row_start[i + 1] - row_start[i]) * (double)(gal_start[k + 1] - gal_start[k]);
    D[(size_t)i * K + k] = s / cnt;
}

// groups that lie inside one query block: cross_tiles_k wrote their sums
__global__ void __launch_bounds__(256) cross_norm_k(double* __restrict__ D, const int32_t* __restrict__ row_start, const int32_t* __restrict__ gal_start,
                                                    const int* __restrict__ is_big, int K)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (k >= K || is_big[i]) return;
    const double cnt = (double)(row_start[i + 1] - row_start[i]) * (double)(gal_start[k + 1] - gal_start[k]);
    D[(size_t)i * K + k] = D[(size_t)i * K + k] / cnt;
}

namespace {
// (value, index) minimum over a wave, smaller index on equal values, left in every lane: the DPP reduction of cluster.hip's wave_argmin
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xf, false); }
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_f64(double v)
{
    return __hiloint2double(dpp_i32<CTRL, ROWS>(__double2hiint(v)), dpp_i32<CTRL, ROWS>(__double2loint(v)));
}
__device__ __forceinline__ void wave_argmin(double& v, int& i)
{
    double m = v;
    m = __builtin_fmin(m, dpp_f64<0x111, 0xf>(m));
    m = __builtin_fmin(m, dpp_f64<0x112, 0xf>(m));
    m = __builtin_fmin(m, dpp_f64<0x114, 0xf>(m));
    m = __builtin_fmin(m, dpp_f64<0x118, 0xf>(m));
    m = __builtin_fmin(m, dpp_f64<0x142, 0xa>(m));
    m = __builtin_fmin(m, dpp_f64<0x143, 0xc>(m));
    const double vmin = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(m), 63), __builtin_amdgcn_readlane(__double2loint(m), 63));
    int c = (v == vmin) ? i : 0x7fffffff;
    c = min(c, dpp_i32<0x111, 0xf>(c));
    c = min(c, dpp_i32<0x112, 0xf>(c));
    c = min(c, dpp_i32<0x114, 0xf>(c));
    c = min(c, dpp_i32<0x118, 0xf>(c));
    c = min(c, dpp_i32<0x142, 0xa>(c));
    c = min(c, dpp_i32<0x143, 0xc>(c));
    v = vmin;
    i = __builtin_amdgcn_readlane(c, 63);
}
} // namespace

// The decision per group, one wave per row of D.  An entry is TAKEN when it is below +inf (`v < bv` from +inf, the comparison of the HAC's
// row minimum: neither NaN nor +inf passes it).  best = the first minimum of the taken entries (lowest k on equal values), second = the
// first minimum over k != best; a row with nothing to take gives (-1, +inf), and so does the second of a row with one taken entry
// (K = 1).  Then best = -1 unless best_dist <= threshold -- hac_persist_k's `!(bv <= threshold)` refuses -- and best_dist keeps the
// measured value either way.  No arithmetic: every output is an input value or an index.
__global__ void __launch_bounds__(256) identify_pick_k(const double* __restrict__ D, int T, int K, double threshold, int32_t* __restrict__ best,
                                                       double* __restrict__ best_dist, int32_t* __restrict__ second, double* __restrict__ second_dist)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;                                // (a whole wave)
    const double* row = D + (size_t)t * K;
    double bv = INFINITY; int bi = 0x7fffffff;
    for (int k = lane; k < K; k += 64) {
        const double v = row[k];
        if (v < bv) { bv = v; bi = k; }                // ascending k per lane: first occurrence kept
    }
    wave_argmin(bv, bi);
    double sv = INFINITY; int si = 0x7fffffff;
    for (int k = lane; k < K; k += 64) {
        const double v = row[k];
        if (k != bi && v < sv) { sv = v; si = k; }
    }
    wave_argmin(sv, si);
    if (lane == 0) {
        best[t] = (bi == 0x7fffffff || !(bv <= threshold)) ? -1 : bi;
        best_dist[t] = bv;
        second[t] = si == 0x7fffffff ? -1 : si;
        second_dist[t] = sv;
    }
}

// every check of a distance call, on the host, before any device work
void identify_check_dist(const char* who, int N, const int32_t* row_start, int T, int M, const int32_t* gal_start, int K, int dim, int metric)
{
    const std::string w(who);
    PVF_REQUIRE(T >= 1 && K >= 1, w + ": T and K must be at least 1");
    PVF_REQUIRE(dim == 128, w + ": dim must be 128 (the descriptor of the embedder; the matrix-core kernel is built for it)");
    PVF_REQUIRE(metric == 0 || metric == 1, w + ": metric 0 (euclidean) or 1 (cosine)");
    PVF_REQUIRE(N >= 1 && M >= 1, w + ": N and M must be at least 1");
    PVF_REQUIRE(N <= (1 << 30) && M <= (1 << 30), w + ": more than 2^30 rows (32-bit block indices)");
    check_groups(who, "row_start", row_start, T, N);
    check_groups(who, "gal_start", gal_start, K, M);
}

void identify_check_pick(const char* who, int T, int K, double threshold)
{
    const std::string w(who);
    PVF_REQUIRE(T >= 1 && K >= 1, w + ": T and K must be at least 1");
    PVF_REQUIRE(!std::isnan(threshold), w + ": the threshold is NaN");
}

// D[t][k] into s_clu1 (returned), and to the host when D_host is given.  Arguments checked by identify_check_dist.
double* gallery_mean_dist_dev(Ctx* c, const double* X, int N, const int32_t* row_start, int T, const double* G, int M, const int32_t* gal_start,
                              int K, int metric, double* D_host)
{
    constexpr int DIM = 128;
    const Blocking q(row_start, T, N), g(gal_start, K, M);
    // column ranges over the gallery's blocks, cut only at blocks that do not take a segment over from their predecessor (the sums of an
    // identity that spans blocks are carried from tile to tile inside a range).  Every (query row group, range) workgroup has work: ~24
    // pieces per workgroup slot (3 resident per CU) as in K10, a piece at least 16 column blocks (its query blocks are loaded once per piece)
    const int row_groups = (q.nb + 3) / 4;
    // (a range is addressed with 32-bit byte offsets: at most 2^20 rows, hence the floor on the number of ranges)
    const std::vector<int> range_b0 = cut_ranges(g, (24 * 3 * c->n_cu + row_groups - 1) / row_groups, (g.nb >> 15) + 1);
    const int n_ranges = (int)range_b0.size() - 1;
    for (int k = 0; k < n_ranges; ++k)
        PVF_REQUIRE(range_b0[k + 1] - range_b0[k] <= (1 << 16), "identify: an identity of more than a million rows (32-bit byte offsets)");
    PVF_REQUIRE(n_ranges <= 65535, "identify: too many column ranges");
    // ---- device buffers: tables in s_clu0, D in s_clu1
    ScratchLayout lay;
    const size_t n_big = std::max<size_t>(q.big_group.size(), 1);
    const auto sX = lay.take<double>((size_t)N * DIM), sG = lay.take<double>((size_t)M * DIM), sNX = lay.take<double>(N), sNG = lay.take<double>(M);
    const auto sQS = lay.take<int>(N), sQG = lay.take<int>((size_t)q.nb * 16), sQP = lay.take<int>((size_t)q.nb * 16);
    const auto sGS = lay.take<int>(M), sGI = lay.take<int>((size_t)g.nb * 16), sGC = lay.take<int>(g.nb);
    const auto sP = lay.take<double>((size_t)std::max(q.n_parts, 1) * K);
    const auto sRow = lay.take<int32_t>(T + 1), sGal = lay.take<int32_t>(K + 1), sRange = lay.take<int>(n_ranges + 1);
    const auto sBigG = lay.take<int>(n_big), sBigC0 = lay.take<int>(n_big), sBigNc = lay.take<int>(n_big), sIsBig = lay.take<int>(T);
    ScratchLayout layD;
    const auto sD = layD.take<double>((size_t)T * K);
    c->s_clu0.ensure(lay.bytes());
    c->s_clu1.ensure(layD.bytes());
    double* dX = sX.in(c->s_clu0); double* dG = sG.in(c->s_clu0); double* dNX = sNX.in(c->s_clu0); double* dNG = sNG.in(c->s_clu0);
    int* dQS = sQS.in(c->s_clu0); int* dQG = sQG.in(c->s_clu0); int* dQP = sQP.in(c->s_clu0);
    int* dGS = sGS.in(c->s_clu0); int* dGI = sGI.in(c->s_clu0); int* dGC = sGC.in(c->s_clu0);
    double* dP = sP.in(c->s_clu0);
    int32_t* dRow = sRow.in(c->s_clu0); int32_t* dGal = sGal.in(c->s_clu0); int* dRange = sRange.in(c->s_clu0);
    int* dBigG = sBigG.in(c->s_clu0); int* dBigC0 = sBigC0.in(c->s_clu0); int* dBigNc = sBigNc.in(c->s_clu0); int* dIsBig = sIsBig.in(c->s_clu0);
    double* dD = sD.in(c->s_clu1);
    auto up = [&](void* d, const void* h, size_t bytes) { if (bytes) HIP_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream)); };
    up(dX, X, (size_t)N * DIM * 8); up(dG, G, (size_t)M * DIM * 8);
    up(dQS, q.segidx.data(), (size_t)N * 4); up(dQG, q.seg_group.data(), (size_t)q.nb * 16 * 4); up(dQP, q.seg_part.data(), (size_t)q.nb * 16 * 4);
    up(dGS, g.segidx.data(), (size_t)M * 4); up(dGI, g.seg_group.data(), (size_t)g.nb * 16 * 4); up(dGC, g.blk_cont.data(), (size_t)g.nb * 4);
    up(dRow, row_start, (size_t)(T + 1) * 4); up(dGal, gal_start, (size_t)(K + 1) * 4); up(dRange, range_b0.data(), (size_t)(n_ranges + 1) * 4);
    up(dIsBig, q.is_big.data(), (size_t)T * 4);
    up(dBigG, q.big_group.data(), q.big_group.size() * 4); up(dBigC0, q.big_c0.data(), q.big_c0.size() * 4); up(dBigNc, q.big_nc.data(), q.big_nc.size() * 4);
    // the staging buffers above are std::vectors: the copies must have run before they go out of scope
    HIP_CHECK(hipStreamSynchronize(c->stream));
    {
        ProfScope ps(c, "identify");
        hipLaunchKernelGGL(id_row_norms_k, dim3((N + 255) / 256), dim3(256), 0, c->stream, dX, N, DIM, dNX);
        hipLaunchKernelGGL(id_row_norms_k, dim3((M + 255) / 256), dim3(256), 0, c->stream, dG, M, DIM, dNG);
        CtArgs a;
        a.X = dX; a.G = dG; a.nrm_x = dNX; a.nrm_g = dNG; a.N = N; a.M = M; a.K = K;
        a.q_segidx = dQS; a.q_seg_group = dQG; a.q_seg_part = dQP; a.g_segidx = dGS; a.g_seg_id = dGI; a.g_blk_cont = dGC;
        a.range_b0 = dRange; a.D = dD; a.P = dP; a.nbq = q.nb; a.metric = metric;
        hipLaunchKernelGGL(cross_tiles_k, dim3(row_groups, n_ranges), dim3(256), 0, c->stream, a);
        // (grid.y is a group index: rows of D in slices of 65535)
        for (int t0 = 0; t0 < T; t0 += 65535) {
            const int nt = std::min(65535, T - t0);
            hipLaunchKernelGGL(cross_norm_k, dim3((K + 255) / 256, nt), dim3(256), 0, c->stream, dD + (size_t)t0 * K, dRow + t0, dGal, dIsBig + t0, K);
        }
        const int nbig = (int)q.big_group.size();
        for (int k0 = 0; k0 < nbig; k0 += 65535) {
            const int n = std::min(65535, nbig - k0);
            hipLaunchKernelGGL(cross_chunks_k, dim3((K + 255) / 256, n), dim3(256), 0, c->stream, dP, dBigG + k0, dBigC0 + k0, dBigNc + k0, dRow, dGal, K, dD);
        }
    }
    HIP_CHECK(hipGetLastError());
    if (D_host) HIP_CHECK(hipMemcpyAsync(D_host, dD, (size_t)T * K * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    return dD;
}

// the decision on a T x K matrix: in HBM (d_D, what gallery_mean_dist_dev returned) or on the host (D_host, uploaded into s_clu1)
void identify_pick_dev(Ctx* c, const double* d_D, const double* D_host, int T, int K, double threshold, int32_t* best, double* best_dist,
                       int32_t* second, double* second_dist)
{
    if (!d_D) {
        ScratchLayout layD;
        const auto sD = layD.take<double>((size_t)T * K);
        c->s_clu1.ensure(layD.bytes());
        double* dD = sD.in(c->s_clu1);
        HIP_CHECK(hipMemcpyAsync(dD, D_host, (size_t)T * K * 8, hipMemcpyHostToDevice, c->stream));
        d_D = dD;
    }
    ScratchLayout lay;
    const auto sBD = lay.take<double>(T), sSD = lay.take<double>(T);
    const auto sB = lay.take<int32_t>(T), sS = lay.take<int32_t>(T);
    c->s_misc.ensure(lay.bytes());
    double* dBD = sBD.in(c->s_misc); double* dSD = sSD.in(c->s_misc); int32_t* dB = sB.in(c->s_misc); int32_t* dS = sS.in(c->s_misc);
    {
        ProfScope ps(c, "identify");
        hipLaunchKernelGGL(identify_pick_k, dim3((T + 3) / 4), dim3(256), 0, c->stream, d_D, T, K, threshold, dB, dBD, dS, dSD);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(best, dB, (size_t)T * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(best_dist, dBD, (size_t)T * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(second, dS, (size_t)T * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(second_dist, dSD, (size_t)T * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
