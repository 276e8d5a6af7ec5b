// cast.hip -- WHO the people of many films are: rank-order clustering on an exact k-NN graph (pvf_cast; CAST.md states the rules in
// integers, tests/cast_ref.py restates them and the GPU tests compare bit for bit).
//
//   the lists   the table is uploaded and quantised ONCE (search_quant_k: float32 [N16][128] + |row|^2, zero rows past N) and stays in HBM.
//               Query batches and table chunks are row ranges of that one buffer: search_tiles_k and search_merge_k (search.hip, unchanged)
//               run on them and write each batch's lists into the device array L [N][k] + counts.  A row is excluded from the lists of
//               its own group; a row without a group gets a group of its own (N + row), so it never meets itself.  No list crosses PCIe.
//   cast_prep_k / cast_first_k   the effective groups, the smallest row of every group, and the forest the group edges leave: a row
//               points at the smallest row of its group.
//   cast_links_k   one wave per node a, four per workgroup.  L_a lies in LDS beside a copy sorted by row index that carries the ranks
//               (key = row << 8 | slot: rows are below 2^24, slots below 256).  For every slot the wave reads L_b with coalesced int32
//               loads (the next list is requested before the current one is used) and looks every entry up in the sorted copy: one pass
//               gives O_b(a), the common rows inside a's prefix and the common rows inside b's prefix, hence both miss counts, r and the
//               decision m * den <= num * r in int64.  No atomics.  One byte per (a, slot).
//   cast_hook_k / cast_jump_k   components: for every link the larger of the two parents is hooked under the smaller (atomicMin), then the
//               forest is flattened by pointer jumping (parent = parent of parent, until a device flag stays clear); repeated until a hook
//               pass changes nothing.  parent[x] <= x always, so a root is the smallest row of its tree and the flat forest IS the labels.
// Device memory: the table (512 B a row) + lists (4 k B a row) + link bytes + O(batch k ranges) of selection arena.
#include "pvf_internal.h"
#include <algorithm>
#include <cstdlib>

static constexpr int CS_DIM = 128, CS_MAX_K = 256, CS_DEFAULT_QBLOCK = 4096, CS_UPLOAD_ROWS = 1 << 16;
static constexpr int64_t CS_MAX_N = (int64_t)1 << 24, CS_MAX_FRAC = (int64_t)1 << 20;
static constexpr unsigned long long CS_NONE = ~0ull;

namespace {
__device__ __forceinline__ void cs_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
} // namespace

// eg[i]: the exclusion group of row i (its group, or N + i); first[g]: the smallest row of group g (INT_MAX: nobody), by atomicMin
__global__ void __launch_bounds__(256) cast_prep_k(const int* __restrict__ group, int N, int* __restrict__ eg, int* __restrict__ first)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int g = group ? group[i] : -1;
    eg[i] = g >= 0 ? g : N + i;
    if (g >= 0) atomicMin(&first[g], i);
}

// the forest of the group edges: a row points at the smallest row of its group (which points at itself)
__global__ void __launch_bounds__(256) cast_first_k(const int* __restrict__ group, int N, const int* __restrict__ first, int* __restrict__ parent)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int g = group ? group[i] : -1;
    parent[i] = g >= 0 ? first[g] : i;
}

// dynamic LDS: 4 waves x (k2 + k2) x 4 bytes, k2 = k rounded up to a power of two, at least 64
__global__ void __launch_bounds__(256) cast_links_k(const int* __restrict__ L, const int* __restrict__ cnt, int N, int k, int k2, long long num,
                                                    long long den, unsigned char* __restrict__ linked, int* __restrict__ m_out, int* __restrict__ r_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cs_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a = blockIdx.x * 4 + wave;
    if (a >= N) return;                                   // (a whole wave; no workgroup barrier below)
    int* la = reinterpret_cast<int*>(cs_dyn) + (size_t)wave * 2 * k2;
    unsigned* sa = reinterpret_cast<unsigned*>(la + k2);
    const int ca = cnt[a];
    const int* La = L + (size_t)a * k;
    for (int s = lane; s < k2; s += 64) {
        const int z = s < ca ? La[s] : -1;
        la[s] = z;
        sa[s] = s < ca ? (((unsigned)z << 8) | (unsigned)s) : 0xffffffffu;
    }
    cs_wave_sync();
    for (int size = 2; size <= k2; size <<= 1) {          // bitonic sort, ascending: the ca entries first (padding is the largest key)
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < k2 / 2; t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                const bool up = (i & size) == 0;
                const unsigned x = sa[i], y = sa[l];
                if ((x > y) == up) { sa[i] = y; sa[l] = x; }
            }
            cs_wave_sync();
        }
    }
    const int ni = (k + 63) >> 6;                         // 64-entry pieces of a list
    int zn[4] = {-1, -1, -1, -1};
    int cbn = 0;
    auto request = [&](int s) {                           // L_b of slot s into zn / cbn (uniform s < ca)
        const int b = la[s];
        cbn = cnt[b];
        const int* Lb = L + (size_t)b * k;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = lane + 64 * i;
            zn[i] = (i < ni && j < cbn) ? Lb[j] : -1;
        }
    };
    if (ca > 0) request(0);
    for (int s = 0; s < ca; ++s) {
        int z[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = zn[i];
        const int cb = cbn;
        if (s + 1 < ca) request(s + 1);
        const int p = s + 1;                              // O_a(b)
        int ob = 0, common_a = 0;
        unsigned long long in_a[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < ni && 64 * i < cb) {                  // (uniform)
                const bool valid = z[i] >= 0;
                const unsigned t = (unsigned)z[i] << 8;
                int lo = 0;
                for (int step = k2 >> 1; step > 0; step >>= 1)
                    if (sa[lo + step - 1] < t) lo += step;
                const unsigned key = sa[lo];
                const bool hit = valid && lo < ca && (key >> 8) == (unsigned)z[i];
                const int rank = (int)(key & 255u) + 1;   // O_a(z)
                in_a[i] = __builtin_amdgcn_ballot_w64(hit);
                common_a += __builtin_popcountll(__builtin_amdgcn_ballot_w64(hit && rank < p));
                const unsigned long long me = __builtin_amdgcn_ballot_w64(valid && z[i] == a);
                if (me) ob = 64 * i + __builtin_ctzll(me) + 1;      // O_b(a)
            }
        }
        const int pb = ob ? ob - 1 : cb;                  // the entries of L_b ahead of a, or all of it
        int common_b = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = pb - 64 * i;                    // lanes of this piece inside the prefix
            if (n > 0) common_b += __builtin_popcountll(n >= 64 ? in_a[i] : (in_a[i] & ((1ull << n) - 1ull)));
        }
        const int m = (p - 1 - common_a) + (pb - common_b);
        const int r = ob ? min(p, ob) : p;
        if (lane == 0) {
            const size_t o = (size_t)a * k + s;
            linked[o] = ((long long)m * den <= num * (long long)r) ? 1 : 0;
            if (m_out) { m_out[o] = m; r_out[o] = r; }
        }
    }
    for (int s = ca + lane; s < k; s += 64) {
        const size_t o = (size_t)a * k + s;
        linked[o] = 0;
        if (m_out) { m_out[o] = -1; r_out[o] = -1; }
    }
}

// one thread per (a, slot): a link hooks the larger parent under the smaller.  The forest is flat when this runs, so the parents are
// roots; a value another thread lowers meanwhile is still a row of the same component, below the row it replaces.
__global__ void __launch_bounds__(256) cast_hook_k(const int* __restrict__ L, const unsigned char* __restrict__ linked, long long n_slots, int k,
                                                   int* __restrict__ parent, int* __restrict__ changed)
{
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_slots || !linked[o]) return;
    const int a = (int)(o / k), b = L[o];
    const int pa = parent[a], pb = parent[b];
    if (pa == pb) return;
    atomicMin(&parent[max(pa, pb)], min(pa, pb));
    *changed = 1;
}

// pointer jumping: every pass halves the depth of the forest
__global__ void __launch_bounds__(256) cast_jump_k(int N, int* __restrict__ parent, int* __restrict__ changed)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int p = parent[i], pp = parent[p];
    if (pp != p) { parent[i] = pp; *changed = 1; }
}

namespace {
struct CastPlan { int64_t qblock, n_batches, dev_bytes; SrPlan sr; };

void cast_check(int64_t N, int dim, int k, int64_t max_d2, int64_t num, int64_t den, const int32_t* group)
{
    PVF_REQUIRE(dim == 128, "pvf_cast: dim must be 128 (the descriptor of the embedder; the matrix-core kernel is built for it)");
    PVF_REQUIRE(N >= 1 && N <= CS_MAX_N, "pvf_cast: N must lie in 1 .. 2^24");
    PVF_REQUIRE(k >= 1 && k <= CS_MAX_K, "pvf_cast: k must lie in 1 .. 256");
    PVF_REQUIRE(max_d2 >= -1, "pvf_cast: max_d2 must be at least -1 (-1: no cut)");
    PVF_REQUIRE(num >= 0 && num <= CS_MAX_FRAC, "pvf_cast: num must lie in 0 .. 2^20");
    PVF_REQUIRE(den >= 1 && den <= CS_MAX_FRAC, "pvf_cast: den must lie in 1 .. 2^20");
    if (group)
        for (int64_t i = 0; i < N; ++i) PVF_REQUIRE(group[i] < N, "pvf_cast: a group must be negative (none) or below N");
}

int cast_k2(int k)
{
    int k2 = 64;
    while (k2 < k) k2 *= 2;
    return k2;
}

// every device buffer of a call: what lives for the whole call (s_clu0) and what a batch uses (s_clu1)
struct CastLayout {
    ScratchLayout lay, layA;
    ScratchSlot<float> Xf; ScratchSlot<double> NX, Xd;
    ScratchSlot<int> EG, Grp, First, Par, Cnt, L, M, R, Chg, AI, AC;
    ScratchSlot<unsigned char> Lk;
    ScratchSlot<unsigned long long> Flag;
    ScratchSlot<long long> AD, BD;
    CastLayout(int64_t N, int k, int64_t qblock, const SrPlan& sp, bool want_mr)
    {
        const size_t N16 = (size_t)(N + 15) / 16 * 16, up_rows = (size_t)std::min<int64_t>(N, CS_UPLOAD_ROWS), slots = (size_t)N * k;
        Xf = lay.take<float>(N16 * CS_DIM);
        NX = lay.take<double>(N16); Xd = lay.take<double>(up_rows * CS_DIM);
        EG = lay.take<int>(N16); Grp = lay.take<int>(N); First = lay.take<int>(N); Par = lay.take<int>(N); Cnt = lay.take<int>(N);
        L = lay.take<int>(slots);
        M = lay.take<int>(want_mr ? slots : 1); R = lay.take<int>(want_mr ? slots : 1);
        Lk = lay.take<unsigned char>(slots);
        Flag = lay.take<unsigned long long>(2);
        Chg = lay.take<int>(2);
        AD = layA.take<long long>((size_t)sp.arena_entries);
        AI = layA.take<int>((size_t)sp.arena_entries); AC = layA.take<int>((size_t)qblock * sp.n_ranges);
        BD = layA.take<long long>((size_t)qblock * k);
    }
};

// queries per batch (PVF_CAST_QBLOCK, the test switch, read at every call; whole 16-row blocks) and the cut of the table (search_plan)
CastPlan cast_plan(int64_t N, int k, bool debug_links)
{
    CastPlan p;
    int64_t qb = CS_DEFAULT_QBLOCK;
    const char* e = getenv("PVF_CAST_QBLOCK");
    if (e && atoll(e) > 0) qb = std::min<int64_t>(atoll(e), (int64_t)1 << 16);
    qb = (std::min(qb, N) + 15) / 16 * 16;
    p.qblock = qb;
    p.n_batches = (N + qb - 1) / qb;
    p.sr = search_plan_of((int)qb, N, k);
    const CastLayout cl(N, k, qb, p.sr, debug_links);
    p.dev_bytes = (int64_t)(cl.lay.bytes() + cl.layA.bytes());
    return p;
}

struct CastDebug { int32_t* idx = nullptr; int64_t* d2 = nullptr; int32_t* count = nullptr; int32_t* m = nullptr; int32_t* r = nullptr; uint8_t* linked = nullptr; };

int read_flag(Ctx* c, const int* d)
{
    int v = 0;
    HIP_CHECK(hipMemcpyAsync(&v, d, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    return v;
}

void cast_dev(Ctx* c, const double* X, int64_t N64, int k, int64_t max_d2, int64_t num, int64_t den, const int32_t* group, int32_t* labels,
              int32_t* n_components, const CastDebug& dbg, bool lists_only)
{
    const int N = (int)N64, N16 = (N + 15) / 16 * 16;
    const bool want_mr = dbg.m != nullptr;
    const CastPlan pl = cast_plan(N, k, want_mr);
    const SrPlan& sp = pl.sr;
    const int qblock = (int)pl.qblock, kp = (int)sp.kp, n_ranges = (int)sp.n_ranges, k2 = cast_k2(k);
    PVF_REQUIRE(n_ranges <= 65535, "pvf_cast: too many column ranges");
    const size_t chunk = (size_t)sp.chunk_rows, up_rows = (size_t)std::min<int64_t>(N, CS_UPLOAD_ROWS), slots = (size_t)N * k;
    const CastLayout cl(N, k, qblock, sp, want_mr);
    c->s_clu0.ensure(cl.lay.bytes());
    c->s_clu1.ensure(cl.layA.bytes());
    float* dXf = cl.Xf.in(c->s_clu0); double* dNX = cl.NX.in(c->s_clu0); double* dXd = cl.Xd.in(c->s_clu0);
    int* dEG = cl.EG.in(c->s_clu0); int* dGrp = cl.Grp.in(c->s_clu0); int* dFirst = cl.First.in(c->s_clu0); int* dPar = cl.Par.in(c->s_clu0);
    int* dCnt = cl.Cnt.in(c->s_clu0); int* dL = cl.L.in(c->s_clu0); int* dM = cl.M.in(c->s_clu0); int* dR = cl.R.in(c->s_clu0);
    unsigned char* dLk = cl.Lk.in(c->s_clu0);
    unsigned long long* dFlag = cl.Flag.in(c->s_clu0);
    int* dChg = cl.Chg.in(c->s_clu0);
    long long* dAD = cl.AD.in(c->s_clu1); int* dAI = cl.AI.in(c->s_clu1); int* dAC = cl.AC.in(c->s_clu1); long long* dBD = cl.BD.in(c->s_clu1);
    // ---- the table: uploaded in pieces, quantised into its place, refused as a whole before anything else runs
    HIP_CHECK(hipMemsetAsync(dFlag, 0xff, 16, c->stream));
    if (N16 > N) {
        HIP_CHECK(hipMemsetAsync(dXf + (size_t)N * CS_DIM, 0, (size_t)(N16 - N) * CS_DIM * 4, c->stream));
        HIP_CHECK(hipMemsetAsync(dNX + N, 0, (size_t)(N16 - N) * 8, c->stream));
        HIP_CHECK(hipMemsetAsync(dEG + N, 0xff, (size_t)(N16 - N) * 4, c->stream));
    }
    for (size_t r0 = 0; r0 < (size_t)N; r0 += up_rows) {
        const int n = (int)std::min(up_rows, (size_t)N - r0);
        HIP_CHECK(hipMemcpyAsync(dXd, X + r0 * CS_DIM, (size_t)n * CS_DIM * 8, hipMemcpyHostToDevice, c->stream));
        ProfScope ps(c, "cast_quant");
        search_quant_launch(c, dXd, n, (long long)r0, dXf + r0 * CS_DIM, dNX + r0, dFlag + 1);
    }
    HIP_CHECK(hipGetLastError());
    unsigned long long flag[2] = {CS_NONE, CS_NONE};
    HIP_CHECK(hipMemcpyAsync(flag, dFlag, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (flag[1] != CS_NONE) {
        char b[200];
        snprintf(b, sizeof b, "pvf_cast: X[%llu][%d] is not finite or lies beyond 2^20 units of 1e-5 (|v| above about 10.48): refused, nothing is clamped",
                 flag[1] / CS_DIM, (int)(flag[1] % CS_DIM));
        throw PvfError(b);
    }
    // ---- groups: the exclusion group of every row, and the forest the group edges leave
    if (group) HIP_CHECK(hipMemcpyAsync(dGrp, group, (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemsetAsync(dFirst, 0x7f, (size_t)N * 4, c->stream));
    {
        ProfScope ps(c, "cast_cc");
        hipLaunchKernelGGL(cast_prep_k, dim3((N + 255) / 256), dim3(256), 0, c->stream, group ? dGrp : nullptr, N, dEG, dFirst);
        hipLaunchKernelGGL(cast_first_k, dim3((N + 255) / 256), dim3(256), 0, c->stream, group ? dGrp : nullptr, N, dFirst, dPar);
    }
    // ---- the lists: query batches x table chunks, both row ranges of the resident table
    SrArgs a;
    a.range_blocks = (int)sp.range_blocks; a.n_ranges = n_ranges; a.k = k; a.kp = kp;
    a.cut = (max_d2 < 0) ? -1.0 : (double)std::min<int64_t>(max_d2, (int64_t)1 << 50);
    a.a_d2 = dAD; a.a_idx = dAI; a.a_cnt = dAC; a.flag = dFlag;
    for (int q0 = 0; q0 < N; q0 += qblock) {
        const int nq = std::min(qblock, N - q0);
        a.Qf = dXf + (size_t)q0 * CS_DIM; a.nq = dNX + q0; a.qgrp = dEG + q0; a.Q = nq; a.nbq = (nq + 15) / 16;
        HIP_CHECK(hipMemsetAsync(dAC, 0, (size_t)qblock * n_ranges * 4, c->stream));
        {
            ProfScope ps(c, "cast_lists");
            for (size_t r0 = 0; r0 < (size_t)N; r0 += chunk) {
                a.Xf = dXf + r0 * CS_DIM; a.nx = dNX + r0; a.rgrp = dEG + r0;
                a.n = (int)std::min(chunk, (size_t)N - r0); a.row0 = (int)r0;
                search_tiles_launch(c, a);
            }
            search_merge_launch(c, a, dL + (size_t)q0 * k, dBD, dCnt + q0);
        }
        HIP_CHECK(hipGetLastError());
        if (dbg.d2) HIP_CHECK(hipMemcpyAsync(dbg.d2 + (size_t)q0 * k, dBD, (size_t)nq * k * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (dbg.idx) {
        HIP_CHECK(hipMemcpyAsync(dbg.idx, dL, slots * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipMemcpyAsync(dbg.count, dCnt, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (lists_only) { HIP_CHECK(hipStreamSynchronize(c->stream)); return; }
    // ---- the links
    {
        ProfScope ps(c, "cast_links");
        hipLaunchKernelGGL(cast_links_k, dim3((N + 3) / 4), dim3(256), (size_t)4 * 2 * k2 * 4, c->stream, dL, dCnt, N, k, k2, (long long)num, (long long)den,
                           dLk, want_mr ? dM : nullptr, want_mr ? dR : nullptr);
    }
    HIP_CHECK(hipGetLastError());
    if (want_mr) {
        HIP_CHECK(hipMemcpyAsync(dbg.m, dM, slots * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipMemcpyAsync(dbg.r, dR, slots * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipMemcpyAsync(dbg.linked, dLk, slots, hipMemcpyDeviceToHost, c->stream));
    }
    // ---- the components
    if (labels) {
        const unsigned hook_blocks = (unsigned)((slots + 255) / 256);
        for (;;) {
            HIP_CHECK(hipMemsetAsync(dChg, 0, 8, c->stream));
            {
                ProfScope ps(c, "cast_cc");
                hipLaunchKernelGGL(cast_hook_k, dim3(hook_blocks), dim3(256), 0, c->stream, dL, dLk, (long long)slots, k, dPar, dChg);
            }
            if (!read_flag(c, dChg)) break;
            do {
                HIP_CHECK(hipMemsetAsync(dChg + 1, 0, 4, c->stream));
                ProfScope ps(c, "cast_cc");
                hipLaunchKernelGGL(cast_jump_k, dim3((N + 255) / 256), dim3(256), 0, c->stream, N, dPar, dChg + 1);
            } while (read_flag(c, dChg + 1));
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(labels, dPar, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (labels && n_components) {
        int32_t n = 0;
        for (int i = 0; i < N; ++i) n += labels[i] == i;
        *n_components = n;
    }
}
} // namespace

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

extern "C" int32_t pvf_cast(pvf_handle h, const double* X, int64_t N, int32_t dim, int32_t k, int64_t max_d2, int64_t num, int64_t den,
                            const int32_t* group, int32_t* labels, int32_t* n_components)
{
    API_BEGIN
    cast_check(N, dim, k, max_d2, num, den, group);
    PVF_REQUIRE(X && labels, "pvf_cast: bad arguments");
    ENTER(c, h);
    cast_dev(c, X, N, k, max_d2, num, den, group, labels, n_components, CastDebug(), false);
    API_END
}

extern "C" int32_t pvf_debug_cast_lists(pvf_handle h, const double* X, int64_t N, int32_t dim, int32_t k, int64_t max_d2, const int32_t* group,
                                        int32_t* idx, int64_t* d2, int32_t* count)
{
    API_BEGIN
    cast_check(N, dim, k, max_d2, 0, 1, group);
    PVF_REQUIRE(X && idx && d2 && count, "pvf_debug_cast_lists: bad arguments");
    ENTER(c, h);
    CastDebug dbg;
    dbg.idx = idx; dbg.d2 = d2; dbg.count = count;
    cast_dev(c, X, N, k, max_d2, 0, 1, group, nullptr, nullptr, dbg, true);
    API_END
}

extern "C" int32_t pvf_debug_cast_links(pvf_handle h, const double* X, int64_t N, int32_t dim, int32_t k, int64_t max_d2, int64_t num, int64_t den,
                                        const int32_t* group, int32_t* m, int32_t* r, uint8_t* linked)
{
    API_BEGIN
    cast_check(N, dim, k, max_d2, num, den, group);
    PVF_REQUIRE(X && m && r && linked, "pvf_debug_cast_links: bad arguments");
    ENTER(c, h);
    CastDebug dbg;
    dbg.m = m; dbg.r = r; dbg.linked = linked;
    cast_dev(c, X, N, k, max_d2, num, den, group, nullptr, nullptr, dbg, false);
    API_END
}

// host only: how pvf_cast would cut a call of these sizes
extern "C" int32_t pvf_cast_plan(int64_t N, int32_t k, int64_t out[6])
{
    API_BEGIN
    cast_check(N, 128, k, -1, 0, 1, nullptr);
    PVF_REQUIRE(out, "pvf_cast_plan: bad arguments");
    const CastPlan p = cast_plan(N, k, false);
    out[0] = p.qblock; out[1] = p.n_batches; out[2] = p.sr.chunk_rows; out[3] = p.sr.n_chunks; out[4] = p.sr.n_ranges; out[5] = p.dev_bytes;
    API_END
}
