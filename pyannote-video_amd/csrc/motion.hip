// motion.hip -- the `motion` verb's device side (MOTION.md): a robust similarity fitted to the dense flow of every consecutive pair of frames.
//   motion_fit_k   one workgroup per pair: the flow [h][w][2] is quantised to 1/64 pixel, a least-squares similarity
//                  (u^ = TX + A X - B Y, v^ = TY + B X + A Y, parameters scaled by 2^16) is fitted over the valid pixels, and three more
//                  times over the pixels whose residual lies within twice the mean residual of the fit before.
// The flow is the caller's own (pvf_flow_motion) or what shot_pair_k left in device scratch (pvf_shot_motion, through shot.hip).  There is
// no floating point behind the quantiser and no atomic: the sums are int64, so their order is free and the row is the same on every run
// (tests/motion_ref.py restates it; the kernel is held to it bit for bit).
#include "pvf_internal.h"
#include <algorithm>

constexpr int MO_WORDS = PVF_MOTION_ROW_WORDS;   // int64 words of a row
constexpr int MO_ROUNDS = PVF_MOTION_ROUNDS;
constexpr int64_t MO_TAU_MIN = PVF_MOTION_TAU_MIN;
constexpr int MO_Q_MAX = 1 << 20;                // |u|, |v| at most, in 1/64 pixel
constexpr int MO_SUMS = 8;
static_assert(MO_WORDS == 10 && MO_ROUNDS == 4 && MO_TAU_MIN == (16 << 16), "the row and the rounds of MOTION.md");

__device__ __forceinline__ int64_t wave_sum64(int64_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// floor(a / b) for b > 0
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b)
{
    int64_t q = a / b;
    if (a % b < 0) --q;
    return q;
}

// floor(num 2^16 / den) for den > 0 without forming num 2^16: quotient and remainder first (MOTION.md "Bounds": rem 2^16 < den 2^16 < 2^59)
__device__ __forceinline__ int64_t floor_div_16(int64_t num, int64_t den)
{
    const int64_t q = floor_div(num, den), rem = num - q * den;
    return q * 65536 + (rem * 65536) / den;
}

struct MoModel { int64_t tx, ty, a, b; };

// a pixel of the pair: valid when both components are finite; u, v = rint(clip(64 f, -2^20, 2^20)), float32 product, half to even
__device__ __forceinline__ bool mo_pixel(const float2* __restrict__ flow, int i, int& u, int& v)
{
    const float2 f = flow[i];                    // one 8-byte load
    if (!(isfinite(f.x) && isfinite(f.y))) return false;
    u = (int)rintf(fminf(fmaxf(f.x * 64.f, -(float)MO_Q_MAX), (float)MO_Q_MAX));
    v = (int)rintf(fminf(fmaxf(f.y * 64.f, -(float)MO_Q_MAX), (float)MO_Q_MAX));
    return true;
}

__device__ __forceinline__ void mo_residual(const MoModel& m, int X, int Y, int u, int v, int64_t& ru, int64_t& rv)
{
    const int64_t du = ((int64_t)u << 16) - (m.tx + m.a * X - m.b * Y), dv = ((int64_t)v << 16) - (m.ty + m.b * X + m.a * Y);
    ru = du < 0 ? -du : du;
    rv = dv < 0 ? -dv : dv;
}

// grid (n_pairs), 256 lanes.  flow [n_pairs][h][w][2] floats: pixel i < P = h w of pair p is the float2 at flow + 2 (p P + i), nothing else is
// read; rows [n_pairs][10] int64: lane 0 writes the ten words of row p.  dfd (device, or null): word 7 is the bits of dfd[p].
// Round k makes two passes over the pair's pixels, lane l taking pixels l, l + 256, ...: the eight sums of the fit over S_k, then the
// residual sum of the new model over S_k (with, in round 0, the sum of |u| + |v|).  S_k (k > 0) is not stored: a pixel belongs to it when its
// residual under the model of round k - 1 is within that round's tau, which both passes recompute.  The sums go through the wave, then
// through s_part; lane 0 solves and hands the model to the others through s_bc.  Every sum stays below 2^63 (MOTION.md "Bounds").
__global__ void __launch_bounds__(256) motion_fit_k(const float* __restrict__ flow_all, int h, int w, const double* __restrict__ dfd,
                                                    int64_t* __restrict__ rows)
{
    __shared__ int64_t s_part[4][MO_SUMS];
    __shared__ int64_t s_bc[6];                  // tx, ty, a, b, tau, stop
    const int tid = threadIdx.x, pair = blockIdx.x, P = h * w;
    const float2* __restrict__ flow = reinterpret_cast<const float2*>(flow_all) + (size_t)pair * P;
    MoModel prev = {0, 0, 0, 0}, cur = {0, 0, 0, 0};
    int64_t tau_prev = 0, tau = 0;
    int64_t n_valid = 0, n_in = 0, m_res = 0, mag = 0, n_fit = 0;       // lane 0's
    for (int k = 0; k < MO_ROUNDS; ++k) {
        // ---- the sums of the fit over S_k
        int64_t acc[MO_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = tid; i < P; i += 256) {
            int u, v;
            if (!mo_pixel(flow, i, u, v)) continue;
            const int y = i / w, x = i - y * w, X = 2 * x - (w - 1), Y = 2 * y - (h - 1);
            if (k > 0) {
                int64_t ru, rv;
                mo_residual(cur, X, Y, u, v, ru, rv);
                if ((ru > rv ? ru : rv) > tau) continue;
            }
            acc[0] += 1; acc[1] += X; acc[2] += Y; acc[3] += X * X + Y * Y;
            acc[4] += u; acc[5] += v;
            acc[6] += (int64_t)X * u + (int64_t)Y * v;
            acc[7] += (int64_t)X * v - (int64_t)Y * u;
        }
#pragma unroll
        for (int j = 0; j < MO_SUMS; ++j) acc[j] = wave_sum64(acc[j]);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int j = 0; j < MO_SUMS; ++j) s_part[tid >> 6][j] = acc[j];
        }
        __syncthreads();
        if (tid == 0) {
            int64_t s[MO_SUMS];
#pragma unroll
            for (int j = 0; j < MO_SUMS; ++j) s[j] = s_part[0][j] + s_part[1][j] + s_part[2][j] + s_part[3][j];
            const int64_t n = s[0], SX = s[1], SY = s[2], ZZ = s[3], Su = s[4], Sv = s[5], Pp = s[6], Qq = s[7];
            if (k == 0) n_valid = n;
            const bool stop = k == 0 ? n == 0 : n < 3;               // no valid pixel at all, or too few left: the model before stands
            if (!stop) {
                const int64_t den = n * ZZ - SX * SX - SY * SY;
                MoModel f = {0, 0, 0, 0};
                if (den != 0) {
                    f.a = floor_div_16(n * Pp - (SX * Su + SY * Sv), den);
                    f.b = floor_div_16(n * Qq - (SX * Sv - SY * Su), den);
                }
                f.tx = floor_div(Su * 65536 - f.a * SX + f.b * SY + (n >> 1), n);
                f.ty = floor_div(Sv * 65536 - f.b * SX - f.a * SY + (n >> 1), n);
                s_bc[0] = f.tx; s_bc[1] = f.ty; s_bc[2] = f.a; s_bc[3] = f.b;
                n_fit = n;
            }
            s_bc[5] = stop;
        }
        __syncthreads();
        if (s_bc[5]) break;                      // (uniform over the block)
        prev = cur; tau_prev = tau;
        cur.tx = s_bc[0]; cur.ty = s_bc[1]; cur.a = s_bc[2]; cur.b = s_bc[3];
        // ---- the residual of the new model over S_k
        int64_t res = 0, absum = 0;
        for (int i = tid; i < P; i += 256) {
            int u, v;
            if (!mo_pixel(flow, i, u, v)) continue;
            const int y = i / w, x = i - y * w, X = 2 * x - (w - 1), Y = 2 * y - (h - 1);
            int64_t ru, rv;
            if (k > 0) {
                mo_residual(prev, X, Y, u, v, ru, rv);
                if ((ru > rv ? ru : rv) > tau_prev) continue;
            } else {
                absum += (u < 0 ? -u : u) + (v < 0 ? -v : v);
            }
            mo_residual(cur, X, Y, u, v, ru, rv);
            res += ru + rv;
        }
        res = wave_sum64(res);
        if (k == 0) absum = wave_sum64(absum);
        if ((tid & 63) == 0) { s_part[tid >> 6][0] = res; s_part[tid >> 6][1] = absum; }
        __syncthreads();
        if (tid == 0) {
            const int64_t sum = s_part[0][0] + s_part[1][0] + s_part[2][0] + s_part[3][0];
            if (k == 0) mag = s_part[0][1] + s_part[1][1] + s_part[2][1] + s_part[3][1];
            n_in = n_fit;
            m_res = sum / (2 * n_fit);           // (both are >= 0)
            s_bc[4] = 2 * m_res > MO_TAU_MIN ? 2 * m_res : MO_TAU_MIN;
        }
        __syncthreads();
        tau = s_bc[4];
    }
    if (tid == 0) {
        int64_t* row = rows + (size_t)pair * MO_WORDS;
        row[0] = n_valid | n_in << 32;
        row[1] = cur.tx; row[2] = cur.ty; row[3] = cur.a; row[4] = cur.b;
        row[5] = m_res; row[6] = mag;
        row[7] = dfd ? __double_as_longlong(dfd[pair]) : 0;
        row[8] = 0;
        row[9] = (int64_t)w | (int64_t)h << 16;
    }
}

static void motion_check_size(const std::string& w, int width, int height)
{
    PVF_REQUIRE(width >= PVF_MOTION_MIN_SIDE && width <= PVF_MOTION_MAX_SIDE && height >= PVF_MOTION_MIN_SIDE && height <= PVF_MOTION_MAX_SIDE,
                w + ": a side outside PVF_MOTION_MIN_SIDE .. PVF_MOTION_MAX_SIDE");
    PVF_REQUIRE((int64_t)width * height <= PVF_MOTION_MAX_PIXELS, w + ": more than PVF_MOTION_MAX_PIXELS pixels");
}

// the launch alone, on c->stream: d_flow [n_pairs][h][w][2], d_dfd [n_pairs] or null, d_rows [n_pairs][10], all on the device
void motion_fit_device(Ctx* c, const float* d_flow, int n_pairs, int h, int w, const double* d_dfd, int64_t* d_rows)
{
    ProfScope prof(c, "motion");
    hipLaunchKernelGGL(motion_fit_k, dim3((unsigned)n_pairs), dim3(256), 0, c->stream, d_flow, h, w, d_dfd, d_rows);
    HIP_CHECK(hipGetLastError());
}

static void flow_motion_check(const float* flow, int n_pairs, int h, int w, const int64_t* rows)
{
    const std::string who("pvf_flow_motion");
    PVF_REQUIRE(n_pairs >= 0, who + ": a negative count");
    motion_check_size(who, w, h);
    PVF_REQUIRE(n_pairs == 0 || (flow && rows), who + ": null flow or rows");
}

static void flow_motion_run(Ctx* c, const float* flow, int n_pairs, int h, int w, int64_t* rows)
{
    if (n_pairs == 0) return;
    const size_t P = (size_t)h * w;
    const int round = std::min(n_pairs, PVF_MOTION_ROUND_PAIRS);
    ScratchLayout lay;
    const auto sFlow = lay.take<float>((size_t)round * P * 2);
    const auto sRows = lay.take<int64_t>((size_t)round * MO_WORDS);
    c->s_act0.ensure(lay.bytes());
    float* d_flow = sFlow.in(c->s_act0);
    int64_t* d_rows = sRows.in(c->s_act0);
    for (int p0 = 0; p0 < n_pairs; p0 += round) {
        const int m = std::min(round, n_pairs - p0);
        HIP_CHECK(hipMemcpyAsync(d_flow, flow + (size_t)p0 * P * 2, (size_t)m * P * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        motion_fit_device(c, d_flow, m, h, w, nullptr, d_rows);
        HIP_CHECK(hipMemcpyAsync(rows + (size_t)p0 * MO_WORDS, d_rows, (size_t)m * MO_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
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

extern "C" int32_t pvf_flow_motion(pvf_handle h, const float* flow, int32_t n_pairs, int32_t height, int32_t width, int64_t* rows)
{
    API_BEGIN
    flow_motion_check(flow, n_pairs, height, width, rows);
    ENTER(c, h);
    flow_motion_run(c, flow, n_pairs, height, width, rows);
    API_END
}

extern "C" int32_t pvf_shot_motion(pvf_handle h, const pvf_handle* frames, int32_t n, int32_t width, int32_t height, const float* tables,
                                   int64_t* rows, double* dfd)
{
    API_BEGIN
    const std::string who("pvf_shot_motion");
    PVF_REQUIRE(n >= 0, who + ": a negative count");
    motion_check_size(who, width, height);
    if (n <= 1) return 0;
    PVF_REQUIRE(frames && tables && rows, who + ": null frames, tables or rows");
    ENTER(c, h);
    std::vector<Frame> f(n);
    for (int i = 0; i < n; ++i) {
        f[i] = c->frame(frames[i]);
        PVF_REQUIRE(f[i].h == f[0].h && f[i].w == f[0].w, who + ": frames of different sizes");
    }
    shot_run(c, f, width, height, tables, dfd, nullptr, nullptr, rows);
    API_END
}
