// jitter.hip -- num_jitters of dlib's compute_face_descriptor(img, shape, num_jitters): J perturbed copies of every aligned 150 x 150 face
// chip, made on the device from the chips in HBM, for the embedder to average (JITTER.md states the semantics; DESIGN.md section 14 the
// kernel, the rounds and the measurement).  The transform of jitter j depends on (seed, j) alone: one table of J sampling jobs serves
// every face of every call, so a descriptor is a function of the face, J and the seed, never of the batch it travelled in.
#include "pvf_internal.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>

#define JIT_S 150                                // side of a chip (the embedder's chip_size)
#define JIT_CHIP_BYTES (JIT_S * JIT_S * 3)       // 67 500: a multiple of 4, not of 16
#define JIT_CHIP_DW (JIT_CHIP_BYTES / 4)         // 16 875 dwords
#define JIT_GROUPS (JIT_S * JIT_S / 4)           // 5 625 runs of 4 consecutive output pixels = 12 bytes = 3 dwords each
#define JIT_LDS_DW (JIT_CHIP_DW + 2)             // + 2: the three aligned dwords around a pixel pair may end 8 bytes past the chip
#define JIT_LDS_BYTES (JIT_LDS_DW * 4)
#define JIT_MIN_RUN 4                            // jitters a block makes from one staged chip, at least (a chip is staged once per block)
static_assert(JIT_CHIP_BYTES % 4 == 0 && (JIT_S * JIT_S) % 4 == 0, "chips are staged, and written, as dwords");
static_assert(JIT_LDS_BYTES == 67508, "one chip and its 8-byte tail");
static_assert(JIT_LDS_BYTES > 64 * 1024 && 2 * JIT_LDS_BYTES <= 160 * 1024, "above the default limit (hipFuncSetAttribute), two blocks per CU");

// ---- the plan (host) -------------------------------------------------------------------------------------------------------------
static uint64_t jit_mix(uint64_t x)
{
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double jit_u(uint64_t seed, int j, int k)
{
    return (double)(jit_mix(seed + (uint64_t)(5 * (int64_t)j + k + 1) * 0x9E3779B97F4A7C15ull) >> 11) * 0x1p-53;
}

struct JitterPlan { ChipDetails d; bool flip; ChipJob job; };

static JitterPlan jitter_plan_one(uint64_t seed, int j)
{
    JitterPlan p;
    const double tx = (-0.02 + jit_u(seed, j, 0) * 0.04) * 144.0;
    const double ty = (-0.02 + jit_u(seed, j, 1) * 0.04) * 144.0;
    const double s = 0.97 + jit_u(seed, j, 2) * (0.99999 - 0.97);
    const double box = 144.0 / s;
    const double angle = (-3.0 + jit_u(seed, j, 3) * 6.0) * M_PI / 180.0;
    p.flip = jit_u(seed, j, 4) > 0.5;
    p.d.l = 75 + tx - box / 2; p.d.t = 75 + ty - box / 2; p.d.r = 75 + tx + box / 2; p.d.b = 75 + ty + box / 2;
    p.d.cs = std::cos(angle); p.d.sn = std::sin(angle);
    p.d.rows = JIT_S; p.d.cols = JIT_S;
    Frame f;                                     // the source of a jitter is a chip: 150 x 150, no pixels needed for the geometry
    f.h = JIT_S; f.w = JIT_S;
    p.job = chip_plan(f, p.d);
    // box <= 144 / 0.97 = 148.46 < 150: the sampled box never covers more source pixels than the chip has, so no pyramid level
    PVF_REQUIRE(!p.job.empty && p.job.levels == 0, "jitter: a plan row needs a pyramid level (box must stay below 150)");
    PVF_REQUIRE(p.job.bx0 >= 0 && p.job.by0 >= 0 && p.job.sw >= 2 && p.job.sh >= 2 && p.job.bx0 + p.job.sw <= JIT_S && p.job.by0 + p.job.sh <= JIT_S,
                "jitter: a plan row's source box leaves the chip");
    return p;
}

void jitter_check_count(const char* who, int J)
{
    PVF_REQUIRE(J >= 0, std::string(who) + ": num_jitters is negative");
    PVF_REQUIRE(J <= 4096, std::string(who) + ": at most 4096 jitters (one forward of the embedder)");
}

// rows of PVF_JITTER_ROW doubles: l t r b cs sn flip m[4] b[2] bx0 by0 sw sh (include/pvface.h)
void jitter_plan_rows(int J, uint64_t seed, double* out)
{
    for (int j = 0; j < J; ++j) {
        const JitterPlan p = jitter_plan_one(seed, j);
        double* o = out + (size_t)j * PVF_JITTER_ROW;
        o[0] = p.d.l; o[1] = p.d.t; o[2] = p.d.r; o[3] = p.d.b; o[4] = p.d.cs; o[5] = p.d.sn; o[6] = p.flip ? 1.0 : 0.0;
        for (int k = 0; k < 4; ++k) o[7 + k] = p.job.m[k];
        o[11] = p.job.b[0]; o[12] = p.job.b[1];
        o[13] = p.job.bx0; o[14] = p.job.by0; o[15] = p.job.sw; o[16] = p.job.sh;
    }
}

// ---- the kernel --------------------------------------------------------------------------------------------------------------------
struct DevJitJob { double m[4], b[2]; int x0, y0, sw, sh, flip, pad_; };

// the six bytes of two neighbouring pixels at byte offset `a` of the staged chip: three aligned dwords, shifted into place
__device__ __forceinline__ void jit_pair(const uint32_t* __restrict__ lds, int a, uint32_t* lo, uint32_t* hi)
{
    const int w = a >> 2;
    const uint32_t sh = (uint32_t)(a & 3);
    const uint32_t w0 = lds[w], w1 = lds[w + 1], w2 = lds[w + 2];
    *lo = __builtin_amdgcn_alignbyte(w1, w0, sh);            // bytes a .. a + 3
    *hi = __builtin_amdgcn_alignbyte(w2, w1, sh);            // bytes a + 4 .. a + 7 (a + 4, a + 5 are read)
}

// One block: one face, a run of its jitters.  The chip goes to LDS once (dword loads: a chip starts on a multiple of 4 bytes, not of
// 16); per jitter a thread makes runs of 4 consecutive output pixels (in the chip's flat pixel order: 150 is no multiple of 4, a run
// may end one row and begin the next) and stores three dwords.  On a mirrored jitter output column c takes extracted column
// 149 - c: the thread walks its source columns backwards and the stores stay ascending.  The arithmetic of a pixel is transform_k's
// (chip.hip), expression for expression, in f64.
// grid (runs per face, n faces), 256 threads, JIT_LDS_BYTES dynamic LDS.  chips [n][150][150][3], out [n][J][150][150][3].
__global__ void __launch_bounds__(256) jitter_k(const uint8_t* __restrict__ chips, const DevJitJob* __restrict__ jobs, int J, int run,
                                                uint8_t* __restrict__ out)
{
    extern __shared__ uint32_t jit_lds[];
    const int face = blockIdx.y;
    const int j0 = blockIdx.x * run, j1 = min(J, j0 + run);
    if (j0 >= J) return;                                     // block-uniform
    const uint32_t* src = reinterpret_cast<const uint32_t*>(chips + (size_t)face * JIT_CHIP_BYTES);
    for (int i = threadIdx.x; i < JIT_LDS_DW; i += 256) jit_lds[i] = i < JIT_CHIP_DW ? src[i] : 0u;
    __syncthreads();
    for (int jj = j0; jj < j1; ++jj) {
        const DevJitJob j = jobs[jj];
        uint32_t* o = reinterpret_cast<uint32_t*>(out + ((size_t)face * J + jj) * JIT_CHIP_BYTES);
        for (int g = threadIdx.x; g < JIT_GROUPS; g += 256) {
            uint32_t px3[4];                                 // the pixels of the run, 0x00BBGGRR
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = 4 * g + q;
                const int r = p / JIT_S, oc = p - r * JIT_S;
                const int c = j.flip ? JIT_S - 1 - oc : oc;
                const double px = j.m[0] * c + j.m[1] * r + j.b[0];
                const double py = j.m[2] * c + j.m[3] * r + j.b[1];
                const double fx = floor(px), fy = floor(py);
                uint32_t v3 = 0;
                if (fx >= 0 && fy >= 0 && fx + 1 < j.sw && fy + 1 < j.sh) {
                    const int left = (int)fx, top = (int)fy;
                    const double lr = px - left, tb = py - top;
                    const int a = ((j.y0 + top) * JIT_S + (j.x0 + left)) * 3;
                    uint32_t t0, t1, b0, b1;                 // t0 = bytes 0 .. 3 of the top pair, t1 = bytes 4 .. 7
                    jit_pair(jit_lds, a, &t0, &t1);
                    jit_pair(jit_lds, a + JIT_S * 3, &b0, &b1);
                    const uint32_t tl3[3] = {t0 & 0xffu, (t0 >> 8) & 0xffu, (t0 >> 16) & 0xffu}, tr3[3] = {t0 >> 24, t1 & 0xffu, (t1 >> 8) & 0xffu};
                    const uint32_t bl3[3] = {b0 & 0xffu, (b0 >> 8) & 0xffu, (b0 >> 16) & 0xffu}, br3[3] = {b0 >> 24, b1 & 0xffu, (b1 >> 8) & 0xffu};
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double tl = tl3[k], tr = tr3[k], bl = bl3[k], br = br3[k];
                        const double v = (1 - tb) * ((1 - lr) * tl + lr * tr) + tb * ((1 - lr) * bl + lr * br);
                        v3 |= (uint32_t)(uint8_t)v << (8 * k);
                    }
                }
                px3[q] = v3;
            }
            o[3 * g] = px3[0] | (px3[1] << 24);
            o[3 * g + 1] = (px3[1] >> 8) | (px3[2] << 16);
            o[3 * g + 2] = (px3[2] >> 16) | (px3[3] << 8);
        }
    }
}

// ---- launches ----------------------------------------------------------------------------------------------------------------------
// chips per round: 4096 (one forward of the embedder), or what PVF_JITTER_CHUNK says, read when the call is made (tests lower it)
int jitter_faces_per_round(int J)
{
    int chunk = 4096;
    const char* e = getenv("PVF_JITTER_CHUNK");
    if (e && atoi(e) > 0) chunk = std::min(chunk, atoi(e));
    return std::max(1, chunk / std::max(J, 1));
}

// the jittered chips of a round live in a buffer of their own (s_trk0 keeps the source chips)
uint8_t* jitter_scratch(Ctx* c, int faces, int J)
{
    ScratchLayout lay;
    const auto sJit = lay.take<uint8_t>((size_t)faces * J * JIT_CHIP_BYTES);
    c->s_jit.ensure(lay.bytes());
    return sJit.in(c->s_jit);
}

// d_chips [n][150][150][3] -> d_out [n][J][150][150][3]; n * J chips must fit d_out.  via_transform: the measurement's other side, the
// same sampling by transform_k over n * J jobs reading the chips in HBM (mirrored jitters come out unmirrored: transform_k has no mirror)
void jitter_chips_dev(Ctx* c, const uint8_t* d_chips, int n, int J, uint64_t seed, uint8_t* d_out, bool via_transform)
{
    PVF_REQUIRE(n > 0 && J > 0 && J <= 4096, "jitter: bad arguments");
    std::vector<JitterPlan> plan(J);
    for (int j = 0; j < J; ++j) plan[j] = jitter_plan_one(seed, j);
    if (via_transform) {
        const size_t nj = (size_t)n * J;
        PVF_REQUIRE(nj <= 65535, "jitter by transform_k: at most 65535 chips per launch");
        ScratchLayout lay;
        const auto sXf = lay.take<DevXfJob>(nj, 16);
        c->s_chip.ensure(lay.bytes());
        DevXfJob* hb = reinterpret_cast<DevXfJob*>(c->stage.take(lay.bytes()));
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < J; ++j) {
                DevXfJob& x = hb[(size_t)i * J + j];
                const ChipJob& q = plan[j].job;
                x.src = d_chips + (size_t)i * JIT_CHIP_BYTES; x.stride_w = JIT_S; x.x0 = q.bx0; x.y0 = q.by0; x.sw = q.sw; x.sh = q.sh;
                memcpy(x.m, q.m, sizeof x.m); memcpy(x.b, q.b, sizeof x.b);
            }
        HIP_CHECK(hipMemcpyAsync(c->s_chip.p, hb, sXf.bytes(), hipMemcpyHostToDevice, c->stream));
        c->stage.sent(c->stream);
        ProfScope ps(c, "jitter_xf");
        transform_launch(c, sXf.in(c->s_chip), (int)nj, JIT_S, JIT_S, d_out);
        HIP_CHECK(hipGetLastError());
        return;
    }
    ScratchLayout lay;
    const auto sJob = lay.take<DevJitJob>(J, 16);
    c->s_chip.ensure(lay.bytes());
    DevJitJob* hb = reinterpret_cast<DevJitJob*>(c->stage.take(lay.bytes()));
    for (int j = 0; j < J; ++j) {
        const ChipJob& q = plan[j].job;
        DevJitJob& x = hb[j];
        memcpy(x.m, q.m, sizeof x.m); memcpy(x.b, q.b, sizeof x.b);
        x.x0 = q.bx0; x.y0 = q.by0; x.sw = q.sw; x.sh = q.sh; x.flip = plan[j].flip ? 1 : 0; x.pad_ = 0;
    }
    HIP_CHECK(hipMemcpyAsync(c->s_chip.p, hb, sJob.bytes(), hipMemcpyHostToDevice, c->stream));
    c->stage.sent(c->stream);
    if (!c->jit_attr_set) {
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(jitter_k), hipFuncAttributeMaxDynamicSharedMemorySize, JIT_LDS_BYTES));
        c->jit_attr_set = true;
    }
    // a block's run: long enough that staging the chip is a small part of its work, short enough that few faces still fill the device
    const int splits = std::min(J, std::max(1, (4 * c->n_cu + n - 1) / n));
    const int run = std::min(J, std::max(JIT_MIN_RUN, (J + splits - 1) / splits));
    const int runs = (J + run - 1) / run;
    PVF_REQUIRE(n <= 65535, "jitter: at most 65535 faces per launch");
    ProfScope ps(c, "jitter");
    hipLaunchKernelGGL(jitter_k, dim3(runs, n), dim3(256), JIT_LDS_BYTES, c->stream, d_chips, sJob.in(c->s_chip), J, run, d_out);
    HIP_CHECK(hipGetLastError());
}

// descriptors of n faces whose chips are on the device: per round, J jittered chips per face, one forward, and the fp32 mean in
// ascending j -- on the host, from what resnet_forward returns (the split embedder's second pass patches that array, so the mean
// comes after it)
void jitter_embed_dev(Ctx* c, const uint8_t* d_chips, int n, int J, uint64_t seed, float* out)
{
    PVF_REQUIRE(J >= 2 && J <= 4096, "jitter: bad arguments");
    const int per = jitter_faces_per_round(J);
    std::vector<float> d((size_t)std::min(per, n) * J * 128);
    for (int i0 = 0; i0 < n; i0 += per) {
        const int m = std::min(per, n - i0);
        uint8_t* dj = jitter_scratch(c, m, J);
        jitter_chips_dev(c, d_chips + (size_t)i0 * JIT_CHIP_BYTES, m, J, seed, dj, false);
        resnet_forward(c, dj, m * J, d.data());
        for (int i = 0; i < m; ++i)
            for (int k = 0; k < 128; ++k) {
                float acc = 0;
                for (int j = 0; j < J; ++j) acc += d[((size_t)i * J + j) * 128 + k];
                out[(size_t)(i0 + i) * 128 + k] = acc / (float)J;
            }
    }
}
