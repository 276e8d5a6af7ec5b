// resnet.hip -- K7: the 29-conv ResNet of dlib's face_recognition_model_v1 (reference pyannote/video/face/face.py:62,74-76)
// as NHWC implicit-GEMM convolutions on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, 157 TF peak),
// with bias + affine + residual add (incl. dlib's zero-extending add_prev and the 2x2 avg-pool skip) + ReLU fused
// into the epilogue.  Batch = all faces of many frames.
#include "pvf_internal.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------
// chip alignment geometry (host; a few doubles per face).  [EXT get_face_chip_details + chip_details]
void face_chip_details(const EmbedModel& m, const int32_t* pts, ChipDetails* out)
{
    const double size = m.chip_size, padding = m.chip_padding;
    double fx[51], fy[51], tx[51], ty[51];
    int n = 0;
    for (int i = 17; i < 68; ++i) {
        if ((55 <= i && i <= 59) || (65 <= i && i <= 67)) continue;
        if (17 <= i && i <= 26) continue;
        fx[n] = ((padding + (double)m.mean_shape[2 * (i - 17)]) / (2 * padding + 1)) * size;
        fy[n] = ((padding + (double)m.mean_shape[2 * (i - 17) + 1]) / (2 * padding + 1)) * size;
        tx[n] = pts[2 * i]; ty[n] = pts[2 * i + 1];
        ++n;
    }
    double mfx = 0, mfy = 0, mtx = 0, mty = 0;
    for (int i = 0; i < n; ++i) { mfx += fx[i]; mfy += fy[i]; mtx += tx[i]; mty += ty[i]; }
    mfx /= n; mfy /= n; mtx /= n; mty /= n;
    double a = 0, b = 0, s = 0;
    for (int i = 0; i < n; ++i) {
        const double ax = fx[i] - mfx, ay = fy[i] - mfy, bx = tx[i] - mtx, by = ty[i] - mty;
        a += ax * bx + ay * by;
        b += ax * by - ay * bx;
        s += ax * ax + ay * ay;
    }
    const double ca = a / s, cb = b / s;
    const double scale = std::sqrt(ca * ca + cb * cb);
    const double hx = size / 2.0, hy = size / 2.0;
    const double cx = (ca * (hx - mfx) - cb * (hy - mfy)) + mtx;
    const double cy = (cb * (hx - mfx) + ca * (hy - mfy)) + mty;
    const double wv = size * scale;
    out->l = cx - wv / 2; out->t = cy - wv / 2; out->r = cx + wv / 2; out->b = cy + wv / 2;
    out->cs = ca / scale; out->sn = cb / scale;
    out->rows = m.chip_size; out->cols = m.chip_size;
}

struct ConvArgs {
    const float* in; int B, H, W, Cin;
    const float* w; int K;             // K = ksz*ksz*Cin (k = (r*ksz + s)*Cin + c), weights transposed: [Cout][K padded to 32]
    const float* frag;                 // the same weights in MFMA fragment order (conv_frag_k), for the layers that have a kernel of their own; or null
    const float* bias; const float* gamma; const float* beta;
    float* out; int OH, OW, Cout;      // output tensor dims
    int AH, AW;                        // conv-valid dims (<= OH, OW)
    int ksz, stride, pad;
    int skip_mode;                     // 0 none, 1 identity [B][OH][OW][Cout], 2 avg-pool 2x2 s2 of x [B][XH][XW][XC]
    const float* skip; int XH, XW, XC, SH, SW;
    // split form (ConvSplit): the weights as f16 hi / lo halves of (w * 2^w_exp), [Cout][Kpad / 32][32 hi, 32 lo]; activations are
    // scaled by 2^EMB_A_SCALE_EXP; out_scale = 2^-(w_exp + 8) undoes both; flags[face] = 1 when a scaled input would overflow f16
    const uint32_t* wsplit; float out_scale; int* flags;
};

// Implicit-GEMM convolution on the matrix cores: conv_tile_k, in two operand forms -- exact fp32 (ConvExact) and, the default, f16 hi / lo
// split operands (ConvSplit; pvf_embedder_split).  A form names its weights, parks a 16-byte quad (k = 4 j4 .. 4 j4 + 3 of a row's chunk)
// of A and of B in LDS, runs a chunk's MFMAs from a lane's row pointers and scales the sums; the kernel holds the rest.  Block tile
// BM x BN = (64 WM) x (32 WN) output pixels x channels, 4 waves; a wave owns a 64 x 32 tile = two 32 x 32 accumulators that share every
// B fragment.  K (= taps x input channels, the order of the oracle's chain) advances in chunks of 32 through LDS; the next chunk's global
// loads are in flight during the MFMAs of the current one.  LDS: one row of 32 k-values per output pixel (A) / output channel (B), 32
// dwords in either form, padded to 36; weights are stored transposed ([cout][K padded to 32], ctx.hip; the split form's: conv_wsplit_k),
// a row Kpad / 4 sixteen-byte units in either form, so that both tiles are staged with the same 16-byte loads along k.

// exact x / d for 0 <= x < 2^22, 1 <= d < 2^22 (rd = 1.0f / d): float estimate, one correction step.  Output pixel -> (face, row, column)
// needs two divisions per tile row; 64-bit integer division is emulated with ~100 instructions, and 16 of them per thread took about as
// long as the K loop of a 3 x 3 x 32 layer.
__device__ __forceinline__ int small_div(int x, int d, float rd)
{
    int q = (int)((float)x * rd);
    const int r = x - q * d;
    q += (r >= d) ? 1 : 0;
    q -= (r < 0) ? 1 : 0;
    return q;
}

// bias + affine + residual add + ReLU and the stores of one block's results (shared by both operand forms of conv_tile_k); `smem` is free
// after the K loop's last barrier and takes each wave's 64 x 32 tile for the transposing store path
template <int WM, int WN>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, float* smem, const f32x16& acc0, const f32x16& acc1, long M, long m0, int n0,
                                              int rel0, int b_first, int hw, float r_hw, float r_ow, int wave, int lane)
{
    constexpr int PITCH = 36;
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, kh = lane >> 5;
    // ---- epilogue: C/D layout of 32x32 MFMA: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
    const int col = n0 + wn * 32 + li;
    const float bias = a.bias[col], g = a.gamma[col], bt = a.beta[col];
    if (a.AH == a.OH && a.AW == a.OW && a.skip_mode != 2) {
        // every output pixel is a convolution result and the skip tensor (if any) has the output's shape: 24 of the 29 layers.
        // The accumulators hold one channel per lane (32 four-byte stores and skip loads per lane, two 128-byte rows per instruction);
        // the wave's tile is turned through LDS so that a lane owns four neighbouring channels of a pixel: 8 sixteen-byte stores (and
        // skip loads), each instruction covering eight full 128-byte rows.  Per-element arithmetic and its order are unchanged.
        float* T = smem + wave * 64 * PITCH;            // (all waves are past the K loop's last barrier)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                T[(t * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * kh) * PITCH + li] = (t == 0 ? acc0[reg] : acc1[reg]);
        __builtin_amdgcn_wave_barrier();                // LDS serves a wave's requests in order; this only pins the compiler's order
        const int c4 = lane & 7, cb = n0 + wn * 32 + 4 * c4;
        const float4 bias4 = *reinterpret_cast<const float4*>(a.bias + cb), g4 = *reinterpret_cast<const float4*>(a.gamma + cb),
                     bt4 = *reinterpret_cast<const float4*>(a.beta + cb);
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int row = it * 8 + (lane >> 3);
            const long m = m0 + wm * 64 + row;
            if (m >= M) continue;
            const float4 x = *reinterpret_cast<const float4*>(&T[row * PITCH + 4 * c4]);
            float4 v = make_float4((x.x + bias4.x) * g4.x + bt4.x, (x.y + bias4.y) * g4.y + bt4.y, (x.z + bias4.z) * g4.z + bt4.z,
                                   (x.w + bias4.w) * g4.w + bt4.w);
            if (a.skip_mode == 1) {
                const float4 sk = *reinterpret_cast<const float4*>(a.skip + (size_t)m * a.Cout + cb);
                v.x += sk.x; v.y += sk.y; v.z += sk.z; v.w += sk.w;
            }
            { v.x = v.x < 0.0f ? 0.0f : v.x; v.y = v.y < 0.0f ? 0.0f : v.y; v.z = v.z < 0.0f ? 0.0f : v.z; v.w = v.w < 0.0f ? 0.0f : v.w; }
            *reinterpret_cast<float4*>(a.out + (size_t)m * a.Cout + cb) = v;
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = (reg & 3) + 8 * (reg >> 2) + 4 * kh;
            const long m = m0 + wm * 64 + t * 32 + row;
            if (m >= M) continue;
            const int rel = rel0 + wm * 64 + t * 32 + row;
            const int bb = small_div(rel, hw, r_hw);
            const int rem = rel - bb * hw;
            const int oy = small_div(rem, a.OW, r_ow);
            const int ox = rem - oy * a.OW;
            const int b = b_first + bb;
            float v = 0.0f;
            if (oy < a.AH && ox < a.AW) v = ((t == 0 ? acc0[reg] : acc1[reg]) + bias) * g + bt;
            if (a.skip_mode == 1) v += a.skip[(size_t)m * a.Cout + col];
            else if (a.skip_mode == 2) {
                if (col < a.XC && oy < a.SH && ox < a.SW) {
                    const float* q = a.skip + (((size_t)b * a.XH + 2 * oy) * a.XW + 2 * ox) * a.XC + col;
                    v += (((q[0] + q[a.XC]) + q[(size_t)a.XW * a.XC]) + q[(size_t)a.XW * a.XC + a.XC]) * 0.25f;
                }
            }
            if (v < 0.0f) v = 0.0f;
            a.out[(size_t)m * a.Cout + col] = v;
        }
}

// Exact fp32 on v_mfma_f32_32x32x2_f32.  A row holds the even k first and the odd k behind them (position (k >> 1) + 16 (k & 1)): lane
// (i, h) of a 32 x 32 x 2 MFMA needs k = 2 s + h for s = 0..15, i.e. 16 CONTIGUOUS floats = 4 ds_read_b128 per 16 MFMAs (the 36-float
// pitch makes them conflict-free), instead of one ds_read_b32 per operand and MFMA.
// (Keeping the activations in that even / odd order in HBM as well -- so that a chunk could be staged with plain 16-byte copies -- was
// measured 10 % SLOWER: the epilogue's stores and skip loads then scatter within each 128-byte line, and four scattered dwords per lane
// quad cost the memory pipeline more than the 36 register moves per chunk that the split on the way into LDS costs.)
struct ConvExact {
    static constexpr bool FLAGS = false;
    static constexpr int LANE_K = 16;                   // dwords between the two half-waves' parts of a row
    static __device__ __forceinline__ const u32x4* weights(const ConvArgs& a) { return reinterpret_cast<const u32x4*>(a.w); }
    static __device__ __forceinline__ bool park_a(uint32_t* row, int j4, const u32x4& v)         // -> whether f16 can hold the quad
    {
        *reinterpret_cast<uint2*>(row + 2 * j4) = make_uint2(v.x, v.z);            // k = 4 j4, 4 j4 + 2   (even half)
        *reinterpret_cast<uint2*>(row + 2 * j4 + 16) = make_uint2(v.y, v.w);       // k = 4 j4 + 1, + 3    (odd half)
        return true;
    }
    static __device__ __forceinline__ void park_b(uint32_t* row, int j4, const u32x4& v) { park_a(row, j4, v); }
    static __device__ __forceinline__ void chunk(const uint32_t* pa0, const uint32_t* pa1, const uint32_t* pb, f32x16& acc0, f32x16& acc1)
    {
        f32x4 fa0[4], fa1[4], fb[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            fa0[q] = *reinterpret_cast<const f32x4*>(pa0 + 4 * q);
            fa1[q] = *reinterpret_cast<const f32x4*>(pa1 + 4 * q);
            fb[q] = *reinterpret_cast<const f32x4*>(pb + 4 * q);
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0[s >> 2][s & 3], fb[s >> 2][s & 3], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1[s >> 2][s & 3], fb[s >> 2][s & 3], acc1, 0, 0, 0);
        }
    }
    static __device__ __forceinline__ void scale(const ConvArgs&, f32x16&, f32x16&) {}
};

// Split f16 on v_mfma_f32_32x32x16_f16.  Every scaled operand is a pair of f16 halves, v = hi + lo + e with hi = f16(v), lo = f16(v - hi)
// (v - hi is exact in fp32), and a product is three MFMA terms, hi.hi + hi.lo + lo.hi, accumulated in fp32 (DESIGN.md section 4 for the
// bound).  The scales are fixed powers of two: activations x 2^8 (EMB_A_SCALE_EXP, the same for every layer and face), weights x 2^w_exp
// per layer with the largest |w| in [2^14, 2^15) (from the weights at model load); the sums are multiplied by 2^-(8 + w_exp), exactly,
// before the fp32 arithmetic of conv_epilogue.  No scale depends on the data, so a face's descriptor never depends on its batch-mates.
// A scaled input that f16 cannot hold (|x| >= 65504 / 256) marks its face in a.flags; resnet_forward embeds those faces again in the
// exact form.  A row holds the chunk's 32 hi halves (16 dwords), then its 32 lo halves: lane (i, h) of k-step s (k = 16 s + 8 h + j)
// reads hi at dword 8 s + 4 h and lo 16 dwords behind, one ds_read_b128 each (conflict-free with the 36-dword pitch).  A is split on
// the way into LDS; a quad of B (split once per model, conv_wsplit_k: j4 < 4 hi halves, j4 >= 4 lo halves) is copied as is.
#define EMB_A_SCALE_EXP 8
#define EMB_F16_LIMIT 65504.0f
struct ConvSplit {
    static constexpr bool FLAGS = true;
    static constexpr int LANE_K = 4;
    static __device__ __forceinline__ const u32x4* weights(const ConvArgs& a) { return reinterpret_cast<const u32x4*>(a.wsplit); }
    static __device__ __forceinline__ bool park_a(uint32_t* row, int j4, const u32x4& v)
    {
        const f32x4 xv = __builtin_bit_cast(f32x4, v) * (float)(1 << EMB_A_SCALE_EXP);   // (the whole vector: a bit_cast of one element read element 0)
        // every value on its own: a NaN fails its comparison (fmaxf over the four would drop a NaN that stands next to a number, and
        // the face would not be marked); a row without a pixel loads zeros only
        const bool ok = __builtin_reduce_and(__builtin_elementwise_abs(xv) < EMB_F16_LIMIT);
        const f16x4 hi = __builtin_convertvector(xv, f16x4), lo = __builtin_convertvector(xv - __builtin_convertvector(hi, f32x4), f16x4);
        *reinterpret_cast<u32x2*>(row + 2 * j4) = __builtin_bit_cast(u32x2, hi);
        *reinterpret_cast<u32x2*>(row + 2 * j4 + 16) = __builtin_bit_cast(u32x2, lo);
        return ok;
    }
    static __device__ __forceinline__ void park_b(uint32_t* row, int j4, const u32x4& v) { *reinterpret_cast<u32x4*>(row + 4 * j4) = v; }
    static __device__ __forceinline__ void chunk(const uint32_t* pa0, const uint32_t* pa1, const uint32_t* pb, f32x16& acc0, f32x16& acc1)
    {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const f16x8 ah0 = *reinterpret_cast<const f16x8*>(pa0 + 8 * s), al0 = *reinterpret_cast<const f16x8*>(pa0 + 16 + 8 * s);
            const f16x8 ah1 = *reinterpret_cast<const f16x8*>(pa1 + 8 * s), al1 = *reinterpret_cast<const f16x8*>(pa1 + 16 + 8 * s);
            const f16x8 bh = *reinterpret_cast<const f16x8*>(pb + 8 * s), bl = *reinterpret_cast<const f16x8*>(pb + 16 + 8 * s);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah0, bh, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah1, bh, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah0, bl, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah1, bl, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al0, bh, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al1, bh, acc1, 0, 0, 0);
        }
    }
    static __device__ __forceinline__ void scale(const ConvArgs& a, f32x16& acc0, f32x16& acc1) { acc0 *= a.out_scale; acc1 *= a.out_scale; }
};

template <int WM, int WN, class Ops>
__global__ void __launch_bounds__(256) conv_tile_k(ConvArgs a)
{
    constexpr int BM = 64 * WM, BN = 32 * WN, KC = 32, PITCH = 36;
    static_assert(WM * WN == 4, "four waves per block");
    constexpr int SM_ROWS = (BM + BN > 256) ? BM + BN : 256;         // A tile, B tile; after the K loop each wave's 64 x 32 results
    __shared__ __attribute__((aligned(16))) float smem[SM_ROWS * PITCH];
    uint32_t* As = reinterpret_cast<uint32_t*>(smem);
    uint32_t* Bs = As + BM * PITCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const long M = (long)a.B * a.OH * a.OW;
    const long m0 = (long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.0f; acc1[i] = 0.0f; }

    // staging roles: A tile = BM rows x 8 quads (4 consecutive k = 4 input channels of one tap), B tile = BN rows x 8 quads.
    // Input pixels are fetched with raw buffer loads: a tap that falls outside the image (or a row past M, or k past K) gets an offset
    // beyond the buffer and comes back as zeros -- no branch around any load, so the address arithmetic of the next chunk is one
    // straight-line block the scheduler spreads between the MFMAs of the current one.
    constexpr int A_F4 = BM * 8 / 256, B_F4 = BN * 8 / 256;
    constexpr int RSRC_FLAGS = 0x00020000, OOB = (int)0x80000000;
    const int hw = a.OH * a.OW;
    const int b_first = (int)(m0 / hw);                                    // the tile's first face: offsets below stay small (scalar)
    const int rel0 = (int)(m0 - (long)b_first * hw);                       // tile rows are rel0 + i within [first face ...): < hw + BM
    const float r_hw = 1.0f / (float)hw, r_ow = 1.0f / (float)a.OW;
    const size_t face = (size_t)a.H * a.W * a.Cin;
    const size_t in_bytes = (size_t)(a.B - b_first) * face * sizeof(float);
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc((void*)(a.in + (size_t)b_first * face), 0,
                                                                           in_bytes > 0x7ffffff0u ? 0x7ffffff0 : (int)in_bytes, RSRC_FLAGS);
    int pa_off[A_F4], pa_y[A_F4], pa_x[A_F4];       // float index of the input pixel under tap (0, 0); its coordinates (y = -2^20: no pixel)
#pragma unroll
    for (int q = 0; q < A_F4; ++q) {
        const int i = (tid + q * 256) >> 3;
        const long m = m0 + i;
        pa_off[q] = 0; pa_y[q] = -(1 << 20); pa_x[q] = 0;
        if (m < M) {
            const int rel = rel0 + i;
            const int bb = small_div(rel, hw, r_hw);
            const int rem = rel - bb * hw;
            const int oy = small_div(rem, a.OW, r_ow);
            const int ox = rem - oy * a.OW;
            if (oy < a.AH && ox < a.AW) {
                pa_y[q] = oy * a.stride - a.pad; pa_x[q] = ox * a.stride - a.pad;
                pa_off[q] = ((bb * a.H + pa_y[q]) * a.W + pa_x[q]) * a.Cin;
            }
        }
    }
    const int Kpad = (a.K + KC - 1) / KC * KC;
    const int j4 = tid & 7;                             // which quad of a row this thread moves
    const u32x4* wrow[B_F4];
#pragma unroll
    for (int q = 0; q < B_F4; ++q) wrow[q] = Ops::weights(a) + (size_t)(n0 + ((tid + q * 256) >> 3)) * (Kpad / 4) + j4;
    u32x4 va[A_F4], vb[B_F4];
    // Three stages per chunk, one chunk apart: its byte offsets are worked out (plain VALU work, spread between the MFMAs of an earlier
    // chunk), its loads are issued right after the barrier of the chunk before it, and it is parked in LDS one barrier later.
    // Chunk walk: (tap row, tap column, first channel) advance with scalar adds, no division in the loop (input channels: a multiple of 32).
    int f_r = 0, f_s = 0, f_c = 0, f_k = 0;             // the chunk whose offsets are computed next
    int voff[A_F4], woff = 0;
    auto offsets = [&]() {
        const int kq = f_k + 4 * j4;
        const int r = f_r, sft = f_s;                   // wave-uniform
        const int delta = (r * a.W + sft) * a.Cin + f_c + 4 * j4;
        const int k_ok = (kq < a.K) ? -1 : 0;
#pragma unroll
        for (int q = 0; q < A_F4; ++q) {
            const int iy = pa_y[q] + r, ix = pa_x[q] + sft;
            // all-ones when the tap lies inside the image: plain integer logic (no short-circuit branches around the loads)
            const int ok = k_ok & -(int)((unsigned)iy < (unsigned)a.H) & -(int)((unsigned)ix < (unsigned)a.W);
            voff[q] = (((pa_off[q] + delta) * 4) & ok) | (OOB & ~ok);
        }
        woff = f_k >> 2;                                // sixteen-byte units: a chunk's row is 8 of them
        if (f_k + KC < Kpad) {                          // (past the last chunk: stay on it; those loads are issued but never parked)
            f_k += KC;
            f_c += KC;
            if (f_c >= a.Cin) { f_c = 0; if (++f_s == a.ksz) { f_s = 0; ++f_r; } }
        }
    };
    auto issue = [&]() {
#pragma unroll
        for (int q = 0; q < A_F4; ++q) va[q] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, voff[q], 0, 0);
#pragma unroll
        for (int q = 0; q < B_F4; ++q) vb[q] = wrow[q][woff];                                        // zero-padded beyond K
    };
    auto park = [&]() {
        int bad = 0;                                    // bit q: slot q holds a value that f16 cannot take
#pragma unroll
        for (int q = 0; q < A_F4; ++q) bad |= Ops::park_a(&As[((tid + q * 256) >> 3) * PITCH], j4, va[q]) ? 0 : (1 << q);
#pragma unroll
        for (int q = 0; q < B_F4; ++q) Ops::park_b(&Bs[((tid + q * 256) >> 3) * PITCH], j4, vb[q]);
        if constexpr (Ops::FLAGS)
            if (bad)
                for (int q = 0; q < A_F4; ++q)
                    if ((bad >> q) & 1) a.flags[b_first + small_div(rel0 + ((tid + q * 256) >> 3), hw, r_hw)] = 1;
    };
    const int li = lane & 31, kh = lane >> 5;
    const uint32_t* pa0 = &As[(wm * 64 + li) * PITCH + Ops::LANE_K * kh];
    const uint32_t* pa1 = pa0 + 32 * PITCH;
    const uint32_t* pb = &Bs[(wn * 32 + li) * PITCH + Ops::LANE_K * kh];
    offsets();
    issue();
    offsets();
    for (int k0 = 0; k0 < Kpad; k0 += KC) {
        park();
        __syncthreads();
        issue();                                      // chunk k0 + KC: in flight during all of this chunk's MFMAs
        __builtin_amdgcn_sched_barrier(0);
        offsets();                                    // chunk k0 + 2 KC
        Ops::chunk(pa0, pa1, pb, acc0, acc1);
        __syncthreads();
    }
    Ops::scale(a, acc0, acc1);
    conv_epilogue<WM, WN>(a, smem, acc0, acc1, M, m0, n0, rel0, b_first, hw, r_hw, r_ow, wave, lane);
}

// (Two other forms of the K loop were built and measured no faster, and are gone: tiles straight into LDS by LDS-DMA, round 4 --
// profiles/r04_conv_lds_vs_regs.txt -- and a spatial input tile reused across the 9 taps, one fetch per pixel and one barrier per block,
// round 5 -- profiles/r05_conv_band_experiment.txt: a layer's MFMAs and its unavoidable HBM traffic are of the same size and run one
// after the other inside a block; the staging of the A operand is not what the matrix pipe waits for.)

// w [cout][Kpad] fp32 -> out [cout][Kpad / 32][32 hi, 32 lo] f16 of w * 2^w_exp
__global__ void __launch_bounds__(256) conv_wsplit_k(const float* __restrict__ w, int total, int w_exp, _Float16* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float v = ldexpf(w[i], w_exp);
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (float)hi);
    const int row32 = i >> 5, kk = i & 31;                // (cout, chunk) rows of 32 k
    out[(size_t)row32 * 64 + kk] = hi;
    out[(size_t)row32 * 64 + 32 + kk] = lo;
}

// What the split form takes for granted about the device, checked once per context (a mismatch is an error, not a fallback): lanes
// (row, k octet) of A and (column, k octet) of B meet in v_mfma_f32_32x32x16_f16 as ConvSplit's LDS reads assume, lane (column, row
// group) receives D as conv_epilogue assumes, and an accumulation of K products inside the matrix pipe stays within the allowance of
// the error bound (2^-22 per addition relative to the sum of the terms' magnitudes: DESIGN.md section 4).  One wave; a, b in lane order.
__global__ void __launch_bounds__(64) embed_probe_k(const uint4* __restrict__ a, const uint4* __restrict__ b, int steps, float* __restrict__ d)
{
    const int lane = threadIdx.x;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (int s = 0; s < steps; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[s * 64 + lane]), __builtin_bit_cast(f16x8, b[s * 64 + lane]), acc, 0, 0, 0);
    for (int i = 0; i < 16; ++i) d[lane * 16 + i] = acc[i];
}

// ---------------------------------------------------------------------------------------------------
// The first layer (7 x 7, stride 2, 3 -> 32 channels on the 150 x 150 chip) straight from the uint8 chips.  Through the generic kernel it
// cost three passes over HBM (an input pass: bytes -> 4-channel floats, 270 KB per face written and read back; the result, 663 KB per
// face) and a K of 7 * 7 * 4 = 196 padded to 224 for 147 real products; its A tile was gathered tap by tap from global memory although
// a block's whole input is 6 KB.  Here a block owns FOUR output rows of one face (288 pixels = nine 32-row MFMA tiles, three per wave,
// three waves): the 13 chip rows under them are parked in LDS as bytes (one contiguous, 4-byte aligned range of the chip), the layer's
// weights next to them in fragment order (stem_frag_k, once per model), and the K loop is unrolled over 77 k-pairs -- the 21 values
// under a tap ROW (7 taps x 3 colours) are 21 consecutive bytes of a chip row, so k runs along them in pairs, eleven per tap row, the
// last pair padded with a zero weight.  Per MFMA a lane reads ONE byte at a constant offset from its pixel's base (ds_read_u8 with an
// immediate), converts it ((q - mean) / 256, as the input pass did) and feeds it with the pair's weight fragment to its three tiles.
// The chain runs over the same products in the same order as the generic kernel's did (taps row-major, colour fastest; that one's
// fourth channel and its k = 196 .. 223 added exact zeros); the pairing inside an MFMA differs ((c0, c1), (c2, next tap's c0) ...
// instead of (c0, c1), (c2, 0)) -- and the descriptors are the same bit for bit (tools/bench_embed.py prints their checksum): the
// 32 x 32 x 2 MFMA adds its two products to the accumulator one after the other.  Measured on 4096 faces: 24.1 -> 22.9 ms for the
// whole network with 98 pairs (the generic pairing), 22.4 -> 21.8 with 77.
#define STEM_ROWS 4
#define STEM_IN_DW 1464                                   // 13 rows x 450 bytes = 5850 bytes
#define STEM_NP 77                                        // k-pairs: 7 tap rows x 11 pairs (21 values of a row + one zero-weight pad)
__global__ void __launch_bounds__(64) stem_frag_k(const float* __restrict__ w, float* __restrict__ frag)
{
    // frag[pair][lane] = weight of channel lane & 31 for the pair's k of this half-wave: tap row r, position t = 2 pp + (lane >> 5) in the
    // row's 21 values (t = 3 q + c: tap column q, colour c; t = 21: the pad); w is the generic layout [cout][224], k = (r * 7 + q) * 4 + c
    const int p = blockIdx.x, l = threadIdx.x;
    const int r = p / 11, t = 2 * (p - r * 11) + (l >> 5);
    frag[p * 64 + l] = (t < 21) ? w[(size_t)(l & 31) * 224 + (r * 7 + t / 3) * 4 + t % 3] : 0.0f;
}

__global__ void __launch_bounds__(192) stem_conv_k(const uint8_t* __restrict__ chips, int B, const float* __restrict__ frag, const float* __restrict__ bias,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ out)
{
    constexpr int S = 150, OW = 72;
    __shared__ uint32_t s_in[STEM_IN_DW];
    __shared__ __attribute__((aligned(16))) float s_b[STEM_NP * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int face = blockIdx.y, oy0 = blockIdx.x * STEM_ROWS;
    {
        // the chips behind a descriptor (a dword past the last chip's end reads as zero); a block's range starts on a multiple of 4:
        // a chip is 67500 bytes, two chip rows 900
        const size_t total = (size_t)B * S * S * 3;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(chips + (size_t)face * S * S * 3), 0,
                                                                             (int)std::min<size_t>(total - (size_t)face * S * S * 3, 0x7ffffff0u), 0x00020000);
        const int first = 2 * oy0 * S * 3;
        for (int i = tid; i < STEM_IN_DW; i += 192) s_in[i] = __builtin_amdgcn_raw_buffer_load_b32(rs, 4 * i, first, 0);
        const float4* f4 = reinterpret_cast<const float4*>(frag);
        float4* b4 = reinterpret_cast<float4*>(s_b);
        for (int i = tid; i < STEM_NP * 16; i += 192) b4[i] = f4[i];
    }
    __syncthreads();
    const int li = lane & 31, kh = lane >> 5;
    const uint8_t* px = reinterpret_cast<const uint8_t*>(s_in);
    const uint8_t* base[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int m = (wave * 3 + t) * 32 + li;           // pixel of the block: row m / 72, column m % 72
        const int oy = m / OW, ox = m - oy * OW;
        base[t] = px + ((2 * oy) * S + 2 * ox) * 3 + kh;
    }
    // colour of this lane's k in pair pp of a row: (2 pp + kh) % 3 -- three cases by pp % 3
    const float M0 = 122.782f, M1 = 117.001f, M2 = 104.298f;
    const float mean3[3] = {kh ? M1 : M0, kh ? M0 : M2, kh ? M2 : M1};
    f32x16 acc[3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
#pragma unroll
    for (int s = 0; s < STEM_NP; ++s) {
        const int r = s / 11, pp = s - r * 11;
        const int off = r * S * 3 + 2 * pp;               // + kh (in the base): the row's 21 bytes under the tap row are consecutive
        const float b = s_b[s * 64 + lane];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const float a = ((float)base[t][off] - mean3[pp % 3]) / 256.0f;
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
        }
    }
    // C layout of the 32 x 32 MFMA: column (channel) = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const float bs = bias[li], g = gamma[li], bt = beta[li];
    float* o = out + ((size_t)face * OW + oy0) * OW * 32 + li;
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int m = (wave * 3 + t) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * kh;
            float v = (acc[t][reg] + bs) * g + bt;
            v = v < 0.0f ? 0.0f : v;
            o[(size_t)m * 32] = v;
        }
}

// ---------------------------------------------------------------------------------------------------
// The six 3 x 3 layers of the 35 x 35 x 32 stage (a quarter of the network's arithmetic, and through the generic kernel its least efficient
// part: 32 output channels are ONE MFMA column tile, so every A element staged through LDS feeds a single MFMA) in the first layer's
// form.  A work item is a band of SEVEN output rows of one face (245 pixels: eight 32-row tiles, two per wave); the nine input rows
// under it sit in LDS with their zero border, [row][column][33 floats] (the odd pitch spreads a tile's pixels over the banks), the
// layer's weights next to them in fragment order (81 KB together: two blocks per CU); the K loop is unrolled over the 144 k-pairs, and
// per MFMA a lane reads ONE float at a constant offset from its pixel's base.  Products, pairing and chain order are the generic
// kernel's (k = (tap, channel), channel pairs (2 j, 2 j + 1)), so is the epilogue's arithmetic: bit-identical results.
// How it got here (4096 faces, per layer; the generic kernel: 1.03-1.17 ms; the layer's MFMAs alone at the clock they run at: 0.8 ms --
// measured with the loads and the stores compiled out): one block per band with the tile loaded slot by slot 1.58 ms (eleven round
// trips to HBM in a row), with all of a thread's slots requested before the first is parked 1.1-1.3 ms, resident blocks that request the
// NEXT band's rows before the current band's MFMAs 0.95-1.12 ms.  What is left beside the MFMAs is parking the rows (44 LDS writes per
// thread), two barriers and the stores, at two waves per SIMD.
#define C32_ROWS 7
#define C32_TILE_FLOATS (9 * 37 * 33)
__global__ void __launch_bounds__(64) conv_frag_k(const float* __restrict__ w, int Kpad, float* __restrict__ frag)
{
    const int s = blockIdx.x, l = threadIdx.x;            // frag[s][lane] = w[channel lane & 31][k = 2 s + (lane >> 5)]
    frag[s * 64 + l] = w[(size_t)(l & 31) * Kpad + 2 * s + (l >> 5)];
}

__global__ void __launch_bounds__(256) conv3x3_c32_k(const float* __restrict__ in, const float* __restrict__ frag, const float* __restrict__ bias,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ skip,
                                                     float* __restrict__ out, int n_items)
{
    constexpr int HW = 35, TW = 37, PITCH = 33, NP = 144;
    constexpr int NSLOT = 9 * TW * 8, PER = (NSLOT + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) float smem_c32[];
    float* T = smem_c32;                                  // [9][37][33]
    float* Bf = smem_c32 + C32_TILE_FLOATS;               // [144][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, kh = lane >> 5;
    // A block is resident for the whole layer and takes every gridDim.x-th band (item = face * 5 + band): the weight fragments are parked
    // once, and the NEXT band's input rows (and this band's skip values) are requested before the current band's MFMAs start, so that
    // what a band costs beside its MFMAs is parking 11 float4 per thread and issuing its stores.
    {
        const float4* f4 = reinterpret_cast<const float4*>(frag);
        float4* b4 = reinterpret_cast<float4*>(Bf);
        for (int i = tid; i < NP * 16; i += 256) b4[i] = f4[i];
    }
    const float bs = bias[li], g = gamma[li], bt = beta[li];
    const float* base[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        int m = (wave * 2 + t) * 32 + li;                 // pixel of the band: row m / 35, column m % 35 (rows past the band: computed on pixel 0, never stored)
        if (m >= C32_ROWS * HW) m = 0;
        const int oy = m / HW, ox = m - oy * HW;
        base[t] = T + (oy * TW + ox) * PITCH + kh;
    }
    const float* bl = Bf + lane;
    // a thread's slots of the tile (four channels of one tile pixel each): where they come from relative to the band's first input row;
    // which of them lie in a border column (always zero), in the tile's first / last row (zero for a face's first / last band)
    int s_off[PER];
    unsigned m_col = 0, m_row0 = 0, m_row8 = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = tid + j * 256;
        const int c4 = i & 7, px = i >> 3;
        const int ry = px / TW, cx = px - ry * TW;
        if ((i < NSLOT) && ((unsigned)(cx - 1) < (unsigned)HW)) m_col |= 1u << j;
        if (ry == 0) m_row0 |= 1u << j;
        if (ry == 8) m_row8 |= 1u << j;
        s_off[j] = (ry * HW + (cx - 1)) * 32 + 4 * c4;
    }
    float4 v[PER];
    float sk[2][16];
    auto request = [&](int item) {                        // the band's nine input rows, zero outside the image
        const int face = item / 5, band = item - face * 5;
        const float* src = in + ((size_t)face * HW + (band * C32_ROWS - 1)) * HW * 32;
        const unsigned ok = m_col & ~(band == 0 ? m_row0 : 0u) & ~(band == 4 ? m_row8 : 0u);
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            v[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if ((ok >> j) & 1u) v[j] = *reinterpret_cast<const float4*>(src + s_off[j]);
        }
    };
    // the band's output (and skip) rows behind buffer descriptors: 245 pixels x 32 channels; the tile rows past the band (the last tile's
    // rows 21 .. 31) fall outside and are dropped / read as zero -- no lane-dependent branch around any access
    constexpr int BAND_BYTES = C32_ROWS * HW * 32 * 4;
    int e_off[2][16];                                     // byte offset of (this lane's channel, accumulator row) inside the band
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) e_off[t][reg] = (((wave * 2 + t) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * kh) * 32 + li) * 4;
    auto request_skip = [&](int item) {                   // the band's skip values: in flight during its own MFMAs
        const int face = item / 5, oy0 = (item - face * 5) * C32_ROWS;
        const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)(skip + ((size_t)face * HW + oy0) * HW * 32), 0, BAND_BYTES, 0x00020000);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) sk[t][reg] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rk, e_off[t][reg], 0, 0));
    };
    int item = blockIdx.x;
    if (item < n_items) request(item);
    while (item < n_items) {
        // park the band that was requested during the previous one's MFMAs
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = tid + j * 256;
            if (i < NSLOT) {
                float* d = T + (i >> 3) * PITCH + 4 * (i & 7);
                d[0] = v[j].x; d[1] = v[j].y; d[2] = v[j].z; d[3] = v[j].w;
            }
        }
        __syncthreads();
        const int next = item + gridDim.x;
        if (next < n_items) request(next);
        if (skip) request_skip(item);
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            const int tap = s >> 4, r = tap / 3, q = tap - r * 3;
            const int off = (r * TW + q) * PITCH + 2 * (s & 15);
            const float b = bl[s * 64];
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(base[t][off], b, acc[t], 0, 0, 0);
        }
        // C layout of the 32 x 32 MFMA: column (channel) = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); a band's pixels are
        // contiguous in the output tensor.  All 32 results are finished first (ONE wait for the skip values), then the 32 stores go out
        // back to back: written value by value the compiler waits before every store for everything in flight -- the next band's rows
        // included -- because the skip value it is about to add might still be on its way.
        const int face = item / 5, oy0 = (item - face * 5) * C32_ROWS;
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)(out + ((size_t)face * HW + oy0) * HW * 32), 0, BAND_BYTES, 0x00020000);
        float x[2][16];
        if (skip) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const float y = ((acc[t][reg] + bs) * g + bt) + sk[t][reg];
                    x[t][reg] = y < 0.0f ? 0.0f : y;
                }
        } else {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const float y = (acc[t][reg] + bs) * g + bt;
                    x[t][reg] = y < 0.0f ? 0.0f : y;
                }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, x[t][reg]), ro, e_off[t][reg], 0, 0);
        __syncthreads();                                  // every wave is done with the tile before the next band is parked
        item = next;
    }
}

__global__ void __launch_bounds__(256) maxpool3s2_k(const float* __restrict__ in, int B, int H, int W, int C, float* __restrict__ out, int OH, int OW)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)B * OH * OW * C;
    if (i >= total) return;
    const int c = (int)(i % C);
    size_t t = i / C;
    const int ox = (int)(t % OW); t /= OW;
    const int oy = (int)(t % OH);
    const int b = (int)(t / OH);
    float mx = -INFINITY;
    for (int r = 0; r < 3; ++r)
        for (int s = 0; s < 3; ++s) {
            const float v = in[(((size_t)b * H + oy * 2 + r) * W + ox * 2 + s) * C + c];
            mx = fmaxf(mx, v);
        }
    out[i] = mx;
}

// avg_pool_everything + fc_no_bias<128>: one block per face
__global__ void __launch_bounds__(256) head_k(const float* __restrict__ x, int HW, const float* __restrict__ fc, float* __restrict__ out)
{
    __shared__ float feat[256];
    const int b = blockIdx.x, t = threadIdx.x;
    float s = 0.0f;
    for (int i = 0; i < HW; ++i) s += x[((size_t)b * HW + i) * 256 + t];
    feat[t] = s / (float)HW;
    __syncthreads();
    if (t < 128) {
        float acc = 0.0f;
        for (int o = 0; o < 256; ++o) acc += feat[o] * fc[(size_t)o * 128 + t];
        out[(size_t)b * 128 + t] = acc;
    }
}

// the layers that conv3x3_c32_k takes: 3 x 3, stride 1, pad 1, 32 -> 32 channels on the 35 x 35 map, all of it convolved, no averaged skip
static bool conv_is_c32(const ConvArgs& a)
{
    return a.Cin == 32 && a.Cout == 32 && a.H == 35 && a.W == 35 && a.OH == 35 && a.OW == 35 && a.AH == 35 && a.AW == 35 && a.ksz == 3 &&
           a.stride == 1 && a.pad == 1 && a.skip_mode != 2;
}

static void launch_conv(Ctx* c, const ConvArgs& a)
{
    const long M = (long)a.B * a.OH * a.OW;
    PVF_REQUIRE(a.Cin % 32 == 0, "conv: input channels must be a multiple of 32 (the 3-channel first layer has a kernel of its own: stem_conv_k)");
    PVF_REQUIRE(a.OH * a.OW < (1 << 21) && a.Cout % 32 == 0, "conv: output map too large for the kernel's index arithmetic / Cout not a multiple of 32");
    // (a tile shape's kernel in the operand form a's weights come in)
    auto tile = [&](auto exact, auto split, dim3 grid) { hipLaunchKernelGGL((a.wsplit ? split : exact), grid, dim3(256), 0, c->stream, a); };
    if (a.frag && conv_is_c32(a)) {
        static std::atomic<uint64_t> attr_set{0};             // per device (a function attribute belongs to the device it was set on)
        const size_t lds = (size_t)(C32_TILE_FLOATS + 144 * 64) * sizeof(float);
        const uint64_t bit = 1ull << (c->device & 63);
        if (!(attr_set.load() & bit)) {
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_c32_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            attr_set.fetch_or(bit);
        }
        const int items = a.B * (35 / C32_ROWS);
        hipLaunchKernelGGL(conv3x3_c32_k, dim3((unsigned)std::min(items, 2 * c->n_cu)), dim3(256), lds, c->stream, a.in, a.frag, a.bias, a.gamma, a.beta,
                           a.skip_mode == 1 ? a.skip : nullptr, a.out, items);
    } else if (a.Cout == 32) {
        tile(conv_tile_k<4, 1, ConvExact>, conv_tile_k<4, 1, ConvSplit>, dim3((unsigned)((M + 255) / 256), 1));
    } else {
        PVF_REQUIRE(a.Cout % 64 == 0, "conv: Cout must be 32 or a multiple of 64");
        tile(conv_tile_k<2, 2, ConvExact>, conv_tile_k<2, 2, ConvSplit>, dim3((unsigned)((M + 127) / 128), a.Cout / 64));
    }
}

// ---- a layer's weights as the kernels read them (the model loader, resnet_run and pvf_debug_conv all come through here) -------------
void conv_layer_upload(ConvLayer& L, const float* w, const float* bias, const float* gamma, const float* beta)
{
    const int cin = L.cin, cout = L.cout, k = L.k;
    // [cout][cin][r][s] -> [cout][kk], kk = (r*k+s)*cp + c, rows zero-padded to a multiple of 32 (the conv kernel's K chunk); the
    // 3-channel input layer is stored with a fourth, all-zero channel (cp = 4) so that the kernel stages one pixel tap with one 16-byte
    // load: x + 0 * w is exact, the chain is unchanged
    const int cp = (cin == 3) ? 4 : cin;
    const int K = k * k * cp, Kpad = (K + 31) / 32 * 32;
    std::vector<float> wt((size_t)cout * Kpad, 0.0f);
    for (int o = 0; o < cout; ++o)
        for (int ci = 0; ci < cin; ++ci)
            for (int r = 0; r < k; ++r)
                for (int s = 0; s < k; ++s) {
                    const int kk = (r * k + s) * cp + ci;
                    wt[(size_t)o * Kpad + kk] = w[(((size_t)o * cin + ci) * k + r) * k + s];
                }
    auto up = [](const float* src, size_t count) {
        float* d = nullptr;
        HIP_CHECK(hipMalloc((void**)&d, count * sizeof(float)));
        HIP_CHECK(hipMemcpy(d, src, count * sizeof(float), hipMemcpyHostToDevice));
        return d;
    };
    L.d_w = up(wt.data(), wt.size());
    // the split path's weight scale: a power of two that puts the largest |w| in [2^14, 2^15) (a function of the weights only)
    float wmax = 0.0f;
    for (float v : wt) wmax = std::max(wmax, std::fabs(v));
    int ex = 0;
    if (wmax > 0.0f && std::isfinite(wmax)) { std::frexp(wmax, &ex); L.w_exp = 15 - ex; }     // wmax = f 2^ex, f in [0.5, 1)
    L.d_bias = up(bias, cout);
    L.d_gamma = up(gamma, cout);
    L.d_beta = up(beta, cout);
}

void conv_layer_free(ConvLayer& L)
{
    for (void* p : {(void*)L.d_w, (void*)L.d_bias, (void*)L.d_gamma, (void*)L.d_beta, (void*)L.d_frag, (void*)L.d_wsplit})
        if (p) (void)hipFree(p);
    L.d_w = L.d_bias = L.d_gamma = L.d_beta = L.d_frag = nullptr;
    L.d_wsplit = nullptr;
}

// the weight side of a's launch (its geometry is filled in): d_w, and what the layer's kernel wants beside it, made on first use -- the
// fragment order for conv3x3_c32_k's layers (`generic`: not even there), else with `split` the f16 halves and their scale
static void conv_bind_weights(Ctx* c, ConvLayer& L, bool split, bool generic, int* flags, ConvArgs& a)
{
    a.w = L.d_w; a.K = L.k * L.k * L.cin; a.bias = L.d_bias; a.gamma = L.d_gamma; a.beta = L.d_beta;
    a.frag = nullptr; a.wsplit = nullptr; a.out_scale = 0.0f; a.flags = nullptr;
    if (!generic && L.cin == 32 && L.cout == 32 && L.k == 3) {     // a 32 -> 32 3 x 3 layer is never split: exact fp32 on any map
        if (!conv_is_c32(a)) return;                                // (a map other than conv3x3_c32_k's: only pvf_debug_conv brings one)
        if (!L.d_frag) {
            HIP_CHECK(hipMalloc(&L.d_frag, 144 * 64 * sizeof(float)));
            hipLaunchKernelGGL(conv_frag_k, dim3(144), dim3(64), 0, c->stream, L.d_w, 288, L.d_frag);
        }
        a.frag = L.d_frag;
        return;                                         // (the 32-channel stage stays on conv3x3_c32_k)
    }
    if (!split) return;
    if (!L.d_wsplit) {
        const int Kpad = (L.k * L.k * L.cin + 31) / 32 * 32;
        const int total = L.cout * Kpad;
        HIP_CHECK(hipMalloc(&L.d_wsplit, (size_t)total * 2 * sizeof(_Float16)));
        hipLaunchKernelGGL(conv_wsplit_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, L.d_w, total, L.w_exp,
                           reinterpret_cast<_Float16*>(L.d_wsplit));
    }
    a.wsplit = L.d_wsplit;
    a.out_scale = std::ldexp(1.0f, -(EMB_A_SCALE_EXP + L.w_exp));
    a.flags = flags;
}

// ---- embed_probe: the f16 matrix pipe against what the split form assumes (once per context, before the first split forward) ----------
static uint16_t f16_bits(float v)
{
    const _Float16 h = (_Float16)v;                     // host conversion: round to nearest even
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

// Two cases of K = 2304 (the network's longest chain, 9 x 256) on one 32 x 32 tile, exact sums in double on the host: (1) pseudo-random
// f16 values of both signs over 2^-10 .. 2^15 -- distinct per (row, k) and (k, column), so a lane map other than the kernel's shows up
// as an error of the order of the sums; (2) the three split terms of pseudo-random fp32 operands at the scales the kernel uses (hi.hi,
// hi.lo, lo.hi in one chain).  The worst |pipe - exact| / sum of |terms| of both is kept (pvf_embedder_split_stats: pipe_err) and must
// stay within the allowance of the bound: K x 2^-22.
static void embed_probe(Ctx* c)
{
    const int steps = 144;
    const int K = steps * 16;
    const size_t nh = (size_t)steps * 64 * 8;
    std::vector<uint16_t> ha(nh), hb(nh);
    std::vector<double> A((size_t)32 * K), B((size_t)K * 32);
    uint8_t* dev = nullptr;
    const size_t fb = nh * 2;
    HIP_CHECK(hipMalloc((void**)&dev, 2 * fb + 64 * 16 * sizeof(float)));
    float* d_d = reinterpret_cast<float*>(dev + 2 * fb);
    float hd[64 * 16];
    // lane l = 32 h + r of k-step s holds A[r][16 s + 8 h + j] and B[16 s + 8 h + j][r] in element j
    auto ia = [&](int r, int k) { return ((size_t)(k >> 4) * 64 + ((k >> 3) & 1) * 32 + r) * 8 + (k & 7); };
    uint64_t st = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st >> 11) * std::ldexp(1.0, -53); };
    auto run = [&]() -> double {
        HIP_CHECK(hipMemcpy(dev, ha.data(), fb, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dev + fb, hb.data(), fb, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(embed_probe_k, dim3(1), dim3(64), 0, c->stream, reinterpret_cast<const uint4*>(dev), reinterpret_cast<const uint4*>(dev + fb),
                           steps, d_d);
        HIP_CHECK(hipMemcpyAsync(hd, d_d, sizeof hd, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        double worst = 0;
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < 16; ++i) {
                const int col = l & 31, row = (i & 3) + 8 * (i >> 2) + 4 * (l >> 5);
                double ex = 0, mag = 0;
                for (int k = 0; k < K; ++k) { const double t = A[(size_t)row * K + k] * B[(size_t)k * 32 + col]; ex += t; mag += std::fabs(t); }
                worst = std::max(worst, std::fabs((double)hd[l * 16 + i] - ex) / (mag > 0 ? mag : 1.0));
            }
        return worst;
    };
    auto put = [&](int r, int k, int col, float av, float bv) {
        ha[ia(r, k)] = f16_bits(av); hb[ia(col, k)] = f16_bits(bv);
        A[(size_t)r * K + k] = (double)(_Float16)av; B[(size_t)k * 32 + col] = (double)(_Float16)bv;
    };
    double worst = 0;
    // case 1
    for (int k = 0; k < K; ++k)
        for (int r = 0; r < 32; ++r) {
            const float av = (float)((rnd() < 0.5 ? -1 : 1) * std::ldexp(1.0 + rnd(), (int)(rnd() * 25) - 10));
            const float bv = (float)((rnd() < 0.5 ? -1 : 1) * std::ldexp(1.0 + rnd(), (int)(rnd() * 25) - 10));
            put(r, k, r, av, bv);
        }
    worst = std::max(worst, run());
    // case 2: k-steps cycle through hi.hi, hi.lo, lo.hi of activations x 2^8 in [0, 2^11) and weights x 2^w in (-2^15, 2^15)
    for (int k = 0; k < K; ++k)
        for (int r = 0; r < 32; ++r) {
            const float x = (float)(rnd() * 2048.0), w = (float)((rnd() * 2 - 1) * 32768.0);
            const _Float16 xh = (_Float16)x, wh = (_Float16)w;
            const float xl = x - (float)xh, wl = w - (float)wh;
            const int term = (k >> 4) % 3;
            put(r, k, r, term == 2 ? xl : (float)xh, term == 1 ? wl : (float)wh);
        }
    worst = std::max(worst, run());
    (void)hipFree(dev);
    c->emb_pipe_err = worst;
    PVF_REQUIRE(worst <= (double)K * std::ldexp(1.0, -22),
                "embed_probe: v_mfma_f32_32x32x16_f16 does not place or accumulate as the split embedder (conv_tile_k's ConvSplit) assumes on this device");
}

// The 14 residual units: input channels, output channels, down-sampling (a stride-2 `a` layer without padding and the 2 x 2 averaged skip)
static const int UN[14][3] = {{32, 32, 0}, {32, 32, 0}, {32, 32, 0}, {32, 64, 1}, {64, 64, 0}, {64, 64, 0}, {64, 64, 0},
                              {64, 128, 1}, {128, 128, 0}, {128, 128, 0}, {128, 256, 1}, {256, 256, 0}, {256, 256, 0}, {256, 256, 1}};
struct UnitDims { int a, s, o; };                        // sides of the `a` layer's output, of the skip map and of the unit's output
static UnitDims unit_dims(int u, int H)                  // unit u on an input map of side H (the maps are square)
{
    const int a = UN[u][2] ? 1 + (H - 3) / 2 : H, s = UN[u][2] ? 1 + (H - 2) / 2 : H;
    return {a, s, std::max(a, s)};
}

// d_chips: [n][150][150][3] u8 on device; h_out [n][128]; split: the convolutions outside the 32-channel stage in the split form, and
// h_flags[n] = 1 for the faces whose activations left its range
// tap (stage access, or null): the activation after tap->stage is copied to tap->h_out as well; launches, buffers and results are the same
static void resnet_run(Ctx* c, const uint8_t* d_chips, int n, float* h_out, bool split, int* h_flags, const EmbedTap* tap = nullptr)
{
    const EmbedModel& e = c->emb;
    PVF_REQUIRE(e.loaded, "embedder not loaded");
    const int S = e.chip_size;
    const int MAXB = 4096;   // faces per forward: the deep layers (9x9 ... 2x2 maps) have few output rows per face, and a grid of one to two rounds of
                             // blocks leaves half the chip idle in its tail (measured at 1024: 1.2 rounds, matrix pipe 50 % busy); 6 GB of activations
    const int h1 = 1 + (S - 7) / 2;       // 72
    const int hp = 1 + (h1 - 3) / 2;      // 35
    const int cap = std::min(n, MAXB);                   // the arenas grow with the largest batch seen, not to the limit
    const size_t big = (size_t)cap * h1 * h1 * 32;
    c->s_act0.ensure(std::max(big, (size_t)cap * S * S * 4) * sizeof(float));
    c->s_act1.ensure(big * sizeof(float));
    c->s_act2.ensure((size_t)cap * hp * hp * 32 * sizeof(float) + (size_t)cap * 128 * sizeof(float));
    PVF_REQUIRE(!tap || n <= MAXB, "embedder stage access: at most 4096 faces");
    auto tapped = [&](int stage, const float* d, int B, int H, int W, int C) {
        if (tap && tap->stage == stage && tap->h_out)
            HIP_CHECK(hipMemcpyAsync(tap->h_out, d, (size_t)B * H * W * C * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    };
    for (int b0 = 0; b0 < n; b0 += MAXB) {
        const int B = std::min(MAXB, n - b0);
        ProfScope ps(c, "conv");
        float* x = c->s_act0.as<float>();
        float* y = c->s_act1.as<float>();
        float* z = c->s_act2.as<float>();
        // conv1 (straight from the uint8 chips) -> y ; maxpool -> z
        const ConvLayer& L0 = e.convs[0];
        PVF_REQUIRE(S == 150 && L0.cout == 32 && L0.k == 7 && h1 == 72, "stem kernel: 150 x 150 chips, 7 x 7 stride 2, 32 channels");
        if (!c->emb.d_stem) {
            HIP_CHECK(hipMalloc(&c->emb.d_stem, STEM_NP * 64 * sizeof(float)));
            hipLaunchKernelGGL(stem_frag_k, dim3(STEM_NP), dim3(64), 0, c->stream, L0.d_w, c->emb.d_stem);
        }
        hipLaunchKernelGGL(stem_conv_k, dim3(h1 / STEM_ROWS, B), dim3(192), 0, c->stream, d_chips + (size_t)b0 * S * S * 3, B, c->emb.d_stem,
                           L0.d_bias, L0.d_gamma, L0.d_beta, y);
        tapped(0, y, B, h1, h1, 32);
        ConvArgs a;
        const size_t npool = (size_t)B * hp * hp * 32;
        hipLaunchKernelGGL(maxpool3s2_k, dim3((unsigned)((npool + 255) / 256)), dim3(256), 0, c->stream, y, B, h1, h1, 32, z, hp, hp);
        tapped(1, z, B, hp, hp, 32);
        // rotate buffers: cur = z (unit input), t1/t2 scratch
        float* cur = z; float* t1 = x; float* t2 = y;
        int H = hp;
        int* flags = nullptr;
        if (split) {
            flags = c->s_emb_flags.as<int>();
            HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)B * sizeof(int), c->stream));
        }
        for (int u = 0; u < 14; ++u) {
            const int cin = UN[u][0], nn = UN[u][1], down = UN[u][2];
            ConvLayer& La = c->emb.convs[1 + 2 * u];
            ConvLayer& Lb = c->emb.convs[2 + 2 * u];
            const int stride = down ? 2 : 1, pad = down ? 0 : 1;
            const auto [ah, sh, oh] = unit_dims(u, H);
            memset(&a, 0, sizeof a);
            a.in = cur; a.B = B; a.H = H; a.W = H; a.Cin = cin;
            a.out = t1; a.OH = ah; a.OW = ah; a.Cout = nn; a.AH = ah; a.AW = ah; a.ksz = 3; a.stride = stride; a.pad = pad; a.skip_mode = 0;
            conv_bind_weights(c, La, split, false, flags, a);
            launch_conv(c, a);
            tapped(2 + 2 * u, t1, B, ah, ah, nn);
            memset(&a, 0, sizeof a);
            a.in = t1; a.B = B; a.H = ah; a.W = ah; a.Cin = nn;
            a.out = t2; a.OH = oh; a.OW = oh; a.Cout = nn; a.AH = ah; a.AW = ah; a.ksz = 3; a.stride = 1; a.pad = 1;
            a.skip_mode = down ? 2 : 1; a.skip = cur; a.XH = H; a.XW = H; a.XC = cin; a.SH = sh; a.SW = sh;
            conv_bind_weights(c, Lb, split, false, flags, a);
            launch_conv(c, a);
            tapped(3 + 2 * u, t2, B, oh, oh, nn);
            float* old = cur; cur = t2; t2 = old;
            H = oh;
        }
        float* d_out = reinterpret_cast<float*>(c->s_act2.as<uint8_t>() + (size_t)cap * hp * hp * 32 * sizeof(float));
        // cur may alias s_act2's front part; the embedding slot sits behind it
        hipLaunchKernelGGL(head_k, dim3(B), dim3(256), 0, c->stream, cur, H * H, e.d_fc, d_out);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(h_out + (size_t)b0 * 128, d_out, (size_t)B * 128 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (split) HIP_CHECK(hipMemcpyAsync(h_flags + b0, flags, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

// The split forward, then the faces it flagged once more through the exact kernels alone (their descriptors are then the exact path's,
// bit for bit: every kernel computes each face on its own)
void resnet_forward(Ctx* c, const uint8_t* d_chips, int n, float* h_out)
{
    if (!c->emb_split) { resnet_run(c, d_chips, n, h_out, false, nullptr); return; }
    if (!c->emb_probe_done) { embed_probe(c); c->emb_probe_done = true; }
    c->s_emb_flags.ensure((size_t)std::min(n, 4096) * sizeof(int));
    std::vector<int> flags(n, 0);
    resnet_run(c, d_chips, n, h_out, true, flags.data());
    c->emb_split_faces += n;
    std::vector<int> redo;
    for (int i = 0; i < n; ++i) if (flags[i]) redo.push_back(i);
    if (redo.empty()) return;
    c->emb_reruns += (int64_t)redo.size();
    const size_t chip = (size_t)150 * 150 * 3;
    c->s_emb_redo.ensure(redo.size() * chip);
    uint8_t* d = c->s_emb_redo.as<uint8_t>();
    for (size_t j = 0; j < redo.size(); ++j)
        HIP_CHECK(hipMemcpyAsync(d + j * chip, d_chips + (size_t)redo[j] * chip, chip, hipMemcpyDeviceToDevice, c->stream));
    std::vector<float> e(redo.size() * 128);
    resnet_run(c, d, (int)redo.size(), e.data(), false, nullptr);
    for (size_t j = 0; j < redo.size(); ++j) memcpy(h_out + (size_t)redo[j] * 128, e.data() + j * 128, 128 * sizeof(float));
}

// ---- stage access ---------------------------------------------------------------------------------
// The forward as resnet_forward's first pass runs it, with one activation copied out (the faces a split run flags are reported, not
// embedded again: the stages are the split kernels' own)
void resnet_debug_stage(Ctx* c, const uint8_t* d_chips, int n, bool split, EmbedTap* tap, int* h_flags)
{
    PVF_REQUIRE(tap && tap->stage >= 0 && tap->stage < EMB_STAGES, "pvf_debug_embed_stage: stage must be 0..29");
    {
        // dims of every stage, as resnet_run walks them
        int H = 72, C = 32;
        if (tap->stage >= 1) H = 35;
        for (int u = 0; 2 + 2 * u <= tap->stage; ++u) {
            C = UN[u][1];
            const UnitDims d = unit_dims(u, H);
            H = (tap->stage == 2 + 2 * u) ? d.a : d.o;
        }
        tap->dims[0] = H; tap->dims[1] = H; tap->dims[2] = C;
    }
    if (!tap->h_out) return;
    if (split) c->s_emb_flags.ensure((size_t)std::min(n, 4096) * sizeof(int));
    std::vector<float> desc((size_t)n * 128);
    std::vector<int> flags(n, 0);
    resnet_run(c, d_chips, n, desc.data(), split, flags.data(), tap);
    if (h_flags) memcpy(h_flags, flags.data(), (size_t)n * sizeof(int));
}

namespace {
struct Scoped {                                          // device memory of one debug call
    void* p = nullptr;
    explicit Scoped(size_t bytes) { HIP_CHECK(hipMalloc(&p, bytes ? bytes : 4)); }
    ~Scoped() { if (p) (void)hipFree(p); }
    Scoped(const Scoped&) = delete;
    Scoped& operator=(const Scoped&) = delete;
};
struct ScopedLayer {
    ConvLayer L{};
    ~ScopedLayer() { conv_layer_free(L); }
};
struct Drain { Ctx* c; ~Drain() { (void)hipStreamSynchronize(c->stream); } };     // nothing of a debug call is in flight when its memory goes
}

void resnet_debug_conv(Ctx* c, const int32_t* g, const float* in, const float* w, const float* bias, const float* gamma, const float* beta,
                       const float* skip, bool split, bool force_generic, float* out, int32_t* flags)
{
    ConvArgs a;
    memset(&a, 0, sizeof a);
    a.B = g[0]; a.H = g[1]; a.W = g[2]; a.Cin = g[3]; a.OH = g[4]; a.OW = g[5]; a.Cout = g[6]; a.AH = g[7]; a.AW = g[8];
    a.ksz = g[9]; a.stride = g[10]; a.pad = g[11]; a.skip_mode = g[12]; a.XH = g[13]; a.XW = g[14]; a.XC = g[15]; a.SH = g[16]; a.SW = g[17];
    // what keeps every access of the kernels inside the tensors handed in (the shapes the launcher takes are launch_conv's business)
    PVF_REQUIRE(in && w && bias && gamma && beta && out, "pvf_debug_conv: null tensor");
    PVF_REQUIRE(a.B > 0 && a.H > 0 && a.W > 0 && a.Cin > 0 && a.OH > 0 && a.OW > 0 && a.Cout > 0 && a.ksz > 0 && a.ksz <= 7 && a.stride > 0 && a.pad >= 0,
                "pvf_debug_conv: bad dimensions");
    PVF_REQUIRE(a.AH > 0 && a.AW > 0 && a.AH <= a.OH && a.AW <= a.OW, "pvf_debug_conv: the convolution's extent must lie inside the output map");
    PVF_REQUIRE(a.skip_mode >= 0 && a.skip_mode <= 2 && (a.skip_mode == 0 || skip), "pvf_debug_conv: skip_mode must be 0..2, with a skip tensor for 1 and 2");
    const size_t n_in = (size_t)a.B * a.H * a.W * a.Cin, n_out = (size_t)a.B * a.OH * a.OW * a.Cout;
    size_t n_skip = 0;
    if (a.skip_mode == 1) n_skip = n_out;
    if (a.skip_mode == 2) {
        PVF_REQUIRE(a.XH > 0 && a.XW > 0 && a.XC > 0 && a.SH >= 0 && a.SW >= 0 && 2 * a.SH <= a.XH && 2 * a.SW <= a.XW,
                    "pvf_debug_conv: the averaged skip map must lie inside the skip tensor");
        n_skip = (size_t)a.B * a.XH * a.XW * a.XC;
    }
    PVF_REQUIRE(n_in < (1u << 30) && n_out < (1u << 30) && n_skip < (1u << 30), "pvf_debug_conv: tensor too large");
    ScopedLayer sl;
    sl.L.cin = a.Cin; sl.L.cout = a.Cout; sl.L.k = a.ksz; sl.L.stride = a.stride; sl.L.pad = a.pad;
    conv_layer_upload(sl.L, w, bias, gamma, beta);
    Scoped d_in(n_in * sizeof(float)), d_out(n_out * sizeof(float)), d_skip(n_skip * sizeof(float));
    HIP_CHECK(hipMemcpyAsync(d_in.p, in, n_in * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (n_skip) HIP_CHECK(hipMemcpyAsync(d_skip.p, skip, n_skip * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemsetAsync(d_out.p, 0xff, n_out * sizeof(float), c->stream));          // (NaN wherever the kernel does not write)
    int* d_flags = nullptr;
    if (split) {
        c->s_emb_flags.ensure((size_t)a.B * sizeof(int));
        d_flags = c->s_emb_flags.as<int>();
        HIP_CHECK(hipMemsetAsync(d_flags, 0, (size_t)a.B * sizeof(int), c->stream));
    }
    a.in = reinterpret_cast<const float*>(d_in.p); a.out = reinterpret_cast<float*>(d_out.p);
    a.skip = n_skip ? reinterpret_cast<const float*>(d_skip.p) : nullptr;
    Drain drain{c};
    conv_bind_weights(c, sl.L, split, force_generic, d_flags, a);
    launch_conv(c, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, d_out.p, n_out * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (flags) {
        if (a.flags) HIP_CHECK(hipMemcpyAsync(flags, d_flags, (size_t)a.B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        else memset(flags, 0, (size_t)a.B * sizeof(int));
    }
    HIP_CHECK(hipStreamSynchronize(c->stream));
}

void resnet_debug_head(Ctx* c, const float* x, int n, int hw, float* out)
{
    PVF_REQUIRE(c->emb.loaded, "embedder not loaded");
    PVF_REQUIRE(x && out && n > 0 && hw > 0 && (size_t)n * hw < (1u << 22), "pvf_debug_embed_head: bad arguments");
    const size_t n_x = (size_t)n * hw * 256;
    Scoped d_x(n_x * sizeof(float)), d_o((size_t)n * 128 * sizeof(float));
    Drain drain{c};
    HIP_CHECK(hipMemcpyAsync(d_x.p, x, n_x * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(head_k, dim3(n), dim3(256), 0, c->stream, reinterpret_cast<const float*>(d_x.p), hw, c->emb.d_fc, reinterpret_cast<float*>(d_o.p));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, d_o.p, (size_t)n * 128 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
