// orb.hip -- ORB features and Hamming ratio-test matching of the shot threading (reference pyannote/video/structure/thread.py:139-170:
// cv2.resize + cvtColor + ORB_create().detectAndCompute on two frames per shot, FlannBasedMatcher.knnMatch(k = 2) on every shot pair
// within the lookahead).  ORB.md lists what is recalled from OpenCV 3.4 and what would flip each behaviour; tests/orb_ref.py restates
// the same arithmetic in numpy, and the two agree bit for bit (integer arithmetic, plus float32 Harris / fastAtan2 / pattern rotation
// written in OpenCV's order; -ffp-contract=off).
//
// Extraction, per chunk of frames:
//   orb_level0_k   the small RGB image (INTER_LINEAR, 11-bit coefficients) and its gray value, one lane per level-0 pixel
//   orb_down_k     level k from level k - 1 (INTER_LINEAR_EXACT, 8-bit coefficients), once per level
//   orb_level_k    one workgroup per (frame, level): FAST-9/16 scores, 3 x 3 non-maximum suppression + the 31-pixel image border (ordered
//                  compaction, raster order), retainBest(2 N) on the FAST score (histogram), Harris, retainBest(N) on the response (rank
//                  count: a point stays iff fewer than N responses are larger -- every point tied with the N-th stays), intensity-centroid
//                  angle, 7 x 7 Gaussian blur, rotated BRIEF.  Level images, score maps and candidate lists live in global scratch (L2)
//   orb_pack_k     per frame: the levels' keypoints one after the other (level, then y, then x) into the context's resident ORB set
// Matching: orb_match_k, one workgroup per pair; the train descriptors pass through LDS in chunks, each lane keeps one query row in
// registers with its best and second-best distance; the ratio test and the count are the epilogue.
#include "pvf_internal.h"
#include <cmath>

namespace {

constexpr int kLevels = 8, kEdge = 31, kFastT = 20, kHalf = 15;
constexpr int kMaxSide = 4095;                       // candidates pack (score << 24 | y << 12 | x)

struct Coef { int idx, c0, c1; };
struct Kp { float x, y, level, score, resp, angle; };

struct OrbPlan {
    int nlev;                                         // levels with a usable interior (both sides > 2 * 31)
    int w[kLevels], h[kLevels], quota[kLevels];
    long long off[kLevels];                           // level offset inside a frame's image-sized buffers
    long long coff[kLevels];                          // level offset inside a frame's candidate buffers
    int ccap[kLevels];                                // candidate capacity of a level
    long long P, C;                                   // per-frame sizes of the image-sized / candidate buffers
    int cap;                                          // keypoints per frame (and per level slot)
};

__constant__ int c_umax[kHalf + 1] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
__constant__ int c_gauss[7] = {18, 34, 48, 56, 48, 34, 18};
__constant__ int c_circle[16][2] = {{0, 3}, {1, 3}, {2, 2}, {3, 1}, {3, 0}, {3, -1}, {2, -2}, {1, -3},
                                    {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};

__device__ __forceinline__ int r101(int i, int n) { if (i < 0) i = -i; if (i >= n) i = 2 * n - 2 - i; return i; }

// ---- level 0: cv2.resize(rgb, (ow, oh)) per channel (the arithmetic of pvf_frame_resize), then RGB -> gray
__global__ void __launch_bounds__(256) orb_level0_k(const uint8_t* const* __restrict__ frames, int ih, int iw, const Coef* __restrict__ cx,
                                                    const Coef* __restrict__ cy, uint8_t* __restrict__ pyr, long long P, int ow, int oh)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= ow) return;
    const uint8_t* in = frames[blockIdx.z];
    const Coef a = cx[x], b = cy[y];
    const int sx1 = min(a.idx + 1, iw - 1), sy1 = min(b.idx + 1, ih - 1);
    const uint8_t* r0 = in + (size_t)b.idx * iw * 3;
    const uint8_t* r1 = in + (size_t)sy1 * iw * 3;
    int v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int S0 = r0[3 * a.idx + k] * a.c0 + r0[3 * sx1 + k] * a.c1;
        const int S1 = r1[3 * a.idx + k] * a.c0 + r1[3 * sx1 + k] * a.c1;
        v[k] = (((b.c0 * (S0 >> 4)) >> 16) + ((b.c1 * (S1 >> 4)) >> 16) + 2) >> 2;
    }
    pyr[blockIdx.z * P + (size_t)y * ow + x] = (uint8_t)((v[0] * 4899 + v[1] * 9617 + v[2] * 1868 + 8192) >> 14);
}

// ---- level k from level k - 1: INTER_LINEAR_EXACT (rows into 8 fraction bits, columns into 16, round half up)
__global__ void __launch_bounds__(256) orb_down_k(uint8_t* __restrict__ pyr, long long P, long long src_off, int iw, int ih,
                                                  long long dst_off, int ow, const Coef* __restrict__ cx, const Coef* __restrict__ cy)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= ow) return;
    const uint8_t* src = pyr + blockIdx.z * P + src_off;
    const Coef a = cx[x], b = cy[y];
    const int sx1 = min(a.idx + 1, iw - 1), sy1 = min(b.idx + 1, ih - 1);
    const uint8_t* r0 = src + (size_t)b.idx * iw;
    const uint8_t* r1 = src + (size_t)sy1 * iw;
    const int H0 = r0[a.idx] * a.c0 + r0[sx1] * a.c1;
    const int H1 = r1[a.idx] * a.c0 + r1[sx1] * a.c1;
    pyr[blockIdx.z * P + dst_off + (size_t)y * ow + x] = (uint8_t)((H0 * b.c0 + H1 * b.c1 + 32768) >> 16);
}

// ordered compaction across the workgroup: this lane's slot among the flagged lanes of the 256, in lane order; *total = flagged lanes
__device__ __forceinline__ int block_slot(bool flag, int* wsum, int* total)
{
    const unsigned long long m = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int off = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int s = wsum[w]; off += w < wave ? s : 0; all += s; }
    __syncthreads();
    *total = all;
    return off + __popcll(m & ((1ull << lane) - 1ull));
}

// FAST-9/16 score (0: not a corner): max over the 16 arcs of 9 of min(centre - circle) or min(circle - centre), minus 1
__device__ __forceinline__ int fast_score(const uint8_t* img, int w, int y, int x)
{
    const int v = img[y * w + x];
    int d[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) d[k] = v - img[(y + c_circle[k][1]) * w + x + c_circle[k][0]];
    // a 9-arc holds one of {0, 8} and one of {4, 12}: cheap rejection for both polarities
    const bool dark = (d[0] > kFastT || d[8] > kFastT) && (d[4] > kFastT || d[12] > kFastT);
    const bool bright = (d[0] < -kFastT || d[8] < -kFastT) && (d[4] < -kFastT || d[12] < -kFastT);
    if (!dark && !bright) return 0;
    int best = -1000;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        int mn = d[s], mx = d[s];
#pragma unroll
        for (int j = 1; j < 9; ++j) { const int e = d[(s + j) & 15]; mn = min(mn, e); mx = max(mx, e); }
        best = max(best, max(mn, -mx));
    }
    return best > kFastT ? best - 1 : 0;
}

__device__ float fast_atan2(float y, float x)
{
    const float k180pi = (float)(180.0 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * k180pi, p3 = -0.3258083974640975f * k180pi;
    const float p5 = 0.1555786518463281f * k180pi, p7 = -0.04432655554792128f * k180pi;
    const float eps = (float)2.220446049250313e-16;
    const float ax = fabsf(x), ay = fabsf(y);
    float a;
    if (ax >= ay) {
        const float c = ay / (ax + eps), c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        const float c = ax / (ay + eps), c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

__global__ void __launch_bounds__(256) orb_level_k(const uint8_t* __restrict__ pyr, uint8_t* __restrict__ score, uint16_t* __restrict__ tmp,
                                                   uint8_t* __restrict__ blur, uint32_t* __restrict__ candA, uint32_t* __restrict__ candB,
                                                   float* __restrict__ resp, OrbPlan pl, const int* __restrict__ pattern,
                                                   Kp* __restrict__ slot_kp, uint8_t* __restrict__ slot_desc, int* __restrict__ slot_n)
{
    __shared__ int wsum[4];
    __shared__ int hist[256];
    __shared__ int s_thr;
    const int f = blockIdx.x, lv = blockIdx.y, tid = threadIdx.x;
    const int w = pl.w[lv], h = pl.h[lv], quota = pl.quota[lv], cap = pl.cap;
    const uint8_t* img = pyr + f * pl.P + pl.off[lv];
    uint8_t* S = score + f * pl.P + pl.off[lv];
    uint16_t* T = tmp + f * pl.P + pl.off[lv];
    uint8_t* B = blur + f * pl.P + pl.off[lv];
    uint32_t* cA = candA + f * pl.C + pl.coff[lv];
    uint32_t* cB = candB + f * pl.C + pl.coff[lv];
    float* R = resp + f * pl.C + pl.coff[lv];
    Kp* okp = slot_kp + ((size_t)f * kLevels + lv) * cap;
    uint8_t* odesc = slot_desc + ((size_t)f * kLevels + lv) * cap * 32;

    // 1. FAST scores where the suppression below reads them: [30, w - 30) x [30, h - 30)
    {
        const int rw = w - 2 * (kEdge - 1), rh = h - 2 * (kEdge - 1);
        for (int i = tid; i < rw * rh; i += 256) {
            const int y = kEdge - 1 + i / rw, x = kEdge - 1 + i % rw;
            S[y * w + x] = (uint8_t)fast_score(img, w, y, x);
        }
    }
    for (int i = tid; i < 256; i += 256) hist[i] = 0;
    __syncthreads();
    // 2. non-maximum suppression inside the image border, raster order
    int nA = 0;
    {
        const int rw = w - 2 * kEdge, rh = h - 2 * kEdge;
        for (int base = 0; base < rw * rh; base += 256) {
            const int i = base + tid;
            bool keep = false;
            int s = 0, y = 0, x = 0;
            if (i < rw * rh) {
                y = kEdge + i / rw; x = kEdge + i % rw;
                s = S[y * w + x];
                keep = s > 0;
                for (int dy = -1; dy <= 1 && keep; ++dy)
                    for (int dx = -1; dx <= 1; ++dx)
                        if ((dy || dx) && !(s > S[(y + dy) * w + x + dx])) { keep = false; break; }
            }
            int tot;
            const int slot = block_slot(keep, wsum, &tot);
            if (keep) {
                cA[nA + slot] = ((uint32_t)s << 24) | ((uint32_t)y << 12) | (uint32_t)x;
                atomicAdd(&hist[s], 1);
            }
            nA += tot;
        }
    }
    __syncthreads();
    // 3. retainBest(2 N) on the FAST score: the 2N-th largest score is the threshold, every point at or above it stays
    if (tid == 0) {
        int thr = 0;
        if (nA > 2 * quota) {
            int acc = 0;
            for (thr = 255; thr > 0; --thr) { acc += hist[thr]; if (acc >= 2 * quota) break; }
        }
        s_thr = thr;
    }
    __syncthreads();
    const int thr = s_thr;
    int nB = 0;
    for (int base = 0; base < nA; base += 256) {
        const int i = base + tid;
        const uint32_t c = i < nA ? cA[i] : 0u;
        const bool keep = i < nA && (int)(c >> 24) >= thr;
        int tot;
        const int slot = block_slot(keep, wsum, &tot);
        if (keep) cB[nB + slot] = c;
        nB += tot;
    }
    __syncthreads();
    // 4. Harris responses (block 7, k = 0.04) on the unblurred level
    {
        const float scale = 1.f / ((float)(4 * 7) * 255.f);
        const float ssss = ((scale * scale) * scale) * scale;
        for (int i = tid; i < nB; i += 256) {
            const int y = (cB[i] >> 12) & 4095, x = cB[i] & 4095;
            int a = 0, b = 0, c = 0;
            for (int dy = -3; dy <= 3; ++dy) {
                const uint8_t* p = img + (y + dy) * w + x;
                for (int dx = -3; dx <= 3; ++dx) {
                    const uint8_t* q = p + dx;
                    const int Ix = (q[1] - q[-1]) * 2 + (q[-w + 1] - q[-w - 1]) + (q[w + 1] - q[w - 1]);
                    const int Iy = (q[w] - q[-w]) * 2 + (q[w - 1] - q[-w - 1]) + (q[w + 1] - q[-w + 1]);
                    a += Ix * Ix; b += Iy * Iy; c += Ix * Iy;
                }
            }
            const float fa = (float)a, fb = (float)b, fc = (float)c, s = fa + fb;
            R[i] = (((fa * fb) - (fc * fc)) - ((0.04f * s) * s)) * ssss;
        }
    }
    __syncthreads();
    // 5. retainBest(N) on the response; the survivors go to this level's slot in raster order
    int nF = 0;
    for (int base = 0; base < nB; base += 256) {
        const int i = base + tid;
        bool keep = i < nB;
        if (keep && nB > quota) {
            const float r = R[i];
            int above = 0;
            for (int j = 0; j < nB && above < quota; ++j) above += R[j] > r;
            keep = above < quota;
        }
        int tot;
        const int slot = block_slot(keep, wsum, &tot);
        if (keep && nF + slot < cap) {
            const uint32_t c = cB[i];
            Kp k;
            k.x = (float)(c & 4095); k.y = (float)((c >> 12) & 4095); k.level = (float)lv; k.score = (float)(c >> 24);
            k.resp = R[i]; k.angle = 0.f;
            okp[nF + slot] = k;
        }
        nF += tot;
    }
    if (tid == 0) slot_n[f * kLevels + lv] = nF;                 // > cap: reported by the host as an error
    nF = min(nF, cap);
    if (nF == 0) return;                                          // (uniform)
    __syncthreads();
    // 6. intensity-centroid angle over the radius-15 disc
    for (int i = tid; i < nF; i += 256) {
        const int x = (int)okp[i].x, y = (int)okp[i].y;
        const uint8_t* c0 = img + y * w + x;
        int m10 = 0, m01 = 0;
        for (int u = -kHalf; u <= kHalf; ++u) m10 += u * c0[u];
        for (int v = 1; v <= kHalf; ++v) {
            const int d = c_umax[v];
            int vs = 0;
            for (int u = -d; u <= d; ++u) {
                const int p = c0[u + v * w], m = c0[u - v * w];
                vs += p - m;
                m10 += u * (p + m);
            }
            m01 += v * vs;
        }
        okp[i].angle = fast_atan2((float)m01, (float)m10);
    }
    // 7. GaussianBlur(7 x 7, sigma 2), reflect-101: rows (8 fraction bits), then columns (round half up from 16 fraction bits)
    for (int i = tid; i < w * h; i += 256) {
        const int y = i / w, x = i - y * w;
        int acc = 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) acc += c_gauss[j] * img[y * w + r101(x + j - 3, w)];
        T[i] = (uint16_t)acc;
    }
    __syncthreads();
    for (int i = tid; i < w * h; i += 256) {
        const int y = i / w, x = i - y * w;
        int acc = 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) acc += c_gauss[j] * (int)T[r101(y + j - 3, h) * w + x];
        B[i] = (uint8_t)((acc + 32768) >> 16);
    }
    __syncthreads();
    // 8. rotated BRIEF: lane = (keypoint, byte), 8 comparisons of rotated pattern points on the blurred level
    for (int i = tid; i < nF * 32; i += 256) {
        const int kp = i >> 5, byte = i & 31;
        const Kp k = okp[kp];
        const int x = (int)k.x, y = (int)k.y;
        const float ang = k.angle * (float)(3.14159265358979323846 / 180.f);
        const float ca = (float)cos((double)ang), sa = (float)sin((double)ang);
        const uint8_t* c0 = B + y * w + x;
        int val = 0;
        for (int b = 0; b < 8; ++b) {
            int t[2];
            for (int e = 0; e < 2; ++e) {
                const int pi = 2 * (16 * byte + 2 * b + e);
                const float px = (float)pattern[pi], py = (float)pattern[pi + 1];
                const int ix = (int)rintf(px * ca - py * sa), iy = (int)rintf(px * sa + py * ca);
                t[e] = c0[iy * w + ix];
            }
            val |= (t[0] < t[1]) << b;
        }
        odesc[(size_t)kp * 32 + byte] = (uint8_t)val;
    }
}

// per frame: its levels one after the other into rows [frame * cap, ...) of the resident set; counts[frame] = -(rows the frame needs)
// when they do not fit
__global__ void __launch_bounds__(256) orb_pack_k(const Kp* __restrict__ slot_kp, const uint8_t* __restrict__ slot_desc,
                                                  const int* __restrict__ slot_n, int nlev, int cap, int first, Kp* __restrict__ kp_out,
                                                  uint8_t* __restrict__ desc_out, int* __restrict__ counts)
{
    const int f = blockIdx.x;
    int start[kLevels + 1];
    start[0] = 0;
    bool over = false;
    for (int l = 0; l < kLevels; ++l) {
        const int n = l < nlev ? slot_n[f * kLevels + l] : 0;
        over |= n > cap;
        start[l + 1] = start[l] + n;
    }
    over |= start[kLevels] > cap;
    const size_t row0 = (size_t)(first + f) * cap;
    if (threadIdx.x == 0) counts[first + f] = over ? -start[kLevels] : start[kLevels];
    if (over) return;
    for (int i = threadIdx.x; i < start[kLevels]; i += 256) {
        int l = 0;
        while (i >= start[l + 1]) ++l;
        const size_t src = ((size_t)f * kLevels + l) * cap + (i - start[l]);
        kp_out[row0 + i] = slot_kp[src];
        const uint4* s = reinterpret_cast<const uint4*>(slot_desc + src * 32);
        uint4* d = reinterpret_cast<uint4*>(desc_out + (row0 + i) * 32);
        d[0] = s[0]; d[1] = s[1];
    }
}

// ---- matching: counts[p] = rows of set a whose two nearest rows of set b (Hamming) pass 10 d1 < 7 d2; 0 if either set has < 2 rows
constexpr int kTrainChunk = 1024;                      // train rows per LDS pass (32 KB)
__global__ void __launch_bounds__(256) orb_match_k(const uint8_t* __restrict__ desc, const int* __restrict__ nrows, int cap,
                                                   const int* __restrict__ pairs, int* __restrict__ out)
{
    __shared__ uint4 tb[kTrainChunk][2];
    __shared__ int s_count;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int a = pairs[2 * p], b = pairs[2 * p + 1];
    const int na = nrows[a], nb = nrows[b];
    if (na < 2 || nb < 2) { if (tid == 0) out[p] = 0; return; }           // (uniform)
    if (tid == 0) s_count = 0;
    const uint4* A = reinterpret_cast<const uint4*>(desc + (size_t)a * cap * 32);
    const uint4* Bd = reinterpret_cast<const uint4*>(desc + (size_t)b * cap * 32);
    for (int q0 = 0; q0 < na; q0 += 256) {
        const int q = q0 + tid;
        uint4 x0 = make_uint4(0, 0, 0, 0), x1 = x0;
        if (q < na) { x0 = A[2 * q]; x1 = A[2 * q + 1]; }
        int d1 = 1 << 20, d2 = 1 << 20;
        for (int t0 = 0; t0 < nb; t0 += kTrainChunk) {
            const int nt = min(kTrainChunk, nb - t0);
            __syncthreads();
            for (int i = tid; i < 2 * nt; i += 256) tb[i >> 1][i & 1] = Bd[2 * t0 + i];
            __syncthreads();
            if (q < na) {
                for (int t = 0; t < nt; ++t) {
                    const uint4 y0 = tb[t][0], y1 = tb[t][1];
                    const int d = __popc(x0.x ^ y0.x) + __popc(x0.y ^ y0.y) + __popc(x0.z ^ y0.z) + __popc(x0.w ^ y0.w) +
                                  __popc(x1.x ^ y1.x) + __popc(x1.y ^ y1.y) + __popc(x1.z ^ y1.z) + __popc(x1.w ^ y1.w);
                    if (d < d1) { d2 = d1; d1 = d; }
                    else if (d < d2) d2 = d;
                }
            }
        }
        const bool pass = q < na && 10 * d1 < 7 * d2;
        const unsigned long long m = __ballot(pass);
        if ((tid & 63) == 0 && m) atomicAdd(&s_count, (int)__popcll(m));
    }
    __syncthreads();
    if (tid == 0) out[p] = s_count;
}

// INTER_LINEAR (11-bit, float fraction) and INTER_LINEAR_EXACT (8-bit, double fraction) coefficient tables
void linear_coefs(int in, int out, std::vector<Coef>& c)
{
    c.resize(out);
    const double scale = (double)in / out;
    for (int d = 0; d < out; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= (float)s;
        if (s < 0) { f = 0; s = 0; }
        if (s >= in - 1) { f = 0; s = in - 1; }
        c[d].idx = s;
        c[d].c0 = (int)(short)nearbyintf((1.f - f) * 2048.f);
        c[d].c1 = (int)(short)nearbyintf(f * 2048.f);
    }
}

void exact_coefs(int in, int out, std::vector<Coef>& c)
{
    c.resize(out);
    const double scale = (double)in / out;
    for (int d = 0; d < out; ++d) {
        const double fx = (d + 0.5) * scale - 0.5;
        const int s = (int)std::floor(fx);
        if (s < 0) c[d] = {0, 256, 0};
        else if (s >= in - 1) c[d] = {in - 1, 256, 0};
        else { const int c1 = (int)std::nearbyint((fx - s) * 256.0); c[d] = {s, 256 - c1, c1}; }
    }
}

// makeRandomPattern: RNG(0x34985739), uniform in [-15, 16), x then y, 512 points
std::vector<int> random_pattern()
{
    std::vector<int> p(1024);
    uint64_t state = 0x34985739ull;
    for (int i = 0; i < 1024; ++i) {
        state = (uint64_t)(uint32_t)state * 4164903690ull + (state >> 32);
        p[i] = (int)((uint32_t)state % 31u) - kHalf;
    }
    return p;
}

size_t al(size_t n) { return (n + 255) / 256 * 256; }

}  // namespace

std::vector<int> orb_level_quota()
{
    const float factor = (float)(1.0 / 1.2);
    float want = 500.f * (1.f - factor) / (1.f - (float)std::pow((double)factor, (double)kLevels));
    std::vector<int> q(kLevels);
    int sum = 0;
    for (int l = 0; l < kLevels - 1; ++l) { q[l] = (int)nearbyintf(want); sum += q[l]; want *= factor; }
    q[kLevels - 1] = std::max(500 - sum, 0);
    return q;
}

// the resident set in s_orb_set: [n][cap] descriptors and keypoints, then the counts.  orb_extract writes it and orb_match_counts finds
// the descriptors and counts again through the same function (a layout is a function of its arguments alone)
struct OrbSetLayout { ScratchLayout lay; ScratchSlot<uint8_t> desc; ScratchSlot<Kp> kp; ScratchSlot<int> cnt; };
static OrbSetLayout orb_set_layout(int n, int cap)
{
    OrbSetLayout s;
    s.desc = s.lay.take<uint8_t>((size_t)n * cap * 32); s.kp = s.lay.take<Kp>((size_t)n * cap); s.cnt = s.lay.take<int>(n);
    return s;
}

void orb_extract(Ctx* c, const std::vector<Frame>& frames, int ow, int oh, int cap, int32_t* counts, float* kp_out, uint8_t* desc_out)
{
    const int n = (int)frames.size();
    c->orb_n = 0;                                             // a refused or failed call leaves no resident set behind
    PVF_REQUIRE(n >= 1 && ow >= 1 && oh >= 1 && ow <= kMaxSide && oh <= kMaxSide, "orb: at least one frame and a small image of at most 4095 x 4095");
    PVF_REQUIRE(cap >= 1 && cap <= 65536, "orb: cap (keypoints per frame) in [1, 65536]");
    const int ih = frames[0].h, iw = frames[0].w;
    for (const Frame& f : frames) PVF_REQUIRE(f.h == ih && f.w == iw, "orb: frames of one size");
    OrbPlan pl{};
    pl.cap = cap;
    const std::vector<int> quota = orb_level_quota();
    std::vector<std::vector<Coef>> cx(kLevels), cy(kLevels);
    long long P = 0, C = 0;
    int nlev = 0;
    for (int l = 0; l < kLevels; ++l) {
        const float s = 1.f / (float)std::pow(1.2, (double)l);
        const int lw = l ? (int)nearbyintf((float)ow * s) : ow, lh = l ? (int)nearbyintf((float)oh * s) : oh;
        if (lw <= 2 * kEdge || lh <= 2 * kEdge) break;        // no interior (runByImageBorder empties it), nor at any coarser level
        pl.w[l] = lw; pl.h[l] = lh; pl.quota[l] = quota[l];
        pl.off[l] = P; P += (long long)al((size_t)lw * lh);
        pl.ccap[l] = lw * lh / 2 + 64;                       // strict 3 x 3 suppression: no two candidates touch
        pl.coff[l] = C; C += (long long)al((size_t)pl.ccap[l]);
        if (l == 0) { linear_coefs(iw, ow, cx[0]); linear_coefs(ih, oh, cy[0]); }
        else { exact_coefs(pl.w[l - 1], lw, cx[l]); exact_coefs(pl.h[l - 1], lh, cy[l]); }
        nlev = l + 1;
    }
    pl.nlev = nlev; pl.P = P; pl.C = C;
    const OrbSetLayout set = orb_set_layout(n, cap);
    c->s_orb_set.ensure(set.lay.bytes());
    uint8_t* d_desc = set.desc.in(c->s_orb_set); Kp* d_kp = set.kp.in(c->s_orb_set); int* d_cnt = set.cnt.in(c->s_orb_set);
    c->orb_n = 0; c->orb_cap = cap;
    if (nlev == 0) {
        HIP_CHECK(hipMemsetAsync(d_cnt, 0, (size_t)n * 4, c->stream));
    } else {
        // tables: coefficients of every level, then the pattern
        std::vector<Coef> tab;
        std::vector<size_t> tx(kLevels), ty(kLevels);
        for (int l = 0; l < nlev; ++l) { tx[l] = tab.size(); tab.insert(tab.end(), cx[l].begin(), cx[l].end()); ty[l] = tab.size(); tab.insert(tab.end(), cy[l].begin(), cy[l].end()); }
        const std::vector<int> pat = random_pattern();
        const int chunk = (int)std::max<long long>(1, std::min<long long>(n, (1ll << 30) / (P * 5 + C * 12 + (long long)kLevels * cap * (sizeof(Kp) + 32))));
        const size_t cP = (size_t)chunk * P, cC = (size_t)chunk * C, cK = (size_t)chunk * kLevels * cap;
        ScratchLayout lay;
        const auto sTab = lay.take<Coef>(tab.size()); const auto sPat = lay.take<int>(pat.size()); const auto sPtr = lay.take<const uint8_t*>(n);
        const auto sPyr = lay.take<uint8_t>(cP), sScore = lay.take<uint8_t>(cP), sBlur = lay.take<uint8_t>(cP); const auto sTmp = lay.take<uint16_t>(cP);
        const auto sCa = lay.take<uint32_t>(cC), sCb = lay.take<uint32_t>(cC); const auto sResp = lay.take<float>(cC);
        const auto sSkp = lay.take<Kp>(cK); const auto sSdesc = lay.take<uint8_t>(cK * 32); const auto sSn = lay.take<int>((size_t)chunk * kLevels);
        lay.pad(8 * 256);                                     // stood for the rounding of the pieces, which take() now counts; kept so that the buffer does not shrink
        c->s_misc.ensure(lay.bytes());
        Coef* d_tab = sTab.in(c->s_misc); int* d_pat = sPat.in(c->s_misc); const uint8_t** d_ptr = sPtr.in(c->s_misc);
        uint8_t* d_pyr = sPyr.in(c->s_misc); uint8_t* d_score = sScore.in(c->s_misc); uint8_t* d_blur = sBlur.in(c->s_misc); uint16_t* d_tmp = sTmp.in(c->s_misc);
        uint32_t* d_ca = sCa.in(c->s_misc); uint32_t* d_cb = sCb.in(c->s_misc); float* d_resp = sResp.in(c->s_misc);
        Kp* d_skp = sSkp.in(c->s_misc); uint8_t* d_sdesc = sSdesc.in(c->s_misc); int* d_sn = sSn.in(c->s_misc);
        std::vector<const uint8_t*> ptrs(n);
        for (int i = 0; i < n; ++i) ptrs[i] = frames[i].d;
        HIP_CHECK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(Coef), hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipMemcpyAsync(d_pat, pat.data(), pat.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipMemcpyAsync(d_ptr, ptrs.data(), ptrs.size() * sizeof(void*), hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));           // (host vectors go out of scope)
        ProfScope ps(c, "orb");
        for (int f0 = 0; f0 < n; f0 += chunk) {
            const int nc = std::min(chunk, n - f0);
            hipLaunchKernelGGL(orb_level0_k, dim3((ow + 255) / 256, oh, nc), dim3(256), 0, c->stream, d_ptr + f0, ih, iw, d_tab + tx[0], d_tab + ty[0],
                               d_pyr, P, ow, oh);
            for (int l = 1; l < nlev; ++l)
                hipLaunchKernelGGL(orb_down_k, dim3((pl.w[l] + 255) / 256, pl.h[l], nc), dim3(256), 0, c->stream, d_pyr, P, pl.off[l - 1], pl.w[l - 1],
                                   pl.h[l - 1], pl.off[l], pl.w[l], d_tab + tx[l], d_tab + ty[l]);
            hipLaunchKernelGGL(orb_level_k, dim3(nc, nlev), dim3(256), 0, c->stream, d_pyr, d_score, d_tmp, d_blur, d_ca, d_cb, d_resp, pl, d_pat,
                               d_skp, d_sdesc, d_sn);
            hipLaunchKernelGGL(orb_pack_k, dim3(nc), dim3(256), 0, c->stream, d_skp, d_sdesc, d_sn, nlev, cap, f0, d_kp, d_desc, d_cnt);
            HIP_CHECK(hipGetLastError());
        }
    }
    std::vector<int32_t> cnt(n);
    HIP_CHECK(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    if (counts) memcpy(counts, cnt.data(), (size_t)n * 4);            // (also on the error below: -needed marks the frames that do not fit)
    int first_over = -1, need = 0;
    for (int i = 0; i < n; ++i)
        if (cnt[i] < 0) { if (first_over < 0) first_over = i; need = std::max(need, -cnt[i]); }
    if (first_over >= 0) {
        char b[256];
        snprintf(b, sizeof b, "orb: frame %d has %d keypoints (ties of retainBest included), more than cap = %d; the largest frame needs cap >= %d: "
                 "call again with a larger cap", first_over, -cnt[first_over], cap, need);
        throw PvfError(b);
    }
    if (kp_out) HIP_CHECK(hipMemcpy(kp_out, d_kp, (size_t)n * cap * sizeof(Kp), hipMemcpyDeviceToHost));
    if (desc_out) HIP_CHECK(hipMemcpy(desc_out, d_desc, (size_t)n * cap * 32, hipMemcpyDeviceToHost));
    c->orb_n = n;
}

void orb_match_counts(Ctx* c, const uint8_t* desc, const int32_t* nrows, int n_sets, int cap, const int32_t* pairs, int64_t n_pairs, int32_t* out)
{
    PVF_REQUIRE(n_pairs >= 0 && n_pairs <= (1ll << 31) - 1 && (n_pairs == 0 || (pairs && out)), "orb match: pairs and an output array");
    const bool resident = desc == nullptr;
    if (resident) {
        PVF_REQUIRE(c->orb_n > 0, "orb match: no descriptors given and no pvf_orb_extract result on this context");
        n_sets = c->orb_n; cap = c->orb_cap;
    } else {
        PVF_REQUIRE(nrows && n_sets >= 1 && cap >= 1, "orb match: descriptors, their row counts, n_sets and cap");
        for (int i = 0; i < n_sets; ++i) PVF_REQUIRE(nrows[i] >= 0 && nrows[i] <= cap, "orb match: a row count outside [0, cap]");
    }
    for (int64_t p = 0; p < 2 * n_pairs; ++p) PVF_REQUIRE(pairs[p] >= 0 && pairs[p] < n_sets, "orb match: a pair names a set that does not exist");
    if (n_pairs == 0) return;
    ScratchLayout lay;
    const auto sPairs = lay.take<int>((size_t)n_pairs * 2), sOut = lay.take<int>(n_pairs);
    const auto sDesc = lay.take<uint8_t>(resident ? 0 : (size_t)n_sets * cap * 32);       // the sets of this call, when it brings its own
    const auto sN = lay.take<int>(resident ? 0 : n_sets);
    lay.pad(256);                                             // reason unknown, kept
    c->s_orb_work.ensure(lay.bytes());
    int* d_pairs = sPairs.in(c->s_orb_work); int* d_out = sOut.in(c->s_orb_work);
    const uint8_t* d_desc;
    const int* d_n;
    if (resident) {
        const OrbSetLayout set = orb_set_layout(c->orb_n, c->orb_cap);
        d_desc = set.desc.in(c->s_orb_set); d_n = set.cnt.in(c->s_orb_set);
    } else {
        uint8_t* dd = sDesc.in(c->s_orb_work); int* dn = sN.in(c->s_orb_work);
        HIP_CHECK(hipMemcpyAsync(dd, desc, (size_t)n_sets * cap * 32, hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipMemcpyAsync(dn, nrows, (size_t)n_sets * 4, hipMemcpyHostToDevice, c->stream));
        d_desc = dd; d_n = dn;
    }
    HIP_CHECK(hipMemcpyAsync(d_pairs, pairs, (size_t)n_pairs * 8, hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, "orb_match");
        hipLaunchKernelGGL(orb_match_k, dim3((unsigned)n_pairs), dim3(256), 0, c->stream, d_desc, d_n, cap, d_pairs, d_out);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipMemcpyAsync(out, d_out, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
