// render_prims.h -- which output pixels a RECT / LINE / TEXT / REDACT primitive covers (DEMO.md "Primitives", REDACT.md "Covered pixels"): the
// device code render.hip draws a frame's list with, and faces.hip the list of a contact sheet (FACES.md "Sheet").
#pragma once
#include "pvf_internal.h"
#include "render_font.h"

// does the primitive's bounding box meet [x0, x1] x [y0, y1]?  (int64: coordinates are any int32)
template <bool REDACT>
__device__ __forceinline__ bool prim_meets(const pvf_prim& p, int64_t x0, int64_t y0, int64_t x1, int64_t y1)
{
    int64_t l, t, r, b;
    if constexpr (REDACT)
        if (p.type == PVF_PRIM_REDACT) return p.a <= x1 && p.c >= x0 && p.b <= y1 && p.d >= y0;       // an inverted box meets nothing it covers
    if (p.type == PVF_PRIM_RECT) { l = (int64_t)p.a - 1; t = (int64_t)p.b - 1; r = (int64_t)p.c + 1; b = (int64_t)p.d + 1; }
    else if (p.type == PVF_PRIM_LINE) { l = min(p.a, p.c); r = max(p.a, p.c); t = min(p.b, p.d); b = max(p.b, p.d); }
    else { const int64_t s = p.scale; l = p.a; r = l + (int64_t)p.d * 6 * s - 1; b = p.b; t = b - 7 * s + 1; }
    return l <= x1 && r >= x0 && t <= y1 && b >= y0;
}

// is output pixel (X, Y) part of the primitive?  DEMO.md "Primitives", REDACT.md "Covered pixels"
template <bool REDACT>
__device__ __forceinline__ bool prim_covers(const pvf_prim& p, const uint8_t* __restrict__ text, int X, int Y)
{
    if constexpr (REDACT)
        if (p.type == PVF_PRIM_REDACT) {
            if (X < p.a || X > p.c || Y < p.b || Y > p.d) return false;
            if (!((p.colour >> 24) & PVF_REDACT_ELLIPSE)) return true;
            // (2X - (l + r))^2 H^2 + (2Y - (t + b))^2 W^2 <= W^2 H^2: inside the box each square is below 2^28 (sides <= 16384)
            const int64_t W = (int64_t)p.c - p.a + 1, H = (int64_t)p.d - p.b + 1;
            const int64_t ex = 2 * (int64_t)X - ((int64_t)p.a + p.c), ey = 2 * (int64_t)Y - ((int64_t)p.b + p.d);
            return ex * ex * (H * H) + ey * ey * (W * W) <= W * W * (H * H);
        }
    if (p.type == PVF_PRIM_RECT) {
        const int64_t l = p.a, t = p.b, r = p.c, b = p.d;
        const bool outer = X >= l - 1 && X <= r + 1 && Y >= t - 1 && Y <= b + 1;
        const bool inner = X >= l + 1 && X <= r - 1 && Y >= t + 1 && Y <= b - 1;
        return outer && !inner;
    }
    if (p.type == PVF_PRIM_LINE) {
        const int64_t dx = (int64_t)p.c - p.a, dy = (int64_t)p.d - p.b;
        const int64_t adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
        const bool xmajor = adx >= ady;                                   // a tie: x
        const int64_t D = xmajor ? adx : ady, d = xmajor ? ady : adx;
        const int64_t M = xmajor ? X : Y, m = xmajor ? Y : X;
        const int64_t M1 = xmajor ? p.a : p.b, m1 = xmajor ? p.b : p.a;
        const int64_t k = (xmajor ? dx : dy) >= 0 ? M - M1 : M1 - M;       // the major-axis step this pixel would be
        if (k < 0 || k > D) return false;
        int64_t step = 0;                                                  // (2 k d + D) // (2 D)
        if (D > 0) {
            if (D <= 32767) step = (uint32_t)(2 * k * d + D) / (uint32_t)(2 * D);          // 2 k d + D < 2^32
            else {                                                         // k d < 2^64: q + (2 rem >= D), without the doubling
                const uint64_t kd = (uint64_t)k * (uint64_t)d, q = kd / (uint64_t)D, rem = kd % (uint64_t)D;
                step = (int64_t)(q + (rem >= (uint64_t)D - rem ? 1 : 0));
            }
        }
        return m == m1 + ((xmajor ? dy : dx) >= 0 ? step : -step);
    }
    const int64_t s = p.scale;
    const int64_t ex = (int64_t)X - p.a, ey = (int64_t)Y - ((int64_t)p.b - 7 * s + 1);
    if (ex < 0 || ey < 0 || ey >= 7 * s || ex >= (int64_t)p.d * 6 * s) return false;
    const int cx = (int)ex / (int)s, row = (int)ey / (int)s;
    const int gi = cx / 6, col = cx - gi * 6;
    if (col == 5) return false;                                            // the sixth column of the 6 x 8 cell is empty
    const int ch = text[p.c + gi];
    const int g = (ch >= 32 && ch <= 126) ? ch - 32 : '?' - 32;
    return (render_font[g][row] >> (4 - col)) & 1;
}

// ---- colour conversion (DEMO.md "Colour conversion"): what render.hip's render_k and tube.hip's crop_k turn a drawn RGB picture into
// (yoff, Y row, U row, V row) of DEMO.md "Colour conversion": round(c * 65536), chroma rows summing to zero
struct RenderCoef { int32_t yoff, y[3], u[3], v[3]; };
static inline RenderCoef render_coef(int flags)
{
    static const RenderCoef tab[4] = {
        {16, {16829, 33039, 6416}, {-9714, -19070, 28784}, {28784, -24103, -4681}},        // BT.601 limited
        {16, {11966, 40254, 4064}, {-6596, -22188, 28784}, {28784, -26145, -2639}},        // BT.709 limited
        {0, {19595, 38470, 7471}, {-11058, -21710, 32768}, {32768, -27439, -5329}},        // BT.601 full
        {0, {13933, 46871, 4732}, {-7509, -25259, 32768}, {32768, -29763, -3005}},         // BT.709 full
    };
    return tab[(flags & PVF_YUV_BT709 ? 1 : 0) | (flags & PVF_YUV_FULL_RANGE ? 2 : 0)];
}

__device__ __forceinline__ int clip_shift(int v, int shift) { return min(max(v, 0), (256 << shift) - 1) >> shift; }      // clamp first (see yuv_clip8)
// the luma of one pixel
__device__ __forceinline__ int yuv_luma(const RenderCoef& k, int r, int g, int b)
{
    return clip_shift(k.y[0] * r + k.y[1] * g + k.y[2] * b + (k.yoff << 16) + 32768, 16);
}
// one chroma sample from the sums of its 2 x 2 pixels (a pixel past an odd picture's edge is its neighbour, counted again); row: k.u or k.v
__device__ __forceinline__ int yuv_chroma(const int32_t (&row)[3], int sr, int sg, int sb)
{
    return clip_shift(row[0] * sr + row[1] * sg + row[2] * sb + (128 << 18) + (1 << 17), 18);
}
