// chip_plan.h -- the host geometry of one image chip (dlib chip_details / extract_image_chips): which sub image of the frame the device
// reads, how many pyramid_down<2> levels it builds and the affine chip -> level image.  No HIP here: a host-only program can include it
// (tests/csrc/chip_plan_check.cpp does, under UBSan).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

// chip extraction plan (host geometry -> device pyramid + bilinear), see chip.hip
struct ChipJob {
    // source frame
    const uint8_t* img; int h, w;
    // bounding box of the needed sub image (inclusive), and number of pyramid_down<2> levels to build (0 = sample the frame)
    int bx0, by0, sw, sh, levels;
    // affine chip -> level image
    double m[4], b[2];
    int rows, cols;
    bool empty;
};
struct ChipDetails { double l, t, r, b, cs, sn; int rows, cols; };

inline void rect_down2(double r[4])
{
    r[0] = r[0] / 2.0 - 1.25; r[1] = r[1] / 2.0 - 0.75;
    r[2] = r[2] / 2.0 - 1.25; r[3] = r[3] / 2.0 - 0.75;
}
inline double drect_area(const double r[4]) { return (r[0] > r[2] || r[1] > r[3]) ? 0.0 : (r[2] - r[0]) * (r[3] - r[1]); }
inline void rot(double cx, double cy, double x, double y, double cs, double sn, double* ox, double* oy)
{
    const double dx = x - cx, dy = y - cy;
    *ox = cs * dx - sn * dy + cx;
    *oy = sn * dx + cs * dy + cy;
}
inline ChipJob chip_plan_geom(const uint8_t* img, int h, int w, const ChipDetails& d)
{
    ChipJob j;
    memset(&j, 0, sizeof j);
    j.img = img; j.h = h; j.w = w; j.rows = d.rows; j.cols = d.cols; j.empty = true;
    // collapsed landmarks (68 identical points: a box of zero area) make the similarity fit of face_chip_details 0 / 0: cs and sn are NaN, and
    // every comparison below would let them through to (int)floor(NaN).  The oracle's chip of such details is black: the empty job.
    if (!(std::isfinite(d.l) && std::isfinite(d.t) && std::isfinite(d.r) && std::isfinite(d.b) && std::isfinite(d.cs) && std::isfinite(d.sn))) return j;
    const double size = (double)d.rows * d.cols;
    const double R[4] = {d.l, d.t, d.r, d.b};
    double grow = 2;
    double rect[4] = {R[0], R[1], R[2], R[3]};
    rect_down2(rect);
    while (drect_area(rect) > size) { rect_down2(rect); grow = grow * 2 + 2; }
    const double cx = (R[0] + R[2]) / 2, cy = (R[1] + R[3]) / 2;
    double xs[4], ys[4];
    rot(cx, cy, R[0], R[1], d.cs, d.sn, &xs[0], &ys[0]);
    rot(cx, cy, R[2], R[1], d.cs, d.sn, &xs[1], &ys[1]);
    rot(cx, cy, R[0], R[3], d.cs, d.sn, &xs[2], &ys[2]);
    rot(cx, cy, R[2], R[3], d.cs, d.sn, &xs[3], &ys[3]);
    double bl = xs[0], bt = ys[0], br = xs[0], bb = ys[0];
    for (int i = 1; i < 4; ++i) {
        if (xs[i] < bl) bl = xs[i];
        if (xs[i] > br) br = xs[i];
        if (ys[i] < bt) bt = ys[i];
        if (ys[i] > bb) bb = ys[i];
    }
    bl -= grow; bt -= grow; br += grow; bb += grow;
    if (bl < 0) bl = 0;
    if (bt < 0) bt = 0;
    if (br > w - 1) br = w - 1;
    if (bb > h - 1) bb = h - 1;
    if (bl > br || bt > bb) return j;
    const int bx0 = (int)std::floor(bl + 0.5), by0 = (int)std::floor(bt + 0.5);
    const int bx1 = (int)std::floor(br + 0.5), by1 = (int)std::floor(bb + 0.5);
    const int sw = bx1 - bx0 + 1, sh = by1 - by0 + 1;
    if (sw <= 0 || sh <= 0) return j;
    int level = -1;
    double lr[4] = {R[0] - bx0, R[1] - by0, R[2] - bx0, R[3] - by0};
    for (;;) {
        double nxt[4] = {lr[0], lr[1], lr[2], lr[3]};
        rect_down2(nxt);
        if (!(drect_area(nxt) > size)) break;
        ++level;
        memcpy(lr, nxt, sizeof nxt);
    }
    const double lcx = (lr[0] + lr[2]) / 2, lcy = (lr[1] + lr[3]) / 2;
    double tlx, tly, trx, try_, blx, bly;
    rot(lcx, lcy, lr[0], lr[1], d.cs, d.sn, &tlx, &tly);
    rot(lcx, lcy, lr[2], lr[1], d.cs, d.sn, &trx, &try_);
    rot(lcx, lcy, lr[0], lr[3], d.cs, d.sn, &blx, &bly);
    j.m[0] = (trx - tlx) / (double)(d.cols - 1);
    j.m[2] = (try_ - tly) / (double)(d.cols - 1);
    j.m[1] = (blx - tlx) / (double)(d.rows - 1);
    j.m[3] = (bly - tly) / (double)(d.rows - 1);
    j.b[0] = tlx; j.b[1] = tly;
    j.bx0 = bx0; j.by0 = by0; j.sw = sw; j.sh = sh; j.levels = level + 1;
    j.empty = false;
    return j;
}
