// chip_plan_check.cpp -- csrc/chip_plan.h on the host, under UBSan with float-cast-overflow (tests/test_ert_edge_cases.py builds and runs
// it): for details that are NaN, infinite, huge, degenerate or ordinary, on frames from 1 x 1 up, the plan is either `empty` or addresses
// only [0, w) x [0, h) with finite coefficients.  Collapsed landmarks (68 identical points) give NaN cs / sn: the empty job, a black chip.
#include <cmath>
#include <cstdio>
#include <initializer_list>
#include <limits>
#include "chip_plan.h"

static int failures = 0, plans = 0, empties = 0;

static void check(const char* what, int h, int w, ChipDetails d)
{
    static const uint8_t pixel = 0;
    const ChipJob j = chip_plan_geom(&pixel, h, w, d);
    ++plans;
    if (j.empty) { ++empties; return; }
    bool ok = j.bx0 >= 0 && j.by0 >= 0 && j.sw >= 1 && j.sh >= 1 && (long)j.bx0 + j.sw <= w && (long)j.by0 + j.sh <= h && j.levels >= 0;
    for (double v : j.m) ok = ok && std::isfinite(v);
    for (double v : j.b) ok = ok && std::isfinite(v);
    if (!ok) {
        ++failures;
        printf("FAIL %s: frame %d x %d, details (%g %g %g %g | %g %g) -> bx0 %d by0 %d sw %d sh %d levels %d m %g %g %g %g b %g %g\n", what, h, w, d.l, d.t,
               d.r, d.b, d.cs, d.sn, j.bx0, j.by0, j.sw, j.sh, j.levels, j.m[0], j.m[1], j.m[2], j.m[3], j.b[0], j.b[1]);
    }
}

static void expect_empty(const char* what, int h, int w, ChipDetails d)
{
    static const uint8_t pixel = 0;
    if (!chip_plan_geom(&pixel, h, w, d).empty) { ++failures; printf("FAIL %s: not empty\n", what); }
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const int sizes[][2] = {{1, 1}, {2, 3}, {5, 1}, {37, 23}, {360, 640}, {1080, 1920}, {2, 1000000}};
    for (const auto& s : sizes) {
        const int h = s[0], w = s[1];
        // what the oracle's face_chip_details gives for 68 identical points: (x, y, x, y, nan, nan)
        for (double x : {100.0, 0.0, -7.0, 2147483647.0, -2147483648.0}) {
            expect_empty("collapsed landmarks", h, w, ChipDetails{x, x, x, x, nan, nan, 150, 150});
            expect_empty("nan cs", h, w, ChipDetails{x, x, x + 50, x + 50, nan, 0.0, 150, 150});
            expect_empty("nan sn", h, w, ChipDetails{x, x, x + 50, x + 50, 1.0, nan, 150, 150});
        }
        const double specials[] = {nan, inf, -inf};
        for (double v : specials)
            for (int field = 0; field < 6; ++field) {
                double f[6] = {10, 10, 60, 60, 1, 0};
                f[field] = v;
                expect_empty("non-finite field", h, w, ChipDetails{f[0], f[1], f[2], f[3], f[4], f[5], 150, 150});
            }
        // finite but extreme: nothing here may leave the frame or overflow an int
        const double big[] = {1e300, 1e18, 4294967296.0, 2147483648.0, 1e6, 1.0, 1e-300, 0.0};
        for (double a : big)
            for (double c : big)
                for (int q = 0; q < 4; ++q) {
                    const double cs = q == 0 ? 1 : q == 1 ? 0 : q == 2 ? std::sqrt(0.5) : -1, sn = q == 0 ? 0 : q == 1 ? 1 : q == 2 ? -std::sqrt(0.5) : 0;
                    check("extreme", h, w, ChipDetails{-a, -c, c, a, cs, sn, 150, 150});
                    check("extreme offset", h, w, ChipDetails{a, a, a + c, a + c, cs, sn, 150, 150});
                    check("extreme inverted", h, w, ChipDetails{c, a, -c, -a, cs, sn, 150, 150});
                    check("extreme tracker chip", h, w, ChipDetails{-a, -c, c, a, cs, sn, 64, 64});
                }
        // ordinary: squares of every size about every place, rotated
        unsigned long long state = 12345;
        auto rnd = [&]() { state = state * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(state >> 11) / 9007199254740992.0; };
        for (int k = 0; k < 20000; ++k) {
            const double side = std::exp(rnd() * 12.0) - 0.5, cx = (rnd() * 3 - 1) * w, cy = (rnd() * 3 - 1) * h, ang = rnd() * 6.283185307179586;
            check("ordinary", h, w, ChipDetails{cx - side / 2, cy - side / 2, cx + side / 2, cy + side / 2, std::cos(ang), std::sin(ang), 150, 150});
        }
    }
    printf("%d plans, %d empty, %d failures\n", plans, empties, failures);
    return failures ? 1 : 0;
}
