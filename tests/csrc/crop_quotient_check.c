/* Checks the quotient crop_k (pyannote-video_amd/csrc/tube.hip: exact_quotient) divides a picture's sums by: with sh chosen so that
 * num >> sh fits 32 bits, q = (int)((float)(uint32_t)(num >> sh) * ((float)2^sh / (float)den)), then one step down if the exact residual
 * num - q den is negative and one step up if it reaches den.  Checked: that this is num / den for every divisor the kernel has (den =
 * L^2, 16 <= L <= 2^18, or 1024 S^2, S <= 1024) and numerators below 256.5 den, the multiples of den and their neighbours among them --
 * that is, that the estimate is never more than one off.  Run by tests/test_tube_ref.py. */
#include <stdio.h>
#include <stdint.h>
static uint64_t s = 88172645463325252ull;
static inline uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
static long bad = 0, cases = 0, worst = 0;
static int bitlen(uint64_t v) { int n = 0; while (v) { ++n; v >>= 1; } return n; }
static void one(uint64_t num, uint64_t den)
{
    int sh = bitlen(den) + 9 - 32;
    if (sh < 0) sh = 0;
    const float rden_s = (float)((uint64_t)1 << sh) / (float)den;
    int q = (int)((float)(uint32_t)(num >> sh) * rden_s), steps = 0;
    int64_t r = (int64_t)num - (int64_t)((uint64_t)(uint32_t)q * den);
    if ((num >> sh) >> 32) { printf("num >> sh does not fit: num=%llu den=%llu\n", (unsigned long long)num, (unsigned long long)den); ++bad; }
    if (r < 0) { --q; r += (int64_t)den; ++steps; }
    if (r >= (int64_t)den) { ++q; ++steps; }
    ++cases;
    if (steps > worst) worst = steps;
    if ((uint64_t)q != num / den) { if (bad < 5) printf("bad: num=%llu den=%llu q=%d steps=%d\n", (unsigned long long)num, (unsigned long long)den, q, steps); ++bad; }
}
static void divisor(uint64_t den)
{
    for (int k = 0; k < 256; k += (k < 8 || k > 248) ? 1 : 13) {
        one(k * den, den); one(k * den + 1, den); one(k * den + den - 1, den); one(k * den + den / 2, den);
        one(k * den + rnd() % den, den);
    }
    one(255 * den + den / 2, den);
}
int main(void)
{
    for (uint64_t L = 16; L <= (1u << 18); L += (L < 4200 ? 1 : 1 + rnd() % 97)) divisor(L * L);
    divisor((uint64_t)(1u << 18) * (1u << 18));
    for (uint64_t S = 1; S <= 1024; ++S) divisor(1024 * S * S);
    printf("%ld cases, %ld differ, at most %ld correction steps\n", cases, bad, worst);
    return bad != 0;
}
