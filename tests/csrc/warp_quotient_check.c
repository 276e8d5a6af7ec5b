/* warp_k (csrc/tube.hip) divides v < 2^16 by d = K^2 <= 256 as (uint32)(((uint64) v * M) >> 24) with M = 2^24 / d + 1.
 * v M / 2^24 = v / d + v e / (d 2^24) with e = M d - 2^24 in 1 .. d; v e < 2^24, so the excess stays below 1 / d, the least distance
 * from v / d to the next integer.  This runs the same arithmetic for all 256 divisors over the whole range of v. */
#include <stdint.h>
#include <stdio.h>

static uint32_t warp_quotient(uint32_t v, uint32_t M) { return (uint32_t)(((uint64_t)v * M) >> 24); }

int main(void)
{
    long differ = 0, checked = 0;
    int divisors = 0;
    for (uint32_t d = 1; d <= 256; ++d, ++divisors) {
        const uint32_t M = ((uint32_t)1 << 24) / d + 1u;
        for (uint32_t v = 0; v < 65536; ++v, ++checked)
            if (warp_quotient(v, M) != v / d) {
                if (differ++ < 5) printf("d %u v %u: %u, not %u\n", d, v, warp_quotient(v, M), v / d);
            }
    }
    printf("%d divisors, %ld quotients, %ld differ\n", divisors, checked, differ);
    return differ != 0;
}
