// strip_sqrt_host_main.cpp -- csrc/strip_sqrt.h (the square root the strip corner kernel takes in its band) as a program of
// its own under the host's sanitizers (test_strip_sqrt_host.py builds and runs it; nothing of the library is linked).
//
// The device seeds sqrt_from_seed with v_sqrt_f32, which is within one ulp of the root.  Here every seed it may return is
// fed: the correctly rounded root and its two neighbours.  For each radicand all three must come back as sqrtf, bit for
// bit: ten million random radicands across the band (uniform in the bit pattern, so every binade gets its share), both ends
// of the band and the floats beside them inside it, exact squares, and the floats one ulp either side of exact squares.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../iceberg_tracking_code_amd/csrc/strip_sqrt.h"

#include <cstdio>
#include <cstdlib>

namespace {

unsigned long long checked = 0;

void check(uint32_t bits)
{
    using namespace icelk;
    if (bits < SQRT_BAND_LO || bits > SQRT_BAND_HI) return;
    const float x = sqrt_float(bits), want = sqrtf(x);
    for (int d = -1; d <= 1; d++) {
        const float seed = sqrt_float(sqrt_bits(want) + (uint32_t)d);
        const float got = sqrt_from_seed(x, seed);
        if (sqrt_bits(got) != sqrt_bits(want)) {
            fprintf(stderr, "strip_sqrt_host_main: x = %a seed = %a: %a, sqrtf %a\n", x, seed, got, want);
            exit(2);
        }
    }
    checked++;
}

}  // namespace

int main(int argc, char** argv)
{
    using namespace icelk;
    const unsigned long long n_random = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
    uint64_t state = 0x9e3779b97f4a7c15ull;
    for (unsigned long long i = 0; i < n_random; i++) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        check(SQRT_BAND_LO + (uint32_t)((state >> 20) % (uint64_t)(SQRT_BAND_HI - SQRT_BAND_LO + 1u)));
    }
    for (uint32_t d = 0; d < 64; d++) {
        check(SQRT_BAND_LO + d);
        check(SQRT_BAND_HI - d);
    }
    // exact squares of 24-bit integers scaled over the band, and their neighbours
    unsigned long long squares = 0;
    for (int e = -48; e <= 31; e++) {
        for (uint32_t m = 1u << 11; m < 1u << 12; m += 1) {          // 12-bit mantissas: m * m is exact in float32
            const float r = ldexpf((float)m, e - 11);
            const uint32_t sq = sqrt_bits(r * r);
            check(sq - 1u);
            check(sq);
            check(sq + 1u);
            squares++;
        }
    }
    printf("radicands checked: %llu (random %llu, squares %llu)\n", checked, n_random, squares);
    return 0;
}
