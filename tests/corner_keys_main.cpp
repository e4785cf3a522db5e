// corner_keys_main.cpp -- csrc/corner_keys.h on the host, as a program of its own (nothing of the library in it): the
// response key, the candidate key and the quality threshold that the corner detector's kernels share, compiled by the
// host compiler with -ffp-contract=off.  Reads cases from a binary file and writes the results as uint32 words;
// tests/test_corner_keys_host.py writes the cases and compares the results with numpy.
//
//   in:   int32 n, uint32[n] float bit patterns        -> per pattern: ordered_key, bits of key_to_float(ordered_key)
//         int32 n, n x {uint32 bits, int32 x, int32 y} -> per case: cand_key low word, high word, cand_response_key,
//                                                         cand_x, cand_y, cand_xy
//         int32 n, n x {uint32 max_key, float64 q}     -> per case: bits of quality_threshold(max_key, q)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../iceberg_tracking_code_amd/csrc/corner_keys.h"

using namespace icelk;

#define REQUIRE(x)                                                   \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("line %d: %s\n", __LINE__, #x);                   \
            exit(1);                                                 \
        }                                                            \
    } while (0)

template <typename T>
static T get(FILE* f)
{
    T v;
    REQUIRE(fread(&v, sizeof v, 1, f) == 1);
    return v;
}

static void put(FILE* f, uint32_t v) { REQUIRE(fwrite(&v, sizeof v, 1, f) == 1); }

static float as_float(uint32_t b)
{
    float v;
    memcpy(&v, &b, sizeof v);
    return v;
}
static uint32_t as_bits(float v)
{
    uint32_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

int main(int argc, char** argv)
{
    REQUIRE(argc == 3);
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    REQUIRE(in && out);
    int n = get<int32_t>(in);
    for (int i = 0; i < n; i++) {
        const unsigned key = ordered_key(as_float(get<uint32_t>(in)));
        put(out, key);
        put(out, as_bits(key_to_float(key)));
    }
    n = get<int32_t>(in);
    for (int i = 0; i < n; i++) {
        const float response = as_float(get<uint32_t>(in));
        const int x = get<int32_t>(in), y = get<int32_t>(in);
        const unsigned long long key = cand_key(response, x, y);
        put(out, (uint32_t)key);
        put(out, (uint32_t)(key >> 32));
        put(out, cand_response_key(key));
        put(out, (uint32_t)cand_x(key));
        put(out, (uint32_t)cand_y(key));
        put(out, cand_xy(key));
    }
    n = get<int32_t>(in);
    for (int i = 0; i < n; i++) {
        const uint32_t max_key = get<uint32_t>(in);
        const double quality = get<double>(in);
        put(out, as_bits(quality_threshold(max_key, quality)));
    }
    REQUIRE(fclose(out) == 0);
    printf("done\n");
    return 0;
}
