// grid_stats_main.cpp -- csrc/grid_stats.h on the host, as a program of its own (nothing of the library in it): the
// text k_grid_std and k_grid_select share with icelk_grid_cell_stats_host, compiled by the host compiler with
// -ffp-contract=off.  Reads segments from a binary file, writes the results' bits; tests/grid_stats_cases.py writes the
// cases and reads the results, tests/test_grid_stats_host.py compares them with numpy itself and runs the program under
// the host's sanitizers.
//
//   in:   int32 ncases, then per case int32 n, float64[n]
//   out:  per case float64 std, median, mad, then float64 lower-middle term, float64 terms <= it (what select_rank found)
// Every segment is held in a buffer of exactly its size, so that a read past its end is seen by AddressSanitizer.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../iceberg_tracking_code_amd/csrc/grid_stats.h"

using namespace icelk;

#define REQUIRE(x)                                                   \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("line %d: %s\n", __LINE__, #x);                   \
            exit(1);                                                 \
        }                                                            \
    } while (0)

struct PlainAt {
    const double* a;
    double operator()(int t) const { return a[t]; }
};

int main(int argc, char** argv)
{
    REQUIRE(argc == 3);
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    REQUIRE(in && out);
    int32_t ncases = 0;
    REQUIRE(fread(&ncases, sizeof ncases, 1, in) == 1);
    long terms = 0;
    for (int k = 0; k < ncases; k++) {
        int32_t n = 0;
        REQUIRE(fread(&n, sizeof n, 1, in) == 1);
        REQUIRE(n >= 0);
        std::vector<double> a((size_t)n);
        if (n) REQUIRE(fread(a.data(), sizeof(double), (size_t)n, in) == (size_t)n);
        const PlainAt at{a.data()};
        double res[5] = {0, 0, 0, 0, 0};
        cell_stats(at, n, &res[0], &res[1], &res[2]);
        bool nan = n == 0;
        for (double x : a) nan = nan || x != x;
        if (!nan) {          // the select on its own: rank and count, for the test to check against a sort
            int count_le = 0;
            res[3] = from_order_key(select_rank(OrderKeyAt<PlainAt>{at}, n, median_rank(n), &count_le));
            res[4] = (double)count_le;
        }
        REQUIRE(fwrite(res, sizeof(double), 5, out) == 5);
        terms += n;
    }
    REQUIRE(fgetc(in) == EOF);
    fclose(in);
    REQUIRE(fclose(out) == 0);
    printf("%d segments, %ld terms\ndone\n", (int)ncases, terms);
    return 0;
}
