// np_sums_main.cpp -- csrc/np_sums.h and csrc/cube_means.h on the host, as a program of its own (nothing of the library
// in it): the text the kernels k_grid_reduce, k_cube_spatial, k_cube_temporal and k_calib_cost run, compiled by the host
// compiler with -ffp-contract=off.  Reads cases from a binary file, writes the results' bits; tests/np_sums_cases.py
// writes the cases and reads the results, tests/test_np_sums_host.py compares them with numpy itself and
// tests/test_np_sums_sanitizers_host.py runs the program under the host's sanitizers.
//
//   in:   int32 ncases, then per case
//           int32 0, int32 n, float64[n]                          -> float64 np_sum, float64 0.0 + np_pairwise_sum
//           int32 1, int32 rows, cols, c, float64[rows * cols]    -> float64[ceil(rows / c) * ceil(cols / c)] block_mean
//   out:  the results one after the other
// Every array is held in a buffer of exactly its size, so that a read past its end is seen by AddressSanitizer.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../iceberg_tracking_code_amd/csrc/cube_means.h"

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

static int32_t read_int(FILE* f)
{
    int32_t v = 0;
    REQUIRE(fread(&v, sizeof v, 1, f) == 1);
    return v;
}

static std::vector<double> read_doubles(FILE* f, size_t n)
{
    std::vector<double> a(n);
    if (n) REQUIRE(fread(a.data(), sizeof(double), n, f) == n);
    return a;
}

int main(int argc, char** argv)
{
    REQUIRE(argc == 3);
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    REQUIRE(in && out);
    const int ncases = read_int(in);
    long sums = 0, fields = 0, cells = 0;
    for (int k = 0; k < ncases; k++) {
        const int kind = read_int(in);
        std::vector<double> res;
        if (kind == 0) {
            const int n = read_int(in);
            REQUIRE(n >= 0);
            const std::vector<double> a = read_doubles(in, (size_t)n);
            res.push_back(np_sum(PlainAt{a.data()}, n));
            res.push_back(0.0 + np_pairwise_sum(PlainAt{a.data()}, n));
            sums++;
        } else {
            REQUIRE(kind == 1);
            const int rows = read_int(in), cols = read_int(in), c = read_int(in);
            REQUIRE(rows >= 1 && cols >= 1 && c >= 1 && c <= kMaxCoarseness);
            const std::vector<double> a = read_doubles(in, (size_t)rows * cols);
            const int cr = (rows + c - 1) / c, cc = (cols + c - 1) / c;      // as launch_cube_spatial has them
            for (int bi = 0; bi < cr; bi++)
                for (int bj = 0; bj < cc; bj++) res.push_back(block_mean(a.data(), rows, cols, c, cc, bi, bj));
            fields++;
            cells += (long)cr * cc;
        }
        REQUIRE(fwrite(res.data(), sizeof(double), res.size(), out) == res.size());
    }
    REQUIRE(fgetc(in) == EOF);
    fclose(in);
    REQUIRE(fclose(out) == 0);
    printf("%ld sums, %ld fields, %ld coarse cells\ndone\n", sums, fields, cells);
    return 0;
}
