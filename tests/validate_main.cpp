// validate_main.cpp -- the normalised median test's rules (csrc/validate.h: the code the host statement runs and the kernels
// compile) as a program of its own under the host's sanitizers (test_validate_sanitizers_host.py builds and runs it; nothing
// of the library is linked).
//
// It reads the catalogue's binary dump (tests/validate_cases.py: dump) -- the cases and the results the numpy restatement
// expects -- and runs validate::run_host on each.  Every input, working and output array is a heap allocation of exactly its
// stated size -- n doubles, n keys, n bytes, groups x cols x rows records -- so a read or a store outside them is
// AddressSanitizer's to find.  The results must equal the expected ones bit for bit (a NaN matching any NaN), the rejected
// counts must add up to the status bytes, and validate::check must pass every case and refuse what it is documented to.
// One line per case, then the count.
#include "../iceberg_tracking_code_amd/csrc/validate.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace icelk;

namespace {

[[noreturn]] void die(const char* what, int a = 0, int b = 0)
{
    fprintf(stderr, "validate_main: %s (%d, %d)\n", what, a, b);
    exit(2);
}

template <typename T>
struct Exact {   // exactly n elements
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p((T*)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_)
    {
        if (!p) die("out of memory");
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
    void read(FILE* f)
    {
        if (n && fread(p, sizeof(T), n, f) != n) die("the dump ends early");
    }
};

bool same(const double* a, const double* b, size_t n)
{
    for (size_t k = 0; k < n; k++)
        if (!(a[k] != a[k] && b[k] != b[k]) && memcmp(a + k, b + k, sizeof(double))) return false;
    return true;
}

void run_case(FILE* f, int index)
{
    int32_t head[6];
    double geom[5];
    if (fread(head, sizeof head, 1, f) != 1 || fread(geom, sizeof geom, 1, f) != 1) die("the dump ends early", index);
    const int n = head[0], ngroups = head[1];
    const bool has_group = head[2] != 0;
    icelk_validate_lattice_t L{geom[0], geom[1], geom[2], head[3], head[4]};
    icelk_validate_params_t P = validate::default_params();
    P.min_neighbours = head[5], P.threshold = geom[3], P.eps = geom[4];
    if (n < 0 || validate::check(L, P, n, ngroups) != ICELK_OK) die("a case of the catalogue was refused", index);
    const size_t nn = (size_t)n, nseg = (size_t)ngroups * (size_t)L.cols * (size_t)L.rows;
    Exact<double> x(nn), y(nn), u(nn), v(nn), want_r2(nn), r2(nn);
    Exact<int32_t> group(has_group ? nn : 0), want_pool(nseg), pool(nseg), rejected((size_t)ngroups);
    Exact<uint8_t> want_status(nn), status(nn);
    Exact<double> want_mu(nseg), want_mv(nseg), want_du(nseg), want_dv(nseg), mu(nseg), mv(nseg), du(nseg), dv(nseg);
    Exact<unsigned long long> keys(nn);
    x.read(f), y.read(f), u.read(f), v.read(f);
    group.read(f);
    want_status.read(f), want_r2.read(f), want_pool.read(f);
    want_mu.read(f), want_mv.read(f), want_du.read(f), want_dv.read(f);
    const icelk_validate_cells_t cells{pool.p, mu.p, mv.p, du.p, dv.p};
    const int judged = validate::run_host(x.p, y.p, u.p, v.p, n, has_group ? group.p : nullptr, ngroups, L, P, keys.p, status.p, r2.p, &cells,
                                          rejected.p);
    int not_judged = 0, n_rejected = 0, counted = 0;
    for (int p = 0; p < n; p++) not_judged += status.p[p] == validate::kNotJudged, n_rejected += status.p[p] == validate::kRejected;
    for (int g = 0; g < ngroups; g++) counted += rejected.p[g];
    if (judged + not_judged != n || counted != n_rejected) die("counts do not add up", index, judged);
    if (memcmp(status.p, want_status.p, nn)) die("status differs", index);
    if (!same(r2.p, want_r2.p, nn)) die("r2 differs", index);
    if (memcmp(pool.p, want_pool.p, nseg * sizeof(int32_t))) die("pool sizes differ", index);
    if (!same(mu.p, want_mu.p, nseg) || !same(mv.p, want_mv.p, nseg) || !same(du.p, want_du.p, nseg) || !same(dv.p, want_dv.p, nseg))
        die("pool statistics differ", index);
    // without the optional outputs: the same verdicts
    Exact<uint8_t> status2(nn);
    Exact<double> r2b(nn);
    if (validate::run_host(x.p, y.p, u.p, v.p, n, has_group ? group.p : nullptr, ngroups, L, P, keys.p, status2.p, r2b.p, nullptr, nullptr) != judged ||
        memcmp(status.p, status2.p, nn) || !same(r2.p, r2b.p, nn))
        die("the call without records differs", index);
    printf("case %d: %d points, %d judged, %d rejected\n", index, n, judged, n_rejected);
}

int check_refusals()
{
    const icelk_validate_lattice_t L{0.0, 1.0, 1.0, 4, 3};
    const icelk_validate_params_t P = validate::default_params();
    int refused = 0;
    const double bad[] = {0.0, -1.0, NAN, INFINITY};
    for (double b : bad) {
        icelk_validate_params_t Q = P;
        icelk_validate_lattice_t M = L;
        Q.threshold = b;
        refused += validate::check(L, Q, 10, 1) == ICELK_EARG;
        Q = P, Q.eps = b;
        refused += validate::check(L, Q, 10, 1) == ICELK_EARG;
        M.side = b;
        refused += validate::check(M, P, 10, 1) == ICELK_EARG;
    }
    icelk_validate_params_t Q = P;
    Q.min_neighbours = 0;
    refused += validate::check(L, Q, 10, 1) == ICELK_EARG;
    icelk_validate_lattice_t M = L;
    M.cols = 0;
    refused += validate::check(M, P, 10, 1) == ICELK_EARG;
    M = L, M.rows = 0;
    refused += validate::check(M, P, 10, 1) == ICELK_EARG;
    refused += validate::check(L, P, 10, 0) == ICELK_EARG;
    refused += validate::check(L, P, (1LL << 27) + 1, 1) == ICELK_ECAP;
    refused += validate::check(L, P, 1LL << 27, 1) == ICELK_OK;
    M = L, M.cols = 1 << 16, M.rows = 1 << 15;
    refused += validate::check(M, P, 10, 1) == ICELK_ECAP;
    M.cols = 0x7fffffff, M.rows = 0x7fffffff;
    refused += validate::check(M, P, 10, 0x7fffffff) == ICELK_ECAP;
    M = L, M.cols = 0x7fffffff, M.rows = 1;
    refused += validate::check(M, P, 10, 1) == ICELK_OK;
    return refused;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) die("usage: validate_main <dump>");
    FILE* f = fopen(argv[1], "rb");
    if (!f) die("cannot open the dump");
    int32_t cases = 0;
    if (fread(&cases, sizeof cases, 1, f) != 1 || cases < 0) die("no case count");
    for (int k = 0; k < cases; k++) run_case(f, k);
    if (fgetc(f) != EOF) die("bytes behind the last case");
    fclose(f);
    const int refused = check_refusals();
    if (refused != 12 + 9) die("check() answered otherwise than documented", refused);
    printf("refusals: %d\n%d cases\ndone\n", refused, cases);
    return 0;
}
