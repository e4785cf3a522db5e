// abi_validate.hip -- the normalised median test between projection and gridding.  The rules are
// validate.h's, the kernels k_validate.hip's.
//
//   host    icelk_validate_host: validate.h on the CPU; no handle, re-entrant
//   device  icelk_validate: the caller's points and groups up, assign, the judged count back (the one wait in the middle, as
//           the gridder's: the sort takes its length from the host), sort, pools, judge, status / r2 / records down.
//           validate_run is that chain without the copies; the validated day gridder (abi_post.hip) runs it on the points it
//           has uploaded for the gridder, with the day tables' windows as groups.
// Every argument is checked before anything is allocated; a refusal leaves the handle as it was.
#include <vector>

#include "icelk_ctx.h"
#include "validate.h"

namespace icelk {

void ValidateDev::alloc(DevBufs& B, int n, int ngroups, const icelk_validate_lattice_t& L, const icelk_validate_params_t& P, hipStream_t s)
{
    nseg = (size_t)ngroups * (size_t)L.cols * (size_t)L.rows;
    A.n = n, A.ngroups = ngroups, A.L = L, A.P = P;
    A.keys = B.get<unsigned long long>((size_t)n);
    keys_sorted = B.get<unsigned long long>((size_t)n);
    A.key_count = B.get<int>(1);
    A.status = B.get<uint8_t>((size_t)n);
    A.r2 = B.get<double>((size_t)n);
    A.cells.pool_n = B.get<int32_t>(nseg);
    for (double** q : {&A.cells.med_u, &A.cells.med_v, &A.cells.mad_u, &A.cells.mad_v}) *q = B.get<double>(nseg);
    A.rejected = B.get<int32_t>((size_t)ngroups);
    for (key_bits = 33; (1LL << (key_bits - 32)) < (long long)nseg;) key_bits++;
    sort_tmp_bytes = sort_keys_asc(s, nullptr, 0, A.keys, keys_sorted, n, key_bits);
    sort_tmp = B.get<uint8_t>(sort_tmp_bytes);
}

int validate_run(Ctx* c, ValidateDev& V, const std::function<void()>& assign, EvPair* t)
{
    const hipStream_t s = c->stream;
    ValidateArgs& A = V.A;
    HIPCHK(c, hipMemsetAsync(A.key_count, 0, sizeof(int), s));
    HIPCHK(c, hipMemsetAsync(A.rejected, 0, sizeof(int32_t) * (size_t)A.ngroups, s));
    if (t) HIPCHK(c, hipEventRecord(t[0].a, s));
    {
        ProfScope p(c, K_VALIDATE_ASSIGN);
        assign();
    }
    if (int rc = check_launch(c, "validate_assign")) return rc;
    if (t) HIPCHK(c, hipEventRecord(t[0].b, s));
    int total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, A.key_count, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (total < 0 || total > A.n) FAIL(c, ICELK_EHIP, "validate: more keys than points");
    if (t) HIPCHK(c, hipEventRecord(t[1].a, s));
    A.sorted = A.keys;
    if (total > 1) {
        sort_keys_asc(s, V.sort_tmp, V.sort_tmp_bytes, A.keys, V.keys_sorted, total, V.key_bits);
        if (int rc = check_launch(c, "validate sort")) return rc;
        A.sorted = V.keys_sorted;
    }
    {
        ProfScope p(c, K_VALIDATE_POOLS);
        launch_validate_pools(s, A, total);
    }
    {
        ProfScope p(c, K_VALIDATE_JUDGE);
        launch_validate_judge(s, A, total);
    }
    if (int rc = check_launch(c, "validate pools / judge")) return rc;
    if (t) HIPCHK(c, hipEventRecord(t[1].b, s));
    return ICELK_OK;
}

namespace {

bool cells_complete(const icelk_validate_cells_t* q) { return !q || (q->pool_n && q->med_u && q->med_v && q->mad_u && q->mad_v); }

// what both entry points refuse, and why
int check_args(const double* x, const double* y, const double* u, const double* v, int n, const int32_t* group, int ngroups,
               const icelk_validate_lattice_t* L, const icelk_validate_params_t& P, const uint8_t* status, const double* r2,
               const icelk_validate_cells_t* cells, const char** why)
{
    *why = "a null pointer, n < 0 or ngroups < 1";
    if (!L || n < 0 || ngroups < 1 || !cells_complete(cells) || (n > 0 && (!x || !y || !u || !v || !status || !r2))) return ICELK_EARG;
    *why = "without group numbers there is one group";
    if (!group && ngroups != 1) return ICELK_EARG;
    const int rc = validate::check(*L, P, n, ngroups);
    *why = rc == ICELK_ECAP ? "more than 2^27 points, or groups x cols x rows does not fit 31 bits"
                            : "threshold, eps and side must be positive and finite, min_neighbours, cols and rows at least 1";
    return rc;
}

}  // namespace

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_validate_host(const double* x, const double* y, const double* u, const double* v, int n, const int32_t* group, int ngroups,
                        const icelk_validate_lattice_t* lattice, const icelk_validate_params_t* params, uint8_t* status, double* r2,
                        const icelk_validate_cells_t* cells)
{
    const icelk_validate_params_t P = params ? *params : validate::default_params();
    const char* why = "";
    if (int rc = check_args(x, y, u, v, n, group, ngroups, lattice, P, status, r2, cells, &why)) return rc;
    std::vector<unsigned long long> keys((size_t)n + 1);
    validate::run_host(x, y, u, v, n, group, ngroups, *lattice, P, keys.data(), status, r2, cells, nullptr);
    return ICELK_OK;
}

int icelk_validate(icelk_t* h, const double* x, const double* y, const double* u, const double* v, int n, const int32_t* group,
                   int ngroups, const icelk_validate_lattice_t* lattice, const icelk_validate_params_t* params, uint8_t* status,
                   double* r2, const icelk_validate_cells_t* cells)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    const icelk_validate_params_t P = params ? *params : validate::default_params();
    const char* why = "";
    if (int rc = check_args(x, y, u, v, n, group, ngroups, lattice, P, status, r2, cells, &why)) FAIL(c, rc, why);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nn = (size_t)n;
    if (n == 0) {   // no point: every record is the empty one, and nothing to launch
        if (cells) {
            const size_t nseg = (size_t)ngroups * (size_t)lattice->cols * (size_t)lattice->rows;
            std::fill(cells->pool_n, cells->pool_n + nseg, 0);
            for (double* q : {cells->med_u, cells->med_v, cells->mad_u, cells->mad_v}) std::fill(q, q + nseg, __builtin_nan(""));
        }
        return ICELK_OK;
    }
    const hipStream_t s = c->stream;
    DevBufs B;
    ValidateDev V;
    double* d[4];
    for (double*& q : d) q = B.get<double>(nn);
    int32_t* d_group = group ? B.get<int32_t>(nn) : nullptr;
    V.alloc(B, n, ngroups, *lattice, P, s);
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    const double* const host[4] = {x, y, u, v};
    for (int k = 0; k < 4; k++) HIPCHK(c, copy_n(d[k], host[k], nn, kH2D, s));
    if (group) HIPCHK(c, copy_n(d_group, group, nn, kH2D, s));
    V.A.x = d[0], V.A.y = d[1], V.A.u = d[2], V.A.v = d[3], V.A.group = d_group;
    if (int rc = validate_run(c, V, [&] { launch_validate_assign(s, V.A); }, nullptr)) return rc;
    HIPCHK(c, copy_n(status, V.A.status, nn, kD2H, s));
    HIPCHK(c, copy_n(r2, V.A.r2, nn, kD2H, s));
    if (cells) {
        HIPCHK(c, copy_n(cells->pool_n, V.A.cells.pool_n, V.nseg, kD2H, s));
        double* const hc[4] = {cells->med_u, cells->med_v, cells->mad_u, cells->mad_v};
        const double* const dc[4] = {V.A.cells.med_u, V.A.cells.med_v, V.A.cells.mad_u, V.A.cells.mad_v};
        for (int k = 0; k < 4; k++) HIPCHK(c, copy_n(hc[k], dc[k], V.nseg, kD2H, s));
    }
    HIPCHK(c, hipStreamSynchronize(s));
    return ICELK_OK;
}

}  // extern "C"
