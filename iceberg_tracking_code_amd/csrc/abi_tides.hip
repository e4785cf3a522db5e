// abi_tides.hip -- the per-cell harmonic fit of the velocity cube.  The rules are tides.h's, the kernels
// k_tides.hip's.
//
//   host    icelk_tide_fit_host: tides.h on the CPU; no handle, re-entrant
//   device  icelk_cube_tide_fit: the basis up, normal -> solve -> residual -> finish on the cube icelk_cube_set left on the
//           device, the results down, one wait at the end.  The cube is read, never written.
//           icelk_cube_tide_predict: coefficients, status and a basis of any length up, predict, the two fields down.
// Every argument is checked before anything is allocated or issued; a refusal leaves the handle as it was.
#include "icelk_ctx.h"
#include "tides.h"

namespace icelk {
namespace {

bool outputs_complete(const double* coef_u, const double* coef_v, const double* rms_u, const double* rms_v, const double* explained_u,
                      const double* explained_v, const int32_t* n, const int32_t* first, const int32_t* last, const int32_t* status)
{
    return coef_u && coef_v && rms_u && rms_v && explained_u && explained_v && n && first && last && status;
}

const char* refusal(int rc)
{
    return rc == ICELK_ECAP ? "more than 18 terms, or the workspace of chunk partials does not fit 31 bits"
                            : "cells, windows and terms must be at least 1, min_samples at least 0";
}

}  // namespace
}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_tide_fit_host(const double* u, const double* v, const double* count, int ncells, int nt, const double* basis, int m,
                        double min_count, int min_samples, double* coef_u, double* coef_v, double* rms_u, double* rms_v,
                        double* explained_u, double* explained_v, int32_t* n, int32_t* first, int32_t* last, int32_t* status,
                        double* residual_u_or_null, double* residual_v_or_null)
{
    if (!u || !v || !count || !basis || !outputs_complete(coef_u, coef_v, rms_u, rms_v, explained_u, explained_v, n, first, last, status))
        return ICELK_EARG;
    if (int rc = tides::check(ncells, nt, m, min_samples)) return rc;
    const tides::FitOut O{coef_u, coef_v, rms_u, rms_v, explained_u, explained_v, n, first, last, status, residual_u_or_null, residual_v_or_null};
    tides::fit_host(u, v, count, ncells, nt, basis, m, min_count, min_samples, O);
    return ICELK_OK;
}

int icelk_cube_tide_fit(icelk_t* h, const double* basis, int nt, int m, double min_count, int min_samples, double* coef_u,
                        double* coef_v, double* rms_u, double* rms_v, double* explained_u, double* explained_v, int32_t* n,
                        int32_t* first, int32_t* last, int32_t* status, double* residual_u_or_null, double* residual_v_or_null,
                        double* device_ms_or_null)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!basis || !outputs_complete(coef_u, coef_v, rms_u, rms_v, explained_u, explained_v, n, first, last, status))
        FAIL(c, ICELK_EARG, "a null pointer");
    if (!c->post.d_cube_u) FAIL(c, ICELK_ESTATE, "icelk_cube_set has not been called");
    if (nt != c->post.cube_nt) FAIL(c, ICELK_EARG, "the basis must have one row per window of the cube");
    const int ncells = c->post.cube_ncells;
    if (int rc = tides::check(ncells, nt, m, min_samples)) FAIL(c, rc, refusal(rc));
    if (device_ms_or_null) *device_ms_or_null = 0.0;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nc = (size_t)ncells, chunks = (size_t)tides::n_chunks(nt), mm = (size_t)m, cube = nc * (size_t)nt;
    DevBufs B;
    TideArgs A{};
    A.u = c->post.d_cube_u, A.v = c->post.d_cube_v, A.count = c->post.d_cube_count;
    A.ncells = ncells, A.nt = nt, A.m = m, A.min_count = min_count, A.min_samples = min_samples;
    double* d_basis = B.get<double>((size_t)nt * mm);
    A.basis = d_basis;
    A.part = B.get<double>((size_t)tides::n_sums(m) * chunks * nc);
    A.ipart = B.get<int32_t>(3 * chunks * nc);
    A.tot = B.get<double>((size_t)tides::n_sums(m) * nc);
    A.mean = B.get<double>(2 * nc);
    A.part2 = B.get<double>(4 * chunks * nc);
    A.coef_u = B.get<double>(nc * mm), A.coef_v = B.get<double>(nc * mm);
    for (double** q : {&A.rms_u, &A.rms_v, &A.explained_u, &A.explained_v}) *q = B.get<double>(nc);
    for (int32_t** q : {&A.n, &A.first, &A.last, &A.status}) *q = B.get<int32_t>(nc);
    A.res_u = residual_u_or_null ? B.get<double>(cube) : nullptr;
    A.res_v = residual_v_or_null ? B.get<double>(cube) : nullptr;
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    const hipStream_t s = c->stream;
    HIPCHK(c, copy_n(d_basis, basis, (size_t)nt * mm, kH2D, s));
    EvPair timer;
    if (device_ms_or_null) {
        if (int rc = timer.create(c)) return rc;
        HIPCHK(c, hipEventRecord(timer.a, s));
    }
    launch_tide_normal(s, A);
    launch_tide_solve(s, A);
    launch_tide_residual(s, A);
    launch_tide_finish(s, A);
    if (int rc = check_launch(c, "tide fit")) return rc;
    if (device_ms_or_null) HIPCHK(c, hipEventRecord(timer.b, s));
    HIPCHK(c, copy_n(coef_u, A.coef_u, nc * mm, kD2H, s));
    HIPCHK(c, copy_n(coef_v, A.coef_v, nc * mm, kD2H, s));
    double* const host[4] = {rms_u, rms_v, explained_u, explained_v};
    const double* const dev[4] = {A.rms_u, A.rms_v, A.explained_u, A.explained_v};
    for (int k = 0; k < 4; k++) HIPCHK(c, copy_n(host[k], dev[k], nc, kD2H, s));
    int32_t* const ihost[4] = {n, first, last, status};
    const int32_t* const idev[4] = {A.n, A.first, A.last, A.status};
    for (int k = 0; k < 4; k++) HIPCHK(c, copy_n(ihost[k], idev[k], nc, kD2H, s));
    if (residual_u_or_null) HIPCHK(c, copy_n(residual_u_or_null, A.res_u, cube, kD2H, s));
    if (residual_v_or_null) HIPCHK(c, copy_n(residual_v_or_null, A.res_v, cube, kD2H, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (device_ms_or_null) {
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, timer.a, timer.b));
        *device_ms_or_null = (double)ms;
    }
    return ICELK_OK;
}

int icelk_cube_tide_predict(icelk_t* h, const double* coef_u, const double* coef_v, const int32_t* status, int ncells, int m,
                            const double* basis, int ntp, double* out_u, double* out_v)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!coef_u || !coef_v || !status || !basis || !out_u || !out_v) FAIL(c, ICELK_EARG, "a null pointer");
    if (ncells < 1 || m < 1 || ntp < 1) FAIL(c, ICELK_EARG, "cells, terms and times must be at least 1");
    if (m > tides::kTideMaxTerms) FAIL(c, ICELK_ECAP, "more than 18 terms");
    if ((long long)ncells * ntp > 0x7fffffffLL || tides::n_chunks(ntp) > 65535) FAIL(c, ICELK_ECAP, "cells x times does not fit 31 bits");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nc = (size_t)ncells, mm = (size_t)m, nout = nc * (size_t)ntp;
    DevBufs B;
    double* d_cu = B.get<double>(nc * mm);
    double* d_cv = B.get<double>(nc * mm);
    int32_t* d_status = B.get<int32_t>(nc);
    double* d_basis = B.get<double>((size_t)ntp * mm);
    double* d_u = B.get<double>(nout);
    double* d_v = B.get<double>(nout);
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    const hipStream_t s = c->stream;
    HIPCHK(c, copy_n(d_cu, coef_u, nc * mm, kH2D, s));
    HIPCHK(c, copy_n(d_cv, coef_v, nc * mm, kH2D, s));
    HIPCHK(c, copy_n(d_status, status, nc, kH2D, s));
    HIPCHK(c, copy_n(d_basis, basis, (size_t)ntp * mm, kH2D, s));
    launch_tide_predict(s, d_cu, d_cv, d_status, ncells, m, d_basis, ntp, d_u, d_v);
    if (int rc = check_launch(c, "tide_predict")) return rc;
    HIPCHK(c, copy_n(out_u, d_u, nout, kD2H, s));
    HIPCHK(c, copy_n(out_v, d_v, nout, kD2H, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return ICELK_OK;
}

}  // extern "C"
