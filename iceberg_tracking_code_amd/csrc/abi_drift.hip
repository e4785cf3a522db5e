// abi_drift.hip -- virtual drifters through the gridded velocities.  The rule is drift.h's, the kernels
// k_drift.hip's.
//
//   host    icelk_drift_host: drift.h on the CPU, both sources; no handle, re-entrant
//   device  icelk_cube_drift: the schedule table and the seeds up, the drift kernel on the cube icelk_cube_set left on the
//           device, the visits kernel if asked, the results down, one wait at the end.  The cube is read, never written.
//           icelk_drift_tide: coefficients, status, the basis rows and the seeds up, the same two kernels.  Needs no cube.
// Every argument is checked before anything is allocated or issued; a refusal leaves the handle as it was.
#include "drift.h"
#include "icelk_ctx.h"

namespace icelk {
namespace {

bool complete(const icelk_drift_lattice_t* L, const icelk_drift_params_t* P, const double* seed_x, const double* seed_y,
              const int32_t* release, const icelk_drift_out_t* O)
{
    return L && P && seed_x && seed_y && release && O && O->x && O->y && O->last_x && O->last_y && O->length && O->status && O->stop_step;
}

const char* refusal(int rc)
{
    return rc == ICELK_ECAP ? "drifters x recorded steps or schedule rows x terms do not fit 31 bits, or more than 18 terms"
                            : "a lattice of 2 x 2 nodes at least with a finite spacing other than 0, n >= 1, a finite step other than 0, "
                              "nsteps >= 1, every >= 1, order 1, 2 or 4 and min_nodes 1 .. 4 are required";
}

// every schedule row's windows lie in the cube
bool windows_inside(const int32_t* k0, const int32_t* k1, int rows, int nt)
{
    for (int r = 0; r < rows; r++)
        if (k0[r] < 0 || k0[r] >= nt || k1[r] < 0 || k1[r] >= nt) return false;
    return true;
}

drift::Out host_out(const icelk_drift_out_t* O) { return drift::Out{O->x, O->y, O->last_x, O->last_y, O->length, O->status, O->stop_step}; }

// The device side that both sources share: the seeds up, `launch` (the source's drift kernel), the visits, everything down.
template <typename Launch>
int run_device(Ctx* c, DevBufs& B, const icelk_drift_lattice_t& L, const icelk_drift_params_t& P, const double* seed_x,
               const double* seed_y, const int32_t* release, int n, const icelk_drift_out_t* out, double* device_ms_or_null,
               const Launch& launch)
{
    const size_t nn = (size_t)n, samples = nn * (size_t)drift::n_out(P), cells = (size_t)L.rows * (size_t)L.cols;
    double* d_sx = B.get<double>(nn);
    double* d_sy = B.get<double>(nn);
    int32_t* d_rel = B.get<int32_t>(nn);
    drift::Out O{};
    O.x = B.get<double>(samples), O.y = B.get<double>(samples);
    for (double** q : {&O.last_x, &O.last_y, &O.length}) *q = B.get<double>(nn);
    O.status = B.get<int32_t>(nn), O.stop_step = B.get<int32_t>(nn);
    int32_t* d_visits = out->visits_or_null ? B.get<int32_t>(cells) : nullptr;
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    const hipStream_t s = c->stream;
    HIPCHK(c, copy_n(d_sx, seed_x, nn, kH2D, s));
    HIPCHK(c, copy_n(d_sy, seed_y, nn, kH2D, s));
    HIPCHK(c, copy_n(d_rel, release, nn, kH2D, s));
    if (d_visits) HIPCHK(c, hipMemsetAsync(d_visits, 0, cells * sizeof(int32_t), s));
    EvPair timer;
    if (device_ms_or_null) {
        if (int rc = timer.create(c)) return rc;
        HIPCHK(c, hipEventRecord(timer.a, s));
    }
    launch(s, DriftSeeds{d_sx, d_sy, d_rel, n}, O);
    if (d_visits) launch_drift_visits(s, L, O.x, O.y, (int)samples, d_visits);
    if (int rc = check_launch(c, "drift")) return rc;
    if (device_ms_or_null) HIPCHK(c, hipEventRecord(timer.b, s));
    HIPCHK(c, copy_n(out->x, O.x, samples, kD2H, s));
    HIPCHK(c, copy_n(out->y, O.y, samples, kD2H, s));
    double* const host[3] = {out->last_x, out->last_y, out->length};
    const double* const dev[3] = {O.last_x, O.last_y, O.length};
    for (int k = 0; k < 3; k++) HIPCHK(c, copy_n(host[k], dev[k], nn, kD2H, s));
    HIPCHK(c, copy_n(out->status, O.status, nn, kD2H, s));
    HIPCHK(c, copy_n(out->stop_step, O.stop_step, nn, kD2H, s));
    if (d_visits) HIPCHK(c, copy_n(out->visits_or_null, d_visits, cells, kD2H, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (device_ms_or_null) {
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, timer.a, timer.b));
        *device_ms_or_null = (double)ms;
    }
    return ICELK_OK;
}

}  // namespace
}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_drift_host(const icelk_drift_lattice_t* lattice, const icelk_drift_params_t* params, const double* u, const double* v,
                     const double* count, int nt, const int32_t* k0, const int32_t* k1, const double* a, const int32_t* flag,
                     double min_count, const double* coef_u, const double* coef_v, const int32_t* status, int m,
                     const double* basis, const double* seed_x, const double* seed_y, const int32_t* release, int n,
                     const icelk_drift_out_t* out)
{
    if (!complete(lattice, params, seed_x, seed_y, release, out)) return ICELK_EARG;
    const bool cube = u != nullptr, tide = coef_u != nullptr;
    if (cube == tide) return ICELK_EARG;
    if (cube ? (!v || !count || !k0 || !k1 || !a || !flag || nt < 1) : (!coef_v || !status || !basis || m < 1)) return ICELK_EARG;
    if (int rc = drift::check(*lattice, *params, n, cube ? 0 : m)) return rc;
    const size_t cells = (size_t)lattice->rows * (size_t)lattice->cols;
    if (cube) {
        if (cells * (size_t)nt > 0x7fffffffULL) return ICELK_ECAP;
        if (!windows_inside(k0, k1, 2 * params->nsteps + 1, nt)) return ICELK_EARG;
        drift::run_host(drift::CubeField{u, v, count, cells, k0, k1, flag, a, min_count, 0, 0, 0.0, 0}, *lattice, *params, seed_x, seed_y,
                        release, n, host_out(out), out->visits_or_null);
    } else {
        drift::run_host(drift::TideField{coef_u, coef_v, status, basis, m, {}}, *lattice, *params, seed_x, seed_y, release, n,
                        host_out(out), out->visits_or_null);
    }
    return ICELK_OK;
}

int icelk_cube_drift(icelk_t* h, const icelk_drift_lattice_t* lattice, const icelk_drift_params_t* params, const int32_t* k0,
                     const int32_t* k1, const double* a, const int32_t* flag, double min_count, const double* seed_x,
                     const double* seed_y, const int32_t* release, int n, const icelk_drift_out_t* out, double* device_ms_or_null)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!complete(lattice, params, seed_x, seed_y, release, out) || !k0 || !k1 || !a || !flag) FAIL(c, ICELK_EARG, "a null pointer");
    if (!c->post.d_cube_u) FAIL(c, ICELK_ESTATE, "icelk_cube_set has not been called");
    if (int rc = drift::check(*lattice, *params, n, 0)) FAIL(c, rc, refusal(rc));
    if ((long long)lattice->rows * lattice->cols != c->post.cube_ncells) FAIL(c, ICELK_EARG, "the lattice must have one node per cell of the cube");
    const int sched = 2 * params->nsteps + 1;
    if (!windows_inside(k0, k1, sched, c->post.cube_nt)) FAIL(c, ICELK_EARG, "a schedule row names a window outside the cube");
    if (device_ms_or_null) *device_ms_or_null = 0.0;
    HIPCHK(c, hipSetDevice(c->device));
    DevBufs B;
    int32_t* d_k0 = B.get<int32_t>((size_t)sched);
    int32_t* d_k1 = B.get<int32_t>((size_t)sched);
    int32_t* d_flag = B.get<int32_t>((size_t)sched);
    double* d_a = B.get<double>((size_t)sched);
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    const hipStream_t s = c->stream;
    HIPCHK(c, copy_n(d_k0, k0, (size_t)sched, kH2D, s));
    HIPCHK(c, copy_n(d_k1, k1, (size_t)sched, kH2D, s));
    HIPCHK(c, copy_n(d_flag, flag, (size_t)sched, kH2D, s));
    HIPCHK(c, copy_n(d_a, a, (size_t)sched, kH2D, s));
    const drift::CubeField F{c->post.d_cube_u, c->post.d_cube_v, c->post.d_cube_count, (size_t)c->post.cube_ncells, d_k0, d_k1, d_flag, d_a,
                             min_count, 0, 0, 0.0, 0};
    return run_device(c, B, *lattice, *params, seed_x, seed_y, release, n, out, device_ms_or_null,
                      [&](hipStream_t st, const DriftSeeds& S, const drift::Out& O) { launch_drift_cube(st, *lattice, *params, F, S, O); });
}

int icelk_drift_tide(icelk_t* h, const icelk_drift_lattice_t* lattice, const icelk_drift_params_t* params, const double* coef_u,
                     const double* coef_v, const int32_t* status, int m, const double* basis, const double* seed_x,
                     const double* seed_y, const int32_t* release, int n, const icelk_drift_out_t* out, double* device_ms_or_null)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!complete(lattice, params, seed_x, seed_y, release, out) || !coef_u || !coef_v || !status || !basis) FAIL(c, ICELK_EARG, "a null pointer");
    if (m < 1) FAIL(c, ICELK_EARG, "terms must be at least 1");
    if (int rc = drift::check(*lattice, *params, n, m)) FAIL(c, rc, refusal(rc));
    if (device_ms_or_null) *device_ms_or_null = 0.0;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cells = (size_t)lattice->rows * (size_t)lattice->cols, mm = (size_t)m, sched = 2 * (size_t)params->nsteps + 1;
    DevBufs B;
    double* d_cu = B.get<double>(cells * mm);
    double* d_cv = B.get<double>(cells * mm);
    int32_t* d_status = B.get<int32_t>(cells);
    double* d_basis = B.get<double>(sched * mm);
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    const hipStream_t s = c->stream;
    HIPCHK(c, copy_n(d_cu, coef_u, cells * mm, kH2D, s));
    HIPCHK(c, copy_n(d_cv, coef_v, cells * mm, kH2D, s));
    HIPCHK(c, copy_n(d_status, status, cells, kH2D, s));
    HIPCHK(c, copy_n(d_basis, basis, sched * mm, kH2D, s));
    const drift::TideField F{d_cu, d_cv, d_status, d_basis, m, {}};
    return run_device(c, B, *lattice, *params, seed_x, seed_y, release, n, out, device_ms_or_null,
                      [&](hipStream_t st, const DriftSeeds& S, const drift::Out& O) { launch_drift_tide(st, *lattice, *params, F, S, O); });
}

}  // extern "C"
