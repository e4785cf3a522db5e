// k_drift.hip -- virtual drifters through the gridded velocities on the device (the rule is drift.h's, the
// host's statement of it drift::run_host).
//
//   drift    one drifter per lane, the whole step loop inside the kernel: drift::run, one template over the two sources.  The
//            two kernels below differ in the field they build from their arguments and in nothing else.  A schedule row is
//            the same for every lane: its address depends on the step counter alone and drift::step takes it outside the
//            lanes' own control flow, so the row (k0, k1, a, flag; or the m basis terms) is read through scalar loads and
//            sits in SGPRs.  The node values are gathered straight from global memory: all lanes of a launch read the same
//            two windows (or the same coefficient table) at a step, 150 KB for a season's lattice, which stays in L2.  Staging a row's node
//            values in LDS per workgroup was measured and lost.
//   visits   one thread per recorded sample, integer atomics: the raster does not depend on the order of execution.
//
// Bounds: a lane returns unless p < n.  A cube index k * ncells + cell is formed in size_t from 0 <= k < nt (checked on the
// host for every schedule row before the launch) and cell < ncells, so it is below ncells * nt < 2^31 (icelk_cube_set).  cell
// = j * cols + i (+ 1, + cols, + cols + 1) with 0 <= i <= cols - 2 and 0 <= j <= rows - 2: drift::stage reaches the nodes
// only after 0 <= fx <= cols - 1 and 0 <= fy <= rows - 1 held, and clamps i = min(floor(fx), cols - 2), j likewise, so i + 1 <=
// cols - 1 and j + 1 <= rows - 1; rows * cols is the cube's ncells, or the length of the status and coefficient tables.  A
// schedule row r runs to 2 * nsteps, the table's last row; a coefficient index cell * m + j is below ncells * m (size_t).  An
// output index o * n + p has o <= nsteps / every and is below n * n_out < 2^31 (drift::check), formed in size_t.  A visit is
// counted only for 0 <= node < rows * cols (drift::visited).
#include "drift.h"
#include "icelk_internal.h"

namespace icelk {

namespace {

using namespace drift;

constexpr int kDriftBlock = 256;

__global__ __launch_bounds__(kDriftBlock) void k_drift_cube(
    icelk_drift_lattice_t L, icelk_drift_params_t P, const double* __restrict__ u, const double* __restrict__ v,
    const double* __restrict__ count, const int32_t* __restrict__ k0, const int32_t* __restrict__ k1, const double* __restrict__ a,
    const int32_t* __restrict__ flag, double min_count, const double* __restrict__ seed_x, const double* __restrict__ seed_y,
    const int32_t* __restrict__ release, int n, double* __restrict__ x, double* __restrict__ y, double* __restrict__ last_x,
    double* __restrict__ last_y, double* __restrict__ length, int32_t* __restrict__ status, int32_t* __restrict__ stop_step)
{
    const int p = blockIdx.x * kDriftBlock + threadIdx.x;
    if (p >= n) return;
    CubeField f{u, v, count, (size_t)L.rows * (size_t)L.cols, k0, k1, flag, a, min_count, 0, 0, 0.0, 0};
    run(f, L, P, seed_x, seed_y, release, p, n, Out{x, y, last_x, last_y, length, status, stop_step});
}

__global__ __launch_bounds__(kDriftBlock) void k_drift_tide(
    icelk_drift_lattice_t L, icelk_drift_params_t P, const double* __restrict__ coef_u, const double* __restrict__ coef_v,
    const int32_t* __restrict__ cell_status, const double* __restrict__ basis, int m, const double* __restrict__ seed_x,
    const double* __restrict__ seed_y, const int32_t* __restrict__ release, int n, double* __restrict__ x, double* __restrict__ y,
    double* __restrict__ last_x, double* __restrict__ last_y, double* __restrict__ length, int32_t* __restrict__ status,
    int32_t* __restrict__ stop_step)
{
    const int p = blockIdx.x * kDriftBlock + threadIdx.x;
    if (p >= n) return;
    TideField f{coef_u, coef_v, cell_status, basis, m, {}};
    run(f, L, P, seed_x, seed_y, release, p, n, Out{x, y, last_x, last_y, length, status, stop_step});
}

__global__ __launch_bounds__(256) void k_drift_visits(icelk_drift_lattice_t L, const double* __restrict__ x, const double* __restrict__ y,
                                                      int samples, int32_t* __restrict__ visits)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= samples) return;
    const long long c = visited(L, x[k], y[k]);
    if (c >= 0) atomicAdd(&visits[c], 1);
}

unsigned blocks(int n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

void launch_drift_cube(hipStream_t s, const icelk_drift_lattice_t& L, const icelk_drift_params_t& P, const drift::CubeField& F,
                       const DriftSeeds& S, const drift::Out& O)
{
    hipLaunchKernelGGL(k_drift_cube, dim3(blocks(S.n, kDriftBlock)), dim3(kDriftBlock), 0, s, L, P, F.u, F.v, F.count, F.k0, F.k1, F.a,
                       F.flag, F.min_count, S.x, S.y, S.release, S.n, O.x, O.y, O.last_x, O.last_y, O.length, O.status, O.stop_step);
}

void launch_drift_tide(hipStream_t s, const icelk_drift_lattice_t& L, const icelk_drift_params_t& P, const drift::TideField& F,
                       const DriftSeeds& S, const drift::Out& O)
{
    hipLaunchKernelGGL(k_drift_tide, dim3(blocks(S.n, kDriftBlock)), dim3(kDriftBlock), 0, s, L, P, F.coef_u, F.coef_v, F.status, F.basis,
                       F.m, S.x, S.y, S.release, S.n, O.x, O.y, O.last_x, O.last_y, O.length, O.status, O.stop_step);
}

void launch_drift_visits(hipStream_t s, const icelk_drift_lattice_t& L, const double* x, const double* y, int samples, int32_t* visits)
{
    hipLaunchKernelGGL(k_drift_visits, dim3(blocks(samples, 256)), dim3(256), 0, s, L, x, y, samples, visits);
}

}  // namespace icelk
