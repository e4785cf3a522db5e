// k_tides.hip -- the per-cell harmonic fit of the velocity cube on the device (the rules are tides.h's, the
// host's statement of them tides::fit_host).
//
// The cube is [window][cell] with the cell fastest: one lane per cell reads coalesced, and the basis row of a window is the
// same for every lane -- its address depends on the block's chunk and the loop counter only, so it is read through scalar
// loads.  A season has few cells (45 x 70) and many windows (6000): the chunks of the rule (kTideChunk windows) are the
// second grid axis, without which the device would stand idle.
//
//   normal    a thread owns (cell, chunk, row i of the normal matrix): A[i][0 .. i], ru[i], rv[i], at most 20 accumulators,
//             all statically indexed after unrolling and so in VGPRs.  blockIdx.z = m is the slice of su, sv, n, first and
//             last.  The chunk partials go to part [sum][chunk][cell] and ipart [3][chunk][cell].
//   solve     one thread per cell: the chunk partials added in ascending order into tot [sum][cell], then tides.h's
//             factor_solve in place on it -- cell-fastest, so every load and store of the triangular loops is coalesced and
//             nothing is indexed in registers.  Writes n, first, last, status, the coefficients [cell][m] and the means.
//   residual  a thread owns (cell, chunk): the coefficients of u and v in 36 statically indexed registers, the second pass
//             over the chunk, the residual cube if asked, four partials to part2.
//   finish    one thread per cell: part2 added in order, rms and explained.
//   predict   a thread owns (cell, 256 windows of the caller's basis).
//
// Bounds: every thread returns unless cell < ncells; t runs below nt (ntp); a cube index t * ncells + cell is below ncells *
// nt < 2^31 (icelk_cube_set), a workspace index below n_sums * chunks * ncells < 2^31 (tides::check), both formed in size_t.
#include "icelk_internal.h"
#include "tides.h"

namespace icelk {

namespace {

using namespace tides;

__device__ __forceinline__ size_t part_at(const TideArgs& A, int sum, int chunks, int chunk, int cell)
{
    return ((size_t)sum * (size_t)chunks + (size_t)chunk) * (size_t)A.ncells + (size_t)cell;
}

// row t of the basis into registers, ahead of the lane's sample test: the loads are wave-uniform and stand in uniform control
// flow, so they are scalar loads and the row sits in SGPRs
__device__ __forceinline__ void load_row(double* br, const double* __restrict__ b, int last)
{
    ICELK_TIDE_UNROLL
    for (int j = 0; j < kTideMaxTerms; j++) br[j] = j <= last ? b[j] : 0.0;
}

__global__ __launch_bounds__(256) void k_tide_normal(TideArgs A, const double* __restrict__ basis)
{
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= A.ncells) return;
    const int chunk = blockIdx.y, row = blockIdx.z, chunks = gridDim.y, m = A.m;
    const int t0 = chunk * kTideChunk, t1 = min(A.nt, t0 + kTideChunk);
    if (row < m) {
        double acc[kRowAcc];
        ICELK_TIDE_UNROLL
        for (int j = 0; j < kRowAcc; j++) acc[j] = 0.0;
        for (int t = t0; t < t1; t++) {
            const size_t at = (size_t)t * (size_t)A.ncells + (size_t)cell;
            const double* __restrict__ b = basis + (size_t)t * (size_t)m;
            double br[kTideMaxTerms];
            load_row(br, b, row);
            const double bi = b[row];
            const double u = A.u[at], v = A.v[at];
            if (is_sample(u, v, A.count[at], A.min_count)) add_row(acc, br, bi, row, u, v);
        }
        ICELK_TIDE_UNROLL
        for (int j = 0; j < kTideMaxTerms; j++)
            if (j <= row) A.part[part_at(A, slot_a(row, j), chunks, chunk, cell)] = acc[j];
        A.part[part_at(A, slot_ru(m, row), chunks, chunk, cell)] = acc[kTideMaxTerms];
        A.part[part_at(A, slot_rv(m, row), chunks, chunk, cell)] = acc[kTideMaxTerms + 1];
        return;
    }
    double su = 0.0, sv = 0.0;
    int n = 0, first = -1, last = -1;
    for (int t = t0; t < t1; t++) {
        const size_t at = (size_t)t * (size_t)A.ncells + (size_t)cell;
        const double u = A.u[at], v = A.v[at];
        if (!is_sample(u, v, A.count[at], A.min_count)) continue;
        su = su + u;
        sv = sv + v;
        n++;
        if (first < 0) first = t;
        last = t;
    }
    A.part[part_at(A, slot_su(m), chunks, chunk, cell)] = su;
    A.part[part_at(A, slot_sv(m), chunks, chunk, cell)] = sv;
    A.ipart[part_at(A, 0, chunks, chunk, cell)] = n;
    A.ipart[part_at(A, 1, chunks, chunk, cell)] = first;
    A.ipart[part_at(A, 2, chunks, chunk, cell)] = last;
}

__global__ __launch_bounds__(256) void k_tide_solve(TideArgs A, int chunks)
{
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= A.ncells) return;
    const int m = A.m, nsums = n_sums(m);
    const size_t ncells = (size_t)A.ncells;
    for (int s = 0; s < nsums; s++) {
        double total = 0.0;
        for (int ch = 0; ch < chunks; ch++) total = total + A.part[part_at(A, s, chunks, ch, cell)];
        A.tot[(size_t)s * ncells + (size_t)cell] = total;
    }
    int n = 0, first = -1, last = -1;
    for (int ch = 0; ch < chunks; ch++) {
        const int f = A.ipart[part_at(A, 1, chunks, ch, cell)];
        n += A.ipart[part_at(A, 0, chunks, ch, cell)];
        if (f < 0) continue;
        if (first < 0) first = f;
        last = A.ipart[part_at(A, 2, chunks, ch, cell)];
    }
    const CellSums W{A.tot + cell, ncells};
    A.mean[cell] = W[slot_su(m)] / (double)n;
    A.mean[ncells + (size_t)cell] = W[slot_sv(m)] / (double)n;
    const int32_t status = factor_solve(W, m, n, A.min_samples);
    for (int j = 0; j < m; j++) {
        A.coef_u[(size_t)cell * (size_t)m + (size_t)j] = status == kOk ? W[slot_ru(m, j)] : __builtin_nan("");
        A.coef_v[(size_t)cell * (size_t)m + (size_t)j] = status == kOk ? W[slot_rv(m, j)] : __builtin_nan("");
    }
    A.n[cell] = n, A.first[cell] = first, A.last[cell] = last, A.status[cell] = status;
}

// a cell's coefficients into kTideMaxTerms registers
__device__ __forceinline__ void load_coef(double* c, const double* __restrict__ coef, int cell, int m)
{
    ICELK_TIDE_UNROLL
    for (int j = 0; j < kTideMaxTerms; j++) c[j] = j < m ? coef[(size_t)cell * (size_t)m + (size_t)j] : 0.0;
}

__global__ __launch_bounds__(256) void k_tide_residual(TideArgs A, const double* __restrict__ basis, double* __restrict__ out_u,
                                                       double* __restrict__ out_v)
{
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= A.ncells) return;
    const int chunk = blockIdx.y, chunks = gridDim.y, m = A.m;
    const int t0 = chunk * kTideChunk, t1 = min(A.nt, t0 + kTideChunk);
    const bool solved = A.status[cell] == kOk;
    double cu[kTideMaxTerms], cv[kTideMaxTerms];
    load_coef(cu, A.coef_u, cell, m);
    load_coef(cv, A.coef_v, cell, m);
    const double mean_u = A.mean[cell], mean_v = A.mean[(size_t)A.ncells + (size_t)cell];
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, p3 = 0.0;
    for (int t = t0; t < t1; t++) {
        const size_t at = (size_t)t * (size_t)A.ncells + (size_t)cell;
        const double u = A.u[at], v = A.v[at];
        double res_u = __builtin_nan(""), res_v = __builtin_nan("");
        double br[kTideMaxTerms];
        load_row(br, basis + (size_t)t * (size_t)m, m - 1);
        if (solved && is_sample(u, v, A.count[at], A.min_count)) {
            res_u = u - predict(cu, br, m);
            res_v = v - predict(cv, br, m);
            const double du = u - mean_u, dv = v - mean_v;
            p0 = p0 + res_u * res_u;
            p1 = p1 + res_v * res_v;
            p2 = p2 + du * du;
            p3 = p3 + dv * dv;
        }
        if (out_u) out_u[at] = res_u;
        if (out_v) out_v[at] = res_v;
    }
    A.part2[part_at(A, 0, chunks, chunk, cell)] = p0;
    A.part2[part_at(A, 1, chunks, chunk, cell)] = p1;
    A.part2[part_at(A, 2, chunks, chunk, cell)] = p2;
    A.part2[part_at(A, 3, chunks, chunk, cell)] = p3;
}

__global__ __launch_bounds__(256) void k_tide_finish(TideArgs A, int chunks)
{
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= A.ncells) return;
    double ss[4];
    ICELK_TIDE_UNROLL
    for (int k = 0; k < 4; k++) {
        double total = 0.0;
        for (int ch = 0; ch < chunks; ch++) total = total + A.part2[part_at(A, k, chunks, ch, cell)];
        ss[k] = total;
    }
    const int n = A.n[cell];
    const int32_t status = A.status[cell];
    finish(ss[0], ss[2], n, A.m, status, &A.rms_u[cell], &A.explained_u[cell]);
    finish(ss[1], ss[3], n, A.m, status, &A.rms_v[cell], &A.explained_v[cell]);
}

__global__ __launch_bounds__(256) void k_tide_predict(const double* __restrict__ coef_u, const double* __restrict__ coef_v,
                                                      const int32_t* __restrict__ status, int ncells, int m,
                                                      const double* __restrict__ basis, int ntp, double* __restrict__ out_u,
                                                      double* __restrict__ out_v)
{
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= ncells) return;
    const int t0 = blockIdx.y * kTideChunk, t1 = min(ntp, t0 + kTideChunk);
    const bool solved = status[cell] == kOk;
    double cu[kTideMaxTerms], cv[kTideMaxTerms];
    load_coef(cu, coef_u, cell, m);
    load_coef(cv, coef_v, cell, m);
    for (int t = t0; t < t1; t++) {
        const size_t at = (size_t)t * (size_t)ncells + (size_t)cell;
        const double* b = basis + (size_t)t * (size_t)m;
        out_u[at] = solved ? predict(cu, b, m) : __builtin_nan("");
        out_v[at] = solved ? predict(cv, b, m) : __builtin_nan("");
    }
}

}  // namespace

void launch_tide_normal(hipStream_t s, const TideArgs& A)
{
    const dim3 grid((unsigned)((A.ncells + 255) / 256), (unsigned)n_chunks(A.nt), (unsigned)(A.m + 1));
    hipLaunchKernelGGL(k_tide_normal, grid, dim3(256), 0, s, A, A.basis);
}

void launch_tide_solve(hipStream_t s, const TideArgs& A)
{
    hipLaunchKernelGGL(k_tide_solve, dim3((unsigned)((A.ncells + 255) / 256)), dim3(256), 0, s, A, n_chunks(A.nt));
}

void launch_tide_residual(hipStream_t s, const TideArgs& A)
{
    const dim3 grid((unsigned)((A.ncells + 255) / 256), (unsigned)n_chunks(A.nt));
    hipLaunchKernelGGL(k_tide_residual, grid, dim3(256), 0, s, A, A.basis, A.res_u, A.res_v);
}

void launch_tide_finish(hipStream_t s, const TideArgs& A)
{
    hipLaunchKernelGGL(k_tide_finish, dim3((unsigned)((A.ncells + 255) / 256)), dim3(256), 0, s, A, n_chunks(A.nt));
}

void launch_tide_predict(hipStream_t s, const double* coef_u, const double* coef_v, const int32_t* status, int ncells, int m,
                         const double* basis, int ntp, double* out_u, double* out_v)
{
    const dim3 grid((unsigned)((ncells + 255) / 256), (unsigned)n_chunks(ntp));
    hipLaunchKernelGGL(k_tide_predict, grid, dim3(256), 0, s, coef_u, coef_v, status, ncells, m, basis, ntp, out_u, out_v);
}

}  // namespace icelk
