// k_cube.hip -- averages of the run-wide velocity cube (s4_postprocess_gridded_utm.py:264-343).
//
// The reference's average_spatially_temporally is called once per averaging period: it slices the cube with a time
// mask (u[:, :, mask]), takes np.nanmean of u and v and np.nansum of count over the selected windows, and for
// coarseness > 1 runs spatial_mean(..., nanmean = 0) over the three fields.  Here the cube stays on the device, laid
// out [window][cell] (cell = row * cols + col), and one launch chain serves every period of a request.
//
// The order of the additions is numpy's, found by measurement:
// - u[:, :, mask] comes out of numpy's fancy indexing with the window axis SLOWEST in memory, so np.sum over that axis
//   is the plain element-wise loop out += a[t]: per cell the windows are added one after the other, ascending, from
//   0.0 -- no pairwise blocks.  NaN counts as +0.0 (and is still added), the mean is sum / (number of non-NaN terms),
//   0.0 / 0 = NaN where a cell was never measured.  A cube of ONE cell is the exception: its selection is a
//   contiguous run, which numpy adds as np.sum adds one (np_sums.h: np_sum).
// - np.mean(axis = (1, 3)) of the zero-padded (R/c, c, C/c, c) view: cube_means.h, shared with the host test.
#include "icelk_internal.h"
#include "cube_means.h"

namespace icelk {

namespace {

// NaN-replaced element t of a one-cell cube's selection
struct SelectedAt {
    const double* __restrict__ a;
    const int* __restrict__ sel;
    __device__ __forceinline__ double operator()(int t) const
    {
        const double x = a[sel[t]];
        return x == x ? x : 0.0;
    }
};

// one thread per (period, cell); a workgroup lies inside one period, so the window list is read with scalar loads
// and a wave reads 512 contiguous bytes of every selected window
__global__ __launch_bounds__(256) void k_cube_temporal(const double* __restrict__ u, const double* __restrict__ v,
                                                       const double* __restrict__ cnt, int ncells,
                                                       const int* __restrict__ sel_offset,
                                                       const int* __restrict__ sel_index, int cell_blocks,
                                                       double* __restrict__ mean_u, double* __restrict__ mean_v,
                                                       double* __restrict__ speed, double* __restrict__ count_sum,
                                                       int* __restrict__ has_data)
{
    const int p = blockIdx.x / cell_blocks;
    const int cell = (blockIdx.x - p * cell_blocks) * 256 + threadIdx.x;
    if (cell >= ncells) return;
    const int k0 = sel_offset[p], k1 = sel_offset[p + 1];
    double su = 0.0, sv = 0.0, sc = 0.0;
    int nu = 0, nv = 0;
#pragma unroll 4
    for (int k = k0; k < k1; k++) {
        const size_t at = (size_t)sel_index[k] * (size_t)ncells + (size_t)cell;
        const double a = u[at], b = v[at], c = cnt[at];
        const bool ua = a == a, vb = b == b;
        su += ua ? a : 0.0;
        sv += vb ? b : 0.0;
        sc += c == c ? c : 0.0;
        nu += ua ? 1 : 0;
        nv += vb ? 1 : 0;
    }
    if (ncells == 1) {   // numpy's order over a contiguous run; nu and nv stand
        su = np_sum(SelectedAt{u, sel_index + k0}, k1 - k0);
        sv = np_sum(SelectedAt{v, sel_index + k0}, k1 - k0);
        sc = np_sum(SelectedAt{cnt, sel_index + k0}, k1 - k0);
    }
    const double mu = su / (double)nu, mv = sv / (double)nv;
    const double sp = hypot_np(mu, mv);
    const size_t o = (size_t)p * (size_t)ncells + (size_t)cell;
    mean_u[o] = mu;
    mean_v[o] = mv;
    speed[o] = sp;
    count_sum[o] = sc;
    if (sp == sp) has_data[p] = 1;   // every writer stores the same value
}

// one thread per (period, coarse cell): the three fields and the speed of the coarse u, v
__global__ __launch_bounds__(64) void k_cube_spatial(const double* __restrict__ mean_u, const double* __restrict__ mean_v,
                                                     const double* __restrict__ count_sum, int rows, int cols, int c,
                                                     int coarse_rows, int coarse_cols, int nperiods,
                                                     double* __restrict__ out_u, double* __restrict__ out_v,
                                                     double* __restrict__ out_speed, double* __restrict__ out_count)
{
    const int ncoarse = coarse_rows * coarse_cols;
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= nperiods * ncoarse) return;
    const int p = idx / ncoarse, k = idx - p * ncoarse;
    const int bi = k / coarse_cols, bj = k - bi * coarse_cols;
    const size_t fine = (size_t)p * (size_t)rows * (size_t)cols;
    const double cu = block_mean(mean_u + fine, rows, cols, c, coarse_cols, bi, bj);
    const double cv = block_mean(mean_v + fine, rows, cols, c, coarse_cols, bi, bj);
    out_u[idx] = cu;
    out_v[idx] = cv;
    out_speed[idx] = hypot_np(cu, cv);
    out_count[idx] = block_mean(count_sum + fine, rows, cols, c, coarse_cols, bi, bj);
}

}  // namespace

void launch_cube_temporal(hipStream_t s, const double* u, const double* v, const double* cnt, int ncells,
                          const int* sel_offset, const int* sel_index, int nperiods, double* mean_u, double* mean_v,
                          double* speed, double* count_sum, int* has_data)
{
    if (ncells <= 0 || nperiods <= 0) return;
    const int cell_blocks = (ncells + 255) / 256;
    hipLaunchKernelGGL(k_cube_temporal, dim3((unsigned)cell_blocks * (unsigned)nperiods), dim3(256), 0, s, u, v, cnt,
                       ncells, sel_offset, sel_index, cell_blocks, mean_u, mean_v, speed, count_sum, has_data);
}

void launch_cube_spatial(hipStream_t s, const double* mean_u, const double* mean_v, const double* count_sum, int rows,
                         int cols, int coarseness, int nperiods, double* out_u, double* out_v, double* out_speed,
                         double* out_count)
{
    const int cr = (rows + coarseness - 1) / coarseness, cc = (cols + coarseness - 1) / coarseness;
    const int n = nperiods * cr * cc;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_cube_spatial, dim3((n + 63) / 64), dim3(64), 0, s, mean_u, mean_v, count_sum, rows, cols,
                       coarseness, cr, cc, nperiods, out_u, out_v, out_speed, out_count);
}

}  // namespace icelk
