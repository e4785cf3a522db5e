// grid_keys.h -- what the kernels that turn points into sorted (segment, point) keys share: k_grid.hip (the gridder, the
// boxes) and k_validate.hip (the pools of the normalised median test).  Device code only.
//
// A key holds its segment in the high 32 bits -- a cell, a box, or window * segments-per-window + that -- and the point
// index in the low 32; sorted ascending (k_sort.hip) the keys of a segment are one run, its points in index order.
#pragma once
#include <hip/hip_runtime.h>

namespace icelk {

// the first of the cnt key slots of this thread: one block-wide scan of the counts, one atomic per workgroup.  Every
// thread of the 256 calls it, once per kernel.
__device__ __forceinline__ int key_slots(int cnt, int* __restrict__ key_count)
{
    __shared__ int wave_tot[4];
    __shared__ int s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    int wbase = 0, total = 0;
    for (int k = 0; k < 4; k++) {
        wbase += k < wave ? wave_tot[k] : 0;
        total += wave_tot[k];
    }
    if (threadIdx.x == 0) s_base = total ? atomicAdd(key_count, total) : 0;
    __syncthreads();
    return s_base + wbase + inc - cnt;
}

// ---- a whole day of time windows in one pass (icelk_grid_bin_windows) ------------------------------------------
// The points of every loaded hour file, concatenated; file f holds [file_off[f], file_off[f + 1]) and belongs to
// camera file_cam[f].  Camera c's window w (slot c * nw + w) loads files win_f0 .. win_f1 (none when f0 > f1) and
// keeps the times in [t_lo, t_hi) -- int64 epoch seconds compared as float64, as numpy compares the float64 time
// array with a Python int.  The windows of a camera are disjoint and ascending, so a binary search finds the only one
// that can hold a time; the point counts only if that window loads its file.  NaN lies in no window.
struct DayTables {
    const long long* file_off;
    const int* file_cam;
    const int* win_f0;
    const int* win_f1;
    const long long* t_lo;
    const long long* t_hi;
    int nfiles, ncam, nw;
};

// the window of point p, -1 for none; *cam its camera and *tp its time (both set whenever p < n)
__device__ __forceinline__ int day_window(const DayTables& D, const double* __restrict__ t, int p, int n, int* cam,
                                          double* tp)
{
    *cam = 0;
    *tp = 0.0;
    if (p >= n) return -1;
    int f = 0, hi = D.nfiles - 1;                       // last file starting at or before p (empty files skipped)
    while (f < hi) {
        const int mid = (f + hi + 1) >> 1;
        if (D.file_off[mid] <= p) f = mid;
        else hi = mid - 1;
    }
    *cam = D.file_cam[f];
    *tp = t[p];
    const long long* lo = D.t_lo + (size_t)*cam * D.nw;
    int a = 0, b = D.nw;                                // windows starting at or before tp
    while (a < b) {
        const int mid = (a + b) >> 1;
        if ((double)lo[mid] <= *tp) a = mid + 1;
        else b = mid;
    }
    const int wc = a - 1;
    const size_t sl = (size_t)*cam * D.nw + wc;
    if (wc >= 0 && f >= D.win_f0[sl] && f <= D.win_f1[sl] && *tp < (double)D.t_hi[sl]) return wc;
    return -1;
}

}  // namespace icelk
