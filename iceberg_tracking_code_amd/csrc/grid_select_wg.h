// grid_select_wg.h -- the exact radix select of grid_stats.h carried out by one workgroup of 256: what k_grid_select
// (k_grid.hip: a cell's median and MAD) and k_stab_median (k_stab.hip: the start shift of a vertex) share.  Device code
// only; the rules and the host's form are grid_stats.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "grid_stats.h"

namespace icelk {

static_assert(kSelectBins == 256, "k_grid_select: one thread per histogram bin");

struct SelectLds {
    int hist[kSelectBins];
    int wave_tot[4];
    int bin, before, in_bin;          // the pass's verdict, from the thread that owns the bin
    unsigned long long above;
};

// select_bin of grid_stats.h by the workgroup: thread x owns bin x, an exclusive scan of the counts (wave shuffles, then
// the four wave totals) tells it the ranks its bin holds, and the one thread whose bin holds rank k says so.  k is below
// the number of counted terms, so there is exactly one.
__device__ __forceinline__ int wg_select_bin(SelectLds* L, int* k, int* below, int* in_bin)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mine = L->hist[threadIdx.x];
    int inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) L->wave_tot[wave] = inc;
    __syncthreads();
    int before = inc - mine;
    for (int w = 0; w < wave; w++) before += L->wave_tot[w];
    if (*k >= before && *k < before + mine) {
        L->bin = threadIdx.x;
        L->before = before;
        L->in_bin = mine;
    }
    __syncthreads();
    *k -= L->before;
    *below += L->before;
    *in_bin = L->in_bin;
    return L->bin;
}

// np.median of the n >= 1 terms whose order keys are sk[0 .. n), none from a NaN, by the whole workgroup: select_rank
// of grid_stats.h with each pass's histogram counted by 256 threads in LDS.  Every thread walks the same t it staged,
// reads the same verdict and so carries the same prefix, rank and count; eight passes and at most one more.  A pass's
// verdict is written two barriers after the last one was read, and a thread zeroes only the bin it alone has read.
// `sk[t]` is whatever the caller's Keys answers for term t -- an array in global memory (wg_median below), keys staged in
// LDS or computed on the way (k_validate.hip); it is asked for the same t up to ten times and must answer alike.
template <typename Keys>
__device__ __forceinline__ double wg_median_of(const Keys& sk, int n, SelectLds* L)
{
    int k = median_rank(n), below = 0, in_bin = 0;
    unsigned long long prefix = 0;
    for (int pass = 0; pass < kSelectPasses; pass++) {
        const int shift = 56 - 8 * pass;
        L->hist[threadIdx.x] = 0;
        __syncthreads();
        for (int t = threadIdx.x; t < n; t += 256) {
            const unsigned long long key = sk[t];
            if (select_matches(key, prefix, shift)) atomicAdd(&L->hist[(key >> shift) & 255], 1);
        }
        __syncthreads();
        const int bin = wg_select_bin(L, &k, &below, &in_bin);
        prefix |= (unsigned long long)bin << shift;
    }
    unsigned long long upper = prefix;
    unsigned long long* s_min = &L->above;
    if (!(n & 1) && !upper_middle_is_same(below + in_bin, n)) {     // the smallest term above the lower middle
        if (threadIdx.x == 0) *s_min = ~0ull;
        __syncthreads();
        unsigned long long best = ~0ull;
        for (int t = threadIdx.x; t < n; t += 256) {
            const unsigned long long q = sk[t];
            if (q > prefix && q < best) best = q;
        }
        if (best != ~0ull) atomicMin(s_min, best);
        __syncthreads();
        upper = *s_min;
    }
    return median_of_middle(from_order_key(prefix), from_order_key(upper), n);
}

// order keys in an array
struct KeyArray {
    const unsigned long long* __restrict__ p;
    __device__ __forceinline__ unsigned long long operator[](int t) const { return p[t]; }
};

__device__ __forceinline__ double wg_median(const unsigned long long* __restrict__ sk, int n, SelectLds* L)
{
    return wg_median_of(KeyArray{sk}, n, L);
}

}  // namespace icelk
