// np_sums.h -- numpy's float64 arithmetic restated for the device, shared by k_grid.hip (per-cell sums of a window's
// velocities, reached through sorted keys) and k_cube.hip (the c x c blocks of spatial_mean, strided).  The caller
// says what "element t" is with a functor `at(t)`; the order of the additions is numpy's and must not change:
// np.sum over a contiguous run adds below 8 terms one after the other from 0.0, otherwise in 8 accumulators, in blocks
// of at most 128 terms, the halves of a longer run aligned to 8 (numpy/core/src/umath/loops_utils.h.src).
// Plain C++ for the host and the device alike: tests/np_sums_main.cpp runs this text on the CPU against numpy itself.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ICELK_SUMS_FN __host__ __device__ inline
#define ICELK_SUMS_INLINE_FN __host__ __device__ __forceinline__
#else
#include <math.h>
#include <stddef.h>
#define ICELK_SUMS_FN inline
#define ICELK_SUMS_INLINE_FN inline
#endif

namespace icelk {

template <typename At>
ICELK_SUMS_INLINE_FN double np_leaf_sum(const At& at, int start, int n)
{
    if (n < 8) {
        double r = 0.0;
        for (int t = 0; t < n; t++) r += at(start + t);
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = at(start + j);
    int t = 8;
    for (; t < n - (n % 8); t += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] += at(start + t + j);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; t < n; t++) res += at(start + t);
    return res;
}

// numpy's pairwise sum over at(first) .. at(first + n - 1), without recursion
template <typename At>
ICELK_SUMS_FN double np_pairwise_sum(const At& at, int n, int first = 0)
{
    struct Frame { int start, n, stage; };
    Frame st[40];
    double vals[40];
    int fp = 0, sp = 0;
    st[fp++] = Frame{first, n, 0};
    while (fp) {
        Frame& f = st[fp - 1];
        if (f.n <= 128) {
            vals[sp++] = np_leaf_sum(at, f.start, f.n);
            fp--;
            continue;
        }
        int n2 = f.n / 2;
        n2 -= n2 % 8;
        if (f.stage == 0) {
            f.stage = 1;
            st[fp++] = Frame{f.start, n2, 0};
        } else if (f.stage == 1) {
            f.stage = 2;
            st[fp++] = Frame{f.start + n2, f.n - n2, 0};
        } else {
            const double r = vals[sp - 2] + vals[sp - 1];
            sp -= 2;
            vals[sp++] = r;
            fp--;
        }
    }
    return vals[0];
}

// np.sum (np.add.reduce, np.mean's sum) over a contiguous run at(0) .. at(n - 1).  numpy's reduction runs through its
// buffered iterator, so the pairwise routine never sees more than the buffer's 8192 elements at a time: from 0.0, one
// chunk of at most 8192 consecutive terms after the other, each chunk pairwise.  Up to 8192 terms that is
// 0.0 + np_pairwise_sum; beyond, one pairwise run over all n terms gives other bits (numpy 2.2).
constexpr int kNpBufferSize = 8192;

// acc + the terms at(0) .. at(n - 1) of one inner loop of a numpy reduction, chunk by chunk
template <typename At>
ICELK_SUMS_FN double np_sum_onto(double acc, const At& at, int n)
{
    for (int first = 0; first < n; first += kNpBufferSize)
        acc = acc + np_pairwise_sum(at, n - first < kNpBufferSize ? n - first : kNpBufferSize, first);
    return acc;
}

template <typename At>
ICELK_SUMS_FN double np_sum(const At& at, int n)
{
    return np_sum_onto(0.0, at, n);
}

// np.hypot: glibc's algorithm (see k_utm.hip hypot_ref)
ICELK_SUMS_INLINE_FN double hypot_np(double x, double y)
{
    double ax = fabs(x), ay = fabs(y);
    if (ax == HUGE_VAL || ay == HUGE_VAL) return HUGE_VAL;   // not isinf: hipcc's host pass has no host isinf in this scope
    if (ax != ax || ay != ay) return ax + ay;
    if (ax < ay) { const double t = ax; ax = ay; ay = t; }
    if (ay <= ax * 0x1p-54) return ax + ay;
    double h = sqrt(ax * ax + ay * ay), t1, t2;
    if (h <= 2.0 * ay) {
        const double delta = h - ay;
        t1 = ax * (2.0 * delta - ax);
        t2 = (delta - 2.0 * (ax - ay)) * delta;
    } else {
        const double delta = h - ax;
        t1 = 2.0 * delta * (ax - 2.0 * ay);
        t2 = (4.0 * delta - ay) * ay + delta * delta;
    }
    h -= (t1 + t2) / (2.0 * h);
    return h;
}

}  // namespace icelk
