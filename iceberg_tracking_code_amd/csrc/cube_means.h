// cube_means.h -- the arithmetic of spatial_mean (s4_postprocess_gridded_utm.py:264-287, nanmean = 0) for one coarse
// cell, as plain C++ for the host and the device alike: k_cube.hip's k_cube_spatial and tests/np_sums_main.cpp run this
// text.  np.mean(axis = (1, 3)) of the zero-padded (R/c, c, C/c, c) view, in numpy's order of additions:
// - two or more coarse columns: per coarse cell, from 0.0, one row of the block after the other, each row of c terms by
//   numpy's pairwise routine (np_sums.h) -- a row of more than 8192 terms in the chunks of numpy's buffer, each added
//   to the running sum as it comes;
// - a single coarse column (cols <= c): numpy merges the two block axes, the c * c terms of a block are one contiguous
//   run, added as np.sum adds one (np_sum: chunks of 8192 terms, each pairwise -- a single chunk up to c = 90).
// The divisor is c * c whatever the padding, NaN propagates.  Verified against numpy up to kMaxCoarseness.
#pragma once
#include "np_sums.h"

namespace icelk {

constexpr int kMaxCoarseness = 8193;    // the largest coarseness checked against numpy: c * c fits 31 bits far beyond it

// element b of block row r, columns from c0: the field inside, the zero padding outside
struct RowAt {
    const double* __restrict__ f;
    int rows, cols, r, c0;
    ICELK_SUMS_INLINE_FN double operator()(int b) const
    {
        const int col = c0 + b;
        return r < rows && col < cols ? f[(size_t)r * cols + col] : 0.0;
    }
};

// element t of a whole c x c block in row-major order (a single coarse column: numpy merges the two block axes)
struct BlockAt {
    const double* __restrict__ f;
    int rows, cols, r0, c;
    ICELK_SUMS_INLINE_FN double operator()(int t) const
    {
        const int r = r0 + t / c, col = t % c;
        return r < rows && col < cols ? f[(size_t)r * cols + col] : 0.0;
    }
};

ICELK_SUMS_FN double block_mean(const double* __restrict__ f, int rows, int cols, int c, int coarse_cols, int bi, int bj)
{
    // Below the field there is padding only: a row or a chunk of zeros adds +0.0, which changes no sum (the running sum
    // starts at +0.0 and so is never -0.0).  They are left out; the chunks keep their places.
    const int r0 = bi * c, inside = rows - r0 < c ? rows - r0 : c;      // block rows that hold cells of the field
    double acc = 0.0;
    if (coarse_cols == 1) {
        const int chunks = (inside * c + kNpBufferSize - 1) / kNpBufferSize;
        const int n = c * c < chunks * kNpBufferSize ? c * c : chunks * kNpBufferSize;
        acc = np_sum(BlockAt{f, rows, cols, r0, c}, n);
    } else {
        for (int a = 0; a < inside; a++) acc = np_sum_onto(acc, RowAt{f, rows, cols, r0 + a, bj * c}, c);
    }
    return acc / (double)(c * c);
}

}  // namespace icelk
