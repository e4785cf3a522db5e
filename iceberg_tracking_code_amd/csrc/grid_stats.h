// grid_stats.h -- numpy's per-cell spread and robust centre restated for the host and the device alike: the standard
// deviation, the median and the median absolute deviation of one cell's velocities (k_grid.hip: k_grid_std,
// k_grid_select; abi_post.hip: icelk_grid_cell_stats_host; tests/grid_stats_main.cpp).  The caller says what
// "element t" is with a functor `at(t)`, as for np_sums.h.  The three rules (numpy 2.2):
//   std     np.std(a, ddof=1): m = np_sum(a) / n, d[t] = (a[t] - m) * (a[t] - m) with each operation rounded once (no
//           contraction), sqrt(np_sum(d) / (n - 1)); one term gives 0.0 / 0 = NaN.
//   median  np.median(a): NaN if a term is NaN; else from the sorted terms s, (0.0 + s[n / 2]) / 1.0 for odd n and
//           ((0.0 + s[n / 2 - 1]) + s[n / 2]) / 2.0 for even n -- np.mean of the middle, so median([-0.0]) is +0.0,
//           median([1e308, 1e308]) is inf and median([-inf, inf]) is NaN.
//   MAD     np.median(np.abs(a - np.median(a))): the same median over fabs(a[t] - med), one rounding; a NaN or
//           infinite med propagates by IEEE rules.
// The middle terms are found without sorting: float64 values map to uint64 keys of the same order (order_key), and an
// exact radix select walks the key's eight bytes from the most significant one -- a 256-bin histogram of the terms that
// share the prefix found so far, then the bin that holds the wanted rank.  Only integer compares decide, so the order
// in which terms are counted cannot change a bit.  The key maps, the pass's match rule and the median's arithmetic are
// shared; the host counts a pass with a plain loop and walks the bins (select_rank, select_bin), the device counts it with
// one workgroup and LDS atomics and finds the same bin with a scan over its 256 threads (k_grid_select).
#pragma once
#include <stdint.h>
#include <string.h>

#include "np_sums.h"

namespace icelk {

// float64 -> uint64 with the same order (negative values flipped, positive ones above them; -0.0 just below +0.0)
ICELK_SUMS_INLINE_FN unsigned long long order_key(double d)
{
    unsigned long long b;
    memcpy(&b, &d, sizeof b);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

ICELK_SUMS_INLINE_FN double from_order_key(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double d;
    memcpy(&d, &b, sizeof d);
    return d;
}

constexpr int kSelectBins = 256, kSelectPasses = 8;

// One pass's verdict: the bin that holds rank *k among the hist[] counts; *k becomes the rank inside that bin and
// *below grows by the terms in the bins before it.
ICELK_SUMS_INLINE_FN int select_bin(const int* hist, int* k, int* below)
{
    int bin = 0;
    for (; bin < kSelectBins - 1 && *k >= hist[bin]; bin++) {
        *k -= hist[bin];
        *below += hist[bin];
    }
    return bin;
}

// terms of the pass that looks at bits [shift, shift + 8): those whose bits above agree with the prefix
ICELK_SUMS_INLINE_FN bool select_matches(unsigned long long key, unsigned long long prefix, int shift)
{
    return shift == 56 || ((key ^ prefix) >> (shift + 8)) == 0;
}

// the middle of the sorted terms -> np.median: lo = s[n / 2 - 1] (even n only), hi = s[n / 2]
ICELK_SUMS_INLINE_FN double median_of_middle(double lo, double hi, int n)
{
    return (n & 1) ? (0.0 + hi) / 1.0 : ((0.0 + lo) + hi) / 2.0;
}

// which rank the select looks for: s[n / 2] for odd n, s[n / 2 - 1] for even n (the upper middle follows from it)
ICELK_SUMS_INLINE_FN int median_rank(int n) { return (n & 1) ? n / 2 : n / 2 - 1; }

// Host and one-thread form.  key_at(t): the keys of n >= 1 terms, none of them from a NaN.  Returns the key of rank k
// (0-based, ascending); *count_le = how many terms are <= it.
template <typename KeyAt>
ICELK_SUMS_FN unsigned long long select_rank(const KeyAt& key_at, int n, int k, int* count_le)
{
    unsigned long long prefix = 0;
    int below = 0, hist[kSelectBins];
    for (int pass = 0; pass < kSelectPasses; pass++) {
        const int shift = 56 - 8 * pass;
        for (int b = 0; b < kSelectBins; b++) hist[b] = 0;
        for (int t = 0; t < n; t++) {
            const unsigned long long key = key_at(t);
            if (select_matches(key, prefix, shift)) hist[(key >> shift) & 255]++;
        }
        const int bin = select_bin(hist, &k, &below);
        prefix |= (unsigned long long)bin << shift;
        if (pass == kSelectPasses - 1) *count_le = below + hist[bin];
    }
    return prefix;
}

// the smallest key above `key`, ~0 when there is none
template <typename KeyAt>
ICELK_SUMS_FN unsigned long long select_next_above(const KeyAt& key_at, int n, unsigned long long key)
{
    unsigned long long best = ~0ull;
    for (int t = 0; t < n; t++) {
        const unsigned long long q = key_at(t);
        if (q > key && q < best) best = q;
    }
    return best;
}

// the upper middle s[n / 2] of an even n, given the lower one and how many terms are <= it
ICELK_SUMS_INLINE_FN bool upper_middle_is_same(int count_le, int n) { return count_le > n / 2; }

template <typename At>
struct OrderKeyAt {
    const At& at;
    ICELK_SUMS_INLINE_FN unsigned long long operator()(int t) const { return order_key(at(t)); }
};

// fabs(at(t) - med): the terms of the MAD
template <typename At>
struct AbsDevAt {
    const At& at;
    double med;
    ICELK_SUMS_INLINE_FN double operator()(int t) const { return fabs(at(t) - med); }
};

// (at(t) - m) * (at(t) - m): the terms of the variance
template <typename At>
struct SqDevAt {
    const At& at;
    double m;
    ICELK_SUMS_INLINE_FN double operator()(int t) const
    {
        const double d = at(t) - m;
        return d * d;
    }
};

// np.std(a, ddof=1) given m = np_sum(a) / n
template <typename At>
ICELK_SUMS_FN double np_std_ddof1(const At& at, int n, double m)
{
    return sqrt(np_sum(SqDevAt<At>{at, m}, n) / (double)(n - 1));
}

// np.median over at(0) .. at(n - 1), n >= 1
template <typename At>
ICELK_SUMS_FN double np_median(const At& at, int n)
{
    for (int t = 0; t < n; t++) {
        const double x = at(t);
        if (x != x) return x;
    }
    const OrderKeyAt<At> keys{at};
    int count_le = 0;
    const unsigned long long a = select_rank(keys, n, median_rank(n), &count_le);
    unsigned long long b = a;
    if (!(n & 1) && !upper_middle_is_same(count_le, n)) b = select_next_above(keys, n, a);
    return median_of_middle(from_order_key(a), from_order_key(b), n);
}

// the three statistics of one cell; n == 0 gives NaN in all of them
template <typename At>
ICELK_SUMS_FN void cell_stats(const At& at, int n, double* out_std, double* out_median, double* out_mad)
{
    if (n <= 0) {
        *out_std = *out_median = *out_mad = __builtin_nan("");
        return;
    }
    *out_std = np_std_ddof1(at, n, np_sum(at, n) / (double)n);
    const double med = np_median(at, n);
    *out_median = med;
    *out_mad = np_median(AbsDevAt<At>{at, med}, n);
}

}  // namespace icelk
