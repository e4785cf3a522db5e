// validate.h -- the spatial-coherence check between projection and gridding: the normalised median test
// of Westerweel & Scarano (2005, Exp. Fluids 39) on a lattice of pools, stated once for the host (icelk_validate_host,
// tests/validate_main.cpp) and the device (k_validate.hip).  It stands on grid_stats.h (np.median's bits, the order keys)
// and np_sums.h; every operation below is rounded once (-ffp-contract=off).
//
//   lattice  (left, top, side, cols, rows), independent of the gridder's cells.  A point's cell is i = floor((x - left) /
//            side), j = floor((top - y) / side).  It is JUDGED if x, y, u, v are finite, 0 <= i < cols, 0 <= j < rows and its
//            group g (a time window of the day form; one group when none is given) lies in 0 .. ngroups - 1.
//   pool     of (group g, cell i, j): every judged point of group g in the cells (i + di, j + dj), |di|, |dj| <= 1, clipped
//            at the lattice edge.  It contains the point under test, so it is never empty for a judged point and holds no
//            NaN.  The paper leaves the point under test out; leaving it out needs a median per point instead of per
//            cell: a declared difference.
//   pool statistics  med_u, mad_u, med_v, mad_v: grid_stats.h's np.median of the pool's u (v) and of fabs(u - med_u).  The
//            terms are finite, so a median is finite or -- the middle pair's sum overflowed -- infinite, never NaN; an
//            infinite median gives an infinite MAD.
//   verdict  ru = fabs(u - med_u) / (mad_u + eps), rv likewise, r2 = ru * ru + rv * rv; rejected iff r2 > threshold *
//            threshold.  A NaN r2 (infinite medians: inf / inf) compares false: kept.
//   status   0 judged and kept, 1 rejected, 2 the pool has fewer than min_neighbours + 1 terms (kept, not judged; r2 is
//            NaN), 3 not judged at all (r2 is NaN).
//
// Keys: a judged point p of segment s = g * cols * rows + j * cols + i gets the key (s << 32) | p.  The column index runs
// fastest, so the (at most) three cells of a lattice row that a pool takes are ONE run of the sorted keys and a pool is at
// most three runs; inside a run the points stand in index order, which no result depends on (the select compares
// integers only).
#pragma once
#include <stdint.h>

#include "../../include/icelk.h"
#include "grid_stats.h"

#include <algorithm>

namespace icelk {
namespace validate {

constexpr uint8_t kKept = 0, kRejected = 1, kFewNeighbours = 2, kNotJudged = 3;
constexpr int kMaxPoints = 1 << 27;

ICELK_SUMS_INLINE_FN icelk_validate_params_t default_params()
{
    icelk_validate_params_t p{};
    p.threshold = 2.0;
    p.eps = 0.01;
    p.min_neighbours = 8;
    return p;
}

// true for finite d (no libm: the same text on the host and the device)
ICELK_SUMS_INLINE_FN bool is_finite(double d) { return d - d == 0.0; }

// ICELK_OK, ICELK_EARG or ICELK_ECAP for a lattice, parameters, n points and ngroups groups
ICELK_SUMS_INLINE_FN int check(const icelk_validate_lattice_t& L, const icelk_validate_params_t& P, long long n, long long ngroups)
{
    if (!(P.threshold > 0.0) || !is_finite(P.threshold) || !(P.eps > 0.0) || !is_finite(P.eps) || !(L.side > 0.0) || !is_finite(L.side) ||
        !is_finite(L.left) || !is_finite(L.top) || P.min_neighbours < 1 || L.cols < 1 || L.rows < 1 || n < 0 || ngroups < 1)
        return ICELK_EARG;
    const long long ncells = (long long)L.cols * (long long)L.rows;
    if (n > kMaxPoints || ngroups > 0x7fffffffLL || ncells > 0x7fffffffLL || ngroups * ncells >= 0x80000000LL) return ICELK_ECAP;
    return ICELK_OK;
}

// the cell of a point: false when a coordinate or a velocity is not finite or the point lies outside the lattice
ICELK_SUMS_INLINE_FN bool cell_of(const icelk_validate_lattice_t& L, double x, double y, double u, double v, int* i, int* j)
{
    if (!is_finite(x) || !is_finite(y) || !is_finite(u) || !is_finite(v)) return false;
    const double fi = floor((x - L.left) / L.side), fj = floor((L.top - y) / L.side);
    if (!(fi >= 0.0 && fi < (double)L.cols && fj >= 0.0 && fj < (double)L.rows)) return false;
    *i = (int)fi;
    *j = (int)fj;
    return true;
}

ICELK_SUMS_INLINE_FN unsigned long long make_key(unsigned seg, int p) { return ((unsigned long long)seg << 32) | (unsigned)p; }

// first index of keys[0 .. n) whose key is >= v
ICELK_SUMS_INLINE_FN int lower_bound(const unsigned long long* keys, int n, unsigned long long v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The pool of one (group, cell): up to three runs of the sorted keys, one per lattice row, the cell's own points a part
// of the middle one.  Term t of the pool is the t-th key of the runs laid end to end.
struct Pool {
    int begin[3], count[3];
    int own_begin, own_count, n;
    ICELK_SUMS_INLINE_FN int key_index(int t) const
    {
        if (t < count[0]) return begin[0] + t;
        t -= count[0];
        return t < count[1] ? begin[1] + t : begin[2] + (t - count[1]);
    }
};

// bound k of a pool's eight: 2 r and 2 r + 1 the first and the past-the-end segment of row j - 1 + r (equal when the row
// lies outside the lattice), 6 and 7 the cell's own
ICELK_SUMS_INLINE_FN unsigned pool_bound_segment(const icelk_validate_lattice_t& L, unsigned seg, int k)
{
    const unsigned ncells = (unsigned)L.cols * (unsigned)L.rows;
    const unsigned g = seg / ncells, c = seg % ncells;
    const int j = (int)(c / (unsigned)L.cols), i = (int)(c % (unsigned)L.cols);
    if (k >= 6) return seg + (unsigned)(k - 6);
    const int jj = j - 1 + (k >> 1);
    if (jj < 0 || jj >= L.rows) return seg;                       // an empty run: begin == end
    const int i0 = i > 0 ? i - 1 : 0, i1 = i + 1 < L.cols ? i + 1 : L.cols - 1;
    return g * ncells + (unsigned)jj * (unsigned)L.cols + (unsigned)((k & 1) ? i1 + 1 : i0);
}

// where bound k lies in the sorted keys (a segment number of 2^31 is past every key: (2^31) << 32 fits the key)
ICELK_SUMS_INLINE_FN int pool_bound(const icelk_validate_lattice_t& L, const unsigned long long* keys, int total, unsigned seg, int k)
{
    return lower_bound(keys, total, (unsigned long long)pool_bound_segment(L, seg, k) << 32);
}

ICELK_SUMS_INLINE_FN Pool pool_from_bounds(const int* b)
{
    Pool P;
    for (int r = 0; r < 3; r++) P.begin[r] = b[2 * r], P.count[r] = b[2 * r + 1] - b[2 * r];
    P.own_begin = b[6];
    P.own_count = b[7] - b[6];
    P.n = P.count[0] + P.count[1] + P.count[2];
    return P;
}

// term t of a pool's u or v, through the sorted keys
struct PoolAt {
    const unsigned long long* keys;
    const double* a;
    Pool pool;
    ICELK_SUMS_INLINE_FN double operator()(int t) const { return a[(unsigned)keys[pool.key_index(t)]]; }
};

// the verdict of one point against its pool's statistics; *r2 is what was compared
ICELK_SUMS_INLINE_FN bool rejects(double u, double v, double med_u, double mad_u, double med_v, double mad_v,
                                   const icelk_validate_params_t& P, double* r2)
{
    const double ru = fabs(u - med_u) / (mad_u + P.eps), rv = fabs(v - med_v) / (mad_v + P.eps);
    *r2 = ru * ru + rv * rv;
    return *r2 > P.threshold * P.threshold;
}

// status and r2 of a keyed point whose pool has pool_n terms
ICELK_SUMS_INLINE_FN uint8_t judge(double u, double v, int pool_n, double med_u, double mad_u, double med_v, double mad_v,
                                    const icelk_validate_params_t& P, double* r2)
{
    if (pool_n <= P.min_neighbours) {   // fewer than min_neighbours + 1 terms
        *r2 = __builtin_nan("");
        return kFewNeighbours;
    }
    return rejects(u, v, med_u, mad_u, med_v, mad_v, P, r2) ? kRejected : kKept;
}

// The whole statement on the host.  group: NULL (every point in group 0) or n group numbers, those outside 0 .. ngroups - 1
// in no group.  keys: n working slots.  status, r2: n each.  pool_n, med_u, med_v, mad_u, mad_v: NULL, or ngroups * cols *
// rows each, (0, NaN, NaN, NaN, NaN) for a (group, cell) without a point of its own.  rejected: NULL or ngroups counts.
// check() has passed.  Returns the number of judged points (the keys written).
inline int run_host(const double* x, const double* y, const double* u, const double* v, int n, const int32_t* group, int ngroups,
                    const icelk_validate_lattice_t& L, const icelk_validate_params_t& P, unsigned long long* keys, uint8_t* status,
                    double* r2, const icelk_validate_cells_t* cells, int32_t* rejected)
{
    const unsigned ncells = (unsigned)L.cols * (unsigned)L.rows;
    const double nan = __builtin_nan("");
    if (cells) {
        const size_t nseg = (size_t)ncells * (size_t)ngroups;
        for (size_t s = 0; s < nseg; s++) {
            cells->pool_n[s] = 0;
            cells->med_u[s] = cells->med_v[s] = cells->mad_u[s] = cells->mad_v[s] = nan;
        }
    }
    if (rejected)
        for (int g = 0; g < ngroups; g++) rejected[g] = 0;
    int total = 0;
    for (int p = 0; p < n; p++) {
        int i = 0, j = 0;
        const int g = group ? group[p] : 0;
        status[p] = kNotJudged;
        r2[p] = nan;
        if (g < 0 || g >= ngroups || !cell_of(L, x[p], y[p], u[p], v[p], &i, &j)) continue;
        keys[total++] = make_key((unsigned)g * ncells + (unsigned)j * (unsigned)L.cols + (unsigned)i, p);
    }
    std::sort(keys, keys + total);
    for (int at = 0; at < total;) {
        const unsigned seg = (unsigned)(keys[at] >> 32);
        int b[8];
        for (int k = 0; k < 8; k++) b[k] = pool_bound(L, keys, total, seg, k);
        const Pool pool = pool_from_bounds(b);
        const PoolAt au{keys, u, pool}, av{keys, v, pool};
        const double med_u = np_median(au, pool.n), med_v = np_median(av, pool.n);
        const double mad_u = np_median(AbsDevAt<PoolAt>{au, med_u}, pool.n), mad_v = np_median(AbsDevAt<PoolAt>{av, med_v}, pool.n);
        if (cells) {
            cells->pool_n[seg] = pool.n;
            cells->med_u[seg] = med_u, cells->med_v[seg] = med_v, cells->mad_u[seg] = mad_u, cells->mad_v[seg] = mad_v;
        }
        for (int k = pool.own_begin; k < pool.own_begin + pool.own_count; k++) {
            const unsigned p = (unsigned)keys[k];
            status[p] = judge(u[p], v[p], pool.n, med_u, mad_u, med_v, mad_v, P, &r2[p]);
            if (status[p] == kRejected && rejected) rejected[seg / ncells]++;
        }
        at = pool.own_begin + pool.own_count;
    }
    return total;
}

}  // namespace validate
}  // namespace icelk
