// tides.h -- the per-cell harmonic fit of the velocity cube, stated once for the host (icelk_tide_fit_host,
// tests/tides_main.cpp) and the device (k_tides.hip).  Plain C++; every operation below is rounded once (-ffp-contract=off)
// and every addition stands in a stated order, so the two agree bit for bit.  No sine or cosine is evaluated here: the
// basis table B[nt][m] (float64, row t the m terms at window t) is made by the caller.
//
//   sample   window t is a sample of a cell iff u and v are finite and count >= min_count (false for a NaN count).  u and
//            v share their samples, hence one normal matrix per cell.
//   sums     A[i][j] = sum B[t][i] * B[t][j] (j <= i), ru[i] = sum B[t][i] * u[t], rv likewise, su = sum u[t], sv = sum
//            v[t], over the cell's samples.  CHUNKED SEQUENTIAL: the windows are taken in chunks of kTideChunk; within a
//            chunk the terms are added in ascending window order onto +0.0, a window that is no sample adds nothing (it is
//            skipped, no +0.0 is added); the chunk totals -- +0.0 for a chunk without a sample -- are added in ascending
//            order onto +0.0.  The chunk length is part of the rule, not a tuning knob: it is what lets the time axis be
//            dealt out to threads.
//   scalars  n (samples), first and last (window index of the first and the last sample, -1 without one).
//   status   1 (too few) when n < max(min_samples, m).  Otherwise Cholesky A = L L^T row by row (factor_solve below, the
//            subtractions in ascending k); 2 (rank deficient) when a pivot s fails s > kTidePivotTol * A[j][j].  Otherwise
//            forward and back substitution for u and for v, and status 0.
//   second pass  for each sample pred = c[0] * B[t][0] + c[1] * B[t][1] + ... (j ascending, the first term not added to
//            zero), res = u - pred; ss_res = sum res * res and ss_tot = sum (u - mean) * (u - mean), mean = su / n, both in
//            the chunked order.  rms = sqrt(ss_res / (n - m)), NaN for n == m; explained = 1 - ss_res / ss_tot, whatever the
//            division gives.  The residual cube holds res at a sample and NaN elsewhere.
//   status != 0  coefficients, rms, explained and the whole residual column of the cell are NaN.
//
// kTidePivotTol = 2^-30 is policy, not a measurement: a pivot that has lost 30 of its 53 bits to cancellation leaves
// coefficients nobody should read.  kTideMaxTerms = 18: the mean, eight constituents, an optional trend.
#pragma once
#include <stdint.h>

#include "../../include/icelk.h"
#include "np_sums.h"

#if defined(__HIPCC__)
#define ICELK_TIDE_UNROLL _Pragma("unroll")
#else
#define ICELK_TIDE_UNROLL _Pragma("GCC unroll 18")
#endif

namespace icelk {
namespace tides {

constexpr int kTideChunk = 256;
constexpr int kTideMaxTerms = 18;
constexpr double kTidePivotTol = 1.0 / 1073741824.0;   // 2^-30
constexpr int32_t kOk = 0, kTooFew = 1, kRankDeficient = 2;

// true for finite d (no libm: the same text on the host and the device)
ICELK_SUMS_INLINE_FN bool is_finite(double d) { return d - d == 0.0; }

ICELK_SUMS_INLINE_FN bool is_sample(double u, double v, double count, double min_count)
{
    return is_finite(u) && is_finite(v) && count >= min_count;
}

// The sums of one cell, numbered: the lower triangle row by row, ru, rv, su, sv.
ICELK_SUMS_INLINE_FN int n_tri(int m) { return m * (m + 1) / 2; }
ICELK_SUMS_INLINE_FN int n_sums(int m) { return n_tri(m) + 2 * m + 2; }
ICELK_SUMS_INLINE_FN int slot_a(int i, int j) { return i * (i + 1) / 2 + j; }
ICELK_SUMS_INLINE_FN int slot_ru(int m, int i) { return n_tri(m) + i; }
ICELK_SUMS_INLINE_FN int slot_rv(int m, int i) { return n_tri(m) + m + i; }
ICELK_SUMS_INLINE_FN int slot_su(int m) { return n_tri(m) + 2 * m; }
ICELK_SUMS_INLINE_FN int slot_sv(int m) { return n_tri(m) + 2 * m + 1; }
ICELK_SUMS_INLINE_FN int n_chunks(int nt) { return (nt + kTideChunk - 1) / kTideChunk; }
constexpr int kMaxSums = kTideMaxTerms * (kTideMaxTerms + 1) / 2 + 2 * kTideMaxTerms + 2;
constexpr int kRowAcc = kTideMaxTerms + 2;   // a row's accumulators: A[i][0 .. i], then ru[i] and rv[i] in the last two

// ICELK_OK, ICELK_EARG or ICELK_ECAP for a cube of ncells x nt and m terms
ICELK_SUMS_INLINE_FN int check(long long ncells, long long nt, long long m, long long min_samples)
{
    if (ncells < 1 || nt < 1 || m < 1 || min_samples < 0) return ICELK_EARG;
    if (m > kTideMaxTerms || ncells > 0x7fffffffLL || nt > 0x7fffffffLL || ncells * nt > 0x7fffffffLL) return ICELK_ECAP;
    const long long chunks = (nt + kTideChunk - 1) / kTideChunk;
    // the workspace of chunk partials, [sum][chunk][cell], is indexed in 31 bits; the chunk axis is a grid dimension
    if (chunks > 65535 || (long long)n_sums((int)m) * chunks * ncells > 0x7fffffffLL) return ICELK_ECAP;
    return ICELK_OK;
}

// One sample into row i's accumulators: acc[j] += B[t][i] * B[t][j] for j <= i, then ru[i] and rv[i].  b: row t of the basis
// (read at j <= i only, every index static after unrolling: the device hands in registers), bi = b[i].
ICELK_SUMS_INLINE_FN void add_row(double* acc, const double* b, double bi, int i, double u, double v)
{
    ICELK_TIDE_UNROLL
    for (int j = 0; j < kTideMaxTerms; j++)
        if (j <= i) acc[j] = acc[j] + bi * b[j];
    acc[kTideMaxTerms] = acc[kTideMaxTerms] + bi * u;
    acc[kTideMaxTerms + 1] = acc[kTideMaxTerms + 1] + bi * v;
}

// the sums of one cell, `stride` doubles apart (1 on the host; the cell count on the device, where the cell runs fastest)
struct CellSums {
    double* p;
    size_t stride;
    ICELK_SUMS_INLINE_FN double& operator[](int k) const { return p[(size_t)k * stride]; }
};

// Status of a cell with n samples whose totals stand in W; for status 0 the factor replaces A and the coefficients of u
// and v replace ru and rv.
ICELK_SUMS_INLINE_FN int32_t factor_solve(const CellSums& W, int m, int n, int min_samples)
{
    if (n < (min_samples > m ? min_samples : m)) return kTooFew;
    for (int i = 0; i < m; i++)
        for (int j = 0; j <= i; j++) {
            const double d = W[slot_a(i, j)];
            double s = d;
            for (int k = 0; k < j; k++) s = s - W[slot_a(i, k)] * W[slot_a(j, k)];
            if (j < i) {
                W[slot_a(i, j)] = s / W[slot_a(j, j)];
            } else {
                if (!(s > kTidePivotTol * d)) return kRankDeficient;
                W[slot_a(i, i)] = sqrt(s);
            }
        }
    for (int comp = 0; comp < 2; comp++) {
        const int r = n_tri(m) + comp * m;
        for (int i = 0; i < m; i++) {   // L y = r
            double s = W[r + i];
            for (int k = 0; k < i; k++) s = s - W[slot_a(i, k)] * W[r + k];
            W[r + i] = s / W[slot_a(i, i)];
        }
        for (int i = m - 1; i >= 0; i--) {   // L^T c = y
            double s = W[r + i];
            for (int k = i + 1; k < m; k++) s = s - W[slot_a(k, i)] * W[r + k];
            W[r + i] = s / W[slot_a(i, i)];
        }
    }
    return kOk;
}

// c[0] * b[0] + c[1] * b[1] + ... + c[m - 1] * b[m - 1]; c has kTideMaxTerms slots
ICELK_SUMS_INLINE_FN double predict(const double* c, const double* b, int m)
{
    double p = c[0] * b[0];
    ICELK_TIDE_UNROLL
    for (int j = 1; j < kTideMaxTerms; j++)
        if (j < m) p = p + c[j] * b[j];
    return p;
}

ICELK_SUMS_INLINE_FN void finish(double ss_res, double ss_tot, int n, int m, int32_t status, double* rms, double* explained)
{
    if (status != kOk) {
        *rms = *explained = __builtin_nan("");
        return;
    }
    *rms = n == m ? __builtin_nan("") : sqrt(ss_res / (double)(n - m));
    *explained = 1.0 - ss_res / ss_tot;
}

// what a fit writes: coef [cell][m]; the others one per cell; residual_u, residual_v NULL or [window][cell]
struct FitOut {
    double *coef_u, *coef_v, *rms_u, *rms_v, *explained_u, *explained_v;
    int32_t *n, *first, *last, *status;
    double *residual_u, *residual_v;
};

// The whole statement on the host, cell by cell.  u, v, count: [window][cell]; check() has passed.
inline void fit_host(const double* u, const double* v, const double* count, int ncells, int nt, const double* basis, int m,
                     double min_count, int min_samples, const FitOut& O)
{
    const double nan = __builtin_nan("");
    const int nsums = n_sums(m), chunks = n_chunks(nt);
    for (int cell = 0; cell < ncells; cell++) {
        double W[kMaxSums];
        for (int s = 0; s < nsums; s++) W[s] = 0.0;
        int n = 0, first = -1, last = -1;
        for (int ch = 0; ch < chunks; ch++) {
            double part[kMaxSums];
            for (int s = 0; s < nsums; s++) part[s] = 0.0;
            const int t1 = (ch + 1) * kTideChunk < nt ? (ch + 1) * kTideChunk : nt;
            for (int t = ch * kTideChunk; t < t1; t++) {
                const size_t at = (size_t)t * (size_t)ncells + (size_t)cell;
                if (!is_sample(u[at], v[at], count[at], min_count)) continue;
                const double* b = basis + (size_t)t * (size_t)m;
                for (int i = 0; i < m; i++) {
                    double acc[kRowAcc];
                    for (int j = 0; j <= i; j++) acc[j] = part[slot_a(i, j)];
                    for (int j = i + 1; j < kTideMaxTerms; j++) acc[j] = 0.0;
                    acc[kTideMaxTerms] = part[slot_ru(m, i)], acc[kTideMaxTerms + 1] = part[slot_rv(m, i)];
                    add_row(acc, b, b[i], i, u[at], v[at]);
                    for (int j = 0; j <= i; j++) part[slot_a(i, j)] = acc[j];
                    part[slot_ru(m, i)] = acc[kTideMaxTerms], part[slot_rv(m, i)] = acc[kTideMaxTerms + 1];
                }
                part[slot_su(m)] = part[slot_su(m)] + u[at];
                part[slot_sv(m)] = part[slot_sv(m)] + v[at];
                n++;
                if (first < 0) first = t;
                last = t;
            }
            for (int s = 0; s < nsums; s++) W[s] = W[s] + part[s];
        }
        const double mean_u = W[slot_su(m)] / (double)n, mean_v = W[slot_sv(m)] / (double)n;
        const int32_t status = factor_solve(CellSums{W, 1}, m, n, min_samples);
        double cu[kTideMaxTerms], cv[kTideMaxTerms];
        for (int j = 0; j < kTideMaxTerms; j++) {
            cu[j] = j < m && status == kOk ? W[slot_ru(m, j)] : nan;
            cv[j] = j < m && status == kOk ? W[slot_rv(m, j)] : nan;
        }
        for (int j = 0; j < m; j++) O.coef_u[(size_t)cell * m + j] = cu[j], O.coef_v[(size_t)cell * m + j] = cv[j];
        O.n[cell] = n, O.first[cell] = first, O.last[cell] = last, O.status[cell] = status;
        double ss[4] = {0.0, 0.0, 0.0, 0.0};   // res u, res v, tot u, tot v
        for (int ch = 0; ch < chunks; ch++) {
            double part[4] = {0.0, 0.0, 0.0, 0.0};
            const int t1 = (ch + 1) * kTideChunk < nt ? (ch + 1) * kTideChunk : nt;
            for (int t = ch * kTideChunk; t < t1; t++) {
                const size_t at = (size_t)t * (size_t)ncells + (size_t)cell;
                double res_u = nan, res_v = nan;
                if (status == kOk && is_sample(u[at], v[at], count[at], min_count)) {
                    const double* b = basis + (size_t)t * (size_t)m;
                    res_u = u[at] - predict(cu, b, m);
                    res_v = v[at] - predict(cv, b, m);
                    const double du = u[at] - mean_u, dv = v[at] - mean_v;
                    part[0] = part[0] + res_u * res_u;
                    part[1] = part[1] + res_v * res_v;
                    part[2] = part[2] + du * du;
                    part[3] = part[3] + dv * dv;
                }
                if (O.residual_u) O.residual_u[at] = res_u;
                if (O.residual_v) O.residual_v[at] = res_v;
            }
            for (int k = 0; k < 4; k++) ss[k] = ss[k] + part[k];
        }
        finish(ss[0], ss[2], n, m, status, &O.rms_u[cell], &O.explained_u[cell]);
        finish(ss[1], ss[3], n, m, status, &O.rms_v[cell], &O.explained_v[cell]);
    }
}

}  // namespace tides
}  // namespace icelk
