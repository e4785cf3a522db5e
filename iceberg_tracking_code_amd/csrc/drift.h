// drift.h -- virtual drifters advected through the gridded velocities, stated once for the host
// (icelk_drift_host, tests/drift_main.cpp) and the device (k_drift.hip).  Plain C++, everything in double; every operation
// below is rounded once (-ffp-contract=off) and stands in a stated order, so the two agree bit for bit.  No time axis is
// searched and no sine is evaluated here: the schedule table, one row per half step, is made by the caller.
//
//   lattice   nodes x0 + i * dx (i < cols), y0 + j * dy (j < rows), cell = j * cols + i; row 0 is the northern row, dy < 0.
//   clock     t_s = start + s * step, s = 0 .. nsteps; schedule row r is the time start + r * step / 2, r = 0 .. 2 * nsteps.
//   field     what a source knows at a schedule row: row(r) takes the row, has_field() is its flag, node(cell, &u, &v) is
//             true for a measured node and then gives its value.
//     cube    row r: windows k0 <= k1, weight a, flag.  A window's node is measured iff u, v are finite and count >=
//             min_count; the node iff both windows' are; its value (1 - a) * u[k0] + a * u[k1], v likewise.
//     tide    row r: m basis terms B.  The node is measured iff the cell's status is 0; its value coef[cell][0] * B[0] +
//             coef[cell][1] * B[1] + ... (j ascending, the first term not added to zero).  The flag is always set.
//   sample    fx = (px - x0) / dx, fy = (py - y0) / dy.  Outside unless 0 <= fx <= cols - 1 and 0 <= fy <= rows - 1 (a NaN
//             fails both).  i = min(floor(fx), cols - 2), j likewise, tx = fx - i, ty = fy - j.  Weights (1 - tx) * (1 - ty),
//             tx * (1 - ty), (1 - tx) * ty, tx * ty over the nodes (j, i), (j, i + 1), (j + 1, i), (j + 1, i + 1).  All four
//             measured: ((w0 * u0 + w1 * u1) + w2 * u2) + w3 * u3, no division.  Fewer: the measured terms added in that order
//             onto +0.0, and their weights likewise; with at least min_nodes of them and a weight sum > 0 the sample is the
//             one sum divided by the other, else it fails (too few measured nodes).
//   stage     fails with no-field when the row's flag is 0, else with left-the-lattice when the position is outside, else
//             with too-few when the sample fails.
//   step s    order 1: k1 at (p, row 2s); p' = p + step * k1.
//             order 2: k2 at (p + (step / 2) * k1, row 2s + 1); p' = p + step * k2.
//             order 4: k3 at (p + (step / 2) * k2, row 2s + 1), k4 at (p + step * k3, row 2s + 2);
//                      p' = p + (step / 6) * (((k1 + 2 * k2) + 2 * k3) + k4).
//             The first stage that fails stops the drifter: it stays at p, status is the stage's reason, stop_step is s.  A
//             non-finite p' stops it likewise, as left-the-lattice.
//   release   drifter p exists from step release[p] on, at its seed, iff the seed is finite and 0 <= release[p] < nsteps;
//             otherwise it is never released: status 4, stop_step -1, last position NaN, length 0.
//   outputs   x, y [n_out][n] at the steps 0, every, 2 * every, ...: the position while release <= s <= stop_step (nsteps for
//             a drifter alive at the end), NaN otherwise.  length: hypot_np of the step displacements added in step order
//             onto +0.0.  visits: every finite recorded sample adds one to the node (floor(fy + 0.5), floor(fx + 0.5)) when
//             that node is on the lattice.
#pragma once
#include <stdint.h>

#include "../../include/icelk.h"
#include "np_sums.h"

#if defined(__HIPCC__)
#define ICELK_DRIFT_UNROLL _Pragma("unroll")
#else
#define ICELK_DRIFT_UNROLL _Pragma("GCC unroll 18")
#endif

namespace icelk {
namespace drift {

constexpr int kMaxTerms = 18;   // tides::kTideMaxTerms
constexpr int32_t kAlive = 0, kLeft = 1, kTooFew = 2, kNoField = 3, kNeverReleased = 4;

// true for finite d (no libm: the same text on the host and the device)
ICELK_SUMS_INLINE_FN bool is_finite(double d) { return d - d == 0.0; }

// ICELK_OK, ICELK_EARG or ICELK_ECAP for n drifters on the lattice and a tide source of m terms (m = 0: the cube source)
ICELK_SUMS_INLINE_FN int check(const icelk_drift_lattice_t& L, const icelk_drift_params_t& P, long long n, long long m)
{
    if (!is_finite(L.x0) || !is_finite(L.y0) || !is_finite(L.dx) || !is_finite(L.dy) || L.dx == 0.0 || L.dy == 0.0) return ICELK_EARG;
    if (L.rows < 2 || L.cols < 2 || n < 1 || m < 0) return ICELK_EARG;
    if (!is_finite(P.step) || P.step == 0.0 || P.nsteps < 1 || P.every < 1) return ICELK_EARG;
    if ((P.order != 1 && P.order != 2 && P.order != 4) || P.min_nodes < 1 || P.min_nodes > 4) return ICELK_EARG;
    if (m > kMaxTerms || (long long)L.rows * L.cols > 0x7fffffffLL) return ICELK_ECAP;
    const long long n_out = P.nsteps / P.every + 1, sched = 2LL * P.nsteps + 1;
    if (n > 0x7fffffffLL || n * n_out > 0x7fffffffLL || sched > 0x7fffffffLL || sched * (m > 0 ? m : 1) > 0x7fffffffLL) return ICELK_ECAP;
    return ICELK_OK;
}

ICELK_SUMS_INLINE_FN int n_out(const icelk_drift_params_t& P) { return P.nsteps / P.every + 1; }

// the cube source.  u, v, count: [window][cell]; k0, k1, a, flag: one per schedule row, 0 <= k0, k1 < windows
struct CubeField {
    const double *u, *v, *count;
    size_t ncells;
    const int32_t *k0, *k1, *flag;
    const double* a;
    double min_count;
    size_t at0, at1;   // the current row
    double w;
    int32_t on;
    ICELK_SUMS_INLINE_FN void row(int r)
    {
        at0 = (size_t)k0[r] * ncells, at1 = (size_t)k1[r] * ncells;
        w = a[r];
        on = flag[r];
    }
    ICELK_SUMS_INLINE_FN bool has_field() const { return on != 0; }
    ICELK_SUMS_INLINE_FN bool window(size_t at) const { return is_finite(u[at]) && is_finite(v[at]) && count[at] >= min_count; }
    ICELK_SUMS_INLINE_FN bool node(size_t cell, double* nu, double* nv) const
    {
        const size_t p = at0 + cell, q = at1 + cell;
        if (!window(p) || !window(q)) return false;
        *nu = (1.0 - w) * u[p] + w * u[q];
        *nv = (1.0 - w) * v[p] + w * v[q];
        return true;
    }
};

// the tide source.  coef [cell][m], status [cell], basis [schedule row][m]
struct TideField {
    const double *coef_u, *coef_v;
    const int32_t* status;
    const double* basis;
    int m;
    double b[kMaxTerms];   // the current row
    ICELK_SUMS_INLINE_FN void row(int r)
    {
        const double* q = basis + (size_t)r * (size_t)m;
        ICELK_DRIFT_UNROLL
        for (int j = 0; j < kMaxTerms; j++) b[j] = j < m ? q[j] : 0.0;
    }
    ICELK_SUMS_INLINE_FN bool has_field() const { return true; }
    ICELK_SUMS_INLINE_FN double predict(const double* c) const
    {
        double p = c[0] * b[0];
        ICELK_DRIFT_UNROLL
        for (int j = 1; j < kMaxTerms; j++)
            if (j < m) p = p + c[j] * b[j];
        return p;
    }
    ICELK_SUMS_INLINE_FN bool node(size_t cell, double* nu, double* nv) const
    {
        if (status[cell] != 0) return false;
        *nu = predict(coef_u + cell * (size_t)m);
        *nv = predict(coef_v + cell * (size_t)m);
        return true;
    }
};

// position -> lattice coordinates; false outside (a NaN position is outside)
ICELK_SUMS_INLINE_FN bool locate(const icelk_drift_lattice_t& L, double px, double py, double* fx, double* fy)
{
    *fx = (px - L.x0) / L.dx;
    *fy = (py - L.y0) / L.dy;
    return *fx >= 0.0 && *fx <= (double)(L.cols - 1) && *fy >= 0.0 && *fy <= (double)(L.rows - 1);
}

// the velocity at (px, py) in the field's current row: kAlive and (*su, *sv), or the reason there is none
template <typename F>
ICELK_SUMS_INLINE_FN int32_t stage(const F& f, const icelk_drift_lattice_t& L, int min_nodes, double px, double py, double* su, double* sv)
{
    if (!f.has_field()) return kNoField;
    double fx, fy;
    if (!locate(L, px, py, &fx, &fy)) return kLeft;
    int i = (int)floor(fx), j = (int)floor(fy);   // 0 <= fx <= cols - 1 < 2^31: the conversion is exact
    if (i > L.cols - 2) i = L.cols - 2;
    if (j > L.rows - 2) j = L.rows - 2;
    const double tx = fx - (double)i, ty = fy - (double)j;
    const double w[4] = {(1.0 - tx) * (1.0 - ty), tx * (1.0 - ty), (1.0 - tx) * ty, tx * ty};
    const size_t c0 = (size_t)j * (size_t)L.cols + (size_t)i;
    const size_t cell[4] = {c0, c0 + 1, c0 + (size_t)L.cols, c0 + (size_t)L.cols + 1};
    double u[4] = {0.0, 0.0, 0.0, 0.0}, v[4] = {0.0, 0.0, 0.0, 0.0};
    bool have[4];
    int measured = 0;
    ICELK_DRIFT_UNROLL
    for (int k = 0; k < 4; k++) {
        have[k] = f.node(cell[k], &u[k], &v[k]);
        measured += have[k] ? 1 : 0;
    }
    if (measured == 4) {
        *su = ((w[0] * u[0] + w[1] * u[1]) + w[2] * u[2]) + w[3] * u[3];
        *sv = ((w[0] * v[0] + w[1] * v[1]) + w[2] * v[2]) + w[3] * v[3];
        return kAlive;
    }
    double au = 0.0, av = 0.0, aw = 0.0;
    ICELK_DRIFT_UNROLL
    for (int k = 0; k < 4; k++)
        if (have[k]) {
            au = au + w[k] * u[k];
            av = av + w[k] * v[k];
            aw = aw + w[k];
        }
    if (measured < min_nodes || !(aw > 0.0)) return kTooFew;
    *su = au / aw;
    *sv = av / aw;
    return kAlive;
}

// Step s of one drifter.  Every caller takes the rows in the same order whether `live` or not (on the device the rows are
// wave-uniform work and stand outside the lanes' own control flow).  kAlive: (*px, *py) moved; otherwise they stay.
template <typename F>
ICELK_SUMS_INLINE_FN int32_t step(F& f, const icelk_drift_lattice_t& L, const icelk_drift_params_t& P, int s, bool live, double* px,
                                  double* py)
{
    const double h = P.step, half = P.step / 2.0, x = *px, y = *py;
    const int mn = P.min_nodes;
    double k1u = 0.0, k1v = 0.0, k2u = 0.0, k2v = 0.0, k3u = 0.0, k3v = 0.0, k4u = 0.0, k4v = 0.0, nx, ny;
    int32_t why = kAlive;
    f.row(2 * s);
    if (live) why = stage(f, L, mn, x, y, &k1u, &k1v);
    if (P.order == 1) {
        nx = x + h * k1u, ny = y + h * k1v;
    } else {
        f.row(2 * s + 1);
        if (live && why == kAlive) why = stage(f, L, mn, x + half * k1u, y + half * k1v, &k2u, &k2v);
        if (P.order == 2) {
            nx = x + h * k2u, ny = y + h * k2v;
        } else {
            if (live && why == kAlive) why = stage(f, L, mn, x + half * k2u, y + half * k2v, &k3u, &k3v);
            f.row(2 * s + 2);
            if (live && why == kAlive) why = stage(f, L, mn, x + h * k3u, y + h * k3v, &k4u, &k4v);
            const double sixth = h / 6.0;
            nx = x + sixth * (((k1u + 2.0 * k2u) + 2.0 * k3u) + k4u);
            ny = y + sixth * (((k1v + 2.0 * k2v) + 2.0 * k3v) + k4v);
        }
    }
    if (!live || why != kAlive) return why;
    if (!is_finite(nx) || !is_finite(ny)) return kLeft;
    *px = nx, *py = ny;
    return kAlive;
}

// what a run writes: x, y [n_out][n]; the others one per drifter
struct Out {
    double *x, *y, *last_x, *last_y, *length;
    int32_t *status, *stop_step;
};

// the whole life of drifter p < n
template <typename F>
ICELK_SUMS_INLINE_FN void run(F& f, const icelk_drift_lattice_t& L, const icelk_drift_params_t& P, const double* seed_x,
                              const double* seed_y, const int32_t* release, int p, int n, const Out& O)
{
    const double nan = __builtin_nan("");
    const double sx = seed_x[p], sy = seed_y[p];
    const int rel = release[p];
    const bool born = is_finite(sx) && is_finite(sy) && rel >= 0 && rel < P.nsteps;
    int32_t status = born ? kAlive : kNeverReleased, stop = born ? P.nsteps : -1;
    double x = nan, y = nan, len = 0.0;
    bool live = false;
    int next_out = 0, o = 0;
    for (int s = 0; s <= P.nsteps; s++) {
        if (born && s == rel) x = sx, y = sy, live = true;
        if (s == next_out) {
            const size_t at = (size_t)o * (size_t)n + (size_t)p;
            O.x[at] = live ? x : nan;
            O.y[at] = live ? y : nan;
            next_out += P.every, o++;
        }
        if (s == P.nsteps) break;
        const double ox = x, oy = y;
        const int32_t why = step(f, L, P, s, live, &x, &y);
        if (!live) continue;
        if (why != kAlive) {
            status = why, stop = s, live = false;
        } else {
            len = len + hypot_np(x - ox, y - oy);
        }
    }
    O.last_x[p] = x, O.last_y[p] = y, O.length[p] = len;
    O.status[p] = status, O.stop_step[p] = stop;
}

// the node a recorded sample visits, or -1 (not finite, or its nearest node is off the lattice)
ICELK_SUMS_INLINE_FN long long visited(const icelk_drift_lattice_t& L, double px, double py)
{
    if (!is_finite(px) || !is_finite(py)) return -1;
    const double gx = floor((px - L.x0) / L.dx + 0.5), gy = floor((py - L.y0) / L.dy + 0.5);
    if (!(gx >= 0.0 && gx <= (double)(L.cols - 1) && gy >= 0.0 && gy <= (double)(L.rows - 1))) return -1;
    return (long long)gy * L.cols + (long long)gx;
}

// The whole statement on the host, drifter by drifter.  check() has passed; visits NULL or [rows][cols].
template <typename F>
inline void run_host(F f, const icelk_drift_lattice_t& L, const icelk_drift_params_t& P, const double* seed_x, const double* seed_y,
                     const int32_t* release, int n, const Out& O, int32_t* visits)
{
    for (int p = 0; p < n; p++) run(f, L, P, seed_x, seed_y, release, p, n, O);
    if (!visits) return;
    const size_t cells = (size_t)L.rows * (size_t)L.cols, samples = (size_t)n_out(P) * (size_t)n;
    for (size_t c = 0; c < cells; c++) visits[c] = 0;
    for (size_t k = 0; k < samples; k++) {
        const long long c = visited(L, O.x[k], O.y[k]);
        if (c >= 0) visits[c]++;
    }
}

}  // namespace drift
}  // namespace icelk
