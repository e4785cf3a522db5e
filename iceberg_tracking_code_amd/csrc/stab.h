// stab.h -- camera shake fitted to land anchors: the rules of the stabilising stage between tracking and
// saving, stated once for the host and the device alike.  The host statement (icelk_stab_tracks_host, abi_stab.hip), the
// kernels (k_stab.hip), tests/stab_main.cpp and tests/stab_restatement.py (numpy, written independently) all compute what
// is stated here bit for bit.  The build's -ffp-contract=off keeps every operation a rounding of its own, in the order
// written.
//
//   input       tracks (n, V, 2) float32 with 2 <= V <= 17, flags n bytes
//   anchors A   the rows with flags != 0 whose 2 V coordinates are all finite, in row order; n_a of them.  x, y are the
//               doubles of vertex 0, X, Y the doubles of vertex k
//   per vertex k = 1 .. V - 1, independently (fit_vertex):
//     n_a < min_anchors: TOO_FEW, the identity, 0 inliers, 0 rounds
//     start     m = (a, b, tx, ty) = (1, 0, np.median(X - x), np.median(Y - y)), g = max(threshold, start_gate)
//     inliers   ex = X - ((a x - b y) + tx), ey = Y - ((b x + a y) + ty), r2 = ex ex + ey ey, w = r2 <= g g
//     rounds    w = inliers(m, g); for r = 1 .. rounds: count(w) < min_anchors: LOST, stop; m = fit(w);
//               g' = max(threshold, g / 2); w' = inliers(m, g'); converged = (w' == w and g' == g); w, g = w', g'; stop
//               when converged
//     fit(w)    every sum is np.sum(wf * (...)) over the anchors in row order, wf = 0.0 | 1.0 (np_sum of np_sums.h);
//               n_in = sum wf; translation: (1, 0, sum wf (X - x) / n_in, sum wf (Y - y) / n_in).  Similarity: mx, my, mX,
//               mY = sum wf x / n_in ..., xc = x - mx ..., D = sum wf (xc xc + yc yc); not D >= n_in min_spread min_spread:
//               the translation fit and DEGENERATE (of the last fit only); else a = sum wf (xc Xc + yc Yc) / D,
//               b = sum wf (xc Yc - yc Xc) / D, tx = mX - (a mx - b my), ty = mY - (b mx + a my)
//     after     count(w) < min_anchors: LOST; all `rounds` rounds done without converging: NOT_CONVERGED (the model is still
//               applied); LOST or TOO_FEW: the model is the identity and rms NaN.  inliers = count(w) (0 for TOO_FEW),
//               rms = sqrt(sum wf r2 / n_in) under the final model, rounds_used = the fits made
//   apply       to every row, anchor or not: det = a a + b b, Xa = X - tx, Ya = Y - ty, x' = (a Xa + b Ya) / det,
//               y' = (a Ya - b Xa) / det, rounded to float32.  Vertex 0, and every vertex under TOO_FEW or LOST, is copied
//               bit for bit; a non-finite row passes through the arithmetic as IEEE has it.  IEEE leaves a NaN's sign and
//               payload open (a subtraction done as an addition of the negated operand flips the sign), so a NaN result
//               is stored as THE quiet NaN 0x7fc00000: the host and the device then agree on those bits too
//   mask flags  ix = (int)floor(x0 + 0.5), iy likewise, in double; flag = mask[iy, ix] != 0, 0 outside the mask (a NaN is
//               outside)
// The workgroup that fits a vertex on the device and the host's plain loop run the SAME fit_vertex: what differs is the
// engine underneath (how a sum, an inlier pass and a median are carried out), and the engines' sums are the same additions
// in the same tree -- np_pairwise_walk below is np_pairwise_sum's stack machine with the leaf left to the caller.
#pragma once
#include <stdint.h>

#include "../../include/icelk.h"
#include "grid_stats.h"

namespace icelk {
namespace stab {

constexpr int kTooFew = ICELK_STAB_TOO_FEW, kLost = ICELK_STAB_LOST, kDegenerate = ICELK_STAB_DEGENERATE,
              kNotConverged = ICELK_STAB_NOT_CONVERGED;
constexpr int kMaxVert = 17, kMaxRounds = 16;

// the policy defaults (not measurements: DESIGN.md 7.13); the threshold is the reference's forward-backward bound (s1:333)
ICELK_SUMS_INLINE_FN icelk_stab_params_t default_params()
{
    icelk_stab_params_t p{};
    p.model = 0, p.threshold = 1.0, p.start_gate = 8.0, p.rounds = 8, p.min_anchors = 10, p.min_spread = 64.0;
    return p;
}

ICELK_SUMS_INLINE_FN bool finite64(double v) { return v - v == 0.0; }
ICELK_SUMS_INLINE_FN bool finite32(float v) { return v - v == 0.0f; }

ICELK_SUMS_INLINE_FN bool params_ok(const icelk_stab_params_t& p)
{
    return (p.model == 0 || p.model == 1) && finite64(p.threshold) && p.threshold > 0.0 && finite64(p.start_gate) && p.rounds >= 1 &&
           p.rounds <= kMaxRounds && p.min_anchors >= 2 && finite64(p.min_spread) && p.min_spread >= 0.0;
}

struct Model {
    double a, b, tx, ty;
};

struct VertexResult {
    Model m;
    double rms;
    int inliers, status, rounds_used, reserved;
};

// ---- anchors: row idx[t] of the table is anchor t
struct Anchors {
    const float* tracks;   // (n, V, 2)
    const int* idx;        // n_a rows, ascending
    int V, k;
    ICELK_SUMS_INLINE_FN double x(int t) const { return (double)tracks[((size_t)idx[t] * V) * 2]; }
    ICELK_SUMS_INLINE_FN double y(int t) const { return (double)tracks[((size_t)idx[t] * V) * 2 + 1]; }
    ICELK_SUMS_INLINE_FN double X(int t) const { return (double)tracks[((size_t)idx[t] * V + k) * 2]; }
    ICELK_SUMS_INLINE_FN double Y(int t) const { return (double)tracks[((size_t)idx[t] * V + k) * 2 + 1]; }
};

ICELK_SUMS_INLINE_FN bool row_finite(const float* row, int V)
{
    bool ok = true;
    for (int i = 0; i < 2 * V; i++) ok = ok && finite32(row[i]);
    return ok;
}

ICELK_SUMS_INLINE_FN uint8_t mask_flag(float x0, float y0, const uint8_t* mask, int w, int h, size_t stride)
{
    const double fx = floor((double)x0 + 0.5), fy = floor((double)y0 + 0.5);
    if (!(fx >= 0.0 && fx < (double)w && fy >= 0.0 && fy < (double)h)) return 0;
    return mask[(size_t)(int)fy * stride + (size_t)(int)fx] != 0 ? 1 : 0;
}

ICELK_SUMS_INLINE_FN double residual2(const Model& m, double x, double y, double X, double Y)
{
    const double ex = X - ((m.a * x - m.b * y) + m.tx);
    const double ey = Y - ((m.b * x + m.a * y) + m.ty);
    return ex * ex + ey * ey;
}

// the start medians' terms: X - x (comp 0), Y - y (comp 1)
struct ShiftAt {
    Anchors A;
    int comp;
    ICELK_SUMS_INLINE_FN double operator()(int t) const { return comp ? A.Y(t) - A.y(t) : A.X(t) - A.x(t); }
};

// ---- the sums' terms
enum TermId { T_N, T_x, T_y, T_X, T_Y, T_DX, T_DY, T_D, T_A, T_B, T_R2, T_COUNT };

struct Means {
    double mx, my, mX, mY;
};

struct TermCtx {
    Anchors A;
    const uint8_t* w;   // n_a bytes, 0 | 1
    Means c;            // read by T_D, T_A, T_B
    Model m;            // read by T_R2
};

template <int W>
struct Term {
    const TermCtx& C;
    ICELK_SUMS_INLINE_FN double operator()(int t) const
    {
        const Anchors& A = C.A;
        const double wf = C.w[t] ? 1.0 : 0.0;
        if constexpr (W == T_N) return wf;
        if constexpr (W == T_x) return wf * A.x(t);
        if constexpr (W == T_y) return wf * A.y(t);
        if constexpr (W == T_X) return wf * A.X(t);
        if constexpr (W == T_Y) return wf * A.Y(t);
        if constexpr (W == T_DX) return wf * (A.X(t) - A.x(t));
        if constexpr (W == T_DY) return wf * (A.Y(t) - A.y(t));
        if constexpr (W == T_R2) return wf * residual2(C.m, A.x(t), A.y(t), A.X(t), A.Y(t));
        if constexpr (W == T_D || W == T_A || W == T_B) {
            const double xc = A.x(t) - C.c.mx, yc = A.y(t) - C.c.my;
            if constexpr (W == T_D) return wf * (xc * xc + yc * yc);
            const double Xc = A.X(t) - C.c.mX, Yc = A.Y(t) - C.c.mY;
            if constexpr (W == T_A) return wf * (xc * Xc + yc * Yc);
            if constexpr (W == T_B) return wf * (xc * Yc - yc * Xc);
        }
        return 0.0;
    }
};

// np_leaf_sum (np_sums.h) cut along its own accumulators, for a leaf of n >= 8 terms: accumulator j is the chain
// at(start + j) + at(start + 8 + j) + ... over the whole blocks of 8 (np_leaf_lane); np_leaf_join adds the eight as np_leaf_sum
// does, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), and then the n % 8 tail terms one after the other.  The same
// additions in the same order, with the eight chains free to run side by side (tests/stab_main.cpp: equal to np_leaf_sum bit
// for bit for every n).
template <typename At>
ICELK_SUMS_INLINE_FN double np_leaf_lane(const At& at, int start, int n, int j)
{
    double r = at(start + j);
    for (int t = 8; t < n - (n % 8); t += 8) r += at(start + t + j);
    return r;
}

template <typename At>
ICELK_SUMS_INLINE_FN double np_leaf_join(const double* r, const At& at, int start, int n)
{
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int t = n - (n % 8); t < n; t++) res += at(start + t);
    return res;
}

// what to do with a term once `which` has named it
struct LeafSum {
    int start, len;
    template <typename At>
    ICELK_SUMS_INLINE_FN double operator()(const At& at) const { return np_leaf_sum(at, start, len); }
};
struct LaneSum {
    int start, len, j;
    template <typename At>
    ICELK_SUMS_INLINE_FN double operator()(const At& at) const { return np_leaf_lane(at, start, len, j); }
};
struct JoinSum {
    const double* r;
    int start, len;
    template <typename At>
    ICELK_SUMS_INLINE_FN double operator()(const At& at) const { return np_leaf_join(r, at, start, len); }
};
struct WholeSum {
    int n;
    template <typename At>
    ICELK_SUMS_INLINE_FN double operator()(const At& at) const { return np_sum(at, n); }
};

template <typename F>
ICELK_SUMS_FN double with_term(int which, const TermCtx& C, const F& f)
{
    switch (which) {
    case T_N: return f(Term<T_N>{C});
    case T_x: return f(Term<T_x>{C});
    case T_y: return f(Term<T_y>{C});
    case T_X: return f(Term<T_X>{C});
    case T_Y: return f(Term<T_Y>{C});
    case T_DX: return f(Term<T_DX>{C});
    case T_DY: return f(Term<T_DY>{C});
    case T_D: return f(Term<T_D>{C});
    case T_A: return f(Term<T_A>{C});
    case T_B: return f(Term<T_B>{C});
    default: return f(Term<T_R2>{C});
    }
}

// np_leaf_sum of term `which` over anchors [start, start + len)
ICELK_SUMS_FN double leaf_of(int which, const TermCtx& C, int start, int len) { return with_term(which, C, LeafSum{start, len}); }

// np_sum of term `which` over all n_a anchors
ICELK_SUMS_FN double sum_of(int which, const TermCtx& C, int n_a) { return with_term(which, C, WholeSum{n_a}); }

// np_pairwise_sum's stack machine (np_sums.h) with the leaf left to the caller: leaf(start, len) is called once per leaf
// (len <= 128), in the order of the leaves' starts, and its values are added exactly as np_pairwise_sum adds its leaf sums.
// With leaf = np_leaf_sum this IS np_pairwise_sum; a leaf that records (start, len) lists the leaves, and one that hands out
// values computed elsewhere replays the additions.  A run of more than 128 terms splits into halves of at least 64, so a
// chunk of at most 8192 terms has at most 128 leaves (kMaxLeaves).
constexpr int kMaxLeaves = 128;

template <typename Leaf>
ICELK_SUMS_FN double np_pairwise_walk(Leaf& leaf, int n, int first)
{
    struct Frame { int start, n, stage; };
    Frame st[40];
    double vals[40];
    int fp = 0, sp = 0;
    st[fp++] = Frame{first, n, 0};
    while (fp) {
        Frame& f = st[fp - 1];
        if (f.n <= 128) {
            vals[sp++] = leaf(f.start, f.n);
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

struct LeafSpan {
    int start, len;
};

// a leaf that lists: tab[0 .. count) are the leaves of the run, in order; count may pass kMaxLeaves, the table does not
struct ListLeaves {
    LeafSpan* tab;
    int count;
    ICELK_SUMS_INLINE_FN double operator()(int start, int len)
    {
        if (count < kMaxLeaves) tab[count] = LeafSpan{start, len};
        count++;
        return 0.0;
    }
};

// a leaf that hands out the values v[0], v[1], ... computed for the listed leaves
struct ReplayLeaves {
    const double* v;
    int next;
    ICELK_SUMS_INLINE_FN double operator()(int, int) { return v[next++]; }
};

// a leaf that computes: np_pairwise_walk with it is np_pairwise_sum of the term
struct ComputeLeaves {
    int which;
    const TermCtx& C;
    ICELK_SUMS_INLINE_FN double operator()(int start, int len) { return leaf_of(which, C, start, len); }
};

// ---- one vertex.  Engine:
//   double median(int comp)                         np.median of X - x (0) / Y - y (1) over the anchors
//   int inliers(const Model&, double g, bool* same) w := (r2 <= g g); returns count(w); *same: w is what it was before
//   void sums(unsigned terms, const Means&, const Model&, double* out)   out[T] = np.sum of term T for every bit T of `terms`
// On the device every thread of the workgroup runs this with the same values; the engine's calls are the collective ones.
template <typename Engine>
ICELK_SUMS_FN bool fit(Engine& E, const icelk_stab_params_t& P, Model* m)
{
    double s[T_COUNT];
    const Means none{0.0, 0.0, 0.0, 0.0};
    const unsigned shift = (1u << T_N) | (1u << T_DX) | (1u << T_DY);
    if (P.model == 0) {
        E.sums(shift, none, *m, s);
        *m = Model{1.0, 0.0, s[T_DX] / s[T_N], s[T_DY] / s[T_N]};
        return false;
    }
    E.sums(shift | (1u << T_x) | (1u << T_y) | (1u << T_X) | (1u << T_Y), none, *m, s);
    const double n_in = s[T_N];
    const Means c{s[T_x] / n_in, s[T_y] / n_in, s[T_X] / n_in, s[T_Y] / n_in};
    const double dx = s[T_DX] / n_in, dy = s[T_DY] / n_in;
    E.sums((1u << T_D) | (1u << T_A) | (1u << T_B), c, *m, s);
    const double D = s[T_D];
    if (!(D >= n_in * P.min_spread * P.min_spread)) {
        *m = Model{1.0, 0.0, dx, dy};
        return true;
    }
    const double a = s[T_A] / D, b = s[T_B] / D;
    *m = Model{a, b, c.mX - (a * c.mx - b * c.my), c.mY - (b * c.mx + a * c.my)};
    return false;
}

template <typename Engine>
ICELK_SUMS_FN VertexResult fit_vertex(Engine& E, int n_a, const icelk_stab_params_t& P)
{
    const Model identity{1.0, 0.0, 0.0, 0.0};
    const double nan = __builtin_nan("");
    VertexResult R{identity, nan, 0, 0, 0, 0};
    if (n_a < P.min_anchors) {
        R.status = kTooFew;
        return R;
    }
    Model m{1.0, 0.0, E.median(0), E.median(1)};
    double g = P.threshold > P.start_gate ? P.threshold : P.start_gate;
    bool same = false, converged = false, lost = false, degenerate = false;
    int count = E.inliers(m, g, &same), used = 0;
    for (int r = 1; r <= P.rounds; r++) {
        if (count < P.min_anchors) {
            lost = true;
            break;
        }
        degenerate = fit(E, P, &m);
        used = r;
        const double half = g / 2.0;
        const double g2 = P.threshold > half ? P.threshold : half;
        count = E.inliers(m, g2, &same);
        converged = same && g2 == g;
        g = g2;
        if (converged) break;
    }
    if (count < P.min_anchors) lost = true;
    R.inliers = count;
    R.rounds_used = used;
    R.status = (lost ? kLost : 0) | (degenerate ? kDegenerate : 0) | (!converged && used == P.rounds ? kNotConverged : 0);
    if (lost) return R;
    double s[T_COUNT];
    E.sums((1u << T_N) | (1u << T_R2), Means{0.0, 0.0, 0.0, 0.0}, m, s);
    R.m = m;
    R.rms = sqrt(s[T_R2] / s[T_N]);
    return R;
}

// ---- apply
ICELK_SUMS_INLINE_FN bool is_identity(int status) { return (status & (kTooFew | kLost)) != 0; }

ICELK_SUMS_INLINE_FN void apply_point(const Model& m, float X, float Y, float* ox, float* oy)
{
    const double det = m.a * m.a + m.b * m.b;
    const double Xa = (double)X - m.tx, Ya = (double)Y - m.ty;
    const double xs = (m.a * Xa + m.b * Ya) / det;
    const double ys = (m.a * Ya - m.b * Xa) / det;
    *ox = xs != xs ? __builtin_nanf("") : (float)xs;
    *oy = ys != ys ? __builtin_nanf("") : (float)ys;
}

// ---- the host statement: plain loops.  idx: n ints and w: n bytes of working space; out_tracks may be `tracks` itself
struct HostEngine {
    TermCtx C;
    uint8_t* w;
    int n_a;
    double median(int comp) const { return np_median(ShiftAt{C.A, comp}, n_a); }
    int inliers(const Model& m, double g, bool* same)
    {
        int count = 0;
        bool eq = true;
        const double gg = g * g;
        for (int t = 0; t < n_a; t++) {
            const uint8_t v = residual2(m, C.A.x(t), C.A.y(t), C.A.X(t), C.A.Y(t)) <= gg ? 1 : 0;
            eq = eq && v == w[t];
            w[t] = v;
            count += v;
        }
        *same = eq;
        return count;
    }
    void sums(unsigned terms, const Means& c, const Model& m, double* out)
    {
        C.c = c, C.m = m;
        for (int T = 0; T < T_COUNT; T++)
            if (terms >> T & 1) out[T] = sum_of(T, C, n_a);
    }
};

inline int anchors_host(const float* tracks, const uint8_t* flags, int n, int V, int* idx)
{
    int n_a = 0;
    for (int i = 0; i < n; i++)
        if (flags[i] != 0 && row_finite(tracks + (size_t)i * V * 2, V)) idx[n_a++] = i;
    return n_a;
}

inline void flags_host(const float* tracks, int n, int V, const uint8_t* mask, int w, int h, size_t stride, uint8_t* flags)
{
    for (int i = 0; i < n; i++) flags[i] = mask_flag(tracks[(size_t)i * V * 2], tracks[(size_t)i * V * 2 + 1], mask, w, h, stride);
}

// results: V - 1 entries, vertex k at k - 1.  Returns n_a
inline int run_host(const float* tracks, const uint8_t* flags, int n, int V, const icelk_stab_params_t& P, int* idx, uint8_t* w,
                    float* out_tracks, VertexResult* results)
{
    const int n_a = anchors_host(tracks, flags, n, V, idx);
    for (int k = 1; k < V; k++) {
        for (int t = 0; t < n_a; t++) w[t] = 0;
        HostEngine E{TermCtx{Anchors{tracks, idx, V, k}, w, Means{0.0, 0.0, 0.0, 0.0}, Model{1.0, 0.0, 0.0, 0.0}}, w, n_a};
        results[k - 1] = fit_vertex(E, n_a, P);
    }
    for (int i = 0; i < n; i++) {
        const float* src = tracks + (size_t)i * V * 2;
        float* dst = out_tracks + (size_t)i * V * 2;
        dst[0] = src[0], dst[1] = src[1];   // (bit for bit: a float copy keeps a NaN's payload on every target we build for)
        for (int k = 1; k < V; k++) {
            const VertexResult& R = results[k - 1];
            if (is_identity(R.status))
                dst[2 * k] = src[2 * k], dst[2 * k + 1] = src[2 * k + 1];
            else
                apply_point(R.m, src[2 * k], src[2 * k + 1], dst + 2 * k, dst + 2 * k + 1);
        }
    }
    return n_a;
}

}  // namespace stab
}  // namespace icelk
