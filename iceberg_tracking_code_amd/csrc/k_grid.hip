// k_grid.hip -- gridding of the projected velocities (second half).
//
// Replaces the per-cell loop of s3_utm_to_gridded_utm.py:391-421: for every square cell of the fjord grid
// (imports/tracking_misc.py:14-56) the reference runs matplotlib's Path(poly).contains_points over ALL velocities
// (cells x points tests), then mean_u = np.sum(u_sel) / n, mean_v likewise, speed = np.hypot(mean_u, mean_v).
//
// Here: one pass over the points finds the cells that contain each point -- only the 3 x 3 cells around its floor
// index can, and each is tested with matplotlib's own crossing rule on the cell's four vertices, formed as the
// reference forms them (left + i * spacing, top - j * spacing, + / - spacing), so points exactly on edges and corners
// land where contains_points puts them (in one, two or no cell).  The (cell, point index) pairs are sorted (rocPRIM
// radix sort, k_sort.hip), which restores the point order inside every cell, and one thread per cell adds its
// velocities in numpy's pairwise order (blocks of 128, 8 accumulators, halves aligned to 8; beyond 8192 terms in the
// chunks of numpy's iterator buffer, np_sums.h) -- float64, bit for bit what np.sum gives -- and takes the hypot (glibc's algorithm, see k_utm.hip).
// Asked for, the sorted runs also give every cell's np.std(ddof=1), np.median and median absolute deviation
// (k_grid_segments, k_grid_std, k_grid_select below; the rules are grid_stats.h's).
// Boxes that form no lattice -- along a transect, around a mooring (imports/tracking_misc.py:76-185) -- have assign kernels
// of their own (k_boxes_assign, k_boxes_day_assign: every point against every box) and share everything behind them.
#include "icelk_internal.h"
#include "grid_keys.h"
#include "grid_stats.h"
#include "grid_select_wg.h"

namespace icelk {

namespace {

__device__ __forceinline__ bool contains_poly(const double* __restrict__ poly, int n, double tx, double ty)
{
    if (n < 3) return false;
    bool inside = false;
    double x0 = poly[0], y0 = poly[1];
    bool f0 = y0 >= ty;
    for (int k = 1; k <= n; k++) {
        const double x1 = k < n ? poly[2 * k] : poly[0];
        const double y1 = k < n ? poly[2 * k + 1] : poly[1];
        const bool f1 = y1 >= ty;
        if (f0 != f1 && (((y1 - ty) * (x0 - x1) >= (x1 - tx) * (y0 - y1)) == f1)) inside = !inside;
        f0 = f1;
        x0 = x1;
        y0 = y1;
    }
    return inside;
}

__global__ __launch_bounds__(256) void k_points_in_polygon(const double* __restrict__ poly, int n,
                                                           const double* __restrict__ pts, int m,
                                                           uint8_t* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    out[i] = contains_poly(poly, n, pts[2 * i], pts[2 * i + 1]) ? 1 : 0;
}

// square cell (i, j): [(x, y), (x + s, y), (x + s, y - s), (x, y - s)] with x = left + i * s, y = top - j * s
// (tracking_misc.py:14-21, 43)
__device__ __forceinline__ bool contains_cell(double left, double top, double s, int i, int j, double tx, double ty)
{
    const double x = left + i * s, y = top - j * s;
    const double p[8] = {x, y, x + s, y, x + s, y - s, x, y - s};
    return contains_poly(p, 4, tx, ty);
}

struct GridGeom {
    double left, top, spacing;
    int cols, rows;
};

// bit k = 3 * (dj + 1) + (di + 1) set: the point lies in cell (i0 + di, j0 + dj)
__device__ __forceinline__ unsigned hit_mask(const GridGeom& g, const uint8_t* __restrict__ cell_on, double tx,
                                             double ty, int* i0, int* j0)
{
    const double fi = floor((tx - g.left) / g.spacing), fj = floor((g.top - ty) / g.spacing);
    // far outside (or not finite): no cell
    if (!(fi >= -2.0 && fi <= (double)g.cols + 1.0 && fj >= -2.0 && fj <= (double)g.rows + 1.0)) {
        *i0 = *j0 = 0;
        return 0u;
    }
    *i0 = (int)fi;
    *j0 = (int)fj;
    unsigned m = 0;
    for (int dj = -1; dj <= 1; dj++)
        for (int di = -1; di <= 1; di++) {
            const int i = *i0 + di, j = *j0 + dj;
            if (i < 0 || j < 0 || i >= g.cols || j >= g.rows || !cell_on[i * g.rows + j]) continue;
            if (contains_cell(g.left, g.top, g.spacing, i, j, tx, ty)) m |= 1u << (3 * (dj + 1) + (di + 1));
        }
    return m;
}

// writes the keys ((seg_base + cell) << 32) | p of the cells in hit mask m
__device__ __forceinline__ void append_keys(unsigned m, int i0, int j0, unsigned seg_base, int rows, int p,
                                            unsigned long long* __restrict__ keys, int* __restrict__ key_count,
                                            int key_cap)
{
    int at = key_slots(__popc(m), key_count);
    for (int k = 0; k < 9; k++)
        if (m & (1u << k)) {
            const int i = i0 + (k % 3) - 1, j = j0 + (k / 3) - 1;
            if (at < key_cap)
                keys[at] = ((unsigned long long)(seg_base + (unsigned)(i * rows + j)) << 32) | (unsigned)p;
            at++;
        }
}

__global__ __launch_bounds__(256) void k_grid_assign(const double* __restrict__ x, const double* __restrict__ y, int n,
                                                     GridGeom g, const uint8_t* __restrict__ cell_on,
                                                     unsigned long long* __restrict__ keys, int* __restrict__ key_count,
                                                     int key_cap)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    int i0 = 0, j0 = 0;
    const unsigned m = p < n ? hit_mask(g, cell_on, x[p], y[p], &i0, &j0) : 0u;
    append_keys(m, i0, j0, 0u, g.rows, p, keys, key_count, key_cap);
}

// ---- a whole day of time windows in one pass (icelk_grid_bin_windows): DayTables and day_window are grid_keys.h's ----
// selected count and time range per (window, camera) slot (-1: the point is in none): lanes of one slot are combined
// first -- a wave's points are consecutive, so nearly always one slot per wave and one set of atomics.  Called by every
// lane of the wave.
__device__ __forceinline__ void day_slot_reduce(int slot, double tp, int* __restrict__ sel_count,
                                                unsigned long long* __restrict__ t_min,
                                                unsigned long long* __restrict__ t_max)
{
    const unsigned long long tk = order_key(tp);
    unsigned long long pending = __ballot(slot >= 0);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int s0 = __shfl(slot, leader);
        const bool mine = slot == s0;
        int c = mine ? 1 : 0;
        unsigned long long mn = mine ? tk : ~0ull, mx = mine ? tk : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            c += __shfl_xor(c, o);
            const unsigned long long a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        if ((threadIdx.x & 63) == leader) {
            atomicAdd(&sel_count[s0], c);
            atomicMin(&t_min[s0], mn);
            atomicMax(&t_max[s0], mx);
        }
        pending &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(256) void k_grid_day_assign(const double* __restrict__ x, const double* __restrict__ y,
                                                         const double* __restrict__ t, int n, DayTables D, GridGeom g,
                                                         const uint8_t* __restrict__ cell_on, int ncells,
                                                         unsigned long long* __restrict__ keys,
                                                         int* __restrict__ key_count, int key_cap,
                                                         int* __restrict__ sel_count,
                                                         unsigned long long* __restrict__ t_min,
                                                         unsigned long long* __restrict__ t_max)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    int cam = 0;
    double tp = 0.0;
    const int w = day_window(D, t, p, n, &cam, &tp);
    day_slot_reduce(w >= 0 ? w * D.ncam + cam : -1, tp, sel_count, t_min, t_max);
    int i0 = 0, j0 = 0;
    const unsigned m = w >= 0 ? hit_mask(g, cell_on, x[p], y[p], &i0, &j0) : 0u;
    append_keys(m, i0, j0, (unsigned)w * (unsigned)ncells, g.rows, p, keys, key_count, key_cap);
}

// ---- boxes that are no lattice: transects and moorings (icelk_boxes_bin, icelk_boxes_bin_windows) ----------------------
// B polygons of three or more vertices each, box b's vertices at xy[2 * off[b]] .. xy[2 * off[b + 1]) as (x, y) pairs.
// The boxes of a transect meet along edges that are no grid lines, so no index arithmetic finds a point's boxes: every
// thread tests its point against every box, with contains_poly on the vertices as they were given, and a point lies in
// none, one or several of them.  The list is staged once per workgroup in LDS (all lanes read the same vertex at the same
// time: a broadcast), with every box's smallest and largest y beside it.
// A box is skipped without the crossing test only where ty lies outside [min y, max y]: then y_k >= ty has the same
// answer at every vertex, no edge has f0 != f1 and nothing toggles -- also for a NaN ty, which compares false everywhere.
// The same shortcut on x is not taken: the side test is a rounded expression, and a point beyond the box's x range on
// an edge's level is decided by that rounding, not by the range.
struct BoxList {
    const double* xy;
    const int* off;
    int nboxes, nvert;
};

// velocities turned into the boxes' frame: u' = u c + v s along, v' = v c - u s across; every operation rounded once
struct BoxRot {
    const double* u;
    const double* v;
    double* ur;
    double* vr;
    double c, s;
    int on;
};

struct BoxLds {
    double* xy;      // 2 * nvert
    double* ylo;     // nboxes
    double* yhi;     // nboxes
    int* off;        // nboxes + 1
};

__device__ __forceinline__ BoxLds stage_boxes(const BoxList& L, double* lds)
{
    BoxLds S{lds, lds + 2 * L.nvert, lds + 2 * L.nvert + L.nboxes, (int*)(lds + 2 * L.nvert + 2 * L.nboxes)};
    for (int k = threadIdx.x; k < 2 * L.nvert; k += 256) S.xy[k] = L.xy[k];
    for (int k = threadIdx.x; k <= L.nboxes; k += 256) S.off[k] = L.off[k];
    __syncthreads();
    for (int b = threadIdx.x; b < L.nboxes; b += 256) {
        double lo = S.xy[2 * S.off[b] + 1], hi = lo;
        for (int k = S.off[b] + 1; k < S.off[b + 1]; k++) {
            const double yk = S.xy[2 * k + 1];
            lo = yk < lo ? yk : lo;
            hi = yk > hi ? yk : hi;
        }
        S.ylo[b] = lo;
        S.yhi[b] = hi;
    }
    __syncthreads();
    return S;
}

__device__ __forceinline__ bool in_box(const BoxLds& S, int b, double tx, double ty)
{
    if (!(ty >= S.ylo[b] && ty <= S.yhi[b])) return false;
    return contains_poly(S.xy + 2 * S.off[b], S.off[b + 1] - S.off[b], tx, ty);
}

// The keys ((seg_base + b) << 32) | p of every box b that holds (tx, ty); `live` false: none.  A thread may have any
// number of hits, so they are counted first (the first and the last hit remembered), the counts scanned (key_slots),
// and the boxes from the first hit to the last walked again to write -- for a point in one box that is one test.
__device__ __forceinline__ void append_box_keys(const BoxLds& S, int nboxes, bool live, double tx, double ty,
                                                unsigned seg_base, int p, unsigned long long* __restrict__ keys,
                                                int* __restrict__ key_count, int key_cap)
{
    int cnt = 0, first = 0, last = -1;
    if (live)
        for (int b = 0; b < nboxes; b++)
            if (in_box(S, b, tx, ty)) {
                if (!cnt) first = b;
                last = b;
                cnt++;
            }
    int at = key_slots(cnt, key_count);
    for (int b = first; b <= last; b++)
        if (b == first || b == last || in_box(S, b, tx, ty)) {
            if (at >= 0 && at < key_cap) keys[at] = ((unsigned long long)(seg_base + (unsigned)b) << 32) | (unsigned)p;
            at++;
        }
}

__device__ __forceinline__ void rotate_velocity(const BoxRot& R, int p)
{
    const double u = R.u[p], v = R.v[p];
    R.ur[p] = u * R.c + v * R.s;
    R.vr[p] = v * R.c - u * R.s;
}

__global__ __launch_bounds__(256) void k_boxes_assign(const double* __restrict__ x, const double* __restrict__ y, int n,
                                                      BoxList L, BoxRot R, unsigned long long* __restrict__ keys,
                                                      int* __restrict__ key_count, int key_cap)
{
    extern __shared__ double box_lds[];
    const BoxLds S = stage_boxes(L, box_lds);
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool live = p < n;
    if (live && R.on) rotate_velocity(R, p);
    append_box_keys(S, L.nboxes, live, live ? x[p] : 0.0, live ? y[p] : 0.0, 0u, p, keys, key_count, key_cap);
}

__global__ __launch_bounds__(256) void k_boxes_day_assign(const double* __restrict__ x, const double* __restrict__ y,
                                                          const double* __restrict__ t, int n, DayTables D, BoxList L,
                                                          BoxRot R, unsigned long long* __restrict__ keys,
                                                          int* __restrict__ key_count, int key_cap,
                                                          int* __restrict__ sel_count,
                                                          unsigned long long* __restrict__ t_min,
                                                          unsigned long long* __restrict__ t_max)
{
    extern __shared__ double box_lds[];
    const BoxLds S = stage_boxes(L, box_lds);
    const int p = blockIdx.x * 256 + threadIdx.x;
    int cam = 0;
    double tp = 0.0;
    const int w = day_window(D, t, p, n, &cam, &tp);
    day_slot_reduce(w >= 0 ? w * D.ncam + cam : -1, tp, sel_count, t_min, t_max);
    if (p < n && R.on) rotate_velocity(R, p);
    const bool live = w >= 0;
    append_box_keys(S, L.nboxes, live, live ? x[p] : 0.0, live ? y[p] : 0.0, (unsigned)w * (unsigned)L.nboxes, p, keys,
                    key_count, key_cap);
}

// element t of the velocities keyed by keys[start + t] (np_sums.h: numpy's pairwise order)
struct KeyedAt {
    const unsigned long long* __restrict__ keys;
    const double* __restrict__ a;
    int start;
    __device__ __forceinline__ double operator()(int t) const { return a[(unsigned)keys[start + t]]; }
};

// np.sum over the velocities of keys[start, start + n): pairwise, in the chunks of numpy's buffer beyond 8192 terms
__device__ __forceinline__ double keyed_sum(const unsigned long long* __restrict__ keys,
                                            const double* __restrict__ a, int start, int n)
{
    return np_sum(KeyedAt{keys, a, start}, n);
}

__device__ __forceinline__ int lower_bound(const unsigned long long* __restrict__ keys, int n, unsigned long long v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void k_grid_reduce(const unsigned long long* __restrict__ keys,
                                                    const int* __restrict__ key_count, const double* __restrict__ u,
                                                    const double* __restrict__ v, int ncells, int* __restrict__ count,
                                                    double* __restrict__ mean_u, double* __restrict__ mean_v,
                                                    double* __restrict__ speed)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= ncells) return;
    const int total = *key_count;
    const int b = lower_bound(keys, total, (unsigned long long)(unsigned)c << 32);
    const int e = lower_bound(keys, total, (unsigned long long)(unsigned)(c + 1) << 32);
    const int n = e - b;
    count[c] = n;
    double mu = 0.0, mv = 0.0, sp = 0.0;
    if (n > 0) {
        mu = keyed_sum(keys, u, b, n) / (double)n;
        mv = keyed_sum(keys, v, b, n) / (double)n;
        sp = hypot_np(mu, mv);
    }
    mean_u[c] = mu;
    mean_v[c] = mv;
    speed[c] = sp;
}

// ---- per-cell spread and robust centre (icelk_grid_bin_stats; the rules are grid_stats.h's) ----------------------------
// The segment table: where each segment's run of sorted keys begins and how long it is, searched once for the two
// kernels below.  An empty segment gets its six NaN here and is touched by neither of them.
__global__ __launch_bounds__(64) void k_grid_segments(const unsigned long long* __restrict__ keys,
                                                      const int* __restrict__ key_count, int nseg,
                                                      int* __restrict__ seg_begin, int* __restrict__ seg_count,
                                                      icelk_grid_stats_t out)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nseg) return;
    const int total = *key_count;
    const int b = lower_bound(keys, total, (unsigned long long)(unsigned)c << 32);
    const int n = lower_bound(keys, total, (unsigned long long)(unsigned)(c + 1) << 32) - b;
    seg_begin[c] = b;
    seg_count[c] = n;
    if (n > 0) return;
    const double nan = __builtin_nan("");
    out.std_u[c] = out.std_v[c] = out.median_u[c] = out.median_v[c] = out.mad_u[c] = out.mad_v[c] = nan;
}

// np.std(ddof=1) per segment around the mean k_grid_reduce left, one thread per segment as there
__global__ __launch_bounds__(64) void k_grid_std(const unsigned long long* __restrict__ keys,
                                                 const int* __restrict__ seg_begin, const int* __restrict__ seg_count,
                                                 const double* __restrict__ u, const double* __restrict__ v, int nseg,
                                                 const double* __restrict__ mean_u, const double* __restrict__ mean_v,
                                                 double* __restrict__ std_u, double* __restrict__ std_v)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nseg) return;
    const int n = seg_count[c];
    if (n <= 0) return;
    const int b = seg_begin[c];
    std_u[c] = np_std_ddof1(KeyedAt{keys, u, b}, n, mean_u[c]);
    std_v[c] = np_std_ddof1(KeyedAt{keys, v, b}, n, mean_v[c]);
}

// Median and MAD of one segment's u (blockIdx.y 0) or v (1): one workgroup of 256.  The values are gathered through
// the sorted keys once and staged as order keys in the segment's own stretch of `scratch` (scratch_stride per array);
// thread x stages and later reads terms x, x + 256, ... only, so no thread reads another's store.  The MAD's terms
// fabs(a - med) overwrite them in place.  NaN is seen while the terms are staged.
__global__ __launch_bounds__(256) void k_grid_select(const unsigned long long* __restrict__ keys,
                                                     const int* __restrict__ seg_begin,
                                                     const int* __restrict__ seg_count, const double* __restrict__ u,
                                                     const double* __restrict__ v,
                                                     unsigned long long* __restrict__ scratch, size_t scratch_stride,
                                                     icelk_grid_stats_t out)
{
    __shared__ SelectLds lds;
    const int c = blockIdx.x;
    const int n = seg_count[c];
    if (n <= 0) return;
    const int b = seg_begin[c];
    const double* __restrict__ a = blockIdx.y ? v : u;
    unsigned long long* __restrict__ sk = scratch + blockIdx.y * scratch_stride + b;
    const double nan = __builtin_nan("");
    int has_nan = 0;
    for (int t = threadIdx.x; t < n; t += 256) {
        const double x = a[(unsigned)keys[b + t]];
        has_nan |= x != x;
        sk[t] = order_key(x);
    }
    const double med = __syncthreads_or(has_nan) ? nan : wg_median(sk, n, &lds);
    has_nan = 0;
    for (int t = threadIdx.x; t < n; t += 256) {
        const double d = fabs(from_order_key(sk[t]) - med);
        has_nan |= d != d;
        sk[t] = order_key(d);
    }
    const double mad = __syncthreads_or(has_nan) ? nan : wg_median(sk, n, &lds);
    if (threadIdx.x == 0) {
        (blockIdx.y ? out.median_v : out.median_u)[c] = med;
        (blockIdx.y ? out.mad_v : out.mad_u)[c] = mad;
    }
}

}  // namespace

void launch_points_in_polygon(hipStream_t s, const double* poly, int n, const double* pts, int m, uint8_t* out)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(k_points_in_polygon, dim3((m + 255) / 256), dim3(256), 0, s, poly, n, pts, m, out);
}

void launch_grid_assign(hipStream_t s, const double* x, const double* y, int n, double left, double top, double spacing,
                        int cols, int rows, const uint8_t* cell_on, unsigned long long* keys, int* key_count, int key_cap)
{
    if (n <= 0) return;
    const GridGeom g{left, top, spacing, cols, rows};
    hipLaunchKernelGGL(k_grid_assign, dim3((n + 255) / 256), dim3(256), 0, s, x, y, n, g, cell_on, keys, key_count,
                       key_cap);
}

void launch_grid_day_assign(hipStream_t s, const double* x, const double* y, const double* t, int n,
                            const long long* file_off, const int* file_cam, const int* win_f0, const int* win_f1,
                            int nfiles, const long long* t_lo, const long long* t_hi, int ncam, int nw, double left,
                            double top, double spacing, int cols, int rows, const uint8_t* cell_on,
                            unsigned long long* keys, int* key_count, int key_cap, int* sel_count,
                            unsigned long long* t_min, unsigned long long* t_max)
{
    if (n <= 0) return;
    const GridGeom g{left, top, spacing, cols, rows};
    const DayTables D{file_off, file_cam, win_f0, win_f1, t_lo, t_hi, nfiles, ncam, nw};
    hipLaunchKernelGGL(k_grid_day_assign, dim3((n + 255) / 256), dim3(256), 0, s, x, y, t, n, D, g, cell_on,
                       cols * rows, keys, key_count, key_cap, sel_count, t_min, t_max);
}

static size_t box_lds_bytes(int nboxes, int nvert)
{
    return sizeof(double) * (2 * (size_t)nvert + 2 * (size_t)nboxes) + sizeof(int) * ((size_t)nboxes + 1);
}

void launch_boxes_assign(hipStream_t s, const double* x, const double* y, int n, const double* box_xy, const int* box_off,
                         int nboxes, int nvert, const double* u, const double* v, double* ur, double* vr, const double* rot,
                         unsigned long long* keys, int* key_count, int key_cap)
{
    if (n <= 0) return;
    const BoxList L{box_xy, box_off, nboxes, nvert};
    const BoxRot R{u, v, ur, vr, rot ? rot[0] : 1.0, rot ? rot[1] : 0.0, rot ? 1 : 0};
    hipLaunchKernelGGL(k_boxes_assign, dim3((n + 255) / 256), dim3(256), box_lds_bytes(nboxes, nvert), s, x, y, n, L, R,
                       keys, key_count, key_cap);
}

void launch_boxes_day_assign(hipStream_t s, const double* x, const double* y, const double* t, int n,
                             const long long* file_off, const int* file_cam, const int* win_f0, const int* win_f1,
                             int nfiles, const long long* t_lo, const long long* t_hi, int ncam, int nw,
                             const double* box_xy, const int* box_off, int nboxes, int nvert, const double* u,
                             const double* v, double* ur, double* vr, const double* rot, unsigned long long* keys,
                             int* key_count, int key_cap, int* sel_count, unsigned long long* t_min,
                             unsigned long long* t_max)
{
    if (n <= 0) return;
    const DayTables D{file_off, file_cam, win_f0, win_f1, t_lo, t_hi, nfiles, ncam, nw};
    const BoxList L{box_xy, box_off, nboxes, nvert};
    const BoxRot R{u, v, ur, vr, rot ? rot[0] : 1.0, rot ? rot[1] : 0.0, rot ? 1 : 0};
    hipLaunchKernelGGL(k_boxes_day_assign, dim3((n + 255) / 256), dim3(256), box_lds_bytes(nboxes, nvert), s, x, y, t, n,
                       D, L, R, keys, key_count, key_cap, sel_count, t_min, t_max);
}

void launch_grid_reduce(hipStream_t s, const unsigned long long* keys, const int* key_count, const double* u,
                        const double* v, int ncells, int* count, double* mean_u, double* mean_v, double* speed)
{
    if (ncells <= 0) return;
    hipLaunchKernelGGL(k_grid_reduce, dim3((ncells + 63) / 64), dim3(64), 0, s, keys, key_count, u, v, ncells, count,
                       mean_u, mean_v, speed);
}

void launch_grid_segments(hipStream_t s, const unsigned long long* keys, const int* key_count, int nseg, int* seg_begin,
                          int* seg_count, const icelk_grid_stats_t& out)
{
    if (nseg <= 0) return;
    hipLaunchKernelGGL(k_grid_segments, dim3((nseg + 63) / 64), dim3(64), 0, s, keys, key_count, nseg, seg_begin,
                       seg_count, out);
}

void launch_grid_std(hipStream_t s, const unsigned long long* keys, const int* seg_begin, const int* seg_count,
                     const double* u, const double* v, int nseg, const double* mean_u, const double* mean_v,
                     const icelk_grid_stats_t& out)
{
    if (nseg <= 0) return;
    hipLaunchKernelGGL(k_grid_std, dim3((nseg + 63) / 64), dim3(64), 0, s, keys, seg_begin, seg_count, u, v, nseg,
                       mean_u, mean_v, out.std_u, out.std_v);
}

void launch_grid_select(hipStream_t s, const unsigned long long* keys, const int* seg_begin, const int* seg_count,
                        const double* u, const double* v, int nseg, unsigned long long* scratch, size_t scratch_stride,
                        const icelk_grid_stats_t& out)
{
    if (nseg <= 0) return;
    hipLaunchKernelGGL(k_grid_select, dim3(nseg, 2), dim3(256), 0, s, keys, seg_begin, seg_count, u, v, scratch,
                       scratch_stride, out);
}

}  // namespace icelk
