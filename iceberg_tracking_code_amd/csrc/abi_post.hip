// abi_post.hip -- after the frame loop: projection, point-in-polygon, gridding (one set / a day of windows), binning
// into transect and mooring boxes (likewise), the velocity cube and its averages.
#include "icelk_ctx.h"
#include "cube_means.h"
#include "grid_stats.h"
#include "validate.h"

namespace icelk {

// ---- what icelk_grid_bin and icelk_grid_bin_windows share ------------------------------------------------------------
// A key holds its segment (a cell, or window * ncells + cell) in the high 32 bits, the point index in the low 32.
struct GridDev {
    const double *du = nullptr, *dv = nullptr;                    // per point (the caller's)
    unsigned long long *keys = nullptr, *keys_sorted = nullptr;   // key_cap each
    int *d_key_count = nullptr, *d_count = nullptr;               // 1, nseg
    double *d_mu = nullptr, *d_mv = nullptr, *d_sp = nullptr;     // nseg each
    void* sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
    int key_cap = 0, nseg = 0, key_bits = 0;
    // only with statistics (alloc_stats): the segment table, the select's staged order keys (u, then v), the six outputs
    int *seg_begin = nullptr, *seg_count = nullptr;               // nseg each
    unsigned long long* stat_keys = nullptr;                      // 2 * key_cap
    icelk_grid_stats_t d_stats = {};                              // nseg each; null members: no statistics

    void alloc(DevBufs& B, int key_cap_, int nseg_)
    {
        key_cap = key_cap_;
        nseg = nseg_;
        keys = B.get<unsigned long long>((size_t)key_cap);
        keys_sorted = B.get<unsigned long long>((size_t)key_cap);
        d_key_count = B.get<int>(1);
        d_count = B.get<int>((size_t)nseg);
        d_mu = B.get<double>((size_t)nseg);
        d_mv = B.get<double>((size_t)nseg);
        d_sp = B.get<double>((size_t)nseg);
    }
    void alloc_stats(DevBufs& B)
    {
        seg_begin = B.get<int>((size_t)nseg);
        seg_count = B.get<int>((size_t)nseg);
        stat_keys = B.get<unsigned long long>(2 * (size_t)key_cap);
        for (double** q : {&d_stats.std_u, &d_stats.std_v, &d_stats.median_u, &d_stats.median_v, &d_stats.mad_u, &d_stats.mad_v})
            *q = B.get<double>((size_t)nseg);
    }
    // the sort's scratch, for key_cap keys: nothing is allocated between the kernels (the day gridder times them)
    void alloc_sort(DevBufs& B, hipStream_t s)
    {
        for (key_bits = 33; (1LL << (key_bits - 32)) < (long long)nseg;) key_bits++;
        sort_tmp_bytes = sort_keys_asc(s, nullptr, 0, keys, keys_sorted, key_cap, key_bits);
        sort_tmp = B.get<uint8_t>(sort_tmp_bytes);
    }
};

// Zero the key counter, assign (the caller's launch, with whatever it enqueues in front of it), read the key count back,
// sort, reduce, and enqueue the copies of the four per-segment outputs; the caller synchronises.  With `stats` (the
// host's six arrays; G.alloc_stats has run) the segment table, the standard deviations and the selections follow the
// reduce on the same stream and their outputs are copied too.  t, if given: t[0] ends behind the assign launch (the
// caller records its start), t[1] goes around sort + reduce (+ statistics) -- the read-back between them is not timed.
template <typename Assign>
static int grid_core(Ctx* c, const GridDev& G, Assign assign, const char* assign_name, EvPair* t, int* count,
                     double* mean_u, double* mean_v, double* speed, const icelk_grid_stats_t* stats)
{
    const hipStream_t s = c->stream;
    HIPCHK(c, hipMemsetAsync(G.d_key_count, 0, sizeof(int), s));
    int rc = assign();
    if (rc) return rc;
    rc = check_launch(c, assign_name);
    if (rc) return rc;
    if (t) HIPCHK(c, hipEventRecord(t[0].b, s));
    // the sort takes the key count from the host
    int total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, G.d_key_count, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (total > G.key_cap) FAIL(c, ICELK_ECAP, "more than two cells or boxes per point on average (all points on cell edges, or boxes that overlap?)");
    if (t) HIPCHK(c, hipEventRecord(t[1].a, s));
    const unsigned long long* sorted = G.keys;
    if (total > 1) {
        sort_keys_asc(s, G.sort_tmp, G.sort_tmp_bytes, G.keys, G.keys_sorted, total, G.key_bits);
        rc = check_launch(c, "grid sort");
        if (rc) return rc;
        sorted = G.keys_sorted;
    }
    launch_grid_reduce(s, sorted, G.d_key_count, G.du, G.dv, G.nseg, G.d_count, G.d_mu, G.d_mv, G.d_sp);
    rc = check_launch(c, "grid_reduce");
    if (rc) return rc;
    if (stats) {
        {
            ProfScope p(c, K_GRID_SEGMENTS);
            launch_grid_segments(s, sorted, G.d_key_count, G.nseg, G.seg_begin, G.seg_count, G.d_stats);
        }
        {
            ProfScope p(c, K_GRID_STD);
            launch_grid_std(s, sorted, G.seg_begin, G.seg_count, G.du, G.dv, G.nseg, G.d_mu, G.d_mv, G.d_stats);
        }
        {
            ProfScope p(c, K_GRID_SELECT);
            launch_grid_select(s, sorted, G.seg_begin, G.seg_count, G.du, G.dv, G.nseg, G.stat_keys, (size_t)G.key_cap,
                               G.d_stats);
        }
        rc = check_launch(c, "grid statistics");
        if (rc) return rc;
    }
    if (t) HIPCHK(c, hipEventRecord(t[1].b, s));
    HIPCHK(c, copy_n(count, G.d_count, (size_t)G.nseg, kD2H, s));
    HIPCHK(c, copy_n(mean_u, G.d_mu, (size_t)G.nseg, kD2H, s));
    HIPCHK(c, copy_n(mean_v, G.d_mv, (size_t)G.nseg, kD2H, s));
    HIPCHK(c, copy_n(speed, G.d_sp, (size_t)G.nseg, kD2H, s));
    if (stats) {
        double* const host[6] = {stats->std_u, stats->std_v, stats->median_u, stats->median_v, stats->mad_u, stats->mad_v};
        const icelk_grid_stats_t& d = G.d_stats;
        const double* const dev[6] = {d.std_u, d.std_v, d.median_u, d.median_v, d.mad_u, d.mad_v};
        for (int k = 0; k < 6; k++) HIPCHK(c, copy_n(host[k], dev[k], (size_t)G.nseg, kD2H, s));
    }
    return ICELK_OK;
}

// element t of a host array (grid_stats.h on the CPU: icelk_grid_cell_stats_host)
struct PlainAt {
    const double* a;
    double operator()(int t) const { return a[t]; }
};

static bool stats_complete(const icelk_grid_stats_t* st)
{
    return st && st->std_u && st->std_v && st->median_u && st->median_v && st->mad_u && st->mad_v;
}

// ---- the day's file and window tables (icelk_grid_bin_windows, icelk_boxes_bin_windows) ------------------------------
static bool day_tables_complete(const icelk_day_tables_t& T)
{
    return T.nfiles >= 1 && T.ncam >= 1 && T.nw >= 1 && T.file_offset && T.file_cam && T.win_f0 && T.win_f1 && T.t_lo && T.t_hi;
}

// the rules of include/icelk.h for complete tables over n points
static int check_day_tables(Ctx* c, const icelk_day_tables_t& T, int n)
{
    const int nfiles = T.nfiles, ncam = T.ncam, nw = T.nw;
    if (T.file_offset[0] != 0 || T.file_offset[nfiles] != n) FAIL(c, ICELK_EARG, "file offsets must span 0 .. n");
    for (int f = 0; f < nfiles; f++)
        if (T.file_offset[f + 1] < T.file_offset[f] || T.file_cam[f] < 0 || T.file_cam[f] >= ncam ||
            (f > 0 && T.file_cam[f] < T.file_cam[f - 1]))
            FAIL(c, ICELK_EARG, "bad file table");
    for (int k = 0; k < ncam; k++)
        for (int w = 0; w < nw; w++) {
            const size_t sl = (size_t)k * nw + w;
            if (T.t_lo[sl] > T.t_hi[sl] || (w + 1 < nw && T.t_hi[sl] > T.t_lo[sl + 1]))
                FAIL(c, ICELK_EARG, "window bounds must be ascending and disjoint per camera");
            if (T.win_f0[sl] <= T.win_f1[sl] && (T.win_f0[sl] < 0 || T.win_f1[sl] >= nfiles || T.file_cam[T.win_f0[sl]] != k ||
                                                 T.file_cam[T.win_f1[sl]] != k))
                FAIL(c, ICELK_EARG, "a window loads files of another camera");
        }
    return ICELK_OK;
}

// the tables on the device, with the per-(window, camera) selection count and time range the assign kernel fills
struct DayDev {
    long long *off = nullptr, *lo = nullptr, *hi = nullptr;
    int *fcam = nullptr, *wf0 = nullptr, *wf1 = nullptr, *sel = nullptr;
    unsigned long long *tmin = nullptr, *tmax = nullptr;
    int nfiles = 0, nslot = 0;

    void alloc(DevBufs& B, const icelk_day_tables_t& T)
    {
        nfiles = T.nfiles;
        nslot = T.nw * T.ncam;
        off = B.get<long long>((size_t)nfiles + 1);
        fcam = B.get<int>((size_t)nfiles);
        wf0 = B.get<int>((size_t)nslot);
        wf1 = B.get<int>((size_t)nslot);
        lo = B.get<long long>((size_t)nslot);
        hi = B.get<long long>((size_t)nslot);
        sel = B.get<int>((size_t)nslot);
        tmin = B.get<unsigned long long>((size_t)nslot);
        tmax = B.get<unsigned long long>((size_t)nslot);
    }
    int upload(Ctx* c, const icelk_day_tables_t& T, hipStream_t s) const
    {
        HIPCHK(c, copy_n(off, T.file_offset, (size_t)nfiles + 1, kH2D, s));
        HIPCHK(c, copy_n(fcam, T.file_cam, (size_t)nfiles, kH2D, s));
        HIPCHK(c, copy_n(wf0, T.win_f0, (size_t)nslot, kH2D, s));
        HIPCHK(c, copy_n(wf1, T.win_f1, (size_t)nslot, kH2D, s));
        HIPCHK(c, copy_n(lo, T.t_lo, (size_t)nslot, kH2D, s));
        HIPCHK(c, copy_n(hi, T.t_hi, (size_t)nslot, kH2D, s));
        return ICELK_OK;
    }
    // in front of the assign kernel: nothing selected, the range empty
    int reset(Ctx* c, hipStream_t s) const
    {
        HIPCHK(c, hipMemsetAsync(sel, 0, sizeof(int) * nslot, s));
        HIPCHK(c, hipMemsetAsync(tmin, 0xff, sizeof(unsigned long long) * nslot, s));
        HIPCHK(c, hipMemsetAsync(tmax, 0, sizeof(unsigned long long) * nslot, s));
        return ICELK_OK;
    }
    // waits for the stream; t_min / t_max keep their 0 where nothing was selected
    int read_back(Ctx* c, hipStream_t s, int* sel_count, double* t_min, double* t_max) const
    {
        HIPCHK(c, copy_n(sel_count, sel, (size_t)nslot, kD2H, s));
        std::vector<unsigned long long> kmin(nslot), kmax(nslot);
        HIPCHK(c, copy_n(kmin.data(), tmin, (size_t)nslot, kD2H, s));
        HIPCHK(c, copy_n(kmax.data(), tmax, (size_t)nslot, kD2H, s));
        HIPCHK(c, hipStreamSynchronize(s));
        for (int k = 0; k < nslot; k++)
            if (sel_count[k] > 0) {
                t_min[k] = from_order_key(kmin[k]);
                t_max[k] = from_order_key(kmax[k]);
            }
        return ICELK_OK;
    }
};

// the sum of the two timed stretches of grid_core
static int elapsed_ms(Ctx* c, const EvPair* timer, double* device_ms)
{
    float a = 0.0f, b = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&a, timer[0].a, timer[0].b));
    HIPCHK(c, hipEventElapsedTime(&b, timer[1].a, timer[1].b));
    *device_ms = (double)a + (double)b;
    return ICELK_OK;
}

// what a day call answers when no point reaches a segment or a slot: zeros, NaN statistics
static void clear_day_outputs(int nseg, int nslot, int* count, double* mean_u, double* mean_v, double* speed,
                              const icelk_grid_stats_t* stats, int* sel_count, double* t_min, double* t_max, double* device_ms)
{
    memset(count, 0, sizeof(int) * nseg);
    memset(mean_u, 0, sizeof(double) * nseg);
    memset(mean_v, 0, sizeof(double) * nseg);
    memset(speed, 0, sizeof(double) * nseg);
    memset(sel_count, 0, sizeof(int) * nslot);
    memset(t_min, 0, sizeof(double) * nslot);
    memset(t_max, 0, sizeof(double) * nslot);
    if (stats)
        for (double* q : {stats->std_u, stats->std_v, stats->median_u, stats->median_v, stats->mad_u, stats->mad_v})
            std::fill(q, q + nseg, __builtin_nan(""));
    if (device_ms) *device_ms = 0.0;
}

// ---- the box list of icelk_boxes_bin / icelk_boxes_bin_windows ------------------------------------------------------
constexpr int kMaxBoxes = 1024, kMaxBoxVertices = 2048;   // 32 KB of vertices in LDS (k_grid.hip)

// ICELK_OK, or the refusal and its text
static int check_boxes(const icelk_boxes_t* b, const char** why)
{
    *why = "";
    if (!b || !b->xy || !b->offset || b->nboxes < 1) return *why = "box list missing or empty", ICELK_EARG;
    if (b->nboxes > kMaxBoxes) return *why = "more than 1024 boxes", ICELK_ECAP;
    if (b->offset[0] != 0) return *why = "box offsets must start at 0", ICELK_EARG;
    for (int k = 0; k < b->nboxes; k++) {
        if (b->offset[k + 1] < b->offset[k]) return *why = "box offsets must ascend", ICELK_EARG;
        if (b->offset[k + 1] - b->offset[k] < 3) return *why = "a polygon of fewer than three vertices", ICELK_EARG;
        if (b->offset[k + 1] > kMaxBoxVertices) return *why = "more than 2048 box vertices", ICELK_ECAP;
    }
    const int nvert = b->offset[b->nboxes];
    for (int k = 0; k < 2 * nvert; k++)
        if (!std::isfinite(b->xy[k])) return *why = "a box vertex is not finite", ICELK_EARG;
    return ICELK_OK;
}

// run the projection kernel over `n` gathered tracks sitting in d_tracks_in and bring the results to the host
int project_core(Ctx* c, const float* d_tracks_in, int n, int nv, const icelk_camera_t* cam, const icelk_utm_filter_t* filt,
                 int host_pitch, double* x, double* y, double* u, double* v, double* speed, uint8_t* keep)
{
    const int m = nv - 1;
    const size_t need = (size_t)n * (m > 0 ? m : 1);
    if (need > c->post.proj_cap) {
        if (c->post.d_proj) hipFree(c->post.d_proj);
        c->post.d_proj = nullptr;
        c->post.proj_cap = 0;
        int rc = dmalloc(c, &c->post.d_proj, 5 * need);
        if (!rc && !c->post.d_keep) rc = dmalloc(c, &c->post.d_keep, (size_t)c->max_pts);   // n <= max_pts always
        if (rc) return rc;
        c->post.proj_cap = need;
    }
    double* P[5];
    for (int k = 0; k < 5; k++) P[k] = c->post.d_proj + (size_t)k * c->post.proj_cap;
    {
        ProfScope p(c, K_PROJECT);
        launch_project_tracks(c->stream, d_tracks_in, n, nv, *cam, *filt, P[0], P[1], P[2], P[3], P[4], c->post.d_keep);
    }
    int rc = check_launch(c, "project_tracks");
    if (rc) return rc;
    double* H[5] = {x, y, u, v, speed};
    for (int k = 0; k < 5; k++)
        if (H[k] && m > 0)
            HIPCHK(c, hipMemcpy2DAsync(H[k], sizeof(double) * host_pitch, P[k], sizeof(double) * m, sizeof(double) * m, n,
                                       hipMemcpyDeviceToHost, c->stream));
    if (keep) HIPCHK(c, hipMemcpyAsync(keep, c->post.d_keep, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

int check_projection_args(Ctx* c, const icelk_camera_t* cam, const icelk_utm_filter_t* filt)
{
    if (!cam || !filt) FAIL(c, ICELK_EARG, "camera / filter missing");
    if (!(filt->interval_s > 0)) FAIL(c, ICELK_EARG, "tracking interval must be positive");
    return ICELK_OK;
}

static void cube_free(Ctx* c)
{
    for (double** q : {&c->post.d_cube_u, &c->post.d_cube_v, &c->post.d_cube_count}) {
        if (*q) hipFree(*q);
        *q = nullptr;
    }
    c->post.cube_ncells = c->post.cube_nt = 0;
}

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_project_tracks(icelk_t* h, const float* tracks, int n, int n_vertices, const icelk_camera_t* cam,
                         const icelk_utm_filter_t* filt, double* x, double* y, double* u, double* v, double* speed,
                         uint8_t* keep)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = check_projection_args(c, cam, filt);
    if (rc) return rc;
    if (n < 0 || n_vertices < 1 || (n > 0 && !tracks)) FAIL(c, ICELK_EARG, "bad track array");
    if (n > c->max_pts) FAIL(c, ICELK_ECAP, "more tracks than max_pts of icelk_create");
    if (n_vertices > kMaxVert) FAIL(c, ICELK_ECAP, "more than 17 vertices per track");
    if (n == 0) return ICELK_OK;
    HIPCHK(c, hipMemcpyAsync(c->d_out_tracks, tracks, sizeof(float) * 2 * (size_t)n * n_vertices, hipMemcpyHostToDevice,
                             c->stream));
    return project_core(c, c->d_out_tracks, n, n_vertices, cam, filt, n_vertices - 1, x, y, u, v, speed, keep);
}

// ---- gridding of projected velocities (s3_utm_to_gridded_utm.py:391-421) ------------------------

int icelk_points_in_polygon(icelk_t* h, const double* poly_xy, int n_poly, const double* pts_xy, int n_pts,
                            uint8_t* inside)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (n_poly < 0 || n_pts < 0 || (n_poly > 0 && !poly_xy) || (n_pts > 0 && (!pts_xy || !inside)))
        FAIL(c, ICELK_EARG, "bad polygon / point arrays");
    if (n_pts == 0) return ICELK_OK;
    DevBufs B;
    double* d_poly = B.get<double>(2 * (size_t)n_poly);
    double* d_pts = B.get<double>(2 * (size_t)n_pts);
    uint8_t* d_out = B.get<uint8_t>((size_t)n_pts);
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    if (n_poly > 0) HIPCHK(c, copy_n(d_poly, poly_xy, 2 * (size_t)n_poly, kH2D, c->stream));
    HIPCHK(c, copy_n(d_pts, pts_xy, 2 * (size_t)n_pts, kH2D, c->stream));
    launch_points_in_polygon(c->stream, d_poly, n_poly, d_pts, n_pts, d_out);
    int rc = check_launch(c, "points_in_polygon");
    if (rc) return rc;
    HIPCHK(c, copy_n(inside, d_out, (size_t)n_pts, kD2H, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

// icelk_grid_bin, and with `stats` icelk_grid_bin_stats
static int grid_bin(icelk_t* h, const double* x, const double* y, const double* u, const double* v, int n, double left,
                    double top, double spacing, int cols, int rows, const uint8_t* cell_on, int* count, double* mean_u,
                    double* mean_v, double* speed, const icelk_grid_stats_t* stats)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (stats && !stats_complete(stats)) FAIL(c, ICELK_EARG, "a member of the statistics struct is null");
    if (n < 0 || cols <= 0 || rows <= 0 || !(spacing > 0) || !cell_on || !count || !mean_u || !mean_v || !speed ||
        (n > 0 && (!x || !y || !u || !v)))
        FAIL(c, ICELK_EARG, "bad gridding arguments");
    if ((long long)cols * rows > (1 << 24) || n > (1 << 27)) FAIL(c, ICELK_ECAP, "grid or point set too large");
    const int ncells = cols * rows;
    // a point lies in one cell, or -- exactly on an edge / corner -- in up to four; 2 n + 1024 keys cover any set
    // whose points are not all on edges, and the count is checked
    const int key_cap = (int)std::min<long long>(2LL * n + 1024, 0x7fffffffLL);
    DevBufs B;
    GridDev G;
    double* dx = B.get<double>((size_t)n);
    double* dy = B.get<double>((size_t)n);
    double* du = B.get<double>((size_t)n);
    double* dv = B.get<double>((size_t)n);
    uint8_t* d_on = B.get<uint8_t>((size_t)ncells);
    const hipStream_t s = c->stream;
    G.alloc(B, key_cap, ncells);
    if (stats) G.alloc_stats(B);
    G.alloc_sort(B, s);
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    G.du = du;
    G.dv = dv;
    if (n > 0) {
        HIPCHK(c, copy_n(dx, x, (size_t)n, kH2D, s));
        HIPCHK(c, copy_n(dy, y, (size_t)n, kH2D, s));
        HIPCHK(c, copy_n(du, u, (size_t)n, kH2D, s));
        HIPCHK(c, copy_n(dv, v, (size_t)n, kH2D, s));
    }
    HIPCHK(c, copy_n(d_on, cell_on, (size_t)ncells, kH2D, s));
    auto assign = [&]() -> int {
        launch_grid_assign(s, dx, dy, n, left, top, spacing, cols, rows, d_on, G.keys, G.d_key_count, key_cap);
        return ICELK_OK;
    };
    int rc = grid_core(c, G, assign, "grid_assign", nullptr, count, mean_u, mean_v, speed, stats);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(s));
    return ICELK_OK;
}

int icelk_grid_bin(icelk_t* h, const double* x, const double* y, const double* u, const double* v, int n, double left,
                   double top, double spacing, int cols, int rows, const uint8_t* cell_on, int* count, double* mean_u,
                   double* mean_v, double* speed)
{
    return grid_bin(h, x, y, u, v, n, left, top, spacing, cols, rows, cell_on, count, mean_u, mean_v, speed, nullptr);
}

int icelk_grid_bin_stats(icelk_t* h, const double* x, const double* y, const double* u, const double* v, int n,
                         double left, double top, double spacing, int cols, int rows, const uint8_t* cell_on,
                         int* count, double* mean_u, double* mean_v, double* speed, const icelk_grid_stats_t* stats)
{
    if (!h) return ICELK_EARG;
    if (!stats) FAIL(C(h), ICELK_EARG, "the statistics struct is null");
    return grid_bin(h, x, y, u, v, n, left, top, spacing, cols, rows, cell_on, count, mean_u, mean_v, speed, stats);
}

// icelk_grid_bin_windows, with `stats` icelk_grid_bin_windows_stats, with `val` icelk_grid_bin_windows_validated: the
// normalised median test runs on the uploaded points in front of the gridder, with the day tables' windows as groups, and
// turns the device copy of t into NaN at every rejected point -- which day_window then finds in no window
static int grid_bin_windows(icelk_t* h, const double* x, const double* y, const double* u, const double* v,
                            const double* t, int n, const int64_t* file_offset, const int* file_cam, const int* win_f0,
                            const int* win_f1, int nfiles, const int64_t* t_lo, const int64_t* t_hi, int ncam, int nw,
                            double left, double top, double spacing, int cols, int rows, const uint8_t* cell_on,
                            int* count, double* mean_u, double* mean_v, double* speed, int* sel_count, double* t_min,
                            double* t_max, double* device_ms, const icelk_grid_stats_t* stats, const ValidateDay* val = nullptr)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (stats && !stats_complete(stats)) FAIL(c, ICELK_EARG, "a member of the statistics struct is null");
    if (val && (!val->L || !val->rejected || (n > 0 && !val->status))) FAIL(c, ICELK_EARG, "the lattice or an output of the validation is null");
    if (n < 0 || nfiles < 1 || ncam < 1 || nw < 1 || cols <= 0 || rows <= 0 || !(spacing > 0) || !file_offset ||
        !file_cam || !win_f0 || !win_f1 || !t_lo || !t_hi || !cell_on || !count || !mean_u || !mean_v || !speed ||
        !sel_count || !t_min || !t_max || (n > 0 && (!x || !y || !u || !v || !t)))
        FAIL(c, ICELK_EARG, "bad gridding arguments");
    const long long ncells_ll = (long long)cols * rows;
    // keys hold (window * ncells + cell) in their high 32 bits, the point index in the low 32; the key counter and
    // the 2 n + 1024 key slots are int
    if (ncells_ll > (1 << 24) || ncells_ll * nw > 0x7fffffffLL || n > (1 << 30))
        FAIL(c, ICELK_ECAP, "grid x windows or point set too large");
    const icelk_day_tables_t T{file_offset, file_cam, win_f0, win_f1, nfiles, t_lo, t_hi, ncam, nw};
    if (int rct = check_day_tables(c, T, n)) return rct;
    if (val) {
        const int rcv = validate::check(*val->L, val->P, n, nw);
        if (rcv == ICELK_ECAP) FAIL(c, rcv, "validation: more than 2^27 points, or windows x cols x rows of the lattice does not fit 31 bits");
        if (rcv) FAIL(c, rcv, "validation: threshold, eps and side must be positive and finite, min_neighbours, cols and rows at least 1");
    }
    const int ncells = (int)ncells_ll, nseg = ncells * nw;
    const int key_cap = (int)std::min<long long>(2LL * n + 1024, 0x7fffffffLL);
    clear_day_outputs(nseg, nw * ncam, count, mean_u, mean_v, speed, stats, sel_count, t_min, t_max, device_ms);
    if (val) std::fill(val->rejected, val->rejected + nw, 0);
    if (n == 0) return ICELK_OK;
    DevBufs B;
    GridDev G;
    DayDev D;
    ValidateDev V;
    const size_t nn = (size_t)n;
    double* dx = B.get<double>(nn);
    double* dy = B.get<double>(nn);
    double* du = B.get<double>(nn);
    double* dv = B.get<double>(nn);
    double* dt = B.get<double>(nn);
    D.alloc(B, T);
    uint8_t* d_on = B.get<uint8_t>((size_t)ncells);
    G.alloc(B, key_cap, nseg);
    if (stats) G.alloc_stats(B);
    const hipStream_t s = c->stream;
    G.alloc_sort(B, s);
    if (val) V.alloc(B, n, nw, *val->L, val->P, s);
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    G.du = du;
    G.dv = dv;
    HIPCHK(c, copy_n(dx, x, nn, kH2D, s));
    HIPCHK(c, copy_n(dy, y, nn, kH2D, s));
    HIPCHK(c, copy_n(du, u, nn, kH2D, s));
    HIPCHK(c, copy_n(dv, v, nn, kH2D, s));
    HIPCHK(c, copy_n(dt, t, nn, kH2D, s));
    if (int rct = D.upload(c, T, s)) return rct;
    HIPCHK(c, copy_n(d_on, cell_on, (size_t)ncells, kH2D, s));
    EvPair vtimer[2];
    if (val) {
        if (device_ms) {
            int rct = vtimer[0].create(c);
            if (!rct) rct = vtimer[1].create(c);
            if (rct) return rct;
        }
        V.A.x = dx, V.A.y = dy, V.A.u = du, V.A.v = dv, V.A.t_kill = dt;
        auto vassign = [&] {
            launch_validate_day_assign(s, V.A, dt, D.off, D.fcam, D.wf0, D.wf1, nfiles, D.lo, D.hi, ncam, nw);
        };
        if (int rct = validate_run(c, V, vassign, device_ms ? vtimer : nullptr)) return rct;
        HIPCHK(c, copy_n(val->status, V.A.status, nn, kD2H, s));
        HIPCHK(c, copy_n(val->rejected, V.A.rejected, (size_t)nw, kD2H, s));
    }
    // device_ms: assign, then sort + reduce; the key-count read-back between them is not counted
    EvPair timer[2];
    auto assign = [&]() -> int {
        if (int rct = D.reset(c, s)) return rct;
        if (device_ms) {
            int rct = timer[0].create(c);
            if (!rct) rct = timer[1].create(c);
            if (rct) return rct;
            HIPCHK(c, hipEventRecord(timer[0].a, s));
        }
        ProfScope p(c, K_GRID_DAY_ASSIGN);
        launch_grid_day_assign(s, dx, dy, dt, n, D.off, D.fcam, D.wf0, D.wf1, nfiles, D.lo, D.hi, ncam, nw, left, top,
                               spacing, cols, rows, d_on, G.keys, G.d_key_count, key_cap, D.sel, D.tmin, D.tmax);
        return ICELK_OK;
    };
    int rc = grid_core(c, G, assign, "grid_day_assign", device_ms ? timer : nullptr, count, mean_u, mean_v, speed, stats);
    if (rc) return rc;
    rc = D.read_back(c, s, sel_count, t_min, t_max);
    if (rc) return rc;
    if (!device_ms) return ICELK_OK;
    rc = elapsed_ms(c, timer, device_ms);
    if (rc || !val) return rc;
    double validation_ms = 0.0;
    rc = elapsed_ms(c, vtimer, &validation_ms);
    *device_ms += validation_ms;
    return rc;
}

// icelk_boxes_bin (T null) and icelk_boxes_bin_windows: the points against the box list, then grid_core with
// nseg = boxes, or windows * boxes
static int boxes_bin(icelk_t* h, const double* x, const double* y, const double* u, const double* v, const double* t,
                     int n, const icelk_day_tables_t* T, const icelk_boxes_t* boxes, const double* rot, int* count,
                     double* mean_u, double* mean_v, double* speed, const icelk_grid_stats_t* stats, int* sel_count,
                     double* t_min, double* t_max, double* device_ms)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (stats && !stats_complete(stats)) FAIL(c, ICELK_EARG, "a member of the statistics struct is null");
    if (n < 0 || !count || !mean_u || !mean_v || !speed || (n > 0 && (!x || !y || !u || !v)))
        FAIL(c, ICELK_EARG, "bad binning arguments");
    if (T && (!day_tables_complete(*T) || !sel_count || !t_min || !t_max || (n > 0 && !t)))
        FAIL(c, ICELK_EARG, "bad binning arguments");
    if (rot && !(std::isfinite(rot[0]) && std::isfinite(rot[1]))) FAIL(c, ICELK_EARG, "the rotation is not finite");
    const char* why = "";
    if (int rcb = check_boxes(boxes, &why)) FAIL(c, rcb, why);
    const int nb = boxes->nboxes, nvert = boxes->offset[nb], nw = T ? T->nw : 1;
    // keys hold (window * nboxes + box) in their high 32 bits; a point may lie in every box, and the key counter is an int
    if ((long long)nb * nw > 0x7fffffffLL || (long long)nb * n > 0x7fffffffLL || n > (T ? 1 << 30 : 1 << 27))
        FAIL(c, ICELK_ECAP, "boxes x windows, boxes x points or point set too large");
    if (T)
        if (int rct = check_day_tables(c, *T, n)) return rct;
    const int nseg = nb * nw;
    const int key_cap = (int)std::min<long long>(2LL * n + 1024, 0x7fffffffLL);
    if (T) {
        clear_day_outputs(nseg, nw * T->ncam, count, mean_u, mean_v, speed, stats, sel_count, t_min, t_max, device_ms);
        if (n == 0) return ICELK_OK;
    }
    DevBufs B;
    GridDev G;
    DayDev D;
    const size_t nn = (size_t)n;
    double* dx = B.get<double>(nn);
    double* dy = B.get<double>(nn);
    double* du = B.get<double>(nn);
    double* dv = B.get<double>(nn);
    double* dur = rot ? B.get<double>(nn) : nullptr;             // the velocities in the boxes' frame (the assign kernel's)
    double* dvr = rot ? B.get<double>(nn) : nullptr;
    double* dt = T ? B.get<double>(nn) : nullptr;
    double* d_bxy = B.get<double>(2 * (size_t)nvert);
    int* d_boff = B.get<int>((size_t)nb + 1);
    if (T) D.alloc(B, *T);
    G.alloc(B, key_cap, nseg);
    if (stats) G.alloc_stats(B);
    const hipStream_t s = c->stream;
    G.alloc_sort(B, s);
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    G.du = rot ? dur : du;
    G.dv = rot ? dvr : dv;
    if (n > 0) {
        HIPCHK(c, copy_n(dx, x, nn, kH2D, s));
        HIPCHK(c, copy_n(dy, y, nn, kH2D, s));
        HIPCHK(c, copy_n(du, u, nn, kH2D, s));
        HIPCHK(c, copy_n(dv, v, nn, kH2D, s));
        if (T) HIPCHK(c, copy_n(dt, t, nn, kH2D, s));
    }
    HIPCHK(c, copy_n(d_bxy, boxes->xy, 2 * (size_t)nvert, kH2D, s));
    HIPCHK(c, copy_n(d_boff, boxes->offset, (size_t)nb + 1, kH2D, s));
    if (T)
        if (int rct = D.upload(c, *T, s)) return rct;
    EvPair timer[2];
    auto assign = [&]() -> int {
        if (!T) {
            ProfScope p(c, K_BOXES_ASSIGN);
            launch_boxes_assign(s, dx, dy, n, d_bxy, d_boff, nb, nvert, du, dv, dur, dvr, rot, G.keys, G.d_key_count, key_cap);
            return ICELK_OK;
        }
        if (int rct = D.reset(c, s)) return rct;
        if (device_ms) {
            int rct = timer[0].create(c);
            if (!rct) rct = timer[1].create(c);
            if (rct) return rct;
            HIPCHK(c, hipEventRecord(timer[0].a, s));
        }
        ProfScope p(c, K_BOXES_DAY_ASSIGN);
        launch_boxes_day_assign(s, dx, dy, dt, n, D.off, D.fcam, D.wf0, D.wf1, T->nfiles, D.lo, D.hi, T->ncam, nw, d_bxy,
                                d_boff, nb, nvert, du, dv, dur, dvr, rot, G.keys, G.d_key_count, key_cap, D.sel, D.tmin,
                                D.tmax);
        return ICELK_OK;
    };
    int rc = grid_core(c, G, assign, T ? "boxes_day_assign" : "boxes_assign", T && device_ms ? timer : nullptr, count, mean_u,
                       mean_v, speed, stats);
    if (rc) return rc;
    if (!T) {
        HIPCHK(c, hipStreamSynchronize(s));
        return ICELK_OK;
    }
    rc = D.read_back(c, s, sel_count, t_min, t_max);
    if (rc) return rc;
    return device_ms ? elapsed_ms(c, timer, device_ms) : ICELK_OK;
}

int icelk_grid_bin_windows(icelk_t* h, const double* x, const double* y, const double* u, const double* v,
                           const double* t, int n, const int64_t* file_offset, const int* file_cam, const int* win_f0,
                           const int* win_f1, int nfiles, const int64_t* t_lo, const int64_t* t_hi, int ncam, int nw,
                           double left, double top, double spacing, int cols, int rows, const uint8_t* cell_on,
                           int* count, double* mean_u, double* mean_v, double* speed, int* sel_count, double* t_min,
                           double* t_max, double* device_ms)
{
    return grid_bin_windows(h, x, y, u, v, t, n, file_offset, file_cam, win_f0, win_f1, nfiles, t_lo, t_hi, ncam, nw,
                            left, top, spacing, cols, rows, cell_on, count, mean_u, mean_v, speed, sel_count, t_min,
                            t_max, device_ms, nullptr);
}

int icelk_grid_bin_windows_stats(icelk_t* h, const double* x, const double* y, const double* u, const double* v,
                                 const double* t, int n, const int64_t* file_offset, const int* file_cam,
                                 const int* win_f0, const int* win_f1, int nfiles, const int64_t* t_lo,
                                 const int64_t* t_hi, int ncam, int nw, double left, double top, double spacing,
                                 int cols, int rows, const uint8_t* cell_on, int* count, double* mean_u, double* mean_v,
                                 double* speed, int* sel_count, double* t_min, double* t_max, double* device_ms,
                                 const icelk_grid_stats_t* stats)
{
    if (!h) return ICELK_EARG;
    if (!stats) FAIL(C(h), ICELK_EARG, "the statistics struct is null");
    return grid_bin_windows(h, x, y, u, v, t, n, file_offset, file_cam, win_f0, win_f1, nfiles, t_lo, t_hi, ncam, nw,
                            left, top, spacing, cols, rows, cell_on, count, mean_u, mean_v, speed, sel_count, t_min,
                            t_max, device_ms, stats);
}

int icelk_grid_bin_windows_validated(icelk_t* h, const double* x, const double* y, const double* u, const double* v,
                                     const double* t, int n, const int64_t* file_offset, const int* file_cam,
                                     const int* win_f0, const int* win_f1, int nfiles, const int64_t* t_lo,
                                     const int64_t* t_hi, int ncam, int nw, double left, double top, double spacing,
                                     int cols, int rows, const uint8_t* cell_on, int* count, double* mean_u, double* mean_v,
                                     double* speed, int* sel_count, double* t_min, double* t_max, double* device_ms,
                                     const icelk_grid_stats_t* stats_or_null, const icelk_validate_lattice_t* lattice,
                                     const icelk_validate_params_t* params, uint8_t* status, int32_t* rejected)
{
    const ValidateDay val{lattice, params ? *params : validate::default_params(), status, rejected};
    return grid_bin_windows(h, x, y, u, v, t, n, file_offset, file_cam, win_f0, win_f1, nfiles, t_lo, t_hi, ncam, nw,
                            left, top, spacing, cols, rows, cell_on, count, mean_u, mean_v, speed, sel_count, t_min,
                            t_max, device_ms, stats_or_null, &val);
}

int icelk_boxes_check(const icelk_boxes_t* boxes)
{
    const char* why = "";
    return check_boxes(boxes, &why);
}

int icelk_boxes_bin(icelk_t* h, const double* x, const double* y, const double* u, const double* v, int n,
                    const icelk_boxes_t* boxes, const double* rot, int* count, double* mean_u, double* mean_v,
                    double* speed, const icelk_grid_stats_t* stats)
{
    return boxes_bin(h, x, y, u, v, nullptr, n, nullptr, boxes, rot, count, mean_u, mean_v, speed, stats, nullptr, nullptr,
                     nullptr, nullptr);
}

int icelk_boxes_bin_windows(icelk_t* h, const double* x, const double* y, const double* u, const double* v,
                            const double* t, int n, const icelk_day_tables_t* day, const icelk_boxes_t* boxes,
                            const double* rot, int* count, double* mean_u, double* mean_v, double* speed,
                            const icelk_grid_stats_t* stats, int* sel_count, double* t_min, double* t_max,
                            double* device_ms)
{
    if (!h) return ICELK_EARG;
    if (!day) FAIL(C(h), ICELK_EARG, "the day tables are null");
    return boxes_bin(h, x, y, u, v, t, n, day, boxes, rot, count, mean_u, mean_v, speed, stats, sel_count, t_min, t_max,
                     device_ms);
}

int icelk_grid_cell_stats_host(const double* a, int n, double* out_std, double* out_median, double* out_mad)
{
    if (n < 0 || (n > 0 && !a) || !out_std || !out_median || !out_mad) return ICELK_EARG;
    cell_stats(PlainAt{a}, n, out_std, out_median, out_mad);
    return ICELK_OK;
}

int icelk_cube_set(icelk_t* h, const double* u, const double* v, const double* count, int ncells, int nt)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!u || !v || !count || ncells < 1 || nt < 1) FAIL(c, ICELK_EARG, "bad cube arguments");
    if ((long long)ncells * nt > 0x7fffffffLL) FAIL(c, ICELK_ECAP, "cells x windows does not fit 31 bits");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    cube_free(c);
    const size_t bytes = sizeof(double) * (size_t)ncells * (size_t)nt;
    if (hipMalloc(&c->post.d_cube_u, bytes) != hipSuccess || hipMalloc(&c->post.d_cube_v, bytes) != hipSuccess ||
        hipMalloc(&c->post.d_cube_count, bytes) != hipSuccess) {
        cube_free(c);
        FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    }
    c->post.cube_ncells = ncells;
    c->post.cube_nt = nt;
    const hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(c->post.d_cube_u, u, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->post.d_cube_v, v, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->post.d_cube_count, count, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return ICELK_OK;
}

int icelk_cube_release(icelk_t* h)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    cube_free(c);
    return ICELK_OK;
}

int icelk_cube_average(icelk_t* h, const int* sel_offset, const int* sel_index, int nperiods, int rows, int cols,
                       int coarseness, double* out_u, double* out_v, double* out_speed, double* out_count,
                       int* out_has_data, double* device_ms)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!sel_offset || nperiods < 1 || rows < 1 || cols < 1 || coarseness < 1 || !out_u || !out_v || !out_speed ||
        !out_count || !out_has_data)
        FAIL(c, ICELK_EARG, "bad cube averaging arguments");
    if (!c->post.d_cube_u) FAIL(c, ICELK_ESTATE, "icelk_cube_set has not been called");
    if ((long long)rows * cols != (long long)c->post.cube_ncells) FAIL(c, ICELK_EARG, "rows x cols is not the cube's cell count");
    if (sel_offset[0] != 0) FAIL(c, ICELK_EARG, "selection offsets must start at 0");
    for (int p = 0; p < nperiods; p++)
        if (sel_offset[p + 1] < sel_offset[p]) FAIL(c, ICELK_EARG, "selection offsets must not decrease");
    const int nsel = sel_offset[nperiods];
    if (nsel > 0 && !sel_index) FAIL(c, ICELK_EARG, "bad cube averaging arguments");
    for (int k = 0; k < nsel; k++)
        if (sel_index[k] < 0 || sel_index[k] >= c->post.cube_nt) FAIL(c, ICELK_EARG, "a selected window lies outside the cube");
    const int ncells = c->post.cube_ncells;
    if ((long long)nperiods * ncells > 0x7fffffffLL) FAIL(c, ICELK_ECAP, "periods x cells does not fit 31 bits");
    // numpy's order of additions changes with the length of a block's rows; beyond this it has not been checked
    if (coarseness > kMaxCoarseness) FAIL(c, ICELK_ECAP, "coarseness above 8193: not checked against numpy");
    const int cr = (rows + coarseness - 1) / coarseness, cc = (cols + coarseness - 1) / coarseness;
    const size_t nfine = (size_t)nperiods * (size_t)ncells, nout = (size_t)nperiods * (size_t)cr * (size_t)cc;
    if (device_ms) *device_ms = 0.0;
    HIPCHK(c, hipSetDevice(c->device));
    DevBufs B;
    int* d_off = B.get<int>((size_t)nperiods + 1);
    int* d_idx = B.get<int>((size_t)nsel);
    int* d_has = B.get<int>((size_t)nperiods);
    double* d_f = B.get<double>(4 * nfine);
    double* d_o = coarseness > 1 ? B.get<double>(4 * nout) : d_f;
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    const hipStream_t s = c->stream;
    HIPCHK(c, copy_n(d_off, sel_offset, (size_t)nperiods + 1, kH2D, s));
    if (nsel > 0) HIPCHK(c, copy_n(d_idx, sel_index, (size_t)nsel, kH2D, s));
    HIPCHK(c, hipMemsetAsync(d_has, 0, sizeof(int) * (size_t)nperiods, s));
    EvPair timer;
    if (device_ms) {
        if (int rct = timer.create(c)) return rct;
        HIPCHK(c, hipEventRecord(timer.a, s));
    }
    // fine fields: u, v, speed, count, one plane of nperiods * ncells each
    launch_cube_temporal(s, c->post.d_cube_u, c->post.d_cube_v, c->post.d_cube_count, ncells, d_off, d_idx, nperiods, d_f, d_f + nfine,
                         d_f + 2 * nfine, d_f + 3 * nfine, d_has);
    int rc = check_launch(c, "cube_temporal");
    if (rc) return rc;
    if (coarseness > 1) {
        launch_cube_spatial(s, d_f, d_f + nfine, d_f + 3 * nfine, rows, cols, coarseness, nperiods, d_o, d_o + nout,
                            d_o + 2 * nout, d_o + 3 * nout);
        rc = check_launch(c, "cube_spatial");
        if (rc) return rc;
    }
    if (device_ms) HIPCHK(c, hipEventRecord(timer.b, s));
    HIPCHK(c, copy_n(out_u, d_o, nout, kD2H, s));
    HIPCHK(c, copy_n(out_v, d_o + nout, nout, kD2H, s));
    HIPCHK(c, copy_n(out_speed, d_o + 2 * nout, nout, kD2H, s));
    HIPCHK(c, copy_n(out_count, d_o + 3 * nout, nout, kD2H, s));
    HIPCHK(c, copy_n(out_has_data, d_has, (size_t)nperiods, kD2H, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (device_ms) {
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, timer.a, timer.b));
        *device_ms = (double)ms;
    }
    return ICELK_OK;
}

}  // extern "C"
