// abi_lk.hip -- plain pyramidal LK: parameters, icelk_pyrlk, icelk_track_fb, icelk_fb_filter.
#include "icelk_ctx.h"

namespace icelk {

int make_lk_params(Ctx* c, int w, int h, int win_w, int win_h, int max_level, int crit_type, int max_count,
                   double epsilon, int flags, double min_eig_thr, float fb_thr, LKParams* P)
{
    if (win_w <= 2 || win_h <= 2) FAIL(c, ICELK_EARG, "winSize must be > 2");
    if (max_level < 0) FAIL(c, ICELK_EARG, "maxLevel must be >= 0");
    if (max_level > kMaxLevels - 1) max_level = kMaxLevels - 1;
    if (win_w * win_h > 64 * 64) FAIL(c, ICELK_EARG, "winSize area above 4096 px is not supported");
    P->win_w = win_w;
    P->win_h = win_h;
    P->top_level = pyramid_top_level(w, h, win_w, win_h, max_level);
    if (!(crit_type & ICELK_CRIT_COUNT)) max_count = 30;
    else max_count = std::min(std::max(max_count, 0), 100);
    if (!(crit_type & ICELK_CRIT_EPS)) epsilon = 0.01;
    else epsilon = std::min(std::max(epsilon, 0.), 10.);
    P->max_count = max_count;
    P->eps2 = epsilon * epsilon;
    // A float evaluation of dx*dx + dy*dy is within 2^-22 (relative) of the double one OpenCV compares with eps^2;
    // outside a 2^-20 band around eps^2 it decides, inside the exact form runs (k_lk_multi.hip)
    if (P->eps2 < 1e-30) {
        P->eps2_lo = -1.f;
        P->eps2_hi = INFINITY;
    } else {
        P->eps2_lo = nextafterf((float)(P->eps2 * (1.0 - 1.0 / (1 << 20))), -INFINITY);
        P->eps2_hi = nextafterf((float)(P->eps2 * (1.0 + 1.0 / (1 << 20))), INFINITY);
    }
    P->flags = flags | c->lk_kernel_flags;
    P->min_eig_thr = (float)min_eig_thr;
    P->fb_thr = fb_thr;
    P->margin = 6;
    P->dist_form = c->fb_dist_form;
    P->sum_mode = c->lk_sum_mode;
    P->sum_guard = c->lk_wide_sums ? 0u : 1u << 26;
    return ICELK_OK;
}

// What icelk_pyrlk and icelk_track_fb do before they fill their LKBuffers: arguments checked in this order, parameters
// made, both pyramids built, p0 uploaded.  n == 0 returns ICELK_OK after the checks that do not look at the points;
// have_bufs: the caller's point buffers are there.
static int lk_prologue(Ctx* c, int slot0, int slot1, const float* p0, bool have_bufs, int n, int win_w, int win_h,
                       int max_level, int crit_type, int max_count, double epsilon, int flags, double min_eig_threshold,
                       float fb_threshold, LKParams* P)
{
    int rc = check_slot(c, slot0, true);
    if (!rc) rc = check_slot(c, slot1, true);
    if (rc) return rc;
    if (n < 0) FAIL(c, ICELK_EARG, "negative point count");
    if (n > c->max_pts) FAIL(c, ICELK_ECAP, "more points than max_pts of icelk_create");
    const Slot& s0 = c->slots[slot0];
    const Slot& s1 = c->slots[slot1];
    if (s0.w != s1.w || s0.h != s1.h) FAIL(c, ICELK_EARG, "frame sizes differ");
    rc = make_lk_params(c, s0.w, s0.h, win_w, win_h, max_level, crit_type, max_count, epsilon, flags, min_eig_threshold,
                        fb_threshold, P);
    if (rc) return rc;
    if (n == 0) return ICELK_OK;
    if (!have_bufs) FAIL(c, ICELK_EARG, "null point buffer");
    rc = ensure_pyramid(c, slot0, P->top_level);
    if (!rc) rc = ensure_pyramid(c, slot1, P->top_level);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_p0, p0, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
    return ICELK_OK;
}

}  // namespace icelk

using namespace icelk;

extern "C" {

// ---- tracker -----------------------------------------------------------------------------------
int icelk_pyrlk(icelk_t* h, int prev_slot, int next_slot, const float* prev_xy, float* next_xy, uint8_t* status,
                float* err, int n, int win_w, int win_h, int max_level, int crit_type, int max_count, double epsilon,
                int flags, double min_eig_threshold)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    LKParams P;
    int rc = lk_prologue(c, prev_slot, next_slot, prev_xy, prev_xy && next_xy, n, win_w, win_h, max_level, crit_type,
                         max_count, epsilon, flags, min_eig_threshold, 1.f, &P);
    if (rc || n == 0) return rc;
    const Slot& s0 = c->slots[prev_slot];
    const Slot& s1 = c->slots[next_slot];
    if (flags & ICELK_FLAG_INITIAL_FLOW)
        HIPCHK(c, hipMemcpyAsync(c->d_p1, next_xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
    LKBuffers B{};
    B.p_in = c->d_p0;
    B.p_fwd = c->d_p1;
    B.st_fwd = c->d_st_f;
    B.err_fwd = err ? c->d_err_f : nullptr;
    if (c->prof) { B.iters = c->d_iters; c->iters_n = n; }
    {
        ProfScope p(c, K_LK);
        rc = launch_lk(c->stream, pyramid_of(s0), pyramid_of(s1), B, n, P, false);
    }
    if (rc) FAIL(c, rc, "unsupported window size");
    rc = check_launch(c, "lk");
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(next_xy, c->d_p1, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, c->stream));
    if (status) HIPCHK(c, hipMemcpyAsync(status, c->d_st_f, n, hipMemcpyDeviceToHost, c->stream));
    if (err) HIPCHK(c, hipMemcpyAsync(err, c->d_err_f, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

int icelk_track_fb(icelk_t* h, int slot0, int slot1, const float* p0, int n, int win_w, int win_h, int max_level,
                   int crit_type, int max_count, double epsilon, double min_eig_threshold, float fb_threshold,
                   float* p1, float* p0r, uint8_t* st_fwd, uint8_t* st_bwd, float* err_fwd, float* err_bwd, float* dist,
                   uint8_t* valid)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    LKParams P;
    int rc = lk_prologue(c, slot0, slot1, p0, p0 != nullptr, n, win_w, win_h, max_level, crit_type, max_count, epsilon, 0,
                         min_eig_threshold, fb_threshold, &P);
    if (rc || n == 0) return rc;
    const Slot& s0 = c->slots[slot0];
    const Slot& s1 = c->slots[slot1];
    LKBuffers B{};
    B.p_in = c->d_p0;
    B.p_fwd = c->d_p1;
    B.st_fwd = c->d_st_f;
    B.err_fwd = err_fwd ? c->d_err_f : nullptr;   // the residual error is only formed for a caller that takes it
    B.p_bwd = c->d_p0r;
    B.st_bwd = c->d_st_b;
    B.err_bwd = err_bwd ? c->d_err_b : nullptr;
    B.dist = c->d_dist;
    B.valid = c->d_valid;
    if (c->prof) { B.iters = c->d_iters; c->iters_n = n; }
    {
        ProfScope p(c, K_LK_FB);
        rc = launch_lk(c->stream, pyramid_of(s0), pyramid_of(s1), B, n, P, true);
    }
    if (rc) FAIL(c, rc, "unsupported window size");
    rc = check_launch(c, "lk_fb");
    if (rc) return rc;
    const size_t fb = sizeof(float) * n;
    if (p1) HIPCHK(c, hipMemcpyAsync(p1, c->d_p1, 2 * fb, hipMemcpyDeviceToHost, c->stream));
    if (p0r) HIPCHK(c, hipMemcpyAsync(p0r, c->d_p0r, 2 * fb, hipMemcpyDeviceToHost, c->stream));
    if (st_fwd) HIPCHK(c, hipMemcpyAsync(st_fwd, c->d_st_f, n, hipMemcpyDeviceToHost, c->stream));
    if (st_bwd) HIPCHK(c, hipMemcpyAsync(st_bwd, c->d_st_b, n, hipMemcpyDeviceToHost, c->stream));
    if (err_fwd) HIPCHK(c, hipMemcpyAsync(err_fwd, c->d_err_f, fb, hipMemcpyDeviceToHost, c->stream));
    if (err_bwd) HIPCHK(c, hipMemcpyAsync(err_bwd, c->d_err_b, fb, hipMemcpyDeviceToHost, c->stream));
    if (dist) HIPCHK(c, hipMemcpyAsync(dist, c->d_dist, fb, hipMemcpyDeviceToHost, c->stream));
    if (valid) HIPCHK(c, hipMemcpyAsync(valid, c->d_valid, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

int icelk_fb_filter(icelk_t* h, const float* p0, const float* p0r, int n, float fb_threshold, float* dist,
                    uint8_t* valid)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (n < 0) FAIL(c, ICELK_EARG, "negative point count");
    if (n > c->max_pts) FAIL(c, ICELK_ECAP, "more points than max_pts of icelk_create");
    if (n == 0) return ICELK_OK;
    if (!p0 || !p0r) FAIL(c, ICELK_EARG, "null point buffer");
    HIPCHK(c, hipMemcpyAsync(c->d_p0, p0, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_p0r, p0r, sizeof(float) * 2 * n, hipMemcpyHostToDevice, c->stream));
    launch_fb_filter(c->stream, c->d_p0, c->d_p0r, n, fb_threshold, c->fb_dist_form, c->d_dist, c->d_valid);
    int rc = check_launch(c, "fb_filter");
    if (rc) return rc;
    if (dist) HIPCHK(c, hipMemcpyAsync(dist, c->d_dist, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    if (valid) HIPCHK(c, hipMemcpyAsync(valid, c->d_valid, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

}  // extern "C"
