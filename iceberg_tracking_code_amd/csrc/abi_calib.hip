// abi_calib.hip -- before the frame loop: the misfit of the camera calibration over many candidates at once.
#include "icelk_ctx.h"

namespace icelk {

constexpr int kCandDoubles = 11;   // X[3], U[3], V[3], sigma in pixels, H (k_calib.hip)

static void calib_free(Ctx* c)
{
    for (double** q : {&c->calib.d_shore, &c->calib.d_water}) {
        if (*q) hipFree(*q);
        *q = nullptr;
    }
    c->calib.M = c->calib.W = 0;
}

// what icelk_calib_residuals and icelk_calib_cost check alike
static int calib_check(Ctx* c, const double* cand, int P, const void* out)
{
    if (!cand || !out || P < 1) FAIL(c, ICELK_EARG, "bad calibration arguments");
    if (!c->calib.d_shore) FAIL(c, ICELK_ESTATE, "icelk_calib_set has not been called");
    if ((long long)P * c->calib.M > 0x7fffffffLL) FAIL(c, ICELK_ECAP, "candidates x points does not fit 31 bits");
    return ICELK_OK;
}

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_calib_set(icelk_t* h, const double* shore_xy, int M, const double* water_xy, int W, double E, double N)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!shore_xy || !water_xy || M < 1 || W < 1) FAIL(c, ICELK_EARG, "bad calibration scene");
    if ((long long)W > 0x3fffffffLL || (long long)M > 0x3fffffffLL) FAIL(c, ICELK_ECAP, "scene too large");
    for (size_t k = 0; k < 2 * (size_t)W; k++)
        if (!std::isfinite(water_xy[k])) FAIL(c, ICELK_EARG, "waterline vertices must be finite");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    calib_free(c);
    if (hipMalloc(&c->calib.d_shore, sizeof(double) * 2 * (size_t)M) != hipSuccess ||
        hipMalloc(&c->calib.d_water, sizeof(double) * 2 * (size_t)W) != hipSuccess) {
        calib_free(c);
        FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    }
    c->calib.M = M;
    c->calib.W = W;
    c->calib.E = E;
    c->calib.N = N;
    const hipStream_t s = c->stream;
    HIPCHK(c, copy_n(c->calib.d_shore, shore_xy, 2 * (size_t)M, kH2D, s));
    HIPCHK(c, copy_n(c->calib.d_water, water_xy, 2 * (size_t)W, kH2D, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return ICELK_OK;
}

int icelk_calib_release(icelk_t* h)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    calib_free(c);
    return ICELK_OK;
}

int icelk_calib_residuals(icelk_t* h, const double* cand, int P, double* out_dist, double* out_tx, double* out_ty,
                          double* device_ms)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    int rc = calib_check(c, cand, P, out_dist);
    if (rc) return rc;
    const auto& S = c->calib;
    const size_t n = (size_t)P * (size_t)S.M;
    if (device_ms) *device_ms = 0.0;
    HIPCHK(c, hipSetDevice(c->device));
    DevBufs B;
    double* d_cand = B.get<double>((size_t)P * kCandDoubles);
    double* d_dist = B.get<double>(n);
    double* d_tx = out_tx ? B.get<double>(n) : nullptr;
    double* d_ty = out_ty ? B.get<double>(n) : nullptr;
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    const hipStream_t s = c->stream;
    HIPCHK(c, copy_n(d_cand, cand, (size_t)P * kCandDoubles, kH2D, s));
    EvPair timer;
    if (device_ms) {
        if (int rct = timer.create(c)) return rct;
        HIPCHK(c, hipEventRecord(timer.a, s));
    }
    launch_calib_residuals(s, d_cand, P, S.d_shore, S.M, S.d_water, S.W, S.E, S.N, d_dist, d_tx, d_ty);
    rc = check_launch(c, "calib_residuals");
    if (rc) return rc;
    if (device_ms) HIPCHK(c, hipEventRecord(timer.b, s));
    HIPCHK(c, copy_n(out_dist, d_dist, n, kD2H, s));
    if (out_tx) HIPCHK(c, copy_n(out_tx, d_tx, n, kD2H, s));
    if (out_ty) HIPCHK(c, copy_n(out_ty, d_ty, n, kD2H, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (device_ms) {
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, timer.a, timer.b));
        *device_ms = (double)ms;
    }
    return ICELK_OK;
}

int icelk_calib_cost(icelk_t* h, const double* cand, int P, double* out_meansq, double* device_ms)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    int rc = calib_check(c, cand, P, out_meansq);
    if (rc) return rc;
    const auto& S = c->calib;
    if (S.M > calib_cost_max_points()) FAIL(c, ICELK_ECAP, "more shoreline points than the cost kernel holds (4096)");
    if (device_ms) *device_ms = 0.0;
    HIPCHK(c, hipSetDevice(c->device));
    DevBufs B;
    double* d_cand = B.get<double>((size_t)P * kCandDoubles);
    double* d_out = B.get<double>((size_t)P);
    if (!B.ok()) FAIL(c, ICELK_ENOMEM, "hipMalloc failed");
    const hipStream_t s = c->stream;
    HIPCHK(c, copy_n(d_cand, cand, (size_t)P * kCandDoubles, kH2D, s));
    EvPair timer;
    if (device_ms) {
        if (int rct = timer.create(c)) return rct;
        HIPCHK(c, hipEventRecord(timer.a, s));
    }
    launch_calib_cost(s, d_cand, P, S.d_shore, S.M, S.d_water, S.W, S.E, S.N, d_out);
    rc = check_launch(c, "calib_cost");
    if (rc) return rc;
    if (device_ms) HIPCHK(c, hipEventRecord(timer.b, s));
    HIPCHK(c, copy_n(out_meansq, d_out, (size_t)P, kD2H, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (device_ms) {
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, timer.a, timer.b));
        *device_ms = (double)ms;
    }
    return ICELK_OK;
}

}  // extern "C"
