// ortho.h -- the arithmetic of the orthophoto: every cell of a map raster projected into a camera's photograph by
// Camera.utm_to_photo (imports/camtools.py:334-392), sampled there, and the cameras merged into one mosaic -- as plain C++
// for the host and the device alike.  The kernel (k_ortho.hip), the host statements (icelk_ortho_coords_host,
// icelk_ortho_add_host) and tests/ortho_restatement.py (numpy, written independently) all compute what is stated here,
// byte for byte and, for the distances, bit for bit.  No libm call; the build's -ffp-contract=off keeps every product and
// sum a rounding of its own.  DESIGN.md 7.12 has the rules and what the picture is not.
//
//   raster      pixel (i, j) of a width x height raster has its centre at tx = x0 + i res, ty = y0 - j res: (x0, y0) is the
//               centre of the top-left pixel, northing decreases with the row.  i and j convert exactly; one product and
//               one sum per coordinate
//   coordinates tx' = tx - E, ty' = ty - N; a = (U2 / H) tx' - U0, b = (V2 / H) tx' - V0, c = (U2 / H) ty' - U1,
//               d = (V2 / H) ty' - V1, p = sigma (X0 - (X2 / H) tx'), q = sigma (X1 - (X2 / H) ty'), den = a d - b c,
//               xi = (d p - b q) / den, yi = ((-c) p + a q) / den, x = xi + half_w, y = yi + half_h (camtools.py:347-390),
//               xs = x - crop_left, ys = y - crop_top (camtools.py:427-428): the cropped frame's coordinates
//   seen        by a camera with a source of sw x sh samples: den != 0; w = sigma X2 + xi U2 + yi V2 is non-zero and has
//               the sign of H (photo_to_utm of the hit returns the point only then: for the mirror point behind the camera
//               H / w < 0); d2 = tx' tx' + ty' ty' <= max_range max_range when max_range > 0; 0 <= xs <= sw - 1 and
//               0 <= ys <= sh - 1 in doubles.  A NaN fails every test
//   sampling    fx = (int)floor(256 xs) (xs >= 0: the conversion truncates; 256 xs < 2^24), ix = fx >> 8, ax = fx & 255,
//               ix1 = min(ix + 1, sw - 1), the same for y.  Bilinear, per channel: ((256 - ax) (256 - ay) p00 +
//               ax (256 - ay) p10 + (256 - ax) ay p01 + ax ay p11 + 32768) >> 16 (the weights add up to 65536: at most
//               255 * 65536 + 32768 < 2^24).  Nearest: the sample at ((fx + 128) >> 8, (fy + 128) >> 8), inside the source
//               because fx <= 256 (sw - 1).  A one-channel source gives R = G = B
//   mosaic      a raster begins with every pixel the fill colour, cover = 0, best = +inf.  Adding camera `index`
//               (0 .. 254) changes a pixel iff it is seen and d2 < best (strict: of two equal distances the earlier
//               addition stays): the sample, cover = index + 1, best = d2.  The nearest camera wins
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/icelk.h"

#ifndef ICELK_ORTHO_FN
#if defined(__HIPCC__)
#define ICELK_ORTHO_FN __host__ __device__ __forceinline__
#else
#define ICELK_ORTHO_FN inline
#endif
#endif

namespace icelk {
namespace ortho {

constexpr int kMaxIndex = 254;        // cover = index + 1 fits a byte, 0 is "no camera"
constexpr int kMaxSource = 65535;     // a source's width and height: 256 xs stays below 2^24
constexpr int kTile = 16;             // k_ortho_add's workgroup is a kTile x kTile tile of the raster

struct Source {
    const uint8_t* px;   // host or device memory, as the caller's
    int w, h;            // samples
    int channels;        // 3: interleaved R G B; 1: one plane
    int64_t pitch;       // bytes between rows, >= w channels
};

struct Hit {
    double xs, ys;   // the cropped frame's coordinates
    double d2;       // squared horizontal distance from the camera
    bool seen;
};

ICELK_ORTHO_FN double infinity() { return __builtin_huge_val(); }

// ---- coordinates and seen
ICELK_ORTHO_FN Hit locate(const icelk_camera_t& C, const icelk_ortho_raster_t& R, int i, int j, int sw, int sh, double max_range)
{
    const double tx0 = R.x0 + (double)i * R.res, ty0 = R.y0 - (double)j * R.res;
    const double tx = tx0 - C.E, ty = ty0 - C.N;
    const double uh = C.U[2] / C.H, vh = C.V[2] / C.H, xh = C.X[2] / C.H;
    const double a = uh * tx - C.U[0];
    const double b = vh * tx - C.V[0];
    const double c = uh * ty - C.U[1];
    const double d = vh * ty - C.V[1];
    const double p = C.sigma * (C.X[0] - xh * tx);
    const double q = C.sigma * (C.X[1] - xh * ty);
    const double den = a * d - b * c;
    const double xi = (d * p - b * q) / den;
    const double yi = (-c * p + a * q) / den;
    Hit h;
    h.xs = (xi + C.half_w) - C.crop_left;
    h.ys = (yi + C.half_h) - C.crop_top;
    h.d2 = tx * tx + ty * ty;
    const double w = C.sigma * C.X[2] + xi * C.U[2] + yi * C.V[2];
    bool seen = den != 0.0 && ((w > 0.0 && C.H > 0.0) || (w < 0.0 && C.H < 0.0));
    if (max_range > 0.0) seen = seen && h.d2 <= max_range * max_range;
    seen = seen && h.xs >= 0.0 && h.xs <= (double)(sw - 1) && h.ys >= 0.0 && h.ys <= (double)(sh - 1);
    h.seen = seen;
    return h;
}

// ---- sampling: (xs, ys) inside [0, sw - 1] x [0, sh - 1].  Every index is inside the source: 0 <= ix <= ix1 <= sw - 1
ICELK_ORTHO_FN void sample(const Source& S, double xs, double ys, int sampling, uint8_t* out)
{
    const int fx = (int)(xs * 256.0), fy = (int)(ys * 256.0);
    const int ch = S.channels;
    if (sampling == 1) {
        const int nx = (fx + 128) >> 8, ny = (fy + 128) >> 8;
        const uint8_t* s = S.px + (int64_t)ny * S.pitch + (int64_t)nx * ch;
        out[0] = s[0];
        out[1] = ch == 3 ? s[1] : s[0];
        out[2] = ch == 3 ? s[2] : s[0];
        return;
    }
    const int ix = fx >> 8, iy = fy >> 8, ax = fx & 255, ay = fy & 255;
    const int ix1 = ix + 1 < S.w ? ix + 1 : S.w - 1, iy1 = iy + 1 < S.h ? iy + 1 : S.h - 1;
    const uint8_t *r0 = S.px + (int64_t)iy * S.pitch, *r1 = S.px + (int64_t)iy1 * S.pitch;
    const uint32_t w00 = (uint32_t)((256 - ax) * (256 - ay)), w10 = (uint32_t)(ax * (256 - ay)), w01 = (uint32_t)((256 - ax) * ay),
                   w11 = (uint32_t)(ax * ay);
    const int64_t o0 = (int64_t)ix * ch, o1 = (int64_t)ix1 * ch;
    for (int k = 0; k < ch; k++) out[k] = (uint8_t)((w00 * r0[o0 + k] + w10 * r0[o1 + k] + w01 * r1[o0 + k] + w11 * r1[o1 + k] + 32768u) >> 16);
    if (ch == 1) out[1] = out[2] = out[0];
}

// ---- mosaic: what adding a camera does to pixel (i, j) whose distance so far is `best`: false leaves the pixel alone
ICELK_ORTHO_FN bool add_pixel(const icelk_camera_t& C, const icelk_ortho_raster_t& R, const Source& S, double max_range, int sampling, int i,
                              int j, double best, uint8_t* out, double* d2)
{
    const Hit h = locate(C, R, i, j, S.w, S.h, max_range);
    if (!h.seen || !(h.d2 < best)) return false;
    sample(S, h.xs, h.ys, sampling, out);
    *d2 = h.d2;
    return true;
}

// what every call checks of its numbers.  x == x fails for a NaN, x - x != 0 for an infinity
ICELK_ORTHO_FN bool finite(double x) { return x - x == 0.0; }
ICELK_ORTHO_FN bool raster_ok(const icelk_ortho_raster_t& R)
{
    return finite(R.x0) && finite(R.y0) && finite(R.res) && R.res > 0.0 && R.width >= 1 && R.height >= 1;
}
ICELK_ORTHO_FN bool camera_ok(const icelk_camera_t& C)
{
    bool ok = finite(C.sigma) && finite(C.H) && finite(C.E) && finite(C.N) && finite(C.half_w) && finite(C.half_h) && finite(C.crop_left) &&
              finite(C.crop_top);
    for (int k = 0; k < 3; k++) ok = ok && finite(C.X[k]) && finite(C.U[k]) && finite(C.V[k]);
    return ok;
}
ICELK_ORTHO_FN bool source_ok(int sw, int sh, int channels, long long stride)
{
    return sw >= 1 && sw <= kMaxSource && sh >= 1 && sh <= kMaxSource && (channels == 1 || channels == 3) && stride >= (long long)sw * channels;
}

// ---- host only: the statement.  rgb: rows rgb_stride >= 3 width bytes apart; cover: rows cover_stride >= width bytes
// apart; best: width height doubles
inline void begin_host(const icelk_ortho_raster_t& R, const uint8_t* fill, uint8_t* rgb, size_t rgb_stride, uint8_t* cover, size_t cover_stride,
                       double* best)
{
    for (int j = 0; j < R.height; j++)
        for (int i = 0; i < R.width; i++) {
            uint8_t* o = rgb + (size_t)j * rgb_stride + 3 * (size_t)i;
            o[0] = fill[0], o[1] = fill[1], o[2] = fill[2];
            cover[(size_t)j * cover_stride + i] = 0;
            best[(size_t)j * R.width + i] = infinity();
        }
}
inline void add_host(const icelk_camera_t& C, const icelk_ortho_raster_t& R, const Source& S, double max_range, int sampling, int index,
                     uint8_t* rgb, size_t rgb_stride, uint8_t* cover, size_t cover_stride, double* best)
{
    for (int j = 0; j < R.height; j++)
        for (int i = 0; i < R.width; i++) {
            uint8_t px[3];
            double d2;
            double& b = best[(size_t)j * R.width + i];
            if (!add_pixel(C, R, S, max_range, sampling, i, j, b, px, &d2)) continue;
            uint8_t* o = rgb + (size_t)j * rgb_stride + 3 * (size_t)i;
            o[0] = px[0], o[1] = px[1], o[2] = px[2];
            cover[(size_t)j * cover_stride + i] = (uint8_t)(index + 1);
            b = d2;
        }
}

}  // namespace ortho
}  // namespace icelk
