// jpeg_rgb.h -- the R G B of image pixel (X, Y) from a decoded file's component planes, as plain C++ for the host and the
// device alike: libjpeg's "fancy" chroma upsampling and its 16-bit fixed-point colour matrix, clamped to 8 bits -- what
// Pillow's decoder hands to whatever comes next (its encoder included: a re-save rounds to these 8-bit values first).
// The output kernel (k_jpeg_out, k_jpeg.hip), the fused crop-and-forward kernel (k_jpeg_crop_fwd, k_jpeg_fwd.hip) and the
// host statement of the latter (jpeg_crop_fwd_host.h) all run exactly the functions below; nothing else rounds a pixel.
// The two latter take their pixels four at a time through crop_row4, the crop's right-edge clamp included.
//
// The chroma sample at image position (X, Y), from a plane of cw x ch samples:
//   mode 0  no subsampling
//   mode 1  2x1 "fancy":  (3 near + neighbour + 1) >> 2 at even X (neighbour on the left), + 2 at odd X (on the right)
//   mode 2  2x2 "fancy":  column sums 3 near row + far row (above at even Y, below at odd Y), then
//           (3 s[j] + s[j-1] + 8) >> 4 at even X, (3 s[j] + s[j+1] + 7) >> 4 at odd X
//   mode 3 / 4  2x1 / 2x2 by plain replication: what libjpeg does for planes of 2 samples' width or less
// Neighbours beyond the plane's edge are the edge sample: the TRUE edge of the plane, whatever box of the image is asked for.
//
// Pixels are made four neighbours of a row at a time.  They need 4 luma samples and, in every mode, at most 4 neighbouring
// chroma samples per row: each group of 4 is ONE dword load at whatever byte address the box puts it (gfx950 under HSA
// takes unaligned vector loads).  Loaded byte by byte -- 36 loads per lane at 4:2:0 instead of 5 -- the output kernel is
// bound by the address unit: 53.8 against 26.8 us per 12 MP frame.  Groups that reach over an edge of the plane are loaded
// byte by byte with the column clamped, so no load leaves the row's n true samples.
#pragma once
#include <stdint.h>
#include <string.h>

#define ICELK_RGB_FN __host__ __device__ __forceinline__

namespace icelk {
namespace rgbpx {

// a decoded file's planes: luma of W true columns, chroma of cw x ch true samples, rows pitch[] bytes apart
struct Planes {
    const uint8_t* plane[3];
    int pitch[3];
    int W, cw, ch;
    int mode;   // chroma upsampling, as above
};

ICELK_RGB_FN int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

typedef uint32_t u32_a1 __attribute__((aligned(1)));

// v[k] = row[clamp(c + k, 0, n - 1)], k = 0..3
ICELK_RGB_FN void load4(const uint8_t* __restrict__ row, int c, int n, int (&v)[4])
{
    if (c >= 0 && c + 3 < n) {
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t w = *reinterpret_cast<const u32_a1*>(row + c);
#else
        uint32_t w;
        memcpy(&w, row + c, 4);
#endif
        v[0] = w & 255;
        v[1] = (w >> 8) & 255;
        v[2] = (w >> 16) & 255;
        v[3] = w >> 24;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = c + k < 0 ? 0 : (c + k > n - 1 ? n - 1 : c + k);
            v[k] = row[j];
        }
    }
}

// the chroma samples of image pixels X0 .. X0+3 in row Y
template <int mode>
ICELK_RGB_FN void chroma4(const uint8_t* __restrict__ p, int pitch, int cw, int ch, int X0, int Y, int (&out)[4])
{
    if (mode == 0) {
        load4(p + (size_t)Y * pitch, X0, cw, out);
        return;
    }
    const int odd = X0 & 1;
    if (mode == 3 || mode == 4) {
        int t[4];
        load4(p + (size_t)(mode == 4 ? Y >> 1 : Y) * pitch, X0 >> 1, cw, t);
#pragma unroll
        for (int i = 0; i < 4; i++) out[i] = odd ? t[(i + 1) >> 1] : t[i >> 1];
        return;
    }
    // the window of 4 samples from one left of pixel X0's own: every pixel's sample and neighbour lie inside
    const int c0 = (X0 >> 1) - 1;
    int t[4];
    if (mode == 1) {
        load4(p + (size_t)Y * pitch, c0, cw, t);
    } else {
        const int i = Y >> 1;
        const int fi = (Y & 1) ? (i + 1 < ch - 1 ? i + 1 : ch - 1) : (i - 1 > 0 ? i - 1 : 0);
        int f[4];
        load4(p + (size_t)i * pitch, c0, cw, t);
        load4(p + (size_t)fi * pitch, c0, cw, f);
#pragma unroll
        for (int k = 0; k < 4; k++) t[k] = 3 * t[k] + f[k];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        // window index of the pixel's own sample and of its neighbour, for even and for odd X0
        const int je = 1 + (i >> 1), jo = 1 + ((i + 1) >> 1);
        const int ne = (i & 1) ? je + 1 : je - 1, no = ((i + 1) & 1) ? jo + 1 : jo - 1;
        const int own = odd ? t[jo] : t[je], nb = odd ? t[no] : t[ne];
        const int xodd = (i + odd) & 1;
        out[i] = mode == 1 ? (3 * own + nb + 1 + xodd) >> 2 : (3 * own + nb + 8 - xodd) >> 4;
    }
}

struct Rgb {
    int r, g, b;
};

// the 16-bit colour matrix, clamped
ICELK_RGB_FN Rgb colour(int lum, int cb, int cr)
{
    const int u = cb - 128, v = cr - 128;
    Rgb c;
    c.r = clamp255(lum + ((91881 * v + 32768) >> 16));
    c.g = clamp255(lum + ((-22554 * u - 46802 * v + 32768) >> 16));
    c.b = clamp255(lum + ((116130 * u + 32768) >> 16));
    return c;
}

// the R G B of image pixels X0 .. X0+3 in row Y (columns beyond the image repeat its last one: callers use what they asked for)
template <int mode>
ICELK_RGB_FN void rgb4(const Planes& P, int X0, int Y, Rgb (&px)[4])
{
    int lum[4], cb[4], cr[4];
    load4(P.plane[0] + (size_t)Y * P.pitch[0], X0, P.W, lum);
    chroma4<mode>(P.plane[1], P.pitch[1], P.cw, P.ch, X0, Y, cb);
    chroma4<mode>(P.plane[2], P.pitch[2], P.cw, P.ch, X0, Y, cr);
#pragma unroll
    for (int i = 0; i < 4; i++) px[i] = colour(lum[i], cb[i], cr[i]);
}

// The pixels at columns x0 .. x0 + 3 of row `row` of a CROP of the image -- w pixels wide, its pixel (0, 0) image pixel
// (left, top) -- the column clamped to the crop's last one (the right-edge padding of a re-save, in crop coordinates).  One
// rgb4 either way: where the four do not all lie inside the crop it is taken at the crop's last four columns and the
// clamped columns are picked from it by shifts (an indexed pick would go to scratch on the device).  A 3-wide crop picks
// from columns 0 .. 2 of the four; the fourth is computed and never picked.
// Read set, all of it inside the planes' true samples: with X = left + (x0 + 3 < w ? x0 : max(w - 4, 0)), luma row
// top + row at columns X .. X + 3 clamped to W - 1 (columns of the crop, left .. left + w - 1; only a 3-wide crop reaches
// one column past it, left + 3, which is used for nothing); chroma at the window chroma4 names for X -- mode 0:
// columns X .. X + 3; modes 3 / 4: samples X / 2 .. X / 2 + 3; modes 1 / 2: samples X / 2 - 1 .. X / 2 + 2, in mode 2 of
// the near row (top + row) / 2 and the far row one above or below it -- every index clamped to 0 .. cw - 1 and 0 .. ch - 1.
template <int mode>
ICELK_RGB_FN void crop_row4(const Planes& P, int left, int top, int w, int x0, int row, Rgb (&px)[4])
{
    const bool inside = x0 + 3 < w;
    const int from = inside ? x0 : (w > 4 ? w - 4 : 0);
    rgb4<mode>(P, from + left, row + top, px);
    if (!inside) {
        // the four pixels' channels in one word each: a pick is a shift, not an indexed register
        uint32_t r = 0, g = 0, b = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            r |= (uint32_t)px[j].r << (8 * j);
            g |= (uint32_t)px[j].g << (8 * j);
            b |= (uint32_t)px[j].b << (8 * j);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int col = x0 + j < w - 1 ? x0 + j : w - 1;
            const int sh = 8 * (col - from);   // pixel 0 .. 3 of the four
            px[j].r = (int)((r >> sh) & 255u);
            px[j].g = (int)((g >> sh) & 255u);
            px[j].b = (int)((b >> sh) & 255u);
        }
    }
}

// the same with the mode taken at run time (host statement)
ICELK_RGB_FN void crop_row4_any(const Planes& P, int left, int top, int w, int x0, int row, Rgb (&px)[4])
{
    switch (P.mode) {
    case 0: crop_row4<0>(P, left, top, w, x0, row, px); break;
    case 1: crop_row4<1>(P, left, top, w, x0, row, px); break;
    case 2: crop_row4<2>(P, left, top, w, x0, row, px); break;
    case 3: crop_row4<3>(P, left, top, w, x0, row, px); break;
    default: crop_row4<4>(P, left, top, w, x0, row, px); break;
    }
}

}  // namespace rgbpx
}  // namespace icelk
