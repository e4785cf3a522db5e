// jpeg_fwd.h -- the forward half of a baseline JPEG codec up to the quantised coefficients, as plain C++ for the host and
// the device alike: what Pillow's `img.save(path)` (libjpeg at its defaults: quality 75, 4:2:0, the Annex K tables) makes
// of interleaved R G B pixels before it entropy-codes them.  The entropy coder is lossless, so "save, then open" is a
// function of these coefficients alone; the reference tracks on such re-saved crops (camtools.py:64-104).
// The device kernel (k_jpeg_fwd.hip) and the host statement (icelk_jpeg_resave_coefficients_host, abi_jpeg_resave.hip)
// both run exactly the functions below.  All of it is 32-bit integer arithmetic, restated from libjpeg's published
// description (tests/jpeg_resave_restatement.py is the same in numpy, written independently, and is what Pillow's files
// are compared with).
//
// Steps, per pixel / sample / block:
//   colour      16-bit fixed-point R G B -> Y Cb Cr (luma / chroma_b / chroma_r)
//   padding     luma: edge samples repeated to the next multiple of 8 in both directions (its real blocks).
//               chroma: the full-resolution plane repeated to the right up to 16 * ceil(w / 16) columns and downwards
//               only to an EVEN number of rows, 2x2 downsampled (downsample), and then the last DOWNSAMPLED row repeated
//               to a multiple of 8.  (sample_rows says which image rows a sample of the padded grid is made of.)
//   transform   samples - 128, the "islow" forward DCT (Loeffler, Ligtenberg and Moschytz, 13-bit constants): rows first,
//               keeping 2 extra bits (fdct8<true>), then columns (fdct8<false>).  The result is 8 times the DCT.
//   quantise    |c| -> (|c| + (qv >> 1)) / qv with qv = 8 q, truncating, the sign restored: by multiply-shift (divide),
//               exact for every numerator the transform can produce
//   dummies     the luma blocks of the MCU-padded grid that hold no sample: AC 0, DC copied (dummy_source)
#pragma once
#include <stdint.h>

#define ICELK_FWD_FN __host__ __device__ __forceinline__

namespace icelk {
namespace fwd {

ICELK_FWD_FN int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
ICELK_FWD_FN int chroma_b(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
ICELK_FWD_FN int chroma_r(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// 2x2 box with the rounding bias 1, 2, 1, 2, ... along the OUTPUT columns, from 1 in every row
ICELK_FWD_FN int downsample(int a, int b, int c, int d, int out_col) { return (a + b + c + d + 1 + (out_col & 1)) >> 2; }

// The image rows behind row `qy` of the 2x2 quads of the padded grid (quad row qy = luma rows 2 qy, 2 qy + 1 = chroma
// row qy), h = image height: luma rows are clamped to the image one by one; a chroma row beyond the last one,
// ceil(h / 2) - 1, is a copy of THAT row -- made of rows h - 2 and h - 1 when h is even, not of row h - 1 twice.
struct QuadRows {
    int y0, y1;     // luma
    int c0, c1;     // chroma
};
ICELK_FWD_FN QuadRows quad_rows(int qy, int h)
{
    QuadRows q;
    q.y0 = 2 * qy < h ? 2 * qy : h - 1;
    q.y1 = 2 * qy + 1 < h ? 2 * qy + 1 : h - 1;
    const int last = (h + 1) / 2 - 1, cy = qy < last ? qy : last;
    q.c0 = 2 * cy;
    q.c1 = 2 * cy + 1 < h ? 2 * cy + 1 : h - 1;
    return q;
}

ICELK_FWD_FN int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// 8-point forward DCT of x[0..7] in place.  first: the row pass (outputs 0 and 4 shifted left by 2, the others descaled
// by 11); else the column pass (0 and 4 descaled by 2, the others by 15).  Samples are -128 .. 127: the row pass stays
// below 2^13 in magnitude, the products of the column pass below 2^29.
template <bool first>
ICELK_FWD_FN void fdct8(int (&x)[8])
{
    const int t0 = x[0] + x[7], t7 = x[0] - x[7], t1 = x[1] + x[6], t6 = x[1] - x[6];
    const int t2 = x[2] + x[5], t5 = x[2] - x[5], t3 = x[3] + x[4], t4 = x[3] - x[4];
    // even part
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = first ? 11 : 15;
    x[0] = first ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    x[4] = first ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    const int ze = (t12 + t13) * 4433;
    x[2] = descale(ze + t13 * 6270, n);
    x[6] = descale(ze - t12 * 15137, n);
    // odd part
    const int z5 = (t4 + t6 + t5 + t7) * 9633;
    const int z1 = -(t4 + t7) * 7373;
    const int z2 = -(t5 + t6) * 20995;
    const int z3 = z5 - (t4 + t6) * 16069;
    const int z4 = z5 - (t5 + t7) * 3196;
    x[7] = descale(t4 * 2446 + z1 + z3, n);
    x[5] = descale(t5 * 16819 + z2 + z4, n);
    x[3] = descale(t6 * 25172 + z2 + z3, n);
    x[1] = descale(t7 * 12299 + z1 + z4, n);
}

// Division by qv = 8 q (8 .. 2040) without a divide.  M = ceil(2^28 / qv) = (2^28 + e) / qv with 0 <= e < qv < 2^11, so
// n M / 2^28 = n / qv + n e / (qv 2^28), and the second term is below 1 / qv -- too small to carry the quotient over
// the next integer -- as long as n e < 2^28: for every n <= 2^17.  (n << 4) M >> 32 is that product's shift, as the high
// half of one 32 x 32 bit multiplication: n << 4 <= 2^21 and M <= 2^25 both fit.
ICELK_FWD_FN uint32_t reciprocal(uint32_t qv) { return ((1u << 28) + qv - 1) / qv; }
ICELK_FWD_FN uint32_t divide(uint32_t n, uint32_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(n << 4, m);
#else
    return (uint32_t)(((uint64_t)(n << 4) * m) >> 32);
#endif
}
// c: a transform output, q: the table entry, m = reciprocal(8 q)
ICELK_FWD_FN int quantise(int c, int q, uint32_t m)
{
    const uint32_t qv = (uint32_t)q << 3;
    const uint32_t a = (uint32_t)(c < 0 ? -c : c) + (qv >> 1);
    const int v = (int)divide(a, m);
    return c < 0 ? -v : v;
}

// Luma block (u, v) of an MCU (u, v in 0, 1) that holds no sample takes its DC from another block of the same MCU, in
// the encoder's block order 00 10 01 11: a block column beyond the real ones from the block to its left; a block row
// beyond the real ones -- both blocks -- from the MCU's top-right block, which may be a dummy itself (then: top-left).
// The first column and the first row of an MCU are always real.  Returns the source as u | v << 1.
ICELK_FWD_FN int dummy_source(int v, bool col1_real, bool row_real)
{
    if (!row_real) return col1_real ? 1 : 0;
    return v << 1;
}

}  // namespace fwd
}  // namespace icelk
