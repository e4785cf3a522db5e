// plot_raster.h -- the arithmetic of the segment picture (s1:397-434: the segment's last gray frame, every surviving track
// as a red line of alpha 0.4, its end point as a red dot of alpha 0.6, the frame's time in a corner), as plain C++ for the
// host and the device alike.  The kernels (k_plot.hip), the host statement (icelk_plot_overlay_host, abi_plot.hip) and
// tests/plot_restatement.py (numpy, written independently) all compute what is stated here, byte for byte.  Everything
// is integer arithmetic apart from one float64 expression per coordinate, whose operations are rounded once each (no
// multiply-add can be formed from them; the library is built with -ffp-contract=off all the same), so the result does
// not depend on the order threads run in.  Matplotlib's rasteriser is not restated: DESIGN.md 7.6 lists the differences.
//
//   size         Wo = min(out_width, W), Ho = max(1, (2 Wo H + W) / (2 W))
//   background   the exact area average of the gray frame: on an axis scaled by Wo source column x covers
//                [x Wo, (x + 1) Wo) and output column i covers [i W, (i + 1) W); the weight is the integer overlap
//                (overlap), rows likewise with Ho and H; v = (sum wx wy g + W H / 2) / (W H) in 64 bits
//   coordinates  a vertex (x, y), float32 in frame pixels with pixel centres at integers, becomes
//                X = floor(((x + 0.5) Wo) / W * 256), Y likewise: units of 1/256 output pixel, output pixel p covers
//                [256 p, 256 p + 256).  A track with a vertex that is not finite or has |x| or |y| >= 2^20 is left out
//   lines        per pair of consecutive vertices: x-major when |dX| >= |dY| (nothing when dX == 0), ends named so that
//                Xa < Xb, every column c with Xa <= 256 c + 128 < Xb hits row (Ya + floor((Yb - Ya)(256 c + 128 - Xa) /
//                (Xb - Xa))) >> 8; else y-major, axes exchanged.  The range is clipped to the image before it is walked
//   dots         the pixel of the last vertex and its four edge neighbours, each if inside the image
//   compositing  n = min(lines, 31), m = min(dots, 31); per channel with red = (255, 0, 0):
//                v1 = (bg TL[n] + red (65536 - TL[n]) + 32768) >> 16, v2 = (v1 TD[m] + red (65536 - TD[m]) + 32768) >> 16,
//                TL[k] = floor(0.6^k 65536 + 0.5), TD[k] = floor(0.4^k 65536 + 0.5), made on the host (make_tables)
//   stamp        opaque (43, 140, 190), a 5 x 7 bitmap font scaled by k = max(1, Wo / 400), advance 6 k, top-left corner
//                at (3 Wo / 100, 4 Ho / 100); pixels outside the image are dropped
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ICELK_PLOT_FN __host__ __device__ __forceinline__
#else
#define ICELK_PLOT_FN inline
#endif

namespace icelk {
namespace plot {

constexpr int kMinWidth = 8;        // a narrower picture is a bad argument
constexpr int kMaxStamp = 48;       // characters
constexpr int kCountCap = 31;       // layers beyond this many change nothing (TL[24..] and TD[13..] are 0 already)
constexpr int kTable = kCountCap + 1;
constexpr int kGlyphW = 5, kGlyphH = 7, kAdvance = 6, kGlyphs = 15;
constexpr int kMaxVertices = 17;    // per track, as the segment tables hold them
constexpr int kStampR = 43, kStampG = 140, kStampB = 190;   // '#2b8cbe'

ICELK_PLOT_FN int out_width_of(int W, int out_width) { return out_width < W ? out_width : W; }
ICELK_PLOT_FN int out_height_of(int W, int H, int Wo)
{
    const int64_t v = (2 * (int64_t)Wo * H + W) / (2 * (int64_t)W);
    return v < 1 ? 1 : (int)v;
}

// ---- background: ns source cells and no output cells along one axis (no <= ns <= 65535)
ICELK_PLOT_FN int first_source(int i, int ns, int no) { return (int)(((int64_t)i * ns) / no); }
ICELK_PLOT_FN int last_source(int i, int ns, int no) { return (int)((((int64_t)i + 1) * ns - 1) / no); }
ICELK_PLOT_FN int overlap(int x, int i, int ns, int no)
{
    const int64_t a0 = (int64_t)x * no, a1 = a0 + no, b0 = (int64_t)i * ns, b1 = b0 + ns;
    const int64_t lo = a0 > b0 ? a0 : b0, hi = a1 < b1 ? a1 : b1;
    return hi > lo ? (int)(hi - lo) : 0;
}
ICELK_PLOT_FN int average(uint64_t sum, int W, int H)
{
    const uint64_t area = (uint64_t)W * (uint64_t)H;
    return (int)((sum + area / 2) / area);
}

// ---- coordinates
ICELK_PLOT_FN bool vertex_ok(float x, float y) { return fabsf(x) < 1048576.0f && fabsf(y) < 1048576.0f; }   // false for NaN
ICELK_PLOT_FN int coord(float v, int no, int ns)
{
    const double a = (double)v + 0.5;
    const double b = a * (double)no;
    const double c = b / (double)ns;
    return (int)floor(c * 256.0);   // |c * 256| <= (2^20 + 0.5) 2^8
}
ICELK_PLOT_FN int64_t floor_div(int64_t a, int64_t b)   // b > 0
{
    const int64_t q = a / b;
    return (a % b) < 0 ? q - 1 : q;
}

// ---- lines: hit(px, py) for every pixel of the pair inside the Wo x Ho image; at most max(Wo, Ho) steps
template <class Hit>
ICELK_PLOT_FN void walk_pair(int X0, int Y0, int X1, int Y1, int Wo, int Ho, Hit&& hit)
{
    const int dX = X1 - X0, dY = Y1 - Y0;
    const bool xmajor = (dX < 0 ? -dX : dX) >= (dY < 0 ? -dY : dY);
    int Ma = xmajor ? X0 : Y0, Na = xmajor ? Y0 : X0, Mb = xmajor ? X1 : Y1, Nb = xmajor ? Y1 : X1;
    if (Ma == Mb) return;
    if (Ma > Mb) {
        int t = Ma;
        Ma = Mb, Mb = t;
        t = Na, Na = Nb, Nb = t;
    }
    const int major_n = xmajor ? Wo : Ho, minor_n = xmajor ? Ho : Wo;
    int c0 = (Ma + 127) >> 8, c1 = (Mb + 127) >> 8;   // centres 256 c + 128 in [Ma, Mb)
    if (c0 < 0) c0 = 0;
    if (c1 > major_n) c1 = major_n;
    const int64_t dn = (int64_t)Nb - Na, dm = (int64_t)Mb - Ma;
    for (int c = c0; c < c1; c++) {
        const int64_t r = ((int64_t)Na + floor_div(dn * (256 * (int64_t)c + 128 - Ma), dm)) >> 8;
        if (r >= 0 && r < minor_n) hit(xmajor ? c : (int)r, xmajor ? (int)r : c);
    }
}

// ---- dots: hit(px, py) for the pixel of (X, Y) and its four edge neighbours, each if inside
template <class Hit>
ICELK_PLOT_FN void walk_dot(int X, int Y, int Wo, int Ho, Hit&& hit)
{
    const int px = X >> 8, py = Y >> 8;
    const int ox[5] = {0, -1, 1, 0, 0}, oy[5] = {0, 0, 0, -1, 1};
    for (int k = 0; k < 5; k++) {
        const int x = px + ox[k], y = py + oy[k];
        if (x >= 0 && x < Wo && y >= 0 && y < Ho) hit(x, y);
    }
}

// ---- compositing
ICELK_PLOT_FN int blend(int under, int over, uint32_t t) { return (int)(((uint32_t)under * t + (uint32_t)over * (65536u - t) + 32768u) >> 16); }
ICELK_PLOT_FN int composite(int bg, int red_c, uint32_t lines, uint32_t dots, const uint32_t* TL, const uint32_t* TD)
{
    const uint32_t n = lines < (uint32_t)kCountCap ? lines : (uint32_t)kCountCap;
    const uint32_t m = dots < (uint32_t)kCountCap ? dots : (uint32_t)kCountCap;
    return blend(blend(bg, red_c, TL[n]), red_c, TD[m]);
}

// ---- stamp
struct Stamp {
    int n;                    // characters
    uint8_t g[kMaxStamp];     // their glyphs
};
ICELK_PLOT_FN int glyph_index(int ch)
{
    if (ch >= '0' && ch <= '9') return ch - '0';
    switch (ch) {
        case '-': return 10;
        case ':': return 11;
        case '.': return 12;
        case '/': return 13;
        case ' ': return 14;
        default: return -1;
    }
}
// row r (0 = top) of glyph g: bit 4 is the leftmost pixel
ICELK_PLOT_FN uint32_t glyph_row(int g, int r)
{
    constexpr uint8_t kFont[kGlyphs][kGlyphH] = {
        {0x0e, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0e},   // '0'
        {0x04, 0x0c, 0x04, 0x04, 0x04, 0x04, 0x0e},   // '1'
        {0x0e, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1f},   // '2'
        {0x1f, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0e},   // '3'
        {0x02, 0x06, 0x0a, 0x12, 0x1f, 0x02, 0x02},   // '4'
        {0x1f, 0x10, 0x1e, 0x01, 0x01, 0x11, 0x0e},   // '5'
        {0x06, 0x08, 0x10, 0x1e, 0x11, 0x11, 0x0e},   // '6'
        {0x1f, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08},   // '7'
        {0x0e, 0x11, 0x11, 0x0e, 0x11, 0x11, 0x0e},   // '8'
        {0x0e, 0x11, 0x11, 0x0f, 0x01, 0x02, 0x0c},   // '9'
        {0x00, 0x00, 0x00, 0x1f, 0x00, 0x00, 0x00},   // '-'
        {0x00, 0x0c, 0x0c, 0x00, 0x0c, 0x0c, 0x00},   // ':'
        {0x00, 0x00, 0x00, 0x00, 0x00, 0x0c, 0x0c},   // '.'
        {0x01, 0x01, 0x02, 0x04, 0x08, 0x10, 0x10},   // '/'
        {0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00},   // ' '
    };
    return kFont[g][r];
}
ICELK_PLOT_FN bool stamp_hit(const Stamp& S, int px, int py, int Wo, int Ho)
{
    const int k = Wo / 400 > 1 ? Wo / 400 : 1;
    const int dx = px - (3 * Wo) / 100, dy = py - (4 * Ho) / 100;
    if (dx < 0 || dy < 0 || dy >= kGlyphH * k) return false;
    const int cell = dx / (kAdvance * k);
    if (cell >= S.n) return false;
    const int col = (dx - cell * kAdvance * k) / k;
    if (col >= kGlyphW) return false;
    return (glyph_row(S.g[cell], dy / k) >> (kGlyphW - 1 - col)) & 1u;
}

// the three bytes of output pixel (px, py)
ICELK_PLOT_FN void resolve_pixel(int bg, uint32_t lines, uint32_t dots, const uint32_t* TL, const uint32_t* TD, const Stamp& S, int px,
                                 int py, int Wo, int Ho, uint8_t* out)
{
    if (stamp_hit(S, px, py, Wo, Ho)) {
        out[0] = kStampR, out[1] = kStampG, out[2] = kStampB;
        return;
    }
    out[0] = (uint8_t)composite(bg, 255, lines, dots, TL, TD);
    out[1] = out[2] = (uint8_t)composite(bg, 0, lines, dots, TL, TD);
}

// ---- host only
inline void make_tables(uint32_t* TL, uint32_t* TD)
{
    for (int k = 0; k < kTable; k++) {
        TL[k] = (uint32_t)floor(pow(0.6, (double)k) * 65536.0 + 0.5);
        TD[k] = (uint32_t)floor(pow(0.4, (double)k) * 65536.0 + 0.5);
    }
}
// stamp (NULL: empty) -> glyphs; false for a character without a glyph or more than kMaxStamp of them
inline bool make_stamp(const char* text, Stamp* S)
{
    S->n = 0;
    for (int k = 0; k < kMaxStamp; k++) S->g[k] = 0;
    if (!text) return true;
    for (int k = 0; text[k]; k++) {
        const int g = glyph_index((unsigned char)text[k]);
        if (k >= kMaxStamp || g < 0) return false;
        S->g[k] = (uint8_t)g;
        S->n = k + 1;
    }
    return true;
}

}  // namespace plot
}  // namespace icelk
