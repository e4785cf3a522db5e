// thumb_raster.h -- the arithmetic of the inset photographs of the velocity map (s3:593-626 for one map, s3:788-829 for
// two): a camera's photo reduced to a thumbnail, and the thumbnail with the camera's name pasted into the map's picture --
// as plain C++ for the host and the device alike.  The kernels (k_thumb.hip), the host statements (icelk_thumb_host,
// icelk_map_overlay_insets_host) and tests/thumb_restatement.py (numpy, written independently) all compute what is stated
// here, byte for byte.  Everything is integer arithmetic.  DESIGN.md 7.8 has the rules and the differences.
//
//   size        a W x H image is fitted into a box bw x bh, proportions kept, never enlarged: Wt = min(bw, W),
//               Ht = max(1, (2 Wt H + W) / (2 W)) (the segment picture's rule); if Ht > bh then Ht = min(bh, H),
//               Wt = min(bw, max(1, (2 Ht W + H) / (2 H))).  W, H in 1 .. 65535 (a JPEG file holds no more), bw, bh in
//               1 .. 16384
//   pixels      every channel is the exact area average by plot_raster.h's overlap weights: on an axis scaled by Wt source
//               column x covers [x Wt, (x + 1) Wt) and output column i covers [i W, (i + 1) W), rows likewise with Ht and H;
//               v = (sum wx wy s + W H / 2) / (W H).  The sums: per source column the rows' sum of wy s is at most
//               H 255 < 2^24 (the wy of an output row add up to H), uint32; the columns' sum of wx times that is at most
//               W H 255 < 2^40 (the wx add up to W), uint64.  One channel gives R = G = B
//   paste       an inset is a thumbnail of w x h pixels with its top-left corner at (x0, y0), wholly inside the picture,
//               opaque; then its label in map_raster.h's glyphs at the picture's text scale, opaque black, (px, py) the
//               label's top-left corner, clipped to the picture.  Insets are drawn in array order: a later one covers
//               an earlier one, its label included
#pragma once
#include <vector>

#include "map_raster.h"

namespace icelk {
namespace thumb {

constexpr int kMaxSource = 65535;      // image width and height
constexpr int kMaxBox = 16384;
constexpr int kMaxInsets = 8;          // resident thumbnails, and insets of one picture
constexpr int kLabelLimit = 1048576;   // |label_px|, |label_py|
constexpr int kThreads = 256;          // k_jpeg_thumb's workgroup:
constexpr int kRowGroups = 4;          // ... its quarters share out the source rows of an output row,
constexpr int kChunk = 4 * (kThreads / kRowGroups);   // ... each summing 256 source columns per pass, four per lane
constexpr int kSpan = kChunk - 8;      // what a workgroup's pixels fill of a pass: the rounding of the two ends and the dword boundary take up to 5
constexpr int kMaxPer = kThreads / 3;  // ... and a lane for every channel of every pixel it makes

// ---- size: false for an image or a box outside the ranges above
ICELK_PLOT_FN bool size(int W, int H, int bw, int bh, int* tw, int* th)
{
    if (W < 1 || W > kMaxSource || H < 1 || H > kMaxSource || bw < 1 || bw > kMaxBox || bh < 1 || bh > kMaxBox) return false;
    int Wt = plot::out_width_of(W, bw), Ht = plot::out_height_of(W, H, Wt);
    if (Ht > bh) {
        Ht = bh < H ? bh : H;
        Wt = plot::out_height_of(H, W, Ht);   // the same rule with the axes exchanged
        if (Wt > bw) Wt = bw;
    }
    *tw = Wt, *th = Ht;
    return true;
}

// ---- pixels: one output pixel's channel from the rows' column sums, x = lo .. hi; column x's sum is kept in `parts` parts
// `stride` apart: col[p stride + x - base]
ICELK_PLOT_FN uint64_t row_sum(const uint32_t* col, int parts, int stride, int base, int lo, int hi, int i, int W, int Wt)
{
    uint64_t acc = 0;
    for (int x = lo; x <= hi; x++) {
        uint32_t s = 0;
        for (int p = 0; p < parts; p++) s += col[p * stride + x - base];
        acc += (uint64_t)plot::overlap(x, i, W, Wt) * s;
    }
    return acc;
}

// k_jpeg_thumb's decomposition: the output pixels of a row a workgroup makes -- as many as one pass of source columns holds,
// at most kMaxPer, the row's pixels in equal shares
ICELK_PLOT_FN int pixels_per_group(int W, int Wt)
{
    const int64_t fit = ((int64_t)kSpan * Wt) / W;
    const int per = fit < 1 ? 1 : (fit > kMaxPer ? kMaxPer : (int)fit);
    const int groups = (Wt + per - 1) / per;
    return (Wt + groups - 1) / groups;
}

// ---- paste
struct Inset {
    int x0, y0, w, h;          // the thumbnail's rectangle in the picture
    const uint8_t* px;         // its pixels, interleaved R G B, rows `pitch` bytes apart; host or device memory, as the caller's
    int pitch;
    map::Text label;
};
// the rectangle [bx0, bx1) x [by0, by1) of the picture an inset can change: thumbnail and label, clipped to the picture
ICELK_PLOT_FN void inset_box(const Inset& I, int k, int Wo, int Ho, int* bx0, int* by0, int* bx1, int* by1)
{
    int x0 = I.x0, y0 = I.y0, x1 = I.x0 + I.w, y1 = I.y0 + I.h;
    if (I.label.n > 0) {
        const int lx1 = I.label.px + I.label.n * plot::kAdvance * k, ly1 = I.label.py + plot::kGlyphH * k;   // |.| < 2^21
        if (I.label.px < x0) x0 = I.label.px;
        if (I.label.py < y0) y0 = I.label.py;
        if (lx1 > x1) x1 = lx1;
        if (ly1 > y1) y1 = ly1;
    }
    *bx0 = x0 < 0 ? 0 : x0, *by0 = y0 < 0 ? 0 : y0;
    *bx1 = x1 > Wo ? Wo : x1, *by1 = y1 > Ho ? Ho : y1;
}
// the three bytes of picture pixel (px, py) where the inset changes it: false leaves `out` alone
ICELK_PLOT_FN bool inset_pixel(const Inset& I, int k, int px, int py, uint8_t* out)
{
    if (map::text_hit(I.label, k, px, py)) {
        out[0] = out[1] = out[2] = 0;
        return true;
    }
    const int dx = px - I.x0, dy = py - I.y0;
    if (dx < 0 || dx >= I.w || dy < 0 || dy >= I.h) return false;
    const uint8_t* s = I.px + (size_t)dy * I.pitch + 3 * (size_t)dx;
    out[0] = s[0], out[1] = s[1], out[2] = s[2];
    return true;
}

// ---- host only
// an interleaved image of 1 or 3 channels -> its Wt x Ht thumbnail, R G B.  Wt <= W, Ht <= H, all >= 1, W, H <= kMaxSource
inline void reduce_host(const uint8_t* img, int W, int H, int channels, size_t stride, int Wt, int Ht, uint8_t* out, size_t out_stride)
{
    std::vector<uint32_t> col((size_t)W);
    for (int j = 0; j < Ht; j++) {
        const int y0 = plot::first_source(j, H, Ht), y1 = plot::last_source(j, H, Ht);
        for (int c = 0; c < channels; c++) {
            for (int x = 0; x < W; x++) {
                uint32_t s = 0;
                for (int y = y0; y <= y1; y++) s += (uint32_t)plot::overlap(y, j, H, Ht) * img[(size_t)y * stride + (size_t)x * channels + c];
                col[x] = s;
            }
            for (int i = 0; i < Wt; i++) {
                const uint64_t acc = row_sum(col.data(), 1, 0, 0, plot::first_source(i, W, Wt), plot::last_source(i, W, Wt), i, W, Wt);
                uint8_t* o = out + (size_t)j * out_stride + 3 * (size_t)i;
                const uint8_t v = (uint8_t)plot::average(acc, W, H);
                if (channels == 1) o[0] = o[1] = o[2] = v;
                else o[c] = v;
            }
        }
    }
}
// every inset in array order into a picture of Wo x Ho pixels
inline void paste_host(const Inset* insets, int n, int Wo, int Ho, uint8_t* rgb, size_t rgb_stride)
{
    const int k = map::text_scale(Wo);
    for (int t = 0; t < n; t++) {
        int bx0, by0, bx1, by1;
        inset_box(insets[t], k, Wo, Ho, &bx0, &by0, &bx1, &by1);
        for (int py = by0; py < by1; py++)
            for (int px = bx0; px < bx1; px++) inset_pixel(insets[t], k, px, py, rgb + (size_t)py * rgb_stride + 3 * (size_t)px);
    }
}

}  // namespace thumb
}  // namespace icelk
