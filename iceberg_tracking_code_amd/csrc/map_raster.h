// map_raster.h -- the arithmetic of the velocity map of a gridded window (s3:449-465, plot_velocities_one_map s3:471-641,
// plot_velocities_two_maps s3:644-844: the grid with its unmeasured cells filled, one arrow per measured cell coloured by
// speed, with plot_switch 2 a second panel with every velocity vector of the window, the fjord's outline, the cameras, four
// strings and a colour bar), as plain C++ for the host and the device alike.  The kernels (k_map.hip), the host statement
// (icelk_map_overlay_host, abi_map.hip) and tests/map_restatement.py (numpy, written independently) all compute what is
// stated here, byte for byte.  Everything is integer arithmetic apart from the float64 expressions named below, whose
// operations are rounded once each (the library is built with -ffp-contract=off; sqrt and division are correctly rounded
// on both sides), and every plane is filled with integer atomics whose result does not depend on the order of arrival.
// Matplotlib's rasteriser is not restated: DESIGN.md 7.7 lists the differences.
//
//   views        a view is a rectangle (x0, y0, w, h) of the picture with world limits xmin < xmax, ymin < ymax; a picture
//                has one or two.  The layout is the host's (velocity_map.map_layout); the rules only see rectangles
//   coordinates  cx = ((x - xmin) w) / (xmax - xmin), cy = ((ymax - y) h) / (ymax - ymin) in float64; X = floor(cx 256),
//                Y = floor(cy 256): units of 1/256 pixel relative to the view's corner, pixel p covers [256 p, 256 p + 256).
//                An item with a cx or cy that is not finite or has |c| >= 2^20 is left out whole.  Everything a view draws
//                is clipped to its rectangle
//   base layer   a uint32 plane, atomicMax of a code: 1 the interior of an unmeasured cell (211, 211, 211), 2 a cell's
//                edge (169, 169, 169), 3 the outline (0, 0, 0); 0 is white.  A cell (left, top, size) has the corners
//                (X0, Y0) of (left, top) and (X1, Y1) of (left + size, top - size); its interior are the pixels with
//                X0 <= 256 p + 128 < X1 and Y0 <= 256 q + 128 < Y1; its edges are the four sides through walk_pair; the
//                outline is walk_pair per pair of consecutive vertices
//   arrows       (x, y, dx, dy, speed) float64 and a pivot.  Left out when speed is negative or not finite.  tail = (x, y)
//                (pivot tail) or (x - dx 0.5, y - dy 0.5) (pivot middle), tip = tail + (dx, dy); position, tail and tip go
//                through the coordinate rule.  (dX, dY) = tip - tail in fixed units, L = sqrt(dX dX + dY dY) in float64.
//                L < 256: the one pixel of the position.  Else hl = min(5 w, L, 48 * 256) with the arrow's width
//                w = max(256, floor(((width vw) / (xmax - xmin)) 256)); u = (dX / L, dY / L); the head's base centre
//                b = tip - hl u; hb = (3 hl) / 10; the head is the triangle tip, floor(b + hb (-uy, ux)),
//                floor(b - hb (-uy, ux)): a pixel is in it when its centre (256 p + 128, 256 q + 128) has all three
//                64-bit edge functions >= 0 on the positively oriented triangle (zero area: nothing), the bounding box
//                clipped to the view before it is walked.  The shaft is walk_pair from the tail to floor(b), thickened to
//                t = clamp((w + 128) >> 8, 1, 7) pixels along the minor axis: the line is moved by -(t - 1) 128 along that
//                axis and every step marks its pixel and the t - 1 after it.  One arrow takes at most
//                7 max(vw, vh) + 97^2 hits whatever its numbers
//   overlap      every hit does atomicMax(top, index + 1) and atomicAdd(count, 1): a pixel has the colour of its
//                highest-indexed arrow (the reference's painter's order) and the transparency T[min(count, 31)],
//                T[k] = floor((1 - alpha)^k 65536 + 0.5) made on the host; v = (under T + over (65536 - T) + 32768) >> 16
//   colour       idx = min(255, floor((speed / vmax) 256)) into a table of 256 x 3 bytes the caller passes
//   resolve      per pixel, in this order: base colour; the arrow blended over it; the cameras of its view as opaque red
//                discs ((256 p + 128 - X)^2 + (256 q + 128 - Y)^2 <= (256 r)^2, r = max(2, 3 Wo / 1000)); the colour bars
//                (index 255 - (255 row) / (h - 1) down the strip, a one-pixel black frame); the texts, opaque black
//   text         at most 16 items (px, py, <= 48 characters): the 5 x 7 glyphs of plot_raster.h plus A-Z (a lower-case
//                letter takes its capital's glyph) , ( ) from the table below, scaled by k = max(1, Wo / 400), advance 6 k,
//                (px, py) the top-left corner; pixels outside the picture are dropped
#pragma once
#include "plot_raster.h"

namespace icelk {
namespace map {

constexpr int kMinWidth = 64;
constexpr int kMaxSide = 16384;        // picture width and height
constexpr int kMaxViews = 2;
constexpr int kMaxCameras = 8;         // per view
constexpr int kMaxTexts = 16;
constexpr int kMaxChars = 48;
constexpr int kCountCap = 31;
constexpr int kTable = kCountCap + 1;
constexpr int kOwnGlyphs = 29;         // A-Z , ( )
constexpr int kGlyphs = plot::kGlyphs + kOwnGlyphs;
constexpr int kMaxHead = 48 * 256;     // fixed units
constexpr int kMaxThick = 7;           // pixels
constexpr int kHeadBox = 97;           // the head's clipped bounding box has at most this many pixels a side
constexpr double kLimit = 1048576.0;   // pixels

struct View {
    int x0, y0, w, h;          // in the picture
    int bar_x0, bar_w;         // the colour bar: columns [bar_x0, bar_x0 + bar_w) of the view's rows; bar_w == 0: none
    double xmin, xmax, ymin, ymax;
};

// ---- coordinates
ICELK_PLOT_FN bool to_fixed(const View& V, double x, double y, int* X, int* Y)
{
    const double ax = x - V.xmin, bx = ax * (double)V.w, cx = bx / (V.xmax - V.xmin);
    const double ay = V.ymax - y, by = ay * (double)V.h, cy = by / (V.ymax - V.ymin);
    if (!(fabs(cx) < kLimit) || !(fabs(cy) < kLimit)) return false;   // NaN fails both
    *X = (int)floor(cx * 256.0);
    *Y = (int)floor(cy * 256.0);
    return true;
}
ICELK_PLOT_FN int arrow_width(const View& V, double width)   // fixed units; a width the caller has checked: finite, > 0
{
    const double a = width * (double)V.w, b = a / (V.xmax - V.xmin), c = floor(b * 256.0);
    return c >= 268435456.0 ? 268435456 : (c > 256.0 ? (int)c : 256);
}
ICELK_PLOT_FN int shaft_thickness(int w)
{
    const int t = (int)(((int64_t)w + 128) >> 8);
    return t < 1 ? 1 : (t > kMaxThick ? kMaxThick : t);
}

// ---- base layer: fill(p, q) / edge(p, q) for the pixels of a cell inside the view
template <class Fill, class Edge>
ICELK_PLOT_FN void walk_cell(const View& V, double left, double top, double size, bool measured, Fill&& fill, Edge&& edge)
{
    int X0, Y0, X1, Y1;
    if (!to_fixed(V, left, top, &X0, &Y0) || !to_fixed(V, left + size, top - size, &X1, &Y1)) return;
    if (!measured) {
        int p0 = (X0 + 127) >> 8, p1 = (X1 + 127) >> 8, q0 = (Y0 + 127) >> 8, q1 = (Y1 + 127) >> 8;
        if (p0 < 0) p0 = 0;
        if (q0 < 0) q0 = 0;
        if (p1 > V.w) p1 = V.w;
        if (q1 > V.h) q1 = V.h;
        for (int q = q0; q < q1; q++)
            for (int p = p0; p < p1; p++) fill(p, q);
    }
    plot::walk_pair(X0, Y0, X1, Y0, V.w, V.h, edge);
    plot::walk_pair(X0, Y1, X1, Y1, V.w, V.h, edge);
    plot::walk_pair(X0, Y0, X0, Y1, V.w, V.h, edge);
    plot::walk_pair(X1, Y0, X1, Y1, V.w, V.h, edge);
}

template <class Hit>
ICELK_PLOT_FN void walk_segment(const View& V, double xa, double ya, double xb, double yb, Hit&& hit)
{
    int X0, Y0, X1, Y1;
    if (!to_fixed(V, xa, ya, &X0, &Y0) || !to_fixed(V, xb, yb, &X1, &Y1)) return;
    plot::walk_pair(X0, Y0, X1, Y1, V.w, V.h, hit);
}

// ---- arrows
// a step of the moved line, walked in a view kMaxThick pixels larger along the minor axis: the step's pixel and the t - 1 after it
template <class Hit>
struct ThickStep {
    Hit& hit;
    int t, minor_n;
    bool xmajor;
    ICELK_PLOT_FN void operator()(int px, int py) const
    {
        const int major = xmajor ? px : py, first = (xmajor ? py : px) - kMaxThick;
        for (int k = 0; k < t; k++) {
            const int m = first + k;
            if (m >= 0 && m < minor_n) hit(xmajor ? major : m, xmajor ? m : major);
        }
    }
};
ICELK_PLOT_FN int64_t edge_fn(int ax, int ay, int bx, int by, int64_t px, int64_t py)
{
    return ((int64_t)bx - ax) * (py - ay) - ((int64_t)by - ay) * (px - ax);
}
ICELK_PLOT_FN bool speed_ok(double speed) { return speed >= 0.0 && speed < HUGE_VAL; }   // false for NaN

// hit(p, q) for every pixel of the arrow inside the view; w: arrow_width, pivot_mid: the pivot is the middle
template <class Hit>
ICELK_PLOT_FN void walk_arrow(const View& V, int w, bool pivot_mid, double x, double y, double dx, double dy, double speed, Hit&& hit)
{
    if (!speed_ok(speed)) return;
    double tx = x, ty = y;
    if (pivot_mid) {
        tx = x - dx * 0.5;
        ty = y - dy * 0.5;
    }
    const double hx = tx + dx, hy = ty + dy;
    int Xp, Yp, Xt, Yt, Xh, Yh;
    if (!to_fixed(V, x, y, &Xp, &Yp) || !to_fixed(V, tx, ty, &Xt, &Yt) || !to_fixed(V, hx, hy, &Xh, &Yh)) return;
    const double fx = (double)(Xh - Xt), fy = (double)(Yh - Yt);   // |.| < 2^29 + 1: exact
    const double L = sqrt(fx * fx + fy * fy);
    if (L < 256.0) {
        const int p = Xp >> 8, q = Yp >> 8;
        if (p >= 0 && p < V.w && q >= 0 && q < V.h) hit(p, q);
        return;
    }
    double hl = 5.0 * (double)w;
    if (L < hl) hl = L;
    if ((double)kMaxHead < hl) hl = (double)kMaxHead;
    const double ux = fx / L, uy = fy / L;
    const double bx = (double)Xh - hl * ux, by = (double)Yh - hl * uy;
    const double hb = (3.0 * hl) / 10.0;
    const int Sx = (int)floor(bx), Sy = (int)floor(by);
    int Ax = (int)floor(bx - hb * uy), Ay = (int)floor(by + hb * ux);
    int Bx = (int)floor(bx + hb * uy), By = (int)floor(by - hb * ux);
    // the shaft
    {
        const int t = shaft_thickness(w), shift = kMaxThick * 256 - (t - 1) * 128;
        const int sx = Sx - Xt, sy = Sy - Yt;
        const bool xmajor = (sx < 0 ? -sx : sx) >= (sy < 0 ? -sy : sy);
        ThickStep<Hit> step{hit, t, xmajor ? V.h : V.w, xmajor};
        if (xmajor)
            plot::walk_pair(Xt, Yt + shift, Sx, Sy + shift, V.w, V.h + kMaxThick, step);
        else
            plot::walk_pair(Xt + shift, Yt, Sx + shift, Sy, V.w + kMaxThick, V.h, step);
    }
    // the head
    int64_t area2 = edge_fn(Xh, Yh, Ax, Ay, Bx, By);
    if (area2 == 0) return;
    if (area2 < 0) {
        int s = Ax;
        Ax = Bx, Bx = s;
        s = Ay, Ay = By, By = s;
    }
    int lox = Xh < Ax ? Xh : Ax, hix = Xh > Ax ? Xh : Ax, loy = Yh < Ay ? Yh : Ay, hiy = Yh > Ay ? Yh : Ay;
    if (Bx < lox) lox = Bx;
    if (Bx > hix) hix = Bx;
    if (By < loy) loy = By;
    if (By > hiy) hiy = By;
    int p0 = lox >> 8, p1 = hix >> 8, q0 = loy >> 8, q1 = hiy >> 8;
    if (p0 < 0) p0 = 0;
    if (q0 < 0) q0 = 0;
    if (p1 > V.w - 1) p1 = V.w - 1;
    if (q1 > V.h - 1) q1 = V.h - 1;
    if (p1 - p0 >= kHeadBox) p1 = p0 + kHeadBox - 1;   // never taken: the head is at most 48 pixels long
    if (q1 - q0 >= kHeadBox) q1 = q0 + kHeadBox - 1;
    for (int q = q0; q <= q1; q++)
        for (int p = p0; p <= p1; p++) {
            const int64_t cx = 256 * (int64_t)p + 128, cy = 256 * (int64_t)q + 128;
            if (edge_fn(Xh, Yh, Ax, Ay, cx, cy) >= 0 && edge_fn(Ax, Ay, Bx, By, cx, cy) >= 0 && edge_fn(Bx, By, Xh, Yh, cx, cy) >= 0) hit(p, q);
        }
}

// ---- colour
ICELK_PLOT_FN int colour_index(double speed, double vmax)
{
    const double a = speed / vmax, v = floor(a * 256.0);
    return v >= 255.0 ? 255 : (int)v;   // speed >= 0
}

// ---- text
ICELK_PLOT_FN int glyph_index(int ch)
{
    if (ch >= 'a' && ch <= 'z') ch -= 'a' - 'A';
    if (ch >= 'A' && ch <= 'Z') return plot::kGlyphs + ch - 'A';
    switch (ch) {
        case ',': return plot::kGlyphs + 26;
        case '(': return plot::kGlyphs + 27;
        case ')': return plot::kGlyphs + 28;
        default: return plot::glyph_index(ch);
    }
}
ICELK_PLOT_FN uint32_t glyph_row(int g, int r)
{
    constexpr uint8_t kFont[kOwnGlyphs][plot::kGlyphH] = {
        {0x0e, 0x11, 0x11, 0x1f, 0x11, 0x11, 0x11},   // 'A'
        {0x1e, 0x11, 0x11, 0x1e, 0x11, 0x11, 0x1e},   // 'B'
        {0x0e, 0x11, 0x10, 0x10, 0x10, 0x11, 0x0e},   // 'C'
        {0x1e, 0x11, 0x11, 0x11, 0x11, 0x11, 0x1e},   // 'D'
        {0x1f, 0x10, 0x10, 0x1e, 0x10, 0x10, 0x1f},   // 'E'
        {0x1f, 0x10, 0x10, 0x1e, 0x10, 0x10, 0x10},   // 'F'
        {0x0e, 0x11, 0x10, 0x17, 0x11, 0x11, 0x0f},   // 'G'
        {0x11, 0x11, 0x11, 0x1f, 0x11, 0x11, 0x11},   // 'H'
        {0x0e, 0x04, 0x04, 0x04, 0x04, 0x04, 0x0e},   // 'I'
        {0x07, 0x02, 0x02, 0x02, 0x02, 0x12, 0x0c},   // 'J'
        {0x11, 0x12, 0x14, 0x18, 0x14, 0x12, 0x11},   // 'K'
        {0x10, 0x10, 0x10, 0x10, 0x10, 0x10, 0x1f},   // 'L'
        {0x11, 0x1b, 0x15, 0x15, 0x11, 0x11, 0x11},   // 'M'
        {0x11, 0x11, 0x19, 0x15, 0x13, 0x11, 0x11},   // 'N'
        {0x0e, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0e},   // 'O'
        {0x1e, 0x11, 0x11, 0x1e, 0x10, 0x10, 0x10},   // 'P'
        {0x0e, 0x11, 0x11, 0x11, 0x15, 0x12, 0x0d},   // 'Q'
        {0x1e, 0x11, 0x11, 0x1e, 0x14, 0x12, 0x11},   // 'R'
        {0x0f, 0x10, 0x10, 0x0e, 0x01, 0x01, 0x1e},   // 'S'
        {0x1f, 0x04, 0x04, 0x04, 0x04, 0x04, 0x04},   // 'T'
        {0x11, 0x11, 0x11, 0x11, 0x11, 0x11, 0x0e},   // 'U'
        {0x11, 0x11, 0x11, 0x11, 0x11, 0x0a, 0x04},   // 'V'
        {0x11, 0x11, 0x11, 0x15, 0x15, 0x15, 0x0a},   // 'W'
        {0x11, 0x11, 0x0a, 0x04, 0x0a, 0x11, 0x11},   // 'X'
        {0x11, 0x11, 0x11, 0x0a, 0x04, 0x04, 0x04},   // 'Y'
        {0x1f, 0x01, 0x02, 0x04, 0x08, 0x10, 0x1f},   // 'Z'
        {0x00, 0x00, 0x00, 0x00, 0x0c, 0x04, 0x08},   // ','
        {0x02, 0x04, 0x08, 0x08, 0x08, 0x04, 0x02},   // '('
        {0x08, 0x04, 0x02, 0x02, 0x02, 0x04, 0x08},   // ')'
    };
    return g < plot::kGlyphs ? plot::glyph_row(g, r) : kFont[g - plot::kGlyphs][r];
}

struct Text {
    int px, py, n;               // top-left corner, characters
    uint8_t g[kMaxChars];        // their glyphs
};
ICELK_PLOT_FN bool text_hit(const Text& S, int k, int px, int py)
{
    const int dx = px - S.px, dy = py - S.py;
    if (dy < 0 || dy >= plot::kGlyphH * k || dx < 0) return false;
    const int cell = dx / (plot::kAdvance * k);
    if (cell >= S.n) return false;
    const int col = (dx - cell * plot::kAdvance * k) / k;
    if (col >= plot::kGlyphW) return false;
    return (glyph_row(S.g[cell], dy / k) >> (plot::kGlyphW - 1 - col)) & 1u;
}

// ---- resolve
struct Panel {
    View V;
    const double* arrows;        // (n, 5): what `top` indexes (speed at 5 i + 4); host or device memory, as the caller's
    double vmax;
    int n_cameras;
    int cam_x[kMaxCameras], cam_y[kMaxCameras];   // fixed units, relative to the view
    uint32_t T[kTable];          // transparency by hit count
};
struct Scene {
    int Wo, Ho, n_views, n_texts;
    Panel P[kMaxViews];
    Text text[kMaxTexts];
    uint8_t table[768];
};

ICELK_PLOT_FN int text_scale(int Wo) { return Wo / 400 > 1 ? Wo / 400 : 1; }
ICELK_PLOT_FN int camera_radius(int Wo) { return (3 * Wo) / 1000 > 2 ? (3 * Wo) / 1000 : 2; }

// the three bytes of picture pixel (px, py)
ICELK_PLOT_FN void resolve_pixel(const Scene& S, uint32_t base, uint32_t top, uint32_t count, int px, int py, uint8_t* out)
{
    const int k = text_scale(S.Wo);
    for (int n = 0; n < S.n_texts; n++)
        if (text_hit(S.text[n], k, px, py)) {
            out[0] = out[1] = out[2] = 0;
            return;
        }
    for (int v = 0; v < S.n_views; v++) {
        const View& V = S.P[v].V;
        if (V.bar_w > 0 && px >= V.bar_x0 && px < V.bar_x0 + V.bar_w && py >= V.y0 && py < V.y0 + V.h) {
            if (px == V.bar_x0 || px == V.bar_x0 + V.bar_w - 1 || py == V.y0 || py == V.y0 + V.h - 1) {
                out[0] = out[1] = out[2] = 0;
            } else {
                const int idx = V.h > 1 ? 255 - (255 * (py - V.y0)) / (V.h - 1) : 255;
                out[0] = S.table[3 * idx], out[1] = S.table[3 * idx + 1], out[2] = S.table[3 * idx + 2];
            }
            return;
        }
    }
    const int g = base == 0 ? 255 : (base == 1 ? 211 : (base == 2 ? 169 : 0));
    out[0] = out[1] = out[2] = (uint8_t)g;
    for (int v = 0; v < S.n_views; v++) {
        const Panel& P = S.P[v];
        const int p = px - P.V.x0, q = py - P.V.y0;
        if (p < 0 || p >= P.V.w || q < 0 || q >= P.V.h) continue;
        const int64_t R = 256 * (int64_t)camera_radius(S.Wo);
        for (int c = 0; c < P.n_cameras; c++) {
            const int64_t ex = 256 * (int64_t)p + 128 - P.cam_x[c], ey = 256 * (int64_t)q + 128 - P.cam_y[c];
            if (ex * ex + ey * ey <= R * R) {
                out[0] = 255, out[1] = out[2] = 0;
                return;
            }
        }
        if (top > 0) {
            const int idx = colour_index(P.arrows[5 * (size_t)(top - 1) + 4], P.vmax);
            const uint32_t t = P.T[count < (uint32_t)kCountCap ? count : (uint32_t)kCountCap];
            for (int c = 0; c < 3; c++) out[c] = (uint8_t)plot::blend(g, S.table[3 * idx + c], t);
        }
        return;
    }
}

// ---- host only
inline void make_table(double alpha, uint32_t* T)
{
    for (int k = 0; k < kTable; k++) T[k] = (uint32_t)floor(pow(1.0 - alpha, (double)k) * 65536.0 + 0.5);
}
// text (n_max + 1 bytes may be read) -> glyphs; false for a character without a glyph or more than kMaxChars of them
inline bool make_text(const char* s, int px, int py, Text* S)
{
    S->px = px, S->py = py, S->n = 0;
    for (int k = 0; k < kMaxChars; k++) S->g[k] = 0;
    for (int k = 0; k <= kMaxChars; k++) {
        if (!s[k]) return true;
        const int g = glyph_index((unsigned char)s[k]);
        if (k >= kMaxChars || g < 0) return false;
        S->g[k] = (uint8_t)g;
        S->n = k + 1;
    }
    return false;
}

}  // namespace map
}  // namespace icelk
