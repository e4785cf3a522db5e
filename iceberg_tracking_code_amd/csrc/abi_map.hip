// abi_map.hip -- the map the reference draws of every gridded window (s3:449-465, plot_switch 1 and 2): the grid, an arrow
// per measured cell coloured by speed, with switch 2 every velocity vector of the window in a second panel, the outline, the
// cameras, four strings and a colour bar -- rasterised on the device and handed to the picture writer that is there as well.
//
//   host    icelk_map_glyph, icelk_map_overlay_host: map_raster.h on the CPU; no handle, re-entrant.
//           icelk_map_overlay_insets_host: the same, then thumb_raster.h's paste
//   device  icelk_map_arrows_set / _release (a day's vectors, resident like the s4 cube) and icelk_map_draw.  On the handle's
//           compute stream (draw_picture): k_picture_clear, then per panel k_map_cells, k_map_polyline, k_map_arrows, then
//           k_map_resolve (k_map.hip), from planes of the map's own (Ctx::Map) into the picture writer's R G B; the file,
//           the optional R G B output, the wait for the device and ICELK_ECAP are the writer's (abi_picture.hip:
//           picture_check, picture_grow, picture_write)
//           icelk_map_draw_insets: the same with one k_map_inset (k_thumb.hip) per inset behind k_map_resolve, from the
//           resident thumbnails of abi_thumb.hip, whose header states that kernel's bounds
//           icelk_map_draw_png: the same drawing with or without insets, and the writer is asked for a PNG: the quality
//           is ignored
//
// Bounds, store by store.  Everything is sized from the picture (Wo x Ho, px = Wo Ho padded to four pixels) and the
// descriptor's counts before anything is enqueued, and check_desc has refused every view that is not inside the picture.
//   k_picture_clear 16-byte stores k < 3 px / 4 into the 3 px words of d_planes
//   k_map_cells     atomicMax into base = d_planes[0 .. px): walk_cell clips the fill's rectangle to [0, vw) x [0, vh) and
//   k_map_polyline  walk_pair clips the range it walks to the view and tests the other coordinate of every hit, whatever the
//                   numbers hold (items with a coordinate that is not finite or beyond 2^20 pixels never get that far); the
//                   hit adds the view's corner: (y0 + q) Wo + x0 + p < Wo Ho because x0 + vw <= Wo and y0 + vh <= Ho.
//                   Reads: cells[3 t ..], measured[t] for t < n_cells; xy[2 t .. 2 t + 3] for t + 1 < n_outline
//   k_map_arrows    atomicMax into top = d_planes[px .. 2 px) and atomicAdd into count = d_planes[2 px .. 3 px) at the same
//                   offset rule: the shaft's steps are walk_pair's in a view enlarged by 7 along the minor axis and
//                   ThickStep tests every pixel it marks against the view itself; the head's box is clipped to the view
//                   before it is walked; the short arrow's one pixel is tested.  Reads: arrows[5 t .. 5 t + 4], group[t] for
//                   t < n, the buffer's n
//   k_map_resolve   reads the three planes at 4-pixel steps below px (padded), the scene, and arrows[5 (top - 1) + 4] with
//                   top <= the panel's n (only k_map_arrows of that panel wrote top inside its view, and the views of two
//                   panels do not overlap: check_desc); stores 12 bytes per four pixels below 3 Wo Ho, the tail byte by byte
#include <memory>
#include <new>
#include <vector>

#include "icelk_ctx.h"

namespace icelk {

void map_destroy(Ctx* c)
{
    Ctx::Map& M = c->map;
    void* p[] = {M.d_planes, M.d_items, M.d_measured, M.d_scene, M.d_arrows, M.d_group};
    for (void* q : p)
        if (q) hipFree(q);
    delete M.h_scene;
    map_insets_free(c);
    M = Ctx::Map{};
}

namespace {

constexpr int kMaxArrows = 1 << 27;
constexpr int kMaxItems = 1 << 24;   // cells, outline vertices

bool finite(double v) { return v > -HUGE_VAL && v < HUGE_VAL; }

map::View view_of(const icelk_map_panel_t& p)
{
    return map::View{p.x0, p.y0, p.w, p.h, p.bar_x0, p.bar_w, p.xmin, p.xmax, p.ymin, p.ymax};
}

bool overlap(int a0, int an, int b0, int bn) { return a0 < b0 + bn && b0 < a0 + an; }

// what needs no handle.  nullptr: fine.  The scene's texts are made on the way
const char* check_desc(const icelk_map_desc_t* d, map::Scene* S)
{
    if (!d) return "null descriptor";
    if (d->width < map::kMinWidth || d->width > map::kMaxSide || d->height < 1 || d->height > map::kMaxSide)
        return "a picture less than 64 pixels wide, or a side outside 1 .. 16384";
    if (d->n_panels < 1 || d->n_panels > map::kMaxViews) return "panels outside 1 .. 2";
    if (!d->table) return "null colour table";
    for (int k = 0; k < d->n_panels; k++) {
        const icelk_map_panel_t& p = d->panel[k];
        if (p.w < 1 || p.h < 1 || p.x0 < 0 || p.y0 < 0 || p.x0 > d->width - p.w || p.y0 > d->height - p.h) return "a view that is not inside the picture";
        if (p.bar_w < 0 || (p.bar_w > 0 && (p.bar_x0 < 0 || p.bar_x0 > d->width - p.bar_w))) return "a colour bar that is not inside the picture";
        if (!finite(p.xmin) || !finite(p.xmax) || !finite(p.ymin) || !finite(p.ymax) || !(p.xmin < p.xmax) || !(p.ymin < p.ymax))
            return "world limits that are not finite and increasing";
        if (p.n_cells < 0 || p.n_cells > kMaxItems || (p.n_cells > 0 && (!p.cells || !p.measured))) return "cells: a count outside 0 .. 2^24 or a null array";
        if (p.n_outline < 0 || p.n_outline > kMaxItems || (p.n_outline > 0 && !p.outline)) return "outline: a count outside 0 .. 2^24 or a null array";
        if (!p.resident && (p.n_arrows < 0 || p.n_arrows > kMaxArrows || (p.n_arrows > 0 && !p.arrows)))
            return "arrows: a count outside 0 .. 2^27 or a null array";
        if (p.n_cameras < 0 || p.n_cameras > map::kMaxCameras || (p.n_cameras > 0 && !p.cameras)) return "more than 8 cameras, or a null array";
        if (p.pivot != 0 && p.pivot != 1) return "a pivot other than 0 (tail) and 1 (middle)";
        if (!finite(p.width) || !(p.width > 0) || !(p.alpha > 0) || !(p.alpha <= 1) || !finite(p.vmax) || !(p.vmax > 0))
            return "a width or vmax that is not finite and positive, or an alpha outside (0, 1]";
        for (int j = 0; j < k; j++) {
            const icelk_map_panel_t& o = d->panel[j];
            if (overlap(p.x0, p.w, o.x0, o.w) && overlap(p.y0, p.h, o.y0, o.h)) return "views that overlap";
        }
    }
    if (d->n_texts < 0 || d->n_texts > map::kMaxTexts) return "more than 16 texts";
    for (int k = 0; k < d->n_texts; k++) {
        const icelk_map_text_t& t = d->text[k];
        if (t.px < -1048576 || t.px > 1048576 || t.py < -1048576 || t.py > 1048576) return "a text position beyond 2^20";
        if (!map::make_text(t.text, t.px, t.py, &S->text[k]))
            return "a text of more than 48 characters, or a character outside 0-9 - : . / space A-Z a-z , ( )";
    }
    return nullptr;
}

// the scene but for its arrow pointers: views, cameras in fixed units, transparency tables, colour table
void fill_scene(const icelk_map_desc_t* d, map::Scene* S)
{
    S->Wo = d->width, S->Ho = d->height, S->n_views = d->n_panels, S->n_texts = d->n_texts;
    for (int k = 0; k < d->n_panels; k++) {
        const icelk_map_panel_t& p = d->panel[k];
        map::Panel& P = S->P[k];
        P.V = view_of(p);
        P.arrows = nullptr;
        P.vmax = p.vmax;
        P.n_cameras = 0;
        for (int c = 0; c < p.n_cameras; c++)   // a camera whose position is not finite or beyond 2^20 pixels is left out
            if (map::to_fixed(P.V, p.cameras[2 * c], p.cameras[2 * c + 1], &P.cam_x[P.n_cameras], &P.cam_y[P.n_cameras])) P.n_cameras++;
        map::make_table(p.alpha, P.T);
    }
    memcpy(S->table, d->table, sizeof(S->table));
}

// the header's code on the CPU
int overlay_host(const icelk_map_desc_t* d, map::Scene& S, const double* resident, const int32_t* group, int n_resident, uint8_t* rgb,
                 int rgb_stride)
{
    const int Wo = d->width, Ho = d->height;
    std::vector<uint32_t> base, top, count;
    try {
        base.assign((size_t)Wo * Ho, 0);
        top.assign((size_t)Wo * Ho, 0);
        count.assign((size_t)Wo * Ho, 0);
    } catch (...) {
        return ICELK_ENOMEM;
    }
    for (int k = 0; k < d->n_panels; k++) {
        const icelk_map_panel_t& p = d->panel[k];
        const map::View V = S.P[k].V;
        auto at = [&](int px, int py) { return (size_t)(V.y0 + py) * Wo + (V.x0 + px); };
        auto code = [&](uint32_t v) {
            return [&base, at, v](int px, int py) {
                uint32_t& b = base[at(px, py)];
                if (b < v) b = v;
            };
        };
        for (int t = 0; t < p.n_cells; t++) map::walk_cell(V, p.cells[3 * (size_t)t], p.cells[3 * (size_t)t + 1], p.cells[3 * (size_t)t + 2], p.measured[t] != 0, code(1), code(2));
        for (int t = 0; t + 1 < p.n_outline; t++)
            map::walk_segment(V, p.outline[2 * (size_t)t], p.outline[2 * (size_t)t + 1], p.outline[2 * (size_t)t + 2], p.outline[2 * (size_t)t + 3], code(3));
        const double* a = p.resident ? resident : p.arrows;
        const int n = p.resident ? n_resident : p.n_arrows;
        const int32_t* g = p.resident && p.group >= 0 ? group : nullptr;
        const int w = map::arrow_width(V, p.width);
        S.P[k].arrows = a;
        for (int t = 0; t < n; t++) {
            if (g && g[t] != p.group) continue;
            const uint32_t id = (uint32_t)t + 1u;
            map::walk_arrow(V, w, p.pivot == 1, a[5 * (size_t)t], a[5 * (size_t)t + 1], a[5 * (size_t)t + 2], a[5 * (size_t)t + 3], a[5 * (size_t)t + 4],
                            [&](int px, int py) {
                                const size_t o = at(px, py);
                                if (top[o] < id) top[o] = id;
                                count[o]++;
                            });
        }
    }
    for (int j = 0; j < Ho; j++)
        for (int i = 0; i < Wo; i++) {
            const size_t o = (size_t)j * Wo + i;
            map::resolve_pixel(S, base[o], top[o], count[o], i, j, rgb + (size_t)j * rgb_stride + 3 * (size_t)i);
        }
    return ICELK_OK;
}

// The insets of a picture against the thumbnails `have` (kMaxInsets entries, host or device memory): what is refused, and
// the paste's arguments.  The descriptor has passed check_desc.  c: a handle, or whatever has an `err` to take the reason
template <typename Handle>
int check_insets(Handle* c, const icelk_map_desc_t* d, const icelk_map_inset_t* in, int n, const icelk_map_inset_pixels_t* have, thumb::Inset* out)
{
    if (n < 0 || n > thumb::kMaxInsets || (n > 0 && (!in || !have))) FAIL(c, ICELK_EARG, "insets: a count outside 0 .. 8 or a null array");
    for (int k = 0; k < n; k++) {
        const icelk_map_inset_t& I = in[k];
        if (I.index < 0 || I.index >= thumb::kMaxInsets) FAIL(c, ICELK_EARG, "an inset index outside 0 .. 7");
        const icelk_map_inset_pixels_t& T = have[I.index];
        if (!T.rgb) FAIL(c, ICELK_ESTATE, "an inset's index holds no thumbnail (icelk_map_inset_set_file, icelk_map_inset_set_pixels)");
        if (T.w < 1 || T.h < 1 || T.stride < 3 * T.w || I.x0 < 0 || I.y0 < 0 || I.x0 > d->width - T.w || I.y0 > d->height - T.h)
            FAIL(c, ICELK_EARG, "a thumbnail that is not wholly inside the picture");
        if (I.label_px < -thumb::kLabelLimit || I.label_px > thumb::kLabelLimit || I.label_py < -thumb::kLabelLimit || I.label_py > thumb::kLabelLimit)
            FAIL(c, ICELK_EARG, "a label position beyond 2^20");
        out[k].x0 = I.x0, out[k].y0 = I.y0, out[k].w = T.w, out[k].h = T.h, out[k].px = T.rgb, out[k].pitch = T.stride;
        char text[sizeof(I.label) + 1];
        memcpy(text, I.label, sizeof(I.label));
        text[sizeof(I.label)] = 0;
        if (!map::make_text(text, I.label_px, I.label_py, &out[k].label))
            FAIL(c, ICELK_EARG, "a label of more than 48 characters, or a character outside 0-9 - : . / space A-Z a-z , ( )");
    }
    return ICELK_OK;
}

// icelk_map_overlay_host and, with insets, icelk_map_overlay_insets_host
int overlay_call(const icelk_map_desc_t* d, const double* resident, const int32_t* group, int n_resident, const icelk_map_inset_t* insets,
                 int n_insets, const icelk_map_inset_pixels_t* have, uint8_t* rgb, int rgb_stride)
{
    std::unique_ptr<map::Scene> S(new (std::nothrow) map::Scene);
    if (!S) return ICELK_ENOMEM;
    if (!rgb || check_desc(d, S.get())) return ICELK_EARG;
    thumb::Inset I[thumb::kMaxInsets];
    struct { std::string err; } nobody;   // no handle: the reason goes nowhere
    if (int rc = check_insets(&nobody, d, insets, n_insets, have, I)) return rc;
    if (rgb_stride < 3 * d->width || n_resident < 0 || n_resident > kMaxArrows) return ICELK_EARG;
    for (int k = 0; k < d->n_panels; k++)
        if (d->panel[k].resident && (!resident || (d->panel[k].group >= 0 && !group))) return ICELK_ESTATE;
    fill_scene(d, S.get());
    if (int rc = overlay_host(d, *S, resident, group, n_resident, rgb, rgb_stride)) return rc;
    thumb::paste_host(I, n_insets, d->width, d->height, rgb, (size_t)rgb_stride);
    return ICELK_OK;
}

struct Picture {
    PictureFile file;
    size_t items;      // doubles of the call's cells, outlines and arrows
    size_t measured;   // bytes
};

// Everything that can be refused is refused here, before anything is enqueued or allocated.  The scene's texts are made
// on the way (check_desc), the insets' paste arguments too (I: kMaxInsets entries)
int check_device_call(Ctx* c, const icelk_map_desc_t* d, PictureFormat format, const icelk_map_inset_t* insets, int n_insets, const uint8_t* rgb,
                      int rgb_stride, const uint64_t* len, map::Scene* S, thumb::Inset* I, Picture* Q)
{
    const Ctx::Map& M = c->map;
    if (const char* why = check_desc(d, S)) FAIL(c, ICELK_EARG, why);
    if (int rc = picture_check(c, d->width, d->height, format, d->quality, rgb, rgb_stride, len, &Q->file)) return rc;
    Q->items = Q->measured = 0;
    for (int k = 0; k < d->n_panels; k++) {
        const icelk_map_panel_t& p = d->panel[k];
        if (p.resident && !M.have_arrows) FAIL(c, ICELK_ESTATE, "a panel draws the resident arrows and none are set (icelk_map_arrows_set)");
        Q->items += 3 * (size_t)p.n_cells + 2 * (size_t)p.n_outline + (p.resident ? 0 : 5 * (size_t)p.n_arrows);
        Q->measured += (size_t)p.n_cells;
    }
    icelk_map_inset_pixels_t have[thumb::kMaxInsets];
    for (int k = 0; k < thumb::kMaxInsets; k++) have[k] = icelk_map_inset_pixels_t{M.d_inset[k], M.inset_w[k], M.inset_h[k], 3 * M.inset_w[k], 0};
    if (int rc = check_insets(c, d, insets, n_insets, have, I)) return rc;
    for (int k = 0; k < d->n_panels; k++)
        if (d->panel[k].resident && d->panel[k].group >= 0 && !M.d_group)
            FAIL(c, ICELK_ESTATE, "a panel asks for one group and the resident arrows have none");
    return ICELK_OK;
}

int grow_planes(Ctx* c, const Picture& Q)
{
    Ctx::Map& M = c->map;
    if (!M.d_scene)
        if (int rc = dmalloc(c, &M.d_scene, 1)) return rc;
    if (int rc = grow(c, &M.d_planes, &M.planes_cap, 3 * Q.file.px)) return rc;
    if (int rc = grow(c, &M.d_items, &M.items_cap, Q.items)) return rc;
    if (int rc = grow(c, &M.d_measured, &M.measured_cap, Q.measured)) return rc;
    return picture_grow(c, Q.file);
}

// the picture into the writer's R G B, enqueued on the handle's compute stream: what every file format starts from.
// M.h_scene holds the checked scene
int draw_picture(Ctx* c, const icelk_map_desc_t* d, size_t px, const thumb::Inset* insets, int n_insets)
{
    Ctx::Map& M = c->map;
    const hipStream_t st = c->stream;
    const int Wo = d->width, Ho = d->height;
    uint8_t* rgb = c->picture.d_rgb;
    uint32_t *base = M.d_planes, *top = M.d_planes + px, *count = M.d_planes + 2 * px;
    map::Scene& S = *M.h_scene;
    fill_scene(d, &S);
    {
        ProfScope p(c, K_MAP_CLEAR);
        launch_picture_clear(st, M.d_planes, 3 * px);
    }
    if (int rc = check_launch(c, "map_clear")) return rc;
    size_t at = 0, at_m = 0;   // doubles / bytes of d_items / d_measured handed out
    for (int k = 0; k < d->n_panels; k++) {
        const icelk_map_panel_t& p = d->panel[k];
        const map::View V = S.P[k].V;
        if (p.n_cells > 0) {
            double* d_cells = M.d_items + at;
            uint8_t* d_meas = M.d_measured + at_m;
            at += 3 * (size_t)p.n_cells, at_m += (size_t)p.n_cells;
            HIPCHK(c, hipMemcpyAsync(d_cells, p.cells, 3 * (size_t)p.n_cells * sizeof(double), hipMemcpyHostToDevice, st));
            HIPCHK(c, hipMemcpyAsync(d_meas, p.measured, (size_t)p.n_cells, hipMemcpyHostToDevice, st));
            {
                ProfScope ps(c, K_MAP_CELLS);
                launch_map_cells(st, V, d_cells, d_meas, p.n_cells, Wo, base);
            }
            if (int rc = check_launch(c, "map_cells")) return rc;
        }
        if (p.n_outline > 0) {
            double* d_xy = M.d_items + at;
            at += 2 * (size_t)p.n_outline;
            HIPCHK(c, hipMemcpyAsync(d_xy, p.outline, 2 * (size_t)p.n_outline * sizeof(double), hipMemcpyHostToDevice, st));
            {
                ProfScope ps(c, K_MAP_POLYLINE);
                launch_map_polyline(st, V, d_xy, p.n_outline, Wo, base);
            }
            if (int rc = check_launch(c, "map_polyline")) return rc;
        }
        const double* d_arrows = M.d_arrows;
        const int32_t* d_group = p.group >= 0 ? M.d_group : nullptr;
        int n = M.n_arrows;
        if (!p.resident) {
            double* dst = M.d_items + at;
            at += 5 * (size_t)p.n_arrows;
            if (p.n_arrows > 0) HIPCHK(c, hipMemcpyAsync(dst, p.arrows, 5 * (size_t)p.n_arrows * sizeof(double), hipMemcpyHostToDevice, st));
            d_arrows = dst, d_group = nullptr, n = p.n_arrows;
        }
        S.P[k].arrows = d_arrows;
        {
            ProfScope ps(c, K_MAP_ARROWS);
            launch_map_arrows(st, V, map::arrow_width(V, p.width), p.pivot == 1, d_arrows, d_group, p.group, n, Wo, top, count);
        }
        if (int rc = check_launch(c, "map_arrows")) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(M.d_scene, &S, sizeof(S), hipMemcpyHostToDevice, st));
    {
        ProfScope p(c, K_MAP_RESOLVE);
        launch_map_resolve(st, M.d_scene, Wo, Ho, base, top, count, rgb);
    }
    if (int rc = check_launch(c, "map_resolve")) return rc;
    for (int k = 0; k < n_insets; k++) {
        {
            ProfScope p(c, K_MAP_INSET);
            launch_map_inset(st, insets[k], Wo, Ho, rgb);
        }
        if (int rc = check_launch(c, "map_inset")) return rc;
    }
    return ICELK_OK;
}

void release_arrows(Ctx* c)
{
    Ctx::Map& M = c->map;
    if (M.d_arrows) hipFree(M.d_arrows);   // waits for everything that may still read them
    if (M.d_group) hipFree(M.d_group);
    M.d_arrows = nullptr, M.d_group = nullptr, M.n_arrows = 0, M.have_arrows = false;
}

}  // namespace

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_map_glyph(int ch, uint8_t* rows)
{
    const int g = map::glyph_index(ch);
    if (!rows || g < 0) return ICELK_EARG;
    for (int r = 0; r < plot::kGlyphH; r++) rows[r] = (uint8_t)map::glyph_row(g, r);
    return ICELK_OK;
}

int icelk_map_overlay_host(const icelk_map_desc_t* d, const double* resident, const int32_t* group, int n_resident, uint8_t* rgb,
                           int rgb_stride)
{
    return overlay_call(d, resident, group, n_resident, nullptr, 0, nullptr, rgb, rgb_stride);
}

int icelk_map_overlay_insets_host(const icelk_map_desc_t* d, const double* resident, const int32_t* group, int n_resident,
                                  const icelk_map_inset_t* insets, int n_insets, const icelk_map_inset_pixels_t* resident_insets,
                                  uint8_t* rgb, int rgb_stride)
{
    return overlay_call(d, resident, group, n_resident, insets, n_insets, resident_insets, rgb, rgb_stride);
}

int icelk_map_arrows_set(icelk_t* h, const double* arrows, const int32_t* group_or_null, int n)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (n < 0 || n > kMaxArrows || (n > 0 && !arrows)) FAIL(c, ICELK_EARG, "arrows: a count outside 0 .. 2^27 or a null array");
    HIPCHK(c, hipSetDevice(c->device));
    release_arrows(c);
    Ctx::Map& M = c->map;
    if (int rc = dmalloc(c, &M.d_arrows, 5 * (size_t)n)) return rc;
    if (group_or_null)
        if (int rc = dmalloc(c, &M.d_group, (size_t)n)) {
            release_arrows(c);
            return rc;
        }
    if (n > 0) {
        hipError_t e = hipMemcpy(M.d_arrows, arrows, 5 * (size_t)n * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess && group_or_null) e = hipMemcpy(M.d_group, group_or_null, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            release_arrows(c);
            HIPCHK(c, e);
        }
    }
    M.n_arrows = n;
    M.have_arrows = true;
    return ICELK_OK;
}

int icelk_map_arrows_release(icelk_t* h)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    release_arrows(c);
    return ICELK_OK;
}

// the three entry points: icelk_map_draw has no insets
static int map_draw_call(icelk_t* h, const char* range, PictureFormat format, const icelk_map_desc_t* d, const icelk_map_inset_t* insets,
                         int n_insets, uint8_t* rgb_or_null, int rgb_stride, uint8_t* file, uint64_t capacity, uint64_t* len)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Range rg(range);
    Ctx::Map& M = c->map;
    if (!M.h_scene) M.h_scene = new (std::nothrow) map::Scene;
    if (!M.h_scene) FAIL(c, ICELK_ENOMEM, "the map's scene");
    Picture Q;
    thumb::Inset I[thumb::kMaxInsets];
    if (int rc = check_device_call(c, d, format, insets, n_insets, rgb_or_null, rgb_stride, len, M.h_scene, I, &Q)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = grow_planes(c, Q)) return rc;
    if (int rc = draw_picture(c, d, Q.file.px, I, n_insets)) return rc;
    return picture_write(c, c->stream, Q.file, rgb_or_null, rgb_stride, file, capacity, len);
}

int icelk_map_draw(icelk_t* h, const icelk_map_desc_t* d, uint8_t* rgb_or_null, int rgb_stride, uint8_t* file, uint64_t capacity,
                   uint64_t* len)
{
    return map_draw_call(h, "icelk map_draw", PICTURE_JPEG, d, nullptr, 0, rgb_or_null, rgb_stride, file, capacity, len);
}

int icelk_map_draw_insets(icelk_t* h, const icelk_map_desc_t* d, const icelk_map_inset_t* insets, int n_insets, uint8_t* rgb_or_null,
                          int rgb_stride, uint8_t* file, uint64_t capacity, uint64_t* len)
{
    return map_draw_call(h, "icelk map_draw_insets", PICTURE_JPEG, d, insets, n_insets, rgb_or_null, rgb_stride, file, capacity, len);
}

int icelk_map_draw_png(icelk_t* h, const icelk_map_desc_t* d, const icelk_map_inset_t* insets_or_null, int n_insets, uint8_t* rgb_or_null,
                       int rgb_stride, uint8_t* file, uint64_t capacity, uint64_t* len)
{
    return map_draw_call(h, "icelk map_draw_png", PICTURE_PNG, d, insets_or_null, n_insets, rgb_or_null, rgb_stride, file, capacity, len);
}

}  // extern "C"
