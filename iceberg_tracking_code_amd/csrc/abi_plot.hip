// abi_plot.hip -- the picture the reference draws of every saved segment (s1:397-434, plot_switch = 1): the segment's last
// gray frame at out_width pixels, its surviving tracks as red lines, their end points as red dots, a stamp in a corner --
// rasterised on the device, where frame and tracks already are, and handed to the picture writer that is there as well.
//
//   host    icelk_plot_size, icelk_plot_glyph, icelk_plot_overlay_host: plot_raster.h on the CPU; no handle, re-entrant
//   device  icelk_plot_tracks (tracks from the host) and icelk_seg_plot (the surviving tracks of a segment, gathered on the
//           device: no track data crosses PCIe).  On the handle's compute stream: k_plot_background, k_picture_clear,
//           k_plot_scatter, k_plot_resolve (k_plot.hip), from planes of plotting's own (Ctx::Plot) into the picture
//           writer's R G B; the file, the optional R G B output, the wait for the device and ICELK_ECAP are the writer's
//           (abi_picture.hip: picture_check, picture_grow, picture_write)
//
// Bounds.  Every store of the kernels is inside a buffer sized from Wo x Ho before anything is enqueued: the background
// kernel writes pixel (i, j) with i < Wo, j < Ho and reads dwords inside the rows of the slot's level 0; the scatter
// kernel clips the range it walks to the image and tests the other coordinate of every hit, whatever the vertices hold
// (tracks with a vertex that is not finite or beyond 2^20 never get that far); the resolve kernel stores 12 bytes per
// four pixels below 3 Wo Ho, the tail byte by byte.
#include <new>
#include <vector>

#include "icelk_ctx.h"

namespace icelk {

void plot_destroy(Ctx* c)
{
    Ctx::Plot& P = c->plot;
    void* p[] = {P.d_bg, P.d_counts, P.d_tables, P.d_tracks};
    for (void* q : p)
        if (q) hipFree(q);
    P = Ctx::Plot{};
}

namespace {

constexpr int kMaxTracks = 1 << 24;

// what needs no handle: the frame's size, the width asked for, the stamp.  nullptr: fine
const char* check_picture(int w, int h, int out_width, const char* stamp, plot::Stamp* S)
{
    if (w < 1 || h < 1 || w > 65535 || h > 65535) return "frame size outside 1 .. 65535";
    if (out_width < plot::kMinWidth) return "a picture less than 8 pixels wide";
    if (!plot::make_stamp(stamp, S)) return "a stamp of more than 48 characters, or a character outside 0-9 - : . / and space";
    return nullptr;
}

const char* check_tracks(const float* tracks, int n, int vertices)
{
    if (n < 0 || n > kMaxTracks) return "track count outside 0 .. 2^24";
    if (n > 0 && (!tracks || vertices < 1 || vertices > plot::kMaxVertices)) return "null tracks, or vertices outside 1 .. 17";
    return nullptr;
}

// the header's code on the CPU: gray (w x h, stride bytes) + tracks -> rgb (Wo x Ho, rgb_stride bytes)
int overlay_host(const uint8_t* gray, int w, int h, int stride, const float* tracks, int n, int nv, int Wo, int Ho, const plot::Stamp& S,
                 uint8_t* rgb, int rgb_stride)
{
    std::vector<uint32_t> lines, dots;
    std::vector<uint8_t> bg;
    try {
        lines.assign((size_t)Wo * Ho, 0);
        dots.assign((size_t)Wo * Ho, 0);
        bg.resize((size_t)Wo * Ho);
    } catch (...) {
        return ICELK_ENOMEM;
    }
    for (int j = 0; j < Ho; j++)
        for (int i = 0; i < Wo; i++) {
            uint64_t sum = 0;
            for (int y = plot::first_source(j, h, Ho); y <= plot::last_source(j, h, Ho); y++) {
                uint64_t row = 0;
                for (int x = plot::first_source(i, w, Wo); x <= plot::last_source(i, w, Wo); x++)
                    row += (uint64_t)plot::overlap(x, i, w, Wo) * gray[(size_t)y * stride + x];
                sum += (uint64_t)plot::overlap(y, j, h, Ho) * row;
            }
            bg[(size_t)j * Wo + i] = (uint8_t)plot::average(sum, w, h);
        }
    for (int t = 0; t < n; t++) {
        const float* v = tracks + (size_t)t * nv * 2;
        bool ok = true;
        for (int k = 0; k < nv; k++) ok = ok && plot::vertex_ok(v[2 * k], v[2 * k + 1]);
        if (!ok) continue;
        auto line = [&](int px, int py) { lines[(size_t)py * Wo + px]++; };
        auto dot = [&](int px, int py) { dots[(size_t)py * Wo + px]++; };
        for (int k = 0; k + 1 < nv; k++)
            plot::walk_pair(plot::coord(v[2 * k], Wo, w), plot::coord(v[2 * k + 1], Ho, h), plot::coord(v[2 * k + 2], Wo, w),
                            plot::coord(v[2 * k + 3], Ho, h), Wo, Ho, line);
        plot::walk_dot(plot::coord(v[2 * nv - 2], Wo, w), plot::coord(v[2 * nv - 1], Ho, h), Wo, Ho, dot);
    }
    uint32_t TL[plot::kTable], TD[plot::kTable];
    plot::make_tables(TL, TD);
    for (int j = 0; j < Ho; j++)
        for (int i = 0; i < Wo; i++) {
            const size_t p = (size_t)j * Wo + i;
            plot::resolve_pixel(bg[p], lines[p], dots[p], TL, TD, S, i, j, Wo, Ho, rgb + (size_t)j * rgb_stride + 3 * (size_t)i);
        }
    return ICELK_OK;
}

struct Picture {
    int slot;
    plot::Stamp stamp;
    PictureFile file;
};

// Everything that can be refused is refused here, before anything is enqueued or allocated
int check_device_call(Ctx* c, int slot, int out_width, const char* stamp, int quality, const uint8_t* rgb, int rgb_stride, const uint64_t* len,
                      Picture* Q)
{
    if (int rc = check_slot(c, slot, true)) return rc;
    if (!c->jpeg.slot_job.empty() && c->jpeg.slot_job[slot] >= 0)
        FAIL(c, ICELK_ESTATE, "the slot's JPEG file is still in flight (icelk_jpeg_async_finish ends it)");
    const Slot& s = c->slots[slot];
    if (const char* why = check_picture(s.w, s.h, out_width, stamp, &Q->stamp)) FAIL(c, ICELK_EARG, why);
    Q->slot = slot;
    const int Wo = plot::out_width_of(s.w, out_width);
    return picture_check(c, Wo, plot::out_height_of(s.w, s.h, Wo), PICTURE_JPEG, quality, rgb, rgb_stride, len, &Q->file);
}

int grow_planes(Ctx* c, const Picture& Q)
{
    Ctx::Plot& P = c->plot;
    if (!P.d_tables) {
        uint32_t T[2 * plot::kTable];
        plot::make_tables(T, T + plot::kTable);
        uint32_t* d = nullptr;
        if (int rc = dmalloc(c, &d, (size_t)2 * plot::kTable)) return rc;
        const hipError_t e = hipMemcpy(d, T, sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            hipFree(d);
            HIPCHK(c, e);
        }
        P.d_tables = d;
    }
    if (int rc = grow(c, &P.d_bg, &P.bg_cap, Q.file.px)) return rc;
    if (int rc = grow(c, &P.d_counts, &P.counts_cap, 2 * Q.file.px)) return rc;
    return picture_grow(c, Q.file);
}

// d_tracks: (n, nv, 2) on the device, ordered on the compute stream.  The four kernels, then the writer
int draw_and_write(Ctx* c, const Picture& Q, const float* d_tracks, int n, int nv, uint8_t* rgb, int rgb_stride, uint8_t* file,
                   uint64_t capacity, uint64_t* len)
{
    Ctx::Plot& P = c->plot;
    const hipStream_t st = c->stream;
    Slot& s = c->slots[Q.slot];
    const int Wo = Q.file.Wo, Ho = Q.file.Ho;
    uint32_t *lines = P.d_counts, *dots = P.d_counts + Q.file.px;
    if (int rc = wait_slot(c, Q.slot)) return rc;
    {
        ProfScope p(c, K_PLOT_BACKGROUND);
        launch_plot_background(st, s.lv[0], Wo, Ho, P.d_bg);
    }
    if (int rc = check_launch(c, "plot_background")) return rc;
    HIPCHK(c, hipEventRecord(s.used_own, st));   // an upload into the slot waits for this reader
    s.used = s.used_own;
    {
        ProfScope p(c, K_PLOT_CLEAR);
        launch_picture_clear(st, P.d_counts, 2 * Q.file.px);
    }
    if (int rc = check_launch(c, "plot_clear")) return rc;
    {
        ProfScope p(c, K_PLOT_SCATTER);
        launch_plot_scatter(st, d_tracks, n, nv, s.w, s.h, Wo, Ho, lines, dots);
    }
    if (int rc = check_launch(c, "plot_scatter")) return rc;
    {
        ProfScope p(c, K_PLOT_RESOLVE);
        launch_plot_resolve(st, P.d_bg, lines, dots, P.d_tables, Q.stamp, Wo, Ho, c->picture.d_rgb);
    }
    if (int rc = check_launch(c, "plot_resolve")) return rc;
    return picture_write(c, st, Q.file, rgb, rgb_stride, file, capacity, len);
}

}  // namespace

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_plot_size(int w, int h_, int out_width, int* ow, int* oh)
{
    plot::Stamp S;
    if (!ow || !oh || check_picture(w, h_, out_width, nullptr, &S)) return ICELK_EARG;
    *ow = plot::out_width_of(w, out_width);
    *oh = plot::out_height_of(w, h_, *ow);
    return ICELK_OK;
}

int icelk_plot_glyph(int ch, uint8_t* rows)
{
    const int g = plot::glyph_index(ch);
    if (!rows || g < 0) return ICELK_EARG;
    for (int r = 0; r < plot::kGlyphH; r++) rows[r] = (uint8_t)plot::glyph_row(g, r);
    return ICELK_OK;
}

int icelk_plot_overlay_host(const uint8_t* gray, int w, int h_, int stride, const float* tracks, int n, int vertices, int out_width,
                            const char* stamp, uint8_t* rgb, int rgb_stride)
{
    plot::Stamp S;
    if (!gray || !rgb || check_picture(w, h_, out_width, stamp, &S) || check_tracks(tracks, n, vertices) || stride < w) return ICELK_EARG;
    const int Wo = plot::out_width_of(w, out_width), Ho = plot::out_height_of(w, h_, Wo);
    if (rgb_stride < 3 * Wo) return ICELK_EARG;
    return overlay_host(gray, w, h_, stride, tracks, n, vertices, Wo, Ho, S, rgb, rgb_stride);
}

int icelk_plot_tracks(icelk_t* h, int slot, const float* tracks, int n, int vertices, int out_width, const char* stamp, int quality,
                      uint8_t* rgb_or_null, int rgb_stride, uint8_t* file, uint64_t capacity, uint64_t* len)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Range rg("icelk plot_tracks");
    if (const char* why = check_tracks(tracks, n, vertices)) FAIL(c, ICELK_EARG, why);
    Picture Q;
    if (int rc = check_device_call(c, slot, out_width, stamp, quality, rgb_or_null, rgb_stride, len, &Q)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = grow_planes(c, Q)) return rc;
    Ctx::Plot& P = c->plot;
    if (n > 0) {
        const size_t floats = (size_t)n * vertices * 2;
        if (int rc = grow(c, &P.d_tracks, &P.tracks_cap, floats)) return rc;
        HIPCHK(c, hipMemcpyAsync(P.d_tracks, tracks, floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    return draw_and_write(c, Q, P.d_tracks, n, n > 0 ? vertices : 1, rgb_or_null, rgb_stride, file, capacity, len);
}

int icelk_seg_plot(icelk_t* h, int slot, int closed, int out_width, const char* stamp, int quality, uint8_t* rgb_or_null, int rgb_stride,
                   uint8_t* file, uint64_t capacity, uint64_t* len, int* out_n)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Range rg("icelk seg_plot");
    Picture Q;
    if (int rc = check_device_call(c, slot, out_width, stamp, quality, rgb_or_null, rgb_stride, len, &Q)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    int n = 0, nv = 0;
    if (int rc = seg_gather_packed(c, closed != 0, &n, &nv)) return rc;
    if (out_n) *out_n = n;
    if (int rc = grow_planes(c, Q)) return rc;
    return draw_and_write(c, Q, c->d_out_tracks, n, n > 0 ? nv : 1, rgb_or_null, rgb_stride, file, capacity, len);
}

}  // extern "C"
