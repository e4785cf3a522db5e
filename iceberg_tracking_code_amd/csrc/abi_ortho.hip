// abi_ortho.hip -- the orthophoto: camera photographs rectified onto a map raster, one mosaic in progress
// per handle, written through the picture writer (abi_picture.hip).  The rule is ortho.h, the kernels are k_ortho.hip's.
//
//   host    icelk_ortho_coords_host, icelk_ortho_begin_host, icelk_ortho_add_host: ortho.h on the CPU; no handle, re-entrant
//   device  icelk_ortho_begin: refusals, then the working set (cover and best planes here, the R G B by picture_grow) and
//           k_ortho_fill.  icelk_ortho_add_pixels uploads the caller's pixels; icelk_ortho_add_jpeg_file takes the
//           synchronous ingest route (jpeg_huff_device -> jpeg_planes(..., on_device), abi_jpeg_ingest.hip: the same
//           files, the same error codes, the host's Huffman decoder inside the call), then k_jpeg_out into the decoder's
//           R G B buffer (a gray file: its luma plane as it is); icelk_ortho_add_slot reads level 0 of a frame slot as
//           every reader of a slot does.  Each then runs k_ortho_add on the compute stream and waits for it.
//           icelk_ortho_write is picture_write on the mosaic.
// The mosaic lives in the picture writer's R G B, which every kind of picture shares: picture_draws counts them, and a
// mosaic whose count has moved on (a segment picture or a map was drawn since) is over -- ICELK_ESTATE until the next begin.
// Bounds: k_ortho.hip's header states them; what it relies on is checked here before every launch.
#include "icelk_ctx.h"

namespace icelk {

void ortho_destroy(Ctx* c)
{
    Ctx::Ortho& O = c->ortho;
    if (O.d_cover) hipFree(O.d_cover);
    if (O.d_best) hipFree(O.d_best);
    if (O.d_src) hipFree(O.d_src);
    O = Ctx::Ortho{};
}

namespace {

icelk_ortho_opts_t opts_of(const icelk_ortho_opts_t* o)
{
    if (o) return *o;
    icelk_ortho_opts_t d{};
    d.max_range = 0.0, d.sampling = 0, d.fill[0] = d.fill[1] = d.fill[2] = 255;
    return d;
}

bool opts_ok(const icelk_ortho_opts_t& o) { return o.max_range == o.max_range && (o.sampling == 0 || o.sampling == 1); }

// what every add call checks before it touches the device
int check_add(Ctx* c, const icelk_camera_t* cam, int index)
{
    const Ctx::Ortho& O = c->ortho;
    if (!cam) FAIL(c, ICELK_EARG, "null camera");
    if (index < 0 || index > ortho::kMaxIndex) FAIL(c, ICELK_EARG, "a camera index outside 0 .. 254");
    if (!ortho::camera_ok(*cam)) FAIL(c, ICELK_EARG, "a camera with a non-finite number");
    if (!O.active) FAIL(c, ICELK_ESTATE, "no orthophoto has been begun (icelk_ortho_begin)");
    if (O.draws != c->picture_draws) FAIL(c, ICELK_ESTATE, "another picture was drawn since icelk_ortho_begin: the mosaic is gone");
    return ICELK_OK;
}

int add_on(Ctx* c, const icelk_camera_t& cam, int index, const ortho::Source& S)
{
    Ctx::Ortho& O = c->ortho;
    {
        ProfScope p(c, K_ORTHO_ADD);
        launch_ortho_add(c->stream, cam, O.raster, S, O.opts.max_range, O.opts.sampling, index, c->picture.d_rgb, O.d_cover, O.d_best);
    }
    return check_launch(c, "ortho_add");
}

}  // namespace

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_ortho_coords_host(const icelk_camera_t* cam, const icelk_ortho_raster_t* raster, int sw, int sh, double max_range, double* xs,
                            double* ys, double* d2, uint8_t* seen)
{
    if (!cam || !raster || !ortho::raster_ok(*raster) || !ortho::camera_ok(*cam) || max_range != max_range) return ICELK_EARG;
    if (sw < 1 || sw > ortho::kMaxSource || sh < 1 || sh > ortho::kMaxSource) return ICELK_EARG;
    for (int j = 0; j < raster->height; j++)
        for (int i = 0; i < raster->width; i++) {
            const ortho::Hit h = ortho::locate(*cam, *raster, i, j, sw, sh, max_range);
            const size_t t = (size_t)j * raster->width + i;
            if (xs) xs[t] = h.xs;
            if (ys) ys[t] = h.ys;
            if (d2) d2[t] = h.d2;
            if (seen) seen[t] = h.seen ? 1 : 0;
        }
    return ICELK_OK;
}

int icelk_ortho_begin_host(const icelk_ortho_raster_t* raster, const icelk_ortho_opts_t* opts_or_null, uint8_t* rgb, int rgb_stride,
                           uint8_t* cover, int cover_stride, double* best)
{
    if (!raster || !rgb || !cover || !best || !ortho::raster_ok(*raster)) return ICELK_EARG;
    const icelk_ortho_opts_t o = opts_of(opts_or_null);
    if (!opts_ok(o) || (long long)rgb_stride < 3LL * raster->width || cover_stride < raster->width) return ICELK_EARG;
    ortho::begin_host(*raster, o.fill, rgb, (size_t)rgb_stride, cover, (size_t)cover_stride, best);
    return ICELK_OK;
}

int icelk_ortho_add_host(const icelk_ortho_raster_t* raster, const icelk_ortho_opts_t* opts_or_null, const icelk_camera_t* cam, int index,
                         const uint8_t* img, int sw, int sh, int channels, int stride, uint8_t* rgb, int rgb_stride, uint8_t* cover,
                         int cover_stride, double* best)
{
    if (!raster || !cam || !img || !rgb || !cover || !best || !ortho::raster_ok(*raster) || !ortho::camera_ok(*cam)) return ICELK_EARG;
    const icelk_ortho_opts_t o = opts_of(opts_or_null);
    if (!opts_ok(o) || (long long)rgb_stride < 3LL * raster->width || cover_stride < raster->width) return ICELK_EARG;
    if (index < 0 || index > ortho::kMaxIndex || !ortho::source_ok(sw, sh, channels, stride)) return ICELK_EARG;
    const ortho::Source S{img, sw, sh, channels, (int64_t)stride};
    ortho::add_host(*cam, *raster, S, o.max_range, o.sampling, index, rgb, (size_t)rgb_stride, cover, (size_t)cover_stride, best);
    return ICELK_OK;
}

int icelk_ortho_begin(icelk_t* h, const icelk_ortho_raster_t* raster, const icelk_ortho_opts_t* opts_or_null)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Ctx::Ortho& O = c->ortho;
    if (!raster) FAIL(c, ICELK_EARG, "null raster");
    if (!ortho::raster_ok(*raster)) FAIL(c, ICELK_EARG, "a raster with res <= 0, a non-finite number or a side below 1");
    const icelk_ortho_opts_t o = opts_of(opts_or_null);
    if (!opts_ok(o)) FAIL(c, ICELK_EARG, "sampling other than 0 (bilinear) and 1 (nearest), or max_range not a number");
    // the PNG writer's limits: the stricter upper ones; a JPEG's width >= 3 is icelk_ortho_write's to refuse
    uint64_t len = 0;
    PictureFile F;
    if (int rc = picture_check(c, raster->width, raster->height, PICTURE_PNG, 0, nullptr, 0, &len, &F)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    O.active = false;
    const size_t n = (size_t)raster->width * raster->height;
    if (int rc = picture_grow(c, F)) return rc;
    if (int rc = grow(c, &O.d_cover, &O.cover_cap, n)) return rc;
    if (int rc = grow(c, &O.d_best, &O.best_cap, n)) return rc;
    {
        ProfScope p(c, K_ORTHO_FILL);
        launch_ortho_fill(c->stream, raster->width, raster->height, o.fill, c->picture.d_rgb, O.d_cover, O.d_best);
    }
    if (int rc = check_launch(c, "ortho_fill")) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    O.raster = *raster, O.opts = o, O.draws = c->picture_draws, O.active = true;
    return ICELK_OK;
}

int icelk_ortho_add_pixels(icelk_t* h, const icelk_camera_t* cam, int index, const uint8_t* img, int sw, int sh, int channels, int stride)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Ctx::Ortho& O = c->ortho;
    if (!img) FAIL(c, ICELK_EARG, "null image");
    if (!ortho::source_ok(sw, sh, channels, stride))
        FAIL(c, ICELK_EARG, "a source side outside 1 .. 65535, channels other than 1 and 3, or a stride smaller than a row");
    if (int rc = check_add(c, cam, index)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t row = (size_t)sw * channels;
    if (int rc = grow(c, &O.d_src, &O.src_cap, row * sh)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(O.d_src, row, img, (size_t)stride, row, (size_t)sh, hipMemcpyHostToDevice, c->stream));
    const ortho::Source S{O.d_src, sw, sh, channels, (int64_t)row};
    if (int rc = add_on(c, *cam, index, S)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // the caller's pixels have been read, the mosaic is up to date
    return ICELK_OK;
}

int icelk_ortho_add_jpeg_file(icelk_t* h, const icelk_camera_t* cam, int index, const uint8_t* data, uint64_t len)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (int rc = check_add(c, cam, index)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    icelk_jpeg_info_t I;
    if (int rc = jpeg_huff_device(c, data, len, &I)) return rc;
    JpegOutArgs A{};
    if (int rc = jpeg_planes(c, &I, nullptr, 0, 0, 0, 0, &A, true)) return rc;
    ortho::Source S{A.plane[0], A.ow, A.oh, 1, (int64_t)A.pitch[0]};   // a gray file: the luma plane, W x H samples at its top-left
    if (I.ncomp != 1) {
        const size_t row = 3 * (size_t)A.ow;
        if (int rc = grow(c, &c->jpeg.d_rgb, &c->jpeg.rgb_cap, row * A.oh)) return rc;
        A.dst = c->jpeg.d_rgb;
        A.dst_pitch = (int)row;
        {
            ProfScope p(c, K_JPEG_OUT);
            launch_jpeg_rgb(c->stream, A);
        }
        if (int rc = check_launch(c, "jpeg_out")) return rc;
        S = ortho::Source{c->jpeg.d_rgb, A.ow, A.oh, 3, (int64_t)row};
    }
    if (int rc = add_on(c, *cam, index, S)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

int icelk_ortho_add_slot(icelk_t* h, const icelk_camera_t* cam, int index, int slot)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (int rc = check_slot(c, slot, true)) return rc;
    if (!c->jpeg.slot_job.empty() && c->jpeg.slot_job[slot] >= 0)
        FAIL(c, ICELK_ESTATE, "the slot's JPEG file is still in flight (icelk_jpeg_async_finish ends it)");
    if (int rc = check_add(c, cam, index)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Slot& s = c->slots[slot];
    if (int rc = wait_slot(c, slot)) return rc;
    if (int rc = wait_event(c, c->stream, s.frame_ev)) return rc;
    const Level& L = s.lv[0];
    const ortho::Source S{L.ptr, L.w, L.h, 1, (int64_t)L.pitch};
    if (int rc = add_on(c, *cam, index, S)) return rc;
    HIPCHK(c, hipEventRecord(s.used_own, c->stream));   // an upload into the slot waits for this reader
    s.used = s.used_own;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

int icelk_ortho_write(icelk_t* h, int format, int quality, uint8_t* rgb_or_null, int rgb_stride, uint8_t* cover_or_null, int cover_stride,
                      uint8_t* file, uint64_t capacity, uint64_t* len)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Ctx::Ortho& O = c->ortho;
    if (format != 0 && format != 1) FAIL(c, ICELK_EARG, "a picture format other than 0 (JPEG) and 1 (PNG)");
    if (!O.active) FAIL(c, ICELK_ESTATE, "no orthophoto has been begun (icelk_ortho_begin)");
    if (O.draws != c->picture_draws) FAIL(c, ICELK_ESTATE, "another picture was drawn since icelk_ortho_begin: the mosaic is gone");
    const int W = O.raster.width, H = O.raster.height;
    if (cover_or_null && cover_stride < W) FAIL(c, ICELK_EARG, "cover stride smaller than the raster's width");
    PictureFile F;
    if (int rc = picture_check(c, W, H, format == 1 ? PICTURE_PNG : PICTURE_JPEG, quality, rgb_or_null, rgb_stride, len, &F)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // the coder's buffers; d_rgb already holds 3 F.px bytes (begin), so grow() leaves it and the mosaic alone
    if (int rc = picture_grow(c, F)) return rc;
    O.draws = c->picture_draws;
    if (cover_or_null)
        HIPCHK(c, hipMemcpy2DAsync(cover_or_null, (size_t)cover_stride, O.d_cover, (size_t)W, (size_t)W, (size_t)H, hipMemcpyDeviceToHost, c->stream));
    const int rc = picture_write(c, c->stream, F, rgb_or_null, rgb_stride, file, capacity, len);
    if (cover_or_null) HIPCHK(c, hipStreamSynchronize(c->stream));   // a refusal of the file must not leave the copy in flight
    return rc;
}

}  // extern "C"
