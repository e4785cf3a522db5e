// abi_picture.hip -- the picture writer: what the segment picture (abi_plot.hip) and the velocity map (abi_map.hip) do once
// their kernels have drawn.  A kind of picture checks its own arguments, calls picture_check and picture_grow, draws its
// Wo x Ho interleaved R G B into c->picture.d_rgb on the handle's compute stream and calls picture_write: a new kind plugs
// in there, a new file format in picture_write's switch.  A JPEG is what Pillow's Image.fromarray(rgb).save(f, "JPEG",
// quality=quality) writes; a PNG (abi_png.hip) holds the pixels exactly.  Every call waits for the device.  After
// ICELK_ECAP (*len says what the file takes, the file buffer is untouched) the call is simply repeated: the picture is a
// function of its arguments.
// Bounds.  picture_grow sizes d_rgb to 3 px bytes, px = Wo Ho padded to four pixels, before anything is enqueued; the
// drawing kernels' headers say why they stay below 3 Wo Ho.  The coders size their own buffers from the file's layout.
#include "icelk_ctx.h"
#include "jpeg_enc_host.h"
#include "jpeg_resave_host.h"

namespace icelk {

void picture_destroy(Ctx* c)
{
    jpeg_resave_free(c->picture);
    c->picture = Ctx::JpegResave{};
    c->picture_w = c->picture_h = 0;
}

static size_t pad4(size_t v) { return (v + 3) & ~(size_t)3; }

// Everything about the file that can be refused is refused here, before anything is allocated or enqueued
int picture_check(Ctx* c, int Wo, int Ho, PictureFormat format, int quality, const uint8_t* rgb, int rgb_stride, const uint64_t* len,
                  PictureFile* F)
{
    if (!len) FAIL(c, ICELK_EARG, "null length");
    if (int rc = format == PICTURE_PNG ? png_check(c, Wo, Ho) : jpeg_resave_check(c, Wo, Ho, quality)) return rc;
    if (rgb && rgb_stride < 3 * Wo) FAIL(c, ICELK_EARG, "rgb stride smaller than 3 x the picture's width");
    *F = PictureFile{format, Wo, Ho, pad4((size_t)Wo * Ho), {}, {}};
    if (format == PICTURE_PNG) return ICELK_OK;   // the quality is not looked at and the picture has no JPEG layout
    resave::resave_info(Wo, Ho, quality, &F->info);
    return jpeg_enc_rc(c, enc::layout_of(&F->info, &F->L));
}

int picture_grow(Ctx* c, const PictureFile& F)
{
    Ctx::JpegResave& R = c->picture;
    c->picture_draws++;   // whoever draws next draws over what d_rgb holds (abi_ortho.hip: the mosaic in progress)
    if (int rc = grow(c, &R.d_rgb, &R.rgb_cap, 3 * F.px)) return rc;
    if (F.format == PICTURE_PNG) return png_grow(c, F.Wo, F.Ho);
    return grow(c, &R.d_rcoef, &R.rcoef_cap, (size_t)F.info.coef_count);
}

// c->picture.d_rgb, drawn on stream st, -> the file and, if asked for, the R G B.  Both coders synchronise st; the copy of
// the R G B goes out behind them, so a refusal of the file has to wait for it (the `pending` of the deliver functions)
int picture_write(Ctx* c, hipStream_t st, const PictureFile& F, uint8_t* rgb, int rgb_stride, uint8_t* file, uint64_t capacity, uint64_t* len)
{
    Ctx::JpegResave& R = c->picture;
    const size_t row = 3 * (size_t)F.Wo;
    uint32_t nbytes = 0;   // PNG: the deflate block's
    c->picture_w = F.Wo, c->picture_h = F.Ho;   // what icelk_picture_frame (abi_movie.hip) makes a movie frame of
    switch (F.format) {
    case PICTURE_JPEG:
        if (int rc = jpeg_fwd_on(c, st, R.d_rgb, R.d_rcoef, F.Wo, F.Ho, F.info)) return rc;
        if (int rc = jpeg_encode_on(c, R.enc, st, F.L, R.d_rcoef)) return rc;
        if (rgb) HIPCHK(c, hipMemcpy2DAsync(rgb, rgb_stride, R.d_rgb, row, row, F.Ho, hipMemcpyDeviceToHost, st));
        return jpeg_deliver_file(c, R.enc, st, rgb != nullptr, F.info, nullptr, 0, file, capacity, len);
    case PICTURE_PNG:
        if (int rc = png_encode_on(c, st, R.d_rgb, (uint32_t)row, F.Wo, F.Ho, &nbytes)) return rc;
        if (rgb) HIPCHK(c, hipMemcpy2DAsync(rgb, rgb_stride, R.d_rgb, row, row, F.Ho, hipMemcpyDeviceToHost, st));
        return png_deliver_file(c, st, rgb != nullptr, F.Wo, F.Ho, nbytes, file, capacity, len);
    }
    FAIL(c, ICELK_EARG, "a picture format other than JPEG and PNG");   // picture_check lets none through
}

}  // namespace icelk
