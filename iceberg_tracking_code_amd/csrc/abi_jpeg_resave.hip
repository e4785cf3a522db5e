// abi_jpeg_resave.hip -- the reference's lossy re-save of the crop (s1:272, camtools.py:64-104: every photo is cropped
// with Pillow and written back as a new JPEG, and the loop tracks on THOSE files) without the file: the entropy coder
// is lossless, so the pixels of "save, then open" are a function of the cropped R G B alone.
//
//   host    the tables (icelk_jpeg_resave_tables) and the coefficients (icelk_jpeg_resave_coefficients_host): jpeg_fwd.h on
//           the CPU, no handle, re-entrant; the code is jpeg_resave_host.h, plain C++ that a program without the library
//           can include (tests/jpeg_resave_host_main.cpp runs it under the host's sanitizers)
//   device  k_jpeg_fwd (the same header) -> k_jpeg_idct -> k_jpeg_out as they stand, fed with the re-save's tables: back
//           to the host as pixels (icelk_jpeg_resave_rgb), or as gray into a slot -- the _resave forms of the three
//           synchronous uploads, which differ only in how the cropped R G B gets into Ctx::Jpeg::d_src
#include <new>
#include <vector>

#include "icelk_ctx.h"
#include "jpeg_fwd.h"
#include "jpeg_resave_host.h"

namespace icelk {

using resave::resave_info;

void jpeg_resave_destroy(Ctx* c)
{
    Ctx::Jpeg& J = c->jpeg;
    jpeg_dec_free(J.resave);
    if (J.d_src) hipFree(J.d_src);
    J.d_src = nullptr;
    J.src_cap = 0;
}

// what the device entry points accept, checked before anything is enqueued
int jpeg_resave_check(Ctx* c, int w, int h, int quality)
{
    if (quality < 1 || quality > 100) FAIL(c, ICELK_EARG, "re-save quality outside 1 .. 100");
    if (w < 3) FAIL(c, ICELK_EARG, "re-save of an image less than 3 pixels wide");   // as the decoder: libjpeg's padding decides there
    if (h < 1 || w > 65535 || h > 65535) FAIL(c, ICELK_EARG, "re-save of an image no JPEG file holds");
    return ICELK_OK;
}

// The forward kernel on stream st: the w x h image at d_src (rows 3 w bytes apart) -> the coefficients of the re-saved
// file that I describes (resave_info) at d_coef.  The synchronous calls run it on the handle's re-save job, a job in flight
// (abi_jpeg_job.hip) on its own buffers.
static JpegFwdArgs fwd_args(const uint8_t* d_src, int16_t* d_coef, int w, int h, const icelk_jpeg_info_t& I)
{
    JpegFwdArgs F{};
    F.rgb = d_src;
    F.pitch = 3 * w;
    F.w = w;
    F.h = h;
    for (int k = 0; k < 3; k++) F.coef[k] = d_coef + I.coef_offset[k];
    F.mcus_x = I.mcus_x;
    F.mcus_y = I.mcus_y;
    F.real_bx = (w + 7) / 8;
    F.real_by = (h + 7) / 8;
    for (int t = 0; t < 2; t++)
        for (int i = 0; i < 64; i++) {
            F.quant[t][i] = I.quant[t][i];
            F.recip[t][i] = fwd::reciprocal((uint32_t)I.quant[t][i] << 3);
        }
    return F;
}

int jpeg_fwd_on(Ctx* c, hipStream_t st, const uint8_t* d_src, int16_t* d_coef, int w, int h, const icelk_jpeg_info_t& I)
{
    const JpegFwdArgs F = fwd_args(d_src, d_coef, w, h, I);
    {
        ProfScope p(c, K_JPEG_FWD, st);
        launch_jpeg_fwd(st, F);
    }
    return check_launch(c, "jpeg_fwd");
}

// The fused form on stream st: the crop box of the decoded planes `O` describes (O.ow x O.oh at O.left, O.top) -> the
// coefficients of the re-saved file that I describes at d_coef, with no R G B image in between.
int jpeg_crop_fwd_on(Ctx* c, hipStream_t st, const JpegOutArgs& O, int16_t* d_coef, const icelk_jpeg_info_t& I)
{
    const JpegFwdArgs F = fwd_args(nullptr, d_coef, O.ow, O.oh, I);
    {
        ProfScope p(c, K_JPEG_CROP_FWD, st);
        launch_jpeg_crop_fwd(st, O, F);
    }
    return check_launch(c, "jpeg_crop_fwd");
}

namespace {

int resave_slot_check(Ctx* c, int slot, int w, int h, int quality, int gray_variant)
{
    if (int rc = check_gray_variant(c, gray_variant)) return rc;
    if (int rc = check_slot(c, slot, false)) return rc;
    if (int rc = jpeg_resave_check(c, w, h, quality)) return rc;
    if (w > c->max_w || h > c->max_h) FAIL(c, ICELK_ECAP, "frame larger than max_w x max_h of icelk_create");
    return ICELK_OK;
}

int grow_src(Ctx* c, int w, int h) { return grow(c, &c->jpeg.d_src, &c->jpeg.src_cap, (size_t)3 * w * h); }

// a host image in R G B order -> d_src
int rgb_to_src(Ctx* c, const uint8_t* rgb, int w, int h, int stride)
{
    if (int rc = grow_src(c, w, h)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(c->jpeg.d_src, 3 * (size_t)w, rgb, stride, 3 * (size_t)w, h, hipMemcpyHostToDevice, c->stream));
    return ICELK_OK;
}

// d_src (w x h, rows 3 w bytes apart) -> the re-saved file's coefficients in the re-save job's d_coef; with_planes: and
// its component planes, `O` ready for k_jpeg_out
int resave_forward(Ctx* c, int w, int h, int quality, icelk_jpeg_info_t* I, JpegOutArgs* O, bool with_planes = true)
{
    Ctx::JpegDec& B = c->jpeg.resave;
    resave_info(w, h, quality, I);
    JpegIdctArgs D;
    if (int rc = jpeg_plane_args(c, B, I, 0, 0, 0, 0, &D, O)) return rc;   // grows d_coef and d_planes
    if (int rc = jpeg_fwd_on(c, c->stream, c->jpeg.d_src, B.d_coef, w, h, *I)) return rc;
    c->jpeg.enc.resaved = true;   // what icelk_jpeg_resave_encode writes the file of
    c->jpeg.enc.stream_ok = false;
    c->jpeg.enc.info = *I;
    if (!with_planes) return ICELK_OK;
    return jpeg_idct_on(c, c->stream, D);
}

// the tail of the three uploads: d_src -> gray of the re-saved image in `slot`
int resave_into_slot(Ctx* c, int slot, int w, int h, int quality, int gray_variant)
{
    icelk_jpeg_info_t I;
    JpegOutArgs O{};
    if (int rc = resave_forward(c, w, h, quality, &I, &O)) return rc;
    return planes_to_gray_slot(c, slot, O, gray_variant);   // O.ow x O.oh is w x h
}

// the cropped R G B of a decoded file (planes of the synchronous job, `O` of jpeg_planes) -> d_src
int planes_to_src(Ctx* c, JpegOutArgs& O)
{
    O.dst = c->jpeg.d_src;
    O.dst_pitch = 3 * O.ow;
    {
        ProfScope p(c, K_JPEG_OUT);
        launch_jpeg_rgb(c->stream, O);
    }
    return check_launch(c, "jpeg_out");
}

// descriptor and crop box of a described file, as jpeg_plane_args checks them; the cropped size
int cropped_size(Ctx* c, const icelk_jpeg_info_t* I, int left, int top, int right, int bottom, int* w, int* h)
{
    if (!I) FAIL(c, ICELK_EARG, "null JPEG descriptor or coefficients");
    if (I->ncomp != 3) FAIL(c, ICELK_EARG, "expected a 3-component JPEG file");
    if (!jpeg_info_ok(*I)) FAIL(c, ICELK_EARG, "JPEG descriptor does not describe a supported file");
    return check_crop_box(c, *I, left, top, right, bottom, w, h);
}

}  // namespace

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_jpeg_resave_tables(int quality, uint16_t* luma, uint16_t* chroma)
{
    if (!luma || !chroma || quality < 1 || quality > 100) return ICELK_EARG;
    resave::quality_tables(quality, luma, chroma);
    return ICELK_OK;
}

int icelk_jpeg_resave_divide_host(int q, uint32_t first, uint32_t count, uint32_t* out)
{
    if (!out || q < 1 || q > 255) return ICELK_EARG;
    const uint32_t m = fwd::reciprocal((uint32_t)q << 3);
    for (uint32_t i = 0; i < count; i++) out[i] = fwd::divide(first + i, m);
    return ICELK_OK;
}

int icelk_jpeg_resave_coefficients_host(const uint8_t* rgb, int w, int h, int stride, int quality, icelk_jpeg_info_t* info, int16_t* coef,
                                        uint64_t capacity)
{
    return resave::coefficients_host(rgb, w, h, stride, quality, info, coef, capacity);
}

int icelk_jpeg_resave_rgb(icelk_t* h, const uint8_t* rgb, int w, int h_, int stride, int quality, uint8_t* out, int out_stride)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!rgb || !out || stride < 3 * w || out_stride < 3 * w) FAIL(c, ICELK_EARG, "bad host image");
    if (int rc = jpeg_resave_check(c, w, h_, quality)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = rgb_to_src(c, rgb, w, h_, stride)) return rc;
    icelk_jpeg_info_t I;
    JpegOutArgs O{};
    if (int rc = resave_forward(c, w, h_, quality, &I, &O)) return rc;
    return jpeg_rgb_out(c, I, O, out, out_stride);
}

int icelk_jpeg_resave_device_coefficients(icelk_t* h, const uint8_t* rgb, int w, int h_, int stride, int quality, int16_t* coef,
                                          uint64_t capacity)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!rgb || !coef || stride < 3 * w) FAIL(c, ICELK_EARG, "bad host image or null coefficient buffer");
    if (int rc = jpeg_resave_check(c, w, h_, quality)) return rc;
    icelk_jpeg_info_t I;
    resave_info(w, h_, quality, &I);
    if (capacity < I.coef_count) FAIL(c, ICELK_ECAP, "coefficient buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = rgb_to_src(c, rgb, w, h_, stride)) return rc;
    JpegOutArgs O{};
    if (int rc = resave_forward(c, w, h_, quality, &I, &O, false)) return rc;
    HIPCHK(c, hipMemcpyAsync(coef, c->jpeg.resave.d_coef, (size_t)I.coef_count * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

int icelk_jpeg_crop_fwd_device_coefficients(icelk_t* h, const uint8_t* data, uint64_t len, int crop_left, int crop_top, int crop_right,
                                            int crop_bottom, int quality, int16_t* coef, uint64_t capacity)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!data || !coef) FAIL(c, ICELK_EARG, "null JPEG file or coefficient buffer");
    icelk_jpeg_info_t I, R;
    if (int rc = icelk_jpeg_describe(data, len, &I)) FAIL(c, rc, jpeg_open_error(rc));
    int w = 0, h_ = 0;
    if (int rc = cropped_size(c, &I, crop_left, crop_top, crop_right, crop_bottom, &w, &h_)) return rc;
    if (int rc = jpeg_resave_check(c, w, h_, quality)) return rc;
    resave_info(w, h_, quality, &R);
    if (capacity < R.coef_count) FAIL(c, ICELK_ECAP, "coefficient buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = jpeg_huff_device(c, data, len, &I)) return rc;
    JpegOutArgs O{};
    if (int rc = jpeg_planes(c, &I, nullptr, crop_left, crop_top, crop_right, crop_bottom, &O, true)) return rc;
    Ctx::JpegDec& B = c->jpeg.resave;
    if (int rc = grow(c, &B.d_coef, &B.coef_cap, (size_t)R.coef_count)) return rc;
    if (int rc = jpeg_crop_fwd_on(c, c->stream, O, B.d_coef, R)) return rc;
    c->jpeg.enc.resaved = true;   // as resave_forward: these are the handle's most recent re-saved coefficients
    c->jpeg.enc.stream_ok = false;
    c->jpeg.enc.info = R;
    HIPCHK(c, hipMemcpyAsync(coef, B.d_coef, (size_t)R.coef_count * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

int icelk_upload_bgr_resave(icelk_t* h, int slot, const uint8_t* host, int w, int h_, int stride, int gray_variant, int quality)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!host || stride < 3 * w) FAIL(c, ICELK_EARG, "bad host image");
    if (int rc = resave_slot_check(c, slot, w, h_, quality, gray_variant)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = rgb_to_src(c, host, w, h_, stride)) return rc;
    return resave_into_slot(c, slot, w, h_, quality, gray_variant);
}

int icelk_upload_jpeg_resave(icelk_t* h, int slot, const icelk_jpeg_info_t* info, const int16_t* coef, int gray_variant, int crop_left,
                             int crop_top, int crop_right, int crop_bottom, int quality)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    int w = 0, h_ = 0;
    if (!coef) FAIL(c, ICELK_EARG, "null JPEG descriptor or coefficients");
    if (int rc = cropped_size(c, info, crop_left, crop_top, crop_right, crop_bottom, &w, &h_)) return rc;
    if (int rc = resave_slot_check(c, slot, w, h_, quality, gray_variant)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = grow_src(c, w, h_)) return rc;
    JpegOutArgs O{};
    if (int rc = jpeg_planes(c, info, coef, crop_left, crop_top, crop_right, crop_bottom, &O)) return rc;
    if (int rc = planes_to_src(c, O)) return rc;
    return resave_into_slot(c, slot, w, h_, quality, gray_variant);
}

int icelk_upload_jpeg_file_resave(icelk_t* h, int slot, const uint8_t* data, uint64_t len, int gray_variant, int crop_left, int crop_top,
                                  int crop_right, int crop_bottom, int quality)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!data) FAIL(c, ICELK_EARG, "null JPEG file");
    icelk_jpeg_info_t I;
    if (int rc = icelk_jpeg_describe(data, len, &I)) FAIL(c, rc, jpeg_open_error(rc));
    int w = 0, h_ = 0;
    if (int rc = cropped_size(c, &I, crop_left, crop_top, crop_right, crop_bottom, &w, &h_)) return rc;
    if (int rc = resave_slot_check(c, slot, w, h_, quality, gray_variant)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = grow_src(c, w, h_)) return rc;
    if (int rc = jpeg_huff_device(c, data, len, &I)) return rc;
    JpegOutArgs O{};
    if (int rc = jpeg_planes(c, &I, nullptr, crop_left, crop_top, crop_right, crop_bottom, &O, true)) return rc;
    if (int rc = planes_to_src(c, O)) return rc;
    return resave_into_slot(c, slot, w, h_, quality, gray_variant);
}

}  // extern "C"
