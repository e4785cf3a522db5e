// abi_movie.hip -- the movie of the day's pictures (s1:452-473, s3:194-215, imports/timelapse.sh): every picture the
// writer has drawn becomes a frame, scaled to the movie's size and coded as a baseline JPEG on the device.  The container
// (a Motion-JPEG AVI) is written by movie.py; here are the scaler and the frame.  DESIGN.md 7.11 has the rule.
//
//   host    icelk_movie_size, icelk_resize_host: resize.h on the CPU; no handle, re-entrant
//   device  resize_on: the axes' tables (made on the host by resize::make_axis, the code icelk_resize_host runs, cached on
//           the handle by (in, out)), then k_resize_rows into a buffer between the passes and k_resize_cols out of it
//           (k_resize.hip); a pass whose sizes agree is skipped, with both skipped the picture is copied.
//           icelk_resize_rgb: host pixels up, resize_on, pixels down.
//           icelk_picture_frame: the R G B the picture writer drew last, still resident in c->picture.d_rgb, through
//           resize_on into the frame's own R G B, and that through the writer's forward kernel and entropy coder: no pixel
//           crosses PCIe, only the tables go up, once per size, and the coded frame comes down.
//           Every call runs on the handle's compute stream and waits for the device.
//
// Bounds.  Every buffer is sized before anything is enqueued: the source 3 w h bytes (rows 3 w apart), between the passes
// (hi - lo) rows of pitch 3 ow rounded up to a dword, lo .. hi - 1 the source rows the vertical table reads, the result
// 3 ow oh bytes padded as picture_grow pads a picture.  An axis' table holds out + out + out pitch words.  k_resize.hip's
// header states the kernels' loads and stores against these.
#include "icelk_ctx.h"
#include "jpeg_enc_host.h"
#include "jpeg_resave_host.h"

namespace icelk {

void movie_destroy(Ctx* c)
{
    Ctx::Movie& M = c->movie;
    for (auto& A : M.axis) {
        if (A.d) hipFree(A.d);
        A = Ctx::Movie::Axis{};
    }
    for (uint8_t** p : {&M.d_mid, &M.d_src, &M.d_out}) {
        if (*p) hipFree(*p);
        *p = nullptr;
    }
    M.mid_cap = M.src_cap = M.out_cap = 0;
    jpeg_resave_free(M.frame);
    M.frame = Ctx::JpegResave{};
}

namespace {

size_t pad4(size_t v) { return (v + 3) & ~(size_t)3; }

// axis `which` of the handle holds the table of in -> out, uploaded on st unless it already does
int axis_on(Ctx* c, hipStream_t st, int which, int in, int out, ResizeAxis* T)
{
    Ctx::Movie::Axis& A = c->movie.axis[which];
    if (!A.valid || A.host.in != in || A.host.out != out) {
        A.valid = false;
        try {
            resize::make_axis(in, out, &A.host);
        } catch (...) {
            FAIL(c, ICELK_ENOMEM, "no memory for an axis' table");
        }
        const size_t n = (size_t)out;
        if (int rc = grow(c, &A.d, &A.cap, 2 * n + n * A.host.pitch)) return rc;
        HIPCHK(c, copy_n(A.d, A.host.first.data(), n, kH2D, st));
        HIPCHK(c, copy_n(A.d + n, A.host.count.data(), n, kH2D, st));
        HIPCHK(c, copy_n(A.d + 2 * n, A.host.k.data(), n * A.host.pitch, kH2D, st));
        A.valid = true;
    }
    *T = ResizeAxis{A.d, A.d + out, A.d + 2 * (size_t)out, A.host.pitch};
    return ICELK_OK;
}

// w x h at d_src (rows src_pitch apart) -> ow x oh at d_dst (rows dst_pitch apart), on st; sides checked by the caller
int resize_on(Ctx* c, hipStream_t st, const uint8_t* d_src, size_t src_pitch, int w, int h, int ow, int oh, uint8_t* d_dst, size_t dst_pitch)
{
    Ctx::Movie& M = c->movie;
    const bool across = w != ow, down = h != oh;
    if (!across && !down) {
        HIPCHK(c, hipMemcpy2DAsync(d_dst, dst_pitch, d_src, src_pitch, 3 * (size_t)w, h, hipMemcpyDeviceToDevice, st));
        return ICELK_OK;
    }
    ResizeAxis X{}, Y{};
    if (across)
        if (int rc = axis_on(c, st, 0, w, ow, &X)) return rc;
    if (down)
        if (int rc = axis_on(c, st, 1, h, oh, &Y)) return rc;
    const int lo = down ? M.axis[1].host.lo : 0, hi = down ? M.axis[1].host.hi : h;
    const uint8_t* rows = d_src + (size_t)lo * src_pitch;   // what the vertical pass reads: row lo first
    size_t rows_pitch = src_pitch;
    if (across) {
        uint8_t* dst = d_dst;
        size_t pitch = dst_pitch;
        if (down) {
            pitch = pad4(3 * (size_t)ow);
            if (int rc = grow(c, &M.d_mid, &M.mid_cap, (size_t)(hi - lo) * pitch)) return rc;
            dst = M.d_mid;
        }
        {
            ProfScope p(c, K_RESIZE_ROWS, st);
            launch_resize_rows(st, rows, src_pitch, hi - lo, X, ow, dst, pitch);
        }
        if (int rc = check_launch(c, "resize_rows")) return rc;
        rows = dst, rows_pitch = pitch;
    }
    if (down) {
        {
            ProfScope p(c, K_RESIZE_COLS, st);
            launch_resize_cols(st, rows, rows_pitch, lo, Y, ow, oh, d_dst, dst_pitch);
        }
        if (int rc = check_launch(c, "resize_cols")) return rc;
    }
    return ICELK_OK;
}

bool sides_ok(int w, int h, int ow, int oh) { return resize::side_ok(w) && resize::side_ok(h) && resize::side_ok(ow) && resize::side_ok(oh); }

}  // namespace

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_movie_size(int w, int h_, int movie_width, int* mw, int* mh)
{
    if (!mw || !mh || !resize::movie_size(w, h_, movie_width, mw, mh)) return ICELK_EARG;
    return ICELK_OK;
}

int icelk_resize_host(const uint8_t* rgb, int w, int h_, int stride, int ow, int oh, uint8_t* out, int out_stride)
{
    if (!rgb || !out || !sides_ok(w, h_, ow, oh) || stride < 3 * w || out_stride < 3 * ow) return ICELK_EARG;
    try {
        resize::resize_host(rgb, w, h_, (size_t)stride, ow, oh, out, (size_t)out_stride);
    } catch (...) {
        return ICELK_ENOMEM;
    }
    return ICELK_OK;
}

int icelk_resize_rgb(icelk_t* h, const uint8_t* rgb, int w, int h_, int stride, int ow, int oh, uint8_t* out, int out_stride)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!rgb || !out) FAIL(c, ICELK_EARG, "null picture or null result");
    if (!sides_ok(w, h_, ow, oh)) FAIL(c, ICELK_EARG, "a side outside 1 .. 16384");
    if (stride < 3 * w || out_stride < 3 * ow) FAIL(c, ICELK_EARG, "a stride smaller than 3 x the width");
    HIPCHK(c, hipSetDevice(c->device));
    Ctx::Movie& M = c->movie;
    const size_t row = 3 * (size_t)w, orow = 3 * (size_t)ow;
    if (int rc = grow(c, &M.d_src, &M.src_cap, row * h_)) return rc;
    if (int rc = grow(c, &M.d_out, &M.out_cap, orow * oh)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(M.d_src, row, rgb, (size_t)stride, row, h_, hipMemcpyHostToDevice, c->stream));
    if (int rc = resize_on(c, c->stream, M.d_src, row, w, h_, ow, oh, M.d_out, orow)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(out, (size_t)out_stride, M.d_out, orow, orow, oh, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

int icelk_picture_size(icelk_t* h, int* w, int* h_)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!w || !h_) FAIL(c, ICELK_EARG, "null size");
    if (c->picture_w < 1) FAIL(c, ICELK_ESTATE, "the handle has drawn no picture yet");
    *w = c->picture_w, *h_ = c->picture_h;
    return ICELK_OK;
}

int icelk_picture_frame(icelk_t* h, int ow, int oh, int quality, uint8_t* rgb_or_null, int rgb_stride, uint8_t* file, uint64_t capacity,
                        uint64_t* len)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!resize::side_ok(ow) || !resize::side_ok(oh)) FAIL(c, ICELK_EARG, "a frame with a side outside 1 .. 16384");
    PictureFile F;
    if (int rc = picture_check(c, ow, oh, PICTURE_JPEG, quality, rgb_or_null, rgb_stride, len, &F)) return rc;
    if (c->picture_w < 1) FAIL(c, ICELK_ESTATE, "the handle has drawn no picture yet");
    HIPCHK(c, hipSetDevice(c->device));
    Ctx::JpegResave& R = c->movie.frame;
    if (int rc = grow(c, &R.d_rgb, &R.rgb_cap, 3 * F.px)) return rc;
    if (int rc = grow(c, &R.d_rcoef, &R.rcoef_cap, (size_t)F.info.coef_count)) return rc;
    hipStream_t st = c->stream;
    const size_t row = 3 * (size_t)ow;
    if (int rc = resize_on(c, st, c->picture.d_rgb, 3 * (size_t)c->picture_w, c->picture_w, c->picture_h, ow, oh, R.d_rgb, row)) return rc;
    if (int rc = jpeg_fwd_on(c, st, R.d_rgb, R.d_rcoef, ow, oh, F.info)) return rc;
    if (int rc = jpeg_encode_on(c, R.enc, st, F.L, R.d_rcoef)) return rc;
    if (rgb_or_null) HIPCHK(c, hipMemcpy2DAsync(rgb_or_null, rgb_stride, R.d_rgb, row, row, oh, hipMemcpyDeviceToHost, st));
    return jpeg_deliver_file(c, R.enc, st, rgb_or_null != nullptr, F.info, nullptr, 0, file, capacity, len);
}

}  // extern "C"
