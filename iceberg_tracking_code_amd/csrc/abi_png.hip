// abi_png.hip -- the PNG writer: an 8-bit R G B picture -> the file, with the pixels exact (the reference writes every
// picture as a PNG: s3:630-637).  The format, the filters, the tokens and the codes are png_enc.h.
//
//   host    icelk_png_bound, icelk_png_filter_host, icelk_png_encode_host: png_enc_host.h, serially; no handle, re-entrant
//   device  icelk_png_encode_rgb (pixels copied up) and, from abi_map.hip, icelk_map_draw_png (the R G B k_map_resolve
//           left on the device; it never visits the host).  On the caller's stream, in a working set of the coder's own
//           (Ctx::Png): the stream buffer zeroed, k_png_filter -> k_png_parse -> k_jpeg_enc_scan -> k_png_pack ->
//           k_png_adler (k_png.hip), with no host look in between; then ONE read of two words, the total bit count and the
//           Adler-32, and the deflate bytes straight into their place in the caller's buffer.  The host writes the
//           signature, IHDR, the chunk frames, the zlib header, the Adler-32 and the three CRC-32s, by table over the
//           delivered bytes (png_enc_host.h: file_frame, file_finish).
//           After ICELK_ECAP (*len says what the file takes) the call is simply repeated: the file is a function of the
//           picture.
// Sizes: 1 <= w, h <= 16384 and N = h (1 + 3 w) <= 2^28, refused before anything is allocated or enqueued (png_check);
// every buffer is sized from w and h alone, the stream to the bound of 9 bits per filtered byte.
//
// Bounds, store by store (n = N, S = png::kSegment, segments = ceil(n / S)):
//   k_png_filter   grid h; row y stores F[y pitch .. (y + 1) pitch) < n; reads rgb rows y - 1 (y > 0) and y, 3 w bytes each
//   k_png_parse    grid segments; reads F[s - 4 .. s + S) as dwords and F[s + i - pitch] for s + i >= pitch: below
//                  segments * S, what F holds; stores tok[s .. s + S) (as much is allocated), seg[segment], adler[3 segment ..]
//   k_png_pack     reads tok[s .. s + S), seg[segment]; stores stream dwords [start / 32, (end + 31) / 32) with
//                  end <= 3 + 9 n: below the (deflate_bytes(9 n) + 3) / 4 + 1 dwords allocated
//   k_png_adler    reads adler[0 .. 3 segments), stores ctl[PNG_ADLER]
#include "icelk_ctx.h"
#include "png_enc_host.h"

namespace icelk {

void png_destroy(Ctx* c)
{
    Ctx::Png& P = c->png;
    void* p[] = {P.d_src, P.d_F, P.d_tok, P.d_seg, P.d_adler, P.d_stream, P.d_ctl};
    for (void* q : p)
        if (q) hipFree(q);
    if (P.h_ctl) hipHostFree(P.h_ctl);
    P = Ctx::Png{};
}

int png_check(Ctx* c, int w, int h)
{
    if (!png::size_ok(w, h)) FAIL(c, ICELK_EARG, "a PNG's sides are 1 .. 16384 and its rows hold 2^28 filtered bytes at most");
    return ICELK_OK;
}

static size_t stream_dwords(uint32_t n) { return ((size_t)png::deflate_bytes(9u * n) + 3) / 4 + 1; }

// the working set of a w x h picture (png_check has passed)
int png_grow(Ctx* c, int w, int h)
{
    Ctx::Png& P = c->png;
    const uint32_t n = png::stream_of(w, h), segments = png::segments_of(n);
    if (!P.d_ctl)
        if (int rc = dmalloc(c, &P.d_ctl, (size_t)PNG_WORDS)) return rc;
    if (!P.h_ctl) HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&P.h_ctl), PNG_WORDS * sizeof(uint32_t)));
    if (int rc = grow(c, &P.d_F, &P.F_cap, (size_t)segments * png::kSegment)) return rc;
    if (int rc = grow(c, &P.d_tok, &P.tok_cap, (size_t)segments * png::kSegment)) return rc;
    if (int rc = grow(c, &P.d_seg, &P.seg_cap, (size_t)segments)) return rc;
    if (int rc = grow(c, &P.d_adler, &P.adler_cap, 3 * (size_t)segments)) return rc;
    return grow(c, &P.d_stream, &P.stream_cap, stream_dwords(n));
}

// The picture at d_rgb (device memory, rows `stride` bytes apart) -> P.d_stream, on stream st, which is synchronised;
// *nbytes: the deflate block's.  png_check and png_grow have passed for w x h
int png_encode_on(Ctx* c, hipStream_t st, const uint8_t* d_rgb, uint32_t stride, int w, int h, uint32_t* nbytes)
{
    Ctx::Png& P = c->png;
    PngArgs A{};
    A.rgb = d_rgb, A.stride = stride, A.w = w, A.h = h;
    A.n = png::stream_of(w, h), A.pitch = png::pitch_of(w);
    A.F = P.d_F, A.tok = P.d_tok, A.seg = P.d_seg, A.adler = P.d_adler, A.stream = P.d_stream, A.ctl = P.d_ctl;
    const uint32_t segments = png::segments_of(A.n);
    HIPCHK(c, hipMemsetAsync(P.d_ctl, 0, PNG_WORDS * sizeof(uint32_t), st));
    HIPCHK(c, hipMemsetAsync(P.d_stream, 0, stream_dwords(A.n) * sizeof(uint32_t), st));
    {
        ProfScope p(c, K_PNG_FILTER, st);
        launch_png_filter(st, A);
    }
    if (int rc = check_launch(c, "png_filter")) return rc;
    {
        ProfScope p(c, K_PNG_PARSE, st);
        launch_png_parse(st, A);
    }
    if (int rc = check_launch(c, "png_parse")) return rc;
    {
        ProfScope p(c, K_PNG_SCAN, st);
        launch_jpeg_enc_scan(st, P.d_seg, segments, P.d_ctl + PNG_TOTAL_BITS);
    }
    if (int rc = check_launch(c, "png_scan")) return rc;
    {
        ProfScope p(c, K_PNG_PACK, st);
        launch_png_pack(st, A);
    }
    if (int rc = check_launch(c, "png_pack")) return rc;
    {
        ProfScope p(c, K_PNG_ADLER, st);
        launch_png_adler(st, P.d_adler, segments, P.d_ctl + PNG_ADLER);
    }
    if (int rc = check_launch(c, "png_adler")) return rc;
    HIPCHK(c, hipMemcpyAsync(P.h_ctl, P.d_ctl, PNG_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    *nbytes = png::deflate_bytes(P.h_ctl[PNG_TOTAL_BITS]);
    return ICELK_OK;
}

// The file around P.d_stream (nbytes, copied on stream st, which is synchronised) into the caller's buffer.
// pending: st holds a copy into another buffer of the caller's, which a refusal has to wait for
int png_deliver_file(Ctx* c, hipStream_t st, bool pending, int w, int h, uint32_t nbytes, uint8_t* out, uint64_t capacity, uint64_t* len)
{
    const Ctx::Png& P = c->png;
    uint8_t* at = nullptr;
    if (png::file_frame(w, h, nbytes, out, capacity, len, &at)) {
        if (pending) HIPCHK(c, hipStreamSynchronize(st));
        FAIL(c, ICELK_ECAP, "the file does not fit the buffer (len says what it takes)");
    }
    HIPCHK(c, hipMemcpyAsync(at, P.d_stream, (size_t)nbytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    png::file_finish(out, nbytes, P.h_ctl[PNG_ADLER]);
    return ICELK_OK;
}

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_png_bound(int w, int h_, uint64_t* bytes)
{
    if (!bytes || !png::size_ok(w, h_)) return ICELK_EARG;
    *bytes = png::bound_of(w, h_);
    return ICELK_OK;
}

int icelk_png_filter_host(const uint8_t* rgb, int w, int h_, int stride, uint8_t* out) { return png::filter_host(rgb, w, h_, stride, out); }

int icelk_png_encode_host(const uint8_t* rgb, int w, int h_, int stride, uint8_t* out, uint64_t capacity, uint64_t* len)
{
    return png::encode_host(rgb, w, h_, stride, out, capacity, len);
}

int icelk_png_encode_rgb(icelk_t* h, const uint8_t* rgb, int w, int h_, int stride, uint8_t* out, uint64_t capacity, uint64_t* len)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Range rg("icelk png_encode_rgb");
    if (!rgb || !len) FAIL(c, ICELK_EARG, "null pixels or length");
    if (int rc = png_check(c, w, h_)) return rc;
    if (stride < 3 * w) FAIL(c, ICELK_EARG, "rgb stride smaller than 3 x the picture's width");
    HIPCHK(c, hipSetDevice(c->device));
    Ctx::Png& P = c->png;
    if (int rc = grow(c, &P.d_src, &P.src_cap, 3 * (size_t)w * h_)) return rc;
    if (int rc = png_grow(c, w, h_)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(P.d_src, 3 * (size_t)w, rgb, (size_t)stride, 3 * (size_t)w, (size_t)h_, hipMemcpyHostToDevice, c->stream));
    uint32_t nbytes = 0;
    if (int rc = png_encode_on(c, c->stream, P.d_src, 3u * (uint32_t)w, w, h_, &nbytes)) return rc;
    return png_deliver_file(c, c->stream, false, w, h_, nbytes, out, capacity, len);
}

}  // extern "C"
