// abi_jpeg_enc.hip -- the JPEG writer: the file Pillow's `img.save(path)` writes, from quantised coefficients.  With it
// the re-save (abi_jpeg_resave.hip) ends where the reference's crop step ends (camtools.py:64-104): in a file.
//
//   host    icelk_jpeg_encode_header, icelk_jpeg_encode_coefficients_host, icelk_jpeg_resave_file_host: jpeg_enc_host.h,
//           which walks the scan serially with jpeg_enc.h; no handle, re-entrant
//   device  icelk_jpeg_encode_coefficients (coefficients copied up) and icelk_jpeg_resave_encode (the coefficients the
//           forward kernel left in the re-save's d_coef; they never visit the host): k_jpeg_enc.hip --
//           count -> scan -> [host reads the total bit count and the validity flag] -> pack -> ff -> scan ->
//           [host reads the FF count] -> stuff -> header, stream and EOI into the caller's buffer.
//           Bit offsets are 32 bits wide: blocks * 1660 < 2^32 is checked before anything is enqueued (ICELK_ECAP;
//           a 12 MP 4:2:0 file has 281 000 blocks, the bound is 2.58 million).  The two reads are a stream
//           synchronisation each; the calls are synchronous anyway.
#include <new>
#include <vector>

#include "icelk_ctx.h"
#include "jpeg_enc_host.h"
#include "jpeg_resave_host.h"

namespace icelk {

void jpeg_enc_free(Ctx::JpegEnc& E)
{
    void* p[] = {E.d_codes, E.d_coef, E.d_bits, E.d_group, E.d_ctl, E.d_packed, E.d_ff, E.d_out};
    for (void* q : p)
        if (q) hipFree(q);
    if (E.h_ctl) hipHostFree(E.h_ctl);
    E = Ctx::JpegEnc{};
}

void jpeg_enc_destroy(Ctx* c) { jpeg_enc_free(c->jpeg.enc); }

void jpeg_resave_free(Ctx::JpegResave& R)
{
    if (R.d_rgb) hipFree(R.d_rgb);
    if (R.d_rcoef) hipFree(R.d_rcoef);
    jpeg_enc_free(R.enc);
    R = Ctx::JpegResave{};
}

int jpeg_enc_rc(Ctx* c, int rc)
{
    switch (rc) {
        case ICELK_OK: return rc;
        case ICELK_EUNSUP: FAIL(c, rc, "the writer takes no restart intervals and two quantisation tables at most");
        case ICELK_ECAP: FAIL(c, rc, "a scan of this many blocks does not fit 32-bit bit offsets");
        default: FAIL(c, rc, "the descriptor does not describe a file the writer takes");
    }
}

// what every coder has whatever the file: the control words on the device, their pinned copy, the tables
int jpeg_enc_prepare(Ctx* c, Ctx::JpegEnc& E)
{
    if (!E.d_ctl)
        if (int rc = dmalloc(c, &E.d_ctl, (size_t)JE_WORDS)) return rc;
    if (!E.h_ctl) HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&E.h_ctl), JE_WORDS * sizeof(uint32_t)));
    if (!E.d_codes) {
        uint32_t* codes = nullptr;
        if (int rc = dmalloc(c, &codes, (size_t)enc::kCodeWords)) return rc;
        hipError_t e = hipMemcpy(codes, &enc::codes(), sizeof(enc::Codes), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            hipFree(codes);
            HIPCHK(c, e);
        }
        E.d_codes = codes;
    }
    return ICELK_OK;
}

// The scan of the coefficients at d_coef (laid out as L says) -> E.d_out, E.stream_len, on stream st with the host reading
// the two sizes in between.  The synchronous calls run it on the handle's coder and compute stream, a crop job
// (abi_jpeg_job.hip) on its own where its budget did not hold the scan.
int jpeg_encode_on(Ctx* c, Ctx::JpegEnc& E, hipStream_t st, const enc::Layout& L, const int16_t* d_coef)
{
    E.stream_ok = false;
    if (int rc = jpeg_enc_prepare(c, E)) return rc;
    const uint32_t groups = (L.blocks + kJpegEncGroup - 1) / kJpegEncGroup;
    if (int rc = grow(c, &E.d_bits, &E.bits_cap, (size_t)L.blocks)) return rc;
    if (int rc = grow(c, &E.d_group, &E.group_cap, (size_t)groups)) return rc;
    JpegEncArgs A{};
    A.L = L;
    A.coef = d_coef;
    A.codes = E.d_codes;
    A.bits = E.d_bits;
    A.group = E.d_group;
    A.ctl = E.d_ctl;
    HIPCHK(c, hipMemsetAsync(E.d_ctl, 0, JE_WORDS * sizeof(uint32_t), st));
    {
        ProfScope p(c, K_JPEG_ENC_COUNT, st);
        launch_jpeg_enc_count(st, A);
    }
    if (int rc = check_launch(c, "jpeg_enc_count")) return rc;
    {
        ProfScope p(c, K_JPEG_ENC_SCAN, st);
        launch_jpeg_enc_scan(st, E.d_group, groups, E.d_ctl + JE_TOTAL_BITS);
    }
    if (int rc = check_launch(c, "jpeg_enc_scan")) return rc;
    HIPCHK(c, hipMemcpyAsync(E.h_ctl, E.d_ctl, JE_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (E.h_ctl[JE_INVALID]) FAIL(c, ICELK_EARG, "a coefficient that the standard Huffman tables have no code for");
    const uint32_t nbytes = (uint32_t)(((uint64_t)E.h_ctl[JE_TOTAL_BITS] + 7) / 8);
    const uint32_t nchunks = (nbytes + kJpegEncChunk - 1) / kJpegEncChunk, nwg = (nchunks + 255) / 256;
    if (int rc = grow(c, &E.d_packed, &E.packed_cap, (size_t)nchunks * (kJpegEncChunk / 4))) return rc;
    if (int rc = grow(c, &E.d_ff, &E.ff_cap, (size_t)nwg)) return rc;
    A.packed = E.d_packed;
    HIPCHK(c, hipMemsetAsync(E.d_packed, 0, (size_t)nchunks * kJpegEncChunk, st));
    {
        ProfScope p(c, K_JPEG_ENC_PACK, st);
        launch_jpeg_enc_pack(st, A);
    }
    if (int rc = check_launch(c, "jpeg_enc_pack")) return rc;
    {
        ProfScope p(c, K_JPEG_ENC_FF, st);
        launch_jpeg_enc_ff(st, E.d_packed, nchunks, E.d_ff);
    }
    if (int rc = check_launch(c, "jpeg_enc_ff")) return rc;
    {
        ProfScope p(c, K_JPEG_ENC_SCAN, st);
        launch_jpeg_enc_scan(st, E.d_ff, nwg, E.d_ctl + JE_FF_TOTAL);
    }
    if (int rc = check_launch(c, "jpeg_enc_scan")) return rc;
    HIPCHK(c, hipMemcpyAsync(E.h_ctl, E.d_ctl, JE_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const uint64_t len = (uint64_t)nbytes + E.h_ctl[JE_FF_TOTAL];
    if (int rc = grow(c, &E.d_out, &E.out_cap, (size_t)len)) return rc;
    {
        ProfScope p(c, K_JPEG_ENC_STUFF, st);
        launch_jpeg_enc_stuff(st, E.d_packed, nbytes, nchunks, E.d_ff, E.d_out);
    }
    if (int rc = check_launch(c, "jpeg_enc_stuff")) return rc;
    E.stream_len = len;
    return ICELK_OK;
}

// Header, E.d_out (E.stream_len bytes, copied on stream st, which is synchronised) and EOI into the caller's buffer.
// pending: st holds a copy into another buffer of the caller's, which a refusal has to wait for
int jpeg_deliver_file(Ctx* c, const Ctx::JpegEnc& E, hipStream_t st, bool pending, const icelk_jpeg_info_t& I, const uint8_t* comment,
                      uint64_t comment_len, uint8_t* out, uint64_t capacity, uint64_t* len)
{
    uint8_t* at = nullptr;
    if (enc::file_frame(I, comment, comment_len, E.stream_len, out, capacity, len, &at)) {
        if (pending) HIPCHK(c, hipStreamSynchronize(st));
        FAIL(c, ICELK_ECAP, "the file does not fit the buffer (len says what it takes)");
    }
    HIPCHK(c, hipMemcpyAsync(at, E.d_out, (size_t)E.stream_len, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return ICELK_OK;
}

namespace {

int encode_device(Ctx* c, const enc::Layout& L, const int16_t* d_coef) { return jpeg_encode_on(c, c->jpeg.enc, c->stream, L, d_coef); }

int deliver(Ctx* c, const icelk_jpeg_info_t& I, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity, uint64_t* len)
{
    return jpeg_deliver_file(c, c->jpeg.enc, c->stream, false, I, comment, comment_len, out, capacity, len);
}

}  // namespace

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_jpeg_encode_header(const icelk_jpeg_info_t* info, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity,
                             uint64_t* len)
{
    return enc::header_host(info, comment, comment_len, out, capacity, len);
}

int icelk_jpeg_encode_coefficients_host(const icelk_jpeg_info_t* info, const int16_t* coef, const uint8_t* comment, uint64_t comment_len,
                                        uint8_t* out, uint64_t capacity, uint64_t* len)
{
    return enc::encode_host(info, coef, comment, comment_len, out, capacity, len);
}

int icelk_jpeg_resave_file_host(const uint8_t* rgb, int w, int h_, int stride, int quality, const uint8_t* comment, uint64_t comment_len,
                                uint8_t* out, uint64_t capacity, uint64_t* len)
{
    icelk_jpeg_info_t I;
    if (int rc = resave::coefficients_host(rgb, w, h_, stride, quality, &I, nullptr, 0)) return rc;
    std::vector<int16_t> coef;
    try {
        coef.resize((size_t)I.coef_count);
    } catch (...) {
        return ICELK_ENOMEM;
    }
    if (int rc = resave::coefficients_host(rgb, w, h_, stride, quality, &I, coef.data(), coef.size())) return rc;
    return enc::encode_host(&I, coef.data(), comment, comment_len, out, capacity, len);
}

int icelk_jpeg_encode_coefficients(icelk_t* h, const icelk_jpeg_info_t* info, const int16_t* coef, const uint8_t* comment,
                                   uint64_t comment_len, uint8_t* out, uint64_t capacity, uint64_t* len)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!coef || !len || !enc::comment_ok(comment, comment_len)) FAIL(c, ICELK_EARG, "null coefficients or length, or a comment no segment holds");
    enc::Layout L;
    if (int rc = jpeg_enc_rc(c, enc::layout_of(info, &L))) return rc;
    Ctx::Jpeg::Enc& E = c->jpeg.enc;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = grow(c, &E.d_coef, &E.coef_cap, (size_t)info->coef_count)) return rc;
    HIPCHK(c, hipMemcpyAsync(E.d_coef, coef, (size_t)info->coef_count * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
    if (int rc = encode_device(c, L, E.d_coef)) return rc;
    return deliver(c, *info, comment, comment_len, out, capacity, len);
}

int icelk_jpeg_resave_encode(icelk_t* h, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity, uint64_t* len)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!len || !enc::comment_ok(comment, comment_len)) FAIL(c, ICELK_EARG, "null length, or a comment no segment holds");
    Ctx::Jpeg::Enc& E = c->jpeg.enc;
    if (!E.resaved) FAIL(c, ICELK_ESTATE, "the handle has not re-saved an image yet");
    HIPCHK(c, hipSetDevice(c->device));
    if (!E.stream_ok) {
        enc::Layout L;
        if (int rc = jpeg_enc_rc(c, enc::layout_of(&E.info, &L))) return rc;
        if (int rc = encode_device(c, L, c->jpeg.resave.d_coef)) return rc;
        E.stream_ok = true;   // kept until the next re-save, so that a call with a larger buffer need not encode again
    }
    return deliver(c, E.info, comment, comment_len, out, capacity, len);
}

}  // extern "C"
