// abi_jpeg_crop.hip -- the reference's crop step (camtools.py:64-104: open, crop, save again as JPEG) as a job of its own:
// icelk_jpeg_crop_config / _start / _poll / _finish / _cancel.  A file goes out in one piece on a decode stream, into
// buffers no frame slot has a share in, and comes back as the bytes Pillow's `crop.save(path)` writes:
//
//   start    the host's share (index, lanes, the checks of descriptor, crop box and re-save), the file into the job's pinned
//            staging area; then, without a wait: the Huffman decoder, inverse DCT, the crop box as R G B, the forward
//            kernel, the coder with its sizes left on the device (the _budget forms of k_jpeg_enc.hip), the verdict kernel
//   poll     a look at the job's pinned verdict words
//   finish   waits for the verdict and fetches the scan by one of three routes (device, host Huffman, over budget); then
//            header, scan and EOI go into the caller's buffer
//
// The driver is abi_jpeg_job.hip (JOB_CROP), shared with the look-ahead decoder (abi_jpeg_async.hip); its file header says
// what runs on a file that does not settle, or whose scan does not fit, and why that is safe.  What is the crop stage's
// own: the job belongs to a ticket, and poll answers 1 only when the coder's verdict is good as well.
#include <new>
#include <vector>

#include "icelk_ctx.h"
#include "jpeg_enc_host.h"

namespace icelk {

namespace {

Ctx::JpegJob* job_of_ticket(Ctx* c, int ticket)
{
    if (ticket < 1) return nullptr;
    for (Ctx::JpegJob* B : c->jpeg.ring)
        if (B->ticket == ticket) return B;
    return nullptr;
}

// the ticket is gone; what the job enqueued is through (the verdict has arrived or its stream was synchronised)
void release(Ctx::JpegJob& B)
{
    B.ticket = -1;
    B.have_scan = false;
}

}  // namespace

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_jpeg_enc_budget(uint32_t blocks, int stream_bytes_per_block, uint32_t total_bits, uint32_t invalid, uint32_t ff_total, uint32_t* out)
{
    if (!out || stream_bytes_per_block < enc::kMinBytesPerBlock || stream_bytes_per_block > enc::kMaxBytesPerBlock) return ICELK_EARG;
    if ((uint64_t)blocks * enc::kMaxBlockBits >= ((uint64_t)1 << 32)) return ICELK_ECAP;
    const uint32_t cap = enc::budget_cap(blocks, stream_bytes_per_block);
    out[0] = cap;
    out[1] = enc::chunks_of(cap);
    out[2] = enc::groups_of(out[1]);
    out[3] = enc::packed_bytes(total_bits);
    out[4] = enc::packed_fits(total_bits, invalid, cap);
    out[5] = enc::live_bytes(total_bits, invalid, cap);
    out[6] = enc::stuffed_fits(total_bits, invalid, ff_total, cap);
    out[7] = enc::budget_verdict(total_bits, invalid, ff_total, cap);
    return ICELK_OK;
}

int icelk_jpeg_encode_budgeted_host(const icelk_jpeg_info_t* info, const int16_t* coef, int stream_bytes_per_block, const uint32_t* force,
                                    uint32_t force_mask, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity,
                                    uint64_t* len, uint32_t* report)
{
    if (!len || !coef || !enc::comment_ok(comment, comment_len)) return ICELK_EARG;
    if (stream_bytes_per_block < enc::kMinBytesPerBlock || stream_bytes_per_block > enc::kMaxBytesPerBlock) return ICELK_EARG;
    enc::Layout L;
    if (int rc = enc::layout_of(info, &L)) return rc;
    const uint32_t cap = enc::budget_cap(L.blocks, stream_bytes_per_block);
    std::vector<uint8_t> packed, scan;
    try {
        packed.resize(cap);
        scan.resize(cap);
    } catch (...) {
        return ICELK_ENOMEM;
    }
    enc::BudgetWalk W;
    if (int rc = enc::encode_budgeted_host(info, coef, stream_bytes_per_block, force, force_mask, packed.data(), scan.data(), &W)) return rc;
    if (report) {
        const uint32_t r[8] = {W.cap, W.total_bits, W.invalid, W.ff_total, W.verdict, W.stuffed, W.packed_stores, W.out_stores};
        memcpy(report, r, sizeof(r));
    }
    *len = 0;
    if (W.verdict != enc::kCoded) return ICELK_OK;
    return enc::file_into(*info, comment, comment_len, scan.data(), W.stuffed, out, capacity, len);
}

int icelk_jpeg_crop_config(icelk_t* h, int stream_bytes_per_block)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (stream_bytes_per_block < enc::kMinBytesPerBlock || stream_bytes_per_block > enc::kMaxBytesPerBlock)
        FAIL(c, ICELK_EARG, "stream bytes per block outside 1 .. 416");
    c->jpeg.crop_bytes_per_block = stream_bytes_per_block;
    return ICELK_OK;
}

int icelk_jpeg_crop_start(icelk_t* h, const uint8_t* file, uint64_t len, int crop_left, int crop_top, int crop_right, int crop_bottom,
                          int quality, int* ticket)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Range rg("icelk jpeg_crop_start");
    if (!file || !ticket) FAIL(c, ICELK_EARG, "null JPEG file or ticket");
    HIPCHK(c, hipSetDevice(c->device));
    const JpegBox box{crop_left, crop_top, crop_right, crop_bottom};
    std::unique_ptr<JpegIndex> X;
    int idx = -1;
    enc::Layout L;
    if (int rc = jpeg_job_open(c, Ctx::JOB_CROP, true, file, len, box, quality, &X, &idx, &L)) return rc;
    Ctx::Jpeg& J = c->jpeg;
    Ctx::JpegJob& B = *J.ring[idx];
    if (int rc = jpeg_job_start(c, B, -1, file, len, *X, box, L)) {
        jpeg_job_abandon(B);
        return rc;
    }
    if (J.crop_next_ticket == 0x7fffffff) J.crop_next_ticket = 1;
    *ticket = B.ticket = J.crop_next_ticket++;
    return ICELK_OK;
}

int icelk_jpeg_crop_poll(icelk_t* h, int ticket, int* state)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!state) FAIL(c, ICELK_EARG, "null state");
    const Ctx::JpegJob* B = job_of_ticket(c, ticket);
    if (!B) FAIL(c, ICELK_ESTATE, "no crop job in flight under this ticket");
    *state = jpeg_job_state(*B, true);
    return ICELK_OK;
}

int icelk_jpeg_crop_finish(icelk_t* h, int ticket, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity,
                           uint64_t* len, icelk_jpeg_crop_stats_t* stats)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Range rg("icelk jpeg_crop_finish");
    if (!len || !enc::comment_ok(comment, comment_len)) FAIL(c, ICELK_EARG, "null length, or a comment no segment holds");
    Ctx::JpegJob* Bp = job_of_ticket(c, ticket);
    if (!Bp) FAIL(c, ICELK_ESTATE, "no crop job in flight under this ticket");
    Ctx::JpegJob& B = *Bp;
    HIPCHK(c, hipSetDevice(c->device));
    if (!B.have_scan) {
        if (int rc = jpeg_job_settle(c, B)) {
            // a failed launch or a damaged file: nothing of the job can be relied on
            hipStreamSynchronize(B.st);
            release(B);
            return rc;
        }
    }
    if (int rc = jpeg_job_file(c, B, comment, comment_len, out, capacity, len)) return rc;
    if (stats) *stats = B.cstats;
    release(B);
    return ICELK_OK;
}

int icelk_jpeg_crop_cancel(icelk_t* h, int ticket)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Ctx::JpegJob* B = job_of_ticket(c, ticket);
    if (!B) FAIL(c, ICELK_ESTATE, "no crop job in flight under this ticket");
    HIPCHK(c, hipSetDevice(c->device));
    const hipError_t e = B->st ? hipStreamSynchronize(B->st) : hipSuccess;
    release(*B);
    HIPCHK(c, e);
    return ICELK_OK;
}

}  // extern "C"
