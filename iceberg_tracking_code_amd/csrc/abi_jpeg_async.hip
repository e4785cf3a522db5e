// abi_jpeg_async.hip -- JPEG files decoded ahead of their frame: icelk_upload_jpeg_file_async / _poll / _finish.
//
// icelk_upload_jpeg_file (abi_jpeg_ingest.hip) decodes on the compute stream and has the host look at the decoder's flags
// three times per file, so a photo's decoding never runs beside the tracker step of the photo before it.  Here the same
// kernels go out in one piece on a decode stream of their own, into a slot the frame loop reaches later:
//
//   start    the host's share (index, lanes, the checks of descriptor, crop and slot), the file's bytes into pinned
//            memory of the job, then H2D copies, rounds 0 .. max_rounds, scan, write, DC, inverse DCT, the output kernel
//            into the slot's level 0, the verdict kernel (k_jpeg_huff.hip), the slot's events.  No wait.
//   poll     a look at the job's pinned verdict words.
//   finish   waits for the verdict.  "Decoded": nothing left to do.  Otherwise the host decoder reads the retained
//            bytes, its coefficients go into the job's own buffer and the transform and the output kernel run again.
//
// The driver is abi_jpeg_job.hip, shared with the crop stage (abi_jpeg_crop.hip); its file header says what runs on a file
// that does not settle and why that is safe.  What is the slot form's own: the job belongs to a slot (Jpeg::slot_job), what a
// finished slot keeps answering to poll (Jpeg::slot_state), and that a finish without a file redoes only the frame.
//
// The re-save form (icelk_upload_jpeg_file_async_resave): the slot gets the frame the reference tracks on, the crop saved
// again as a JPEG (quality, 4:2:0) and opened (JOB_SLOT_RESAVE); with want_file the budgeted coder of a crop job codes the
// re-saved coefficients behind it.  poll answers by the decoder's verdict alone: a scan over its budget concerns only the
// file.  finish runs everything behind the Huffman phases again (a wanted file is dropped); finish_file does so too and
// returns the file by the crop job's three routes.
#include "icelk_ctx.h"
#include "jpeg_enc_host.h"

namespace icelk {

// the job leaves its slot; `state`: what icelk_jpeg_async_poll keeps answering for the slot
static void release_job(Ctx* c, Ctx::JpegJob& B, int state)
{
    c->jpeg.slot_state[B.slot] = state;
    c->jpeg.slot_job[B.slot] = -1;
    B.slot = -1;
    B.want_file = B.have_scan = false;
}

// a failed launch or a damaged file at finish: nothing of the slot or the job can be relied on
static int drop_job(Ctx* c, Ctx::JpegJob& B, int rc)
{
    hipStreamSynchronize(B.st);
    c->slots[B.slot].levels_built = 0;
    release_job(c, B, 2);
    return rc;
}

static int job_of(Ctx* c, int slot, Ctx::JpegJob** B)
{
    *B = nullptr;
    if (int rc = check_slot(c, slot, false)) return rc;
    const Ctx::Jpeg& J = c->jpeg;
    if (!J.slot_job.empty() && J.slot_job[slot] >= 0) *B = J.ring[J.slot_job[slot]];
    return ICELK_OK;
}

}  // namespace icelk

using namespace icelk;

extern "C" {

// the start of both forms.  resave: the re-save form at `quality`; want_file: the job codes the crop's file as well
static int upload_async(icelk_t* h, int slot, const uint8_t* data, uint64_t len, int gray_variant, int crop_left, int crop_top,
                        int crop_right, int crop_bottom, bool resave, int quality, bool want_file)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Range rg("icelk upload_jpeg_file_async");
    if (int rc = check_gray_variant(c, gray_variant)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Ctx::JpegJob* old = nullptr;
    if (int rc = job_of(c, slot, &old)) return rc;
    if (old) FAIL(c, ICELK_ESTATE, "the slot's JPEG file is still in flight (icelk_jpeg_async_finish ends it)");
    if (!data) FAIL(c, ICELK_EARG, "null JPEG file");
    const JpegBox box{crop_left, crop_top, crop_right, crop_bottom};
    std::unique_ptr<JpegIndex> X;
    int idx = -1;
    enc::Layout L{};
    if (int rc = jpeg_job_open(c, resave ? Ctx::JOB_SLOT_RESAVE : Ctx::JOB_SLOT, want_file, data, len, box, quality, &X, &idx, &L)) return rc;
    Ctx::JpegJob& B = *c->jpeg.ring[idx];
    B.variant = gray_variant;
    if (int rc = jpeg_job_start(c, B, slot, data, len, *X, box, L)) {
        jpeg_job_abandon(B);
        return rc;
    }
    c->jpeg.slot_job[slot] = idx;
    c->jpeg.slot_state[slot] = 0;
    return ICELK_OK;
}

int icelk_upload_jpeg_file_async(icelk_t* h, int slot, const uint8_t* data, uint64_t len, int gray_variant, int crop_left,
                                 int crop_top, int crop_right, int crop_bottom)
{
    return upload_async(h, slot, data, len, gray_variant, crop_left, crop_top, crop_right, crop_bottom, false, 0, false);
}

int icelk_upload_jpeg_file_async_resave(icelk_t* h, int slot, const uint8_t* data, uint64_t len, int gray_variant, int crop_left,
                                        int crop_top, int crop_right, int crop_bottom, int quality, int want_file)
{
    return upload_async(h, slot, data, len, gray_variant, crop_left, crop_top, crop_right, crop_bottom, true, quality, want_file != 0);
}

int icelk_jpeg_async_poll(icelk_t* h, int slot, int* state)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!state) FAIL(c, ICELK_EARG, "null state");
    Ctx::JpegJob* B = nullptr;
    if (int rc = job_of(c, slot, &B)) return rc;
    if (!B) {
        if (c->jpeg.slot_state.empty() || c->jpeg.slot_state[slot] < 0) FAIL(c, ICELK_ESTATE, "no JPEG file was started into this slot");
        *state = c->jpeg.slot_state[slot];
        return ICELK_OK;
    }
    *state = jpeg_job_state(*B, false);
    return ICELK_OK;
}

int icelk_jpeg_async_finish(icelk_t* h, int slot, icelk_jpeg_huff_stats_t* stats)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Range rg("icelk jpeg_async_finish");
    HIPCHK(c, hipSetDevice(c->device));
    Ctx::JpegJob* Bp = nullptr;
    if (int rc = job_of(c, slot, &Bp)) return rc;
    if (!Bp) FAIL(c, ICELK_ESTATE, "no JPEG file in flight in this slot");
    Ctx::JpegJob& B = *Bp;
    if (B.have_scan) {
        // icelk_jpeg_async_finish_file has done all of it and ran out of room: the file is dropped
        const icelk_jpeg_huff_stats_t done = B.cstats.huff;
        release_job(c, B, done.fallback == ICELK_JPEG_FALLBACK_NONE ? 1 : 2);
        if (stats) *stats = done;
        return ICELK_OK;
    }
    icelk_jpeg_huff_stats_t st;
    if (int rc = jpeg_job_verdict(c, B, &st, nullptr)) return drop_job(c, B, rc);   // a failed launch
    const uint32_t why = st.fallback;
    int rc = ICELK_OK;
    if (why != ICELK_JPEG_FALLBACK_NONE) {
        rc = jpeg_job_redo_on_host(c, B, nullptr);
        // after an error the slot holds no frame; what the chain wrote into it is ordered in front of the next upload by
        // the slot's `ready` event, which stays pending
        if (rc) c->slots[slot].levels_built = 0;
    }
    release_job(c, B, why == ICELK_JPEG_FALLBACK_NONE ? 1 : 2);
    if (!rc && stats) *stats = st;
    return rc;
}

int icelk_jpeg_async_finish_file(icelk_t* h, int slot, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity,
                                 uint64_t* len, icelk_jpeg_crop_stats_t* stats)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Range rg("icelk jpeg_async_finish_file");
    if (!len || !enc::comment_ok(comment, comment_len)) FAIL(c, ICELK_EARG, "null length, or a comment no segment holds");
    HIPCHK(c, hipSetDevice(c->device));
    Ctx::JpegJob* Bp = nullptr;
    if (int rc = job_of(c, slot, &Bp)) return rc;
    if (!Bp) FAIL(c, ICELK_ESTATE, "no JPEG file in flight in this slot");
    Ctx::JpegJob& B = *Bp;
    if (!B.want_file) FAIL(c, ICELK_ESTATE, "the slot's JPEG file was started without a file to write");
    if (!B.have_scan)
        if (int rc = jpeg_job_settle(c, B)) return drop_job(c, B, rc);
    if (int rc = jpeg_job_file(c, B, comment, comment_len, out, capacity, len)) return rc;
    if (stats) *stats = B.cstats;
    release_job(c, B, B.cstats.huff.fallback == ICELK_JPEG_FALLBACK_NONE ? 1 : 2);
    return ICELK_OK;
}

}  // extern "C"
