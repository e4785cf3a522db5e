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
// What runs on a file that does not settle.  The host cannot stop the chain, so scan, write, DC pass, transform and
// output kernel run on whatever the rounds left.  That is safe by the construction of jpeg_lanes.h, which is what is
// relied on here: decode() is total and reads no byte outside its segment; a lane decodes the bits of its own
// subsequence only, so its loop ends; write_lane clamps its first block to the segment's blocks and every store goes
// to block_base(g) with g < total_blocks, at a zigzag position < 64; the DC pass and the transform walk the image's
// blocks, not the stream (tests/jpeg_lanes_states.cpp runs this order and arbitrary states on the CPU, under the host's
// sanitizers).  What they leave in the job's buffers and in the slot is garbage that nobody may consume:
// the slot counts as filled only after finish has returned ICELK_OK, and finish overwrites all of it.
//
// The re-save form (icelk_upload_jpeg_file_async_resave): the slot gets the frame the reference tracks on, the crop saved
// again as a JPEG (quality, 4:2:0) and opened.  Behind the source's inverse DCT the chain goes on with the fused kernel
// (k_jpeg_crop_fwd, k_jpeg_fwd.hip: the crop box of the planes -> the re-saved file's coefficients in d_rcoef, no R G B image
// in between), the inverse DCT of THOSE into planes of the job's own (d_planes2), the output kernel from them into the
// slot's level 0; with want_file the budgeted coder of a crop job (abi_jpeg_crop.hip) codes d_rcoef behind it, and the
// verdict kernel is the crop job's, the coder's words "not asked" without a file.  poll answers by the decoder's verdict
// alone: a scan over its budget concerns only the file.  On a file that does not settle the fused kernel reads the planes
// at clamped coordinates inside them and stores whole blocks of the re-saved layout (its file header says why), the second
// inverse DCT walks that layout, and the coder's stores are bounded by the budget for ANY contents of its control words
// (the header of abi_jpeg_crop.hip): the same garbage-nobody-consumes as above.  finish runs everything behind the Huffman
// phases again (a wanted file is dropped); finish_file does so too and returns the file by the crop job's three routes.
//
// Jobs.  Every file in flight owns one Ctx::JpegJob (device buffers as the synchronous calls' job, plus the pinned
// staging area and the pinned verdict words) from start to finish; the ring grows when every job is in flight and is
// never sized by the frame maximum.  A job's kernels are through when its verdict has arrived (the verdict kernel is
// the last of the chain) or finish has synchronised its stream, so a freed job can go out on the other stream at once.
#include "icelk_ctx.h"
#include "jpeg_enc_host.h"
#include "jpeg_resave_host.h"

namespace icelk {

static void free_job(Ctx::JpegJob* B)
{
    void* p[] = {B->d_coef, B->d_planes, B->d_file, B->d_seg, B->d_tabs, B->d_T, B->d_X, B->d_cnt, B->d_P, B->d_ctl, B->d_dc, B->d_rgb, B->d_rcoef, B->d_planes2};
    for (void* q : p)
        if (q) hipFree(q);
    jpeg_enc_free(B->enc);
    if (B->h_out) hipHostFree(B->h_out);
    if (B->h_stage) hipHostFree(B->h_stage);
    if (B->h_verdict) hipHostFree(B->h_verdict);
    if (B->done) hipEventDestroy(B->done);
    delete B;
}

// icelk_destroy: files in flight are waited for, nobody will finish them
void jpeg_async_destroy(Ctx* c)
{
    for (auto& q : c->jpeg.dec)
        if (q) {
            hipStreamSynchronize(q);
            hipStreamDestroy(q);
            q = nullptr;
        }
    if (c->jpeg.fetch) {
        hipStreamSynchronize(c->jpeg.fetch);
        hipStreamDestroy(c->jpeg.fetch);
        c->jpeg.fetch = nullptr;
    }
    for (Ctx::JpegJob* B : c->jpeg.ring) free_job(B);
    c->jpeg.ring.clear();
}

// icelk_sync: the decode streams count as streams of the handle; the jobs stay their slots' until finish
int jpeg_async_sync(Ctx* c)
{
    for (auto q : c->jpeg.dec)
        if (q) HIPCHK(c, hipStreamSynchronize(q));
    return ICELK_OK;
}

// a job that neither a slot nor a ticket (abi_jpeg_crop.hip) owns; a new one when all are in flight
int jpeg_take_job(Ctx* c, int* idx)
{
    Ctx::Jpeg& J = c->jpeg;
    for (size_t k = 0; k < J.ring.size(); k++)
        if (J.ring[k]->slot < 0 && J.ring[k]->ticket < 0) return *idx = (int)k, ICELK_OK;
    Ctx::JpegJob* B = new (std::nothrow) Ctx::JpegJob;
    if (!B) FAIL(c, ICELK_ENOMEM, "no memory for a JPEG job");
    if (hipHostMalloc(reinterpret_cast<void**>(&B->h_verdict), JV_WORDS * sizeof(uint32_t), hipHostMallocMapped) != hipSuccess ||
        hipEventCreateWithFlags(&B->done, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        free_job(B);
        FAIL(c, ICELK_ENOMEM, "no pinned memory for a JPEG job");
    }
    memset(B->h_verdict, 0, JV_WORDS * sizeof(uint32_t));
    try {
        J.ring.push_back(B);
    } catch (...) {
        free_job(B);
        FAIL(c, ICELK_ENOMEM, "no memory for a JPEG job");
    }
    return *idx = (int)J.ring.size() - 1, ICELK_OK;
}

// the decode streams, created at the first asynchronous file: two in turn, as Ctx::copy_hi (abi_frames.hip)
int jpeg_decode_stream(Ctx* c, hipStream_t* out)
{
    Ctx::Jpeg& J = c->jpeg;
    const unsigned k = J.dec_seq++ % (unsigned)J.dec_streams;
    if (!J.dec[k]) {
        if (J.dec_high) HIPCHK(c, create_priority_stream(&J.dec[k]));
        else HIPCHK(c, hipStreamCreateWithFlags(&J.dec[k], hipStreamNonBlocking));
    }
    *out = J.dec[k];
    return ICELK_OK;
}

// inverse DCT and output kernel of job B into its slot's level 0, on the job's stream
static int transform_into_slot(Ctx* c, Ctx::JpegJob& B)
{
    if (int rc = jpeg_idct_on(c, B.st, B.idct)) return rc;
    if (!B.resave) return jpeg_gray_on(c, B.st, B.out, c->slots[B.slot], B.variant);
    if (int rc = jpeg_crop_fwd_on(c, B.st, B.out, B.d_rcoef, B.rinfo)) return rc;
    if (int rc = jpeg_idct_on(c, B.st, B.ridct)) return rc;
    return jpeg_gray_on(c, B.st, B.rout, c->slots[B.slot], B.variant);
}

// the job leaves its slot; `state`: what icelk_jpeg_async_poll keeps answering for the slot
static void release_job(Ctx* c, Ctx::JpegJob& B, int state)
{
    c->jpeg.slot_state[B.slot] = state;
    c->jpeg.slot_job[B.slot] = -1;
    B.slot = -1;
    B.resave = B.want_file = B.have_scan = false;
}

// The job's pinned staging area: tables | segment table | file.  The copies of a start read it when the stream gets there,
// and the host decoder reads the file from it at finish: the caller's buffer is free when the start returns.  The tables
// and the segment table are copied in by the caller once it knows that something goes out.
int jpeg_stage_file(Ctx* c, Ctx::JpegJob& B, const JpegIndex& X, size_t seg_bytes, const uint8_t* data, uint64_t len)
{
    const size_t file_off = (sizeof(X.tabs) + seg_bytes + 255) & ~(size_t)255, want = file_off + (size_t)len;
    if (B.stage_cap < want) {
        const size_t take = want + want / 4;   // headroom as jpeg_huff_setup's
        if (B.h_stage) HIPCHK(c, hipHostFree(B.h_stage));
        B.h_stage = nullptr;
        B.stage_cap = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&B.h_stage), take, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            FAIL(c, ICELK_ENOMEM, "no pinned memory for the JPEG file");
        }
        B.stage_cap = take;
    }
    B.file_off = file_off;
    B.len = len;
    memcpy(B.h_stage + file_off, data, (size_t)len);
    return ICELK_OK;
}

static int start_job(Ctx* c, Ctx::JpegJob& B, int slot, const uint8_t* data, uint64_t len, JpegIndex& X, int left, int top, int right,
                     int bottom, const enc::Layout* L = nullptr)
{
    Ctx::Jpeg& J = c->jpeg;
    const bool host_only = B.host_only;
    if (int rc = jpeg_plane_args(c, B, &B.info, left, top, right, bottom, &B.idct, &B.out)) return rc;
    // begin_frame's check, taken before anything is allocated for the file
    if (B.out.ow > c->max_w || B.out.oh > c->max_h) FAIL(c, ICELK_ECAP, "frame larger than max_w x max_h of icelk_create");
    JpegHuffArgs H{};
    size_t seg_bytes = 0;
    if (!host_only) {
        jpeg_index_lanes(X, (uint32_t)J.subseq_bits, J.max_hops);
        if (int rc = jpeg_huff_setup(c, B, X, len, &H, true)) return rc;
        seg_bytes = X.seg.size() * sizeof(lanes::Seg);
    }
    if (int rc = jpeg_stage_file(c, B, X, seg_bytes, data, len)) return rc;
    if (B.resave) {
        if (int rc = grow(c, &B.d_rcoef, &B.rcoef_cap, (size_t)B.rinfo.coef_count)) return rc;
        if (int rc = grow(c, &B.d_planes2, &B.planes2_cap, jpeg_plane_bytes(B.rinfo))) return rc;
        jpeg_plane_layout(B.rinfo, 0, 0, 0, 0, B.d_rcoef, B.d_planes2, &B.ridct, &B.rout);
        if (B.want_file) {
            B.budget = enc::budget_cap(L->blocks, J.crop_bytes_per_block);
            if (int rc = jpeg_budget_buffers(c, B, *L)) return rc;
        }
    }
    if (int rc = jpeg_decode_stream(c, &B.st)) return rc;
    // from here on the slot is taken: whatever fails below leaves it without a frame
    if (int rc = begin_frame(c, slot, B.out.ow, B.out.oh)) return rc;
    B.slot = slot;
    Slot& s = c->slots[slot];
    const hipStream_t st = B.st;
    if (int rc = foreign_write_begin(c, s, st)) return rc;   // the slot is left as icelk_upload_gray_async leaves it
    if (host_only) return ICELK_OK;   // nothing goes out before finish, which has the host decoder take the file
    memcpy(B.h_stage, X.tabs, sizeof(X.tabs));
    memcpy(B.h_stage + sizeof(X.tabs), X.seg.data(), seg_bytes);
    B.segments = X.scan.nseg;
    B.subsequences = X.scan.nlanes;
    if (int rc = jpeg_huff_stage(c, B, X, B.h_stage + B.file_off, B.h_stage + sizeof(X.tabs), B.h_stage, len, st)) return rc;
    {
        // every round at once: one that no group takes part in returns after two loads per workgroup
        ProfScope p(c, K_JPEG_HUFF, st);
        for (int q = 0; q <= J.max_rounds; q++) launch_jpeg_huff_sync(st, H, q);
        jpeg_huff_finish_phases(st, H);
    }
    if (int rc = check_launch(c, "jpeg_huff")) return rc;
    if (int rc = transform_into_slot(c, B)) return rc;
    if (B.want_file)
        if (int rc = jpeg_encode_budgeted(c, B, *L)) return rc;
    B.seq = (B.seq + 1) & 0x3fffffffu;
    if (B.resave) {
        ProfScope p(c, K_JPEG_CROP_VERDICT, st);
        launch_jpeg_crop_verdict(st, B.d_ctl, J.max_rounds, B.want_file ? B.enc.d_ctl : nullptr, B.budget, B.h_verdict, B.seq);
    } else {
        launch_jpeg_huff_verdict(st, B.d_ctl, J.max_rounds, B.h_verdict, B.seq);
    }
    if (int rc = check_launch(c, B.resave ? "jpeg_crop_verdict" : "jpeg_huff_verdict")) return rc;
    HIPCHK(c, hipEventRecord(B.done, st));
    return foreign_write_end(c, s, st);
}

bool jpeg_verdict_here(const Ctx::JpegJob& B)
{
    return __atomic_load_n(B.h_verdict + JV_SEQ, __ATOMIC_ACQUIRE) == B.seq;
}

// Waits for the verdict by polling the pinned sequence word, as fetch_counts (abi_detect.hip): the event is looked at
// now and then, so that a failed launch ends the wait with its error instead of hanging it.
int jpeg_await_verdict(Ctx* c, Ctx::JpegJob& B)
{
    for (unsigned it = 1;; it++) {
        if (jpeg_verdict_here(B)) return ICELK_OK;
        if ((it & 4095u) == 0) {
            const hipError_t q = hipEventQuery(B.done);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) HIPCHK(c, q);
            (void)hipGetLastError();
        }
        __builtin_ia32_pause();
    }
    HIPCHK(c, hipEventSynchronize(B.done));
    if (!jpeg_verdict_here(B)) FAIL(c, ICELK_EHIP, "the JPEG verdict did not arrive");
    return ICELK_OK;
}

// the decoder's statistics of the job's file, from the verdict that has arrived (fallback is the caller's to fill in)
void jpeg_huff_stats_of(const Ctx::JpegJob& B, icelk_jpeg_huff_stats_t* st)
{
    const uint32_t* v = B.h_verdict;
    st->segments = B.segments;
    st->subsequences = B.subsequences;
    st->rounds = v[JV_ROUNDS];
    st->max_hops = v[JV_MAX_HOPS];
    st->total_hops = v[JV_TOTAL_HOPS];
    st->lanes_in_step = v[JV_IN_STEP];
    st->spanning_blocks = v[JV_SPANS];
}

// the serial decoder takes the job's file (from the pinned copy): its coefficients replace the lanes', the transform and
// the output kernel run again
static int host_takes_job(Ctx* c, Ctx::JpegJob& B)
{
    std::vector<int16_t> host;
    if (int rc = jpeg_host_into_job(c, B, B.h_stage + B.file_off, B.len, B.info, B.st, host)) return rc;
    if (int rc = transform_into_slot(c, B)) return rc;
    if (int rc = foreign_write_end(c, c->slots[B.slot], B.st)) return rc;
    HIPCHK(c, hipStreamSynchronize(B.st));   // `host` is free again, and so is everything the job owns
    return ICELK_OK;
}

// What icelk_jpeg_async_finish_file waits for and redoes, by the three routes of a crop job's settle (abi_jpeg_crop.hip):
// afterwards the slot holds its frame, the job's pinned area the scan, and cstats says how both got there.
static int settle_file(Ctx* c, Ctx::JpegJob& B)
{
    icelk_jpeg_crop_stats_t& S = B.cstats;
    memset(&S, 0, sizeof(S));
    enc::Layout L;
    if (int rc = jpeg_enc_rc(c, enc::layout_of(&B.rinfo, &L))) return rc;
    S.blocks = L.blocks;
    S.budget = B.budget;
    uint32_t why = ICELK_JPEG_FALLBACK_SIZE, coder = enc::kOverBudget;
    if (!B.host_only) {
        if (int rc = jpeg_await_verdict(c, B)) return rc;
        const uint32_t* v = B.h_verdict;
        jpeg_huff_stats_of(B, &S.huff);
        why = v[JV_VERDICT] == JV_DECODED ? ICELK_JPEG_FALLBACK_NONE : v[JV_VERDICT];
        coder = v[JV_ENC_VERDICT];
    }
    S.huff.fallback = why;
    if (why != ICELK_JPEG_FALLBACK_NONE) {
        S.route = ICELK_JPEG_CROP_HOST_HUFFMAN;
        if (int rc = host_takes_job(c, B)) return rc;   // the slot's frame again, from the host decoder's coefficients
        if (int rc = jpeg_encode_on(c, B.enc, B.st, L, B.d_rcoef)) return rc;
        return jpeg_fetch_scan(c, B, B.enc.stream_len, true);
    }
    if (coder != enc::kCoded) {
        S.route = ICELK_JPEG_CROP_OVER_BUDGET;   // or a coefficient without a code, which the coder below reports
        if (int rc = jpeg_encode_on(c, B.enc, B.st, L, B.d_rcoef)) return rc;
        return jpeg_fetch_scan(c, B, B.enc.stream_len, true);
    }
    S.route = ICELK_JPEG_CROP_DEVICE;
    return jpeg_fetch_scan(c, B, B.h_verdict[JV_ENC_LEN], false);
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
    Ctx::Jpeg& J = c->jpeg;
    JpegIndex* X = new (std::nothrow) JpegIndex;
    if (!X) FAIL(c, ICELK_ENOMEM, "no memory for the file's index");
    struct Drop {
        JpegIndex* p;
        ~Drop() { delete p; }
    } drop{X};
    icelk_jpeg_info_t info;
    bool host_only = false;
    int rc = jpeg_open(c, data, len, *X, &info, &host_only);
    if (rc) return rc;
    if (info.ncomp != 3) FAIL(c, ICELK_EARG, "expected a 3-component JPEG file");
    icelk_jpeg_info_t rinfo{};
    enc::Layout L{};
    if (resave) {
        if (!jpeg_info_ok(info)) FAIL(c, ICELK_EARG, "JPEG descriptor does not describe a supported file");
        int w = 0, h_ = 0;
        if ((rc = check_crop_box(c, info, crop_left, crop_top, crop_right, crop_bottom, &w, &h_))) return rc;
        if ((rc = jpeg_resave_check(c, w, h_, quality))) return rc;
        resave::resave_info(w, h_, quality, &rinfo);
        if (want_file && (rc = jpeg_enc_rc(c, enc::layout_of(&rinfo, &L)))) return rc;   // blocks * 1660 < 2^32 among it
    }
    if (J.slot_job.empty()) {
        if (const char* e = getenv("ICELK_JPEG_ASYNC_STREAMS")) J.dec_streams = atoi(e) == 1 ? 1 : 2;
        if (const char* e = getenv("ICELK_JPEG_ASYNC_PRIO")) J.dec_high = !strcmp(e, "high");
        try {
            J.slot_job.assign(c->n_slots, -1);
            J.slot_state.assign(c->n_slots, -1);
        } catch (...) {
            J.slot_job.clear();
            FAIL(c, ICELK_ENOMEM, "no memory for the JPEG jobs");
        }
    }
    int idx = -1;
    if ((rc = jpeg_take_job(c, &idx))) return rc;
    Ctx::JpegJob& B = *J.ring[idx];
    B.info = info;
    B.variant = gray_variant;
    B.host_only = host_only;
    B.slot = -1;
    B.resave = resave;
    B.want_file = resave && want_file;
    B.have_scan = false;
    B.rinfo = rinfo;
    rc = start_job(c, B, slot, data, len, *X, crop_left, crop_top, crop_right, crop_bottom, &L);
    if (rc) {
        // what went out before the failure may still use the job's buffers
        if (B.slot >= 0) hipStreamSynchronize(B.st);
        B.slot = -1;
        B.resave = B.want_file = false;
        return rc;
    }
    J.slot_job[slot] = idx;
    J.slot_state[slot] = 0;
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
    if (B->have_scan) *state = B->cstats.huff.fallback == ICELK_JPEG_FALLBACK_NONE ? 1 : 2;   // finish_file ran out of room
    else if (B->host_only) *state = 2;
    else if (!jpeg_verdict_here(*B)) *state = 0;
    else *state = B->h_verdict[JV_VERDICT] == JV_DECODED ? 1 : 2;
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
    memset(&st, 0, sizeof(st));
    uint32_t why = ICELK_JPEG_FALLBACK_SIZE;
    if (!B.host_only) {
        if (int rc = jpeg_await_verdict(c, B)) {
            // a failed launch: nothing of the slot or the job can be relied on
            hipStreamSynchronize(B.st);
            c->slots[slot].levels_built = 0;
            release_job(c, B, 2);
            return rc;
        }
        const uint32_t* v = B.h_verdict;
        jpeg_huff_stats_of(B, &st);
        why = v[JV_VERDICT] == JV_DECODED ? ICELK_JPEG_FALLBACK_NONE : v[JV_VERDICT];
    }
    st.fallback = why;
    int rc = ICELK_OK;
    if (why != ICELK_JPEG_FALLBACK_NONE) {
        rc = host_takes_job(c, B);
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
    if (!B.have_scan) {
        if (int rc = settle_file(c, B)) {
            // a failed launch or a damaged file: nothing of the slot or the job can be relied on
            hipStreamSynchronize(B.st);
            c->slots[slot].levels_built = 0;
            release_job(c, B, 2);
            return rc;
        }
        B.cstats.stream_len = B.scan_len;
    }
    enc::Bytes H(nullptr, 0);
    enc::header_bytes(B.rinfo, comment, comment_len, H);
    *len = H.n + B.scan_len + 2;
    if (!out || capacity < *len) FAIL(c, ICELK_ECAP, "the file does not fit the buffer (len says what it takes)");
    enc::Bytes F(out, capacity);
    enc::header_bytes(B.rinfo, comment, comment_len, F);
    memcpy(out + F.n, B.h_out, (size_t)B.scan_len);
    out[F.n + B.scan_len] = 0xFF;
    out[F.n + B.scan_len + 1] = 0xD9;
    if (stats) *stats = B.cstats;
    release_job(c, B, B.cstats.huff.fallback == ICELK_JPEG_FALLBACK_NONE ? 1 : 2);
    return ICELK_OK;
}

}  // extern "C"
