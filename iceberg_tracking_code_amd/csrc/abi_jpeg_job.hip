// abi_jpeg_job.hip -- the driver of a JPEG file in flight: what the look-ahead decoder (abi_jpeg_async.hip: a job owned by
// a frame slot) and the crop stage (abi_jpeg_crop.hip: a job owned by a ticket) share.  The kernels go out in one piece on
// a decode stream and the host looks at nothing until it is asked to:
//
//   open     the file's index, the checks of descriptor, crop box and re-save, a job of the ring          jpeg_job_open
//   start    plane arguments, lanes, buffers, the file into the job's pinned staging area; then, without a wait: H2D
//            copies, rounds 0 .. max_rounds, scan, write, DC, the kind's middle (jpeg_job_transform), the budgeted coder
//            if a file is wanted, the verdict kernel (k_jpeg_huff.hip), the job's event                   jpeg_job_start
//   poll     a look at the job's pinned verdict words                                                     jpeg_job_state
//   settle   waits for the verdict, then one of three routes.  Coded: one copy of exactly the stuffed length into the
//            job's pinned area, on a fetch stream that no newer job is queued on, and one synchronisation of that
//            stream.  The decoder did not settle: the host decoder reads the retained bytes and everything behind the
//            Huffman phases runs again on the job's stream (jpeg_job_redo_on_host), the coder with host-read sizes
//            (jpeg_encode_on).  Over budget: only that coder runs again                                   jpeg_job_settle
//   file     header, the scan of the pinned area and EOI into the caller's buffer                         jpeg_job_file
//
// The middle by kind.  JOB_SLOT: inverse DCT, gray into the slot's level 0.  JOB_SLOT_RESAVE: inverse DCT, the fused kernel
// (k_jpeg_crop_fwd, k_jpeg_fwd.hip: the crop box of the planes -> the re-saved file's coefficients in rs.d_rcoef, no R G B
// image in between), the inverse DCT of THOSE into planes of the job's own (d_planes2), gray from them into the slot.
// JOB_CROP: inverse DCT, the crop box as R G B (launch_jpeg_rgb), the forward kernel (jpeg_fwd_on).  Only the slot kinds
// check max_w x max_h, take the slot (begin_frame, foreign_write_begin / _end) and may go without a file.
//
// What runs on a file that does not settle, or whose scan does not fit.  The host cannot stop the chain, so everything
// behind the rounds runs on whatever they left.  That is safe by construction, which is what is relied on here:
//   * jpeg_lanes.h: decode() is total and reads no byte outside its segment; a lane decodes the bits of its own
//     subsequence only, so its loop ends; write_lane clamps its first block to the segment's blocks and every store goes
//     to block_base(g) with g < total_blocks, at a zigzag position < 64; the DC pass and the transform walk the image's
//     blocks, not the stream (tests/jpeg_lanes_states.cpp runs this order and arbitrary states on the CPU, under the
//     host's sanitizers).
//   * the output kernels walk the crop box, not the stream, and turn whatever the planes hold into 8-bit samples; the
//     fused kernel reads the planes at clamped coordinates inside them and stores whole blocks of the re-saved layout (its
//     file header says why), and the second inverse DCT walks that layout; the forward kernel reads w x h samples of the
//     job's R G B and writes the blocks of the re-saved file's layout.  The forward DCT of 8-bit samples is bounded --
//     samples are -128 .. 127, so even with table entries of 1 a DC value stays within +-1024 (a DC difference within
//     +-2047, category 11) and an AC value below 1024 in magnitude (category 10) -- so every coefficient has a code
//     whatever the pixels are: a block codes to kMaxBlockBits at most, a count fits 16 bits and the offsets 32 (blocks *
//     1660 < 2^32 is checked in open).
//   * count and the first scan write per-block and per-group arrays sized by the block count.  pack, ff and stuff are the
//     device-sized forms: d_packed (whole chunks, zeroed over its capacity) and d_out hold `budget` bytes, d_ff one word
//     per workgroup of that capacity, and every store is inside them by three uniform exits on the control words --
//     pack leaves when the packed bytes exceed the budget or a coefficient had no code, ff counts only the chunks pack
//     wrote (0 for the workgroups behind them), stuff leaves when packed bytes + FF count exceed the budget.  Beyond that
//     a workgroup of pack stores only a stretch that ends inside the budget and a lane of stuff only bytes that do, so the
//     claim holds for ANY contents of the control words, not just the chain's own (tests/jpeg_enc_budget_main.cpp walks
//     the same decisions, jpeg_enc.h, with buffers of exactly the budget under the host's sanitizers).
// What such a chain leaves in the job's buffers and in the slot is garbage that nobody may consume: finish reads the
// verdict first and overwrites all of it, and the slot counts as filled only after finish has returned ICELK_OK.
//
// Jobs.  Every file in flight owns one Ctx::JpegJob from start to finish; the ring grows when every job is in flight and
// is never sized by the frame maximum.  A job's kernels are through when its verdict has arrived (the verdict kernel is
// the last of the chain) or its stream was synchronised, so a freed job can go out on the other stream at once.
#include "icelk_ctx.h"
#include "jpeg_enc_host.h"
#include "jpeg_resave_host.h"

namespace icelk {

static void free_job(Ctx::JpegJob* B)
{
    jpeg_dec_free(B->dec);
    jpeg_resave_free(B->rs);
    if (B->d_planes2) hipFree(B->d_planes2);
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

// icelk_sync: the decode streams count as streams of the handle; the jobs stay their owners' until finish
int jpeg_async_sync(Ctx* c)
{
    for (auto q : c->jpeg.dec)
        if (q) HIPCHK(c, hipStreamSynchronize(q));
    return ICELK_OK;
}

// a job that neither a slot nor a ticket owns; a new one when all are in flight
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

// the decode streams, created at the first file in flight: two in turn, as Ctx::copy_hi (abi_frames.hip)
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

// the coder's buffers at the job's budget: nothing of them is sized by what a file measures
int jpeg_budget_buffers(Ctx* c, Ctx::JpegJob& B, const enc::Layout& L)
{
    Ctx::JpegEnc& E = B.rs.enc;
    const uint32_t cap = B.budget, chunks = enc::chunks_of(cap);
    if (int rc = jpeg_enc_prepare(c, E)) return rc;
    if (int rc = grow(c, &E.d_bits, &E.bits_cap, (size_t)L.blocks)) return rc;
    if (int rc = grow(c, &E.d_group, &E.group_cap, (size_t)(L.blocks + kJpegEncGroup - 1) / kJpegEncGroup)) return rc;
    if (int rc = grow(c, &E.d_packed, &E.packed_cap, (size_t)chunks * (kJpegEncChunk / 4))) return rc;
    if (int rc = grow(c, &E.d_ff, &E.ff_cap, (size_t)enc::groups_of(chunks))) return rc;
    return grow(c, &E.d_out, &E.out_cap, (size_t)cap);
}

// count, scan, pack, ff, scan, stuff on the job's stream with no look at the sizes
int jpeg_encode_budgeted(Ctx* c, Ctx::JpegJob& B, const enc::Layout& L)
{
    Ctx::JpegEnc& E = B.rs.enc;
    const hipStream_t st = B.st;
    const uint32_t cap = B.budget, chunks = enc::chunks_of(cap), groups = (L.blocks + kJpegEncGroup - 1) / kJpegEncGroup;
    JpegEncArgs A{};
    A.L = L;
    A.coef = B.rs.d_rcoef;
    A.codes = E.d_codes;
    A.bits = E.d_bits;
    A.group = E.d_group;
    A.ctl = E.d_ctl;
    A.packed = E.d_packed;
    HIPCHK(c, hipMemsetAsync(E.d_ctl, 0, JE_WORDS * sizeof(uint32_t), st));
    HIPCHK(c, hipMemsetAsync(E.d_packed, 0, (size_t)chunks * kJpegEncChunk, st));
    {
        ProfScope p(c, K_JPEG_ENC_COUNT, st);
        launch_jpeg_enc_count(st, A);
    }
    {
        ProfScope p(c, K_JPEG_ENC_SCAN, st);
        launch_jpeg_enc_scan(st, E.d_group, groups, E.d_ctl + JE_TOTAL_BITS);
    }
    {
        ProfScope p(c, K_JPEG_ENC_PACK_BUDGET, st);
        launch_jpeg_enc_pack_budget(st, A, cap);
    }
    {
        ProfScope p(c, K_JPEG_ENC_FF_BUDGET, st);
        launch_jpeg_enc_ff_budget(st, E.d_packed, E.d_ctl, cap, E.d_ff);
    }
    {
        ProfScope p(c, K_JPEG_ENC_SCAN, st);
        launch_jpeg_enc_scan(st, E.d_ff, enc::groups_of(chunks), E.d_ctl + JE_FF_TOTAL);
    }
    {
        ProfScope p(c, K_JPEG_ENC_STUFF_BUDGET, st);
        launch_jpeg_enc_stuff_budget(st, E.d_packed, E.d_ctl, cap, E.d_ff, E.d_out);
    }
    return check_launch(c, "jpeg_enc (budgeted)");
}

// The scan at enc.d_out (n bytes) into the job's pinned area.  The copy goes out on the handle's fetch stream behind the
// job's event, not on the job's decode stream: newer jobs are queued there already (two streams in turn, several tickets
// in flight), and the oldest ticket's finish must not wait for their chains.  again: the coder ran again on the job's
// stream behind the verdict, so the event is recorded once more behind it.
int jpeg_fetch_scan(Ctx* c, Ctx::JpegJob& B, uint64_t n, bool again)
{
    Ctx::Jpeg& J = c->jpeg;
    if (!J.fetch) HIPCHK(c, hipStreamCreateWithFlags(&J.fetch, hipStreamNonBlocking));
    if (again) HIPCHK(c, hipEventRecord(B.done, B.st));
    if (B.hout_cap < n) {
        const size_t take = (size_t)n + (size_t)n / 4;   // the photos of a folder all differ a little in length
        if (B.h_out) HIPCHK(c, hipHostFree(B.h_out));
        B.h_out = nullptr;
        B.hout_cap = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&B.h_out), take ? take : 1, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            FAIL(c, ICELK_ENOMEM, "no pinned memory for the coded scan");
        }
        B.hout_cap = take;
    }
    HIPCHK(c, hipStreamWaitEvent(J.fetch, B.done, 0));   // recorded by start, or just now: a job nothing went out for is `again`
    HIPCHK(c, hipMemcpyAsync(B.h_out, B.rs.enc.d_out, (size_t)n, hipMemcpyDeviceToHost, J.fetch));
    HIPCHK(c, hipStreamSynchronize(J.fetch));
    B.scan_len = B.cstats.stream_len = n;
    B.have_scan = true;
    return ICELK_OK;
}

// ---- open --------------------------------------------------------------------------------------------------------------------
// The file's index (on the heap: it is large), the checks that need no job, and a job of the ring (*idx) with its fields reset.
// The re-saving kinds check descriptor, crop box and re-save and fill rs.rinfo; L is filled when a file is wanted.
int jpeg_job_open(Ctx* c, Ctx::JpegJobKind kind, bool want_file, const uint8_t* data, uint64_t len, const JpegBox& box, int quality,
                  std::unique_ptr<JpegIndex>* X, int* idx, enc::Layout* L)
{
    Ctx::Jpeg& J = c->jpeg;
    X->reset(new (std::nothrow) JpegIndex);
    if (!*X) FAIL(c, ICELK_ENOMEM, "no memory for the file's index");
    icelk_jpeg_info_t info, rinfo{};
    bool host_only = false;
    if (int rc = jpeg_open(c, data, len, **X, &info, &host_only)) return rc;
    if (info.ncomp != 3) FAIL(c, ICELK_EARG, "expected a 3-component JPEG file");
    want_file = kind == Ctx::JOB_CROP || (kind == Ctx::JOB_SLOT_RESAVE && want_file);
    if (kind != Ctx::JOB_SLOT) {
        if (!jpeg_info_ok(info)) FAIL(c, ICELK_EARG, "JPEG descriptor does not describe a supported file");
        int w = 0, h = 0;
        if (int rc = check_crop_box(c, info, box.left, box.top, box.right, box.bottom, &w, &h)) return rc;
        if (int rc = jpeg_resave_check(c, w, h, quality)) return rc;
        resave::resave_info(w, h, quality, &rinfo);
        if (want_file)
            if (int rc = jpeg_enc_rc(c, enc::layout_of(&rinfo, L))) return rc;   // blocks * 1660 < 2^32 among it
    }
    if (kind != Ctx::JOB_CROP && J.slot_job.empty()) {
        // Read when the first SLOT job starts, as they always were: a handle that starts crop jobs first has created its
        // decode streams by then, and for those the variables are never looked at
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
    if (int rc = jpeg_take_job(c, idx)) return rc;
    Ctx::JpegJob& B = *J.ring[*idx];
    B.kind = kind;
    B.want_file = want_file;
    B.info = info;
    B.rs.rinfo = rinfo;
    B.host_only = host_only;
    B.have_scan = B.enqueued = false;
    B.slot = B.ticket = -1;
    return ICELK_OK;
}

// ---- start -------------------------------------------------------------------------------------------------------------------
// the crop box of the job's planes as R G B into rs.d_rgb, on the job's stream
static int crop_rgb(Ctx* c, Ctx::JpegJob& B)
{
    JpegOutArgs O = B.out;
    O.dst = B.rs.d_rgb;
    O.dst_pitch = 3 * O.ow;
    {
        ProfScope p(c, K_JPEG_CROP_RGB, B.st);
        launch_jpeg_rgb(B.st, O);
    }
    return check_launch(c, "jpeg_crop_rgb");
}

// the middle of the chain, by kind (the head of this file), from the coefficients in dec.d_coef on the job's stream
static int jpeg_job_transform(Ctx* c, Ctx::JpegJob& B)
{
    if (int rc = jpeg_idct_on(c, B.st, B.idct)) return rc;
    switch (B.kind) {
        case Ctx::JOB_SLOT: return jpeg_gray_on(c, B.st, B.out, c->slots[B.slot], B.variant);
        case Ctx::JOB_SLOT_RESAVE:
            if (int rc = jpeg_crop_fwd_on(c, B.st, B.out, B.rs.d_rcoef, B.rs.rinfo)) return rc;
            if (int rc = jpeg_idct_on(c, B.st, B.ridct)) return rc;
            return jpeg_gray_on(c, B.st, B.rout, c->slots[B.slot], B.variant);
        default:
            if (int rc = crop_rgb(c, B)) return rc;
            return jpeg_fwd_on(c, B.st, B.rs.d_rgb, B.rs.d_rcoef, B.out.ow, B.out.oh, B.rs.rinfo);
    }
}

// The whole chain of an opened job.  slot: the slot kinds' frame slot.  After a failure the caller abandons the job
// (jpeg_job_abandon); a slot taken by then is left without a frame.
int jpeg_job_start(Ctx* c, Ctx::JpegJob& B, int slot, const uint8_t* data, uint64_t len, JpegIndex& X, const JpegBox& box,
                   const enc::Layout& L)
{
    Ctx::Jpeg& J = c->jpeg;
    Ctx::JpegDec& D = B.dec;
    const bool slotted = B.kind != Ctx::JOB_CROP, resave = B.kind != Ctx::JOB_SLOT;
    if (int rc = jpeg_plane_args(c, D, &B.info, box.left, box.top, box.right, box.bottom, &B.idct, &B.out)) return rc;
    // begin_frame's check, taken before anything is allocated for the file
    if (slotted && (B.out.ow > c->max_w || B.out.oh > c->max_h)) FAIL(c, ICELK_ECAP, "frame larger than max_w x max_h of icelk_create");
    JpegHuffArgs H{};
    size_t seg_bytes = 0;
    if (!B.host_only) {
        jpeg_index_lanes(X, (uint32_t)J.subseq_bits, J.max_hops);
        if (int rc = jpeg_huff_setup(c, D, X, len, &H, true)) return rc;
        seg_bytes = X.seg.size() * sizeof(lanes::Seg);
    }
    if (int rc = jpeg_stage_file(c, B, X, seg_bytes, data, len)) return rc;
    if (B.kind == Ctx::JOB_CROP)
        if (int rc = grow(c, &B.rs.d_rgb, &B.rs.rgb_cap, (size_t)3 * B.out.ow * B.out.oh)) return rc;
    if (resave)
        if (int rc = grow(c, &B.rs.d_rcoef, &B.rs.rcoef_cap, (size_t)B.rs.rinfo.coef_count)) return rc;
    if (B.kind == Ctx::JOB_SLOT_RESAVE) {
        if (int rc = grow(c, &B.d_planes2, &B.planes2_cap, jpeg_plane_bytes(B.rs.rinfo))) return rc;
        jpeg_plane_layout(B.rs.rinfo, 0, 0, 0, 0, B.rs.d_rcoef, B.d_planes2, &B.ridct, &B.rout);
    }
    if (B.want_file) {
        B.budget = enc::budget_cap(L.blocks, J.crop_bytes_per_block);
        if (int rc = jpeg_budget_buffers(c, B, L)) return rc;
    }
    if (int rc = jpeg_decode_stream(c, &B.st)) return rc;
    const hipStream_t st = B.st;
    if (slotted) {
        // from here on the slot is taken: whatever fails below leaves it without a frame
        if (int rc = begin_frame(c, slot, B.out.ow, B.out.oh)) return rc;
        B.slot = slot;
    }
    B.enqueued = true;   // from here on something of the job may be in flight: a failure has to wait for the stream
    if (slotted)
        if (int rc = foreign_write_begin(c, c->slots[slot], st)) return rc;   // the slot is left as icelk_upload_gray_async leaves it
    if (B.host_only) return ICELK_OK;   // nothing goes out before finish, which has the host decoder take the file
    memcpy(B.h_stage, X.tabs, sizeof(X.tabs));
    memcpy(B.h_stage + sizeof(X.tabs), X.seg.data(), seg_bytes);
    B.segments = X.scan.nseg;
    B.subsequences = X.scan.nlanes;
    if (int rc = jpeg_huff_stage(c, D, X, B.h_stage + B.file_off, B.h_stage + sizeof(X.tabs), B.h_stage, len, st)) return rc;
    {
        // every round at once: one that no group takes part in returns after two loads per workgroup
        ProfScope p(c, K_JPEG_HUFF, st);
        for (int q = 0; q <= J.max_rounds; q++) launch_jpeg_huff_sync(st, H, q);
        jpeg_huff_finish_phases(st, H);
    }
    if (int rc = check_launch(c, "jpeg_huff")) return rc;
    if (int rc = jpeg_job_transform(c, B)) return rc;
    if (B.want_file)
        if (int rc = jpeg_encode_budgeted(c, B, L)) return rc;
    B.seq = (B.seq + 1) & 0x3fffffffu;
    if (resave) {
        // the coder's words are "not asked" without a file
        ProfScope p(c, K_JPEG_CROP_VERDICT, st);
        launch_jpeg_crop_verdict(st, D.d_ctl, J.max_rounds, B.want_file ? B.rs.enc.d_ctl : nullptr, B.budget, B.h_verdict, B.seq);
    } else {
        launch_jpeg_huff_verdict(st, D.d_ctl, J.max_rounds, B.h_verdict, B.seq);
    }
    if (int rc = check_launch(c, resave ? "jpeg_crop_verdict" : "jpeg_huff_verdict")) return rc;
    HIPCHK(c, hipEventRecord(B.done, st));
    return slotted ? foreign_write_end(c, c->slots[slot], st) : ICELK_OK;
}

// a start has failed: what went out before the failure may still use the job's buffers; then the job is free again
void jpeg_job_abandon(Ctx::JpegJob& B)
{
    if (B.enqueued) hipStreamSynchronize(B.st);
    B.enqueued = B.want_file = false;
    B.slot = B.ticket = -1;
}

// ---- verdict, poll, settle ---------------------------------------------------------------------------------------------------
bool jpeg_verdict_here(const Ctx::JpegJob& B)
{
    return __atomic_load_n(B.h_verdict + JV_SEQ, __ATOMIC_ACQUIRE) == B.seq;
}

// Waits for the verdict by polling the pinned sequence word (await_pinned_seq, abi_frames.hip)
int jpeg_await_verdict(Ctx* c, Ctx::JpegJob& B)
{
    if (int rc = await_pinned_seq(c, reinterpret_cast<const int*>(B.h_verdict + JV_SEQ), (int)B.seq, B.done)) return rc;
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

// Waits for the job's verdict and reads it: the decoder's statistics with `fallback` (ICELK_JPEG_FALLBACK_NONE: decoded)
// and, if asked for, the coder's verdict.  A job nothing went out for is the host decoder's and over its budget.
int jpeg_job_verdict(Ctx* c, Ctx::JpegJob& B, icelk_jpeg_huff_stats_t* huff, uint32_t* coder)
{
    memset(huff, 0, sizeof(*huff));
    huff->fallback = ICELK_JPEG_FALLBACK_SIZE;
    if (coder) *coder = enc::kOverBudget;
    if (B.host_only) return ICELK_OK;
    if (int rc = jpeg_await_verdict(c, B)) return rc;
    const uint32_t* v = B.h_verdict;
    jpeg_huff_stats_of(B, huff);
    huff->fallback = v[JV_VERDICT] == JV_DECODED ? ICELK_JPEG_FALLBACK_NONE : v[JV_VERDICT];
    if (coder) *coder = v[JV_ENC_VERDICT];
    return ICELK_OK;
}

// 0: in flight, 1: the device did all of it, 2: finish has work to do (or had).  with_coder: "all of it" includes the file
// (a crop job); without, the decoder's verdict alone answers: a scan over its budget concerns only the file
int jpeg_job_state(const Ctx::JpegJob& B, bool with_coder)
{
    if (B.have_scan)   // settled already
        return B.cstats.huff.fallback == ICELK_JPEG_FALLBACK_NONE && (!with_coder || B.cstats.route == ICELK_JPEG_CROP_DEVICE) ? 1 : 2;
    if (B.host_only) return 2;
    if (!jpeg_verdict_here(B)) return 0;
    const uint32_t* v = B.h_verdict;
    return v[JV_VERDICT] == JV_DECODED && (!with_coder || v[JV_ENC_VERDICT] == enc::kCoded) ? 1 : 2;
}

// The serial decoder takes the job's file (from the pinned copy): its coefficients replace the lanes' and the middle of the
// chain runs again; with L the coder behind it, with host-read sizes.  The decoder's vector must outlive its copy:
// jpeg_encode_on synchronises, without a coder the stream is synchronised here, and so it is after an error.
int jpeg_job_redo_on_host(Ctx* c, Ctx::JpegJob& B, const enc::Layout* L)
{
    std::vector<int16_t> host;
    int rc = jpeg_host_into_job(c, B.dec, B.h_stage + B.file_off, B.len, B.info, B.st, host);
    if (!rc) rc = jpeg_job_transform(c, B);
    if (!rc && B.kind != Ctx::JOB_CROP) rc = foreign_write_end(c, c->slots[B.slot], B.st);
    if (!rc && L) rc = jpeg_encode_on(c, B.rs.enc, B.st, *L, B.rs.d_rcoef);
    if (rc) {
        hipStreamSynchronize(B.st);   // the copy of `host` may still be on its way
        return rc;
    }
    if (!L) HIPCHK(c, hipStreamSynchronize(B.st));   // `host` is free again, and so is everything the job owns
    return ICELK_OK;
}

// Everything the finish of a job with a file waits for and redoes: afterwards the job's pinned area holds the scan (a slot
// its frame) and cstats says how they got there
int jpeg_job_settle(Ctx* c, Ctx::JpegJob& B)
{
    icelk_jpeg_crop_stats_t& S = B.cstats;
    memset(&S, 0, sizeof(S));
    enc::Layout L;
    if (int rc = jpeg_enc_rc(c, enc::layout_of(&B.rs.rinfo, &L))) return rc;
    uint32_t coder = 0;
    icelk_jpeg_huff_stats_t huff;
    if (int rc = jpeg_job_verdict(c, B, &huff, &coder)) return rc;
    S.blocks = L.blocks;
    S.budget = B.budget;
    S.huff = huff;
    if (huff.fallback != ICELK_JPEG_FALLBACK_NONE) {
        // what the chain coded is the re-save of garbage: the host decoder's coefficients, then everything behind them
        S.route = ICELK_JPEG_CROP_HOST_HUFFMAN;
        if (int rc = jpeg_job_redo_on_host(c, B, &L)) return rc;
        return jpeg_fetch_scan(c, B, B.rs.enc.stream_len, true);
    }
    if (coder != enc::kCoded) {
        S.route = ICELK_JPEG_CROP_OVER_BUDGET;   // or a coefficient without a code, which the coder below reports
        if (int rc = jpeg_encode_on(c, B.rs.enc, B.st, L, B.rs.d_rcoef)) return rc;
        return jpeg_fetch_scan(c, B, B.rs.enc.stream_len, true);
    }
    S.route = ICELK_JPEG_CROP_DEVICE;
    return jpeg_fetch_scan(c, B, B.h_verdict[JV_ENC_LEN], false);
}

// header, the settled job's scan and EOI into the caller's buffer
int jpeg_job_file(Ctx* c, const Ctx::JpegJob& B, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity,
                  uint64_t* len)
{
    if (enc::file_into(B.rs.rinfo, comment, comment_len, B.h_out, B.scan_len, out, capacity, len))
        FAIL(c, ICELK_ECAP, "the file does not fit the buffer (len says what it takes)");
    return ICELK_OK;
}

}  // namespace icelk
