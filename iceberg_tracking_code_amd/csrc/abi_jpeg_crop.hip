// abi_jpeg_crop.hip -- the reference's crop step (camtools.py:64-104: open, crop, save again as JPEG) as a job of its own:
// icelk_jpeg_crop_config / _start / _poll / _finish / _cancel.  A file goes out in one piece on a decode stream, into
// buffers no frame slot has a share in, and comes back as the bytes Pillow's `crop.save(path)` writes:
//
//   start    the host's share as icelk_upload_jpeg_file_async (index, lanes, descriptor, crop box) plus the re-save's
//            checks; the file into the job's pinned staging area; then, without a wait: H2D copies, the Huffman rounds and
//            phases, inverse DCT, the crop box as R G B (launch_jpeg_rgb), the forward kernel (jpeg_fwd_on), the coder with
//            its sizes left on the device (count, scan, pack, ff, scan, stuff: the _budget forms of k_jpeg_enc.hip), the
//            verdict kernel, the job's event
//   poll     a look at the job's pinned verdict words
//   finish   waits for the verdict.  Coded: one copy of exactly the stuffed length into the job's pinned area, on a fetch
//            stream that no newer job is queued on, and one synchronisation of that stream.  The decoder did not settle: the host decoder reads the retained bytes and everything
//            behind the Huffman phases runs again on the job's stream, the coder with host-read sizes (jpeg_encode_on).
//            Over budget: only that coder runs again.  Then header, scan and EOI go into the caller's buffer
//
// What runs on a file that does not settle, or whose scan does not fit.  The host cannot stop the chain.  For the decoder's
// kernels the header of abi_jpeg_async.hip says why that is safe; here the chain goes on:
//   * the output kernel walks the crop box, not the stream, and turns whatever the planes hold into 8-bit samples of the
//     job's R G B; the forward kernel reads those w x h samples and writes the blocks of the re-saved file's layout.  The
//     forward DCT of 8-bit samples is bounded -- samples are -128 .. 127, so even with table entries of 1 a DC value stays
//     within +-1024 (a DC difference within +-2047, category 11) and an AC value below 1024 in magnitude (category 10) --
//     so every coefficient has a code whatever the pixels are: a block codes to kMaxBlockBits at most, a
//     count fits 16 bits and the offsets 32 (blocks * 1660 < 2^32 is checked in start).
//   * count and the first scan write per-block and per-group arrays sized by the block count.  pack, ff and stuff are the
//     device-sized forms: d_packed (whole chunks, zeroed over its capacity) and d_out hold `budget` bytes, d_ff one word
//     per workgroup of that capacity, and every store is inside them by three uniform exits on the control words --
//     pack leaves when the packed bytes exceed the budget or a coefficient had no code, ff counts only the chunks pack
//     wrote (0 for the workgroups behind them), stuff leaves when packed bytes + FF count exceed the budget.  Beyond that
//     a workgroup of pack stores only a stretch that ends inside the budget and a lane of stuff only bytes that do, so the
//     claim holds for ANY contents of the control words, not just the chain's own (tests/jpeg_enc_budget_main.cpp walks
//     the same decisions, jpeg_enc.h, with buffers of exactly the budget under the host's sanitizers).
// What such a chain leaves in the job is garbage nobody consumes: finish reads the verdict first and overwrites all of it.
#include <new>
#include <vector>

#include "icelk_ctx.h"
#include "jpeg_enc_host.h"
#include "jpeg_resave_host.h"

namespace icelk {

// ---- shared with the slot-bound re-save job (abi_jpeg_async.hip)
// the coder's buffers at the job's budget: nothing of them is sized by what a file measures
int jpeg_budget_buffers(Ctx* c, Ctx::JpegJob& B, const enc::Layout& L)
{
    Ctx::JpegEnc& E = B.enc;
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
    Ctx::JpegEnc& E = B.enc;
    const hipStream_t st = B.st;
    const uint32_t cap = B.budget, chunks = enc::chunks_of(cap), groups = (L.blocks + kJpegEncGroup - 1) / kJpegEncGroup;
    JpegEncArgs A{};
    A.L = L;
    A.coef = B.d_rcoef;
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

// The scan at E.d_out (n bytes) into the job's pinned area.  The copy goes out on the handle's fetch stream behind the
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
    HIPCHK(c, hipMemcpyAsync(B.h_out, B.enc.d_out, (size_t)n, hipMemcpyDeviceToHost, J.fetch));
    HIPCHK(c, hipStreamSynchronize(J.fetch));
    B.scan_len = n;
    B.have_scan = true;
    return ICELK_OK;
}

namespace {

Ctx::JpegJob* job_of_ticket(Ctx* c, int ticket)
{
    if (ticket < 1) return nullptr;
    for (Ctx::JpegJob* B : c->jpeg.ring)
        if (B->ticket == ticket) return B;
    return nullptr;
}

// the crop box of the job's planes as R G B into d_rgb, on the job's stream
int crop_rgb(Ctx* c, Ctx::JpegJob& B)
{
    JpegOutArgs O = B.out;
    O.dst = B.d_rgb;
    O.dst_pitch = 3 * O.ow;
    {
        ProfScope p(c, K_JPEG_CROP_RGB, B.st);
        launch_jpeg_rgb(B.st, O);
    }
    return check_launch(c, "jpeg_crop_rgb");
}

// inverse DCT of the job's coefficients, the crop box, the forward kernel: d_coef -> d_rcoef
int transform_and_resave(Ctx* c, Ctx::JpegJob& B)
{
    if (int rc = jpeg_idct_on(c, B.st, B.idct)) return rc;
    if (int rc = crop_rgb(c, B)) return rc;
    return jpeg_fwd_on(c, B.st, B.d_rgb, B.d_rcoef, B.out.ow, B.out.oh, B.rinfo);
}

int start_job(Ctx* c, Ctx::JpegJob& B, const uint8_t* data, uint64_t len, JpegIndex& X, int left, int top, int right, int bottom,
              const enc::Layout& L)
{
    Ctx::Jpeg& J = c->jpeg;
    if (int rc = jpeg_plane_args(c, B, &B.info, left, top, right, bottom, &B.idct, &B.out)) return rc;
    JpegHuffArgs H{};
    size_t seg_bytes = 0;
    if (!B.host_only) {
        jpeg_index_lanes(X, (uint32_t)J.subseq_bits, J.max_hops);
        if (int rc = jpeg_huff_setup(c, B, X, len, &H, true)) return rc;
        seg_bytes = X.seg.size() * sizeof(lanes::Seg);
    }
    if (int rc = jpeg_stage_file(c, B, X, seg_bytes, data, len)) return rc;
    if (int rc = grow(c, &B.d_rgb, &B.rgb_cap, (size_t)3 * B.out.ow * B.out.oh)) return rc;
    if (int rc = grow(c, &B.d_rcoef, &B.rcoef_cap, (size_t)B.rinfo.coef_count)) return rc;
    B.budget = enc::budget_cap(L.blocks, J.crop_bytes_per_block);
    if (int rc = jpeg_budget_buffers(c, B, L)) return rc;
    if (int rc = jpeg_decode_stream(c, &B.st)) return rc;
    if (B.host_only) return ICELK_OK;   // nothing goes out before finish, which has the host decoder take the file
    const hipStream_t st = B.st;
    memcpy(B.h_stage, X.tabs, sizeof(X.tabs));
    memcpy(B.h_stage + sizeof(X.tabs), X.seg.data(), seg_bytes);
    B.segments = X.scan.nseg;
    B.subsequences = X.scan.nlanes;
    B.ticket = 0;   // from here on something of the job is in flight: a failure has to wait for the stream
    if (int rc = jpeg_huff_stage(c, B, X, B.h_stage + B.file_off, B.h_stage + sizeof(X.tabs), B.h_stage, len, st)) return rc;
    {
        ProfScope p(c, K_JPEG_HUFF, st);
        for (int q = 0; q <= J.max_rounds; q++) launch_jpeg_huff_sync(st, H, q);
        jpeg_huff_finish_phases(st, H);
    }
    if (int rc = check_launch(c, "jpeg_huff")) return rc;
    if (int rc = transform_and_resave(c, B)) return rc;
    if (int rc = jpeg_encode_budgeted(c, B, L)) return rc;
    B.seq = (B.seq + 1) & 0x3fffffffu;
    {
        ProfScope p(c, K_JPEG_CROP_VERDICT, st);
        launch_jpeg_crop_verdict(st, B.d_ctl, J.max_rounds, B.enc.d_ctl, B.budget, B.h_verdict, B.seq);
    }
    if (int rc = check_launch(c, "jpeg_crop_verdict")) return rc;
    HIPCHK(c, hipEventRecord(B.done, st));
    return ICELK_OK;
}

// everything finish waits for and redoes: afterwards the job's pinned area holds the scan and cstats says how it got there
int settle(Ctx* c, Ctx::JpegJob& B)
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
        // what the chain coded is the re-save of garbage: the host decoder's coefficients, then everything behind them
        S.route = ICELK_JPEG_CROP_HOST_HUFFMAN;
        std::vector<int16_t> host;
        int rc = jpeg_host_into_job(c, B, B.h_stage + B.file_off, B.len, B.info, B.st, host);
        if (!rc) rc = transform_and_resave(c, B);
        if (!rc) rc = jpeg_encode_on(c, B.enc, B.st, L, B.d_rcoef);   // synchronises: `host` is free
        if (rc) {
            hipStreamSynchronize(B.st);   // the copy of `host` may still be on its way
            return rc;
        }
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
    enc::Bytes H(nullptr, 0);
    enc::header_bytes(*info, comment, comment_len, H);
    *len = H.n + W.stuffed + 2;
    if (!out || capacity < *len) return ICELK_ECAP;
    enc::Bytes B(out, capacity);
    enc::header_bytes(*info, comment, comment_len, B);
    B.put(scan.data(), W.stuffed);
    B.put16(0xFFD9);
    return ICELK_OK;
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
    Ctx::Jpeg& J = c->jpeg;
    JpegIndex* X = new (std::nothrow) JpegIndex;
    if (!X) FAIL(c, ICELK_ENOMEM, "no memory for the file's index");
    struct Drop {
        JpegIndex* p;
        ~Drop() { delete p; }
    } drop{X};
    icelk_jpeg_info_t info;
    bool host_only = false;
    int rc = jpeg_open(c, file, len, *X, &info, &host_only);
    if (rc) return rc;
    if (info.ncomp != 3) FAIL(c, ICELK_EARG, "expected a 3-component JPEG file");
    if (!jpeg_info_ok(info)) FAIL(c, ICELK_EARG, "JPEG descriptor does not describe a supported file");
    int w = 0, h_ = 0;
    if ((rc = check_crop_box(c, info, crop_left, crop_top, crop_right, crop_bottom, &w, &h_))) return rc;
    if ((rc = jpeg_resave_check(c, w, h_, quality))) return rc;
    icelk_jpeg_info_t rinfo;
    resave::resave_info(w, h_, quality, &rinfo);
    enc::Layout L;
    if ((rc = jpeg_enc_rc(c, enc::layout_of(&rinfo, &L)))) return rc;   // blocks * 1660 < 2^32 among it
    int idx = -1;
    if ((rc = jpeg_take_job(c, &idx))) return rc;
    Ctx::JpegJob& B = *J.ring[idx];
    B.info = info;
    B.rinfo = rinfo;
    B.host_only = host_only;
    B.have_scan = false;
    B.slot = -1;
    B.ticket = -1;
    rc = start_job(c, B, file, len, *X, crop_left, crop_top, crop_right, crop_bottom, L);
    if (rc) {
        // what went out before the failure may still use the job's buffers
        if (B.ticket == 0) hipStreamSynchronize(B.st);
        B.ticket = -1;
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
    if (B->have_scan) *state = B->cstats.route == ICELK_JPEG_CROP_DEVICE ? 1 : 2;
    else if (B->host_only) *state = 2;
    else if (!jpeg_verdict_here(*B)) *state = 0;
    else *state = B->h_verdict[JV_VERDICT] == JV_DECODED && B->h_verdict[JV_ENC_VERDICT] == enc::kCoded ? 1 : 2;
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
        if (int rc = settle(c, B)) {
            // a failed launch or a damaged file: nothing of the job can be relied on
            hipStreamSynchronize(B.st);
            release(B);
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
