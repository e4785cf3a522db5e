// abi_jpeg_ingest.hip -- JPEG ingest: the steps every mode is composed from, and the synchronous entry points.
//
//   jpeg_open               a file's index (jpeg_open_core, abi_jpeg.hip), or the news that only the serial decoder takes it
//   jpeg_huff_setup         the buffers of a job for that file and the Huffman kernels' arguments
//   jpeg_huff_stage         file, segment table and tables into the job, control words and coefficients cleared
//   jpeg_huff_finish_phases scan, write and the DC pass behind the rounds (the rounds are the caller's: see jpeg_huff_device)
//   jpeg_host_into_job      the serial decoder takes the file: its coefficients into the job
//   jpeg_plane_args         what the box needs of a described file, checked: arguments of the two pixel kernels
//   jpeg_idct_on / jpeg_gray_on   the two pixel kernels on a stream; planes_to_gray_slot: the end of a synchronous upload
//
// The re-save (abi_jpeg_resave.hip) puts its forward kernel between jpeg_planes and planes_to_gray_slot, the job
// driver (abi_jpeg_job.hip) runs the same steps on a decode stream between foreign_write_begin / _end (abi_frames.hip).
#include "icelk_ctx.h"

namespace icelk {

void jpeg_dec_free(Ctx::JpegDec& D)
{
    void* p[] = {D.d_coef, D.d_planes, D.d_file, D.d_seg, D.d_tabs, D.d_T, D.d_X, D.d_cnt, D.d_P, D.d_ctl, D.d_dc};
    for (void* q : p)
        if (q) hipFree(q);
    D = Ctx::JpegDec{};
}

int check_crop_box(Ctx* c, const icelk_jpeg_info_t& I, int left, int top, int right, int bottom, int* w, int* h)
{
    if (left < 0 || top < 0 || right < 0 || bottom < 0 || (long long)left + right >= I.width || (long long)top + bottom >= I.height)
        FAIL(c, ICELK_EARG, "crop box leaves no image");
    *w = I.width - left - right;
    *h = I.height - top - bottom;
    return ICELK_OK;
}

// ---- coefficients -> planes -> pixels (k_jpeg.hip) ------------------------------------------------------------------------
// The block rows the pixel box [left, W - right) x [top, H - bottom) needs and the blocks to transform: fills `A` and `out`
// (planes, chroma mode, box) for the transform and the output kernel, and grows job B's coefficient and plane buffers.
// The descriptor comes from the caller: nothing in it is trusted beyond what jpeg_info_ok has checked against the image size.
int jpeg_plane_args(Ctx* c, Ctx::JpegDec& B, const icelk_jpeg_info_t* I, int left, int top, int right, int bottom, JpegIdctArgs* Ap,
                    JpegOutArgs* out)
{
    if (!I) FAIL(c, ICELK_EARG, "null JPEG descriptor or coefficients");
    if (!jpeg_info_ok(*I)) FAIL(c, ICELK_EARG, "JPEG descriptor does not describe a supported file");
    if (int rc = check_crop_box(c, *I, left, top, right, bottom, &out->ow, &out->oh)) return rc;
    if (int rc = grow(c, &B.d_coef, &B.coef_cap, (size_t)I->coef_count)) return rc;
    if (int rc = grow(c, &B.d_planes, &B.planes_cap, jpeg_plane_bytes(*I))) return rc;
    jpeg_plane_layout(*I, left, top, right, bottom, B.d_coef, B.d_planes, Ap, out);
    return ICELK_OK;
}

size_t jpeg_plane_bytes(const icelk_jpeg_info_t& I)
{
    size_t n = 0;
    for (int k = 0; k < I.ncomp; k++) n += (size_t)I.blocks_x[k] * 8 * I.blocks_y[k] * 8;
    return n;
}

// jpeg_plane_args without its checks and allocations: descriptor and box are known to be good, d_coef holds I.coef_count
// values and d_planes jpeg_plane_bytes(I) bytes (the second plane buffer of a slot-bound re-save job, abi_jpeg_job.hip)
void jpeg_plane_layout(const icelk_jpeg_info_t& Iref, int left, int top, int right, int bottom, int16_t* d_coef, uint8_t* d_planes,
                       JpegIdctArgs* Ap, JpegOutArgs* out)
{
    const icelk_jpeg_info_t* I = &Iref;
    out->ow = I->width - left - right;
    out->oh = I->height - top - bottom;
    const int nc = I->ncomp;
    const bool sub_x = nc == 3 && I->hmax == 2, sub_y = nc == 3 && I->vmax == 2;
    // libjpeg filters only planes wider than 2 samples, narrower ones are replicated
    const bool fancy = I->comp_w[1] > 2;
    size_t plane_off[3], plane_bytes = 0;
    for (int k = 0; k < nc; k++) {
        plane_off[k] = plane_bytes;
        plane_bytes += (size_t)I->blocks_x[k] * 8 * I->blocks_y[k] * 8;
    }
    JpegIdctArgs& A = *Ap;
    A = JpegIdctArgs{};
    const int x0 = left, x1 = I->width - right - 1, y0 = top, y1 = I->height - bottom - 1;   // first / last pixel kept
    A.first[0] = 0;
    for (int k = 0; k < 3; k++) {
        if (k >= nc) {
            A.first[k + 1] = A.first[k];
            continue;
        }
        // samples of this component the box touches: chroma one more on every subsampled side (the filter's neighbour)
        int sx0 = x0, sx1 = x1, sy0 = y0, sy1 = y1;
        if (k > 0 && sub_x) sx0 = std::max(x0 / 2 - 1, 0), sx1 = std::min(x1 / 2 + 1, I->comp_w[k] - 1);
        if (k > 0 && sub_y) sy0 = std::max(y0 / 2 - 1, 0), sy1 = std::min(y1 / 2 + 1, I->comp_h[k] - 1);
        A.bx0[k] = sx0 / 8;
        A.by0[k] = sy0 / 8;
        A.nbx[k] = sx1 / 8 - A.bx0[k] + 1;
        const int nby = sy1 / 8 - A.by0[k] + 1;
        A.first[k + 1] = A.first[k] + A.nbx[k] * nby;
        A.blocks_x[k] = I->blocks_x[k];
        A.pitch[k] = I->blocks_x[k] * 8;
        A.coef[k] = d_coef + I->coef_offset[k];
        A.plane[k] = d_planes + plane_off[k];
        memcpy(A.quant[k], I->quant[k], sizeof(A.quant[k]));
        out->plane[k] = A.plane[k];
        out->pitch[k] = A.pitch[k];
    }
    out->W = I->width;
    out->cw = I->comp_w[nc - 1];
    out->ch = I->comp_h[nc - 1];
    out->mode = !sub_x ? 0 : (sub_y ? (fancy ? 2 : 4) : (fancy ? 1 : 3));
    out->left = left;
    out->top = top;
}

int jpeg_idct_on(Ctx* c, hipStream_t st, const JpegIdctArgs& A)
{
    {
        ProfScope p(c, K_JPEG_IDCT, st);
        launch_jpeg_idct(st, A);
    }
    return check_launch(c, "jpeg_idct");
}

// the output kernel on stream st: the planes of `O` as gray into level 0 of slot s
int jpeg_gray_on(Ctx* c, hipStream_t st, JpegOutArgs O, const Slot& s, int gray_variant)
{
    O.dst = s.lv[0].ptr;
    O.dst_pitch = s.lv[0].pitch;
    {
        ProfScope p(c, K_JPEG_OUT, st);
        launch_jpeg_gray(st, O, gray_variant);
    }
    return check_launch(c, "jpeg_out");
}

// the end of every synchronous upload: the planes of `O` become the slot's frame; the caller's buffers are free again
int planes_to_gray_slot(Ctx* c, int slot, const JpegOutArgs& O, int gray_variant)
{
    int rc = begin_frame(c, slot, O.ow, O.oh);
    if (rc) return rc;
    Slot& s = c->slots[slot];
    rc = jpeg_gray_on(c, c->stream, O, s, gray_variant);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return end_frame(c, s);
}

// jpeg_plane_args for the synchronous job, then: uploads the block rows the box needs and transforms its blocks on the
// compute stream.  on_device: the job's d_coef holds the file's coefficients already (jpeg_huff_device), nothing is uploaded.
int jpeg_planes(Ctx* c, const icelk_jpeg_info_t* I, const int16_t* coef, int left, int top, int right, int bottom, JpegOutArgs* out,
                bool on_device)
{
    if (!I || (!coef && !on_device)) FAIL(c, ICELK_EARG, "null JPEG descriptor or coefficients");
    Ctx::JpegDec& B = c->jpeg.sync;
    JpegIdctArgs A;
    if (int rc = jpeg_plane_args(c, B, I, left, top, right, bottom, &A, out)) return rc;
    for (int k = 0; k < I->ncomp && !on_device; k++) {
        // whole block rows by0 .. by0 + nby - 1: contiguous in the layout
        const int nby = (A.first[k + 1] - A.first[k]) / A.nbx[k];
        const size_t row = (size_t)I->blocks_x[k] * 64, from = I->coef_offset[k] + (size_t)A.by0[k] * row;
        HIPCHK(c, hipMemcpyAsync(B.d_coef + from, coef + from, row * nby * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
    }
    return jpeg_idct_on(c, c->stream, A);
}

// the planes of jpeg_planes -> the decoded image on the host (the tail of icelk_jpeg_decode_rgb and of its _file form)
int jpeg_rgb_out(Ctx* c, const icelk_jpeg_info_t& I, JpegOutArgs& O, uint8_t* out, int stride)
{
    const size_t row = (size_t)O.ow * I.ncomp;
    if (stride < 0 || (size_t)stride < row) FAIL(c, ICELK_EARG, "stride smaller than a row of the image");
    if (I.ncomp == 1) {
        HIPCHK(c, hipMemcpy2DAsync(out, stride, O.plane[0], O.pitch[0], row, O.oh, hipMemcpyDeviceToHost, c->stream));
    } else {
        int rc = grow(c, &c->jpeg.d_rgb, &c->jpeg.rgb_cap, row * O.oh);
        if (rc) return rc;
        O.dst = c->jpeg.d_rgb;
        O.dst_pitch = (int)row;
        {
            ProfScope p(c, K_JPEG_OUT);
            launch_jpeg_rgb(c->stream, O);
        }
        rc = check_launch(c, "jpeg_out");
        if (rc) return rc;
        HIPCHK(c, hipMemcpy2DAsync(out, stride, c->jpeg.d_rgb, row, row, O.oh, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

// ---- the file's bytes -> coefficients in a job's d_coef (k_jpeg_huff.hip) -------------------------------------------------
const char* jpeg_open_error(int rc)
{
    return rc == ICELK_EUNSUP ? "a JPEG file of a kind the decoder does not take" : "not a JPEG file, or a damaged one";
}

// X and *info of a file; *host_only: the lanes' positions are 32 bits, a file of 256 MiB or more takes the host decoder
// at once and only *info is filled
int jpeg_open(Ctx* c, const uint8_t* data, uint64_t len, JpegIndex& X, icelk_jpeg_info_t* info, bool* host_only)
{
    const int rc = jpeg_open_core(data, len, X, info, host_only);
    if (rc) FAIL(c, rc, *host_only ? "not a JPEG file the decoder takes" : jpeg_open_error(rc));
    return ICELK_OK;
}

// The serial decoder takes the file: its coefficients, kept in `keep` until stream st is through, go into job J.
int jpeg_host_into_job(Ctx* c, Ctx::JpegDec& J, const uint8_t* data, uint64_t len, const icelk_jpeg_info_t& I, hipStream_t st,
                       std::vector<int16_t>& keep)
{
    try {
        keep.resize((size_t)I.coef_count);
    } catch (...) {
        FAIL(c, ICELK_ENOMEM, "no memory for the coefficients");
    }
    if (int rc = jpeg_host_decode(data, (size_t)len, keep.data(), I.coef_count)) FAIL(c, rc, jpeg_open_error(rc));   // headers passed: "damaged"
    HIPCHK(c, hipMemcpyAsync(J.d_coef, keep.data(), keep.size() * sizeof(int16_t), hipMemcpyHostToDevice, st));
    return ICELK_OK;
}

// the synchronous form: when the lanes' work bound was hit, or to have the last word on a stream that contradicts itself
static int jpeg_huff_fallback(Ctx* c, const uint8_t* data, uint64_t len, const icelk_jpeg_info_t& I, uint32_t why)
{
    c->jpeg.stats.fallback = why;
    std::vector<int16_t> host;
    if (int rc = jpeg_host_into_job(c, c->jpeg.sync, data, len, I, c->stream, host)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

// The buffers of job J for a file of `len` bytes indexed as X (jpeg_index, jpeg_index_lanes), and the kernels' arguments.
// headroom: what grows with the file's length is taken a quarter larger than this file needs -- growing a buffer frees
// it, which waits for the whole device, and the photos of a folder all differ a little in length (asynchronous jobs).
int jpeg_huff_setup(Ctx* c, Ctx::JpegDec& J, const JpegIndex& X, uint64_t len, JpegHuffArgs* Hp, bool headroom)
{
    const lanes::Scan& A = X.scan;
    auto pad = [&](size_t n) { return headroom ? n + n / 4 : n; };
    JpegHuffArgs& H = *Hp;
    H.A = A;
    H.ngroups = (A.nlanes + lanes::kGroup - 1) / lanes::kGroup;
    H.ri_mcus = A.seg_blocks ? A.seg_blocks / (uint32_t)A.bpm : (uint32_t)A.nmcu;
    H.cps = (H.ri_mcus + kJpegDcChunk - 1) / kJpegDcChunk;
    if (int r2 = grow(c, &J.d_coef, &J.coef_cap, (size_t)X.info.coef_count)) return r2;
    if (int r2 = grow(c, &J.d_file, &J.file_cap, pad((size_t)len))) return r2;
    if (int r2 = grow(c, &J.d_seg, &J.seg_cap, pad((size_t)A.nseg + 1))) return r2;
    if (!J.d_tabs) if (int r2 = dmalloc(c, &J.d_tabs, lanes::kTables)) return r2;
    if (!J.d_ctl) if (int r2 = dmalloc(c, &J.d_ctl, JH_WORDS)) return r2;
    if (J.lane_cap < (size_t)A.nlanes + 1) {
        // the four arrays of the lanes grow together
        const size_t want = pad((size_t)A.nlanes + 1);
        size_t cap = 0;
        if (int r2 = grow(c, &J.d_T, &cap, want)) return r2;
        cap = 0;
        if (int r2 = grow(c, &J.d_cnt, &cap, want)) return r2;
        cap = 0;
        if (int r2 = grow(c, &J.d_P, &cap, want)) return r2;
        J.lane_cap = want;
    }
    if (int r2 = grow(c, &J.d_X, &J.group_cap, pad((size_t)2 * H.ngroups))) return r2;
    if (int r2 = grow(c, &J.d_dc, &J.dc_cap, pad((size_t)3 * A.nseg * H.cps))) return r2;
    H.data = J.d_file;
    H.seg = J.d_seg;
    H.tabs = J.d_tabs;
    H.T = J.d_T;
    H.cnt = J.d_cnt;
    H.P = J.d_P;
    H.X = J.d_X;
    H.ctl = J.d_ctl;
    H.coef = J.d_coef;
    H.dc = J.d_dc;
    return ICELK_OK;
}

// The file's `len` bytes, X's segment table and X's tables, each from where the caller keeps them (its own memory, or the
// job's pinned staging area), into job J on stream st; the control words and the coefficients cleared behind them.
int jpeg_huff_stage(Ctx* c, Ctx::JpegDec& J, const JpegIndex& X, const uint8_t* file, const void* seg, const void* tabs, uint64_t len,
                    hipStream_t st)
{
    HIPCHK(c, hipMemcpyAsync(J.d_file, file, (size_t)len, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(J.d_seg, seg, X.seg.size() * sizeof(lanes::Seg), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(J.d_tabs, tabs, sizeof(X.tabs), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(J.d_ctl, 0, JH_WORDS * sizeof(uint32_t), st));
    HIPCHK(c, hipMemsetAsync(J.d_coef, 0, (size_t)X.info.coef_count * sizeof(int16_t), st));
    return ICELK_OK;
}

// Phases 2 and 3 and the DC pass, inside the caller's ProfScope.  The DC pass runs on whatever the lanes wrote: were they
// irregular, the serial decoder overwrites all of it.
void jpeg_huff_finish_phases(hipStream_t st, const JpegHuffArgs& H)
{
    launch_jpeg_huff_scan(st, H);
    launch_jpeg_huff_write(st, H);
    launch_jpeg_huff_dc(st, H);
}

int jpeg_huff_device(Ctx* c, const uint8_t* data, uint64_t len, icelk_jpeg_info_t* info)
{
    if (!data || !info) FAIL(c, ICELK_EARG, "null JPEG file");
    Ctx::Jpeg& J = c->jpeg;
    Ctx::JpegDec& B = J.sync;
    memset(&J.stats, 0, sizeof(J.stats));
    JpegIndex X;
    bool host_only = false;
    if (int rc = jpeg_open(c, data, len, X, info, &host_only)) return rc;
    if (host_only) {
        if (int r2 = grow(c, &B.d_coef, &B.coef_cap, (size_t)info->coef_count)) return r2;
        return jpeg_huff_fallback(c, data, len, *info, ICELK_JPEG_FALLBACK_SIZE);
    }
    jpeg_index_lanes(X, (uint32_t)J.subseq_bits, J.max_hops);
    const lanes::Scan& A = X.scan;
    JpegHuffArgs H{};
    if (int r2 = jpeg_huff_setup(c, B, X, len, &H, false)) return r2;
    hipStream_t st = c->stream;
    if (int r2 = jpeg_huff_stage(c, B, X, data, X.seg.data(), X.tabs, len, st)) return r2;
    J.stats.segments = A.nseg;
    J.stats.subsequences = A.nlanes;
    uint32_t ctl[JH_WORDS];
    // Phase 1.  A round that no group takes part in costs a launch of workgroups that return at once, so the rounds go out
    // a few at a time and the host looks at their flags afterwards: the fixed point is reached when one changed nothing.
    bool settled = false, bound = false;
    {
        ProfScope p(c, K_JPEG_HUFF);
        launch_jpeg_huff_sync(st, H, 0);
        int r = 1;
        while (!settled && !bound && r <= J.max_rounds) {
            const int r_end = std::min(J.max_rounds, r + 3);
            for (int q = r; q <= r_end; q++) launch_jpeg_huff_sync(st, H, q);
            if (int r2 = check_launch(c, "jpeg_huff_sync")) return r2;
            HIPCHK(c, hipMemcpyAsync(ctl, B.d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            bound = ctl[JH_BOUND] != 0;
            for (int q = r; q <= r_end && !settled; q++) settled = ctl[JH_ROUND0 + q] == 0;
            r = r_end + 1;
        }
    }
    J.stats.rounds = 1;
    for (int q = 1; q <= J.max_rounds && ctl[JH_ROUND0 + q]; q++) J.stats.rounds++;
    J.stats.max_hops = ctl[JH_MAX_HOPS];
    J.stats.total_hops = ctl[JH_TOTAL_HOPS];
    if (bound || !settled) return jpeg_huff_fallback(c, data, len, X.info, ICELK_JPEG_FALLBACK_BOUND);
    {
        ProfScope p(c, K_JPEG_HUFF);
        jpeg_huff_finish_phases(st, H);
    }
    if (int r2 = check_launch(c, "jpeg_huff_write")) return r2;
    HIPCHK(c, hipMemcpyAsync(ctl, B.d_ctl, JH_ROUND0 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    J.stats.lanes_in_step = ctl[JH_IN_STEP];
    J.stats.spanning_blocks = ctl[JH_SPANS];
    if (ctl[JH_IRREGULAR]) return jpeg_huff_fallback(c, data, len, X.info, ICELK_JPEG_FALLBACK_STREAM);
    return ICELK_OK;
}

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_upload_jpeg(icelk_t* h, int slot, const icelk_jpeg_info_t* info, const int16_t* coef, int gray_variant,
                      int crop_left, int crop_top, int crop_right, int crop_bottom)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (int rc = check_gray_variant(c, gray_variant)) return rc;
    if (info && info->ncomp != 3) FAIL(c, ICELK_EARG, "expected a 3-component JPEG file");
    HIPCHK(c, hipSetDevice(c->device));
    JpegOutArgs O{};
    int rc = check_slot(c, slot, false);
    if (!rc) rc = jpeg_planes(c, info, coef, crop_left, crop_top, crop_right, crop_bottom, &O);
    if (rc) return rc;
    return planes_to_gray_slot(c, slot, O, gray_variant);
}

int icelk_jpeg_decode_rgb(icelk_t* h, const icelk_jpeg_info_t* info, const int16_t* coef, uint8_t* out, int stride)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!out || !info) FAIL(c, ICELK_EARG, "null output image or descriptor");
    HIPCHK(c, hipSetDevice(c->device));
    JpegOutArgs O{};
    int rc = jpeg_planes(c, info, coef, 0, 0, 0, 0, &O);
    if (rc) return rc;
    return jpeg_rgb_out(c, *info, O, out, stride);
}

int icelk_jpeg_huff_config(icelk_t* h, int subseq_bits, int max_hops, int max_rounds)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!jpeg_huff_config_ok(subseq_bits, max_hops, max_rounds)) FAIL(c, ICELK_EARG, "bad subsequence length or work bound");
    c->jpeg.subseq_bits = subseq_bits;
    c->jpeg.max_hops = max_hops;
    c->jpeg.max_rounds = max_rounds;
    return ICELK_OK;
}

int icelk_jpeg_huff_stats(icelk_t* h, icelk_jpeg_huff_stats_t* stats)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!stats) FAIL(c, ICELK_EARG, "null statistics");
    *stats = c->jpeg.stats;
    return ICELK_OK;
}

int icelk_upload_jpeg_file(icelk_t* h, int slot, const uint8_t* data, uint64_t len, int gray_variant, int crop_left, int crop_top,
                           int crop_right, int crop_bottom)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (int rc = check_gray_variant(c, gray_variant)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = check_slot(c, slot, false);
    if (rc) return rc;
    icelk_jpeg_info_t I;
    if (data && !icelk_jpeg_describe(data, len, &I) && I.ncomp != 3) FAIL(c, ICELK_EARG, "expected a 3-component JPEG file");
    rc = jpeg_huff_device(c, data, len, &I);
    if (rc) return rc;
    JpegOutArgs O{};
    rc = jpeg_planes(c, &I, nullptr, crop_left, crop_top, crop_right, crop_bottom, &O, true);
    if (rc) return rc;
    return planes_to_gray_slot(c, slot, O, gray_variant);
}

int icelk_jpeg_decode_rgb_file(icelk_t* h, const uint8_t* data, uint64_t len, uint8_t* out, int stride)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!out) FAIL(c, ICELK_EARG, "null output image");
    HIPCHK(c, hipSetDevice(c->device));
    icelk_jpeg_info_t I;
    int rc = jpeg_huff_device(c, data, len, &I);
    if (rc) return rc;
    JpegOutArgs O{};
    rc = jpeg_planes(c, &I, nullptr, 0, 0, 0, 0, &O, true);
    if (rc) return rc;
    return jpeg_rgb_out(c, I, O, out, stride);
}

int icelk_jpeg_device_coefficients(icelk_t* h, const uint8_t* data, uint64_t len, int16_t* coef, uint64_t capacity)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!coef) FAIL(c, ICELK_EARG, "null coefficient buffer");
    HIPCHK(c, hipSetDevice(c->device));
    icelk_jpeg_info_t I;
    int rc = jpeg_huff_device(c, data, len, &I);
    if (rc) return rc;
    if (capacity < I.coef_count) FAIL(c, ICELK_ECAP, "coefficient buffer too small");
    HIPCHK(c, hipMemcpyAsync(coef, c->jpeg.sync.d_coef, (size_t)I.coef_count * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

}  // extern "C"
