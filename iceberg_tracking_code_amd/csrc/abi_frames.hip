// abi_frames.hip -- frame slots: layout, slot events, pyramids, the ingest entry points, level download.
#include "icelk_ctx.h"

namespace icelk {

// What the kernels that read and write whole dwords rely on (k_pyramid.hip stage 1 / copy_out, the tracker's tile loader,
// the corner kernels' staging): every level starts on a 256-B boundary, its row pitch is a multiple of 64 B >= the width
// rounded up to 4, so an aligned dword that STARTS inside a row (x = 0 mod 4, x < w) ends inside that row's pitch; and
// the allocation ends >= 256 B behind the last level, so a dword read that starts inside the last row of the last level
// stays inside the allocation.  Checked for every geometry a handle lays out (icelk_create, begin_frame).
bool layout_ok(const Slot& s)
{
    for (int l = 0; l < kMaxLevels; l++) {
        const Level& L = s.lv[l];
        if (((uintptr_t)L.ptr & 255u) || (L.pitch % kPitchAlign) || L.pitch < ((L.w + 3) & ~3)) return false;
        if (L.ptr + (size_t)L.pitch * L.h + 256 > s.base + s.bytes) return false;
    }
    return true;
}

// level geometry of a w x h frame inside a slot allocation
void layout_levels(Slot& s, int w, int h)
{
    size_t off = 0;
    int lw = w, lh = h;
    for (int l = 0; l < kMaxLevels; l++) {
        s.lv[l].w = lw;
        s.lv[l].h = lh;
        s.lv[l].pitch = align_up(lw, kPitchAlign);
        s.lv[l].ptr = s.base + off;
        off += (size_t)s.lv[l].pitch * lh;
        off = (off + 255) & ~(size_t)255;
        lw = (lw + 1) / 2;
        lh = (lh + 1) / 2;
    }
}

size_t slot_bytes(int w, int h)
{
    size_t off = 0;
    int lw = w, lh = h;
    for (int l = 0; l < kMaxLevels; l++) {
        off += (size_t)align_up(lw, kPitchAlign) * lh;
        off = (off + 255) & ~(size_t)255;
        lw = (lw + 1) / 2;
        lh = (lh + 1) / 2;
    }
    return off + 256;
}

int pyramid_top_level(int w, int h, int win_w, int win_h, int max_level)
{
    for (int level = 0; level <= max_level; level++) {
        w = (w + 1) / 2;
        h = (h + 1) / 2;
        if (w <= win_w || h <= win_h) return level;
    }
    return max_level;
}

int check_slot(Ctx* c, int slot, bool need_image)
{
    if (slot < 0 || slot >= c->n_slots) FAIL(c, ICELK_EARG, "slot index out of range");
    if (need_image && c->slots[slot].levels_built < 1) FAIL(c, ICELK_ESTATE, "slot holds no frame");
    return ICELK_OK;
}

// An event wait costs a barrier packet on the waiting queue, processed one after the other between its kernels: none
// when the event has completed already (also: was never recorded)
int wait_event(Ctx* c, hipStream_t s, hipEvent_t e)
{
    if (hipEventQuery(e) == hipSuccess) return ICELK_OK;
    (void)hipGetLastError();   // hipErrorNotReady is the expected answer
    HIPCHK(c, hipStreamWaitEvent(s, e, 0));
    return ICELK_OK;
}

int wait_slot(Ctx* c, int slot)
{
    Slot& s = c->slots[slot];
    if (s.pending) {
        if (int rcw = wait_event(c, c->stream, s.ready)) return rcw;
        s.pending = false;
    }
    return ICELK_OK;
}

static int mark_used(Ctx* c, int slot)
{
    Slot& s = c->slots[slot];
    HIPCHK(c, hipEventRecord(s.used_own, c->stream));
    s.used = s.used_own;
    return ICELK_OK;
}

int begin_frame(Ctx* c, int slot, int w, int h)
{
    int rc = check_slot(c, slot, false);
    if (rc) return rc;
    if (!c->jpeg.slot_job.empty() && c->jpeg.slot_job[slot] >= 0)
        FAIL(c, ICELK_ESTATE, "the slot's JPEG file is still in flight (icelk_jpeg_async_finish ends it)");
    if (w <= 0 || h <= 0) FAIL(c, ICELK_EARG, "empty image");
    if (w > c->max_w || h > c->max_h) FAIL(c, ICELK_ECAP, "frame larger than max_w x max_h of icelk_create");
    rc = flush_deferred_slot(c, slot);
    if (rc) return rc;
    Slot& s = c->slots[slot];
    // a detector launch on another stream may still read the frame this slot holds (compute-stream ingest paths
    // write level 0 right after this call; the copy-stream path waits for the same event itself)
    if (int rcw = wait_event(c, c->stream, s.det_used)) return rcw;
    if (int rcw = wait_event(c, c->stream, s.eig_used)) return rcw;
    // ... and a pyramid build enqueued ahead (icelk_build_pyramid_ahead) may still be writing levels >= 1 of the frame
    // this slot held: the ingest paths below clear `pending`, so the dependency is taken here
    if (s.pending) {
        if (int rcw = wait_event(c, c->stream, s.ready)) return rcw;
    }
    s.w = w;
    s.h = h;
    layout_levels(s, w, h);
    if (!layout_ok(s)) FAIL(c, ICELK_ECAP, "slot layout violates the dword-access invariant (internal)");
    s.levels_built = 0;
    s.gen++;
    return ICELK_OK;
}

// levels levels_built .. top_level of a slot on stream st: up to three levels per launch (k_pyramid.hip); the
// level-by-level kernel (k_image.hip) stays selectable (ICELK_PYR_PER_LEVEL=1) as the second statement of the arithmetic
static int build_levels(Ctx* c, Slot& s, int top_level, hipStream_t st)
{
    const bool per_level = c->pyr_per_level;
    while (s.levels_built < top_level + 1) {
        const int l = s.levels_built;
        const int n = per_level ? 1 : std::min(3, top_level + 1 - l);
        {
            ProfScope p(c, K_PYRDOWN, st);
            if (per_level) launch_pyrdown(st, s.lv[l - 1], s.lv[l]);
            // pyramids built ahead (beside a tracker launch) use one-wave workgroups, which fit into the slot of a single
            // retiring tracker wave (k_pyramid.hip)
            else launch_pyramid_fused(st, s.lv, l - 1, n, st == c->pyr_stream);
        }
        int rc = check_launch(c, "pyramid");
        if (rc) return rc;
        s.levels_built += n;
    }
    return ICELK_OK;
}

int ensure_pyramid(Ctx* c, int slot, int top_level)
{
    Slot& s = c->slots[slot];
    int rc = wait_slot(c, slot);
    if (rc) return rc;
    if (top_level + 1 > kMaxLevels) FAIL(c, ICELK_EARG, "maxLevel too large");
    const bool build = s.levels_built < top_level + 1;
    rc = build_levels(c, s, top_level, c->stream);
    if (rc) return rc;
    return build ? mark_used(c, slot) : ICELK_OK;
}

Pyramid pyramid_of(const Slot& s)
{
    Pyramid p;
    for (int l = 0; l < kMaxLevels; l++) p.lv[l] = s.lv[l];
    return p;
}

// the counterpart of begin_frame for the ingest paths of the compute stream: level 0 of the slot is written (enqueued)
int end_frame(Ctx* c, Slot& s)
{
    HIPCHK(c, hipEventRecord(s.frame_ev, c->stream));
    s.levels_built = 1;
    s.pending = false;
    return ICELK_OK;
}

// ---- JPEG ingest: coefficients -> planes -> pixels (k_jpeg.hip) ----------------------------------------------------------
// The block rows the pixel box [left, W - right) x [top, H - bottom) needs and the blocks to transform: fills `A` and `out`
// (planes, chroma mode, box) for the transform and the output kernel, and grows job B's coefficient and plane buffers.
// The descriptor comes from the caller: nothing in it is trusted beyond what jpeg_info_ok has checked against the image size.
int jpeg_plane_args(Ctx* c, Ctx::JpegJob& B, const icelk_jpeg_info_t* I, int left, int top, int right, int bottom, JpegIdctArgs* Ap,
                    JpegOutArgs* out)
{
    if (!I) FAIL(c, ICELK_EARG, "null JPEG descriptor or coefficients");
    if (!jpeg_info_ok(*I)) FAIL(c, ICELK_EARG, "JPEG descriptor does not describe a supported file");
    if (left < 0 || top < 0 || right < 0 || bottom < 0 || (long long)left + right >= I->width ||
        (long long)top + bottom >= I->height)
        FAIL(c, ICELK_EARG, "crop box leaves no image");
    const int nc = I->ncomp;
    const bool sub_x = nc == 3 && I->hmax == 2, sub_y = nc == 3 && I->vmax == 2;
    // libjpeg filters only planes wider than 2 samples, narrower ones are replicated
    const bool fancy = I->comp_w[1] > 2;
    size_t plane_off[3], plane_bytes = 0;
    for (int k = 0; k < nc; k++) {
        plane_off[k] = plane_bytes;
        plane_bytes += (size_t)I->blocks_x[k] * 8 * I->blocks_y[k] * 8;
    }
    if (int rc = grow(c, &B.d_coef, &B.coef_cap, (size_t)I->coef_count)) return rc;
    if (int rc = grow(c, &B.d_planes, &B.planes_cap, plane_bytes)) return rc;
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
        A.coef[k] = B.d_coef + I->coef_offset[k];
        A.plane[k] = B.d_planes + plane_off[k];
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
    out->ow = I->width - left - right;
    out->oh = I->height - top - bottom;
    return ICELK_OK;
}

// jpeg_plane_args for the synchronous job, then: uploads the block rows the box needs and transforms its blocks on the
// compute stream.  on_device: the job's d_coef holds the file's coefficients already (jpeg_huff_device), nothing is uploaded.
int jpeg_planes(Ctx* c, const icelk_jpeg_info_t* I, const int16_t* coef, int left, int top, int right, int bottom, JpegOutArgs* out,
                bool on_device)
{
    if (!I || (!coef && !on_device)) FAIL(c, ICELK_EARG, "null JPEG descriptor or coefficients");
    Ctx::JpegJob& B = c->jpeg.sync;
    JpegIdctArgs A;
    if (int rc = jpeg_plane_args(c, B, I, left, top, right, bottom, &A, out)) return rc;
    for (int k = 0; k < I->ncomp && !on_device; k++) {
        // whole block rows by0 .. by0 + nby - 1: contiguous in the layout
        const int nby = (A.first[k + 1] - A.first[k]) / A.nbx[k];
        const size_t row = (size_t)I->blocks_x[k] * 64, from = I->coef_offset[k] + (size_t)A.by0[k] * row;
        HIPCHK(c, hipMemcpyAsync(B.d_coef + from, coef + from, row * nby * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
    }
    {
        ProfScope p(c, K_JPEG_IDCT);
        launch_jpeg_idct(c->stream, A);
    }
    return check_launch(c, "jpeg_idct");
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

// ---- JPEG ingest: the file's bytes -> coefficients in the synchronous job's d_coef (k_jpeg_huff.hip) ---------------------------------
// The serial decoder takes the file: when the lanes' work bound was hit, or to have the last word on a stream that
// contradicts itself.
static int jpeg_huff_fallback(Ctx* c, const uint8_t* data, uint64_t len, const icelk_jpeg_info_t& I, uint32_t why)
{
    c->jpeg.stats.fallback = why;
    std::vector<int16_t> host;
    try {
        host.resize((size_t)I.coef_count);
    } catch (...) {
        FAIL(c, ICELK_ENOMEM, "no memory for the coefficients");
    }
    if (int rc = jpeg_host_decode(data, (size_t)len, host.data(), I.coef_count)) FAIL(c, rc, "not a JPEG file, or a damaged one");
    HIPCHK(c, hipMemcpyAsync(c->jpeg.sync.d_coef, host.data(), host.size() * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

// The buffers of job J for a file of `len` bytes indexed as X (jpeg_index, jpeg_index_lanes), and the kernels' arguments.
// headroom: what grows with the file's length is taken a quarter larger than this file needs -- growing a buffer frees
// it, which waits for the whole device, and the photos of a folder all differ a little in length (asynchronous jobs).
int jpeg_huff_setup(Ctx* c, Ctx::JpegJob& J, const JpegIndex& X, uint64_t len, JpegHuffArgs* Hp, bool headroom)
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

int jpeg_huff_device(Ctx* c, const uint8_t* data, uint64_t len, icelk_jpeg_info_t* info)
{
    if (!data || !info) FAIL(c, ICELK_EARG, "null JPEG file");
    Ctx::Jpeg& J = c->jpeg;
    Ctx::JpegJob& B = J.sync;
    memset(&J.stats, 0, sizeof(J.stats));
    JpegIndex X;
    int rc = jpeg_index(data, (size_t)len, X);
    if (rc == ICELK_EUNSUP && len >= ((uint64_t)1 << 28)) {
        rc = icelk_jpeg_describe(data, len, info);
        if (rc) FAIL(c, rc, "not a JPEG file the decoder takes");
        if (int r2 = grow(c, &B.d_coef, &B.coef_cap, (size_t)info->coef_count)) return r2;
        return jpeg_huff_fallback(c, data, len, *info, ICELK_JPEG_FALLBACK_SIZE);
    }
    if (rc) FAIL(c, rc, rc == ICELK_EUNSUP ? "a JPEG file of a kind the decoder does not take" : "not a JPEG file, or a damaged one");
    *info = X.info;
    jpeg_index_lanes(X, (uint32_t)J.subseq_bits, J.max_hops);
    const lanes::Scan& A = X.scan;
    JpegHuffArgs H{};
    if (int r2 = jpeg_huff_setup(c, B, X, len, &H, false)) return r2;
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(B.d_file, data, (size_t)len, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(B.d_seg, X.seg.data(), X.seg.size() * sizeof(lanes::Seg), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(B.d_tabs, X.tabs, sizeof(X.tabs), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(B.d_ctl, 0, JH_WORDS * sizeof(uint32_t), st));
    HIPCHK(c, hipMemsetAsync(B.d_coef, 0, (size_t)X.info.coef_count * sizeof(int16_t), st));
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
    // Phases 2 and 3 and the DC pass.  The DC pass runs on whatever the lanes wrote: were they irregular, the serial
    // decoder overwrites all of it.
    {
        ProfScope p(c, K_JPEG_HUFF);
        launch_jpeg_huff_scan(st, H);
        launch_jpeg_huff_write(st, H);
        launch_jpeg_huff_dc(st, H);
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

// ---- ingest ------------------------------------------------------------------------------------
int icelk_upload_gray(icelk_t* h, int slot, const uint8_t* host, int w, int h_, int stride)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!host || stride < w) FAIL(c, ICELK_EARG, "bad host image");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = begin_frame(c, slot, w, h_);
    if (rc) return rc;
    Slot& s = c->slots[slot];
    HIPCHK(c, hipMemcpy2DAsync(s.lv[0].ptr, s.lv[0].pitch, host, stride, w, h_, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return end_frame(c, s);
}

int icelk_upload_gray_async(icelk_t* h, int slot, const uint8_t* pinned_host, int w, int h_, int stride)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Range rg("icelk upload_gray_async");
    if (!pinned_host || stride < w) FAIL(c, ICELK_EARG, "bad host image");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = begin_frame(c, slot, w, h_);
    if (rc) return rc;
    Slot& s = c->slots[slot];
    // Two streams in turn (see Ctx::copy_hi), of the high-priority class.  With streams of the compute stream's own class
    // every second upload -- always those of ONE of the two streams -- started 60-180 us after the copy before it had
    // ended (profiles/r04_c3_modes.txt): that stream shared its hardware queue with the compute stream, and the barrier
    // that carries an upload's dependencies stood behind a 250-us tracker launch.  C3 with 6 uploads in flight:
    // 3 650-3 800 -> 4 040-4 110 pairs/s (profiles/r04_c3_copy_prio.txt).
    const unsigned useq = c->upload_seq++ % 2u;
    if (!c->copy_hi[useq]) HIPCHK(c, create_priority_stream(&c->copy_hi[useq]));
    const hipStream_t cs = c->copy_hi[useq];
    // the copy must not overtake the launches that still read this slot (Slot::used / det_used)
    if (int rcw = wait_event(c, cs, s.used)) return rcw;
    if (s.pending) if (int rcw = wait_event(c, cs, s.ready)) return rcw;   // an upload or a pyramid built ahead still in flight
    if (int rcw = wait_event(c, cs, s.det_used)) return rcw;
    if (int rcw = wait_event(c, cs, s.eig_used)) return rcw;
    HIPCHK(c, hipMemcpy2DAsync(s.lv[0].ptr, s.lv[0].pitch, pinned_host, stride, w, h_, hipMemcpyHostToDevice, cs));
    HIPCHK(c, hipEventRecord(s.ready, cs));
    HIPCHK(c, hipEventRecord(s.frame_ev, cs));
    s.pending = true;
    s.levels_built = 1;
    return ICELK_OK;
}

int icelk_host_alloc(void** out, uint64_t bytes)
{
    if (!out) return ICELK_EARG;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? ICELK_OK : ICELK_ENOMEM;
}

int icelk_host_free(void* p) { return hipHostFree(p) == hipSuccess ? ICELK_OK : ICELK_EHIP; }

int icelk_upload_bgr(icelk_t* h, int slot, const uint8_t* host, int w, int h_, int stride, int gray_variant)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!host || stride < 3 * w) FAIL(c, ICELK_EARG, "bad host image");
    if (gray_variant != ICELK_GRAY_CV3 && gray_variant != ICELK_GRAY_CV4) FAIL(c, ICELK_EARG, "bad gray variant");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = begin_frame(c, slot, w, h_);
    if (rc) return rc;
    Slot& s = c->slots[slot];
    HIPCHK(c, hipMemcpy2DAsync(c->d_bgr, c->bgr_pitch, host, stride, 3 * (size_t)w, h_, hipMemcpyHostToDevice, c->stream));
    {
        ProfScope p(c, K_GRAY);
        launch_bgr2gray(c->stream, c->d_bgr, c->bgr_pitch, s.lv[0].ptr, s.lv[0].pitch, w, h_, gray_variant);
    }
    rc = check_launch(c, "bgr2gray");
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return end_frame(c, s);
}

int icelk_upload_jpeg(icelk_t* h, int slot, const icelk_jpeg_info_t* info, const int16_t* coef, int gray_variant,
                      int crop_left, int crop_top, int crop_right, int crop_bottom)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (gray_variant != ICELK_GRAY_CV3 && gray_variant != ICELK_GRAY_CV4) FAIL(c, ICELK_EARG, "bad gray variant");
    if (info && info->ncomp != 3) FAIL(c, ICELK_EARG, "expected a 3-component JPEG file");
    HIPCHK(c, hipSetDevice(c->device));
    JpegOutArgs O{};
    int rc = check_slot(c, slot, false);
    if (!rc) rc = jpeg_planes(c, info, coef, crop_left, crop_top, crop_right, crop_bottom, &O);
    if (rc) return rc;
    rc = begin_frame(c, slot, O.ow, O.oh);
    if (rc) return rc;
    Slot& s = c->slots[slot];
    O.dst = s.lv[0].ptr;
    O.dst_pitch = s.lv[0].pitch;
    {
        ProfScope p(c, K_JPEG_OUT);
        launch_jpeg_gray(c->stream, O, gray_variant);
    }
    rc = check_launch(c, "jpeg_out");
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // the caller's coefficient buffer is free again
    return end_frame(c, s);
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
    if (gray_variant != ICELK_GRAY_CV3 && gray_variant != ICELK_GRAY_CV4) FAIL(c, ICELK_EARG, "bad gray variant");
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
    rc = begin_frame(c, slot, O.ow, O.oh);
    if (rc) return rc;
    Slot& s = c->slots[slot];
    O.dst = s.lv[0].ptr;
    O.dst_pitch = s.lv[0].pitch;
    {
        ProfScope p(c, K_JPEG_OUT);
        launch_jpeg_gray(c->stream, O, gray_variant);
    }
    rc = check_launch(c, "jpeg_out");
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return end_frame(c, s);
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

int icelk_set_gray_device(icelk_t* h, int slot, const void* dev, int w, int h_, int stride)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!dev || stride < w) FAIL(c, ICELK_EARG, "bad device image");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = begin_frame(c, slot, w, h_);
    if (rc) return rc;
    Slot& s = c->slots[slot];
    HIPCHK(c, hipMemcpy2DAsync(s.lv[0].ptr, s.lv[0].pitch, dev, stride, w, h_, hipMemcpyDeviceToDevice, c->stream));
    return end_frame(c, s);
}

int icelk_cvt_bgr_device(icelk_t* h, int slot, const void* dev_bgr, int w, int h_, int stride, int gray_variant)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!dev_bgr || stride < 3 * w) FAIL(c, ICELK_EARG, "bad device image");
    if (gray_variant != ICELK_GRAY_CV3 && gray_variant != ICELK_GRAY_CV4) FAIL(c, ICELK_EARG, "bad gray variant");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = begin_frame(c, slot, w, h_);
    if (rc) return rc;
    Slot& s = c->slots[slot];
    {
        ProfScope p(c, K_GRAY);
        launch_bgr2gray(c->stream, reinterpret_cast<const uint8_t*>(dev_bgr), stride, s.lv[0].ptr, s.lv[0].pitch, w, h_,
                        gray_variant);
    }
    rc = check_launch(c, "bgr2gray");
    if (rc) return rc;
    return end_frame(c, s);
}

int icelk_synth_frame_affine(icelk_t* h, int slot, int w, int h_, int64_t ux, int64_t uy, uint32_t seed,
                             const int32_t* affine)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (affine)
        for (int k = 0; k < 4; k++)
            if (affine[k] > (1 << 13) || affine[k] < -(1 << 13)) FAIL(c, ICELK_EARG, "affine coefficient beyond +-2^-7");
    int rc = begin_frame(c, slot, w, h_);
    if (rc) return rc;
    Slot& s = c->slots[slot];
    {
        ProfScope p(c, K_SYNTH);
        launch_synth(c->stream, s.lv[0], ux, uy, seed, affine);
    }
    rc = check_launch(c, "synth");
    if (rc) return rc;
    return end_frame(c, s);
}

int icelk_synth_frame(icelk_t* h, int slot, int w, int h_, int64_t ux, int64_t uy, uint32_t seed)
{
    return icelk_synth_frame_affine(h, slot, w, h_, ux, uy, seed, nullptr);
}

int icelk_drop_pyramid(icelk_t* h, int slot)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    int rc = check_slot(c, slot, true);
    if (!rc) rc = flush_deferred_slot(c, slot);
    if (rc) return rc;
    c->slots[slot].levels_built = 1;
    return ICELK_OK;
}

int icelk_download_level(icelk_t* h, int slot, int level, uint8_t* host, int stride, int* w, int* h_)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = check_slot(c, slot, true);
    if (rc) return rc;
    Slot& s = c->slots[slot];
    if (level < 0 || level >= s.levels_built) FAIL(c, ICELK_ESTATE, "pyramid level not built");
    rc = wait_slot(c, slot);
    if (rc) return rc;
    const Level& L = s.lv[level];
    if (w) *w = L.w;
    if (h_) *h_ = L.h;
    if (host) {
        if (stride < L.w) FAIL(c, ICELK_EARG, "stride smaller than the level width");
        HIPCHK(c, hipMemcpy2DAsync(host, stride, L.ptr, L.pitch, L.w, L.h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return ICELK_OK;
}

int icelk_build_pyramid(icelk_t* h, int slot, int win_w, int win_h, int max_level, int* out_levels)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = check_slot(c, slot, true);
    if (rc) return rc;
    if (win_w <= 2 || win_h <= 2 || max_level < 0) FAIL(c, ICELK_EARG, "bad pyramid parameters");
    if (max_level > kMaxLevels - 1) max_level = kMaxLevels - 1;
    Slot& s = c->slots[slot];
    const int top = pyramid_top_level(s.w, s.h, win_w, win_h, max_level);
    rc = ensure_pyramid(c, slot, top);
    if (rc) return rc;
    if (out_levels) *out_levels = top;
    return ICELK_OK;
}

int icelk_build_pyramid_ahead(icelk_t* h, int slot, int win_w, int win_h, int max_level)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    Range rg("icelk build_pyramid_ahead");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = check_slot(c, slot, true);
    if (rc) return rc;
    if (win_w <= 2 || win_h <= 2 || max_level < 0) FAIL(c, ICELK_EARG, "bad pyramid parameters");
    if (max_level > kMaxLevels - 1) max_level = kMaxLevels - 1;
    Slot& s = c->slots[slot];
    const int top = pyramid_top_level(s.w, s.h, win_w, win_h, max_level);
    if (s.levels_built >= top + 1) return ICELK_OK;
    const hipStream_t cs = c->pyr_stream;
    // level 0 must be there (it may have been written on the compute stream), and launches that still read the
    // slot's previous pyramid must be through
    if (int rcw = wait_event(c, cs, s.frame_ev)) return rcw;
    if (s.pending) if (int rcw = wait_event(c, cs, s.ready)) return rcw;
    if (int rcw = wait_event(c, cs, s.used)) return rcw;
    rc = build_levels(c, s, top, cs);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(s.ready, cs));
    s.pending = true;
    return ICELK_OK;
}

}  // extern "C"
