// abi_frames.hip -- frame slots: layout, slot events, pyramids, the uploads of pixels, level download (JPEG files:
// abi_jpeg_ingest.hip).
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

// Waits until the pinned word holds seq (a kernel's system-scope release store) by polling it: the host learns of it when
// it lands in its memory, not when the runtime has processed an event's completion signal and woken the thread.  The
// event behind that kernel is looked at now and then, so that a failed launch ends the wait with its error, not a hang
int await_pinned_seq(Ctx* c, const int* word, int seq, hipEvent_t ev)
{
    for (unsigned it = 1;; it++) {
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return ICELK_OK;
        if ((it & 4095u) == 0) {
            const hipError_t q = hipEventQuery(ev);
            if (q == hipSuccess) break;             // complete: the synchronize below returns at once
            if (q != hipErrorNotReady) HIPCHK(c, q);
            (void)hipGetLastError();
        }
        __builtin_ia32_pause();
    }
    HIPCHK(c, hipEventSynchronize(ev));
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

// A stream other than the compute stream is about to write level 0 of slot s (begin_frame has been through): the write
// must not overtake the launches that still read the slot (Slot::used / det_used / eig_used), nor an upload or a
// pyramid built ahead that is still in flight
int foreign_write_begin(Ctx* c, Slot& s, hipStream_t st)
{
    if (int rc = wait_event(c, st, s.used)) return rc;
    if (s.pending) if (int rc = wait_event(c, st, s.ready)) return rc;
    if (int rc = wait_event(c, st, s.det_used)) return rc;
    return wait_event(c, st, s.eig_used);
}

// ... and has written it (enqueued): the counterpart of end_frame
int foreign_write_end(Ctx* c, Slot& s, hipStream_t st)
{
    HIPCHK(c, hipEventRecord(s.ready, st));
    HIPCHK(c, hipEventRecord(s.frame_ev, st));
    s.pending = true;
    s.levels_built = 1;
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
    if (int rcw = foreign_write_begin(c, s, cs)) return rcw;
    HIPCHK(c, hipMemcpy2DAsync(s.lv[0].ptr, s.lv[0].pitch, pinned_host, stride, w, h_, hipMemcpyHostToDevice, cs));
    return foreign_write_end(c, s, cs);
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
    if (int rcv = check_gray_variant(c, gray_variant)) return rcv;
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
    if (int rcv = check_gray_variant(c, gray_variant)) return rcv;
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
