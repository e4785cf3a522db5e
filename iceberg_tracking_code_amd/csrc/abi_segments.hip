// abi_segments.hip -- segment tracking: pair jobs, the deferred pair, stage / switch / cancel, template tables,
// read-out, archive and live counts.
#include "icelk_ctx.h"

namespace icelk {

// the compute stream must see the current segment set initialised (detection stream) before it touches it
static int seg_wait(Ctx* c)
{
    if (c->seg_ready_pending) {
        if (int rcw = wait_event(c, c->stream, c->sb[c->sb_cur].ready)) return rcw;
        c->seg_ready_pending = false;
    }
    return ICELK_OK;
}

// the segment-pair job of set `set` across slots s0 -> s1; `primary` jobs also fill the handle's per-feature diagnostic
// arrays (positions, status, error, distance of the latest launch) -- one job per launch can own them
static LKJob seg_job(Ctx* c, int set, const Slot& s0, const Slot& s1, const LKParams& P, bool primary)
{
    Ctx::SegBuf& S = c->sb[set];
    LKJob j{};
    j.I = pyramid_of(s0);
    j.J = pyramid_of(s1);
    j.n = S.upper;
    LKBuffers& B = j.B;
    B.p_in = S.live;
    if (primary) {
        B.p_fwd = c->d_p1;
        B.st_fwd = c->d_st_f;
        B.p_bwd = c->d_p0r;
        B.st_bwd = c->d_st_b;
        // no err_fwd / err_bwd: the segment loop has no use for the residual error (s1:323,326 drop it), and the tracker
        // kernels skip forming it when nobody takes it
        B.dist = c->d_dist;
        B.valid = c->d_valid;
    }
    B.seg_alive = S.alive;
    B.order = c->use_order ? S.order : nullptr;
    B.order_border = c->use_order ? S.order_border : nullptr;
    // Dealing the sorted sequence to the XCDs pays while neighbouring windows barely overlap (C2: 244 -> 233 us);
    // with dense features every XCD would work on one spot of the frame at a time and its L2 channels
    // serialise (REF: 2 060 us walking the table linearly, 2 680 us dealt, 2 230 us unsorted)
    const double overlap = (double)(P.win_w + 12) * (P.win_h + 12) * S.upper / ((double)s0.w * s0.h);
    B.order_plain = overlap >= 2.0 ? 1 : 0;
    B.seg_xy = S.live;
    B.seg_tracks = S.tracks;
    B.seg_quality = S.quality;
    B.seg_vert = S.vert;
    B.seg_max_vert = kMaxVert;
    B.seg_tracked = c->d_tracked;
    // templates: taken from the pair before if it left them for this vertex, left for the pair after unless this is the
    // segment's last
    const int quads = lk_fast_eligible(P) ? lk_template_quads(P.win_w, P.win_h) : 0;
    const int key = (P.win_w << 16) | (P.win_h << 8) | (P.top_level + 1);
    // (the templates were built on the frame and pyramid that sat in the pair's second slot: they serve the next pair
    // only if that very frame is now its first)
    const int slot0 = (int)(&s0 - c->slots.data()), slot1 = (int)(&s1 - c->slots.data());
    bool take = quads > 0 && S.tmpl_for == S.vert && S.tmpl_key == key && S.tmpl_slot == slot0 && S.tmpl_gen == s0.gen;
    S.tmpl_for = -1;
    if (quads > 0 && !c->tmpl.off) {
        const bool last = c->track_len_hint > 0 && S.vert >= c->track_len_hint;
        const size_t per_row = (size_t)(P.top_level + 1) * ((size_t)quads * 64) * 16;
        const size_t need = (size_t)std::max(S.upper, 1) * per_row;
        // The two tables are sized ONCE per row geometry (window, levels), for max_pts rows within the handle's template
        // budget (ICELK_TEMPLATE_BUDGET_MB, default 8 GB for both; never more than half of what the device has free) --
        // not by the segments seen: growing them meant hipFree + hipMalloc in the middle of the frame loop (a device-wide
        // synchronisation) while a pair held back by icelk_seg_track_defer could still point into the freed table.  A
        // segment with more tracks than rows fit simply takes no part.  Another row geometry (other LK parameters) is the
        // one case that allocates again: a waiting pair goes out first, and hipFree waits for whatever is in flight.
        if (!last && c->tmpl.row_bytes != per_row) {
            if (c->defer.pending) (void)flush_deferred(c);   // its job carries pointers into the tables about to go
            for (void*& b : c->tmpl.buf) {
                if (b) hipFree(b);
                b = nullptr;
            }
            c->tmpl.bytes = 0;
            c->tmpl.row_bytes = per_row;
            for (Ctx::SegBuf& o : c->sb) o.tmpl_for = -1;
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
            const size_t budget = std::min(c->tmpl.budget / 2, free_b / 4);   // per table
            const size_t rows = std::min((size_t)std::max(c->max_pts, 1), budget / per_row);
            const size_t alloc = rows * per_row;
            if (rows > 0 && hipMalloc(&c->tmpl.buf[0], alloc) == hipSuccess && hipMalloc(&c->tmpl.buf[1], alloc) == hipSuccess) {
                c->tmpl.bytes = alloc;
            } else {
                (void)hipGetLastError();
                if (c->tmpl.buf[0]) hipFree(c->tmpl.buf[0]);
                c->tmpl.buf[0] = c->tmpl.buf[1] = nullptr;
                c->tmpl.off = true;   // no room: every pair builds its own templates, as before (icelk_seg_template_info says so)
                c->tmpl.failed = true;
            }
        }
        if (c->tmpl.row_bytes != per_row) take = false;   // (the last pair of a segment with another row geometry)
        if (c->tmpl.bytes >= need && c->tmpl.row_bytes == per_row) {
            B.tmpl_levels = P.top_level + 1;
            if (take) {
                B.tmpl_in = c->tmpl.buf[set & 1];
                c->tmpl.taken++;
            }
            if (!last) {
                c->tmpl.left++;
                B.tmpl_out = c->tmpl.buf[set & 1];
                S.tmpl_for = S.vert + 1;
                S.tmpl_key = key;
                S.tmpl_slot = slot1;
                S.tmpl_gen = s1.gen;
            }
        }
    }
    return j;
}

// one event behind a tracker launch, for everything the launch read or wrote
static int record_launch(Ctx* c, hipEvent_t* ev)
{
    *ev = c->launch_ev[c->launch_seq++ % kLaunchEvents];
    HIPCHK(c, hipEventRecord(*ev, c->stream));
    return ICELK_OK;
}

static void seg_launched(Ctx* c, hipEvent_t ev, int set, int slot_prev, int slot_next)
{
    c->slots[slot_prev].used = ev;
    c->slots[slot_next].used = ev;
    c->sb[set].used = ev;
}

// a pair waiting for a partner goes out on its own
int flush_deferred(Ctx* c)
{
    if (!c->defer.pending) return ICELK_OK;
    Ctx::Deferred& d = c->defer;
    d.pending = false;
    int rc;
    {
        ProfScope p(c, K_LK_FB);
        rc = launch_lk(c->stream, d.job.I, d.job.J, d.job.B, d.job.n, d.P, true);
    }
    if (rc) FAIL(c, rc, "unsupported window size");
    rc = check_launch(c, "lk_fb");
    if (rc) return rc;
    hipEvent_t ev;
    rc = record_launch(c, &ev);
    if (rc) return rc;
    seg_launched(c, ev, d.set, d.slot_prev, d.slot_next);
    return ICELK_OK;
}

// before a slot's frame or pyramid is overwritten: a waiting pair that reads it must have been launched
int flush_deferred_slot(Ctx* c, int slot)
{
    if (c->defer.pending && (c->defer.slot_prev == slot || c->defer.slot_next == slot)) return flush_deferred(c);
    return ICELK_OK;
}

static bool same_lk_params(const LKParams& a, const LKParams& b)
{
    return a.win_w == b.win_w && a.win_h == b.win_h && a.top_level == b.top_level && a.max_count == b.max_count &&
           a.eps2 == b.eps2 && a.flags == b.flags && a.min_eig_thr == b.min_eig_thr && a.fb_thr == b.fb_thr &&
           a.margin == b.margin && a.dist_form == b.dist_form && a.sum_mode == b.sum_mode &&
           a.sum_guard == b.sum_guard;
}

// shared by icelk_seg_track / icelk_seg_track_async / icelk_seg_track_defer
static int seg_track_core(Ctx* c, int slot_prev, int slot_next, int win_w, int win_h, int max_level, int crit_type,
                          int max_count, double epsilon, double min_eig_threshold, float fb_threshold, bool defer)
{
    Range rg(defer ? "icelk seg_track_defer" : "icelk seg_track (fused forward+backward LK launch)");
    int rc = check_slot(c, slot_prev, true);
    if (!rc) rc = check_slot(c, slot_next, true);
    if (rc) return rc;
    if (!c->seg_active) FAIL(c, ICELK_ESTATE, "icelk_seg_detect has not been called");
    Ctx::SegBuf& S = c->sb[c->sb_cur];
    if (S.vert >= kMaxVert) FAIL(c, ICELK_ECAP, "segment longer than the device track table");
    Slot& s0 = c->slots[slot_prev];
    Slot& s1 = c->slots[slot_next];
    if (s0.w != s1.w || s0.h != s1.h) FAIL(c, ICELK_EARG, "frame sizes differ");
    LKParams P;
    rc = make_lk_params(c, s0.w, s0.h, win_w, win_h, max_level, crit_type, max_count, epsilon, 0, min_eig_threshold,
                        fb_threshold, &P);
    if (rc) return rc;
    // a waiting pair of THIS segment comes first (pairs of a segment are sequential)
    if (c->defer.pending && c->defer.set == c->sb_cur) {
        rc = flush_deferred(c);
        if (rc) return rc;
    }
    rc = ensure_pyramid(c, slot_prev, P.top_level);
    if (!rc) rc = ensure_pyramid(c, slot_next, P.top_level);
    if (rc) return rc;
    rc = seg_wait(c);
    if (rc) return rc;
    if (S.upper > 0) {
        // tiles (half window + search margin) of a feature this close to the edge reach over it at the upper levels
        c->border_px = (std::max(win_w, win_h) / 2 + kLkTileMargin + 2) << std::max(P.top_level - 1, 0);
        LKJob job = seg_job(c, c->sb_cur, s0, s1, P, true);
        // workgroup stamps describe ONE job: no pairing while they are on -- unless ICELK_LK_STAMPS_PAIR asks for the
        // stamps of a joint launch (indexed by workgroup: tools/lk_stamps_pair.py tells the jobs apart)
        static const bool stamp_pairs = getenv("ICELK_LK_STAMPS_PAIR") != nullptr;
        const bool diag = c->d_stamps != nullptr && !stamp_pairs;
        if (defer && !c->defer.pending && !diag) {
            // nothing goes out now: the pair waits for the first pair of the next segment (or another waiting pair)
            Ctx::Deferred& d = c->defer;
            d.pending = true;
            d.set = c->sb_cur;
            d.slot_prev = slot_prev;
            d.slot_next = slot_next;
            d.job = job;
            d.P = P;
            S.vert += 1;
            return ICELK_OK;
        }
        bool paired = false;
        if (c->defer.pending) {
            Ctx::Deferred& d = c->defer;
            if (!diag && same_lk_params(d.P, P)) {
                LKJob other = d.job;
                // the diagnostic arrays belong to the job of the current segment
                other.B.p_fwd = other.B.p_bwd = other.B.err_fwd = other.B.err_bwd = other.B.dist = nullptr;
                other.B.st_fwd = other.B.st_bwd = other.B.valid = nullptr;
                if (c->d_stamps && stamp_pairs && (size_t)(other.n + job.n + 32) <= c->stamps_cap) {
                    other.B.stamps = job.B.stamps = c->d_stamps;
                    hipMemsetAsync(c->d_stamps, 0, 3 * c->stamps_cap * 8, c->stream);
                }
                {
                    ProfScope p(c, K_LK_FB_PAIR);
                    paired = launch_lk_pair(c->stream, other, job, P);
                }
                if (paired) {
                    d.pending = false;
                    rc = check_launch(c, "lk_fb_pair");
                    if (rc) return rc;
                }
            }
            if (!paired) {
                rc = flush_deferred(c);
                if (rc) return rc;
            }
        }
        if (!paired) {
            LKBuffers& B = job.B;
            if (c->prof) {
                B.iters = c->d_iters;
                c->iters_n = S.upper;
                hipMemsetAsync(c->d_iters, 0xff, sizeof(uint32_t) * (size_t)S.upper, c->stream);   // dead tracks stay ~0
            }
            if (c->d_stamps && !stamp_pairs) {
                B.stamps = c->d_stamps;
                hipMemsetAsync(c->d_stamps, 0, 3 * c->stamps_cap * 8, c->stream);
            }
            {
                ProfScope p(c, K_LK_FB);
                rc = launch_lk(c->stream, job.I, job.J, B, job.n, P, true);
            }
            if (rc) FAIL(c, rc, "unsupported window size");
            rc = check_launch(c, "lk_fb");
            if (rc) return rc;
        }
        hipEvent_t ev;
        rc = record_launch(c, &ev);
        if (rc) return rc;
        if (paired) seg_launched(c, ev, c->defer.set, c->defer.slot_prev, c->defer.slot_next);
        seg_launched(c, ev, c->sb_cur, slot_prev, slot_next);
    } else if (c->defer.pending && !defer) {
        rc = flush_deferred(c);
        if (rc) return rc;
    }
    S.vert += 1;
    return ICELK_OK;
}

}  // namespace icelk

using namespace icelk;

extern "C" {

// ---- segment state -----------------------------------------------------------------------------
int icelk_seg_detect_begin(icelk_t* h, int slot, int use_mask, int max_corners, double quality_level,
                            double min_distance, int block_size)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    return detect_begin(c, slot, use_mask, max_corners, quality_level, min_distance, block_size, true);
}

int icelk_seg_detect_prepare(icelk_t* h, int slot, int use_mask, int block_size)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (block_size <= 0) FAIL(c, ICELK_EARG, "bad detector parameters");
    return detect_prepare(c, slot, use_mask, block_size);
}

// The corners of the detection in flight become a new segment in the OTHER set of segment buffers (the current one
// keeps being tracked); icelk_seg_switch makes it current.
static int seg_stage(Ctx* c, int max_corners, int* out_n)
{
    if (c->seg_staged) FAIL(c, ICELK_ESTATE, "a staged segment is waiting for icelk_seg_switch");
    // the new segment goes into the set after the current one, on the tail stream right behind the corner list
    Ctx::SegBuf& nb = c->sb[(c->sb_cur + 1) % kSegSets];
    DetectResult r;
    int rc = detect_finish(c, max_corners, c->max_pts, &nb, &r);
    if (rc) return rc;
    if (!r.order_written) {
        const hipStream_t ds = c->tail_stream;
        if (!r.tables_written) {
            // launches that still touch that set (a segment closed several switches ago) must be through
            if (int rcw = wait_event(c, ds, nb.used)) return rcw;
            launch_seg_init(ds, c->d_corners, r.n, nb.live, nb.alive, nb.tracks, kMaxVert);
        }
        if (c->use_order) launch_seg_order(ds, c->d_corners, r.n, r.w, r.h, c->border_px, nb.order, nb.order_border);
        rc = check_launch(c, "seg_init");
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(c->corners_free, ds));
        HIPCHK(c, hipEventRecord(nb.ready, ds));
    }
    c->seg_staged = true;
    c->staged_n = r.n;
    if (out_n) *out_n = r.n;
    return ICELK_OK;
}

static int seg_switch(Ctx* c)
{
    if (!c->seg_staged) FAIL(c, ICELK_ESTATE, "no staged segment (icelk_seg_detect_stage has not been called)");
    // a pair still waiting from before the previous switch has found no partner
    if (c->defer.pending && c->defer.set != c->sb_cur) {
        int rc = flush_deferred(c);
        if (rc) return rc;
    }
    c->seg_staged = false;
    c->closed_valid = c->seg_active;
    c->sb_cur = (c->sb_cur + 1) % kSegSets;
    c->seg_ready_pending = true;
    c->sb[c->sb_cur].vert = 1;
    c->sb[c->sb_cur].tmpl_for = -1;
    c->sb[c->sb_cur].upper = c->staged_n;
    c->seg_active = true;
    return ICELK_OK;
}

int icelk_seg_detect_stage(icelk_t* h, int max_corners, int* out_n)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    return seg_stage(c, max_corners, out_n);
}

int icelk_seg_detect_stage_try(icelk_t* h, int max_corners, int* out_n, int* out_done)
{
    if (!h || !out_done) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    *out_done = 0;
    if (c->seg_staged) FAIL(c, ICELK_ESTATE, "a staged segment is waiting for icelk_seg_switch");
    bool arrived = false;
    int rc = detect_counts_arrived(c, &arrived);
    if (rc || !arrived) return rc;
    rc = seg_stage(c, max_corners, out_n);
    if (rc) return rc;
    *out_done = 1;
    return ICELK_OK;
}

int icelk_seg_switch(icelk_t* h)
{
    if (!h) return ICELK_EARG;
    return seg_switch(C(h));
}

int icelk_seg_detect_cancel(icelk_t* h)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    // whatever was enqueued for the abandoned detections runs to its end: nothing is left reading a slot or a mask
    HIPCHK(c, hipStreamSynchronize(c->eig_stream));
    HIPCHK(c, hipStreamSynchronize(c->det_stream));
    HIPCHK(c, hipStreamSynchronize(c->tail_stream));
    for (auto& S : c->dset)
        if (S.job.active) {
            S.job.active = false;
            S.counters_clean = false;   // its counters were never reset by a tail: the next detection of the set resets them
        }
    for (auto& e : c->eo) e.valid = false;   // prepared candidates are dropped
    c->seg_staged = false;                   // a staged segment is forgotten (its set is simply staged into again)
    return ICELK_OK;
}

int icelk_seg_detect_finish(icelk_t* h, int max_corners, int* out_n)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = seg_stage(c, max_corners, out_n);
    if (rc) return rc;
    return seg_switch(c);
}

int icelk_seg_detect(icelk_t* h, int slot, int use_mask, int max_corners, double quality_level, double min_distance,
                     int block_size, int* out_n)
{
    int rc = icelk_seg_detect_begin(h, slot, use_mask, max_corners, quality_level, min_distance, block_size);
    if (rc) return rc;
    return icelk_seg_detect_finish(h, max_corners, out_n);
}

int icelk_seg_track_async(icelk_t* h, int slot_prev, int slot_next, int win_w, int win_h, int max_level, int crit_type,
                          int max_count, double epsilon, double min_eig_threshold, float fb_threshold)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    return seg_track_core(c, slot_prev, slot_next, win_w, win_h, max_level, crit_type, max_count, epsilon,
                          min_eig_threshold, fb_threshold, false);
}

int icelk_seg_track_defer(icelk_t* h, int slot_prev, int slot_next, int win_w, int win_h, int max_level, int crit_type,
                          int max_count, double epsilon, double min_eig_threshold, float fb_threshold)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    return seg_track_core(c, slot_prev, slot_next, win_w, win_h, max_level, crit_type, max_count, epsilon,
                          min_eig_threshold, fb_threshold, true);
}

int icelk_seg_track_len_hint(icelk_t* h, int track_len)
{
    if (!h || track_len < 0) return ICELK_EARG;
    C(h)->track_len_hint = track_len;
    return ICELK_OK;
}

int icelk_seg_template_stats(icelk_t* h, long long* out)
{
    if (!h || !out) return ICELK_EARG;
    out[0] = C(h)->tmpl.taken;
    out[1] = C(h)->tmpl.left;
    return ICELK_OK;
}

int icelk_seg_template_info(icelk_t* h, long long* bytes_per_table, long long* rows, int* state)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (bytes_per_table) *bytes_per_table = (long long)c->tmpl.bytes;
    if (rows) *rows = c->tmpl.row_bytes ? (long long)(c->tmpl.bytes / c->tmpl.row_bytes) : 0;
    if (state) *state = c->tmpl.failed ? 2 : (c->tmpl.off ? 1 : 0);
    return ICELK_OK;
}

int icelk_seg_tail_stats(icelk_t* h, long long* out)
{
    if (!h || !out) return ICELK_EARG;
    out[0] = C(h)->tails_dev;
    out[1] = C(h)->tails_host;
    return ICELK_OK;
}

int icelk_seg_flush(icelk_t* h)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    return flush_deferred(c);
}

// which segment a read-out addresses: the current one, or the one closed by the latest switch
static int seg_pick(Ctx* c, bool closed, int* set)
{
    if (!c->seg_active) FAIL(c, ICELK_ESTATE, "icelk_seg_detect has not been called");
    if (closed && !c->closed_valid) FAIL(c, ICELK_ESTATE, "no closed segment");
    *set = closed ? (c->sb_cur + kSegSets - 1) % kSegSets : c->sb_cur;
    // its waiting pair, if any, belongs to the result
    if (c->defer.pending && c->defer.set == *set) {
        int rc = flush_deferred(c);
        if (rc) return rc;
    }
    return closed ? ICELK_OK : seg_wait(c);
}

static int seg_live_core(Ctx* c, bool closed, int* out_live, int64_t* out_tracked_total)
{
    int set = 0;
    int rc = seg_pick(c, closed, &set);
    if (rc) return rc;
    launch_seg_stats(c->stream, c->sb[set].alive, c->sb[set].upper, c->d_tracked, c->h_seg);
    rc = check_launch(c, "seg_stats");
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int n = (int)c->h_seg[0];
    const unsigned long long t = c->h_seg[1];
    if (out_live) *out_live = n;
    if (out_tracked_total) *out_tracked_total = (int64_t)t;
    return ICELK_OK;
}

int icelk_seg_live(icelk_t* h, int* out_live, int64_t* out_tracked_total)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    return seg_live_core(c, false, out_live, out_tracked_total);
}

int icelk_seg_track(icelk_t* h, int slot_prev, int slot_next, int win_w, int win_h, int max_level, int crit_type,
                    int max_count, double epsilon, double min_eig_threshold, float fb_threshold, int* out_live)
{
    int rc = icelk_seg_track_async(h, slot_prev, slot_next, win_w, win_h, max_level, crit_type, max_count, epsilon,
                                   min_eig_threshold, fb_threshold);
    if (rc) return rc;
    return icelk_seg_live(h, out_live, nullptr);
}

static int seg_read_core(Ctx* c, bool closed, float* tracks, float* quality, int cap, int max_vertices, int* out_n,
                         int* out_vertices)
{
    int n = 0;
    int rc = seg_live_core(c, closed, &n, nullptr);
    if (rc) return rc;
    Ctx::SegBuf& S = c->sb[closed ? (c->sb_cur + kSegSets - 1) % kSegSets : c->sb_cur];
    const int nv = S.vert;
    if (out_n) *out_n = n;
    if (out_vertices) *out_vertices = nv;
    if (!tracks && !quality) return ICELK_OK;
    if (n > cap || nv > max_vertices) FAIL(c, ICELK_ECAP, "host track buffers too small");
    if (n == 0) return ICELK_OK;
    launch_seg_gather(c->stream, S.alive, S.upper, S.tracks, S.quality, nv, kMaxVert, c->d_out_tracks, c->d_out_quality);
    rc = check_launch(c, "seg_gather");
    if (rc) return rc;
    // host layout: (n, max_vertices, 2) and (n, max_vertices-1) with the caller's vertex dimension
    if (tracks)
        HIPCHK(c, hipMemcpy2DAsync(tracks, sizeof(float) * 2 * max_vertices, c->d_out_tracks, sizeof(float) * 2 * nv,
                                   sizeof(float) * 2 * nv, n, hipMemcpyDeviceToHost, c->stream));
    if (quality && nv > 1)
        HIPCHK(c, hipMemcpy2DAsync(quality, sizeof(float) * (max_vertices - 1), c->d_out_quality, sizeof(float) * (nv - 1),
                                   sizeof(float) * (nv - 1), n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

}  // extern "C"

// The surviving tracks of the current segment (closed: of the one the latest switch closed), packed (n, vertices, 2) in
// the handle's read-out buffer d_out_tracks, on the compute stream: what the read-outs copy to the host, for a consumer
// on the device (abi_plot.hip).  A pair of the segment that still waits goes out first.  Waits for the count.
int icelk::seg_gather_packed(Ctx* c, bool closed, int* out_n, int* out_vertices)
{
    int n = 0;
    if (int rc = seg_live_core(c, closed, &n, nullptr)) return rc;
    Ctx::SegBuf& S = c->sb[closed ? (c->sb_cur + kSegSets - 1) % kSegSets : c->sb_cur];
    *out_n = n;
    *out_vertices = S.vert;
    if (n == 0) return ICELK_OK;
    launch_seg_gather(c->stream, S.alive, S.upper, S.tracks, S.quality, S.vert, kMaxVert, c->d_out_tracks, c->d_out_quality);
    return check_launch(c, "seg_gather");
}

// The same without the wait: the rows are counted on the device (*dev_count, written on the compute stream), *out_upper
// bounds them.  What a consumer that needs no host look in between starts from (abi_stab.hip).
int icelk::seg_gather_counted(Ctx* c, bool closed, int* dev_count, int* out_upper, int* out_vertices)
{
    int set = 0;
    if (int rc = seg_pick(c, closed, &set)) return rc;
    Ctx::SegBuf& S = c->sb[set];
    *out_upper = S.upper;
    *out_vertices = S.vert;
    launch_seg_gather(c->stream, S.alive, S.upper, S.tracks, S.quality, S.vert, kMaxVert, c->d_out_tracks, c->d_out_quality, dev_count);
    return check_launch(c, "seg_gather");
}

extern "C" {

int icelk_seg_read(icelk_t* h, float* tracks, float* quality, int cap, int max_vertices, int* out_n, int* out_vertices)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    return seg_read_core(c, false, tracks, quality, cap, max_vertices, out_n, out_vertices);
}

int icelk_seg_read_closed(icelk_t* h, float* tracks, float* quality, int cap, int max_vertices, int* out_n,
                          int* out_vertices)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    return seg_read_core(c, true, tracks, quality, cap, max_vertices, out_n, out_vertices);
}

static int seg_archive_core(Ctx* c, bool closed, void* dev_tracks, void* dev_quality, void* dev_count, int cap_rows,
                            int* out_vertices)
{
    if (!dev_tracks || !dev_count) FAIL(c, ICELK_EARG, "null device buffer");
    int set = 0;
    int rc = seg_pick(c, closed, &set);
    if (rc) return rc;
    Ctx::SegBuf& S = c->sb[set];
    if (cap_rows < S.upper) FAIL(c, ICELK_ECAP, "archive rows < tracks of the segment");
    const int nv = S.vert;
    if (out_vertices) *out_vertices = nv;
    // quality is optional: the gather kernel writes it next to the tracks; without a destination it goes to the
    // handle's own read-out buffer
    launch_seg_gather(c->stream, S.alive, S.upper, S.tracks, S.quality, nv, kMaxVert, reinterpret_cast<float*>(dev_tracks),
                      dev_quality ? reinterpret_cast<float*>(dev_quality) : c->d_out_quality, reinterpret_cast<int*>(dev_count));
    rc = check_launch(c, "seg_archive");
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(S.used_own, c->stream));
    S.used = S.used_own;
    return ICELK_OK;
}

int icelk_seg_archive(icelk_t* h, void* dev_tracks, void* dev_quality, void* dev_count, int cap_rows, int* out_vertices)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    return seg_archive_core(c, false, dev_tracks, dev_quality, dev_count, cap_rows, out_vertices);
}

int icelk_seg_archive_closed(icelk_t* h, void* dev_tracks, void* dev_quality, void* dev_count, int cap_rows,
                             int* out_vertices)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    return seg_archive_core(c, true, dev_tracks, dev_quality, dev_count, cap_rows, out_vertices);
}

int icelk_seg_project(icelk_t* h, const icelk_camera_t* cam, const icelk_utm_filter_t* filt, int cap, int max_vectors,
                      double* x, double* y, double* u, double* v, double* speed, uint8_t* keep, int* out_n,
                      int* out_vectors)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = check_projection_args(c, cam, filt);
    if (rc) return rc;
    if (!c->seg_active) FAIL(c, ICELK_ESTATE, "icelk_seg_detect has not been called");
    int n = 0;
    rc = icelk_seg_live(h, &n, nullptr);
    if (rc) return rc;
    Ctx::SegBuf& S = c->sb[c->sb_cur];
    const int nv = S.vert;
    if (out_n) *out_n = n;
    if (out_vectors) *out_vectors = nv - 1;
    if (n > cap || nv - 1 > max_vectors) FAIL(c, ICELK_ECAP, "host buffers too small");
    if (n == 0) return ICELK_OK;
    launch_seg_gather(c->stream, S.alive, S.upper, S.tracks, S.quality, nv, kMaxVert, c->d_out_tracks, c->d_out_quality);
    rc = check_launch(c, "seg_gather");
    if (rc) return rc;
    return project_core(c, c->d_out_tracks, n, nv, cam, filt, max_vectors, x, y, u, v, speed, keep);
}

}  // extern "C"
