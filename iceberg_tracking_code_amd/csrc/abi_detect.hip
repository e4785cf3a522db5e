// abi_detect.hip -- corner detector: candidate buffers, detector sets, the counts round trip, prepare / begin /
// finish, mask, icelk_min_eig_map, icelk_good_features, statistics.
#include "icelk_ctx.h"

namespace icelk {

// ---- candidate buffers and detector sets: allocation and release ----------------------------------------------------
int alloc_eig_out(Ctx* c, Ctx::EigOut& e, int cand_cap)
{
    const int w = c->max_w, h = c->max_h;
    CandBuf& b = e.buf;
    int rc;
    if ((rc = dmalloc(c, &b.max_key, 1)) || (rc = dmalloc(c, &b.raw, (size_t)cand_cap)) ||
        (rc = dmalloc(c, &b.blk_count, candidate_blocks(w, h) * 4)))
        return rc;
    // the two-pass detector's scratch (~20 MB per buffer at 12 MP) only on a handle created with its switch set: a
    // handle without it runs the strip kernel whatever the switch says later (launch_candidates looks at D.cb.acand)
    if (getenv("ICELK_TWO_PASS_CORNERS") &&
        ((rc = dmalloc(c, &b.acand, fast_cand_entries(w, h))) || (rc = dmalloc(c, &b.acount, fast_tiles(w, h))) ||
         (rc = dmalloc(c, &b.amaxc, fast_max_entries(w, h))) || (rc = dmalloc(c, &b.amaxn, fast_tiles(w, h))) ||
         (rc = dmalloc(c, &b.aemax, fast_tiles(w, h))) || (rc = dmalloc(c, &b.fmax_key, 8)) ||
         (rc = dmalloc(c, &b.aties, fast_cand_entries(w, h) + fast_tiles(w, h)))))
        return rc;
    if (hipEventCreateWithFlags(&e.done, hipEventDisableTiming) != hipSuccess) FAIL(c, ICELK_EHIP, "hipEventCreate failed");
    return ICELK_OK;
}

void free_eig_out(Ctx::EigOut& e)
{
    const CandBuf& b = e.buf;
    void* p[] = {b.raw, b.blk_count, b.max_key, b.acand, b.acount, b.amaxc, b.amaxn, b.aemax, b.fmax_key, b.aties};
    for (void* q : p)
        if (q) hipFree(q);
    if (e.done) hipEventDestroy(e.done);
}

// everything a detection in flight owns but its candidate buffer; D.eig is set by the caller (one map for both sets)
int alloc_det_set(Ctx* c, Ctx::DetSet& S, int cand_cap)
{
    DetectScratch& D = S.D;
    D.cand_cap = cand_cap;
    D.sort_tmp_bytes = sort_tmp_bytes(cand_cap);
    const size_t nc = c->ncell_cap;
    int rc;
    if ((rc = dmalloc(c, &D.cand, (size_t)cand_cap)) || (rc = dmalloc(c, &D.cand_count, 1)) ||
        (rc = dmalloc(c, &D.cell_count, nc)) || (rc = dmalloc(c, &D.cell_start, nc)) || (rc = dmalloc(c, &D.cell_fill, nc)) ||
        (rc = dmalloc(c, &D.chunk_tot, (nc / 2048 + 2) * 32)) || (rc = dmalloc(c, &D.cell_cand, (size_t)cand_cap)) ||
        (rc = dmalloc(c, &D.state, (size_t)cand_cap)) || (rc = dmalloc(c, &D.undecided, 64)) ||
        (rc = dmalloc(c, &D.acc, (size_t)cand_cap)) || (rc = dmalloc(c, &D.acc_sorted, (size_t)cand_cap)) ||
        (rc = dmalloc(c, &D.acc_count, 1)) || (rc = dmalloc(c, &D.key_hist, 1 << 16)) || (rc = dmalloc(c, &D.prune_key, 1)) ||
        (rc = dmalloc(c, (uint8_t**)&D.sort_tmp, D.sort_tmp_bytes)) || (rc = dmalloc(c, &D.tail_ctl, TC_WORDS_)) ||
        (rc = dmalloc(c, &D.tail_resp, tail_resp_words())) || (rc = dmalloc(c, &D.tail_bins, kTailOrderBins + 2)))
        return rc;
    if (hipMemset(D.tail_resp, 0, sizeof(int) * tail_resp_words()) != hipSuccess ||
        hipMemset(D.tail_ctl, 0, sizeof(int) * TC_WORDS_) != hipSuccess ||
        hipMemset(D.tail_bins, 0, sizeof(int) * (kTailOrderBins + 2)) != hipSuccess)
        FAIL(c, ICELK_EHIP, "hipMemset failed");
    if (hipHostMalloc(reinterpret_cast<void**>(&S.h_counts), sizeof(int) * CW_WORDS_, hipHostMallocMapped) != hipSuccess ||
        hipEventCreateWithFlags(&S.counts_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.tail_done, hipEventDisableTiming) != hipSuccess)
        FAIL(c, ICELK_EHIP, "hipHostMalloc failed");
    memset(S.h_counts, 0, sizeof(int) * CW_WORDS_);
    return ICELK_OK;
}

void free_det_set(Ctx::DetSet& S)
{
    const DetectScratch& D = S.D;
    void* p[] = {D.cand, D.cand_count, D.cell_count, D.cell_start, D.cell_fill, D.chunk_tot, D.cell_cand, D.state, D.undecided,
                 D.acc, D.acc_sorted, D.acc_count, D.key_hist, D.prune_key, D.sort_tmp, D.tail_ctl, D.tail_resp, D.tail_bins};
    for (void* q : p)
        if (q) hipFree(q);
    if (S.h_counts) hipHostFree(S.h_counts);
    if (S.counts_ev) hipEventDestroy(S.counts_ev);
    if (S.tail_done) hipEventDestroy(S.tail_done);
}

// ---- detector core shared by icelk_good_features and icelk_seg_detect --------------------------
// detect_begin enqueues K6..K8 on the detection stream and returns at once; detect_finish waits for the
// counts, sorts the accepted corners and leaves the first of them in c->d_corners (device), in response order.
__global__ void k_publish_counts(const int* __restrict__ cand, const int* __restrict__ acc,
                                 const int* __restrict__ undecided, const unsigned* __restrict__ prune_key,
                                 int* __restrict__ host_out, int seq)
{
    host_out[CW_CAND] = *cand;
    host_out[CW_ACC] = *acc;
    host_out[CW_UNDECIDED] = *undecided;
    host_out[CW_PRUNED] = (int)(*prune_key != 0u);
    __threadfence_system();
    // the word the host polls (await_pinned_seq)
    __hip_atomic_store(host_out + CW_SEQ, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the set of the oldest detection in flight, or -1
static int det_oldest(const Ctx* c)
{
    int k = -1;
    for (int i = 0; i < 2; i++)
        if (c->dset[i].job.active && (k < 0 || c->dset[i].job.seq < c->dset[k].job.seq)) k = i;
    return k;
}

// a set with no detection in flight, or -1
static int det_free(const Ctx* c)
{
    for (int i = 0; i < 2; i++)
        if (!c->dset[i].job.active) return i;
    return -1;
}

// The detector as the handle has it set now: what a candidate stage enqueued now computes.  For the smaller eigenvalue k
// and the Harris form are not part of it, so they do not tell two candidate buffers apart either
static Response detector_now(const Ctx* c)
{
    if (c->detector_kind != ICELK_DETECTOR_HARRIS) return Response{};
    return Response{ICELK_DETECTOR_HARRIS, c->detector_k, c->harris_tail};
}

// what a candidate buffer must hold to serve a detection of `slot` as it is now
static Ctx::CandKey eo_want(const Ctx* c, int slot, int use_mask, int block_size, const Response& resp)
{
    return {slot, block_size, use_mask, c->slots[slot].gen, c->mask_gen, resp};
}

static bool eo_holds(const Ctx::EigOut& e, const Ctx::CandKey& want) { return e.valid && e.key == want; }

// a candidate buffer no detection in flight reads: the one that holds what `want` asks for if there is one, else one
// without valid content, else any
static int eo_free(const Ctx* c, const Ctx::CandKey& want)
{
    bool busy[3] = {false, false, false};
    for (const auto& S : c->dset)
        if (S.job.active) busy[S.eo_active] = true;
    int pick = -1;
    for (int i = 0; i < 3; i++) {
        if (busy[i]) continue;
        const Ctx::EigOut& e = c->eo[i];
        if (eo_holds(e, want)) return i;
        if (pick < 0 || (c->eo[pick].valid && !e.valid)) pick = i;
    }
    return pick;
}

// make eo[idx] the candidate buffer of set S: the stages read (and the non-prepared corner kernel writes) it
void activate_eig_out(Ctx* c, Ctx::DetSet& S, int idx)
{
    S.eo_active = idx;
    S.D.cb = c->eo[idx].buf;
}

// Does the strip kernel produce this handle's candidates at block_size (else: the any-blockSize kernels, which serve no
// prepare launch and no fused map)?  The switch is read at every call: it is set and cleared on a live handle.
static bool strip_kernel_serves(const Ctx* c, int block_size, const Response& resp)
{
    return fused_block_size(block_size) && !getenv("ICELK_GENERIC_CORNERS") && !c->corner_variant &&
           !(resp.kind == ICELK_DETECTOR_HARRIS && resp.tail);
}

static int next_counts_seq(Ctx::DetSet& S) { return S.counts_seq = (S.counts_seq + 1) & 0x3fffffff; }

// The counts of set S's detection go to its pinned host words behind whatever is queued on the detection stream, and
// an event of the set marks them.  detect_begin ends with this, so the host round trip of that detection waits for
// ITS kernels only -- not for the min-distance stage of the next detection that may be queued behind them.
static int publish_counts(Ctx* c, Ctx::DetSet& S)
{
    hipLaunchKernelGGL(k_publish_counts, dim3(1), dim3(1), 0, c->det_stream, S.job.cand_count_ptr, S.D.acc_count,
                       S.D.undecided + suppress_launch_count() - 1, S.D.prune_key, S.h_counts, next_counts_seq(S));
    HIPCHK(c, hipEventRecord(S.counts_ev, c->det_stream));
    return ICELK_OK;
}

// the pinned counts (CountsWord) once their sequence word has been seen; n_out and status: of a device-driven tail only
struct Counts {
    int candidates, accepted, undecided, pruned, n_out, status;
};

// the host round trip of a detection: publishes the counts unless the job's last launch did, and waits for them
static int fetch_counts(Ctx* c, Ctx::DetSet& S, Counts* n, bool published = false)
{
    int rc = published ? ICELK_OK : publish_counts(c, S);
    if (rc || (rc = await_pinned_seq(c, S.h_counts + CW_SEQ, S.counts_seq, S.counts_ev))) return rc;
    const int* w = S.h_counts;
    *n = {w[CW_CAND], w[CW_ACC], w[CW_UNDECIDED], w[CW_PRUNED], w[CW_NOUT], w[CW_STATUS]};
    return ICELK_OK;
}

// the mask a detection of a w x h frame reads: none unless use_mask, else the handle's, which must fit the frame
static int pick_mask(Ctx* c, int use_mask, int w, int h, const uint8_t** mask)
{
    *mask = nullptr;
    if (!use_mask) return ICELK_OK;
    if (!c->has_mask) FAIL(c, ICELK_ESTATE, "use_mask set but no mask uploaded");
    if (c->mask_w != w || c->mask_h != h) FAIL(c, ICELK_EARG, "mask size differs from the frame");
    *mask = c->d_mask;
    return ICELK_OK;
}

// Corner candidates of a frame ahead of its detection (strip kernel only; anything else is left to
// detect_begin).  Runs on eig_stream into the spare buffer; detect_begin adopts it when slot, frame
// generation, blockSize, mask and detector (kind, k) still match.
int detect_prepare(Ctx* c, int slot, int use_mask, int block_size)
{
    Range rg("icelk detect_prepare (corner candidates ahead)");
    int rc = check_slot(c, slot, true);
    if (rc) return rc;
    const Response resp = detector_now(c);   // the snapshot: the buffer is keyed by it
    if (!strip_kernel_serves(c, block_size, resp)) return ICELK_OK;
    Slot& s = c->slots[slot];
    const uint8_t* mask = nullptr;
    if ((rc = pick_mask(c, use_mask, s.w, s.h, &mask))) return rc;
    const Ctx::CandKey want = eo_want(c, slot, use_mask, block_size, resp);
    Ctx::EigOut& e = c->eo[eo_free(c, want)];
    if (eo_holds(e, want)) return ICELK_OK;   // already there
    const hipStream_t es = c->eig_stream;
    // level 0 only: `ready` would also wait for a pyramid built ahead, which the detector never reads
    if (int rcw = wait_event(c, es, s.frame_ev)) return rcw;
    HIPCHK(c, hipMemsetAsync(e.buf.max_key, 0, sizeof(unsigned), es));
    DetectScratch T{};   // the corner kernel touches the candidate buffer only
    T.cb = e.buf;
    // the quality level is not known yet: the one of the latest detection begun on this handle is taken (0 at first: every
    // local maximum gets its exact key); detect_begin adopts the result only if its own level is not lower
    const double prep_quality = c->prep_quality;
    {
        ProfScope p(c, K_EIG, es);
        launch_candidates(es, T, s.lv[0], block_size, mask, c->mask_pitch, prep_quality, false, nullptr, 0, resp);
    }
    if ((rc = check_launch(c, "corner candidates (prepared)"))) return rc;
    HIPCHK(c, hipEventRecord(e.done, es));
    HIPCHK(c, hipEventRecord(s.eig_used, es));
    e.buf = T.cb;   // with the geometry of the regions written
    e.valid = true;
    e.key = want;
    e.quality = prep_quality;
    return ICELK_OK;
}

// ---- detect_begin, phase by phase ------------------------------------------------------------------------------------
// Arguments and capacities: the set the detection takes (*k), the mask it reads, the cells of its min-distance grid
static int begin_checks(Ctx* c, int slot, int use_mask, double quality, double min_distance, int block_size, int* k,
                        const uint8_t** mask, size_t* ncell)
{
    if (int rc = check_slot(c, slot, true)) return rc;
    if (!(quality > 0) || min_distance < 0 || block_size <= 0) FAIL(c, ICELK_EARG, "bad detector parameters");
    if (min_eig_lds_bytes(block_size) > 150 * 1024) FAIL(c, ICELK_EARG, "blockSize too large");
    *k = det_free(c);
    if (*k < 0) FAIL(c, ICELK_ESTATE, "two detections are in flight already");
    c->dset_last = *k;
    const Slot& s = c->slots[slot];
    if (int rc = pick_mask(c, use_mask, s.w, s.h, mask)) return rc;
    if (min_distance >= 1) {
        const int cell = (int)lrint(min_distance);
        *ncell = (size_t)((s.w + cell - 1) / cell) * ((s.h + cell - 1) / cell);
        if (*ncell + 1 > c->ncell_cap) FAIL(c, ICELK_ECAP, "cell grid larger than allocated");
    }
    return ICELK_OK;
}

// The job of a detection begun now.  Top-K pruning (k_min_distance.hip) is worthwhile when maxCorners is a real cap: only the
// strongest candidates can be among the first maxCorners accepted ones; how many to keep follows the share that survived
// the minDistance rule in the detection before (update_prune_factor), and relax_on_host verifies that maxCorners came out
static DetectJob new_job(const Ctx* c, const Slot& s, int max_corners, double quality, double min_distance, size_t ncell)
{
    DetectJob J;
    J.w = s.w;
    J.h = s.h;
    J.quality = quality;
    J.min_distance = min_distance;
    J.ncell = ncell;
    J.max_corners = max_corners;
    J.resp = detector_now(c);   // the snapshot: whatever icelk_set_detector does from here on, this detection keeps it
    if (min_distance >= 1 && max_corners > 0 && max_corners <= (1 << 24) && !getenv("ICELK_NO_PRUNE"))
        J.prune_want = (int)std::min(8.0 * max_corners, std::ceil(c->prune_factor * max_corners));
    return J;
}

// Claims a candidate buffer no detection in flight reads for set S.  What detect_prepare left there for this very frame
// is adopted; else the corner kernel fills it here, once a prepare launch that wrote it (for another frame) is through,
// with its maximum starting from zero.  The frame must be in the slot, and the tail of this set's previous detection (it
// sorted this set's accepted keys and reset its counters on the tail stream) through.  That reset normally leaves the
// counters zeroed, off the critical path: they are reset here only the first time or when the cell grid grew.
static int begin_candidates(Ctx* c, Ctx::DetSet& S, int slot, int use_mask, const uint8_t* mask, int block_size)
{
    const DetectJob& J = S.job;
    Slot& s = c->slots[slot];
    const hipStream_t ds = c->det_stream;
    if (int rcw = wait_event(c, ds, s.frame_ev)) return rcw;   // level 0 only (see detect_prepare)
    if (int rcw = wait_event(c, ds, S.tail_done)) return rcw;
    const bool strip = strip_kernel_serves(c, block_size, J.resp);
    const bool need_reset = !S.counters_clean || J.ncell > S.reset_ncell;
    const Ctx::CandKey want = eo_want(c, slot, use_mask, block_size, J.resp);
    const int spare_idx = eo_free(c, want);
    Ctx::EigOut& spare = c->eo[spare_idx];
    const bool prepared = eo_holds(spare, want) && strip && spare.quality <= J.quality;
    c->prep_quality = J.quality;
    spare.valid = false;   // adopted, or overwritten: either way it is not offered again
    S.counters_clean = false;
    activate_eig_out(c, S, spare_idx);
    if (int rcw = wait_event(c, ds, spare.done)) return rcw;
    if (prepared) {
        if (need_reset) launch_detect_reset(ds, S.D, (int)J.ncell, 1);
    } else {
        ProfScope p(c, K_EIG, ds);
        HIPCHK(c, hipMemsetAsync(spare.buf.max_key, 0, sizeof(unsigned), ds));
        if (need_reset) launch_detect_reset(ds, S.D, (int)J.ncell, 1);
        launch_candidates(ds, S.D, s.lv[0], block_size, mask, c->mask_pitch, J.quality, !strip, nullptr, c->corner_variant, J.resp);
        HIPCHK(c, hipEventRecord(s.det_used, ds));   // nothing after this launch reads the frame
    }
    return check_launch(c, "corner candidates");
}

// The min-distance stage (with the device-driven tail's gather behind it), or for minDistance < 1 the flat list
static int begin_min_distance(Ctx* c, Ctx::DetSet& S, bool dev_tail)
{
    DetectJob& J = S.job;
    DetectScratch& D = S.D;
    const hipStream_t ds = c->det_stream;
    if (J.min_distance >= 1) {
        J.cand_count_ptr = D.cell_start + J.ncell;
        ProfScope p(c, K_SUPPRESS, ds);
        launch_min_distance(ds, D, J.w, J.h, J.min_distance, J.quality, J.prune_want, dev_tail);
        const int last = suppress_launch_count() - 1;
        if (dev_tail) launch_tail_gather(ds, D, (int)J.ncell, J.quality, last, J.max_corners, c->max_pts, c->tail_force_status);
    } else {
        J.cand_count_ptr = D.cand_count;
        launch_flatten(ds, D, J.quality);
    }
    return check_launch(c, "min_distance");
}

// The segment set the detection begun now in dset[k] will start its segment in: behind the current one, the staged one
// and the one the other detection in flight has reserved (segments are staged and switched to in the order of _begin)
static int reserve_seg_set(const Ctx* c, int k)
{
    return (c->sb_cur + 1 + (c->seg_staged ? 1 : 0) + (c->dset[k ^ 1].job.active ? 1 : 0)) % kSegSets;
}

// The tail driven by the device-side counts (k_tail.hip), behind the min-distance stage: it writes the segment's tables
// into the set reserved here, once launches that still touch it (a segment closed several switches ago) are through
static int begin_device_tail(Ctx* c, Ctx::DetSet& S, int k)
{
    DetectJob& J = S.job;
    const hipStream_t ds = c->det_stream;
    const int target = reserve_seg_set(c, k);
    Ctx::SegBuf& nb = c->sb[target];
    if (int rcw = wait_event(c, ds, nb.used)) return rcw;
    next_counts_seq(S);
    {
        ProfScope p(c, K_EMIT, ds);
        launch_tail_device(ds, S.D, J.quality, nb.live, nb.alive, nb.tracks, kMaxVert, c->use_order ? nb.order : nullptr,
                           nb.order_border, tail_order_geometry(J.w, J.h, c->border_px), tail_reset_of(S.D, (int)J.ncell),
                           S.h_counts, S.counts_seq);
    }
    if (int rc = check_launch(c, "tail (device-driven)")) return rc;
    HIPCHK(c, hipEventRecord(nb.ready, ds));
    HIPCHK(c, hipEventRecord(S.counts_ev, ds));
    J.dev_tail = true;
    J.seg_set = target;
    return ICELK_OK;
}

// for_segment: the corners start a segment (icelk_seg_detect_begin) -- the tail of the detection is then enqueued here,
// driven by the device; otherwise (icelk_good_features) detect_finish runs the tail after the host round trip
int detect_begin(Ctx* c, int slot, int use_mask, int max_corners, double quality, double min_distance, int block_size,
                 bool for_segment)
{
    Range rg("icelk detect_begin (candidates + min-distance stage)");
    int k = -1;
    const uint8_t* mask = nullptr;
    size_t ncell = 0;
    int rc = begin_checks(c, slot, use_mask, quality, min_distance, block_size, &k, &mask, &ncell);
    if (rc) return rc;
    Ctx::DetSet& S = c->dset[k];
    S.job = new_job(c, c->slots[slot], max_corners, quality, min_distance, ncell);
    const bool dev_tail = for_segment && !c->host_tail && min_distance >= 1;
    if ((rc = begin_candidates(c, S, slot, use_mask, mask, block_size))) return rc;
    if ((rc = begin_min_distance(c, S, dev_tail))) return rc;
    if ((rc = dev_tail ? begin_device_tail(c, S, k) : publish_counts(c, S))) return rc;
    S.job.active = true;
    S.job.seq = ++c->job_seq;
    return ICELK_OK;
}

// ---- detect_finish, phase by phase -----------------------------------------------------------------------------------
static int over_capacity(Ctx* c) { FAIL(c, ICELK_ECAP, "more corners than the output capacity (raise max_pts)"); }

// Next time: candidates per accepted corner as seen now, and half as many again; 8x to begin with, after a detection that
// fell short (its stage was redone) and after one that was not pruned at all
static void update_prune_factor(Ctx* c, const DetectJob& J, int max_corners, const Counts& n, bool fell_short)
{
    if (J.prune_want <= 0 || max_corners <= 0) return;
    const bool start_over = fell_short || !n.pruned || n.accepted <= 0;
    c->prune_factor = start_over ? 8.0 : std::min(8.0, std::max(2.0, 1.5 * (double)n.candidates / n.accepted));
}

static void record_stats(Ctx* c, int candidates, int accepted)
{
    c->last_candidates = candidates;
    c->last_accepted = accepted;
}

// The tail ran on the device already and the host adopts its verdict: done (out->order_written), an error, or -- the
// relaxation not converged, the pruned set short, the bins skewed -- the host's tail on the counts the device published
static int adopt_device_verdict(Ctx* c, Ctx::DetSet& S, const Counts& n, int max_corners, int cap, const Ctx::SegBuf* seg,
                                DetectResult* out)
{
    const DetectJob& J = S.job;
    if (!seg || seg != &c->sb[J.seg_set] || max_corners != J.max_corners)
        FAIL(c, ICELK_ESTATE, "the segment staged is not the one its detection was begun for (set / maxCorners differ)");
    if (n.status == TAIL_OVERFLOW) return over_capacity(c);
    if (n.status != TAIL_OK) return ICELK_OK;
    if (n.n_out > cap) return over_capacity(c);
    update_prune_factor(c, J, max_corners, n, false);
    record_stats(c, n.candidates, n.accepted);
    S.reset_ncell = J.ncell;
    S.counters_clean = true;    // k_tail_order left them zeroed
    c->tails_dev++;
    out->n = n.n_out;
    out->tables_written = out->order_written = true;
    return ICELK_OK;
}

// The min-distance relaxation continued from the host until no candidate is undecided; when the pruned candidate set did
// not yield maxCorners corners, the stage once more on all candidates.  *n: the counts behind all that
static int relax_on_host(Ctx* c, Ctx::DetSet& S, int max_corners, Counts* n)
{
    const DetectJob& J = S.job;
    const hipStream_t ds = c->det_stream;
    auto converge = [&]() -> int {
        for (int guard = 0; n->undecided != 0; guard++) {
            if (guard > 100000) FAIL(c, ICELK_EHIP, "min-distance suppression did not converge");
            continue_min_distance(ds, S.D, J.w, J.h, J.min_distance);
            if (int r = fetch_counts(c, S, n)) return r;
        }
        return ICELK_OK;
    };
    if (int rc = converge()) return rc;
    const bool fell_short = J.prune_want > 0 && n->pruned && (max_corners <= 0 || n->accepted < max_corners);
    if (fell_short) {
        launch_detect_reset(ds, S.D, (int)J.ncell, 0);
        launch_min_distance(ds, S.D, J.w, J.h, J.min_distance, J.quality, 0);
        int rc = check_launch(c, "min_distance (unpruned)");
        if (rc || (rc = fetch_counts(c, S, n)) || (rc = converge())) return rc;
    }
    update_prune_factor(c, J, max_corners, *n, fell_short);
    return ICELK_OK;
}

// The corners by response, on the tail stream: the accepted keys, or for minDistance < 1 every candidate.  *total: how
// many there are (0: nothing was enqueued)
static int sort_corners(Ctx* c, Ctx::DetSet& S, const Counts& n, const unsigned long long** sorted, int* total)
{
    DetectScratch& D = S.D;
    const bool relaxed = S.job.min_distance >= 1;
    *total = relaxed ? n.accepted : n.candidates;
    record_stats(c, n.candidates, *total);
    if (*total == 0) return ICELK_OK;
    sort_keys_desc(c->tail_stream, D, relaxed ? D.acc : D.cand, relaxed ? D.acc_sorted : D.cell_cand, *total);
    *sorted = relaxed ? D.acc_sorted : D.cell_cand;
    return check_launch(c, "sort");
}

// The first n sorted keys become the corner list in c->d_corners.  seg != null: and the tables of the segment they start
// in that set, with the reset of this set's counters, as ONE launch (k_tail), once launches that still touch the set are
// through.  Otherwise the reset follows the list, for this set's next detection, which waits for tail_done
static int tail_or_emit(Ctx* c, Ctx::DetSet& S, const unsigned long long* sorted, int n, Ctx::SegBuf* seg, DetectResult* out)
{
    const DetectJob& J = S.job;
    const hipStream_t ts = c->tail_stream;
    if (int rcw = seg ? wait_event(c, ts, seg->used) : ICELK_OK) return rcw;
    {
        ProfScope p(c, K_EMIT, ts);
        if (seg) launch_tail_fused(ts, sorted, n, c->d_corners, seg->live, seg->alive, seg->tracks, kMaxVert, S.D, (int)J.ncell, 1);
        else launch_emit_corners(ts, sorted, n, J.w, c->d_corners);
    }
    if (int rc = check_launch(c, seg ? "tail" : "emit")) return rc;
    HIPCHK(c, hipEventRecord(c->det_done, ts));
    if (!seg) launch_detect_reset(ts, S.D, (int)J.ncell, 1);
    HIPCHK(c, hipEventRecord(S.tail_done, ts));
    out->tables_written = seg != nullptr;
    S.reset_ncell = J.ncell;
    S.counters_clean = true;
    out->n = n;
    return ICELK_OK;
}

// Finishes the oldest detection in flight.  seg != null (seg_stage): its corners start a segment in that set.  Everything
// behind the host round trip -- sort, corner list, counter reset, the segment's tables -- goes to the tail stream: the
// detection stream may already hold the min-distance stage of the NEXT detection (the other set), and the two have
// nothing in common but d_corners, which only tails touch.
int detect_finish(Ctx* c, int max_corners, int cap, Ctx::SegBuf* seg, DetectResult* out)
{
    Range rg("icelk detect_finish (host round trip, sort, corner list)");
    *out = DetectResult{};
    const int k = det_oldest(c);
    if (k < 0) FAIL(c, ICELK_ESTATE, "no detection in flight");
    c->dset_last = k;
    Ctx::DetSet& S = c->dset[k];
    const DetectJob& J = S.job;
    S.job.active = false;
    out->w = J.w;
    out->h = J.h;
    Counts n{};
    int rc = fetch_counts(c, S, &n, true);   // the one host round trip of a detection
    if (rc) return rc;
    if (J.dev_tail && ((rc = adopt_device_verdict(c, S, n, max_corners, cap, seg, out)) || out->order_written)) return rc;
    c->tails_host++;
    if (J.min_distance >= 1 && (rc = relax_on_host(c, S, max_corners, &n))) return rc;
    const unsigned long long* sorted = nullptr;
    int total = 0;
    if ((rc = sort_corners(c, S, n, &sorted, &total)) || total == 0) return rc;
    const int n_out = max_corners > 0 && total > max_corners ? max_corners : total;
    if (n_out > cap || n_out > c->max_pts) return over_capacity(c);
    return tail_or_emit(c, S, sorted, n_out, seg, out);
}

// for icelk_seg_detect_stage_try: have the counts of the oldest detection in flight arrived?  They are published behind
// its min-distance stage (publish_counts); no wait: a look at the sequence word, and if it is not there at the event
int detect_counts_arrived(Ctx* c, bool* arrived)
{
    *arrived = false;
    const int k = det_oldest(c);
    if (k < 0) FAIL(c, ICELK_ESTATE, "no detection in flight");
    const Ctx::DetSet& S = c->dset[k];
    if (__atomic_load_n(S.h_counts + CW_SEQ, __ATOMIC_ACQUIRE) != S.counts_seq) {
        const hipError_t q = hipEventQuery(S.counts_ev);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();
            return ICELK_OK;
        }
        HIPCHK(c, q);
    }
    *arrived = true;
    return ICELK_OK;
}

}  // namespace icelk

using namespace icelk;

extern "C" {

// ---- detector ----------------------------------------------------------------------------------
int icelk_set_mask(icelk_t* h, const uint8_t* host_mask, int w, int h_, int stride)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (!host_mask) {
        c->has_mask = false;
        c->mask_gen++;
        return ICELK_OK;
    }
    if (w <= 0 || h_ <= 0 || stride < w) FAIL(c, ICELK_EARG, "bad mask");
    if (w > c->max_w || h_ > c->max_h) FAIL(c, ICELK_ECAP, "mask larger than max_w x max_h");
    HIPCHK(c, hipStreamSynchronize(c->det_stream));
    HIPCHK(c, hipStreamSynchronize(c->eig_stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy2DAsync(c->d_mask, c->mask_pitch, host_mask, stride, w, h_, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->has_mask = true;
    c->mask_gen++;
    c->mask_w = w;
    c->mask_h = h_;
    return ICELK_OK;
}

int icelk_set_mask_polygon(icelk_t* h, const double* poly_xy, int n, double crop_left, double crop_top, int w, int h_)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (n < 0 || n > 65536 || (n > 0 && !poly_xy) || w <= 0 || h_ <= 0) FAIL(c, ICELK_EARG, "bad polygon / frame size");
    if (w > c->max_w || h_ > c->max_h) FAIL(c, ICELK_ECAP, "mask larger than max_w x max_h");
    // no detection may be reading the old mask
    HIPCHK(c, hipStreamSynchronize(c->det_stream));
    HIPCHK(c, hipStreamSynchronize(c->eig_stream));
    double* d_poly = nullptr;
    int rc = dmalloc(c, &d_poly, 2 * (size_t)(n > 0 ? n : 1));
    if (rc) return rc;
    hipError_t e = n > 0 ? hipMemcpyAsync(d_poly, poly_xy, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream)
                         : hipSuccess;
    if (e == hipSuccess) {
        launch_polygon_mask(c->stream, d_poly, n, crop_left, crop_top, w, h_, c->d_mask, c->mask_pitch);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(d_poly);
    if (e != hipSuccess) {
        c->err = std::string("polygon mask: ") + hipGetErrorString(e);
        return ICELK_EHIP;
    }
    c->has_mask = true;
    c->mask_gen++;
    c->mask_w = w;
    c->mask_h = h_;
    return ICELK_OK;
}

int icelk_download_mask(icelk_t* h, uint8_t* host_mask, int stride, int* w, int* h_)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->has_mask) FAIL(c, ICELK_ESTATE, "no mask set");
    if (w) *w = c->mask_w;
    if (h_) *h_ = c->mask_h;
    if (!host_mask) return ICELK_OK;
    if (stride < c->mask_w) FAIL(c, ICELK_EARG, "bad host stride");
    HIPCHK(c, hipMemcpy2DAsync(host_mask, stride, c->d_mask, c->mask_pitch, c->mask_w, c->mask_h, hipMemcpyDeviceToHost,
                               c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

// icelk_min_eig_map / icelk_harris_map: the response map of a slot's frame, by the kernel a detection would take
static int response_map(Ctx* c, int slot, int block_size, const Response& resp, float* host_out, int stride_elems)
{
    HIPCHK(c, hipSetDevice(c->device));
    int rc = check_slot(c, slot, true);
    if (rc) return rc;
    Slot& s = c->slots[slot];
    if (!host_out || stride_elems < s.w || block_size <= 0) FAIL(c, ICELK_EARG, "bad argument");
    if (min_eig_lds_bytes(block_size) > 150 * 1024) FAIL(c, ICELK_EARG, "blockSize too large");
    rc = wait_slot(c, slot);
    if (rc) return rc;
    const int k = det_free(c);     // scratch of a set no detection in flight owns
    if (k < 0) FAIL(c, ICELK_ESTATE, "two detections are in flight");
    c->dset_last = k;
    Ctx::DetSet& S = c->dset[k];
    HIPCHK(c, hipStreamSynchronize(c->stream));       // the frame is in place
    HIPCHK(c, hipStreamSynchronize(c->det_stream));   // the detector scratch is free
    HIPCHK(c, hipStreamSynchronize(c->tail_stream));
    {
        ProfScope p(c, K_EIG);
        launch_detect_reset(c->stream, S.D, 0, 3);
        S.counters_clean = false;
        if (strip_kernel_serves(c, block_size, resp)) {
            launch_candidates(c->stream, S.D, s.lv[0], block_size, nullptr, 0, 1.0, false, S.D.eig, 0, resp);
        } else {
            launch_min_eig(c->stream, s.lv[0], block_size, S.D.eig, nullptr, 0, S.D.cb.max_key, c->corner_variant, resp);
        }
    }
    rc = check_launch(c, "min_eig");
    if (rc) return rc;
    HIPCHK(c, hipMemcpy2DAsync(host_out, sizeof(float) * stride_elems, S.D.eig, sizeof(float) * s.w, sizeof(float) * s.w,
                               s.h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

int icelk_min_eig_map(icelk_t* h, int slot, int block_size, float* host_out, int stride_elems)
{
    if (!h) return ICELK_EARG;
    return response_map(C(h), slot, block_size, Response{}, host_out, stride_elems);
}

int icelk_harris_map(icelk_t* h, int slot, int block_size, double k, float* host_out, int stride_elems)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (!std::isfinite(k)) FAIL(c, ICELK_EARG, "k is not finite");
    return response_map(c, slot, block_size, Response{ICELK_DETECTOR_HARRIS, k, c->harris_tail}, host_out, stride_elems);
}

int icelk_set_detector(icelk_t* h, int kind, double k)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (kind != ICELK_DETECTOR_MIN_EIG && kind != ICELK_DETECTOR_HARRIS) FAIL(c, ICELK_EARG, "unknown detector kind");
    if (!std::isfinite(k)) FAIL(c, ICELK_EARG, "k is not finite");
    // nothing else: detections in flight carry their own copy (DetectJob::resp), prepared candidates theirs (CandKey::resp)
    c->detector_kind = kind;
    c->detector_k = k;
    return ICELK_OK;
}

int icelk_get_detector(icelk_t* h, int* kind, double* k)
{
    if (!h) return ICELK_EARG;
    const Ctx* c = C(h);
    if (kind) *kind = c->detector_kind;
    if (k) *k = c->detector_k;
    return ICELK_OK;
}

int icelk_good_features(icelk_t* h, int slot, int use_mask, int max_corners, double quality_level, double min_distance,
                        int block_size, float* out_xy, int cap, int* out_n)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (!out_n || cap < 0 || (cap > 0 && !out_xy)) FAIL(c, ICELK_EARG, "bad output buffer");
    // begin + finish in one go: the detection finished must be the one begun here
    if (det_oldest(c) >= 0) FAIL(c, ICELK_ESTATE, "a detection is in flight (icelk_seg_detect_begin without _stage / _finish)");
    DetectResult r;
    int rc = detect_begin(c, slot, use_mask, max_corners, quality_level, min_distance, block_size, false);
    if (rc || (rc = detect_finish(c, max_corners, cap, nullptr, &r))) return rc;
    if (r.n > 0) {
        HIPCHK(c, hipMemcpyAsync(out_xy, c->d_corners, sizeof(float) * 2 * r.n, hipMemcpyDeviceToHost, c->tail_stream));
        HIPCHK(c, hipStreamSynchronize(c->tail_stream));
    }
    *out_n = r.n;
    return ICELK_OK;
}

int icelk_detect_stats(icelk_t* h, int* n_candidates, int* n_accepted)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    if (n_candidates) *n_candidates = c->last_candidates;
    if (n_accepted) *n_accepted = c->last_accepted;
    return ICELK_OK;
}

int icelk_detect_fast_stats(icelk_t* h, int slot_w, int slot_h, long long* out)
{
    if (!h || !out) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    const CandBuf& e = c->eo[c->dset[c->dset_last].eo_active].buf;
    if (!e.acand) FAIL(c, ICELK_EARG, "the two-pass detector was not enabled when this handle was created (ICELK_TWO_PASS_CORNERS)");
    const size_t nt = fast_tiles(slot_w, slot_h);
    std::vector<int> cnt(nt), mx(nt);
    unsigned fk[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpy(cnt.data(), e.acount, nt * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(mx.data(), e.amaxn, nt * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(fk, e.fmax_key, sizeof fk, hipMemcpyDeviceToHost));
    long long listed = 0, whole = 0, maxc = 0, maxover = 0, biggest = 0;
    for (size_t i = 0; i < nt; i++) {
        if (cnt[i] > 256) whole++;
        else listed += cnt[i];
        if (cnt[i] > biggest) biggest = cnt[i];
        if (mx[i] > 16) maxover++;
        else maxc += mx[i];
    }
    out[0] = (long long)nt; out[1] = listed; out[2] = whole; out[3] = (long long)fk[1]; out[4] = maxc; out[5] = maxover;
    out[6] = biggest; out[7] = (long long)fk[2];
    return ICELK_OK;
}

int icelk_detect_max_key(icelk_t* h, unsigned* out_key)
{
    if (!h || !out_key) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    const CandBuf& e = c->eo[c->dset[c->dset_last].eo_active].buf;
    HIPCHK(c, hipMemcpy(out_key, e.max_key, sizeof(unsigned), hipMemcpyDeviceToHost));
    return ICELK_OK;
}

}  // extern "C"
