// abi_detect.hip -- corner detector: candidate buffers, detector sets, the counts round trip, prepare / begin /
// finish, mask, icelk_min_eig_map, icelk_good_features, statistics.
#include "icelk_ctx.h"

namespace icelk {

// ---- candidate buffers and detector sets: allocation and release ----------------------------------------------------
int alloc_eig_out(Ctx* c, Ctx::EigOut& e, int cand_cap)
{
    const int w = c->max_w, h = c->max_h;
    int rc;
    if ((rc = dmalloc(c, &e.max_key, 1)) || (rc = dmalloc(c, &e.raw, (size_t)cand_cap)) ||
        (rc = dmalloc(c, &e.blk_count, candidate_blocks(w, h) * 4)))
        return rc;
    // the two-pass detector's scratch (~20 MB per buffer at 12 MP) only on a handle created with its switch set: a
    // handle without it runs the strip kernel whatever the switch says later (launch_candidates looks at D.acand)
    if (getenv("ICELK_TWO_PASS_CORNERS") &&
        ((rc = dmalloc(c, &e.acand, fast_cand_entries(w, h))) || (rc = dmalloc(c, &e.acount, fast_tiles(w, h))) ||
         (rc = dmalloc(c, &e.amaxc, fast_max_entries(w, h))) || (rc = dmalloc(c, &e.amaxn, fast_tiles(w, h))) ||
         (rc = dmalloc(c, &e.aemax, fast_tiles(w, h))) || (rc = dmalloc(c, &e.fmax_key, 8)) ||
         (rc = dmalloc(c, &e.aties, fast_cand_entries(w, h) + fast_tiles(w, h)))))
        return rc;
    if (hipEventCreateWithFlags(&e.done, hipEventDisableTiming) != hipSuccess) FAIL(c, ICELK_EHIP, "hipEventCreate failed");
    return ICELK_OK;
}

void free_eig_out(Ctx::EigOut& e)
{
    void* p[] = {e.raw, e.blk_count, e.max_key, e.acand, e.acount, e.amaxc, e.amaxn, e.aemax, e.fmax_key, e.aties};
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
    if (hipHostMalloc(reinterpret_cast<void**>(&S.h_counts), 64, hipHostMallocMapped) != hipSuccess ||
        hipEventCreateWithFlags(&S.counts_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&S.tail_done, hipEventDisableTiming) != hipSuccess)
        FAIL(c, ICELK_EHIP, "hipHostMalloc failed");
    memset(S.h_counts, 0, 64);
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
// counts, sorts the accepted corners and leaves the first *n_out of them in c->d_corners (device), in
// response order.
constexpr int kCountsSeq = 8;   // word of the pinned counts that carries the sequence number of the publication
__global__ void k_publish_counts(const int* __restrict__ cand, const int* __restrict__ acc,
                                 const int* __restrict__ undecided, const unsigned* __restrict__ prune_key,
                                 int* __restrict__ host_out, int seq)
{
    host_out[0] = *cand;
    host_out[1] = *acc;
    host_out[2] = *undecided;
    host_out[3] = (int)(*prune_key != 0u);
    __threadfence_system();
    // the host polls this word (fetch_counts): it learns of the counts when they land in its memory, not when the
    // runtime has processed the completion signal of an event behind this kernel and woken the waiting thread
    __hip_atomic_store(host_out + kCountsSeq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
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

// what a candidate buffer must hold to serve a detection of `slot` as it is now
static Ctx::EigOut eo_want(const Ctx* c, int slot, int use_mask, int block_size)
{
    Ctx::EigOut want;
    want.slot = slot;
    want.gen = c->slots[slot].gen;
    want.block_size = block_size;
    want.use_mask = use_mask;
    want.mask_gen = c->mask_gen;
    return want;
}

// does e hold the prepared candidates `want` asks for (slot, frame generation, blockSize, mask, mask generation)?
static bool eo_holds(const Ctx::EigOut& e, const Ctx::EigOut& want)
{
    return e.valid && e.slot == want.slot && e.gen == want.gen && e.block_size == want.block_size &&
           e.use_mask == want.use_mask && e.mask_gen == want.mask_gen;
}

// a candidate buffer no detection in flight reads: the one that holds what `want` asks for if there is one, else one
// without valid content, else any
static int eo_free(const Ctx* c, const Ctx::EigOut& want)
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

// point a detector scratch at candidate buffer e: the stages read (and the non-prepared corner kernel writes) e
static void point_at_eig_out(DetectScratch& D, const Ctx::EigOut& e)
{
    D.raw = e.raw;
    D.blk_count = e.blk_count;
    D.max_key = e.max_key;
    D.acand = e.acand;
    D.acount = e.acount;
    D.amaxc = e.amaxc;
    D.amaxn = e.amaxn;
    D.aemax = e.aemax;
    D.fmax_key = e.fmax_key;
    D.aties = e.aties;
    D.src_nblk = e.nblk;
    D.src_region = e.region;
}

// make eo[idx] the candidate buffer of set S
void activate_eig_out(Ctx* c, Ctx::DetSet& S, int idx)
{
    S.eo_active = idx;
    point_at_eig_out(S.D, c->eo[idx]);
}

// The counts of set S's detection go to its pinned host words behind whatever is queued on the detection stream, and
// an event of the set marks them.  detect_begin ends with this, so the host round trip of that detection waits for
// ITS kernels only -- not for the min-distance stage of the next detection that may be queued behind them.
static int publish_counts(Ctx* c, Ctx::DetSet& S)
{
    S.counts_seq = (S.counts_seq + 1) & 0x3fffffff;
    hipLaunchKernelGGL(k_publish_counts, dim3(1), dim3(1), 0, c->det_stream, S.job.cand_count_ptr, S.D.acc_count,
                       S.D.undecided + suppress_launch_count() - 1, S.D.prune_key, S.h_counts, S.counts_seq);
    HIPCHK(c, hipEventRecord(S.counts_ev, c->det_stream));
    return ICELK_OK;
}

// have the counts published last arrived?  (the sequence word, no runtime call)
static inline bool counts_here(const int* h_counts, int seq)
{
    return __atomic_load_n(h_counts + kCountsSeq, __ATOMIC_ACQUIRE) == seq;
}

// Waits for the counts by polling the pinned sequence word; the event is looked at now and then, so that a failed
// kernel ends the wait with its error instead of hanging it.
static int fetch_counts(Ctx* c, Ctx::DetSet& S, bool published = false)
{
    if (!published) {
        int rc = publish_counts(c, S);
        if (rc) return rc;
    }
    for (unsigned it = 1;; it++) {
        if (counts_here(S.h_counts, S.counts_seq)) return ICELK_OK;
        if ((it & 4095u) == 0) {
            const hipError_t q = hipEventQuery(S.counts_ev);
            if (q == hipSuccess) break;             // complete: the synchronize below returns at once
            if (q != hipErrorNotReady) HIPCHK(c, q);
            (void)hipGetLastError();
        }
        __builtin_ia32_pause();
    }
    HIPCHK(c, hipEventSynchronize(S.counts_ev));
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

// Corner candidates of a frame ahead of its detection (fused kernel only; anything else is left to
// detect_begin).  Runs on eig_stream into the spare buffer; detect_begin adopts it when slot, frame
// generation, blockSize and mask still match.
int detect_prepare(Ctx* c, int slot, int use_mask, int block_size)
{
    Range rg("icelk detect_prepare (corner candidates ahead)");
    int rc = check_slot(c, slot, true);
    if (rc) return rc;
    if (!fused_block_size(block_size) || getenv("ICELK_GENERIC_CORNERS") || c->corner_variant) return ICELK_OK;
    Slot& s = c->slots[slot];
    const uint8_t* mask = nullptr;
    if ((rc = pick_mask(c, use_mask, s.w, s.h, &mask))) return rc;
    const Ctx::EigOut want = eo_want(c, slot, use_mask, block_size);
    Ctx::EigOut& e = c->eo[eo_free(c, want)];
    if (eo_holds(e, want)) return ICELK_OK;   // already there
    const hipStream_t es = c->eig_stream;
    // level 0 only: `ready` would also wait for a pyramid built ahead, which the detector never reads
    if (int rcw = wait_event(c, es, s.frame_ev)) return rcw;
    HIPCHK(c, hipMemsetAsync(e.max_key, 0, sizeof(unsigned), es));
    DetectScratch T{};   // the corner kernel touches the candidate buffer only
    point_at_eig_out(T, e);
    // the quality level is not known yet: the one of the latest detection begun on this handle is taken (0 at first: every
    // local maximum gets its exact key); detect_begin adopts the result only if its own level is not lower
    const double prep_quality = c->prep_quality;
    {
        ProfScope p(c, K_EIG, es);
        launch_candidates(es, T, s.lv[0], block_size, mask, c->mask_pitch, prep_quality, false, nullptr);
    }
    rc = check_launch(c, "corner candidates (prepared)");
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(e.done, es));
    HIPCHK(c, hipEventRecord(s.eig_used, es));
    e.nblk = T.src_nblk;
    e.region = T.src_region;
    e.valid = true;
    e.slot = slot;
    e.gen = s.gen;
    e.block_size = block_size;
    e.use_mask = use_mask;
    e.mask_gen = c->mask_gen;
    e.quality = prep_quality;
    return ICELK_OK;
}

// for_segment: the corners start a segment (icelk_seg_detect_begin) -- the tail of the detection is then enqueued here, behind
// the min-distance stage, driven by the device-side counts (k_tail.hip), and writes the segment's tables into the set it
// reserves; otherwise (icelk_good_features) detect_finish runs the tail after the host round trip
int detect_begin(Ctx* c, int slot, int use_mask, int max_corners, double quality, double min_distance, int block_size,
                 bool for_segment)
{
    Range rg("icelk detect_begin (candidates + min-distance stage)");
    int rc = check_slot(c, slot, true);
    if (rc) return rc;
    if (!(quality > 0) || min_distance < 0 || block_size <= 0) FAIL(c, ICELK_EARG, "bad detector parameters");
    if (min_eig_lds_bytes(block_size) > 150 * 1024) FAIL(c, ICELK_EARG, "blockSize too large");
    const int k = det_free(c);
    if (k < 0) FAIL(c, ICELK_ESTATE, "two detections are in flight already");
    c->dset_last = k;
    Ctx::DetSet& S = c->dset[k];
    Slot& s = c->slots[slot];
    const hipStream_t ds = c->det_stream;
    const int w = s.w, h = s.h;
    const uint8_t* mask = nullptr;
    if ((rc = pick_mask(c, use_mask, w, h, &mask))) return rc;
    DetectScratch& D = S.D;
    size_t ncell = 0;
    if (min_distance >= 1) {
        const int cell = (int)lrint(min_distance);
        ncell = (size_t)((w + cell - 1) / cell) * ((h + cell - 1) / cell);
        if (ncell + 1 > c->ncell_cap) FAIL(c, ICELK_ECAP, "cell grid larger than allocated");
    }
    // the frame must be in the slot (ingest on the compute or the copy stream), and the tail of this set's previous detection (it sorted this set's accepted keys and
    // reset its counters on the tail stream) must be through
    if (int rcw = wait_event(c, ds, s.frame_ev)) return rcw;   // level 0 only (see detect_prepare)
    if (int rcw = wait_event(c, ds, S.tail_done)) return rcw;
    const bool generic = getenv("ICELK_GENERIC_CORNERS") != nullptr || c->corner_variant != 0;
    // counters are normally left zeroed by the previous detection (the reset runs after its last kernel,
    // off the critical path); reset here only the first time or when the cell grid grew
    const bool need_reset = !S.counters_clean || ncell > S.reset_ncell;
    const Ctx::EigOut want = eo_want(c, slot, use_mask, block_size);
    const int spare_idx = eo_free(c, want);
    Ctx::EigOut& spare = c->eo[spare_idx];
    const bool prepared = eo_holds(spare, want) && !generic && spare.quality <= quality;
    c->prep_quality = quality;
    spare.valid = false;   // adopted below, or overwritten: either way it is not offered again
    if (prepared) {
        if (need_reset) launch_detect_reset(ds, D, (int)ncell, 1);
        activate_eig_out(c, S, spare_idx);
        if (int rcw = wait_event(c, ds, spare.done)) return rcw;
    } else {
        ProfScope p(c, K_EIG, ds);
        // this detection's candidates go into a buffer no detection in flight reads; a prepare launch that wrote it
        // (for another frame) must be through, and its maximum starts from zero
        activate_eig_out(c, S, spare_idx);
        if (int rcw = wait_event(c, ds, spare.done)) return rcw;
        HIPCHK(c, hipMemsetAsync(spare.max_key, 0, sizeof(unsigned), ds));
        if (need_reset) launch_detect_reset(ds, D, (int)ncell, 1);
        launch_candidates(ds, D, s.lv[0], block_size, mask, c->mask_pitch, quality, generic, nullptr, c->corner_variant);
        HIPCHK(c, hipEventRecord(s.det_used, ds));   // nothing after this launch reads the frame
    }
    S.counters_clean = false;
    rc = check_launch(c, "corner candidates");
    if (rc) return rc;
    DetectJob& J = S.job;
    J.w = w;
    J.h = h;
    J.quality = quality;
    J.min_distance = min_distance;
    J.ncell = ncell;
    // top-K pruning (k_corners.hip): worthwhile when maxCorners is a real cap.  Only the strongest candidates can be among
    // the first maxCorners accepted ones; how many to keep follows the share that survived the minDistance rule in the
    // detection before (with half as many again; 8x to begin with and after a shortfall), and detect_finish verifies
    // that maxCorners corners came out -- else the stage runs once more on all candidates
    J.prune_want = 0;
    if (min_distance >= 1 && max_corners > 0 && max_corners <= (1 << 24) && !getenv("ICELK_NO_PRUNE"))
        J.prune_want = (int)std::min(8.0 * max_corners, std::ceil(c->prune_factor * max_corners));
    J.dev_tail = false;
    J.seg_set = -1;
    J.max_corners = max_corners;
    const bool dev_tail = for_segment && !c->host_tail && min_distance >= 1;
    if (min_distance >= 1) {
        J.cand_count_ptr = D.cell_start + ncell;
        ProfScope p(c, K_SUPPRESS, ds);
        launch_min_distance(ds, D, w, h, min_distance, quality, J.prune_want, dev_tail);
        if (dev_tail)
            launch_tail_gather(ds, D, (int)ncell, quality, suppress_launch_count() - 1, max_corners, c->max_pts, c->tail_force_status);
    } else {
        J.cand_count_ptr = D.cand_count;
        launch_flatten(ds, D, quality);
    }
    rc = check_launch(c, "min_distance");
    if (rc) return rc;
    if (dev_tail) {
        // the set the new segment goes into: behind the current one, the staged one and the one the other detection in
        // flight has reserved (segments are staged and switched to in the order their detections were begun)
        const Ctx::DetSet& other = c->dset[k ^ 1];
        const int ahead = (c->seg_staged ? 1 : 0) + (other.job.active ? 1 : 0);
        const int target = (c->sb_cur + 1 + ahead) % kSegSets;
        Ctx::SegBuf& nb = c->sb[target];
        // launches that still touch that set (a segment closed several switches ago) must be through
        if (int rcw = wait_event(c, ds, nb.used)) return rcw;
        S.counts_seq = (S.counts_seq + 1) & 0x3fffffff;
        {
            ProfScope p(c, K_EMIT, ds);
            launch_tail_device(ds, D, quality, nb.live, nb.alive, nb.tracks, kMaxVert, c->use_order ? nb.order : nullptr,
                               nb.order_border, tail_order_geometry(w, h, c->border_px), tail_reset_of(D, (int)ncell),
                               S.h_counts, kCountsSeq, S.counts_seq);
        }
        rc = check_launch(c, "tail (device-driven)");
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(nb.ready, ds));
        HIPCHK(c, hipEventRecord(S.counts_ev, ds));
        J.dev_tail = true;
        J.seg_set = target;
    } else {
        rc = publish_counts(c, S);
        if (rc) return rc;
    }
    J.active = true;
    J.seq = ++c->job_seq;
    return ICELK_OK;
}

// seg != null (seg_stage): the corners start a segment in that set -- corner list, the segment's tables and the counter
// reset go out as ONE launch (k_tail) instead of three; *seg_done tells seg_stage that the tables are written
// *dev_done: the device-driven tail has written everything (tables AND launch order): nothing is left to enqueue
// *finished: the job of the detection finished here (the oldest in flight)
int detect_finish(Ctx* c, int max_corners, int cap, int* n_out, Ctx::SegBuf* seg, bool* seg_done, bool* dev_done,
                  DetectJob* finished)
{
    Range rg("icelk detect_finish (host round trip, sort, corner list)");
    if (seg_done) *seg_done = false;
    if (dev_done) *dev_done = false;
    const int k = det_oldest(c);
    if (k < 0) FAIL(c, ICELK_ESTATE, "no detection in flight");
    c->dset_last = k;
    Ctx::DetSet& S = c->dset[k];
    DetectJob& J = S.job;
    J.active = false;
    if (finished) *finished = J;
    *n_out = 0;
    const hipStream_t ds = c->det_stream;
    // Everything behind the host round trip -- sort, corner list, the reset of this set's counters, and in seg_stage the
    // new segment's tables -- goes to the tail stream: the detection stream may already hold the min-distance stage of
    // the NEXT detection (the other set), and the two have nothing in common but d_corners, which only tails touch.
    const hipStream_t ts = c->tail_stream;
    DetectScratch& D = S.D;
    int rc = fetch_counts(c, S, true);   // the one host round trip of a detection: {candidates, accepted, undecided}
    if (rc) return rc;
    if (J.dev_tail) {
        // the tail ran on the device already; the host adopts its verdict
        const int status = S.h_counts[5];
        if (!seg || seg != &c->sb[J.seg_set] || max_corners != J.max_corners)
            FAIL(c, ICELK_ESTATE, "the segment staged is not the one its detection was begun for (set / maxCorners differ)");
        if (status == TAIL_OVERFLOW) FAIL(c, ICELK_ECAP, "more corners than the output capacity (raise max_pts)");
        if (status == TAIL_OK) {
            const int total = S.h_counts[1], n = S.h_counts[4];
            if (n > cap) FAIL(c, ICELK_ECAP, "more corners than the output capacity (raise max_pts)");
            if (J.prune_want > 0 && max_corners > 0)
                c->prune_factor = !S.h_counts[3] || total <= 0 ? 8.0 : std::min(8.0, std::max(2.0, 1.5 * (double)S.h_counts[0] / total));
            c->last_candidates = S.h_counts[0];
            c->last_accepted = total;
            S.reset_ncell = J.ncell;
            S.counters_clean = true;    // k_tail_order left them zeroed
            c->tails_dev++;
            *n_out = n;
            if (seg_done) *seg_done = true;
            if (dev_done) *dev_done = true;
            return ICELK_OK;
        }
        // not converged / pruned set fell short: the host's tail below, on the counts the device published
    }
    c->tails_host++;
    const unsigned long long* sorted = nullptr;
    int total = 0;
    if (J.min_distance >= 1) {
        auto converge = [&]() -> int {
            for (int guard = 0; S.h_counts[2] != 0; guard++) {
                if (guard > 100000) FAIL(c, ICELK_EHIP, "min-distance suppression did not converge");
                continue_min_distance(ds, D, J.w, J.h, J.min_distance);
                int r = fetch_counts(c, S);
                if (r) return r;
            }
            return ICELK_OK;
        };
        if ((rc = converge())) return rc;
        bool redone = false;
        if (J.prune_want > 0 && S.h_counts[3] && (max_corners <= 0 || S.h_counts[1] < max_corners)) {
            // the pruned candidate set did not yield maxCorners corners: redo the stage on all candidates
            redone = true;
            launch_detect_reset(ds, D, (int)J.ncell, 0);
            launch_min_distance(ds, D, J.w, J.h, J.min_distance, J.quality, 0);
            if ((rc = check_launch(c, "min_distance (unpruned)"))) return rc;
            if ((rc = fetch_counts(c, S))) return rc;
            if ((rc = converge())) return rc;
        }
        total = S.h_counts[1];
        if (J.prune_want > 0 && max_corners > 0) {
            // next time: candidates per accepted corner as seen now, and half as many again; a detection that fell short
            // (it was redone above) or was not pruned at all starts over at 8x
            const bool fell_short = !S.h_counts[3] || redone;
            c->prune_factor = fell_short || total <= 0 ? 8.0 : std::min(8.0, std::max(2.0, 1.5 * (double)S.h_counts[0] / total));
        }
        c->last_candidates = S.h_counts[0];
        c->last_accepted = total;
        if (total == 0) return ICELK_OK;
        sort_keys_desc(ts, D, D.acc, D.acc_sorted, total);
        sorted = D.acc_sorted;
    } else {
        total = S.h_counts[0];
        c->last_candidates = total;
        c->last_accepted = total;
        if (total == 0) return ICELK_OK;
        sort_keys_desc(ts, D, D.cand, D.cell_cand, total);
        sorted = D.cell_cand;
    }
    rc = check_launch(c, "sort");
    if (rc) return rc;
    int n = total;
    if (max_corners > 0 && n > max_corners) n = max_corners;
    if (n > cap || n > c->max_pts) FAIL(c, ICELK_ECAP, "more corners than the output capacity (raise max_pts)");
    if (seg) {
        // launches that still touch the segment set (a segment closed two switches ago) must be through
        if (int rcw = wait_event(c, ts, seg->used)) return rcw;
        {
            ProfScope p(c, K_EMIT, ts);
            launch_tail_fused(ts, sorted, n, c->d_corners, seg->live, seg->alive, seg->tracks, kMaxVert, D, (int)J.ncell, 1);
        }
        rc = check_launch(c, "tail");
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(c->det_done, ts));
        HIPCHK(c, hipEventRecord(S.tail_done, ts));
        *seg_done = true;
    } else {
        {
            ProfScope p(c, K_EMIT, ts);
            launch_emit_corners(ts, sorted, n, J.w, c->d_corners);
        }
        rc = check_launch(c, "emit");
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(c->det_done, ts));
        launch_detect_reset(ts, D, (int)J.ncell, 1);   // for this set's next detection, which waits for tail_done
        HIPCHK(c, hipEventRecord(S.tail_done, ts));
    }
    S.reset_ncell = J.ncell;
    S.counters_clean = true;
    *n_out = n;
    return ICELK_OK;
}

static int detect_core(Ctx* c, int slot, int use_mask, int max_corners, double quality, double min_distance,
                       int block_size, int cap, int* n_out)
{
    *n_out = 0;
    // begin + finish in one go: the detection finished must be the one begun here
    if (det_oldest(c) >= 0) FAIL(c, ICELK_ESTATE, "a detection is in flight (icelk_seg_detect_begin without _stage / _finish)");
    int rc = detect_begin(c, slot, use_mask, max_corners, quality, min_distance, block_size, false);
    if (rc) return rc;
    return detect_finish(c, max_corners, cap, n_out);
}

// for icelk_seg_detect_stage_try: have the counts of the oldest detection in flight arrived?  They are published behind
// its min-distance stage (publish_counts); no wait
int detect_counts_arrived(Ctx* c, bool* arrived)
{
    *arrived = false;
    const int k = det_oldest(c);
    if (k < 0) FAIL(c, ICELK_ESTATE, "no detection in flight");
    if (!counts_here(c->dset[k].h_counts, c->dset[k].counts_seq)) {
        const hipError_t q = hipEventQuery(c->dset[k].counts_ev);
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

int icelk_min_eig_map(icelk_t* h, int slot, int block_size, float* host_out, int stride_elems)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
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
        if (fused_block_size(block_size) && !getenv("ICELK_GENERIC_CORNERS") && !c->corner_variant) {
            launch_candidates(c->stream, S.D, s.lv[0], block_size, nullptr, 0, 1.0, false, S.D.eig);
        } else {
            launch_min_eig(c->stream, s.lv[0], block_size, S.D.eig, nullptr, 0, S.D.max_key, c->corner_variant);
        }
    }
    rc = check_launch(c, "min_eig");
    if (rc) return rc;
    HIPCHK(c, hipMemcpy2DAsync(host_out, sizeof(float) * stride_elems, S.D.eig, sizeof(float) * s.w, sizeof(float) * s.w,
                               s.h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ICELK_OK;
}

int icelk_good_features(icelk_t* h, int slot, int use_mask, int max_corners, double quality_level, double min_distance,
                        int block_size, float* out_xy, int cap, int* out_n)
{
    if (!h) return ICELK_EARG;
    Ctx* c = C(h);
    HIPCHK(c, hipSetDevice(c->device));
    if (!out_n || cap < 0 || (cap > 0 && !out_xy)) FAIL(c, ICELK_EARG, "bad output buffer");
    int n = 0;
    int rc = detect_core(c, slot, use_mask, max_corners, quality_level, min_distance, block_size, cap, &n);
    if (rc) return rc;
    if (n > 0) {
        HIPCHK(c, hipMemcpyAsync(out_xy, c->d_corners, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, c->tail_stream));
        HIPCHK(c, hipStreamSynchronize(c->tail_stream));
    }
    *out_n = n;
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
    const Ctx::EigOut& e = c->eo[c->dset[c->dset_last].eo_active];
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
    const Ctx::EigOut& e = c->eo[c->dset[c->dset_last].eo_active];
    HIPCHK(c, hipMemcpy(out_key, e.max_key, sizeof(unsigned), hipMemcpyDeviceToHost));
    return ICELK_OK;
}

}  // extern "C"
