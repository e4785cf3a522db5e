// icelk_ctx.h -- what the host-side translation units (abi_*.hip) share: the handle, the error macros, the
// profiling / tracing scopes and the few helpers that cross a stage boundary.  The contract with the kernel files
// is icelk_internal.h.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <mutex>

#include "icelk_internal.h"

namespace icelk {

constexpr int kSegSets = 6;
constexpr int kLaunchEvents = 32;
constexpr int kMaxVert = 17;  // vertices per track kept on the device (track_len <= 16; reference uses 2)

struct DetectJob {
    bool active = false;
    int w = 0, h = 0;
    double quality = 0, min_distance = 0;
    size_t ncell = 0;
    const int* cand_count_ptr = nullptr;
    int prune_want = 0;   // > 0: top-K pruning is on for this job
    Response resp;        // the detector as it was set when the candidate stage was enqueued (icelk_set_detector)
    unsigned long long seq = 0;   // order of icelk_seg_detect_begin calls: the oldest job in flight is finished first
    // device-driven tail (k_tail.hip): enqueued behind the min-distance stage by detect_begin; the corners of this detection
    // start a segment in set `seg_set`, cut at max_corners
    bool dev_tail = false;
    int seg_set = -1;
    int max_corners = 0;
};

struct Ctx {
    // ---- abi_handle.hip: the handle itself, its switches, diagnostics and the profiling table
    int device = 0;
    int max_w = 0, max_h = 0, n_slots = 0, max_pts = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::string err;
    int side_pick[4] = {-1, -1, -1, -1};   // which of the probed candidate streams became detection / candidates / pyramid / tail
    double probe_limit = 0, probe_quickest = 0;
    int fb_dist_form = ICELK_FB_HYPOT;     // icelk_set_fb_distance
    int lk_sum_mode = 0;                   // icelk_set_variant "lk_sums"
    int lk_wide_sums = 0;                  // icelk_set_variant "lk_wide_sums"
    int corner_variant = 0;                // icelk_set_variant "sobel_fma" (bits 0-1) | "eig_fma" (bit 2)
    int harris_tail = 0;                   // icelk_set_variant "harris_tail"
    int detector_kind = ICELK_DETECTOR_MIN_EIG;   // icelk_set_detector: read when a candidate stage is enqueued
    double detector_k = 0.04;
    int lk_kernel_flags = 0;               // icelk_set_lk_kernel: ICELK_FLAG_GENERIC_KERNEL / _ONE_PER_WAVE or 0
    // diagnostics: ICELK_LK_STAMPS=<file> records entry / exit time and placement of every workgroup of the LAST
    // segment tracker launch and writes them to the file when the handle is destroyed (tools/lk_stamps.py reads it)
    uint32_t* d_iters = nullptr;   // per-feature iteration counts of the latest tracker launch (while profiling is on)
    int iters_n = 0;
    unsigned long long* d_stamps = nullptr;
    size_t stamps_cap = 0;     // workgroups
    std::string stamps_path;
    // profiling
    bool prof = false;
    bool prof_tracker_only = false;   // icelk_prof_enable(h, 2): every other kernel goes untimed (no event records on its stream)
    std::vector<ProfEvt> evts, evt_pool;
    int prof_launches[K_COUNT_] = {0};
    double prof_ms[K_COUNT_] = {0};

    // ---- abi_frames.hip: frame slots, pyramids, ingest (the JPEG jobs: abi_jpeg_ingest.hip and the files behind it)
    std::vector<Slot> slots;
    // the streams of icelk_upload_gray_async, created at the first such upload.  Uploads alternate between two streams:
    // between two copies of ONE stream the runtime spends ~50 us (completion signal of the first, dependency of the
    // second: 220 us copies came out 270 us apart), which a copy queued on the other stream fills.  HIGH priority since
    // round 4 -- a stream of the compute stream's class can share its hardware queue, and then the copy's dependencies
    // wait behind a tracker launch
    hipStream_t copy_hi[2] = {nullptr, nullptr};
    unsigned upload_seq = 0;
    // pyramids built ahead of their step: not on an upload stream, where a 12 MB upload of a LATER frame would stand
    // between a pyramid and the tracker launch that waits for it
    hipStream_t pyr_stream = nullptr;
    // staging for 3-channel uploads
    uint8_t* d_bgr = nullptr;
    int bgr_pitch = 0;
    bool pyr_per_level = false;            // ICELK_PYR_PER_LEVEL=1: one pyrDown launch per level (A/B, second statement)
    // JPEG ingest.  What ONE file owns while it is decoded: coefficients, component planes, and for the Huffman decoding
    // on the device (icelk_upload_jpeg_file ...) the file, its segments and tables and the lanes' arrays; grown on demand,
    // because the file may be larger than max_w x max_h (the crop is what has to fit).  The synchronous calls share one
    // job; every file of icelk_upload_jpeg_file_async has its own until icelk_jpeg_async_finish (abi_jpeg_job.hip).
    // The JPEG writer (abi_jpeg_enc.hip), allocated at first use: the tables, the blocks' bit lengths, the groups' offsets,
    // the packed and the stuffed stream -- grown to what a file measures by the synchronous calls, which share one
    // (Jpeg::enc), allocated to the job's budget by a crop job, which has its own.  `resaved` / `info`: the handle has run
    // the forward kernel, and for which file; `stream_ok`: d_out holds that file's scan (stream_len bytes)
    struct JpegEnc {
        uint32_t* d_codes = nullptr;
        int16_t* d_coef = nullptr;     // of icelk_jpeg_encode_coefficients only
        uint16_t* d_bits = nullptr;
        uint32_t *d_group = nullptr, *d_ctl = nullptr, *d_packed = nullptr, *d_ff = nullptr;
        uint8_t* d_out = nullptr;
        uint32_t* h_ctl = nullptr;     // pinned
        size_t coef_cap = 0, bits_cap = 0, group_cap = 0, packed_cap = 0, ff_cap = 0, out_cap = 0;   // elements
        bool resaved = false, stream_ok = false;
        icelk_jpeg_info_t info{};
        uint64_t stream_len = 0;
    };
    // One file's working set is split by owner, and every part has ONE free function (which nulls what it frees): a field
    // added to a part is freed wherever the part is embedded.
    // The decoder's part (jpeg_dec_free, abi_jpeg_ingest.hip): coefficients, planes and the Huffman decoder's arrays
    struct JpegDec {
        int16_t* d_coef = nullptr;
        uint8_t* d_planes = nullptr;
        size_t coef_cap = 0, planes_cap = 0;   // elements / bytes
        uint8_t* d_file = nullptr;
        lanes::Seg* d_seg = nullptr;
        lanes::HuffTable* d_tabs = nullptr;
        uint64_t *d_T = nullptr, *d_X = nullptr;
        uint32_t *d_cnt = nullptr, *d_P = nullptr, *d_ctl = nullptr;
        int32_t* d_dc = nullptr;
        size_t file_cap = 0, seg_cap = 0, lane_cap = 0, group_cap = 0, dc_cap = 0;
    };
    // The re-save's part (jpeg_resave_free, abi_jpeg_enc.hip): what the forward kernel reads and writes, and the coder
    // behind it.  A crop job and a slot-bound re-save job have one each, the picture writer has one for every picture
    struct JpegResave {
        uint8_t* d_rgb = nullptr;        // the R G B image, rows 3 * width bytes apart
        int16_t* d_rcoef = nullptr;      // the re-save's coefficients (described by rinfo)
        size_t rgb_cap = 0, rcoef_cap = 0;
        JpegEnc enc;                     // the coder's buffers: at the job's budget, or grown to what a picture measures
        icelk_jpeg_info_t rinfo{};       // of the re-saved file (jobs only)
    };
    // A file in flight (abi_jpeg_job.hip; freed by free_job there): the two parts above and what start, poll and finish keep.
    // kind: a slot's frame as decoded / a slot's frame re-saved (icelk_upload_jpeg_file_async_resave: the crop box of
    // dec.d_planes goes through the fused kernel into rs.d_rcoef, whose inverse DCT needs planes of its own before the
    // gray of the slot is made of them) / a crop job (abi_jpeg_crop.hip: decode -> crop -> re-save -> encode, owned by a
    // ticket instead of a slot)
    enum JpegJobKind { JOB_SLOT, JOB_SLOT_RESAVE, JOB_CROP };
    struct JpegJob {
        JpegDec dec;
        JpegResave rs;
        JpegJobKind kind = JOB_SLOT;
        bool want_file = false;          // the chain codes rs.d_rcoef as well (always, for a crop job)
        uint8_t* h_stage = nullptr;      // pinned: tables | segment table | the file's bytes (what the host decoder reads)
        size_t stage_cap = 0, file_off = 0;
        uint32_t* h_verdict = nullptr;   // pinned, device-visible: JpegVerdictWord
        uint32_t seq = 0;                // h_verdict[JV_SEQ] == seq: the verdict of the file in flight has arrived
        hipEvent_t done = nullptr;       // behind the verdict kernel
        hipStream_t st = nullptr;        // the decode stream the file went out on
        int slot = -1;                   // the slot that owns the job, -1: none
        int ticket = -1;                 // the ticket that owns the job, -1: none
        bool enqueued = false;           // something of the job may be on its stream: a failing start waits for it
        bool host_only = false;          // nothing was enqueued (a file of 256 MiB or more): the host decoder takes it
        uint64_t len = 0;
        int variant = 0;
        uint32_t segments = 0, subsequences = 0;
        icelk_jpeg_info_t info{};
        JpegIdctArgs idct{};             // of the file and its crop: what a second transform after the host decoder runs on
        JpegOutArgs out{};
        uint8_t* d_planes2 = nullptr;    // JOB_SLOT_RESAVE: the planes of the re-saved file
        size_t planes2_cap = 0;
        JpegIdctArgs ridct{};            // of the re-saved file, whole
        JpegOutArgs rout{};
        uint8_t* h_out = nullptr;        // pinned: the finished scan
        size_t hout_cap = 0;
        uint32_t budget = 0;             // bytes the stuffed scan may take on the device
        bool have_scan = false;          // h_out holds the scan (scan_len bytes): finish has done its waiting
        uint64_t scan_len = 0;
        icelk_jpeg_crop_stats_t cstats{};
    };
    struct Jpeg {
        JpegDec sync;                                          // the working set of every synchronous call
        // the re-save (abi_jpeg_resave.hip), allocated at first use: the cropped R G B image the forward kernel reads
        // (rows 3 * width bytes apart), and the coefficients and planes of the re-saved file (of `resave` only those two)
        JpegDec resave;
        uint8_t* d_src = nullptr;
        size_t src_cap = 0;
        // the JPEG writer of the synchronous calls (JpegEnc above)
        using Enc = JpegEnc;
        Enc enc;
        uint8_t* d_rgb = nullptr;                              // the decoded image (icelk_jpeg_decode_rgb only)
        size_t rgb_cap = 0;
        int subseq_bits = 512, max_hops = lanes::kGroup, max_rounds = 8;   // icelk_jpeg_huff_config
        icelk_jpeg_huff_stats_t stats{};                                     // of the latest synchronous file
        // asynchronous ingest: a small ring of jobs (allocated at first use, grown when all are in flight), which job a
        // slot owns (-1: none), what icelk_jpeg_async_poll answers for a slot whose job is finished, and the decode streams
        std::vector<JpegJob*> ring;
        std::vector<int> slot_job, slot_state;
        hipStream_t dec[2] = {nullptr, nullptr};
        unsigned dec_seq = 0;
        int dec_streams = 2;                                   // ICELK_JPEG_ASYNC_STREAMS=1|2 (A/B)
        bool dec_high = false;                                 // ICELK_JPEG_ASYNC_PRIO=high|normal
        int crop_bytes_per_block = enc::kDefaultBytesPerBlock;   // icelk_jpeg_crop_config
        int crop_next_ticket = 1;
        hipStream_t fetch = nullptr;                           // D2H copies of finished scans (abi_jpeg_job.hip: jpeg_fetch_scan)
    } jpeg;

    // ---- abi_picture.hip: the picture writer's working set, allocated at first use: d_rgb is what k_plot_resolve and
    // k_map_resolve (and k_map_inset) write and the forward kernel or the PNG coder reads.  It belongs to pictures alone
    // -- the re-save's and the crop jobs' buffers are never touched, so crops and pictures can be asked for together --
    // and ONE set serves the segment picture and the velocity map.  That is safe because every picture call runs on the
    // handle's compute stream and has waited for the device when it returns: no two are ever in flight.  An asynchronous
    // picture call would break it: the next call would draw over, or grow() would free, what the first still reads
    JpegResave picture;
    int picture_w = 0, picture_h = 0;   // of the picture d_rgb holds: the one picture_write saw last (0: none yet)

    // ---- abi_movie.hip: the scaler and the movie frame, allocated at first use.  The two axes' tables stay on the device,
    // keyed by (in, out): every frame of a movie has the same sizes and uploads nothing.  `frame` is the movie frame's own
    // working set (its R G B, coefficients and coder), so a frame leaves the picture's R G B and file as they are
    struct Movie {
        struct Axis {                    // [0] horizontal, [1] vertical
            resize::Axis host;           // what the upload reads: lives as long as the handle
            int32_t* d = nullptr;        // first | count | k
            size_t cap = 0;
            bool valid = false;          // d holds host's table
        } axis[2];
        uint8_t *d_mid = nullptr, *d_src = nullptr, *d_out = nullptr;   // between the passes; icelk_resize_rgb's picture and result
        size_t mid_cap = 0, src_cap = 0, out_cap = 0;
        JpegResave frame;
    } movie;

    // ---- abi_plot.hip: the segment picture's own buffers, allocated at first use
    struct Plot {
        uint8_t* d_bg = nullptr;        // Wo x Ho gray plane, padded to four pixels
        uint32_t* d_counts = nullptr;   // lines | dots, each padded to four pixels
        uint32_t* d_tables = nullptr;   // TL | TD
        float* d_tracks = nullptr;      // the caller's tracks (icelk_plot_tracks)
        size_t bg_cap = 0, counts_cap = 0, tracks_cap = 0;
    } plot;

    // ---- abi_map.hip: the velocity map's own buffers, allocated at first use.  The day's arrows
    // of icelk_map_arrows_set and the inset thumbnails of icelk_map_inset_set_* stay resident until release / destroy
    struct Map {
        uint32_t* d_planes = nullptr;   // base | top | count, each padded to four pixels
        double* d_items = nullptr;      // per call: cells, outline and the caller's arrows of every panel
        uint8_t* d_measured = nullptr;
        map::Scene* d_scene = nullptr;
        map::Scene* h_scene = nullptr;  // what the copy into d_scene reads: lives as long as the handle
        size_t planes_cap = 0, items_cap = 0, measured_cap = 0;
        double* d_arrows = nullptr;     // resident: (n, 5)
        int32_t* d_group = nullptr;     // resident: NULL or n
        int n_arrows = 0;
        bool have_arrows = false;
        // resident: the thumbnails of icelk_map_inset_set_file / _pixels, R G B rows 3 inset_w bytes apart; NULL: not set
        uint8_t* d_inset[thumb::kMaxInsets] = {};
        int inset_w[thumb::kMaxInsets] = {}, inset_h[thumb::kMaxInsets] = {};
    } map;

    // ---- abi_png.hip: the PNG writer, allocated at first use and grown to what a picture takes.  A working set of its own:
    // a picture's PNG (picture_write) reads the writer's R G B and writes here, icelk_png_encode_rgb uploads into d_src
    struct Png {
        uint8_t* d_src = nullptr;       // the caller's picture (icelk_png_encode_rgb only), rows 3 * width bytes apart
        uint8_t* d_F = nullptr;         // the filtered stream, whole segments
        uint16_t* d_tok = nullptr;      // the tokens, whole segments
        uint32_t *d_seg = nullptr, *d_adler = nullptr, *d_stream = nullptr, *d_ctl = nullptr;
        uint32_t* h_ctl = nullptr;      // pinned
        size_t src_cap = 0, F_cap = 0, tok_cap = 0, seg_cap = 0, adler_cap = 0, stream_cap = 0;   // elements
    } png;

    // ---- abi_ortho.hip: the mosaic in progress, allocated at first use.  Its R G B is the picture writer's d_rgb (one
    // picture at a time: `draws` is picture_draws as the mosaic's own calls left it, and another kind of picture drawn
    // in between ends the mosaic); cover and best are planes of the raster's width x height
    struct Ortho {
        uint8_t* d_cover = nullptr;
        double* d_best = nullptr;
        uint8_t* d_src = nullptr;       // the pixels of icelk_ortho_add_pixels
        size_t cover_cap = 0, best_cap = 0, src_cap = 0;
        bool active = false;
        unsigned long long draws = 0;
        icelk_ortho_raster_t raster{};
        icelk_ortho_opts_t opts{};
    } ortho;
    // ---- abi_stab.hip: the anchor mask (resident until released) and the scratch of a stabilisation, allocated at first use
    // for max_pts rows; keys and w are sized by the vertices seen so far
    struct Stab {
        uint8_t* d_mask = nullptr;      // mask_w x mask_h bytes, rows mask_w apart
        int mask_w = 0, mask_h = 0;
        float* d_tracks = nullptr;      // the caller's table (icelk_stab_tracks)
        uint8_t *d_flags = nullptr, *d_anchor = nullptr, *d_w = nullptr;
        int* d_idx = nullptr;           // max_pts row numbers
        unsigned long long* d_keys = nullptr;
        double* d_med = nullptr;        // 2 (kMaxVert - 1)
        StabOut* d_out = nullptr;       // the per-vertex results and the counts
        size_t tracks_cap = 0, keys_cap = 0, w_cap = 0;
        bool ready = false;
    } stab;
    unsigned long long picture_draws = 0;   // picture_grow calls: every picture drawn into picture.d_rgb makes one first

    // ---- abi_lk.hip: point buffers of the plain LK entry points (the segment tracker's diagnostic arrays too)
    float *d_p0 = nullptr, *d_p1 = nullptr, *d_p0r = nullptr, *d_err_f = nullptr, *d_err_b = nullptr, *d_dist = nullptr;
    uint8_t *d_st_f = nullptr, *d_st_b = nullptr, *d_valid = nullptr;

    // ---- abi_detect.hip: detector streams, mask, candidate buffers, detector sets
    // Detection (corner candidates, min-distance, sort) runs on its own stream: it only needs the frame,
    // not the tracker's results, so it overlaps the LK launch of the same frame (s1:323-326 vs s1:437).
    hipStream_t det_stream = nullptr;
    hipEvent_t det_done = nullptr;      // corners of the latest detection are in d_corners
    hipEvent_t corners_free = nullptr;  // the compute stream has consumed d_corners
    float* d_corners = nullptr;         // (max_pts,2) corner list of the latest detection finished by the host's tail
    // detector mask
    uint8_t* d_mask = nullptr;
    int mask_pitch = 0;
    bool has_mask = false;
    int mask_w = 0, mask_h = 0;
    size_t ncell_cap = 0;
    // Output of the corner kernel (candidate regions, per-tile counts, masked maximum), triple buffered: the
    // candidates of a FUTURE detection frame can be produced (icelk_seg_detect_prepare, on eig_stream) while the
    // min-distance stages of the detections in flight still read their own.  A detector set's D.cb always mirrors
    // eo[its eo_active].buf (activate_eig_out).
    struct CandKey {   // whose candidates a buffer holds: a slot's frame as it was (gen), for one blockSize, one mask, one detector
        int slot = -1, block_size = 0, use_mask = 0;
        unsigned long long gen = 0, mask_gen = 0;
        Response resp;
        bool operator==(const CandKey& o) const
        {
            return slot == o.slot && gen == o.gen && block_size == o.block_size && use_mask == o.use_mask && mask_gen == o.mask_gen &&
                   resp == o.resp;
        }
    };
    struct EigOut {
        CandBuf buf{};
        double quality = 0;          // candidates below max * quality were never given their exact key (0: none were cut)
        hipEvent_t done = nullptr;
        bool valid = false;          // holds the prepared candidates `key` names
        CandKey key;
    } eo[3];
    // Two detections may be in flight (begun, not finished): the min-distance stage of frame d+2 is issued before the
    // host round trip of frame d, so that the round trip finds kernels that had a whole tracker launch to finish
    // instead of standing in a serial loop with them.  Everything a detection owns is in its detector set; every
    // detector function is handed the set it works on.
    struct DetSet {
        DetectScratch D{};                // D.eig (the full-frame map of icelk_min_eig_map) is shared by both sets
        DetectJob job{};
        int* h_counts = nullptr;          // pinned, device-visible: the job's counts, laid out by CountsWord (icelk_internal.h)
        int counts_seq = 0;               // its word CW_SEQ == counts_seq: the counts published last have arrived
        hipEvent_t counts_ev = nullptr;   // h_counts holds the counts of this set's detection
        hipEvent_t tail_done = nullptr;   // the tail of this set's latest detection (sort, emit, counter reset) is through
        size_t reset_ncell = 0;           // the detector counters are known to be zero for grids up to this many cells
        bool counters_clean = false;
        int eo_active = 0;                // the candidate buffer D points at
    } dset[2];
    // the set of the latest detector call (begin, finish, min_eig_map): icelk_detect_fast_stats reports its candidate buffer
    int dset_last = 0;
    hipStream_t tail_stream = nullptr;     // see detect_finish
    unsigned long long job_seq = 0;
    hipStream_t eig_stream = nullptr;
    unsigned long long mask_gen = 0;
    double prep_quality = 0;   // qualityLevel of the latest detection begun: what icelk_seg_detect_prepare cuts its candidates at

    bool host_tail = false;           // ICELK_HOST_TAIL=1: the tail of every detection through the host, as before round 4 (A/B)
    int tail_force_status = 0;        // ICELK_TAIL_FORCE_STATUS=1|2: the device verdict is forced to "host's tail" (tests of that path)
    long long tails_dev = 0, tails_host = 0;   // segments staged by the device-driven tail / by the host's
    int last_candidates = 0, last_accepted = 0;   // of the latest detection
    double prune_factor = 8.0;                    // candidates kept per corner wanted (top-K pruning: new_job, update_prune_factor)

    // ---- abi_segments.hip: segment sets, template tables, the deferred pair, read-out buffers
    // Segment state, six sets (kSegSets).  More than one because, while the tracker launch of a detection frame still
    // extends the closing segment in one set, the new segment is initialised in another (on the detection stream, right
    // after the corners are emitted) -- the next tracker launch does not have to wait for an initialisation queued
    // behind its predecessor.
    // Six sets rotate: the current segment, the one staged for the next switch (sb_cur + 1), the one closed by the
    // latest switch (sb_cur - 1), whose last pair may still be waiting (icelk_seg_track_defer) and whose tracks stay
    // readable (icelk_seg_archive_closed) until the switch after, the one before that, which a tracker launch
    // may still be working on when the host, a launch ahead of the device, stages the next segment -- and, since the tail
    // of a detection writes the new segment's tables without the host (k_tail.hip), the sets behind the staged one that
    // the detections in flight (two at most) have reserved (DetectJob::seg_set).
    struct SegBuf {
        float* live = nullptr;      // (max_pts,2) current position of every track of the segment
        uint8_t* alive = nullptr;   // 1 while the track survives
        int* order = nullptr;       // spatial launch order of the segment's tracks (k_seg_order)
        int* order_border = nullptr;   // 1 int: leading entries of `order` that are border features
        float* tracks = nullptr;    // [track][kMaxVert][2]
        float* quality = nullptr;   // [track][kMaxVert-1]
        // last launch on the compute stream that touches this set: own event or a shared launch event (see Slot::used)
        hipEvent_t used = nullptr, used_own = nullptr;
        hipEvent_t ready = nullptr;   // the tables of the segment staged in this set are written (detection or tail stream)
        int vert = 0, upper = 0;    // vertices so far, tracks of the segment (= corners detected)
        // templates the backward pass of the latest pair left in tmpl.buf[set & 1] serve the forward pass of the pair that
        // writes vertex `tmpl_for` (with the window / levels of tmpl_key); -1: none
        int tmpl_for = -1, tmpl_key = 0, tmpl_slot = -1;
        unsigned long long tmpl_gen = 0;
    } sb[kSegSets];
    // Template reuse between the pairs of a segment (LKBuffers::tmpl_out; k_lk_fast.hip).  Consecutive segments use
    // consecutive sets, and at most two segments have launches in flight: two tables, picked by the parity of the set.
    struct {
        void* buf[2] = {nullptr, nullptr};
        size_t bytes = 0;          // per table
        size_t row_bytes = 0;      // bytes per track the tables were laid out for (levels x quads x 64 lanes x 16 B)
        size_t budget = (size_t)8 << 30;   // both tables together (ICELK_TEMPLATE_BUDGET_MB)
        int quads = 0, levels = 0;
        bool off = false;          // ICELK_NO_TEMPLATE_REUSE, or the tables could not be allocated
        bool failed = false;       // ... the latter
        long long taken = 0, left = 0;   // pairs whose forward pass took templates / whose backward pass left them
    } tmpl;
    int track_len_hint = 0;        // icelk_seg_track_len_hint: pairs per segment (0: unknown -- every pair leaves templates)
    hipEvent_t launch_ev[kLaunchEvents] = {nullptr};   // one per tracker launch, round robin
    int launch_seq = 0;
    int sb_cur = 0;
    bool closed_valid = false;
    struct Deferred {
        bool pending = false;
        int set = 0, slot_prev = 0, slot_next = 0;
        LKJob job{};
        LKParams P{};
    } defer;
    bool seg_ready_pending = false;   // the compute stream has not been told yet to wait for the current set's tables (SegBuf::ready)
    bool use_order = true;                 // ICELK_NO_ORDER=1 launches in detector order (A/B measurements)
    // features this close to the frame border count as slow (launched first): from the window and pyramid depth of the
    // latest tracker call
    int border_px = (10 + kLkTileMargin + 2) << 2;
    bool seg_active = false;
    bool seg_staged = false;   // the OTHER set holds a new segment waiting for icelk_seg_switch
    int staged_n = 0;
    unsigned long long* d_tracked = nullptr;   // 64 sharded counters
    unsigned long long* h_seg = nullptr;   // pinned: {alive tracks, features tracked}
    float *d_out_tracks = nullptr, *d_out_quality = nullptr;

    // ---- abi_post.hip: scratch of what runs after the frame loop
    struct Post {
        // projection epilogue: outputs x, y, u, v, speed (5 planes of proj_cap doubles) + keep bytes, grown on demand
        double* d_proj = nullptr;
        uint8_t* d_keep = nullptr;
        size_t proj_cap = 0;
        // the velocity cube of icelk_cube_set: u, v, count as [window][cell] float64, resident until release / destroy
        double *d_cube_u = nullptr, *d_cube_v = nullptr, *d_cube_count = nullptr;
        int cube_ncells = 0, cube_nt = 0;
    } post;

    // ---- abi_calib.hip: the scene of icelk_calib_set, resident until release / destroy
    struct Calib {
        double* d_shore = nullptr;   // (M, 2): xi, yi relative to the image centre
        double* d_water = nullptr;   // (W, 2): waterline vertices
        int M = 0, W = 0;
        double E = 0, N = 0;
    } calib;
};

// once per process (defined in abi_handle.hip)
extern std::string g_create_err;
extern std::mutex g_mu;

#define HIPCHK(c, expr)                                                                      \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            (c)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                    \
            return ICELK_EHIP;                                                               \
        }                                                                                    \
    } while (0)

#define FAIL(c, code, msg)   \
    do {                     \
        (c)->err = (msg);    \
        return (code);       \
    } while (0)

inline Ctx* C(icelk_t* h) { return reinterpret_cast<Ctx*>(h); }

inline int check_launch(Ctx* c, const char* what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        c->err = std::string(what) + ": " + hipGetErrorString(e);
        return ICELK_EHIP;
    }
    return ICELK_OK;
}

// ---- roctx ranges (tracing) --------------------------------------------------------------------
// ICELK_ROCTX=1: the host calls of the frame loop appear as named ranges in a rocprofv3 --marker-trace (tracker launch,
// detection begin / stage, candidates ahead, pyramid ahead, upload).  The marker library is looked up at run time
// (librocprofiler-sdk-roctx.so, else libroctx64.so): no link-time dependency, nothing is called when the variable is unset.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx();
};
Roctx& roctx();   // one per process: abi_handle.hip
struct Range {
    bool on;
    explicit Range(const char* name) : on(roctx().push != nullptr)
    {
        if (on) roctx().push(name);
    }
    ~Range()
    {
        if (on) roctx().pop();
    }
};

struct ProfScope {
    Ctx* c;
    int id;
    hipStream_t st;
    ProfEvt ev{};
    ProfScope(Ctx* c_, int id_, hipStream_t st_ = nullptr) : c(c_), id(id_), st(st_ ? st_ : c_->stream)
    {
        on = c->prof && (!c->prof_tracker_only || id == K_LK_FB || id == K_LK_FB_PAIR || id == K_LK);
        if (on) {
            if (!c->evt_pool.empty()) {
                ev = c->evt_pool.back();
                c->evt_pool.pop_back();
            } else {
                hipEventCreate(&ev.a);
                hipEventCreate(&ev.b);
            }
            ev.id = id;
            hipEventRecord(ev.a, st);
        }
    }
    ~ProfScope()
    {
        if (on) {
            hipEventRecord(ev.b, st);
            c->evts.push_back(ev);
        }
    }
    bool on = false;
};

inline int check_gray_variant(Ctx* c, int gray_variant)
{
    if (gray_variant != ICELK_GRAY_CV3 && gray_variant != ICELK_GRAY_CV4) FAIL(c, ICELK_EARG, "bad gray variant");
    return ICELK_OK;
}

inline int align_up(int v, int a) { return (v + a - 1) / a * a; }

template <typename T>
int dmalloc(Ctx* c, T** p, size_t count)
{
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), sizeof(T) * (count ? count : 1));
    if (e != hipSuccess) {
        c->err = std::string("hipMalloc: ") + hipGetErrorString(e);
        return ICELK_ENOMEM;
    }
    return ICELK_OK;
}

template <typename T>
int grow(Ctx* c, T** p, size_t* cap, size_t want)
{
    if (*cap >= want) return ICELK_OK;
    if (*p) HIPCHK(c, hipFree(*p));   // waits for everything that may still use the buffer
    *p = nullptr;
    *cap = 0;
    if (int rc = dmalloc(c, p, want)) return rc;
    *cap = want;
    return ICELK_OK;
}

// ---- per-call device buffers, copies and timing of the stages after the frame loop (abi_post.hip, abi_calib.hip)
struct DevBufs {   // frees whatever was allocated when it goes out of scope; remembers a failed allocation
    std::vector<void*> p;
    bool failed = false;
    ~DevBufs()
    {
        for (void* q : p)
            if (q) hipFree(q);
    }
    template <typename T>
    T* get(size_t count)
    {
        void* q = nullptr;
        if (hipMalloc(&q, sizeof(T) * (count ? count : 1)) != hipSuccess) return failed = true, nullptr;
        p.push_back(q);
        return reinterpret_cast<T*>(q);
    }
    bool ok() const { return !failed; }
};

// n elements on stream s (D and S differ in name at most: int64_t / long long)
template <typename D, typename S>
inline hipError_t copy_n(D* dst, const S* src, size_t n, hipMemcpyKind kind, hipStream_t s)
{
    static_assert(sizeof(D) == sizeof(S), "element sizes differ");
    return hipMemcpyAsync(dst, src, sizeof(D) * n, kind, s);
}
constexpr hipMemcpyKind kH2D = hipMemcpyHostToDevice, kD2H = hipMemcpyDeviceToHost;

// two events around a stretch of a stream: the device_ms of the day gridder and of the cube average
struct EvPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EvPair()
    {
        if (a) hipEventDestroy(a);
        if (b) hipEventDestroy(b);
    }
    int create(Ctx* c)
    {
        HIPCHK(c, hipEventCreate(&a));
        HIPCHK(c, hipEventCreate(&b));
        return ICELK_OK;
    }
};

// ---- the normalised median test's device side (abi_validate.hip), shared by icelk_validate and the validated day gridder
// The working arrays of one pass over n points and ngroups groups: keys, sorted keys, the sort's scratch, status, r2, the
// per-(group, cell) records, the groups' rejected counts.  The caller sets A.x, A.y, A.u, A.v (and A.group, A.t_kill).
struct ValidateDev {
    ValidateArgs A{};
    unsigned long long* keys_sorted = nullptr;
    void* sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0, nseg = 0;
    int key_bits = 0;
    void alloc(DevBufs& B, int n, int ngroups, const icelk_validate_lattice_t& L, const icelk_validate_params_t& P, hipStream_t s);
};
// Counters zeroed, `assign` (the caller's launch of one of the two assign kernels), the judged count read back -- the one
// wait --, sort, pools, judge; the results stay on the device.  t, if given: t[0] goes around the assign kernel, t[1] around
// the rest, as grid_core's.
int validate_run(Ctx* c, ValidateDev& V, const std::function<void()>& assign, EvPair* t);
// the lattice, the parameters and the outputs the validated day gridder takes (abi_post.hip)
struct ValidateDay {
    const icelk_validate_lattice_t* L;
    icelk_validate_params_t P;
    uint8_t* status;
    int32_t* rejected;
};

// ---- helpers that cross a stage boundary (each defined in the file named) -------------------------------------------
// abi_handle.hip
void prof_drain(Ctx* c);
hipError_t create_priority_stream(hipStream_t* s);
// abi_frames.hip
bool layout_ok(const Slot& s);
void layout_levels(Slot& s, int w, int h);
size_t slot_bytes(int w, int h);
int pyramid_top_level(int w, int h, int win_w, int win_h, int max_level);
int check_slot(Ctx* c, int slot, bool need_image);
int wait_event(Ctx* c, hipStream_t s, hipEvent_t e);
int await_pinned_seq(Ctx* c, const int* word, int seq, hipEvent_t ev);
int wait_slot(Ctx* c, int slot);
int ensure_pyramid(Ctx* c, int slot, int top_level);
Pyramid pyramid_of(const Slot& s);
int begin_frame(Ctx* c, int slot, int w, int h);
int end_frame(Ctx* c, Slot& s);
int foreign_write_begin(Ctx* c, Slot& s, hipStream_t st);
int foreign_write_end(Ctx* c, Slot& s, hipStream_t st);
// abi_jpeg.hip
bool jpeg_info_ok(const icelk_jpeg_info_t& in);
struct JpegIndex {   // a file as the lanes of jpeg_lanes.h see it
    icelk_jpeg_info_t info;
    lanes::HuffTable tabs[lanes::kTables];
    lanes::Scan scan;
    std::vector<lanes::Seg> seg;   // scan.nseg + 1
};
int jpeg_index(const uint8_t* d, size_t len, JpegIndex& X);
int jpeg_open_core(const uint8_t* data, uint64_t len, JpegIndex& X, icelk_jpeg_info_t* info, bool* host_only);
void jpeg_index_lanes(JpegIndex& X, uint32_t S, int max_hops);
bool jpeg_huff_config_ok(int subseq_bits, int max_hops, int max_rounds);
int jpeg_host_decode(const uint8_t* data, size_t len, int16_t* coef, uint64_t capacity);
// abi_jpeg_ingest.hip: the ingest steps (listed at the head of that file)
int check_crop_box(Ctx* c, const icelk_jpeg_info_t& I, int left, int top, int right, int bottom, int* w, int* h);
int jpeg_plane_args(Ctx* c, Ctx::JpegDec& B, const icelk_jpeg_info_t* I, int left, int top, int right, int bottom, JpegIdctArgs* A,
                    JpegOutArgs* out);
size_t jpeg_plane_bytes(const icelk_jpeg_info_t& I);
void jpeg_plane_layout(const icelk_jpeg_info_t& I, int left, int top, int right, int bottom, int16_t* d_coef, uint8_t* d_planes,
                       JpegIdctArgs* A, JpegOutArgs* out);
int jpeg_idct_on(Ctx* c, hipStream_t st, const JpegIdctArgs& A);
int jpeg_gray_on(Ctx* c, hipStream_t st, JpegOutArgs O, const Slot& s, int gray_variant);
int planes_to_gray_slot(Ctx* c, int slot, const JpegOutArgs& O, int gray_variant);
int jpeg_planes(Ctx* c, const icelk_jpeg_info_t* I, const int16_t* coef, int left, int top, int right, int bottom, JpegOutArgs* out,
                bool on_device = false);
int jpeg_rgb_out(Ctx* c, const icelk_jpeg_info_t& I, JpegOutArgs& O, uint8_t* out, int stride);
const char* jpeg_open_error(int rc);
int jpeg_open(Ctx* c, const uint8_t* data, uint64_t len, JpegIndex& X, icelk_jpeg_info_t* info, bool* host_only);
int jpeg_host_into_job(Ctx* c, Ctx::JpegDec& J, const uint8_t* data, uint64_t len, const icelk_jpeg_info_t& I, hipStream_t st,
                       std::vector<int16_t>& keep);
int jpeg_huff_setup(Ctx* c, Ctx::JpegDec& B, const JpegIndex& X, uint64_t len, JpegHuffArgs* H, bool headroom);
int jpeg_huff_stage(Ctx* c, Ctx::JpegDec& J, const JpegIndex& X, const uint8_t* file, const void* seg, const void* tabs, uint64_t len,
                    hipStream_t st);
void jpeg_huff_finish_phases(hipStream_t st, const JpegHuffArgs& H);
int jpeg_huff_device(Ctx* c, const uint8_t* data, uint64_t len, icelk_jpeg_info_t* info);
void jpeg_dec_free(Ctx::JpegDec& D);
// abi_jpeg_resave.hip
void jpeg_resave_destroy(Ctx* c);
int jpeg_resave_check(Ctx* c, int w, int h, int quality);
int jpeg_fwd_on(Ctx* c, hipStream_t st, const uint8_t* d_src, int16_t* d_coef, int w, int h, const icelk_jpeg_info_t& I);
int jpeg_crop_fwd_on(Ctx* c, hipStream_t st, const JpegOutArgs& O, int16_t* d_coef, const icelk_jpeg_info_t& I);
// abi_jpeg_enc.hip
void jpeg_enc_destroy(Ctx* c);
void jpeg_enc_free(Ctx::JpegEnc& E);
void jpeg_resave_free(Ctx::JpegResave& R);
int jpeg_enc_rc(Ctx* c, int rc);
int jpeg_enc_prepare(Ctx* c, Ctx::JpegEnc& E);
int jpeg_encode_on(Ctx* c, Ctx::JpegEnc& E, hipStream_t st, const enc::Layout& L, const int16_t* d_coef);
int jpeg_deliver_file(Ctx* c, const Ctx::JpegEnc& E, hipStream_t st, bool pending, const icelk_jpeg_info_t& I, const uint8_t* comment,
                      uint64_t comment_len, uint8_t* out, uint64_t capacity, uint64_t* len);
// abi_jpeg_job.hip: the driver of a file in flight (its steps are listed at the head of that file)
void jpeg_async_destroy(Ctx* c);
int jpeg_async_sync(Ctx* c);
int jpeg_take_job(Ctx* c, int* idx);
int jpeg_decode_stream(Ctx* c, hipStream_t* out);
int jpeg_stage_file(Ctx* c, Ctx::JpegJob& B, const JpegIndex& X, size_t seg_bytes, const uint8_t* data, uint64_t len);
bool jpeg_verdict_here(const Ctx::JpegJob& B);
int jpeg_await_verdict(Ctx* c, Ctx::JpegJob& B);
void jpeg_huff_stats_of(const Ctx::JpegJob& B, icelk_jpeg_huff_stats_t* st);
int jpeg_budget_buffers(Ctx* c, Ctx::JpegJob& B, const enc::Layout& L);
int jpeg_encode_budgeted(Ctx* c, Ctx::JpegJob& B, const enc::Layout& L);
int jpeg_fetch_scan(Ctx* c, Ctx::JpegJob& B, uint64_t n, bool again);
struct JpegBox {
    int left, top, right, bottom;
};
int jpeg_job_open(Ctx* c, Ctx::JpegJobKind kind, bool want_file, const uint8_t* data, uint64_t len, const JpegBox& box, int quality,
                  std::unique_ptr<JpegIndex>* X, int* idx, enc::Layout* L);
int jpeg_job_start(Ctx* c, Ctx::JpegJob& B, int slot, const uint8_t* data, uint64_t len, JpegIndex& X, const JpegBox& box,
                   const enc::Layout& L);
void jpeg_job_abandon(Ctx::JpegJob& B);
int jpeg_job_verdict(Ctx* c, Ctx::JpegJob& B, icelk_jpeg_huff_stats_t* huff, uint32_t* coder);
int jpeg_job_redo_on_host(Ctx* c, Ctx::JpegJob& B, const enc::Layout* L);
int jpeg_job_settle(Ctx* c, Ctx::JpegJob& B);
int jpeg_job_state(const Ctx::JpegJob& B, bool with_coder);
int jpeg_job_file(Ctx* c, const Ctx::JpegJob& B, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity,
                  uint64_t* len);
// abi_plot.hip
void plot_destroy(Ctx* c);
// abi_map.hip
void map_destroy(Ctx* c);
// abi_thumb.hip
void map_insets_free(Ctx* c);
// abi_png.hip
void png_destroy(Ctx* c);
int png_check(Ctx* c, int w, int h);
int png_grow(Ctx* c, int w, int h);
int png_encode_on(Ctx* c, hipStream_t st, const uint8_t* d_rgb, uint32_t stride, int w, int h, uint32_t* nbytes);
int png_deliver_file(Ctx* c, hipStream_t st, bool pending, int w, int h, uint32_t nbytes, uint8_t* out, uint64_t capacity, uint64_t* len);
// abi_picture.hip: the picture writer (its steps are listed at the head of that file)
enum PictureFormat { PICTURE_JPEG, PICTURE_PNG };
struct PictureFile {          // the file to write: what picture_check makes of the caller's arguments
    PictureFormat format;
    int Wo, Ho;
    size_t px;                // Wo Ho padded to four pixels: what every plane of a picture is sized to
    icelk_jpeg_info_t info;   // JPEG: of the file
    enc::Layout L;
};
void picture_destroy(Ctx* c);
int picture_check(Ctx* c, int Wo, int Ho, PictureFormat format, int quality, const uint8_t* rgb, int rgb_stride, const uint64_t* len,
                  PictureFile* F);
int picture_grow(Ctx* c, const PictureFile& F);
int picture_write(Ctx* c, hipStream_t st, const PictureFile& F, uint8_t* rgb_or_null, int rgb_stride, uint8_t* file, uint64_t capacity,
                  uint64_t* len);
// abi_movie.hip
void movie_destroy(Ctx* c);
// abi_ortho.hip
void ortho_destroy(Ctx* c);
// abi_stab.hip
void stab_destroy(Ctx* c);
// abi_lk.hip
int make_lk_params(Ctx* c, int w, int h, int win_w, int win_h, int max_level, int crit_type, int max_count,
                   double epsilon, int flags, double min_eig_thr, float fb_thr, LKParams* P);
// abi_detect.hip
int alloc_eig_out(Ctx* c, Ctx::EigOut& e, int cand_cap);
void free_eig_out(Ctx::EigOut& e);
int alloc_det_set(Ctx* c, Ctx::DetSet& S, int cand_cap);
void free_det_set(Ctx::DetSet& S);
void activate_eig_out(Ctx* c, Ctx::DetSet& S, int idx);
int detect_prepare(Ctx* c, int slot, int use_mask, int block_size);
int detect_begin(Ctx* c, int slot, int use_mask, int max_corners, double quality, double min_distance, int block_size,
                 bool for_segment);
// what detect_finish leaves behind; of a segment's tables and launch order the device-driven tail writes both, the host's the tables
struct DetectResult {
    int n = 0;   // corners
    bool tables_written = false, order_written = false;
    int w = 0, h = 0;   // of the frame the finished job detected on
};
int detect_finish(Ctx* c, int max_corners, int cap, Ctx::SegBuf* seg, DetectResult* out);
int detect_counts_arrived(Ctx* c, bool* arrived);
// abi_segments.hip
int flush_deferred(Ctx* c);
int flush_deferred_slot(Ctx* c, int slot);
int seg_gather_packed(Ctx* c, bool closed, int* out_n, int* out_vertices);
int seg_gather_counted(Ctx* c, bool closed, int* dev_count, int* out_upper, int* out_vertices);
// abi_post.hip
int check_projection_args(Ctx* c, const icelk_camera_t* cam, const icelk_utm_filter_t* filt);
int project_core(Ctx* c, const float* d_tracks_in, int n, int nv, const icelk_camera_t* cam, const icelk_utm_filter_t* filt,
                 int host_pitch, double* x, double* y, double* u, double* v, double* speed, uint8_t* keep);

}  // namespace icelk
