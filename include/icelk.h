/*
 * icelk.h -- C ABI of the MI355X-native sparse Lucas-Kanade tracking library (libicelk.so).
 *
 * This is the drop-in boundary for the ONE hot path of glacierbliss/iceberg_tracking_code: the
 * per-frame loop of s1_lucaskanade_tracking.py:307-450 (twin: s0_1_test_lucaskanade_tracking.py:77-181).
 * The reference has no FFI layer; the seam is three cv2 calls.  Each entry point below names the
 * reference call site it replaces.  Plain C: pointers and sizes only, no C++/torch types, no exceptions.
 *
 * Conventions
 *   - every function returns ICELK_OK (0) or a negative ICELK_E* code; icelk_last_error() gives text.
 *   - the caller owns every host buffer; the library owns all device memory (frames, pyramids, points).
 *   - a handle is bound to one GPU and is not thread-safe; use one handle per thread/process.
 *     Multi-GPU = one process per GPU, one handle each (DESIGN.md "Multi-GPU").
 *   - a handle owns SEVEN HIP streams: compute (tracker launches, segment bookkeeping; replaceable by the
 *     caller's stream, icelk_set_stream), two copy streams (icelk_upload_gray_async alternates between them), pyramid
 *     (icelk_build_pyramid_ahead), detection (min-distance stage), tail (what follows a detection's host round trip:
 *     sort, corner list, the new segment's tables) and candidates (the corner kernel of icelk_seg_detect_prepare).
 *     They are ordered against each other by events inside the library; a call whose outputs are host buffers has
 *     finished with them when it returns.  icelk_sync waits for ALL of them (and launches a pair held back by
 *     icelk_seg_track_defer first): after it nothing of the handle reads or writes any slot, mask or point buffer.
 *   - "slot" = a device-resident frame with its Gaussian pyramid.  Slots let the caller keep the
 *     previous frame (prev_gray = frame_gray, s1:450) and its pyramid on the GPU instead of
 *     rebuilding both pyramids in every cv2.calcOpticalFlowPyrLK call as OpenCV does.
 *   - points are interleaved (x, y) float32, i.e. numpy (N,1,2) float32 as cv2 returns them.
 *   - calls are synchronous with respect to their host outputs unless named *_async.
 */
#ifndef ICELK_H
#define ICELK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct icelk_ctx icelk_t;

#define ICELK_OK 0
#define ICELK_EARG (-1)    /* bad argument                       -> Python ValueError   */
#define ICELK_ENOMEM (-2)  /* host or device allocation failed   -> Python MemoryError  */
#define ICELK_EHIP (-3)    /* HIP runtime error                  -> Python RuntimeError */
#define ICELK_ECAP (-4)    /* exceeds the capacity given at icelk_create                */
#define ICELK_ESTATE (-5)  /* slot empty / pyramid missing / segment not started        */
#define ICELK_EUNSUP (-6)  /* a valid JPEG file of a kind the device decoder does not take */

/* cv2.TERM_CRITERIA_COUNT / cv2.TERM_CRITERIA_EPS (criteria tuple at s1:248) */
#define ICELK_CRIT_COUNT 1
#define ICELK_CRIT_EPS 2
/* cv2.OPTFLOW_USE_INITIAL_FLOW / cv2.OPTFLOW_LK_GET_MIN_EIGENVALS */
#define ICELK_FLAG_INITIAL_FLOW 4
#define ICELK_FLAG_MIN_EIGENVALS 8
/* testing aid: force the window-size-generic LK kernel where a specialised one exists (same results) */
#define ICELK_FLAG_GENERIC_KERNEL 0x100
/* the several-features-per-wave form of the specialised kernels (k_lk_multi.hip) instead of the default
 * one-feature-per-wave form: fewer instructions per feature, lower occupancy; same results */
#define ICELK_FLAG_MULTI_PER_WAVE 0x200
/* fixed-point coefficient sets of cv2.cvtColor(COLOR_BGR2GRAY): OpenCV 3.x (14 bit), 4.x (15 bit) */
#define ICELK_GRAY_CV3 3
#define ICELK_GRAY_CV4 4
/* forward-backward distance of icelk_track_fb / icelk_seg_track: np.hypot on float32 as s1:330 (default), or the
 * float32 expression (dx**2 + dy**2)**0.5 of the demo script s0_1:99 */
#define ICELK_FB_HYPOT 0
#define ICELK_FB_SQRT 1

#define ICELK_MAX_LEVELS 12 /* pyramid images per slot (maxLevel <= 11) */

/* ---- library / handle ------------------------------------------------------------------- */
int icelk_version(void);
/* Text of the last error on this handle (or of the last failed icelk_create when h == NULL). */
const char* icelk_last_error(icelk_t* h);
/* One handle per GPU.  max_w/max_h (<= 65535) bound the frame size, n_slots the resident frames,
 * max_pts the features per call (maxCorners / len(tracks)). */
int icelk_create(int device, int max_w, int max_h, int n_slots, int max_pts, icelk_t** out);
int icelk_destroy(icelk_t* h);
/* Run all work on the caller's HIP stream (hipStream_t as void*; NULL = the handle's own stream). */
int icelk_set_stream(icelk_t* h, void* hip_stream);
int icelk_sync(icelk_t* h);
/* Testing / measurement aid: which of the three bit-identical tracker kernels every LK call of this handle uses:
 * 0 = the default choice, ICELK_FLAG_GENERIC_KERNEL, or ICELK_FLAG_MULTI_PER_WAVE. */
int icelk_set_lk_kernel(icelk_t* h, int which);
/* How the fused tracker calls form dist from |p0 - p0r| (ICELK_FB_HYPOT / ICELK_FB_SQRT); the two can differ in
 * the last bit, which flips `valid` for a distance within one ulp of the threshold. */
int icelk_set_fb_distance(icelk_t* h, int form);
/* Named variants of the OpenCV semantics that depend on how OpenCV was BUILT (the oracle names the
 * same switches: oracle/icelk_oracle.c orc_set_variant, and tools/oracle_variants.py measures how far they are apart).
 * 0 is the default of each and what the tuned kernels compute; a non-zero value routes the call through the
 * window-generic tracker kernel / the any-blockSize corner kernel, which carry the variants (slower, same interface):
 *   "lk_sums"    1 | 2   A11, A12, A22, b1, b2 summed in the float lanes of OpenCV 3.x's SSE2 block | 4.x's CV_SIMD128 block
 *                        instead of exactly (at the reference's own parameters 5 of 40 416 features move by more than
 *                        1e-3 px between the forms, none changes status)
 *   "sobel_fma"  bit 0   the Sobel column pass fused (4.x SymmColumnSmallVec_32f in an FMA3 build); bit 1: the row pass fused
 *   "eig_fma"    1       calcMinEigenVal's (a-c)^2 + b^2 as one fused multiply-add
 *   "harris_tail" 1      the Harris response (icelk_set_detector) as calcHarris' scalar tail computes it, k kept a double:
 *                        (float)((double)(fl(a c) - fl(b b)) - (k (double)fl(a + c)) (double)fl(a + c)); 0 = its float lanes.
 *                        Read only while the Harris detector is selected (and by icelk_harris_map); on the test frames the two
 *                        forms differ in the last bit of about half the map and give the same corner list.
 * (the corner SET is the same under all of them on the test frames, the order of near-equal corners changes.)
 * A cv2 cross-check that finds one of them to be what the reference's OpenCV build does flips this switch.
 * One name is a testing aid and changes no result:
 *   "lk_wide_sums" 1     the tuned tracker kernels reduce A11 .. b2 in 64 bits everywhere; by default (0) a wave whose lane
 *                        partials all lie below 2^25 in magnitude takes the 32-bit reduction, which gives the same float bit
 *                        for bit.  (No switch forces the 32-bit arm: beyond the guard it would be wrong.) */
int icelk_set_variant(icelk_t* h, const char* name, int value);

/* ---- frame ingest: replaces cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY) at s1:283,311 / s0_1:71,80 */
/* host 8-bit gray image -> slot (level 0); invalidates the slot's pyramid. */
int icelk_upload_gray(icelk_t* h, int slot, const uint8_t* host, int w, int h_, int stride);
/* host 8-bit 3-channel image -> gray in slot.  Channel 0 gets the "B" coefficient: feeding PIL's RGB
 * arrays, as the reference does (s1:310-311), reproduces its swapped weights. */
int icelk_upload_bgr(icelk_t* h, int slot, const uint8_t* host, int w, int h_, int stride, int gray_variant);
/* same two, from device memory (e.g. a torch tensor's data_ptr) */
int icelk_set_gray_device(icelk_t* h, int slot, const void* dev, int w, int h_, int stride);
int icelk_cvt_bgr_device(icelk_t* h, int slot, const void* dev_bgr, int w, int h_, int stride, int gray_variant);
/* asynchronous upload from PINNED host memory on the handle's copy stream (double-buffered
 * streaming, BASELINE.json configs[2]); compute on `slot` waits for the copy by an event. */
int icelk_upload_gray_async(icelk_t* h, int slot, const uint8_t* pinned_host, int w, int h_, int stride);
int icelk_host_alloc(void** out, uint64_t bytes); /* pinned host memory for the call above */
int icelk_host_free(void* p);
/* procedural frame generated on the device (integer value noise, bit-identical to
 * iceberg_tracking_code_amd/synth.py); ux,uy = shift in 1/256 px. */
int icelk_synth_frame(icelk_t* h, int slot, int w, int h_, int64_t ux, int64_t uy, uint32_t seed);
/* the same with a small affine deformation on top of the shift: the texture is sampled at
 * x + ux/256 + (a[0] x + a[1] y) / 2^20,  y + uy/256 + (a[2] x + a[3] y) / 2^20  (|a[k]| <= 2^13, i.e. 0.8 %), so the
 * motion between two frames varies over the frame (shear / scale / rotation); NULL = none. */
int icelk_synth_frame_affine(icelk_t* h, int slot, int w, int h_, int64_t ux, int64_t uy, uint32_t seed,
                             const int32_t* affine);
/* Forget levels >= 1 of a slot whose level 0 stays resident, so the next tracker call rebuilds the
 * pyramid (a frame that is already in HBM re-enters the loop without a copy). */
int icelk_drop_pyramid(icelk_t* h, int slot);
/* read back pyramid level `level` of a slot (level 0 = the gray frame). */
int icelk_download_level(icelk_t* h, int slot, int level, uint8_t* host, int stride, int* w, int* h_);

/* ---- pyramid: cv::buildOpticalFlowPyramid inside cv2.calcOpticalFlowPyrLK (s1:323,326) -------- */
/* Builds levels 1..L of the slot, L = min(max_level, first level whose successor is <= winSize).
 * *out_levels receives L.  icelk_pyrlk / icelk_track_fb call this themselves when needed. */
int icelk_build_pyramid(icelk_t* h, int slot, int win_w, int win_h, int max_level, int* out_levels);
/* The same build enqueued on the handle's copy stream, for a frame that will be tracked LATER: it follows an
 * icelk_upload_gray_async of the slot in stream order and overlaps whatever the compute stream is doing; the
 * next call that needs the pyramid waits for it.  Returns at once. */
int icelk_build_pyramid_ahead(icelk_t* h, int slot, int win_w, int win_h, int max_level);

/* ---- tracker: replaces cv2.calcOpticalFlowPyrLK(img0, img1, p0, None, **lk_params) s1:323,326 - */
/* next_xy is an input as well when flags has ICELK_FLAG_INITIAL_FLOW.  n == 0 is not an error. */
int icelk_pyrlk(icelk_t* h, int prev_slot, int next_slot, const float* prev_xy, float* next_xy,
                uint8_t* status, float* err, int n, int win_w, int win_h, int max_level,
                int crit_type, int max_count, double epsilon, int flags, double min_eig_threshold);
/* Fused forward + backward + distance test of s1:323-333 (one launch, pyramids built once):
 *   p1 = LK(slot0 -> slot1, p0);  p0r = LK(slot1 -> slot0, p1);
 *   dist = np.hypot(|p0 - p0r|) on float32 (s1:329-330; see icelk_set_fb_distance);  valid = dist < fb_threshold.
 * Any output pointer may be NULL. */
int icelk_track_fb(icelk_t* h, int slot0, int slot1, const float* p0, int n, int win_w, int win_h,
                   int max_level, int crit_type, int max_count, double epsilon, double min_eig_threshold,
                   float fb_threshold, float* p1, float* p0r, uint8_t* st_fwd, uint8_t* st_bwd,
                   float* err_fwd, float* err_bwd, float* dist, uint8_t* valid);

/* The filter of s1:329-333 on its own, for callers of the plain icelk_pyrlk: diff = abs(p0 - p0r) in float32,
 * dist = np.hypot(diff) (or the s0_1:99 form, icelk_set_fb_distance), valid = dist < fb_threshold.  Runs the very
 * device function the fused launches end with.  dist / valid may be NULL. */
int icelk_fb_filter(icelk_t* h, const float* p0, const float* p0r, int n, float fb_threshold, float* dist,
                    uint8_t* valid);

/* ---- detector: replaces cv2.goodFeaturesToTrack(frame_gray, mask=mask, **feature_params) s1:437 */
/* Mask (s1:285-294) is uploaded once and reused; NULL clears it. */
int icelk_set_mask(icelk_t* h, const uint8_t* host_mask, int w, int h_, int stride);
/* The mask of s1:285-291 built on the device from the digitised water polygon: poly_xy = n (x, y) pairs on the
 * UNCROPPED photo (`maskpoly`, camtools.py:165); the polygon is shifted by the crop offsets and every pixel centre of
 * the w x h_ frame is tested as Camera.mask_meshgrid does (camtools.py:184-211, matplotlib's contains_points rule,
 * radius 0); inside = 255.  n <= 65536. */
int icelk_set_mask_polygon(icelk_t* h, const double* poly_xy, int n, double crop_left, double crop_top, int w, int h_);
/* Copy the current mask to the host (parity / inspection). */
int icelk_download_mask(icelk_t* h, uint8_t* host_mask, int stride, int* w, int* h_);
/* cornerMinEigenVal map of the slot (debug / parity). */
int icelk_min_eig_map(icelk_t* h, int slot, int block_size, float* host_out, int stride_elems);
/* Which corner response the detector ranks by: cv2.goodFeaturesToTrack's useHarrisDetector / k.
 *   ICELK_DETECTOR_MIN_EIG  the smaller eigenvalue of the blockSize x blockSize covariance sums (Shi-Tomasi; the default; k is
 *                           ignored and kept as given)
 *   ICELK_DETECTOR_HARRIS   det - k tr^2 of the same sums a = S dx^2, b = S dx dy, c = S dy^2, which are NOT halved as
 *                           calcMinEigenVal halves them.  Default form, calcHarris' float lanes: every operation rounded to
 *                           float32, nothing fused,  t = a + c;  R = (a c - b b) - (kf t) t,  kf = (float)k.  The build-dependent
 *                           alternative is icelk_set_variant "harris_tail" 1.  Both forms are written from knowledge of upstream
 *                           OpenCV; as for the rest of the detector, parity with OpenCV is unpinned, a numpy
 *                           restatement (tests/harris_restatement.py) pins them.
 * The setting is snapshotted when a detection's candidate stage is enqueued (icelk_good_features, icelk_seg_detect, _begin,
 * _prepare): a detection in flight keeps the detector it was begun with, whatever is set afterwards, and _begin adopts
 * prepared candidates only if kind and k match too.  A map whose masked maximum is <= 0 yields no corner (with Harris a real
 * case: a pure ramp is negative everywhere).  The opt-in two-pass candidate kernel (ICELK_TWO_PASS_CORNERS) serves the smaller
 * eigenvalue only: with Harris selected the switch is ignored.  ICELK_EARG for an unknown kind or a non-finite k, before any
 * GPU work. */
#define ICELK_DETECTOR_MIN_EIG 0
#define ICELK_DETECTOR_HARRIS 1
int icelk_set_detector(icelk_t* h, int kind, double k);
int icelk_get_detector(icelk_t* h, int* kind, double* k); /* either pointer may be NULL */
/* cv2.cornerHarris(src, blockSize, 3, k) of the slot: the twin of icelk_min_eig_map.  k is this call's own; the handle's
 * detector setting is neither read nor changed ("harris_tail" is read). */
int icelk_harris_map(icelk_t* h, int slot, int block_size, double k, float* host_out, int stride_elems);
/* Corners in response order (Shi-Tomasi, or Harris under icelk_set_detector).  max_corners <= 0 = unlimited (up to max_pts).
 * *out_n == 0 corresponds to cv2 returning None (guarded at s1:445). */
int icelk_good_features(icelk_t* h, int slot, int use_mask, int max_corners, double quality_level,
                        double min_distance, int block_size, float* out_xy, int cap, int* out_n);

/* Work counters of the latest detection on this handle: local maxima above the quality threshold, and
 * corners surviving the minDistance rule (before the maxCorners cut). */
int icelk_detect_stats(icelk_t* h, int* n_candidates, int* n_accepted);
/* Work counters of the two-pass candidate stage of the latest detection on a frame_w x frame_h frame (diagnostics; waits
 * for the device): out[0] tiles, [1] pixels listed as possible local maxima, [2] tiles whose list overflowed, [3] entries
 * handed to the 3x3 tie pass, [4] pixels listed as possible carriers of the maximum, [5] tiles whose such list overflowed,
 * [6] longest tile list, [7] listed pixels that got their exact value in the one-pixel pass (certain, above the cut). */
int icelk_detect_fast_stats(icelk_t* h, int frame_w, int frame_h, long long* out);
/* The masked maximum of the response map (eigenvalue or Harris) as the candidate stage of the latest detection (or icelk_min_eig_map / icelk_harris_map) on this
 * handle published it: the order-preserving key of the float (sign set: ~bits, else bits | 0x80000000), 0 if no pixel
 * counted (diagnostics and tests; waits for the device). */
int icelk_detect_max_key(icelk_t* h, unsigned* out_key);

/* ---- device-resident segment state: the `tracks` / `trackquality` lists of s1:299-300,335-359 --
 * A segment starts at a detection frame (counter % track_len == 0, s1:362,437-448) and is extended
 * by one vertex per tracked frame; only tracks passing the forward-backward test survive, in order.
 * Nothing crosses PCIe until icelk_seg_read. */
int icelk_seg_detect(icelk_t* h, int slot, int use_mask, int max_corners, double quality_level,
                     double min_distance, int block_size, int* out_n);
/* The same detection split in two, for pipelined loops: _begin enqueues the detector on the handle's
 * detection stream (it needs the frame only, so it overlaps a tracker launch issued after it) and returns
 * at once; _finish waits for it and starts the new segment.  TWO detections may be in flight (a third _begin returns
 * ICELK_ESTATE); _finish / _stage take them in the order they were begun and wait for the kernels of that one only.
 * Beginning the detection of frame d+2 before staging the one of frame d lets the host round trip of a detection find
 * kernels that had a whole tracker launch to finish, instead of standing in a serial loop with them.
 * _stage / _finish must be passed the max_corners their detection was begun with (ICELK_ESTATE otherwise): the cut has
 * been made on the device by then.  A _stage / _finish that fails drops its detection; one begun after it is still in
 * flight but can no longer be staged, so icelk_seg_detect_cancel comes next. */
int icelk_seg_detect_begin(icelk_t* h, int slot, int use_mask, int max_corners, double quality_level,
                           double min_distance, int block_size);
int icelk_seg_detect_finish(icelk_t* h, int max_corners, int* out_n);
/* Abandon everything that was started ahead and never used: detections begun but not finished (up to two), prepared
 * candidates, a staged segment that was never switched to.  Waits for their kernels, then forgets them; the current
 * segment and every slot stay as they are.  For a loop that announced frames ahead (look-ahead) and ends, or jumps,
 * before they arrive: afterwards the one-call forms (icelk_good_features, icelk_seg_detect) work again. */
int icelk_seg_detect_cancel(icelk_t* h);
/* _finish in two halves, for loops that know their frames some steps ahead: _stage waits for the OLDEST detection in
 * flight and builds the new segment in the handle's next set of segment buffers (six rotate) while the current segment
 * is still being tracked; icelk_seg_switch (no GPU work, no wait) makes the staged segment the current one.  One
 * segment can be staged at a time.  With the detection of frame c begun at step c-4 and staged at step c-2 (behind the
 * _switch of that step), the one host round trip of a detection is off the critical path: the tracker launch of
 * frame c finds its segment ready.  _finish == _stage followed by _switch. */
int icelk_seg_detect_stage(icelk_t* h, int max_corners, int* out_n);
/* _stage that never waits: *out_done = 0 (and nothing done) while the kernels of the oldest detection in flight have
 * not delivered their counts yet, else _stage (*out_done = 1).  A loop that looks ahead calls this at every step from
 * the first one at which the detection may be through, and the waiting form only when the segment is needed at the
 * next step: the host thread -- which also issues the uploads and the tracker launches -- then never stands behind the
 * detector's kernels (with the waiting form it stood there for a third of every period of the PCIe-fed loop). */
int icelk_seg_detect_stage_try(icelk_t* h, int max_corners, int* out_n, int* out_done);
int icelk_seg_switch(icelk_t* h);
/* Optional, ahead of _begin: produce the corner candidates (min-eigenvalue map + non-max test, the part of
 * s1:437 that depends on nothing but the frame and blockSize) of a frame that is already in `slot`, on a stream of
 * its own and into a spare buffer (three exist: two detections in flight + one prepared), while earlier detections are
 * still in their min-distance stage.  A later _begin for the same slot/frame/blockSize/mask/detector adopts the result;
 * otherwise it is dropped.  Results are identical either way. */
int icelk_seg_detect_prepare(icelk_t* h, int slot, int use_mask, int block_size);
int icelk_seg_track(icelk_t* h, int slot_prev, int slot_next, int win_w, int win_h, int max_level,
                    int crit_type, int max_count, double epsilon, double min_eig_threshold,
                    float fb_threshold, int* out_live);
/* tracks: (n, n_vertices, 2) float32; quality: (n, n_vertices-1) float32 -- the arrays np.savez
 * writes at s1:394-395.  cap = rows available in the host buffers, max_vertices = their vertex
 * dimension. */
int icelk_seg_read(icelk_t* h, float* tracks, float* quality, int cap, int max_vertices, int* out_n,
                   int* out_vertices);
/* The same gather into DEVICE memory of the caller (e.g. one slice of a torch tensor that is all-gathered over RCCL at
 * the end of a sharded run, BASELINE.json configs[3]): rows of the surviving tracks, packed, (n, n_vertices, 2) float32
 * at dev_tracks, (n, n_vertices-1) at dev_quality (may be NULL), n as one int32 at dev_count.  cap_rows = rows the
 * buffers hold, must be >= the tracks the segment started with.  Enqueued on the handle's compute stream: no wait, no
 * host read-back. */
int icelk_seg_archive(icelk_t* h, void* dev_tracks, void* dev_quality, void* dev_count, int cap_rows, int* out_vertices);
/* The LAST pair of a segment and the FIRST pair of the next one are independent (s1:362 tracks the old features across
 * (c-1, c), s1:440 starts the new segment from the corners of frame c, tracked across (c, c+1) one loop pass later).
 * icelk_seg_track_defer takes the arguments of icelk_seg_track_async but launches nothing: the pair waits, and the next
 * icelk_seg_track_async / _defer after icelk_seg_switch sends both pairs to the device as ONE tracker launch (ramp-up
 * and tail of the launch are paid once; every workgroup still tracks one feature exactly as before).  The waiting pair
 * goes out on its own whenever its result or its frames are needed first: icelk_seg_flush, icelk_sync, a read-out of
 * its segment, a second switch, or an ingest / icelk_drop_pyramid into one of its two slots; also when the partner's
 * LK parameters differ.  Results are those of icelk_seg_track_async in every case.
 * After icelk_seg_switch the segment it closed stays addressable until the switch after: the _closed forms of the
 * read-outs gather from it (and launch its waiting pair first if it still waits). */
int icelk_seg_track_defer(icelk_t* h, int slot_prev, int slot_next, int win_w, int win_h, int max_level,
                          int crit_type, int max_count, double epsilon, double min_eig_threshold,
                          float fb_threshold);
int icelk_seg_flush(icelk_t* h);
/* Pairs per segment of the loop that drives this handle (`track_len` of s1_lucaskanade_tracking.py:128,362); 0 = unknown
 * (the default).  A hint, results never depend on it: the backward pass of pair v of a segment builds, level by level,
 * exactly the templates (patch, derivatives, 2x2 matrix) that the forward pass of pair v+1 builds again -- frame v+1 at
 * the positions the tracks have reached -- so the window-specialised kernels leave them in HBM for the next launch
 * instead.  With the hint the LAST pair of a segment does not write templates nobody will read.
 * ICELK_NO_TEMPLATE_REUSE=1 turns the reuse off altogether (A/B). */
int icelk_seg_track_len_hint(icelk_t* h, int track_len);
/* out[0] = segment pairs of this handle whose forward pass took its templates from the pair before, out[1] = pairs whose
 * backward pass left templates for a successor (diagnostics; tests/test_gpu_api.py uses it to see the reuse engage and
 * refuse: a pair whose first frame is not the frame the templates were built on builds its own). */
int icelk_seg_template_stats(icelk_t* h, long long* out);
/* The template tables behind icelk_seg_track_len_hint: bytes of ONE of the two tables, the tracks (rows) it has room for,
 * and state 0 = in use (or not needed yet), 1 = switched off (ICELK_NO_TEMPLATE_REUSE), 2 = off because the allocation
 * failed.  They are allocated once per row geometry (window, pyramid levels) at the first pair that can use them, for
 * max_pts rows within ICELK_TEMPLATE_BUDGET_MB (default 8192 for both tables; at most half of the free device memory); a
 * segment with more tracks than rows builds its own templates. */
int icelk_seg_template_info(icelk_t* h, long long* bytes_per_table, long long* rows, int* state);
/* out[0] = segments whose tables were written by the device-driven tail of their detection (k_tail.hip: sort, maxCorners
 * cut, corner list = the reset `tracks = [[(x, y)] ...]` of s1:440-448, launch order -- all from the device-side counts,
 * enqueued by icelk_seg_detect_begin; icelk_seg_detect_stage only adopts the verdict), out[1] = segments staged by the
 * host's tail (min-distance relaxation not converged, a pruned candidate set that fell short of maxCorners,
 * minDistance < 1, or ICELK_HOST_TAIL=1).  Results are the same either way. */
int icelk_seg_tail_stats(icelk_t* h, long long* out);
int icelk_seg_read_closed(icelk_t* h, float* tracks, float* quality, int cap, int max_vertices, int* out_n,
                          int* out_vertices);
int icelk_seg_archive_closed(icelk_t* h, void* dev_tracks, void* dev_quality, void* dev_count, int cap_rows,
                             int* out_vertices);
/* non-blocking variants for pipelined loops: no host read-back, counts stay on the device */
int icelk_seg_track_async(icelk_t* h, int slot_prev, int slot_next, int win_w, int win_h, int max_level,
                          int crit_type, int max_count, double epsilon, double min_eig_threshold,
                          float fb_threshold);
int icelk_seg_live(icelk_t* h, int* out_live, int64_t* out_tracked_total);

/* ---- projection of finished tracks to map coordinates + plausibility filter (the consumer of the path) --
 * Replaces the per-track Python loops of s2_cam_to_utm.py:243-347: every vertex is moved to uncropped photo
 * coordinates (imports/camtools.py:414-421) and projected onto the sea-level plane (Camera.photo_to_utm,
 * imports/camtools.py:286-332); u, v [m/s] = vertex difference / interval, speed = hypot(u, v); a track is
 * dropped when mean(speed) < min_speed or max(speed) > max_speed, or -- if max(speed) > speed_threshold -- when
 * consecutive vectors differ by more than max_speedfactor in speed or max_angle degrees in direction.
 * float64 throughout, the reference's operation order.  X, U, V are the direction cosines of
 * camtools.py:300-316, formed by the caller (utm.py does it with numpy, as the reference does). */
typedef struct icelk_camera {
    double X[3], U[3], V[3];
    double sigma;              /* image_width / sensor_width * sigma   (camtools.py:145) */
    double H, E, N;            /* camera height above the water (tide corrected), easting, northing */
    double half_w, half_h;     /* pic['width'] / 2.0, pic['height'] / 2.0 of the UNCROPPED photo */
    double crop_left, crop_top;
} icelk_camera_t;
typedef struct icelk_utm_filter {
    double interval_s;         /* seconds between consecutive vertices (the `_at_{dt}sec_` of the file name) */
    double max_speed, min_speed, max_speedfactor, max_angle, speed_threshold;   /* s2_cam_to_utm.py:84-88 */
} icelk_utm_filter_t;
/* tracks: host (n, n_vertices, 2) float32, the `tracks` array of one .npz (s1:394-395).  x, y, u, v, speed: host
 * (n, n_vertices-1) float64, x/y = map position of each vector's FIRST vertex (s2:296-297).  keep: n bytes --
 * 1 kept, 0 dropped, 2 = the reference raises ValueError on this track (max() of an empty list: fewer than two
 * vectors and faster than speed_threshold).  n <= max_pts, n_vertices <= 17. */
int icelk_project_tracks(icelk_t* h, const float* tracks, int n, int n_vertices, const icelk_camera_t* cam,
                         const icelk_utm_filter_t* filt, double* x, double* y, double* u, double* v, double* speed,
                         uint8_t* keep);
/* The same for the segment held on the device (icelk_seg_*): gather of the surviving tracks + projection, only
 * results cross PCIe.  cap = rows of the host buffers, max_vectors = their second dimension. */
int icelk_seg_project(icelk_t* h, const icelk_camera_t* cam, const icelk_utm_filter_t* filt, int cap, int max_vectors,
                      double* x, double* y, double* u, double* v, double* speed, uint8_t* keep, int* out_n,
                      int* out_vectors);

/* ---- gridding of the projected velocities (s3_utm_to_gridded_utm.py:391-421) --------------------------------
 * matplotlib.path.Path(poly).contains_points(points) with radius 0 (the rule of icelk_set_mask_polygon) for arbitrary
 * float64 points: used for "does the fjord outline contain the cell centre" (imports/tracking_misc.py:49). */
int icelk_points_in_polygon(icelk_t* h, const double* poly_xy, int n_poly, const double* pts_xy, int n_pts,
                            uint8_t* inside);
/* Square cells of `spacing` from (left, top), cols x rows, cell (i, j) = column i, row j downwards, stored at
 * i * rows + j as the reference walks them (tracking_misc.py:41-43); cell_on[] marks the cells the grid keeps.  For
 * every kept cell: count of the n velocities (x, y, u, v; float64) whose position lies in it by contains_points'
 * rule, and for count > 0 mean_u = np.sum(u_sel) / count (numpy's pairwise order), mean_v, speed = hypot. */
int icelk_grid_bin(icelk_t* h, const double* x, const double* y, const double* u, const double* v, int n, double left,
                   double top, double spacing, int cols, int rows, const uint8_t* cell_on, int* count, double* mean_u,
                   double* mean_v, double* speed);
/* Every time window of a day in one pass (the loop of s3_utm_to_gridded_utm.py:286-421 around the binning above).
 * x, y, u, v, t (float64, n): the points of every loaded hour file, concatenated camera by camera, hour by hour.  File
 * f holds points [file_offset[f], file_offset[f + 1]) (file_offset[0] = 0, [nfiles] = n, non-decreasing) and comes
 * from camera file_cam[f] (0 .. ncam-1, non-decreasing).  Camera c's window w (slot c * nw + w) loads files
 * win_f0 .. win_f1 of that camera (none: win_f0 > win_f1) and keeps the points with t_lo <= t < t_hi (int64 epoch
 * seconds, compared as float64); per camera the windows must be ascending and disjoint (t_lo[w] <= t_hi[w] <=
 * t_lo[w + 1]).  A point is binned in the window that keeps its time if that window loads its file, else nowhere.
 * Out, per (window w, cell k) at w * cols * rows + k: count, mean_u, mean_v, speed -- for every window what
 * icelk_grid_bin gives on that window's points in concatenation order, bit for bit.  Per (window w, camera c) at
 * w * ncam + c: sel_count = points selected, t_min / t_max = their smallest / largest t (0 when none).
 * device_ms (may be NULL): HIP-event time of the kernels (assign, sort, reduce); uploads and read-backs excluded.
 * ICELK_ECAP when nw * cols * rows does not fit 31 bits, cols * rows > 2^24 or n > 2^30. */
int icelk_grid_bin_windows(icelk_t* h, const double* x, const double* y, const double* u, const double* v,
                           const double* t, int n, const int64_t* file_offset, const int* file_cam, const int* win_f0,
                           const int* win_f1, int nfiles, const int64_t* t_lo, const int64_t* t_hi, int ncam, int nw,
                           double left, double top, double spacing, int cols, int rows, const uint8_t* cell_on,
                           int* count, double* mean_u, double* mean_v, double* speed, int* sel_count, double* t_min,
                           double* t_max, double* device_ms);
/* Spread and robust centre per cell, beside the mean: the two calls above with six more outputs (host float64, laid
 * out as mean_u is: per cell, or per (window w, cell k) at w * cols * rows + k).  With u_sel a cell's velocities in
 * the order the mean adds them, bit for bit what numpy 2.2 answers:
 *   std_u    = np.std(u_sel, ddof=1): m = np.sum(u_sel) / n (the mean above), d = (u_sel - m) * (u_sel - m) with every
 *              operation rounded once, sqrt(np.sum(d) / (n - 1)), both sums in numpy's order; one point gives NaN;
 *   median_u = np.median(u_sel): NaN if a term is NaN; else with s the sorted terms (0.0 + s[n / 2]) / 1.0 for odd n,
 *              ((0.0 + s[n / 2 - 1]) + s[n / 2]) / 2.0 for even n -- so the median of [-0.0] is +0.0, of
 *              [1e308, 1e308] inf, of [-inf, inf] NaN;
 *   mad_u    = np.median(np.abs(u_sel - median_u)): the same median over fabs(u_sel - median_u), one rounding; a NaN
 *              or infinite median propagates by IEEE rules;
 * and std_v, median_v, mad_v likewise.  A cell without points has NaN in all six (the sign of a NaN is not numpy's
 * everywhere).  count, mean_u, mean_v, speed and the other outputs are those of the call without statistics, and
 * device_ms covers the kernels of the statistics too.  `stats` and its six members must not be null: ICELK_EARG,
 * checked with every other argument before anything is allocated or enqueued. */
typedef struct icelk_grid_stats {
    double *std_u, *std_v, *median_u, *median_v, *mad_u, *mad_v;
} icelk_grid_stats_t;
int icelk_grid_bin_stats(icelk_t* h, const double* x, const double* y, const double* u, const double* v, int n,
                         double left, double top, double spacing, int cols, int rows, const uint8_t* cell_on,
                         int* count, double* mean_u, double* mean_v, double* speed, const icelk_grid_stats_t* stats);
int icelk_grid_bin_windows_stats(icelk_t* h, const double* x, const double* y, const double* u, const double* v,
                                 const double* t, int n, const int64_t* file_offset, const int* file_cam,
                                 const int* win_f0, const int* win_f1, int nfiles, const int64_t* t_lo,
                                 const int64_t* t_hi, int ncam, int nw, double left, double top, double spacing,
                                 int cols, int rows, const uint8_t* cell_on, int* count, double* mean_u, double* mean_v,
                                 double* speed, int* sel_count, double* t_min, double* t_max, double* device_ms,
                                 const icelk_grid_stats_t* stats);
/* The three rules on the host, for one cell's n terms (n >= 0; a may be NULL when n == 0): the statement the kernels
 * are tested against.  No handle and no GPU.  ICELK_EARG for n < 0 or a null pointer. */
int icelk_grid_cell_stats_host(const double* a, int n, double* out_std, double* out_median, double* out_mad);

/* ---- binning into transect and mooring boxes (imports/tracking_misc.py:76-185) ---------------------------------
 * The same products as the gridder's -- count, mean_u, mean_v, speed and, asked for, the six statistics above -- for a
 * list of polygons that form no lattice: the rotated boxes along a transect or around a mooring.  Box b has the vertices
 * xy[2 * offset[b]] .. xy[2 * offset[b + 1]) as (x, y) pairs, tested as given by contains_points' rule; the boxes may
 * overlap and share edges, so a point counts in none, one or several of them.  A box's velocities are added in the
 * order of the points, as Path(poly).contains_points(points) selects them.
 * offset[0] = 0, ascending, three or more vertices per polygon, finite vertices: else ICELK_EARG.  nboxes in 1 .. 1024
 * and at most 2048 vertices in all: else ICELK_ECAP. */
typedef struct icelk_boxes {
    const double* xy;
    const int* offset; /* nboxes + 1 */
    int nboxes;
} icelk_boxes_t;
/* Host only, no handle and no GPU: ICELK_OK for a list the two calls below take, else what they would return for it. */
int icelk_boxes_check(const icelk_boxes_t* boxes);
/* One window.  rot: NULL, or {cos a, sin a} -- every point's velocity is then first turned into the frame of a transect of
 * azimuth a, u' = u cos + v sin (along), v' = v cos - u sin (across), each product and sum rounded once, and the outputs are
 * those of u', v'.  Out, per box: count, mean_u, mean_v, speed; stats may be NULL, else its six members are filled as
 * icelk_grid_bin_stats fills them (a null member: ICELK_EARG).  Every argument is checked before anything is allocated.
 * ICELK_ECAP also when n * nboxes does not fit 31 bits, n > 2^27, or -- seen after the boxes were tested -- the points lie
 * in more than 2 n + 1024 boxes altogether; the handle stays usable. */
int icelk_boxes_bin(icelk_t* h, const double* x, const double* y, const double* u, const double* v, int n,
                    const icelk_boxes_t* boxes, const double* rot, int* count, double* mean_u, double* mean_v,
                    double* speed, const icelk_grid_stats_t* stats);
/* The file and window tables of icelk_grid_bin_windows, under the same rules. */
typedef struct icelk_day_tables {
    const int64_t* file_offset; /* nfiles + 1 */
    const int* file_cam;        /* nfiles */
    const int* win_f0;          /* ncam * nw */
    const int* win_f1;
    int nfiles;
    const int64_t* t_lo; /* ncam * nw */
    const int64_t* t_hi;
    int ncam, nw;
} icelk_day_tables_t;
/* Every time window of a day in one pass: for window w what icelk_boxes_bin gives on the points icelk_grid_bin_windows
 * would select for it, bit for bit, per (window w, box b) at w * nboxes + b.  sel_count, t_min, t_max (per (window,
 * camera) at w * ncam + c) and device_ms (may be NULL) are that call's.  ICELK_ECAP when nw * nboxes or n * nboxes does
 * not fit 31 bits or n > 2^30, and for more than 2 n + 1024 keys as above. */
int icelk_boxes_bin_windows(icelk_t* h, const double* x, const double* y, const double* u, const double* v,
                            const double* t, int n, const icelk_day_tables_t* day, const icelk_boxes_t* boxes,
                            const double* rot, int* count, double* mean_u, double* mean_v, double* speed,
                            const icelk_grid_stats_t* stats, int* sel_count, double* t_min, double* t_max,
                            double* device_ms);

/* ---- averages of the run-wide velocity cube (s4_postprocess_gridded_utm.py:264-343) -------------------------
 * The stacked gridded windows of a run: u, v, count (host float64, NaN where a window has no entry for a cell), laid
 * out [window][cell] with cell = row * cols + col -- nt planes of ncells values.  icelk_cube_set uploads them; they
 * stay on the device, owned by the handle, until icelk_cube_release, the next icelk_cube_set or icelk_destroy.
 * ICELK_ECAP when ncells * nt does not fit 31 bits. */
int icelk_cube_set(icelk_t* h, const double* u, const double* v, const double* count, int ncells, int nt);
int icelk_cube_release(icelk_t* h);
/* Every averaging period of a request in one pass.  Period p selects the windows sel_index[sel_offset[p] ..
 * sel_offset[p + 1]) (offsets from 0, non-decreasing; indices in [0, nt), ascending for the reference's order).  Per
 * period and cell: np.nanmean of u and of v and np.nansum of count over the selected windows, as numpy computes them
 * on cube[:, :, mask] (windows added one after the other; NaN where none holds a value); with coarseness > 1 then the
 * reference's spatial_mean(..., nanmean = 0) of the three fields (zero padding to a multiple of coarseness, divisor
 * coarseness^2, NaN propagates, numpy's order of additions).  rows * cols must be the cube's ncells.
 * Out (host), per period p at p * out_cells + k with out_cells = ceil(rows / coarseness) * ceil(cols / coarseness):
 * out_u, out_v, out_count, and out_speed = np.hypot(out_u, out_v); out_has_data[p] = 1 iff some cell of the period's
 * uncoarsened fields has a non-NaN speed (the reference's "no data available" test).  device_ms (may be NULL):
 * HIP-event time of the kernels; uploads and read-backs excluded.  Arguments are checked before anything is issued;
 * ICELK_ESTATE without a cube, ICELK_ECAP when nperiods * ncells does not fit 31 bits or coarseness > 8193 (the largest
 * checked against numpy: the project answers as numpy does or refuses). */
int icelk_cube_average(icelk_t* h, const int* sel_offset, const int* sel_index, int nperiods, int rows, int cols,
                       int coarseness, double* out_u, double* out_v, double* out_speed, double* out_count,
                       int* out_has_data, double* device_ms);

/* ---- camera calibration: the shoreline misfit (s0_2_camera_calibration.py:117-152, 231-275) -------------------
 * The scene: M shoreline points digitised on a photo, as (xi, yi) = (x - width / 2, y - height / 2) pairs, the W
 * vertices of the waterline on the map as (x, y) pairs (finite, or ICELK_EARG), and the camera position E, N.
 * icelk_calib_set uploads it; it stays on the device, owned by the handle, until icelk_calib_release, the next
 * icelk_calib_set or icelk_destroy.  ICELK_EARG for M < 1, W < 1 or null pointers. */
int icelk_calib_set(icelk_t* h, const double* shore_xy, int M, const double* water_xy, int W, double E, double N);
int icelk_calib_release(icelk_t* h);
/* P candidates of 11 doubles each: X[3], U[3], V[3] (the direction vectors of photo_to_utm, s0_2:124-136), sigma
 * scaled to pixels, H.  Per candidate p and point m, at p * M + m: out_dist = the distance from the projected point
 * (tx, ty) of s0_2:146-150 to the nearest waterline vertex, bit for bit what optimizefun_calibration returns (NaN
 * where tx or ty is NaN, inf where one is infinite); out_tx, out_ty (each may be NULL): the projected point.
 * device_ms (may be NULL): HIP-event time of the kernel; uploads and read-backs excluded.  Arguments are checked
 * before anything is issued; ICELK_ESTATE without a scene, ICELK_ECAP when P * M does not fit 31 bits. */
int icelk_calib_residuals(icelk_t* h, const double* cand, int P, double* out_dist, double* out_tx, double* out_ty,
                          double* device_ms);
/* The same without the (P, M) output: out_meansq[p] = np.mean(residuals[p] ** 2), the squares added in numpy's
 * pairwise order.  Also ICELK_ECAP for a scene of more than 4096 shoreline points. */
int icelk_calib_cost(icelk_t* h, const double* cand, int P, double* out_meansq, double* device_ms);

/* ---- JPEG ingest: the host reads the entropy-coded stream, the device does the rest ------------- */
/* What a baseline JPEG file says about itself, and how its quantised DCT coefficients are laid out in memory.
 * Coefficients are int16, component after component (coef_offset[c], in int16 units); inside a component the 8x8 blocks
 * stand in raster order over the MCU-padded block grid (blocks_x[c] x blocks_y[c]), 64 values per block in natural
 * (row-major, de-zigzagged) order, not yet multiplied by the quantisation table.  quant[c] is the table of component c
 * in the same natural order.  comp_w / comp_h are the true plane sizes ceil(width * h / hmax), ceil(height * v / vmax):
 * chroma upsampling replicates the samples at THOSE edges.
 * Taken: SOF0, 8 bit, Huffman coded, one interleaved scan; 1 component, or 3 (YCbCr) with luma sampling 1x1, 2x1 or 2x2
 * and chroma 1x1; 8-bit DQT; DRI / RSTn; APPn / COM skipped; width >= 3.  Everything else that is a valid file is
 * ICELK_EUNSUP (progressive, arithmetic, 12 bit, 4 components, other sampling factors, several scans, DNL, an Adobe
 * marker with transform != 1, component ids R G B); a stream that breaks off or contradicts itself is ICELK_EARG. */
typedef struct icelk_jpeg_info {
    int32_t width, height, ncomp;
    int32_t hmax, vmax;          /* sampling factors of component 0; the others are 1 x 1 */
    int32_t mcus_x, mcus_y;
    int32_t restart_interval;    /* MCUs between RSTn markers, 0: none */
    int32_t comp_w[3], comp_h[3];
    int32_t blocks_x[3], blocks_y[3];
    uint64_t coef_offset[3];
    uint64_t coef_count;         /* int16 values in all: what icelk_jpeg_read_coefficients writes */
    uint16_t quant[3][64];
} icelk_jpeg_info_t;
/* Host only, no handle, re-entrant (callable from several threads at once, without a GPU): the headers of the file
 * in data[0 .. len). */
int icelk_jpeg_describe(const uint8_t* data, uint64_t len, icelk_jpeg_info_t* info);
/* Host only, no handle, re-entrant: Huffman-decodes the file's scan into coef[0 .. info.coef_count); capacity = int16
 * values coef has room for (ICELK_ECAP when too few).  No byte outside data[0 .. len) is read; a truncated or malformed
 * stream gives ICELK_EARG.  coef may be pinned memory of icelk_host_alloc. */
int icelk_jpeg_read_coefficients(const uint8_t* data, uint64_t len, int16_t* coef, uint64_t capacity);
/* Coefficients -> gray frame in `slot`, exactly what icelk_upload_bgr leaves there when given the file's decoded RGB
 * pixels (libjpeg's integer inverse DCT, "fancy" chroma upsampling and YCbCr -> RGB, bit for bit) with crop_* pixels cut
 * off at the four sides: dequantisation, inverse DCT, upsampling, colour conversion, crop and gray run on the device, RGB
 * is never stored.  The cropped size must fit max_w x max_h of icelk_create, the file itself need not.  Only the blocks
 * the crop needs are transformed.  3-component files only (as icelk_upload_bgr takes 3-channel images only). */
int icelk_upload_jpeg(icelk_t* h, int slot, const icelk_jpeg_info_t* info, const int16_t* coef, int gray_variant,
                      int crop_left, int crop_top, int crop_right, int crop_bottom);
/* Coefficients -> the decoded image on the host: interleaved R G B (3 * width bytes per row) for 3 components, the
 * single plane (width bytes per row) for 1; stride in bytes. */
int icelk_jpeg_decode_rgb(icelk_t* h, const icelk_jpeg_info_t* info, const int16_t* coef, uint8_t* out, int stride);

/* ---- Huffman decoding on the device (opt-in) ----------------------------------------------------
 * The entropy-coded data is cut into subsequences of subseq_bits raw bits, one decoder lane each; lanes that start
 * out of step fall into step with the true decoder by iterating to a fixed point (self-synchronisation), then every
 * lane writes the coefficients of its own stretch.  The result equals icelk_jpeg_read_coefficients element for element,
 * for the same set of files.  The work is bounded: a chain of more than max_hops subsequences in one round, or more than
 * max_rounds rounds, and the file is decoded by icelk_jpeg_read_coefficients inside the same call; so is a file whose
 * stream contradicts itself, and then that decoder's verdict (ICELK_EARG, or its coefficients) is the call's. */
#define ICELK_JPEG_TABLE_BYTES 11328      /* 4 DC + 4 AC tables as the lanes read them */
#define ICELK_JPEG_FALLBACK_NONE 0
#define ICELK_JPEG_FALLBACK_BOUND 1       /* the fixed point was not reached within max_hops / max_rounds */
#define ICELK_JPEG_FALLBACK_STREAM 2      /* the stream contradicts itself: the serial decoder had the last word */
#define ICELK_JPEG_FALLBACK_SIZE 3        /* a file of 256 MiB or more */
typedef struct icelk_jpeg_scan {
    uint32_t segments;                    /* entropy-coded segments: 1, or the restart intervals */
    uint32_t blocks_per_mcu, blocks_per_segment /* 0: one segment */, total_blocks;
    uint8_t component[8], dc_table[8], ac_table[8];   /* of every block of an MCU */
} icelk_jpeg_scan_t;
typedef struct icelk_jpeg_huff_stats {
    uint32_t segments, subsequences;
    uint32_t rounds;                      /* rounds that changed an entry state, the first one included */
    uint32_t max_hops;                    /* most entry states one chain overwrote in one round */
    uint32_t lanes_in_step;               /* lanes whose starting guess was the true state */
    uint32_t spanning_blocks;             /* blocks that begin in one subsequence and end in another */
    uint32_t fallback;                    /* ICELK_JPEG_FALLBACK_* */
    uint32_t reserved;
    uint64_t total_hops;
} icelk_jpeg_huff_stats_t;
/* Host only, no handle, re-entrant: headers as icelk_jpeg_describe, then the entropy-coded segments (found with memchr):
 * seg_begin[s] .. seg_end[s] are the bytes of segment s; the RSTn markers between them must count D0 .. D7 cyclically and
 * be ceil(MCUs / restart interval) - 1 in number (ICELK_EARG otherwise).  seg_begin / seg_end may be NULL (scan->segments
 * says how many there are; ICELK_ECAP when seg_capacity is too small); tables: NULL or ICELK_JPEG_TABLE_BYTES bytes. */
int icelk_jpeg_index(const uint8_t* data, uint64_t len, icelk_jpeg_info_t* info, icelk_jpeg_scan_t* scan, uint32_t* seg_begin,
                     uint32_t* seg_end, uint64_t seg_capacity, void* tables);
/* Host only, no handle, re-entrant: icelk_jpeg_read_coefficients by the lanes' algorithm, the same code as the device
 * runs, phase by phase and lane by lane on the CPU.  subseq_bits: a multiple of 32; stats may be NULL. */
int icelk_jpeg_read_coefficients_lanes(const uint8_t* data, uint64_t len, int16_t* coef, uint64_t capacity, int subseq_bits,
                                       int max_hops, int max_rounds, icelk_jpeg_huff_stats_t* stats);
/* subseq_bits: a multiple of 32, >= 32; max_hops >= 1; 1 <= max_rounds <= 255.  Defaults: 512, 256, 8 (DESIGN.md 7.2 says why). */
int icelk_jpeg_huff_config(icelk_t* h, int subseq_bits, int max_hops, int max_rounds);
/* of the file the handle decoded last */
int icelk_jpeg_huff_stats(icelk_t* h, icelk_jpeg_huff_stats_t* stats);
/* icelk_upload_jpeg from the file's bytes: the coefficients are decoded on the device and never visit the host. */
int icelk_upload_jpeg_file(icelk_t* h, int slot, const uint8_t* data, uint64_t len, int gray_variant, int crop_left, int crop_top,
                           int crop_right, int crop_bottom);
/* ---- icelk_upload_jpeg_file ahead of the frame (opt-in) ----
 * Starts the decoding of a file into `slot` and returns without waiting: the host's share is done in the call (the
 * file's index, the checks of descriptor, crop and slot -- their errors are returned here, with the codes of
 * icelk_upload_jpeg_file), the bytes are copied into pinned memory of the library (the caller's buffer is free on return)
 * and every device phase, the verdict on the file included, is enqueued on a decode stream that is not the compute stream,
 * behind the launches that still read the slot.  The file owns a working set of its own until icelk_jpeg_async_finish
 * (at 12 MP: ~36 MB of coefficients, 18 MB of planes and the file; the sets are kept and reused).  Between this call
 * and a finish that returns ICELK_OK the slot holds NO frame the caller may use -- unless icelk_jpeg_async_poll says 1.
 * ICELK_ESTATE when the slot's previous file has not been finished; every other upload call into such a slot fails the
 * same way. */
int icelk_upload_jpeg_file_async(icelk_t* h, int slot, const uint8_t* data, uint64_t len, int gray_variant, int crop_left,
                                 int crop_top, int crop_right, int crop_bottom);
/* Never blocks, no runtime call: *state = 0 the file is in flight, 1 it is decoded (the slot's frame may be used by calls
 * of this handle: they wait for it on the device), 2 the host decoder has to take it (icelk_jpeg_async_finish does).
 * After finish the slot keeps answering what its last file ended as.  ICELK_ESTATE for a slot that never had a file. */
int icelk_jpeg_async_poll(icelk_t* h, int slot, int* state);
/* Waits for the verdict on the slot's file.  Decoded: ICELK_OK and, if stats is not NULL, the statistics of THIS file
 * (icelk_jpeg_huff_stats keeps reporting the latest synchronous file).  Work bound hit, not settled or a stream that
 * contradicts itself: the host decoder reads the library's copy of the bytes, its coefficients are transformed into the
 * slot, stats->fallback names the reason and the host decoder's verdict is the call's, as in icelk_upload_jpeg_file.
 * After ICELK_OK the slot is as icelk_upload_gray_async leaves it; after an error it holds no frame and any upload call
 * may fill it.  Either way the file's working set is free again.  ICELK_ESTATE without a file in flight. */
int icelk_jpeg_async_finish(icelk_t* h, int slot, icelk_jpeg_huff_stats_t* stats_or_null);
/* icelk_jpeg_decode_rgb from the file's bytes. */
int icelk_jpeg_decode_rgb_file(icelk_t* h, const uint8_t* data, uint64_t len, uint8_t* out, int stride);
/* The coefficients as the device decodes them, copied back (for tests): coef[0 .. info.coef_count). */
int icelk_jpeg_device_coefficients(icelk_t* h, const uint8_t* data, uint64_t len, int16_t* coef, uint64_t capacity);

/* ---- the reference's lossy re-save of the crop (opt-in) -----------------------------------------
 * The reference never tracks on the pixels of the photos it is given: every photo is cropped with Pillow and written back
 * with `img_crop.save(outpath)` (s1:272, camtools.py:64-104) -- a new baseline JPEG at Pillow's defaults (quality 75, 4:2:0
 * chroma, libjpeg's standard tables) -- and the loop decodes THOSE files.  The entropy coder is lossless, so the pixels of
 * "save, then open" are a function of the cropped R G B alone: colour conversion, padding and 2x2 downsampling, libjpeg's
 * integer forward DCT and quantisation (csrc/jpeg_fwd.h; on the device k_jpeg_fwd.hip), then the decoder of the section
 * above on those coefficients.  No file is written.  Everything equals Pillow (libjpeg) bit for bit; nothing below changes
 * what the calls above do.  quality: 1 .. 100, Pillow's `quality=` (its default, the reference's, is 75). */
/* Host only, no handle, re-entrant: the two quantisation tables of that file (the Annex K tables scaled by libjpeg's
 * rule), 64 entries each in natural order. */
int icelk_jpeg_resave_tables(int quality, uint16_t* luma, uint16_t* chroma);
/* Host only, no handle, re-entrant: the quantised coefficients of the file Pillow would write for the w x h_ image at rgb
 * (interleaved R G B, stride in bytes), and in *info what icelk_jpeg_describe would say about that file -- so that
 * icelk_upload_jpeg / icelk_jpeg_decode_rgb take them as they take a file's.  The same code as the device runs, on the
 * CPU.  coef may be NULL (the descriptor only); capacity in int16 values (ICELK_ECAP when too few).  The dummy blocks of
 * the MCU-padded grid are written as the encoder writes them (AC 0, DC of the block before), so that whole planes compare. */
int icelk_jpeg_resave_coefficients_host(const uint8_t* rgb, int w, int h_, int stride, int quality, icelk_jpeg_info_t* info,
                                        int16_t* coef, uint64_t capacity);
/* Host only: out[i] = (first + i) / (8 q), truncating, by the multiply-shift the quantiser uses on the host and on the
 * device (for tests: it is exact for every numerator up to 2^17, far beyond what the transform of 8-bit samples gives). */
int icelk_jpeg_resave_divide_host(int q, uint32_t first, uint32_t count, uint32_t* out);
/* R G B in, the R G B of the re-saved image out (both on the host, strides in bytes), computed on the device.
 * w >= 3, as for the decoder. */
int icelk_jpeg_resave_rgb(icelk_t* h, const uint8_t* rgb, int w, int h_, int stride, int quality, uint8_t* out, int out_stride);
/* The coefficients as the device's forward kernel makes them, copied back (for tests): the layout of
 * icelk_jpeg_resave_coefficients_host. */
int icelk_jpeg_resave_device_coefficients(icelk_t* h, const uint8_t* rgb, int w, int h_, int stride, int quality, int16_t* coef,
                                          uint64_t capacity);
/* icelk_upload_bgr, icelk_upload_jpeg and icelk_upload_jpeg_file with the re-save between the crop and the gray
 * conversion: the slot holds what icelk_upload_bgr leaves there when given the pixels of Image.open(re-saved crop).  The
 * arguments are the parents' plus quality.  The cropped R G B is made on the device (or copied there), re-saved by the
 * forward kernel and decoded by the kernels of the section above with the re-save's tables.  Checked before anything is
 * enqueued: quality 1 .. 100, cropped width >= 3, the sizes as in the parents.  Scratch buffers are allocated at first
 * use and freed with the handle.  The look-ahead form is icelk_upload_jpeg_file_async_resave, below the crop job. */
/* The coefficients as the fused crop-and-forward kernel makes them from a file's decoded planes, copied back (for tests):
 * the file is decoded on the device as by icelk_upload_jpeg_file, its crop box goes through k_jpeg_crop_fwd, and coef gets
 * the re-saved file's coefficients in the layout of icelk_jpeg_resave_coefficients_host for the cropped size.  No slot. */
int icelk_jpeg_crop_fwd_device_coefficients(icelk_t* h, const uint8_t* data, uint64_t len, int crop_left, int crop_top, int crop_right,
                                            int crop_bottom, int quality, int16_t* coef, uint64_t capacity);
int icelk_upload_bgr_resave(icelk_t* h, int slot, const uint8_t* host, int w, int h_, int stride, int gray_variant, int quality);
int icelk_upload_jpeg_resave(icelk_t* h, int slot, const icelk_jpeg_info_t* info, const int16_t* coef, int gray_variant,
                             int crop_left, int crop_top, int crop_right, int crop_bottom, int quality);
int icelk_upload_jpeg_file_resave(icelk_t* h, int slot, const uint8_t* data, uint64_t len, int gray_variant, int crop_left,
                                  int crop_top, int crop_right, int crop_bottom, int quality);

/* ---- the re-saved crop as a file (opt-in) --------------------------------------------------------
 * The bytes `img.save(path)` writes (Pillow, libjpeg at its defaults: baseline, the Huffman tables of T.81 Annex K.3, no
 * restart intervals) are a function of the quantised coefficients: SOI, APP0 (JFIF 1.01, density 1 : 1 without a unit,
 * whatever the source said: `crop().save()` carries neither dpi nor Exif over), one COM segment if a comment is given
 * (comment != NULL; Pillow carries the source's last one over), one DQT segment per table slot, SOF0, one DHT segment per
 * table in the order DC0, AC0, DC1, AC1, SOS, the scan with a 00 behind every FF and its last byte filled with 1-bits, EOI.
 * Descriptors: laid out as icelk_jpeg_describe lays a file out; 1 component, or 3 with luma 1x1, 2x1 or 2x2; table slot 0
 * is quant[0], slot 1 is quant[1], which quant[2] must equal (else ICELK_EUNSUP); restart_interval != 0 is ICELK_EUNSUP.
 * A DC difference beyond +-2047 or an AC value beyond +-1023 has no code in those tables: ICELK_EARG, nothing is written.
 * ICELK_ECAP: `out` is too small (or NULL) and *len says what the file takes -- or the scan has so many blocks that
 * blocks * 1660 bits do not fit the 32 bits that bit offsets are carried in (2.58 million blocks; 12 MP have 281 000). */
/* Host only, no handle, re-entrant: SOI up to the end of the SOS segment. */
int icelk_jpeg_encode_header(const icelk_jpeg_info_t* info, const uint8_t* comment, uint64_t comment_len, uint8_t* out,
                             uint64_t capacity, uint64_t* len);
/* Host only, no handle, re-entrant: the whole file, the scan walked serially (csrc/jpeg_enc.h, the code of the device). */
int icelk_jpeg_encode_coefficients_host(const icelk_jpeg_info_t* info, const int16_t* coef, const uint8_t* comment,
                                        uint64_t comment_len, uint8_t* out, uint64_t capacity, uint64_t* len);
/* Host only: icelk_jpeg_resave_coefficients_host, then the call above -- what Image.fromarray(rgb).save(f, "JPEG",
 * quality=quality) writes. */
int icelk_jpeg_resave_file_host(const uint8_t* rgb, int w, int h_, int stride, int quality, const uint8_t* comment,
                                uint64_t comment_len, uint8_t* out, uint64_t capacity, uint64_t* len);
/* icelk_jpeg_encode_coefficients_host on the device (csrc/k_jpeg_enc.hip): the coefficients are copied up and entropy-coded
 * there; the same bytes and the same error codes.  For tests, and for coefficients from icelk_jpeg_read_coefficients. */
int icelk_jpeg_encode_coefficients(icelk_t* h, const icelk_jpeg_info_t* info, const int16_t* coef, const uint8_t* comment,
                                   uint64_t comment_len, uint8_t* out, uint64_t capacity, uint64_t* len);
/* The file of the handle's most recent re-save -- the last call that ran the forward kernel: icelk_upload_bgr_resave,
 * icelk_upload_jpeg_resave, icelk_upload_jpeg_file_resave, icelk_jpeg_resave_rgb, icelk_jpeg_resave_device_coefficients --
 * coded straight from the coefficients that call left on the device.  No slot is touched.  ICELK_ESTATE: the handle has
 * never re-saved.  After ICELK_ECAP the call can be repeated with a larger buffer: the coded scan is kept until the next
 * re-save (or icelk_jpeg_encode_coefficients).  Buffers are allocated at first use and freed with the handle. */
int icelk_jpeg_resave_encode(icelk_t* h, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity,
                             uint64_t* len);

/* ---- the crop step on its own: decode, crop, re-save and encode with no host wait (opt-in) -------
 * The reference's crop_image_parallel (camtools.py:64-104, 237-258) writes a folder of re-saved crops before anything is
 * tracked.  A crop job makes one such file: icelk_jpeg_crop_start does the host's share (as icelk_upload_jpeg_file_async:
 * index, lanes, the checks of descriptor, crop box, quality and cropped size -- their errors are returned there), copies
 * the bytes into pinned memory of the library and enqueues, on a decode stream and without a wait, the Huffman decoding,
 * the inverse DCT, the crop box as R G B, the re-save's forward kernel, the entropy coder and a verdict.  No frame slot
 * is touched and max_w x max_h of icelk_create bound neither the photo nor the crop.  Every job in flight owns a working
 * set of its own (at 12 MP and 48 bytes per block ~160 MB: the decoder's set, the cropped R G B, the re-save's coefficients
 * and 27 MB for the coder; the sets are kept and reused).
 * The coder's sizes stay on the device: the job may take stream_bytes_per_block x blocks bytes for the stuffed scan
 * (icelk_jpeg_crop_config; 1 .. 416, default 48: a 12 MP photo takes 7 at quality 75 and 17 at 95, uniform noise at
 * quality 100 takes 84).  A scan that does not fit is coded again by icelk_jpeg_crop_finish with the sizes read by the
 * host; a file the device's Huffman decoder does not settle is decoded by the host decoder there.  The bytes are the same
 * on every route: those of icelk_upload_jpeg_file_resave followed by icelk_jpeg_resave_encode. */
#define ICELK_JPEG_CROP_DEVICE 0          /* coded on the device within the budget, no host wait before the verdict */
#define ICELK_JPEG_CROP_HOST_HUFFMAN 1    /* the host decoder took the file (huff.fallback says why); the chain ran again */
#define ICELK_JPEG_CROP_OVER_BUDGET 2     /* the scan did not fit the budget: coded again with host-read sizes */
typedef struct icelk_jpeg_crop_stats {
    icelk_jpeg_huff_stats_t huff;         /* of the source file's decoding */
    uint32_t route;                       /* ICELK_JPEG_CROP_* */
    uint32_t blocks;                      /* of the re-saved file's scan */
    uint64_t budget;                      /* bytes the stuffed scan could take on the device */
    uint64_t stream_len;                  /* bytes of the stuffed scan */
} icelk_jpeg_crop_stats_t;
/* Host only, no handle: the decisions the device-sized kernels take on their control words (csrc/jpeg_enc.h), for tests.
 * out[0 .. 8) = capacity in bytes, its chunks of 64 bytes, its workgroups of 256 chunks, bytes of the packed stream,
 * 1 if pack runs, bytes ff and stuff walk, 1 if stuff runs, the verdict (1 coded, 2 over budget, 3 invalid). */
int icelk_jpeg_enc_budget(uint32_t blocks, int stream_bytes_per_block, uint32_t total_bits, uint32_t invalid, uint32_t ff_total,
                          uint32_t* out);
/* Host only, no handle, re-entrant: the budgeted chain in the kernels' order on the CPU (csrc/jpeg_enc_host.h), with
 * buffers of exactly the capacity.  Coded: the whole file as icelk_jpeg_encode_coefficients_host writes it, ICELK_OK.
 * Over budget or invalid: nothing is written, *len = 0, ICELK_OK.  report (may be NULL): 8 words -- capacity, total bits,
 * invalid, FF count, verdict, stuffed bytes, bytes pack stored, bytes stuff stored.  force / force_mask: control words
 * (bit k of the mask: word k of total bits, invalid, FF count) overwritten behind the scan that wrote them; NULL / 0: none.
 * ICELK_ECAP: `out` is too small, *len says what it takes. */
int icelk_jpeg_encode_budgeted_host(const icelk_jpeg_info_t* info, const int16_t* coef, int stream_bytes_per_block, const uint32_t* force,
                                    uint32_t force_mask, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity,
                                    uint64_t* len, uint32_t* report);
/* 1 .. 416 bytes of stuffed scan per block that a crop job started from now on may take on the device. */
int icelk_jpeg_crop_config(icelk_t* h, int stream_bytes_per_block);
/* Starts a crop job for the file and returns its ticket without waiting; `file` is free on return.  crop_*: pixels to
 * drop on each side; quality 1 .. 100; the cropped width must be >= 3.  Error codes as icelk_upload_jpeg_file_resave, and
 * ICELK_ECAP for a crop of so many blocks that blocks * 1660 bits do not fit 32 bits; no ticket is taken then. */
int icelk_jpeg_crop_start(icelk_t* h, const uint8_t* file, uint64_t len, int crop_left, int crop_top, int crop_right, int crop_bottom,
                          int quality, int* ticket);
/* Never blocks: *state = 0 in flight, 1 coded on the device, 2 icelk_jpeg_crop_finish has host work to do. */
int icelk_jpeg_crop_poll(icelk_t* h, int ticket, int* state);
/* Waits for the job's verdict, takes the routes named above, and writes the file -- header (with one COM segment when
 * comment != NULL), scan, EOI -- into out.  ICELK_ECAP: out is too small (or NULL), *len says what the file takes and the
 * ticket stays valid: the call can be repeated.  After ICELK_OK or any other error the ticket is gone and its working set
 * free.  stats may be NULL.  ICELK_ESTATE: no such ticket in flight. */
int icelk_jpeg_crop_finish(icelk_t* h, int ticket, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity,
                           uint64_t* len, icelk_jpeg_crop_stats_t* stats);
/* Waits for what the job has enqueued and drops the ticket. */
int icelk_jpeg_crop_cancel(icelk_t* h, int ticket);

/* ---- the re-save ahead of the frame: icelk_upload_jpeg_file_async with the re-save, optionally with the file (opt-in) ----
 * One enqueued job per photo gives the slot the frame the reference tracks on and, with want_file, the crop file it would
 * have written: the host's share and checks are those of icelk_upload_jpeg_file_async plus those of
 * icelk_upload_jpeg_file_resave (and, with want_file, of icelk_jpeg_crop_start), all before the slot is taken; then H2D
 * copies, Huffman rounds and phases, the source's inverse DCT, the fused crop-and-forward kernel (the crop box of the planes
 * straight to the re-saved file's coefficients), their inverse DCT into planes of the job's own, the gray into the slot's
 * level 0, with want_file the budgeted coder under icelk_jpeg_crop_config, a verdict and the slot's events go out on a
 * decode stream in one piece.  Memory per job in flight at 12 MP: the plain job's ~56 MB, plus 36 MB for the re-saved
 * coefficients and 18 MB for the second planes -- no cropped R G B image (36 MB in a crop job) -- plus 27 MB for the coder
 * with want_file.
 * icelk_jpeg_async_poll is unchanged in meaning: 1 = the slot's frame is usable, decided by the decoder's verdict alone (a
 * scan over its budget concerns only the file).  icelk_jpeg_async_finish works on such a job: on the decoder's fallback
 * everything behind the Huffman phases runs again into the slot; a wanted file is dropped.  Errors, icelk_sync,
 * icelk_destroy with jobs in flight and a busy slot (ICELK_ESTATE) are as in the plain form. */
int icelk_upload_jpeg_file_async_resave(icelk_t* h, int slot, const uint8_t* data, uint64_t len, int gray_variant, int crop_left,
                                        int crop_top, int crop_right, int crop_bottom, int quality, int want_file);
/* icelk_jpeg_async_finish for a job started with want_file, and the file as icelk_jpeg_crop_finish returns it, by the same
 * three routes (stats->route; the copy goes over the fetch stream).  ICELK_ECAP: out is too small (or NULL), *len says what
 * the file takes, the slot's frame is final and the job stays with its slot: the call can be repeated (or
 * icelk_jpeg_async_finish drops the file).  After ICELK_OK the job is released.  ICELK_ESTATE: no job in flight in the
 * slot, or one started without want_file. */
int icelk_jpeg_async_finish_file(icelk_t* h, int slot, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity,
                                 uint64_t* len, icelk_jpeg_crop_stats_t* stats);

/* ---- the picture of a segment (opt-in) -----------------------------------------------------------
 * At every segment it saves the reference draws a picture (s1:397-434, plot_switch = 1): the segment's last gray frame,
 * 1200 pixels wide, every surviving track as a red line of alpha 0.4, its end point as a red dot of alpha 0.6, the frame's
 * time in a corner.  Here the same content is rasterised on the device, where frame and tracks already are, and written as
 * a baseline JPEG file by the writer of the sections above.  The pixels are this library's, not matplotlib's; the rules
 * are csrc/plot_raster.h (DESIGN.md 7.6 states them and lists the differences), integer arithmetic that the device, the
 * host statement below and tests/plot_restatement.py compute byte for byte alike:
 *   size        Wo = min(out_width, w), Ho = max(1, (2 Wo h + w) / (2 w)); out_width < 8 is ICELK_EARG
 *   background  the exact area average of the gray frame, R = G = B
 *   tracks      (n, vertices, 2) float32 in frame pixels, pixel centres at integers; vertices 1 .. 17, n <= 2^24; one
 *               pixel wide lines without antialiasing, a 5-pixel plus sign at the last vertex; a track with a vertex that
 *               is not finite or has |x| or |y| >= 2^20 is left out whole; n == 0 gives the bare frame
 *   stamp       NULL or up to 48 characters of 0-9 - : . / and space (else ICELK_EARG), a 5 x 7 bitmap font, opaque
 *   file        what Image.fromarray(rgb).save(f, "JPEG", quality=quality) writes for that R G B; quality 1 .. 100 */
/* Host only, no handle, re-entrant: the size of the picture of a w x h frame. */
int icelk_plot_size(int w, int h_, int out_width, int* ow, int* oh);
/* Host only: the 7 rows of the glyph of character ch, top first, bit 4 = the leftmost of its 5 pixels; ICELK_EARG for a
 * character without a glyph. */
int icelk_plot_glyph(int ch, uint8_t* rows);
/* Host only, no handle, re-entrant: the picture's R G B (Wo x Ho, interleaved, rgb_stride bytes per row) of the gray frame
 * at gray (stride bytes per row), by the code the device runs, on the CPU. */
int icelk_plot_overlay_host(const uint8_t* gray, int w, int h_, int stride, const float* tracks, int n, int vertices, int out_width,
                            const char* stamp, uint8_t* rgb, int rgb_stride);
/* The picture of the frame `slot` holds (ICELK_ESTATE when it holds none) with the tracks at `tracks` (host), as a file.
 * Four kernels (csrc/k_plot.hip), the re-save's forward kernel and the entropy coder run on the handle's compute stream,
 * on a working set that belongs to pictures alone (the velocity map's calls share its R G B, coefficients and coder) --
 * the "most recent re-save" of icelk_jpeg_resave_encode and the crop jobs are untouched; it is allocated at first use (at 1200 x 800: 1 MB gray, 7.7 MB counts, 2.9 MB R G B, 2.9 MB
 * coefficients and the coder's buffers) and freed with the handle.  The call waits for the device.  Arguments are checked
 * before anything is enqueued; after an error nothing has been written.  ICELK_ECAP: `file` is too small (or NULL), *len
 * says what the file takes and the call can be repeated.  rgb_or_null: receives the R G B the writer was given (tests). */
int icelk_plot_tracks(icelk_t* h, int slot, const float* tracks, int n, int vertices, int out_width, const char* stamp, int quality,
                      uint8_t* rgb_or_null, int rgb_stride, uint8_t* file, uint64_t capacity, uint64_t* len);
/* The same with the surviving tracks of the current segment (closed = 0) or of the segment the latest switch closed
 * (closed = 1), gathered on the device as icelk_seg_archive / _closed gather them, into a buffer of the library's: no track
 * data crosses PCIe.  A pair of that segment still waiting inside the library goes out first.  *out_n (may be NULL): the
 * tracks drawn. */
int icelk_seg_plot(icelk_t* h, int slot, int closed, int out_width, const char* stamp, int quality, uint8_t* rgb_or_null, int rgb_stride,
                   uint8_t* file, uint64_t capacity, uint64_t* len, int* out_n);

/* ---- the velocity map of a gridded window (opt-in) ----------------------------------------------
 * For every time window the reference draws a map of the fjord (s3:449-465, plot_switch 1: plot_velocities_one_map,
 * s3:471-641; plot_switch 2: plot_velocities_two_maps, s3:644-844): the grid with its unmeasured cells filled, one arrow
 * per measured cell coloured by speed, with switch 2 a second panel with every velocity vector of the window, the fjord's
 * outline, the cameras, four strings and a colour bar.  Here the same content is rasterised on the device and written as a
 * baseline JPEG file.  The pixels are this library's, not matplotlib's; the rules are csrc/map_raster.h (DESIGN.md 7.7
 * states them and lists the differences), which the device, the host statement below and tests/map_restatement.py compute
 * byte for byte alike:
 *   picture     width 64 .. 16384, height 1 .. 16384 (else ICELK_EARG); one or two panels, each a rectangle of the picture
 *               (the view) with world limits and, beside it, a colour bar; everything a panel draws is clipped to its view
 *   cells       (n, 3) float64 left, top, size and one byte each: measured or not.  Unmeasured cells are filled light gray;
 *               every cell's four sides are dark gray lines
 *   outline     (n, 2) float64, a black polyline
 *   arrows      (n, 5) float64 x, y, dx, dy, speed in world units (dy points north): a shaft of the panel's width and a
 *               triangular head, pivot at the tail or the middle, coloured table[min(255, floor(speed / vmax * 256))]; where
 *               arrows overlap the highest index gives the colour and the opacity is 1 - (1 - alpha)^min(hits, 31); an arrow
 *               with a coordinate that is not finite or beyond 2^20 pixels, or a speed that is negative or not finite, is
 *               left out; n <= 2^27.  resident != 0: the arrows of icelk_map_arrows_set instead (arrows is ignored); with
 *               group >= 0 only those whose group is `group`
 *   cameras     (n, 2) float64, n <= 8: opaque red discs
 *   texts       at most 16 items of at most 48 characters of 0-9 - : . / space A-Z a-z , ( ) (else ICELK_EARG); a 5 x 7
 *               bitmap font, lower case drawn as capitals, opaque black, (px, py) the top-left corner in the picture
 *   file        what Image.fromarray(rgb).save(f, "JPEG", quality=quality) writes for that R G B; quality 1 .. 100 */
typedef struct {
    int32_t x0, y0, w, h;          /* the view: inside the picture, w, h >= 1 */
    int32_t bar_x0, bar_w;         /* the colour bar: columns [bar_x0, bar_x0 + bar_w) of the view's rows; bar_w 0: none */
    double xmin, xmax, ymin, ymax; /* world limits, xmin < xmax, ymin < ymax */
    const double* cells;
    const uint8_t* measured;
    int32_t n_cells;
    int32_t n_outline;
    const double* outline;
    const double* arrows;
    int32_t n_arrows;
    int32_t resident;
    int32_t group;
    int32_t pivot;                 /* 0: the tail, 1: the middle */
    double width;                  /* of the shaft in world units, finite, > 0 */
    double alpha;                  /* 0 < alpha <= 1 */
    double vmax;                   /* the speed of the colour table's end, finite, > 0 */
    const double* cameras;
    int32_t n_cameras;
    int32_t reserved;
} icelk_map_panel_t;
typedef struct {
    int32_t px, py;                /* |px|, |py| <= 2^20 */
    char text[56];                 /* NUL-terminated */
} icelk_map_text_t;
typedef struct {
    int32_t width, height, n_panels, n_texts, quality, reserved;
    icelk_map_panel_t panel[2];
    icelk_map_text_t text[16];
    const uint8_t* table;          /* 256 x 3 bytes R G B */
} icelk_map_desc_t;
/* Host only: the 7 rows of the glyph of character ch in a map's texts, as icelk_plot_glyph gives a stamp's. */
int icelk_map_glyph(int ch, uint8_t* rows);
/* Host only, no handle, re-entrant: the picture's R G B (width x height, interleaved, rgb_stride bytes per row) by the code
 * the device runs, on the CPU.  resident (n_resident, 5) and group (NULL or n_resident) stand for what
 * icelk_map_arrows_set holds; a panel with resident != 0 while resident is NULL is ICELK_ESTATE. */
int icelk_map_overlay_host(const icelk_map_desc_t* d, const double* resident, const int32_t* group, int n_resident, uint8_t* rgb,
                           int rgb_stride);
/* A day's arrows (n, 5) and, if not NULL, the group (the window, say) of each, copied to the device, where they stay until
 * the next set, icelk_map_arrows_release or icelk_destroy: every picture of the day draws from the one upload.  n <= 2^27. */
int icelk_map_arrows_set(icelk_t* h, const double* arrows, const int32_t* group_or_null, int n);
int icelk_map_arrows_release(icelk_t* h);
/* The picture d describes, as a file.  k_picture_clear, k_map_cells, k_map_polyline, k_map_arrows and k_map_resolve
 * (csrc/k_map.hip), then the re-save's forward kernel and the entropy coder run on the handle's compute stream, on a
 * working set that belongs to pictures alone (planes of the map's own; R G B, coefficients and coder shared with the
 * segment picture's calls) -- the "most recent re-save" of icelk_jpeg_resave_encode and the crop jobs are untouched; it
 * is allocated at first use (at 1400 x 1000: 16.8 MB planes, 4.2 MB R G B, 4.2 MB
 * coefficients, the call's items and the coder's buffers) and freed with the handle.  The call waits for the device.
 * Every argument is checked before anything is enqueued or allocated; after an error nothing has been written.
 * ICELK_ESTATE: a panel asks for resident arrows and none are set.  ICELK_ECAP: `file` is too small (or NULL), *len says
 * what the file takes and the call can be repeated.  rgb_or_null: receives the R G B the writer was given (tests). */
int icelk_map_draw(icelk_t* h, const icelk_map_desc_t* d, uint8_t* rgb_or_null, int rgb_stride, uint8_t* file, uint64_t capacity,
                   uint64_t* len);

/* ---- the inset photographs of the velocity map (opt-in) ------------------------------------------
 * The reference's maps carry, in a corner, the photograph each camera took in the middle of the window with the camera's
 * name on it (s3:593-626 for one map, s3:788-829 for two).  Here a photo is decoded on the device as
 * icelk_jpeg_decode_rgb_file decodes it, reduced to a thumbnail there without its full-size R G B ever being stored
 * (k_jpeg_thumb, csrc/k_thumb.hip), kept resident, and pasted into the map's R G B behind k_map_resolve (k_map_inset).
 * The rules are csrc/thumb_raster.h, which the device, the host statements below and
 * tests/thumb_restatement.py compute byte for byte alike:
 *   size     a w x h image is fitted into a box box_w x box_h, proportions kept, never enlarged: tw = min(box_w, w),
 *            th = max(1, (2 tw h + w) / (2 w)) (icelk_plot_size's rule); if th > box_h then th = min(box_h, h),
 *            tw = min(box_w, max(1, (2 th w + h) / (2 h))).  w, h in 1 .. 65535, box_w, box_h in 1 .. 16384, else ICELK_EARG
 *   pixels   every channel the exact area average: v = (sum wx wy s + w h / 2) / (w h) with the integer overlap weights of
 *            the segment picture's background; a one-channel image gives R = G = B.  The source samples of a file are
 *            the decoded R G B icelk_jpeg_decode_rgb_file returns, that is Pillow's
 *   paste    a thumbnail opaque with its top-left corner at (x0, y0), wholly inside the picture, then its label: at most
 *            48 characters of a map text's character set in its glyphs and at the picture's text scale, opaque black,
 *            (label_px, label_py) its top-left corner, clipped to the picture; an empty label draws nothing.  Insets are
 *            drawn in array order, behind everything icelk_map_draw draws: a later inset covers an earlier one */
typedef struct {
    int32_t x0, y0;                /* the thumbnail's top-left corner in the picture */
    int32_t index;                 /* which resident thumbnail, 0 .. 7 */
    int32_t label_px, label_py;    /* |label_px|, |label_py| <= 2^20 */
    int32_t reserved;
    char label[56];                /* NUL-terminated */
} icelk_map_inset_t;
typedef struct {
    const uint8_t* rgb;            /* interleaved R G B, stride bytes per row; NULL: this index holds no thumbnail */
    int32_t w, h, stride, reserved;
} icelk_map_inset_pixels_t;
/* Host only, no handle, re-entrant: the size of the thumbnail of a w x h image in a box. */
int icelk_thumb_size(int w, int h_, int box_w, int box_h, int* tw, int* th);
/* Host only, no handle, re-entrant: the tw x th thumbnail (R G B, out_stride bytes per row) of an interleaved image of 1 or
 * 3 channels (stride bytes per row), by the code the device runs, on the CPU.  1 <= tw <= w, 1 <= th <= h. */
int icelk_thumb_host(const uint8_t* img, int w, int h_, int channels, int stride, int tw, int th, uint8_t* out_rgb, int out_stride);
/* Host only: icelk_map_overlay_host, then the insets.  resident_insets[8] stands for what icelk_map_inset_set_* hold: an
 * inset whose index has rgb == NULL there is ICELK_ESTATE.  n_insets 0 .. 8; the other refusals are icelk_map_draw_insets'. */
int icelk_map_overlay_insets_host(const icelk_map_desc_t* d, const double* resident, const int32_t* group, int n_resident,
                                  const icelk_map_inset_t* insets, int n_insets, const icelk_map_inset_pixels_t* resident_insets,
                                  uint8_t* rgb, int rgb_stride);
/* The tw x th thumbnail of a JPEG file given as bytes: decoded on the device as icelk_jpeg_decode_rgb_file does (the same
 * files, the same error codes, the host's Huffman decoder inside the call where the lanes give up), reduced by k_jpeg_thumb
 * from the component planes and copied to out_rgb (stride >= 3 tw bytes per row).  1 <= tw <= width, 1 <= th <= height,
 * else ICELK_EARG.  The call waits for the device. */
int icelk_jpeg_thumb_file(icelk_t* h, const uint8_t* data, uint64_t len, int tw, int th, uint8_t* out_rgb, int stride);
/* The same, but the thumbnail stays on the device as resident inset `index` (0 .. 7) until the next set of that index,
 * icelk_map_inset_release or icelk_destroy.  After an error the index holds what it held. */
int icelk_map_inset_set_file(icelk_t* h, int index, const uint8_t* data, uint64_t len, int tw, int th);
/* A ready thumbnail (R G B, stride >= 3 tw bytes per row, tw and th in 1 .. 16384) as resident inset `index`: for files
 * the device decoder refuses, reduced on the host with icelk_thumb_host, and for tests. */
int icelk_map_inset_set_pixels(icelk_t* h, int index, const uint8_t* rgb, int tw, int th, int stride);
int icelk_map_inset_release(icelk_t* h);
/* icelk_map_draw with insets: everything icelk_map_draw draws, texts included, then per inset, in array order, k_map_inset
 * (csrc/k_thumb.hip) on the map's R G B.  n_insets 0 .. 8; with 0 the file is icelk_map_draw's.  Refused before anything
 * is enqueued or allocated, besides what icelk_map_draw refuses: an index outside 0 .. 7, a thumbnail's rectangle that is
 * not wholly inside the picture, a label of more than 48 characters or with a character outside a map text's, a label
 * position beyond 2^20 (ICELK_EARG); an index that holds no thumbnail (ICELK_ESTATE).  ICELK_ECAP and the repeat are
 * icelk_map_draw's. */
int icelk_map_draw_insets(icelk_t* h, const icelk_map_desc_t* d, const icelk_map_inset_t* insets, int n_insets, uint8_t* rgb_or_null,
                          int rgb_stride, uint8_t* file, uint64_t capacity, uint64_t* len);

/* ---- the PNG writer ------------------------------------------------------------ */
/* An 8-bit R G B picture as a PNG file with the pixels exact: signature, IHDR (8 bits, colour type 2, no interlace), one
 * IDAT, IEND.  IDAT is a zlib stream (78 01) of ONE fixed-Huffman deflate block over the filtered rows -- per row the
 * filter type (of None, Sub, Up, Average, Paeth the one with the smallest sum of absolute values as signed bytes, ties to
 * the lowest type) and the filtered bytes -- parsed greedily in segments of 4096 bytes with the match distances 1, 3 and
 * 1 + 3 w (csrc/png_enc.h).  1 <= w, h <= 16384 and h (1 + 3 w) <= 2^28, stride >= 3 w, else ICELK_EARG.
 * icelk_png_bound: the largest file the coder writes for a w x h picture (9 bits per filtered byte and the fixed parts).
 * icelk_png_filter_host: the filtered rows, h (1 + 3 w) bytes.
 * icelk_png_encode_host: the file, on the host.  ICELK_ECAP when it does not fit `capacity` (out may be NULL then), with
 * *len = what it takes; otherwise *len bytes are written.  None of the three takes a handle; they are re-entrant. */
int icelk_png_bound(int w, int h, uint64_t* bytes);
int icelk_png_filter_host(const uint8_t* rgb, int w, int h, int stride, uint8_t* out);
int icelk_png_encode_host(const uint8_t* rgb, int w, int h, int stride, uint8_t* out, uint64_t capacity, uint64_t* len);
/* The same file, byte for byte, with filters, deflate and Adler-32 on the device (csrc/k_png.hip): host pixels up, file
 * down.  Synchronous.  Refusals come before anything is allocated or enqueued.  ICELK_ECAP as above; the call is then
 * repeated with a larger buffer. */
int icelk_png_encode_rgb(icelk_t* h, const uint8_t* rgb, int w, int h_, int stride, uint8_t* out, uint64_t capacity, uint64_t* len);
/* icelk_map_draw (insets_or_null NULL, n_insets 0) or icelk_map_draw_insets up to and including k_map_resolve / k_map_inset,
 * then the PNG writer on the R G B that is resident on the device: the file decodes to exactly the pixels rgb_or_null
 * receives.  d->quality is ignored.  Refusals, ICELK_ECAP and the repeat are those calls'. */
int icelk_map_draw_png(icelk_t* h, const icelk_map_desc_t* d, const icelk_map_inset_t* insets_or_null, int n_insets, uint8_t* rgb_or_null,
                       int rgb_stride, uint8_t* file, uint64_t capacity, uint64_t* len);

/* ---- the movie of the pictures (opt-in) ------------------------------------------
 * The reference ends a day of s1 and a run of s3 with a movie of the pictures it drew (s1:452-473, s3:194-215: mencoder,
 * 8 frames per second, scaled to 2000 pixels wide).  Here every frame is a baseline JPEG of the picture scaled on the
 * device -- byte for byte Image.fromarray(rgb).resize((ow, oh), Image.BICUBIC).save(f, "JPEG", quality=quality) -- and
 * the container, a Motion-JPEG AVI, is written by the Python package (movie.py).  The rule is csrc/resize.h, which the
 * device, the host statement below and tests/movie_restatement.py compute byte for byte alike:
 *   size     mw = movie_width (<= 0: the picture's own width), mh = max(16, (mw h div w + 8) div 16 * 16): the proportions
 *            kept, the height rounded to the nearest multiple of 16
 *   axis     `in` samples -> `out`: scale = in / out, fs = max(scale, 1), support = 2 fs; output xx has
 *            center = (xx + 0.5) scale and reads samples max(0, (int)(center - support + 0.5)) up to, not including,
 *            min(in, (int)(center + support + 0.5)) with the bicubic weights (a = -0.5) of (j + first - center + 0.5) (1 / fs),
 *            divided by their sum and rounded to 22 fractional bits
 *   sample   clip(0, 255, (2^21 + sum k_j s_j) >> 22) in 32-bit signed arithmetic; the horizontal pass first, rounded to
 *            8 bits, then the vertical pass; a pass with in == out is skipped
 * Every side (w, h, ow, oh) is in 1 .. 16384, else ICELK_EARG. */
/* Host only, no handle, re-entrant. */
int icelk_movie_size(int w, int h_, int movie_width, int* mw, int* mh);
/* Host only, no handle, re-entrant: the w x h picture (R G B, stride bytes per row) resampled to ow x oh (out_stride bytes
 * per row) by the code the device's tables come from, on the CPU. */
int icelk_resize_host(const uint8_t* rgb, int w, int h_, int stride, int ow, int oh, uint8_t* out, int out_stride);
/* The same on the device (k_resize_rows, k_resize_cols: csrc/k_resize.hip): host pixels up, pixels down.  Synchronous.  The
 * two axes' tables stay on the device until other sizes are asked for.  Refusals come before anything is allocated or
 * enqueued. */
int icelk_resize_rgb(icelk_t* h, const uint8_t* rgb, int w, int h_, int stride, int ow, int oh, uint8_t* out, int out_stride);
/* Host only: the size of the handle's most recent picture, what icelk_movie_size is asked with.  ICELK_ESTATE: none yet. */
int icelk_picture_size(icelk_t* h, int* w, int* h_);
/* The movie frame of the handle's most recent picture (icelk_plot_tracks, icelk_seg_plot, icelk_map_draw and its forms,
 * JPEG or PNG): the picture's R G B, still resident on the device, resized to ow x oh into a buffer of the frame's own and
 * coded by the writer's forward kernel and entropy coder on the handle's compute stream.  No pixel crosses PCIe.  The
 * picture's own file and R G B are not touched, and neither is the "most recent re-save".  ow >= 3, quality 1 .. 100.
 * ICELK_ESTATE: the handle has drawn no picture.  ICELK_ECAP: `file` is too small (or NULL), *len says what the file
 * takes and the call can be repeated.  rgb_or_null: receives the frame's R G B (tests).  The call waits for the device. */
int icelk_picture_frame(icelk_t* h, int ow, int oh, int quality, uint8_t* rgb_or_null, int rgb_stride, uint8_t* file, uint64_t capacity,
                        uint64_t* len);

/* ---- the orthophoto (opt-in) -----------------------------------------------------
 * The inverse direction of the projection above: every cell of a map raster is projected into a camera's photograph by
 * Camera.utm_to_photo (imports/camtools.py:334-392) and the crop offsets (camtools.py:423-430), sampled there, and the
 * cameras are merged into one mosaic in which the nearest camera wins.  The rule is csrc/ortho.h, which the device
 * (k_ortho_add, csrc/k_ortho.hip), the host statements below and tests/ortho_restatement.py compute byte for byte alike:
 *   raster   (x0, y0) is the map position of the centre of pixel (0, 0), the top-left one; res > 0 metres; pixel (i, j)
 *            is at tx = x0 + i res, ty = y0 - j res (northing decreases with the row)
 *   seen     pixel (i, j) is seen by a camera with a source of sw x sh samples iff the projection's denominator is
 *            non-zero, the point lies in front of the camera (sigma X2 + xi U2 + yi V2 has the sign of H), its squared
 *            distance d2 is at most max_range^2 when max_range > 0, and 0 <= xs <= sw - 1, 0 <= ys <= sh - 1
 *   sample   fx = floor(256 xs), ix = fx >> 8, ax = fx & 255, ix1 = min(ix + 1, sw - 1), likewise y; bilinear with the
 *            16-bit weights (256 - ax)(256 - ay) ..., + 32768, >> 16; nearest: ((fx + 128) >> 8, (fy + 128) >> 8).  One
 *            channel is replicated to R, G, B
 *   mosaic   begun with the fill colour, cover 0, best +inf; adding camera `index` (0 .. 254) changes a pixel iff it is
 *            seen and d2 < best: the sample, cover = index + 1, best = d2
 * A source is at most 65535 samples a side. */
typedef struct icelk_ortho_raster {
    double x0, y0, res;
    int width, height;
} icelk_ortho_raster_t;
typedef struct icelk_ortho_opts {
    double max_range;          /* metres; <= 0: no limit */
    int sampling;              /* 0 bilinear, 1 nearest */
    uint8_t fill[3];
} icelk_ortho_opts_t;
/* Host only, no handle, re-entrant.  The cropped frame's coordinates, the squared distance and `seen` of every pixel of the
 * raster, row-major (width * height entries each; any of the four may be NULL).  xs, ys are the reference's numbers bit for
 * bit wherever it computes finite ones, seen or not.  ICELK_EARG: a null camera or raster, res <= 0, a non-finite number,
 * sides below 1 or sw, sh outside 1 .. 65535. */
int icelk_ortho_coords_host(const icelk_camera_t* cam, const icelk_ortho_raster_t* raster, int sw, int sh, double max_range, double* xs,
                            double* ys, double* d2, uint8_t* seen);
/* Host only, no handle, re-entrant: the statement on the caller's planes.  rgb: rows rgb_stride >= 3 width bytes apart,
 * cover: rows cover_stride >= width bytes apart, best: width * height doubles.  opts NULL: no range limit, bilinear, white. */
int icelk_ortho_begin_host(const icelk_ortho_raster_t* raster, const icelk_ortho_opts_t* opts_or_null, uint8_t* rgb, int rgb_stride,
                           uint8_t* cover, int cover_stride, double* best);
int icelk_ortho_add_host(const icelk_ortho_raster_t* raster, const icelk_ortho_opts_t* opts_or_null, const icelk_camera_t* cam, int index,
                         const uint8_t* img, int sw, int sh, int channels, int stride, uint8_t* rgb, int rgb_stride, uint8_t* cover,
                         int cover_stride, double* best);
/* The same on the device.  icelk_ortho_begin starts a mosaic in the picture writer's R G B (k_ortho_fill); it refuses,
 * before anything is allocated, what the PNG writer refuses for a width x height picture (sides 1 .. 16384, height *
 * (1 + 3 width) <= 2^28: the stricter upper limits of the two formats; the JPEG writer's lower limit, width >= 3, is
 * icelk_ortho_write's to refuse for a JPEG alone, so that a narrow raster can still be read back or written as a PNG),
 * res <= 0, non-finite numbers and a sampling other than 0 and 1: ICELK_EARG.  The add calls run k_ortho_add on the
 * handle's compute stream and wait for it; ICELK_ESTATE before a begin, ICELK_EARG for an index outside 0 .. 254, a null
 * pointer or a non-finite camera.
 *   _add_pixels     host pixels up (channels 1 or 3, stride >= sw * channels, else ICELK_EARG)
 *   _add_jpeg_file  a JPEG file given as bytes: decoded on the device as icelk_jpeg_decode_rgb_file does (the same files,
 *                   the same error codes, the host's Huffman decoder inside the call where the device's gives up); a gray
 *                   file is sampled from its luma plane
 *   _add_slot       level 0 of the frame `slot` holds (ICELK_ESTATE when it holds none)
 * icelk_ortho_write: the mosaic through the picture writer (format 0: JPEG at `quality`, 1: PNG), so icelk_picture_frame
 * makes a movie frame of it.  rgb_or_null / cover_or_null receive the R G B (rgb_stride >= 3 width) and the cover plane
 * (cover_stride >= width).  ICELK_ECAP: `file` is too small (or NULL), *len says what the file takes, and the call is
 * simply repeated; the mosaic stays as it is and further cameras can be added after a write.  The call waits for the device. */
int icelk_ortho_begin(icelk_t* h, const icelk_ortho_raster_t* raster, const icelk_ortho_opts_t* opts_or_null);
int icelk_ortho_add_pixels(icelk_t* h, const icelk_camera_t* cam, int index, const uint8_t* img, int sw, int sh, int channels, int stride);
int icelk_ortho_add_jpeg_file(icelk_t* h, const icelk_camera_t* cam, int index, const uint8_t* data, uint64_t len);
int icelk_ortho_add_slot(icelk_t* h, const icelk_camera_t* cam, int index, int slot);
int icelk_ortho_write(icelk_t* h, int format, int quality, uint8_t* rgb_or_null, int rgb_stride, uint8_t* cover_or_null, int cover_stride,
                      uint8_t* file, uint64_t capacity, uint64_t* len);

/* ---- camera shake fitted to land anchors (opt-in) ---------------------------------
 * A stage between tracking and saving.  The tracks of a segment that start on static ground (inside an anchor mask) are the
 * anchors; for every vertex k >= 1 the motion of the picture from the segment's first frame to frame k is fitted to them, a
 * robust translation or similarity, and every track's vertex k is mapped back through the fit: the table comes out in the
 * coordinates of the segment's first frame.  The rules are csrc/stab.h, which the kernels (csrc/k_stab.hip), the host
 * statement below and tests/stab_restatement.py compute bit for bit alike:
 *   anchors  rows with flags != 0 whose 2 V coordinates are all finite, in row order; x, y = vertex 0, X, Y = vertex k
 *   start    (a, b, tx, ty) = (1, 0, median(X - x), median(Y - y)), gate g = max(threshold, start_gate)
 *   inlier   ex = X - ((a x - b y) + tx), ey = Y - ((b x + a y) + ty), ex ex + ey ey <= g g
 *   rounds   at most `rounds`: fewer than min_anchors inliers: LOST; fit to the inliers (numpy-ordered sums); g halves down to
 *            the threshold; converged when the inlier set and the gate both stay
 *   fit      translation: the mean shift of the inliers.  Similarity: least squares about the centroids; when the inliers'
 *            spread sum((x - mx)^2 + (y - my)^2) is not >= n_in min_spread^2: the translation fit and DEGENERATE
 *   apply    x' = (a (X - tx) + b (Y - ty)) / (a a + b b), y' = (a (Y - ty) - b (X - tx)) / (a a + b b), to every row; vertex
 *            0 and the vertices of a TOO_FEW or LOST fit are copied bit for bit; a NaN result is stored as 0x7fc00000
 * threshold is the reference's forward-backward bound (s1:333); start_gate, rounds, min_anchors and min_spread are policy
 * defaults, not measurements.  Results per vertex k = 1 .. V - 1 (entry k - 1): motion (a, b, tx, ty), inliers, rms of the
 * inliers (NaN without a model), status bits, rounds_used (fits made). */
#define ICELK_STAB_TOO_FEW 1
#define ICELK_STAB_LOST 2
#define ICELK_STAB_DEGENERATE 4
#define ICELK_STAB_NOT_CONVERGED 8
typedef struct icelk_stab_params {
    int model;                 /* 0 translation, 1 similarity */
    int rounds;                /* 1 .. 16 */
    int min_anchors;           /* >= 2 */
    int reserved;
    double threshold;          /* inlier distance, px, > 0 */
    double start_gate;         /* first gate, px */
    double min_spread;         /* px, >= 0 */
} icelk_stab_params_t;
/* Host only, no handle, no GPU, re-entrant: the statement the kernels are tested against.  tracks: (n, n_vertices, 2) with
 * 2 <= n_vertices <= 17, flags: n bytes, out_tracks: as tracks (may be tracks itself); motion 4 (V - 1) doubles, the other
 * four V - 1 entries; *n_anchors: the anchors found.  params NULL: translation, 1.0, 8.0, 8 rounds, 10 anchors, 64.0.
 * ICELK_EARG: a null pointer, n < 0, n_vertices outside 2 .. 17 or a parameter outside its range. */
int icelk_stab_tracks_host(const float* tracks, const uint8_t* flags, int n, int n_vertices, const icelk_stab_params_t* params_or_null,
                           float* out_tracks, double* motion, int32_t* inliers, double* rms, int32_t* status, int32_t* rounds_used,
                           int* n_anchors);
/* Host only: flags[i] = mask[iy, ix] != 0 with ix = (int)floor(x0 + 0.5), iy likewise (doubles of row i's vertex 0), 0
 * outside the w x h_ mask (rows `stride` >= w bytes apart). */
int icelk_stab_anchor_flags_host(const float* tracks, int n, int n_vertices, const uint8_t* mask, int w, int h_, int stride, uint8_t* flags);
/* The same through the device, a host table up and down like icelk_project_tracks: k_stab_flags, k_stab_compact,
 * k_stab_median, k_stab_rounds, k_stab_apply on the handle's compute stream, one wait at the end.  ICELK_ECAP: more rows
 * than the handle's max_pts.  Bad parameters are ICELK_EARG before anything is enqueued. */
int icelk_stab_tracks(icelk_t* h, const float* tracks, const uint8_t* flags, int n, int n_vertices, const icelk_stab_params_t* params_or_null,
                      float* out_tracks, double* motion, int32_t* inliers, double* rms, int32_t* status, int32_t* rounds_used,
                      int* n_anchors);
/* The anchor mask of icelk_seg_stab_read: w x h_ bytes (rows `stride` apart), non-zero = static ground; uploaded once and
 * resident until replaced, released (host_mask NULL) or the handle is destroyed.  ICELK_EARG: a mask larger than the
 * handle's frames or a stride below w. */
int icelk_stab_set_anchor_mask(icelk_t* h, const uint8_t* host_mask, int w, int h_, int stride);
/* icelk_seg_read (closed != 0: icelk_seg_read_closed) with the stabilisation in between: the segment's surviving tracks are
 * gathered, flagged from the resident anchor mask, fitted and corrected on the device, and come back with their quality,
 * their flags (n bytes, 1 = under the mask) and the per-vertex results.  Sizing as icelk_seg_read: with tracks NULL only
 * *out_n and *out_vertices are set.  The call with buffers waits for the device once: the rows are counted there, min(cap,
 * corners of the segment) rows are copied (rows behind *out_n hold no result) and a count above cap is ICELK_ECAP after the
 * fact.  ICELK_ESTATE without an anchor mask or before the segment's first pair. */
int icelk_seg_stab_read(icelk_t* h, int closed, const icelk_stab_params_t* params_or_null, float* tracks, float* quality, uint8_t* flags,
                        int cap, int max_vertices, int* out_n, int* out_vertices, double* motion, int32_t* inliers, double* rms,
                        int32_t* status, int32_t* rounds_used, int* n_anchors);

/* ---- validation of projected velocities: the normalised median test ------------ */
/* A spatial-coherence check between projection and gridding (Westerweel & Scarano 2005), stated in csrc/validate.h.
 * Lattice: a point's cell is i = floor((x - left) / side), j = floor((top - y) / side); it is judged if x, y, u, v are
 * finite, 0 <= i < cols, 0 <= j < rows and its group lies in 0 .. ngroups - 1.  The pool of (group, cell) is every judged
 * point of the group in the 3 x 3 cells around it, clipped at the lattice edge, the point under test included (the paper
 * leaves it out: a declared difference).  med_u, mad_u, med_v, mad_v are np.median's bits (icelk_grid_stats_t's rules) of
 * the pool's u, of fabs(u - med_u), and likewise for v.  With ru = fabs(u - med_u) / (mad_u + eps), rv likewise and r2 =
 * ru * ru + rv * rv, every operation rounded once, the point is rejected iff r2 > threshold * threshold (a NaN r2 keeps it).
 * status: 0 judged and kept, 1 rejected, 2 a pool of fewer than min_neighbours + 1 terms (kept, r2 NaN), 3 not judged
 * (not finite, outside the lattice, in no group; r2 NaN).
 * The defaults -- threshold 2.0, eps 0.01 m/s, min_neighbours 8 -- are policy, not measurements. */
typedef struct icelk_validate_lattice {
    double left, top, side;
    int cols, rows;
} icelk_validate_lattice_t;
typedef struct icelk_validate_params {
    double threshold, eps;
    int min_neighbours, reserved;
} icelk_validate_params_t;
/* per (group g, cell i, j) at g * cols * rows + j * cols + i: the pool's size and statistics; 0 and four NaN for a cell
 * without a point of its own.  All five members or none. */
typedef struct icelk_validate_cells {
    int32_t* pool_n;
    double *med_u, *med_v, *mad_u, *mad_v;
} icelk_validate_cells_t;
/* x, y, u, v (float64, n); group: NULL (one group, ngroups must be 1) or n group numbers (int32; outside 0 .. ngroups - 1:
 * in no group); params: NULL for the defaults; status (uint8, n), r2 (float64, n); cells: NULL or the five arrays.
 * Kernels of csrc/k_validate.hip: assign, the gridder's sort, pool statistics, judge; one wait for the key count.
 * ICELK_EARG: a null pointer, a threshold, eps or side that is not positive and finite, min_neighbours < 1, cols or rows
 * < 1, ngroups < 1.  ICELK_ECAP: n > 2^27 or ngroups * cols * rows >= 2^31; the handle stays usable.  Everything is
 * checked before anything is allocated. */
int icelk_validate(icelk_t* h, const double* x, const double* y, const double* u, const double* v, int n, const int32_t* group,
                   int ngroups, const icelk_validate_lattice_t* lattice, const icelk_validate_params_t* params, uint8_t* status,
                   double* r2, const icelk_validate_cells_t* cells);
/* The same statement on the CPU: no handle, no GPU, re-entrant.  The kernels are tested against it bit for bit. */
int icelk_validate_host(const double* x, const double* y, const double* u, const double* v, int n, const int32_t* group, int ngroups,
                        const icelk_validate_lattice_t* lattice, const icelk_validate_params_t* params, uint8_t* status, double* r2,
                        const icelk_validate_cells_t* cells);
/* icelk_grid_bin_windows_stats with `stats` nullable and the validation in front of the gridder: the points are uploaded
 * once, the validation runs with the day tables' windows as groups (all cameras of a window share its pools), the DEVICE
 * copy of t becomes NaN at every rejected point, and the unchanged gridder chain runs on that copy -- "NaN lies in no
 * window", so a rejected point is neither selected, counted in sel_count / t_min / t_max, nor binned.  The caller's arrays
 * are not written.  Out also: status (uint8, n) and rejected (int32, nw: the window's rejected points).  device_ms covers
 * the validation's kernels too.  Refusals are those of the two calls it joins, all before anything is allocated. */
int icelk_grid_bin_windows_validated(icelk_t* h, const double* x, const double* y, const double* u, const double* v,
                                     const double* t, int n, const int64_t* file_offset, const int* file_cam,
                                     const int* win_f0, const int* win_f1, int nfiles, const int64_t* t_lo,
                                     const int64_t* t_hi, int ncam, int nw, double left, double top, double spacing,
                                     int cols, int rows, const uint8_t* cell_on, int* count, double* mean_u, double* mean_v,
                                     double* speed, int* sel_count, double* t_min, double* t_max, double* device_ms,
                                     const icelk_grid_stats_t* stats_or_null, const icelk_validate_lattice_t* lattice,
                                     const icelk_validate_params_t* params, uint8_t* status, int32_t* rejected);

/* ---- tidal harmonics of the velocity cube, per cell ---------------------------- */
/* A least-squares fit of m terms -- a mean, cosine and sine of some tidal constituents, perhaps a trend -- to the samples of
 * every cell, stated in csrc/tides.h.  basis: float64 [nt][m], row t the m terms at window t, made by the caller: no sine or
 * cosine is evaluated here.  Window t is a sample of a cell iff u and v are finite and count >= min_count (false for a NaN
 * count).  Normal equations summed in chunks of 256 windows (ascending inside a chunk, chunk totals ascending), Cholesky with
 * the pivot test s > 2^-30 * A[j][j], forward and back substitution, every operation rounded once.
 * Out, per cell: coef_u, coef_v [cell][m]; rms = sqrt(ss_res / (n - m)), NaN for n == m; explained = 1 - ss_res / ss_tot; n
 * (samples), first, last (window index of the first and last sample, -1 without one); status 0 fitted, 1 fewer than
 * max(min_samples, m) samples, 2 rank deficient -- coefficients, rms, explained and residuals are NaN for status != 0.
 * residual_u_or_null, residual_v_or_null: NULL or [window][cell], u - prediction at a sample, NaN elsewhere.
 * device_ms_or_null: the kernels' time by HIP events.
 * icelk_cube_tide_fit runs the kernels of csrc/k_tides.hip on the cube icelk_cube_set left on the device and leaves it as it
 * was.  ICELK_ESTATE without a cube; ICELK_EARG for a null pointer, an nt that is not the cube's, m < 1 or min_samples < 0;
 * ICELK_ECAP for m > 18 or when (m (m + 1) / 2 + 2 m + 2) * ceil(nt / 256) * ncells does not fit 31 bits.  Everything is
 * checked before anything is allocated or issued. */
int icelk_cube_tide_fit(icelk_t* h, const double* basis, int nt, int m, double min_count, int min_samples, double* coef_u,
                        double* coef_v, double* rms_u, double* rms_v, double* explained_u, double* explained_v, int32_t* n,
                        int32_t* first, int32_t* last, int32_t* status, double* residual_u_or_null, double* residual_v_or_null,
                        double* device_ms_or_null);
/* out_u, out_v [ntp][cell]: coef[cell][0] * basis[t][0] + coef[cell][1] * basis[t][1] + ... in that order, NaN for a cell
 * whose status is not 0.  basis [ntp][m] of any length.  Needs no cube.  ICELK_EARG for a null pointer or ncells, m or ntp
 * < 1; ICELK_ECAP for m > 18 or when ncells * ntp does not fit 31 bits. */
int icelk_cube_tide_predict(icelk_t* h, const double* coef_u, const double* coef_v, const int32_t* status, int ncells, int m,
                            const double* basis, int ntp, double* out_u, double* out_v);
/* icelk_cube_tide_fit on host arrays u, v, count [nt][ncells], by the same csrc/tides.h: no handle, no GPU, re-entrant.  The
 * kernels are tested against it bit for bit. */
int icelk_tide_fit_host(const double* u, const double* v, const double* count, int ncells, int nt, const double* basis, int m,
                        double min_count, int min_samples, double* coef_u, double* coef_v, double* rms_u, double* rms_v,
                        double* explained_u, double* explained_v, int32_t* n, int32_t* first, int32_t* last, int32_t* status,
                        double* residual_u_or_null, double* residual_v_or_null);

/* ---- virtual drifters through the gridded velocities ---------------------------- */
/* Particles advected through the velocity cube, or through a tidal fit of it, by the rule of csrc/drift.h: bilinear in
 * space, linear in time, a fixed step, Euler, midpoint or classical Runge-Kutta.  Everything is double. */
typedef struct {
    double x0, y0, dx, dy;   /* node (j, i) lies at (x0 + i * dx, y0 + j * dy); cell = j * cols + i */
    int rows, cols;          /* at least 2 x 2 */
} icelk_drift_lattice_t;
typedef struct {
    double step;             /* seconds, finite, not 0; negative: the field runs backwards */
    int nsteps, every;       /* steps 0 .. nsteps; positions are recorded at the steps 0, every, 2 * every, ... */
    int order, min_nodes;    /* 1, 2 or 4; 1 .. 4 measured nodes a sample needs */
} icelk_drift_params_t;
typedef struct {
    double *x, *y;           /* [nsteps / every + 1][n]; NaN before the release and after the stop */
    double *last_x, *last_y, *length;   /* per drifter: the last position (NaN if never released), the path's length */
    int32_t *status;         /* ICELK_DRIFT_* */
    int32_t *stop_step;      /* the step that failed; nsteps for a drifter alive at the end, -1 if never released */
    int32_t *visits_or_null; /* [rows][cols]: recorded finite samples per nearest node */
} icelk_drift_out_t;
enum { ICELK_DRIFT_ALIVE = 0, ICELK_DRIFT_LEFT = 1, ICELK_DRIFT_TOO_FEW = 2, ICELK_DRIFT_NO_FIELD = 3, ICELK_DRIFT_NEVER_RELEASED = 4 };
/* The schedule table has 2 * nsteps + 1 rows, row r the time start + r * step / 2, and is made by the caller: no time axis
 * is searched and no sine is evaluated here.
 * icelk_cube_drift: the cube icelk_cube_set left on the device, which stays as it was.  Per row the windows k0 <= k1 that
 * bracket its time, the weight a of k1 and a flag, 0 for "no field at that time".  A window's node is measured iff u, v are
 * finite and count >= min_count.  lattice->rows * cols must be the cube's ncells.
 * icelk_drift_tide: coef_u, coef_v [cell][m] and status [cell] as icelk_cube_tide_predict takes them, basis [2 * nsteps +
 * 1][m].  Needs no cube.
 * seed_x, seed_y, release: one per drifter; a drifter exists from step release[p] on iff its seed is finite and 0 <=
 * release[p] < nsteps.
 * ICELK_ESTATE without a cube (icelk_cube_drift); ICELK_EARG for a null pointer, a lattice below 2 x 2 or with a spacing
 * that is 0 or not finite or, for the cube, of another cell count, n < 1, step 0 or not finite, nsteps < 1, every < 1, an
 * order not in {1, 2, 4}, min_nodes outside 1 .. 4, m < 1, a k0 or k1 outside the cube's windows; ICELK_ECAP when n *
 * (nsteps / every + 1) or (2 * nsteps + 1) * m does not fit 31 bits, or m > 18.  Everything is checked before anything is
 * allocated or issued.  device_ms_or_null: the kernels' time by HIP events. */
int icelk_cube_drift(icelk_t* h, const icelk_drift_lattice_t* lattice, const icelk_drift_params_t* params, const int32_t* k0,
                     const int32_t* k1, const double* a, const int32_t* flag, double min_count, const double* seed_x,
                     const double* seed_y, const int32_t* release, int n, const icelk_drift_out_t* out, double* device_ms_or_null);
int icelk_drift_tide(icelk_t* h, const icelk_drift_lattice_t* lattice, const icelk_drift_params_t* params, const double* coef_u,
                     const double* coef_v, const int32_t* status, int m, const double* basis, const double* seed_x,
                     const double* seed_y, const int32_t* release, int n, const icelk_drift_out_t* out, double* device_ms_or_null);
/* Both sources on host arrays by the same csrc/drift.h: no handle, no GPU, re-entrant.  The cube source when u is given
 * (u, v, count [nt][rows * cols] with k0, k1, a, flag), the tide source when coef_u is (with coef_v, status, m, basis);
 * exactly one of the two, the other's pointers NULL.  The kernels are tested against it bit for bit. */
int icelk_drift_host(const icelk_drift_lattice_t* lattice, const icelk_drift_params_t* params, const double* u, const double* v,
                     const double* count, int nt, const int32_t* k0, const int32_t* k1, const double* a, const int32_t* flag,
                     double min_count, const double* coef_u, const double* coef_v, const int32_t* status, int m,
                     const double* basis, const double* seed_x, const double* seed_y, const int32_t* release, int n,
                     const icelk_drift_out_t* out);

/* ---- measurement ------------------------------------------------------------------------------ */
/* Per-kernel HIP-event timing on the handle's streams (bench.py's roofline leg).  on = 1: every kernel; on = 2: the
 * tracker launches only (each timed kernel costs two event records on its stream, which the chains of short detector
 * kernels feel); on = 0: off, durations collected so far are added up. */
int icelk_prof_enable(icelk_t* h, int on);
int icelk_prof_reset(icelk_t* h);
/* LK iterations every feature of the latest tracker call ran while profiling was enabled: forward pass in the low 16
 * bits, backward pass in the high 16 (0xffffffff = a track that was already dead); *out_n = features of that call.
 * The iterations-per-feature histogram of bench.py comes from here. */
int icelk_prof_iterations(icelk_t* h, uint32_t* host_out, int cap, int* out_n);
/* Outcome of the hardware-queue probe icelk_create ran for this handle: picks[0..3] = which of the eight
 * candidate streams became the detection / candidates / pyramid / tail stream; *quickest = the smallest fraction of the filler's duration after which a one-wave kernel on a candidate stream
 * came back beside a busy compute stream, *limit = the fraction above which a stream counted as held up.  Throughput
 * depends on these picks, results do not: bench.py records them with every line. */
int icelk_stream_probe_info(icelk_t* h, int* picks, double* quickest, double* limit);
int icelk_prof_count(void);
const char* icelk_prof_name(int kernel_id);
int icelk_prof_get(icelk_t* h, int kernel_id, int* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* ICELK_H */
