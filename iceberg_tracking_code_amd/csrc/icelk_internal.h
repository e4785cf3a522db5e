// icelk_internal.h -- shared between the translation units of libicelk.so (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/icelk.h"
#include "jpeg_enc.h"
#include "jpeg_lanes.h"
#include "plot_raster.h"
#include "png_enc.h"
#include "map_raster.h"
#include "thumb_raster.h"
#include "resize.h"
#include "ortho.h"
#include "stab.h"

namespace icelk {

constexpr int kMaxLevels = ICELK_MAX_LEVELS;
constexpr int kPitchAlign = 64;  // bytes; every level row starts 64-B aligned (dword / dwordx4 loads)

// One pyramid level in device memory (unpadded; borders are reflected inside the kernels).
struct Level {
    uint8_t* ptr;
    int w, h, pitch;
};

// By-value kernel argument: the whole pyramid of one frame.
struct Pyramid {
    Level lv[kMaxLevels];
};

struct LKParams {
    int win_w, win_h;
    int top_level;      // effective maxLevel (levels used = top_level + 1)
    int max_count;      // clamped criteria.maxCount
    double eps2;        // clamped criteria.epsilon squared
    int flags;
    float min_eig_thr;
    float fb_thr;
    int margin;         // search-region margin R of the LDS-staged J tile
    float eps2_lo, eps2_hi;   // float values below / above which (double)dx*dx + (double)dy*dy <= eps2 is decided
    int dist_form;      // forward-backward distance: 0 = np.hypot on float32 (s1:330), 1 = (dx^2+dy^2)^0.5 (s0_1:99)
    // how A11, A12, A22, b1, b2 are summed (icelk_set_variant "lk_sums"): 0 = exactly (int64), one rounding; 1 / 2 = in the
    // float lanes of OpenCV 3.x's SSE2 block / 4.x's CV_SIMD128 block (oracle/icelk_oracle.c orc_set_variant).  Non-zero
    // runs in the window-generic kernel only.
    int sum_mode;
    // bound of the narrow-sum guard of the tuned kernels (lk_common.h): 2^26, or 0 under icelk_set_variant "lk_wide_sums" 1,
    // which no lane passes, so every sum takes the 64-bit arm.  A kernel argument: it sits in a scalar register.
    unsigned sum_guard;
};

// kernel ids for the profiling table
enum KernelId {
    K_GRAY = 0,
    K_PYRDOWN,
    K_LK,
    K_LK_FB,
    K_EIG,
    K_SUPPRESS,
    K_EMIT,
    K_PROJECT,
    K_SYNTH,
    K_LK_FB_PAIR,   // two segment pairs in one launch (icelk_seg_track_defer)
    K_JPEG_IDCT,    // dequantise + inverse DCT (k_jpeg.hip)
    K_JPEG_OUT,     // upsample + colour + crop + gray / RGB
    K_JPEG_HUFF,    // Huffman decoding: synchronise, scan, write, DC (k_jpeg_huff.hip)
    K_JPEG_FWD,     // the re-save's forward half: colour, downsampling, forward DCT, quantisation (k_jpeg_fwd.hip)
    K_JPEG_ENC_COUNT,   // the JPEG writer (k_jpeg_enc.hip): bit length of every block
    K_JPEG_ENC_SCAN,    // ... prefix sums (bit offsets of the groups, FF counts of the stretches)
    K_JPEG_ENC_PACK,    // ... the blocks' bits at their offsets
    K_JPEG_ENC_FF,      // ... FF bytes of the packed stream
    K_JPEG_ENC_STUFF,   // ... the stream with a 00 behind every FF
    K_JPEG_ENC_PACK_BUDGET,    // the device-sized forms of a job with a file (abi_jpeg_job.hip)
    K_JPEG_ENC_FF_BUDGET,
    K_JPEG_ENC_STUFF_BUDGET,
    K_JPEG_CROP_RGB,           // the crop box of the decoded planes as R G B into the job
    K_JPEG_CROP_VERDICT,
    K_JPEG_CROP_FWD,           // the crop box of the decoded planes straight to the re-save's coefficients (k_jpeg_fwd.hip)
    K_PLOT_BACKGROUND,         // the segment picture (k_plot.hip): area-averaged gray plane
    K_PLOT_CLEAR,              // ... the count planes zeroed
    K_PLOT_SCATTER,            // ... lines and dots counted
    K_PLOT_RESOLVE,            // ... counts, background, tables and stamp -> R G B
    K_MAP_CLEAR,               // the velocity map (k_map.hip): the three planes zeroed
    K_MAP_CELLS,               // ... unmeasured cells filled, cell edges
    K_MAP_POLYLINE,            // ... the outline
    K_MAP_ARROWS,              // ... shafts and heads: top index and hit count
    K_MAP_RESOLVE,             // ... planes, cameras, bars and texts -> R G B
    K_JPEG_THUMB,              // the inset photographs (k_thumb.hip): decoded planes -> area-averaged R G B thumbnail
    K_MAP_INSET,               // ... a thumbnail and its label into the map's R G B
    K_PNG_FILTER,              // the PNG writer (k_png.hip): the five row filters, the smallest kept -> the filtered stream
    K_PNG_PARSE,               // ... a segment's tokens, their bit count, its Adler piece
    K_PNG_SCAN,                // ... bit offset of every segment (k_jpeg_enc_scan)
    K_PNG_PACK,                // ... the deflate bits
    K_PNG_ADLER,               // ... the pieces joined
    K_RESIZE_ROWS,             // the movie's scaler (k_resize.hip): the horizontal pass
    K_RESIZE_COLS,             // ... the vertical pass
    K_GRID_SEGMENTS,           // the per-cell statistics (k_grid.hip): begin and count of every segment
    K_GRID_STD,                // ... np.std(ddof=1), one thread per segment
    K_GRID_SELECT,             // ... median and MAD, one workgroup per segment and array
    // (new entries go in front of the three box entries, which tests/test_transect_host.py holds to be the table's last)
    K_ORTHO_FILL,              // the orthophoto (k_ortho.hip): a mosaic begun -- fill colour, cover 0, best +inf
    K_ORTHO_ADD,               // ... a camera's photograph gathered into the raster
    // (... and in front of the five stab entries, which tests/test_stab_host.py holds to stand right before those)
    K_VALIDATE_ASSIGN,         // the normalised median test (k_validate.hip): keys of the judged points (both assign forms)
    K_VALIDATE_POOLS,         // ... median and MAD of every pool, one workgroup per (group, cell) and component
    K_VALIDATE_JUDGE,          // ... status and r2 of every keyed point, rejected counts
    K_STAB_FLAGS,              // camera shake (k_stab.hip): flags and anchors of every row
    K_STAB_COMPACT,            // ... the anchors' row numbers, in row order
    K_STAB_MEDIAN,             // ... the start shift of every vertex
    K_STAB_ROUNDS,             // ... the robust fit, one workgroup per vertex
    K_STAB_APPLY,              // ... every row mapped back through its vertex's fit
    K_BOXES_ASSIGN,            // transect / mooring boxes (k_grid.hip): every point against every box, one window
    K_BOXES_DAY_ASSIGN,        // ... a whole day of windows
    K_GRID_DAY_ASSIGN,         // the day gridder's assign kernel, for comparison with the one above
    K_COUNT_
};

struct Slot {
    uint8_t* base = nullptr;  // one allocation holding all levels
    size_t bytes = 0;
    int w = 0, h = 0;
    int levels_built = 0;     // number of valid images (0 = empty, 1 = level 0 only)
    Level lv[kMaxLevels];
    hipEvent_t ready = nullptr;   // upload-complete event (async uploads)
    bool pending = false;
    hipEvent_t frame_ev = nullptr;  // level 0 written (recorded on the compute stream by every ingest call)
    // last readers of the slot: pyramid/tracker launches on the compute stream, the corner kernel on the
    // detection stream.  An asynchronous upload into the slot waits for exactly these, not for everything that
    // happens to be queued, so frame t+1 crosses PCIe while frame t is being tracked.
    // `used` refers to the event that covers the latest such launch: the slot's own (`used_own`) or one shared by
    // everything a tracker launch touched (Ctx::launch_ev), so that a launch costs one event record, not one per slot
    hipEvent_t used = nullptr, used_own = nullptr, det_used = nullptr;
    hipEvent_t eig_used = nullptr;   // the corner kernel of icelk_seg_detect_prepare (candidates stream) reads level 0
    unsigned long long gen = 0;   // bumped whenever a new frame enters the slot
};

struct ProfEvt {
    hipEvent_t a, b;
    int id;
};

struct Ctx;  // full definition in icelk_ctx.h

// ---- launchers (each defined in its kernel TU) -------------------------------------------------
void launch_bgr2gray(hipStream_t s, const uint8_t* src, int src_pitch, uint8_t* dst, int dst_pitch,
                     int w, int h, int variant);
void launch_pyrdown(hipStream_t s, const Level& src, const Level& dst);
// lv[first+1 .. first+n] (n = 1..3) from lv[first] in ONE launch (k_pyramid.hip)
void launch_pyramid_fused(hipStream_t s, const Level* lv, int first, int n, bool one_wave = false);
void launch_synth(hipStream_t s, const Level& dst, int64_t ux, int64_t uy, uint32_t seed, const int* affine);

// JPEG ingest (k_jpeg.hip).  By-value kernel arguments.
struct JpegIdctArgs {
    const int16_t* coef[3];   // device: a component's blocks, raster order over blocks_x[c] per row, 64 values each
    uint8_t* plane[3];        // device: the component's samples, pitch[c] >= 8 * blocks_x[c] (a multiple of 8)
    int pitch[3], blocks_x[3];
    int bx0[3], by0[3], nbx[3];   // the rectangle of blocks to transform
    int first[4];             // component c owns the launch's blocks first[c] .. first[c+1]-1
    uint16_t quant[3][64];
};
struct JpegOutArgs {
    const uint8_t* plane[3];
    int pitch[3];
    int W;                    // image width = true width of the luma plane
    int cw, ch;               // true size of the chroma planes
    int mode;                 // chroma upsampling: 0 none, 1 / 2 triangle filter 2x1 / 2x2, 3 / 4 replication 2x1 / 2x2
    int left, top, ow, oh;    // output pixel (x, y) is image pixel (x + left, y + top)
    uint8_t* dst;
    int dst_pitch;
    int k0, k1, k2, shift;    // gray weights (launch_jpeg_gray fills them in)
};
void launch_jpeg_idct(hipStream_t s, const JpegIdctArgs& A);
void launch_jpeg_gray(hipStream_t s, JpegOutArgs A, int variant);
void launch_jpeg_rgb(hipStream_t s, JpegOutArgs A);

// The forward half of the re-save (k_jpeg_fwd.hip; the arithmetic is jpeg_fwd.h): interleaved R G B -> quantised
// coefficients of a 4:2:0 file in the layout of icelk_jpeg_info_t.  By-value kernel arguments.
struct JpegFwdArgs {
    const uint8_t* rgb;       // device: h rows of w pixels, 3 bytes each, `pitch` bytes apart
    int pitch, w, h;
    int16_t* coef[3];         // device: the components' blocks, 16-byte aligned
    int mcus_x, mcus_y;       // luma has 2 mcus_x x 2 mcus_y blocks, chroma mcus_x x mcus_y
    int real_bx, real_by;     // luma blocks that hold samples: ceil(w / 8), ceil(h / 8); the others are dummies
    uint16_t quant[2][64];    // luma, chroma
    uint32_t recip[2][64];    // fwd::reciprocal(8 * quant)
};
void launch_jpeg_fwd(hipStream_t s, const JpegFwdArgs& A);
// The same from the crop box of a decoded file's planes (O: planes, chroma mode, left, top; O.dst is not used), fused: the
// crop is A.w x A.h, A.rgb is not read.  The pixels are k_jpeg_out's (jpeg_rgb.h).
void launch_jpeg_crop_fwd(hipStream_t s, const JpegOutArgs& O, const JpegFwdArgs& A);

// The JPEG writer's entropy coder (k_jpeg_enc.hip; the arithmetic is jpeg_enc.h).  All pointers are device memory.
constexpr int kJpegEncGroup = 64;        // blocks (lanes) per workgroup of count and pack: one wave
constexpr int kJpegEncScanPass = 1024;   // entries the prefix sum takes per pass of its loop
constexpr int kJpegEncChunk = 64;        // bytes of the packed stream per lane of ff and stuff; 256 lanes per workgroup
enum JpegEncCtl { JE_TOTAL_BITS = 0, JE_INVALID, JE_FF_TOTAL, JE_WORDS = 4 };   // words of JpegEncArgs::ctl
struct JpegEncArgs {
    enc::Layout L;
    const int16_t* coef;      // 16-byte aligned
    const uint32_t* codes;    // enc::Codes
    uint16_t* bits;           // per block of the scan: its length
    uint32_t* group;          // per kJpegEncGroup blocks: the sum of their lengths, after the scan the bit offset of the first
    uint32_t* ctl;            // JpegEncCtl
    uint32_t* packed;         // the unstuffed stream, zero-filled to whole chunks before pack runs
};
void launch_jpeg_enc_count(hipStream_t s, const JpegEncArgs& A);
void launch_jpeg_enc_scan(hipStream_t s, uint32_t* v, uint32_t n, uint32_t* total);   // in place, exclusive
void launch_jpeg_enc_pack(hipStream_t s, const JpegEncArgs& A);
void launch_jpeg_enc_ff(hipStream_t s, const uint32_t* packed, uint32_t nchunks, uint32_t* wg_ff);
void launch_jpeg_enc_stuff(hipStream_t s, const uint32_t* packed, uint32_t nbytes, uint32_t nchunks, const uint32_t* wg_off, uint8_t* out);
// The device-sized forms of a job with a file (abi_jpeg_job.hip): `cap` bytes are allocated for the stuffed scan, packed (whole
// chunks of it, zeroed) and out; the sizes come from ctl, where count and the scans left them.  wg_ff has
// enc::groups_of(enc::chunks_of(cap)) entries, which the second scan runs over.
void launch_jpeg_enc_pack_budget(hipStream_t s, const JpegEncArgs& A, uint32_t cap);
void launch_jpeg_enc_ff_budget(hipStream_t s, const uint32_t* packed, const uint32_t* ctl, uint32_t cap, uint32_t* wg_ff);
void launch_jpeg_enc_stuff_budget(hipStream_t s, const uint32_t* packed, const uint32_t* ctl, uint32_t cap, const uint32_t* wg_off, uint8_t* out);
// last in a crop job's chain: the words of JpegVerdictWord (below) to the job's pinned words, the sequence word last.
// enc_ctl NULL: no file was asked for (a slot-bound re-save job without one), the coder's words say enc::kNotAsked
void launch_jpeg_crop_verdict(hipStream_t s, const uint32_t* huff_ctl, int max_rounds, const uint32_t* enc_ctl, uint32_t cap, uint32_t* host_words,
                              uint32_t seq);

// Huffman decoding on the device (k_jpeg_huff.hip; the algorithm is jpeg_lanes.h).  All pointers are device memory.
constexpr int kJpegMaxRounds = 255;
constexpr int kJpegDcChunk = 16;   // MCUs one thread of the DC pass sums up
enum JpegHuffCtl {                 // words of JpegHuffArgs::ctl
    JH_BOUND = 0,     // a chain stopped at max_hops
    JH_IRREGULAR,     // the write phase met a stream that contradicts itself
    JH_IN_STEP,       // lanes whose guess was the true state
    JH_SPANS,         // blocks that began in one lane and ended in another
    JH_MAX_HOPS,
    JH_TOTAL_HOPS,
    JH_ROUND0 = 8,    // ctl[JH_ROUND0 + r] != 0: round r changed an entry state
    JH_WORDS = JH_ROUND0 + kJpegMaxRounds + 1
};
struct JpegHuffArgs {
    lanes::Scan A;
    const uint8_t* data;            // the file
    const lanes::Seg* seg;          // A.nseg + 1
    const lanes::HuffTable* tabs;   // lanes::kTables
    uint64_t* T;                    // [lane] entry state
    uint32_t* cnt;                  // [lane] blocks completed in the subsequence
    uint32_t* P;                    // [lane + 1] exclusive prefix sum of cnt over all lanes
    uint64_t* X;                    // [2][group] exit state of a group, by the round's parity
    uint32_t* ctl;
    int16_t* coef;
    int32_t* dc;                    // [chunk][3] sums of DC differences, then their prefix inside the restart interval
    uint32_t ngroups;
    uint32_t ri_mcus, cps;          // MCUs per restart interval, chunks per restart interval
};
void launch_jpeg_huff_sync(hipStream_t s, const JpegHuffArgs& H, int round);
void launch_jpeg_huff_scan(hipStream_t s, const JpegHuffArgs& H);
void launch_jpeg_huff_write(hipStream_t s, const JpegHuffArgs& H);
void launch_jpeg_huff_dc(hipStream_t s, const JpegHuffArgs& H);
// What k_jpeg_huff_verdict publishes about a file to pinned host words, the sequence word last
enum JpegVerdictWord {
    JV_VERDICT = 0,   // JV_DECODED, or the ICELK_JPEG_FALLBACK_* reason the host decoder has to take the file for
    JV_ROUNDS,
    JV_MAX_HOPS,
    JV_TOTAL_HOPS,
    JV_IN_STEP,
    JV_SPANS,
    JV_ENC_VERDICT,   // crop jobs (k_jpeg_crop_verdict): enc::Verdict of the budgeted coder
    JV_ENC_LEN,       // ... bytes of the stuffed scan when it is enc::kCoded
    JV_SEQ = 8,
    JV_WORDS = 16
};
constexpr uint32_t JV_DECODED = 0x100;
void launch_jpeg_huff_verdict(hipStream_t s, const uint32_t* ctl, int max_rounds, uint32_t* host_words, uint32_t seq);
// The decoder's words of a verdict (JV_VERDICT .. JV_SPANS) from its control words, by the one wave of a verdict kernel
// (k_jpeg_huff_verdict, k_jpeg_crop_verdict): lane 0 stores them; the caller fences and stores the sequence word.
__device__ __forceinline__ void jpeg_huff_verdict_words(const uint32_t* __restrict__ ctl, int max_rounds, uint32_t* __restrict__ out)
{
    __shared__ uint32_t first_quiet;   // the first round in 1 .. max_rounds that changed nothing, max_rounds + 1: none
    if (threadIdx.x == 0) first_quiet = (uint32_t)max_rounds + 1u;
    __syncthreads();
    for (uint32_t q = 1 + threadIdx.x; q <= (uint32_t)max_rounds; q += blockDim.x)
        if (ctl[JH_ROUND0 + q] == 0) atomicMin(&first_quiet, q);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const bool settled = first_quiet <= (uint32_t)max_rounds;
    const bool bound = ctl[JH_BOUND] != 0;
    uint32_t verdict = JV_DECODED;
    if (bound || !settled) verdict = ICELK_JPEG_FALLBACK_BOUND;
    else if (ctl[JH_IRREGULAR]) verdict = ICELK_JPEG_FALLBACK_STREAM;
    out[JV_VERDICT] = verdict;
    out[JV_ROUNDS] = first_quiet;   // round 0 and the first_quiet - 1 rounds behind it changed an entry state
    out[JV_MAX_HOPS] = ctl[JH_MAX_HOPS];
    out[JV_TOTAL_HOPS] = ctl[JH_TOTAL_HOPS];
    out[JV_IN_STEP] = ctl[JH_IN_STEP];
    out[JV_SPANS] = ctl[JH_SPANS];
}

// The segment picture (k_plot.hip; the arithmetic is plot_raster.h).  All pointers are device memory.  bg (bytes) and the
// two count planes (words) are padded to a multiple of four pixels; counts = lines | dots, `words` in all; tables = TL | TD,
// plot::kTable words each; rgb: rows 3 Wo bytes apart.  tracks: (n, nv, 2) float32.
void launch_plot_background(hipStream_t s, const Level& src, int Wo, int Ho, uint8_t* bg);
void launch_picture_clear(hipStream_t s, uint32_t* planes, size_t words);   // the map's three planes as well
void launch_plot_scatter(hipStream_t s, const float* tracks, int n, int nv, int W, int H, int Wo, int Ho, uint32_t* lines, uint32_t* dots);
void launch_plot_resolve(hipStream_t s, const uint8_t* bg, const uint32_t* lines, const uint32_t* dots, const uint32_t* tables,
                         const plot::Stamp& stamp, int Wo, int Ho, uint8_t* rgb);

// k_map.hip: the velocity map.  planes: base | top | count, each padded to four pixels; cells (n, 3), xy (n, 2), arrows
// (n, 5) float64 on the device; group: NULL or one int32 per arrow; d_scene: a map::Scene in device memory
void launch_map_cells(hipStream_t s, const map::View& V, const double* cells, const uint8_t* measured, int n, int Wo, uint32_t* base);
void launch_map_polyline(hipStream_t s, const map::View& V, const double* xy, int n, int Wo, uint32_t* base);
void launch_map_arrows(hipStream_t s, const map::View& V, int w, bool pivot_mid, const double* arrows, const int32_t* group, int want, int n,
                       int Wo, uint32_t* top, uint32_t* count);
void launch_map_resolve(hipStream_t s, const map::Scene* d_scene, int Wo, int Ho, const uint32_t* base, const uint32_t* top,
                        const uint32_t* count, uint8_t* rgb);

// k_thumb.hip: the inset photographs.  A: the planes of a whole decoded file (left = top = 0, ow x oh the image), dst the
// Wt x Ht thumbnail (R G B, dst_pitch bytes per row); ncomp 1 or 3.  I.px: device memory; rgb: the map's R G B, 3 Wo bytes per row
void launch_jpeg_thumb(hipStream_t s, const JpegOutArgs& A, int ncomp, int Wt, int Ht);
void launch_map_inset(hipStream_t s, const thumb::Inset& I, int Wo, int Ho, uint8_t* rgb);

// k_stab.hip: camera shake fitted to land anchors (the rules are stab.h's; the bounds are stated at the head of k_stab.hip).
// The five kernels of one stabilisation, launched in this order on one stream; K_STAB_FLAGS + step is the step's profiling id
enum StabStep { STAB_FLAGS, STAB_COMPACT, STAB_MEDIAN, STAB_ROUNDS, STAB_APPLY, STAB_STEPS };
struct StabOut {               // what one copy brings back
    stab::VertexResult res[stab::kMaxVert - 1];
    int n_a, n;                // anchors; rows of a gathered segment
};
struct StabArgs {
    float* tracks;             // (n, V, 2), corrected in place
    int n, V;                  // n: the rows, or their upper bound when n_ptr says how many there are
    const int* n_ptr;          // NULL, or the device's count of the rows (<= n)
    const uint8_t* in_flags;   // n bytes, or NULL: the flags come from the mask
    const uint8_t* mask;       // mask_w x mask_h bytes, rows mask_w apart
    int mask_w, mask_h;
    uint8_t *flags, *anchor;   // n bytes each (flags may be in_flags)
    int *idx, *n_a;
    unsigned long long* keys;  // 2 (V - 1) stretches of `stride`
    uint8_t* w;                // V - 1 stretches of `stride`
    size_t stride;             // >= n
    double* med;               // 2 (V - 1)
    stab::VertexResult* res;   // V - 1
    icelk_stab_params_t P;
};
void launch_stab_step(hipStream_t s, const StabArgs& A, int step);

// k_ortho.hip: the orthophoto (the arithmetic is ortho.h).  rgb: rows 3 R.width bytes apart, cover: R.width bytes, best:
// R.width doubles, all R.height rows, device memory; S.px device memory
void launch_ortho_fill(hipStream_t s, int width, int height, const uint8_t* fill, uint8_t* rgb, uint8_t* cover, double* best);
void launch_ortho_add(hipStream_t s, const icelk_camera_t& cam, const icelk_ortho_raster_t& R, const ortho::Source& S, double max_range,
                      int sampling, int index, uint8_t* rgb, uint8_t* cover, double* best);

// k_png.hip: the PNG writer (the arithmetic is png_enc.h).  All pointers are device memory; F and tok are allocated in
// whole segments (png::segments_of(n) * png::kSegment elements), stream is zero before pack and holds
// png::deflate_bytes(9 n) bytes rounded up to dwords, plus one
constexpr int kPngLanes = 256;   // lanes per workgroup of every kernel; parse and pack take png::kSegment / 256 positions per lane
enum PngCtl { PNG_TOTAL_BITS = 0, PNG_ADLER, PNG_WORDS = 4 };   // words of PngArgs::ctl
struct PngArgs {
    const uint8_t* rgb;   // the picture, rows `stride` bytes apart
    uint32_t stride;
    int w, h;
    uint32_t n, pitch;    // bytes of the filtered stream, of one of its rows (1 + 3 w)
    uint8_t* F;           // the filtered stream
    uint16_t* tok;        // per position of F: the token that begins there, or 0
    uint32_t* seg;        // per segment: the bits of its tokens, after the scan the sum of those before it
    uint32_t* adler;      // per segment: A, B, n of png::Adler
    uint32_t* stream;     // the deflate block
    uint32_t* ctl;        // PngCtl
};
void launch_png_filter(hipStream_t s, const PngArgs& A);
void launch_png_parse(hipStream_t s, const PngArgs& A);
void launch_png_pack(hipStream_t s, const PngArgs& A);
void launch_png_adler(hipStream_t s, const uint32_t* pieces, uint32_t n, uint32_t* value);

// k_resize.hip: the movie's scaler (the arithmetic is resize.h).  An axis' table on the device: output o reads the source
// samples first[o] .. first[o] + count[o] - 1 with the weights k[o * pitch + j]; 0 <= first, first + count <= the axis' `in`,
// first and first + count never decrease with o
struct ResizeAxis {
    const int32_t *first, *count, *k;
    int pitch;
};
// rows: the `rows` rows at src (src_pitch bytes apart, X.in pixels) -> ow pixels each at dst (dst_pitch bytes apart)
// cols: ow pixels of each of oh rows at dst; output row y reads src rows first[y] - lo ..., lo the first source row src holds
void launch_resize_rows(hipStream_t s, const uint8_t* src, size_t src_pitch, int rows, const ResizeAxis& X, int ow, uint8_t* dst, size_t dst_pitch);
void launch_resize_cols(hipStream_t s, const uint8_t* src, size_t src_pitch, int lo, const ResizeAxis& Y, int ow, int oh, uint8_t* dst,
                        size_t dst_pitch);

// LK.  p_in/p_out etc. are device pointers.  fb = fused forward+backward.
struct LKBuffers {
    const float* p_in;   // (n,2)
    float* p_fwd;        // (n,2) forward result (in/out when INITIAL_FLOW)
    uint8_t* st_fwd;
    float* err_fwd;
    float* p_bwd;        // fb only
    uint8_t* st_bwd;
    float* err_bwd;
    float* dist;
    uint8_t* valid;
    const int* n_dev;    // optional device-side count (overrides n when non-null)
    const int* order;    // optional launch order (k_tracks.hip k_seg_order); results do not depend on it
    int order_plain;     // walk the order table linearly instead of dealing it to the XCDs (dense features)
    const int* order_border;   // number of leading table entries that are border features: launched first, undealt
    // Segment mode (icelk_seg_track): the launch itself keeps the track table.  Feature f is track f of the
    // segment; dead tracks (seg_alive[f] == 0) exit at once, survivors of the forward-backward test get their
    // new vertex and distance appended and their position updated in place -- the Python loop of
    // s1_lucaskanade_tracking.py:335-359 without a separate compaction launch.
    uint8_t* seg_alive;
    float* seg_xy;               // (n,2) current position of every track; also the input points in this mode
    float* seg_tracks;           // [track][max_vert][2]
    float* seg_quality;          // [track][max_vert-1]
    int seg_vert, seg_max_vert;  // vertex written by this launch
    unsigned long long* seg_tracked;   // 64 sharded counters: features tracked (for throughput accounting)
    // diagnostics (ICELK_LK_STAMPS=<file>): per workgroup {s_memtime at entry, at exit, HW_ID | XCC_ID << 32}
    unsigned long long* stamps;
    // measurement (icelk_prof_enable): LK iterations each feature ran, forward pass in the low half, backward in the high
    uint32_t* iters;
    // Template reuse across the pairs of a segment (window-specialised kernels only; see k_lk_fast.hip): the BACKWARD pass
    // of pair v builds, at every level, the template of frame v+1 at the position the forward pass of pair v+1 starts
    // from -- the same patch, derivatives and 2x2 matrix.  tmpl_out: where the backward pass leaves them; tmpl_in: where
    // the forward pass of this launch finds the ones of the launch before (null: built here).
    // Layout: [track][level][quad][lane] 16-byte pieces; the dword behind a lane's template carries A11 / A12 / A22 (lanes 0-2).
    void* tmpl_out;
    const void* tmpl_in;
    int tmpl_levels;     // levels per track in those tables (top_level + 1 of the launch that wrote them)
};
// 16-byte pieces per lane and level of a stored template for this window (0: no window-specialised kernel, no reuse)
int lk_template_quads(int win_w, int win_h);
// will launch_lk / launch_lk_pair run the window-specialised one-feature-per-wave kernel for these parameters?
bool lk_fast_eligible(const LKParams& P);
// search-tile margin of the window-specialised tracker kernels (lk_fast_tiles.h); the host needs it to tell which features'
// tiles reach over the frame border
constexpr int kLkTileMargin = 1;
// one tracker job: a frame pair and the features tracked across it
struct LKJob {
    Pyramid I, J;
    LKBuffers B;
    int n;
};
size_t lk_lds_bytes(const LKParams& P);
int launch_lk(hipStream_t s, const Pyramid& I, const Pyramid& J, const LKBuffers& B, int n, const LKParams& P,
              bool fb);
// Two INDEPENDENT jobs with the same LK parameters in one launch (the last pair of a closing segment and the first pair
// of the next one: s1:362,440 make them independent): ramp-up and tail of the launch are paid once for both.  Returns
// false when no kernel for this window takes two jobs (the caller then launches them one after the other).
bool launch_lk_pair(hipStream_t s, const LKJob& a, const LKJob& b, const LKParams& P);

// Detector stages.
// A candidate buffer: what the corner kernel writes (launch_candidates) and the stages behind it read.  Three exist
// (Ctx::EigOut in icelk_ctx.h); a detector scratch carries a copy of the one it works on.
struct CandBuf {
    unsigned long long* raw;   // candidate regions written by the corner kernel
    int* blk_count;        // candidates per producer workgroup (region layout, see k_corners.hip; corner_keys.h: the keys)
    unsigned* max_key;     // 1 (order-preserving key of the masked maximum)
    // two-pass detector (k_corners_fast.hip): what its integer pass hands to its exact passes -- per tile the pixels that can
    // be a local maximum {y << 16 | x, upper bound} and those that can carry the maximum, the tile's largest upper bound,
    // and the largest lower bound of the whole frame
    uint2 *acand, *amaxc;
    int *acount, *amaxn;
    float* aemax;
    unsigned* fmax_key;      // [0] largest lower bound of the frame, [1] entries in aties
    unsigned* aties;         // pixels (y << 16 | x) whose neighbourhood the exact pass must look at; 0x80000000 | tile: whole tile
    int nblk, region;        // geometry of the candidate regions the buffer holds
};
struct DetectScratch {
    float* eig;            // w*h
    CandBuf cb;            // the candidate buffer of the detection in flight
    unsigned long long* cand;   // candidate keys (value bits << 32 | raster index)
    int* cand_count;       // 1
    int cand_cap;
    int* cell_count;       // grid cells + 1
    int* cell_start;       // grid cells + 1
    int* cell_fill;        // grid cells
    int* chunk_tot;        // candidates per 2048 cells (offsets of the scan's workgroups)
    unsigned long long* cell_cand;  // candidates grouped by cell
    uint8_t* state;        // per grouped candidate: 0 undecided, 1 accepted, 2 rejected
    int* undecided;        // 1
    unsigned long long* acc;   // accepted keys
    unsigned long long* acc_sorted;
    int* acc_count;        // 1
    void* sort_tmp;
    size_t sort_tmp_bytes;
    unsigned* key_hist;    // histogram of the response keys (top-K pruning); 65536 entries allocated
    unsigned* prune_key;   // 1: candidates with a smaller response key are ignored (0 = none)
    // device-driven tail (k_tail.hip): control words (TailCtl), response-bin histogram / offsets / cursors, histogram of the launch order
    int* tail_ctl;
    int* tail_resp;
    int* tail_bins;
};
// k_tail.hip: words of DetectScratch::tail_ctl
enum TailCtl { TC_TICKET_GATHER = 0, TC_TICKET_RANK, TC_TICKET_ORDER, TC_NOUT, TC_STATUS, TC_CAND, TC_ACC, TC_UNDECIDED, TC_PRUNED, TC_WORDS_ = 16 };
// verdict of the device-driven tail (CW_STATUS): anything but TAIL_OK leaves the tail to the host (detect_finish)
enum TailStatus { TAIL_OK = 0, TAIL_UNDECIDED = 1, TAIL_PRUNED_SHORT = 2, TAIL_OVERFLOW = 3, TAIL_SKEWED = 4 };
// Words of a detector set's pinned counts (Ctx::DetSet::h_counts).  k_publish_counts (abi_detect.hip) writes the first four,
// the last workgroup of k_tail_order (k_tail.hip) the first six; then either stores the publication's sequence number in
// CW_SEQ, which the host polls.  CW_NOUT and CW_STATUS keep what the latest tail left there when k_publish_counts
// publishes: the host looks at them only for a job whose dev_tail is set.
enum CountsWord { CW_CAND = 0, CW_ACC, CW_UNDECIDED, CW_PRUNED, CW_NOUT, CW_STATUS, CW_SEQ = 8, CW_WORDS_ = 16 };
constexpr int kTailOrderBins = 8192;
constexpr int kTailRespBins = 4096;
struct TailOrderGeo {   // cells of the launch order (k_tracks.hip k_seg_order): bin 0 = border features
    int cw_shift, ch_shift, cells_x, ncells, w, h, border_px;
};
struct DetectCounters {  // the counters of a detector set: what a detection leaves zeroed for the next one (corner_keys.h reset_counters)
    int* cell_count;
    int* cell_fill;
    int ncell;
    int* chunk_tot;
    int* undecided;
    int* acc_count;
    int* cand_count;
    unsigned* max_key;
    unsigned* key_hist;
    unsigned* prune_key;
};
TailOrderGeo tail_order_geometry(int w, int h, int border_px);
size_t tail_resp_words();
DetectCounters tail_reset_of(DetectScratch& D, int ncell);   // k_min_distance.hip
// the accepted candidates -> D.acc (what k_gather_accepted does) + their response-bin histogram, bin offsets and the verdict
void launch_tail_gather(hipStream_t s, DetectScratch& D, int ncell, double quality, int undecided_index, int max_corners,
                        int cap, int force_status);
// rank + corner tables of the new segment + launch order + counter reset + counts to the host, all from device-side counts
void launch_tail_device(hipStream_t s, DetectScratch& D, double quality, float* seg_xy, uint8_t* seg_alive, float* seg_tracks,
                        int max_vert, int* order, int* order_border, const TailOrderGeo& geo, const DetectCounters& rs,
                        int* host_counts, int seq);
// The corner response a candidate stage computes (icelk_set_detector; k_corners.hip harris_of: the arithmetic)
struct Response {
    int kind = 0;     // ICELK_DETECTOR_MIN_EIG | ICELK_DETECTOR_HARRIS
    double k = 0;     // Harris: the free parameter; not read for the smaller eigenvalue
    int tail = 0;     // Harris: icelk_set_variant "harris_tail" (the any-blockSize kernel only)
    bool operator==(const Response& o) const { return kind == o.kind && k == o.k && tail == o.tail; }
};
void launch_min_eig(hipStream_t s, const Level& img, int block_size, float* eig, const uint8_t* mask,
                    int mask_pitch, unsigned* max_key, int variant = 0, const Response& resp = Response{});
bool fused_block_size(int bs);
// mode: 0 = the cell grid and the counters; | 1 = the key histogram too; | 2 = and the masked maximum D.cb.max_key (only where
// the candidate buffer behind it is known to be this detection's: it may have been handed on since)
void launch_detect_reset(hipStream_t s, DetectScratch& D, int ncell, int mode);
// K6+K7: local maxima into per-workgroup regions of D.cb.raw (stream order, no host sync)
void launch_candidates(hipStream_t s, DetectScratch& D, const Level& img, int block_size, const uint8_t* mask,
                       int mask_pitch, double quality, bool use_generic, float* eig_out_or_null, int variant = 0,
                       const Response& resp = Response{});
// K6 + K7 in two passes for blockSize 3 / 5 / 7 / 10 (integer bracket of the map, exact arithmetic at the possible maxima
// only): same regions, counts and max_key as launch_candidates' one-pass kernel.  quality <= 0: no threshold cut.
bool launch_candidates_fast(hipStream_t s, DetectScratch& D, const Level& img, int block_size, const uint8_t* mask,
                            int mask_pitch, double quality);
size_t fast_tiles(int w, int h);
size_t fast_cand_entries(int w, int h);
size_t fast_max_entries(int w, int h);
size_t fast_key_capacity(int w, int h);
size_t fast_regions(int w, int h);
size_t candidate_capacity(int w, int h);   // keys the region layout needs
size_t candidate_blocks(int w, int h);
// k_min_distance.hip.  minDistance < 1: candidates above the threshold, flat in D.cand / D.cand_count
void launch_flatten(hipStream_t s, DetectScratch& D, double quality);
// K8: regions -> D.acc / D.acc_count (unsorted accepted keys); candidates counted in D.cell_start[ncell];
// D.undecided[suppress_launch_count()-1] != 0 afterwards means the relaxation has not converged yet: call
// continue_min_distance and look again.
// prune_want > 0: only the ~prune_want strongest candidates take part (valid iff the accepted ones reach maxCorners)
// no_gather: the caller gathers the accepted candidates itself (launch_tail_gather: the device-driven tail)
void launch_min_distance(hipStream_t s, DetectScratch& D, int w, int h, double min_distance, double quality,
                         int prune_want, bool no_gather = false);
void continue_min_distance(hipStream_t s, DetectScratch& D, int w, int h, double min_distance);
int suppress_launch_count();
size_t sort_tmp_bytes(int n);
void sort_keys_desc(hipStream_t s, DetectScratch& D, const unsigned long long* in, unsigned long long* out,
                    int n);
void launch_emit_corners(hipStream_t s, const unsigned long long* keys, int n, int w, float* xy);
// corner list + the new segment's tables + the detector set's counter reset in one launch (k_tail)
void launch_tail_fused(hipStream_t s, const unsigned long long* keys, int n, float* corners, float* seg_xy,
                       uint8_t* seg_alive, float* seg_tracks, int max_vert, DetectScratch& D, int ncell, int mode);

// Segment bookkeeping (k_tracks.hip).
void launch_fb_filter(hipStream_t s, const float* p0, const float* p0r, int n, float thr, int form, float* dist,
                      uint8_t* valid);
void launch_seg_init(hipStream_t s, const float* corners, int n, float* xy, uint8_t* alive, float* tracks,
                     int max_vert);
// projection epilogue (k_utm.hip); the structs are the public ones
typedef icelk_camera_t UtmCamera;
typedef icelk_utm_filter_t UtmFilter;
void launch_project_tracks(hipStream_t s, const float* tracks, int n, int nv, const UtmCamera& cam, const UtmFilter& f,
                           double* x, double* y, double* u, double* v, double* speed, uint8_t* keep);
void launch_points_in_polygon(hipStream_t s, const double* poly, int n, const double* pts, int m, uint8_t* out);
void launch_grid_assign(hipStream_t s, const double* x, const double* y, int n, double left, double top, double spacing,
                        int cols, int rows, const uint8_t* cell_on, unsigned long long* keys, int* key_count, int key_cap);
void launch_grid_day_assign(hipStream_t s, const double* x, const double* y, const double* t, int n,
                            const long long* file_off, const int* file_cam, const int* win_f0, const int* win_f1,
                            int nfiles, const long long* t_lo, const long long* t_hi, int ncam, int nw, double left,
                            double top, double spacing, int cols, int rows, const uint8_t* cell_on,
                            unsigned long long* keys, int* key_count, int key_cap, int* sel_count,
                            unsigned long long* t_min, unsigned long long* t_max);
// boxes that are no lattice (transects, moorings): nboxes polygons, box b's nvert-in-all vertices at box_xy[2 * box_off[b]]
// .. ; key segment = box, or window * nboxes + box.  rot: NULL, or {cos, sin} -- then the kernel also writes u c + v s and
// v c - u s of every point into ur, vr (what the reduce is then given); dynamic LDS: 16 nvert + 20 nboxes + 4 bytes
void launch_boxes_assign(hipStream_t s, const double* x, const double* y, int n, const double* box_xy, const int* box_off,
                         int nboxes, int nvert, const double* u, const double* v, double* ur, double* vr, const double* rot,
                         unsigned long long* keys, int* key_count, int key_cap);
void launch_boxes_day_assign(hipStream_t s, const double* x, const double* y, const double* t, int n,
                             const long long* file_off, const int* file_cam, const int* win_f0, const int* win_f1,
                             int nfiles, const long long* t_lo, const long long* t_hi, int ncam, int nw,
                             const double* box_xy, const int* box_off, int nboxes, int nvert, const double* u,
                             const double* v, double* ur, double* vr, const double* rot, unsigned long long* keys,
                             int* key_count, int key_cap, int* sel_count, unsigned long long* t_min,
                             unsigned long long* t_max);
void launch_grid_reduce(hipStream_t s, const unsigned long long* keys, const int* key_count, const double* u,
                        const double* v, int ncells, int* count, double* mean_u, double* mean_v, double* speed);
// per-segment std, median and MAD (grid_stats.h): the segment table, then one thread / one workgroup per segment.  `out`
// holds device pointers; scratch: 2 * scratch_stride keys, scratch_stride >= the key count
void launch_grid_segments(hipStream_t s, const unsigned long long* keys, const int* key_count, int nseg, int* seg_begin,
                          int* seg_count, const icelk_grid_stats_t& out);
void launch_grid_std(hipStream_t s, const unsigned long long* keys, const int* seg_begin, const int* seg_count,
                     const double* u, const double* v, int nseg, const double* mean_u, const double* mean_v,
                     const icelk_grid_stats_t& out);
void launch_grid_select(hipStream_t s, const unsigned long long* keys, const int* seg_begin, const int* seg_count,
                        const double* u, const double* v, int nseg, unsigned long long* scratch, size_t scratch_stride,
                        const icelk_grid_stats_t& out);
// the normalised median test (k_validate.hip; the rules are validate.h's).  Device pointers throughout: x, y, u, v, status, r2
// and keys n each; `sorted` the keys in ascending order (the caller's sort; `keys` itself for fewer than two); cells' five
// arrays ngroups * cols * rows each; rejected ngroups, zeroed by the caller; group NULL: group 0 (the day form takes the
// window of the day tables instead); t_kill NULL, or the times that become NaN at every rejected point.  `total`: the judged
// points, what key_count holds after the assign kernel.
struct ValidateArgs {
    const double *x, *y, *u, *v;
    int n;
    const int32_t* group;
    int ngroups;
    icelk_validate_lattice_t L;
    icelk_validate_params_t P;
    unsigned long long* keys;
    const unsigned long long* sorted;
    int* key_count;
    uint8_t* status;
    double* r2;
    icelk_validate_cells_t cells;
    int32_t* rejected;
    double* t_kill;
};
void launch_validate_assign(hipStream_t s, const ValidateArgs& A);
void launch_validate_day_assign(hipStream_t s, const ValidateArgs& A, const double* t, const long long* file_off, const int* file_cam,
                                const int* win_f0, const int* win_f1, int nfiles, const long long* t_lo, const long long* t_hi, int ncam,
                                int nw);
void launch_validate_pools(hipStream_t s, const ValidateArgs& A, int total);
void launch_validate_judge(hipStream_t s, const ValidateArgs& A, int total);
int validate_pool_lds_terms();   // the largest pool whose order keys are staged in LDS
// averages of the velocity cube (k_cube.hip): the cube [window][cell], the periods' windows as CSR offsets + indices
void launch_cube_temporal(hipStream_t s, const double* u, const double* v, const double* cnt, int ncells,
                          const int* sel_offset, const int* sel_index, int nperiods, double* mean_u, double* mean_v,
                          double* speed, double* count_sum, int* has_data);
void launch_cube_spatial(hipStream_t s, const double* mean_u, const double* mean_v, const double* count_sum, int rows,
                         int cols, int coarseness, int nperiods, double* out_u, double* out_v, double* out_speed,
                         double* out_count);
// the per-cell harmonic fit of the cube (k_tides.hip; the rules are tides.h's).  Device pointers throughout.  u, v, count: the
// cube [window][cell]; basis [nt][m]; part [sum][chunk][cell], ipart [n | first | last][chunk][cell], tot [sum][cell], mean [u |
// v][cell], part2 [res u | res v | tot u | tot v][chunk][cell]; coef [cell][m]; the other outputs one per cell; res_u, res_v
// NULL or [window][cell].
struct TideArgs {
    const double *u, *v, *count;
    int ncells, nt;
    const double* basis;
    int m;
    double min_count;
    int min_samples;
    double* part;
    int32_t* ipart;
    double *tot, *mean, *part2;
    double *coef_u, *coef_v, *rms_u, *rms_v, *explained_u, *explained_v;
    int32_t *n, *first, *last, *status;
    double *res_u, *res_v;
};
void launch_tide_normal(hipStream_t s, const TideArgs& A);
void launch_tide_solve(hipStream_t s, const TideArgs& A);
void launch_tide_residual(hipStream_t s, const TideArgs& A);
void launch_tide_finish(hipStream_t s, const TideArgs& A);
// out_u, out_v [ntp][cell] from coef [cell][m], status [cell] and basis [ntp][m]; NaN where status != 0
void launch_tide_predict(hipStream_t s, const double* coef_u, const double* coef_v, const int32_t* status, int ncells, int m,
                         const double* basis, int ntp, double* out_u, double* out_v);
// virtual drifters (k_drift.hip; the rule and the fields are drift.h's).  Device pointers throughout: the field's tables, the
// seeds and release steps of the n drifters, the outputs x, y [n_out][n] and one per drifter.
namespace drift {
struct CubeField;
struct TideField;
struct Out;
}  // namespace drift
struct DriftSeeds {
    const double *x, *y;
    const int32_t* release;
    int n;
};
void launch_drift_cube(hipStream_t s, const icelk_drift_lattice_t& L, const icelk_drift_params_t& P, const drift::CubeField& F,
                       const DriftSeeds& S, const drift::Out& O);
void launch_drift_tide(hipStream_t s, const icelk_drift_lattice_t& L, const icelk_drift_params_t& P, const drift::TideField& F,
                       const DriftSeeds& S, const drift::Out& O);
// visits [rows][cols], zeroed by the caller: += 1 at the nearest node of every finite sample of x, y [samples]
void launch_drift_visits(hipStream_t s, const icelk_drift_lattice_t& L, const double* x, const double* y, int samples, int32_t* visits);
// the calibration misfit (k_calib.hip): candidates of 11 doubles (X, U, V, sigma in pixels, H), shoreline points
// (xi, yi) relative to the image centre, waterline vertices (x, y); out_tx / out_ty may be null
void launch_calib_residuals(hipStream_t s, const double* cand, int P, const double* shore, int M, const double* water,
                            int W, double E, double N, double* out_dist, double* out_tx, double* out_ty);
void launch_calib_cost(hipStream_t s, const double* cand, int P, const double* shore, int M, const double* water, int W,
                       double E, double N, double* out_meansq);
int calib_cost_max_points();   // the most shoreline points launch_calib_cost takes
size_t sort_keys_asc(hipStream_t s, void* tmp, size_t tmp_bytes, const unsigned long long* in, unsigned long long* out,
                     int n, int end_bit);
void launch_polygon_mask(hipStream_t s, const double* poly, int n, double crop_left, double crop_top, int w, int h,
                         uint8_t* mask, int pitch);
void launch_seg_order(hipStream_t s, const float* xy, int n, int w, int h, int border_px, int* order, int* border_count);
// {alive tracks, features tracked so far} -> host_out[0..1] (pinned, 64-bit each)
void launch_seg_stats(hipStream_t s, const uint8_t* alive, int n, const unsigned long long* tracked_shards,
                      unsigned long long* host_out);
// rows of the alive tracks, in track order, packed into out_tracks (n_alive, nvert, 2) / out_quality
void launch_seg_gather(hipStream_t s, const uint8_t* alive, int n, const float* tracks, const float* quality,
                       int nvert, int max_vert, float* out_tracks, float* out_quality, int* out_count = nullptr);
size_t min_eig_lds_bytes(int block_size);

}  // namespace icelk
