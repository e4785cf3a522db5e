// k_min_distance.hip -- the selection stage (K8) of the Shi-Tomasi corner detector: from the candidate regions the
// corner kernel leaves (k_corners.hip, or its two-pass form k_corners_fast.hip) to the corner list.
//
// Replaces the part of cv2.goodFeaturesToTrack behind the local maxima (s1_lucaskanade_tracking.py:437): the quality
// threshold, the minDistance rule, the maxCorners cut.
//   K8 min distance: OpenCV accepts candidates greedily in response order.  Equivalent parallel form: a
//         candidate is accepted iff no ACCEPTED candidate of higher priority lies closer than minDistance;
//         relax "reject if an accepted stronger neighbour exists / accept if every stronger neighbour is
//         rejected" to the fixed point over a cell grid of round(minDistance) px (3x3 cell search, as OpenCV's
//         grid).  Only the accepted set is sorted (k_sort.hip).
// Also here: the reset of a detector set's counters (k_detect_reset; the one statement of what is reset is
// reset_counters in corner_keys.h, which k_tail.hip calls too), the corner list from sorted keys (k_emit) and the host's
// tail in one launch (k_tail).  The tail driven by the device is k_tail.hip.
// The whole detection is enqueued without host round trips; the host synchronises once, to learn the
// number of accepted corners.
#include <cmath>

#include "corner_keys.h"

namespace icelk {

namespace {

// workgroup-aggregated append: every thread offers at most one key per call; one global atomic per call
__device__ __forceinline__ void block_append(bool keep, unsigned long long key, unsigned long long* out,
                                             int* out_count, int* s_cnt, int* s_base)
{
    if (threadIdx.x == 0) *s_cnt = 0;
    __syncthreads();
    const int pos = keep ? atomicAdd(s_cnt, 1) : 0;
    __syncthreads();
    if (threadIdx.x == 0 && *s_cnt) *s_base = atomicAdd(out_count, *s_cnt);
    __syncthreads();
    if (keep) out[*s_base + pos] = key;
    __syncthreads();
}

// regions -> flat list of the candidates above max * qualityLevel (minDistance < 1 path: everything is sorted)
__global__ __launch_bounds__(256) void k_flatten(CandSrc src, const unsigned* __restrict__ max_key, double quality,
                                                 unsigned long long* __restrict__ cand, int* __restrict__ cand_count)
{
    __shared__ int s_cnt, s_base;
    const float thr = threshold_of(max_key, quality);
    for (int b = blockIdx.x; b < src.nblk; b += gridDim.x) {
        const int cnt = src.blk_count[b];
        for (int i0 = 0; i0 < cnt; i0 += 256) {
            const int i = i0 + threadIdx.x;
            unsigned long long key = 0;
            bool keep = false;
            if (i < cnt) {
                key = src.keys[(size_t)b * src.region + i];
                keep = key_to_float(cand_response_key(key)) > thr;
            }
            block_append(keep, key, cand, cand_count, &s_cnt, &s_base);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K8 helpers.
// Every kernel of the min-distance stage is launched as ONE-WAVE workgroups (CT = 64 threads) with at most 8 KB of
// LDS and no more than 128 VGPRs: that is the footprint of a single k_lk_fast wave, so while a tracker launch
// owns the chip (it holds every VGPR) such a workgroup fits into the hole any retiring tracker wave leaves and
// the stage progresses beside it; wider workgroups wait for the tracker's tail (tools/ubench/corun.hip:
// 64 threads / 4 KB LDS 30-60 us beside a register-saturating kernel, >= 128 threads or 16 KB 250-340 us).
// ------------------------------------------------------------------------------------------------
// (CT, SCAN_CHUNK, CHUNK_TOT_STRIDE: corner_keys.h)
__device__ __forceinline__ void chunk_add(int* __restrict__ chunk_tot, bool active, int chunk)
{
    unsigned long long pending = __ballot(active);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int c = __shfl(chunk, leader);
        const unsigned long long same = __ballot(active && chunk == c) & pending;
        if ((int)threadIdx.x == leader) atomicAdd(&chunk_tot[c * CHUNK_TOT_STRIDE], __popcll(same));
        pending &= ~same;
    }
}

__global__ __launch_bounds__(CT) void k_cell_count(CandSrc src, const unsigned* __restrict__ max_key, double quality,
                                                   const unsigned* __restrict__ prune_key, int w, int cell, int gw,
                                                   int* __restrict__ cell_count, int* __restrict__ chunk_tot)
{
    const float thr = threshold_of(max_key, quality);
    const unsigned pk = *prune_key;
    for (int b = blockIdx.x; b < src.nblk; b += gridDim.x) {
        const int cnt = src.blk_count[b];
        for (int i0 = 0; i0 < cnt; i0 += CT) {
            const int i = i0 + threadIdx.x;
            bool keep = false;
            int c = 0;
            if (i < cnt) {
                const unsigned long long key = src.keys[(size_t)b * src.region + i];
                keep = cand_response_key(key) >= pk && key_to_float(cand_response_key(key)) > thr;
                const unsigned xy = cand_xy(key);
                const int y = xy_y(xy), x = xy_x(xy);
                c = (y / cell) * gw + (x / cell);
            }
            if (keep) atomicAdd(&cell_count[c], 1);
            chunk_add(chunk_tot, keep, c / SCAN_CHUNK);
        }
    }
}

// ---- top-K pruning when maxCorners caps the output ------------------------------------------------
// Whether a candidate is accepted depends only on STRONGER candidates, so the accepted candidates among the K
// strongest are exactly the greedy-accepted ones among them; if they number >= maxCorners, the weaker
// candidates can never appear in the output and need not be binned, relaxed or sorted.  K is found from a
// 16384-bin histogram of the response key (its top 14 bits); the host checks "accepted >= maxCorners" at its
// one synchronisation point and reruns unpruned otherwise.
constexpr int KEY_SHIFT = 18;                 // bin width: sign, exponent and 5 mantissa bits of the key
// KEY_BINS (corner_keys.h) bins are counted DOWN from the bin of the maximum
// Responses cluster in a few hundred bins, so a global-memory histogram would serialise on a handful of L2
// atomic addresses: every workgroup histograms into LDS (8 KB) and flushes its non-empty bins.
__device__ __forceinline__ int key_bin(unsigned key, unsigned max_key)
{
    const int b = (int)(max_key >> KEY_SHIFT) - (int)(key >> KEY_SHIFT);
    return b < 0 ? 0 : (b >= KEY_BINS ? KEY_BINS - 1 : b);
}

__global__ __launch_bounds__(CT) void k_key_hist(CandSrc src, const unsigned* __restrict__ max_key, double quality,
                                                 unsigned* __restrict__ hist)
{
    __shared__ unsigned lh[KEY_BINS];
    for (int i = threadIdx.x; i < KEY_BINS; i += CT) lh[i] = 0;
    __syncthreads();
    const float thr = threshold_of(max_key, quality);
    const unsigned mk = *max_key;
    for (int b = blockIdx.x; b < src.nblk; b += gridDim.x) {
        const int cnt = src.blk_count[b];
        for (int i = threadIdx.x; i < cnt; i += CT) {
            const unsigned k = cand_response_key(src.keys[(size_t)b * src.region + i]);
            if (key_to_float(k) > thr) atomicAdd(&lh[key_bin(k, mk)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < KEY_BINS; i += CT) {
        const unsigned v = lh[i];
        if (v) atomicAdd(&hist[i], v);
    }
}

// prune_key = lowest key of the strongest bins that together hold >= want candidates (0 = keep everything).
// One wave; lane l owns bins [32 l, 32 l + 32), bin 0 being the strongest.
__global__ __launch_bounds__(CT) void k_key_select(const unsigned* __restrict__ hist, unsigned want,
                                                   const unsigned* __restrict__ max_key,
                                                   unsigned* __restrict__ prune_key)
{
    constexpr int PER = KEY_BINS / CT;
    const int lane = threadIdx.x;
    unsigned s = 0;
    for (int i = 0; i < PER; i++) s += hist[lane * PER + i];
    unsigned incl = s;   // candidates in this lane's bins and all stronger ones
#pragma unroll
    for (int o = 1; o < CT; o <<= 1) {
        const unsigned v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    const unsigned total = __shfl(incl, CT - 1);
    if (lane == 0 && total < want) *prune_key = 0u;
    const unsigned above = incl - s;
    if (above < want && incl >= want) {
        unsigned run = above;
        for (int i = 0; i < PER; i++) {
            run += hist[lane * PER + i];
            if (run >= want) {
                const int bin = lane * PER + i;   // keep bins 0..bin
                const int top = (int)(*max_key >> KEY_SHIFT);
                // the last bin also collects everything weaker: keeping it means keeping all
                *prune_key = (bin >= KEY_BINS - 1 || top - bin <= 0) ? 0u : (unsigned)(top - bin) << KEY_SHIFT;
                break;
            }
        }
    }
}

// exclusive scan of the cell counts, SCAN_CHUNK cells per one-wave workgroup: the offset of a chunk is the sum of the
// chunk totals before it (kept by k_cell_count), inside the chunk 8 rounds of 4 cells per lane.  start[n] = total.
__global__ __launch_bounds__(CT) void k_scan(const int* __restrict__ count, const int* __restrict__ chunk_tot,
                                             int* __restrict__ start, int n)
{
    const int lane = threadIdx.x;
    const int lo = blockIdx.x * SCAN_CHUNK;
    int run = 0;
    for (int c = lane; c < (int)blockIdx.x; c += CT) run += chunk_tot[c * CHUNK_TOT_STRIDE];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) run += __shfl_xor(run, o);
    for (int r = 0; r < SCAN_CHUNK / (4 * CT); r++) {
        const int i0 = lo + r * 4 * CT + 4 * lane;
        int c[4], s = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            c[k] = i0 + k < n ? count[i0 + k] : 0;
            s += c[k];
        }
        int inc = s;
#pragma unroll
        for (int o = 1; o < CT; o <<= 1) {
            const int v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        int at = run + inc - s;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (i0 + k < n) start[i0 + k] = at;
            at += c[k];
            if (i0 + k == n - 1) start[n] = at;
        }
        run += __shfl(inc, CT - 1);
    }
    if (n == 0 && blockIdx.x == 0 && lane == 0) start[0] = 0;
}

__global__ __launch_bounds__(CT) void k_cell_fill(CandSrc src, const unsigned* __restrict__ max_key, double quality,
                                                   const unsigned* __restrict__ prune_key, int w, int cell, int gw,
                                                   const int* __restrict__ cell_start, int* __restrict__ cell_fill,
                                                   unsigned long long* __restrict__ cell_cand,
                                                   uint8_t* __restrict__ state)
{
    const float thr = threshold_of(max_key, quality);
    const unsigned pk = *prune_key;
    for (int b = blockIdx.x; b < src.nblk; b += gridDim.x) {
        const int cnt = src.blk_count[b];
        for (int i = threadIdx.x; i < cnt; i += CT) {
            const unsigned long long key = src.keys[(size_t)b * src.region + i];
            if (cand_response_key(key) < pk || !(key_to_float(cand_response_key(key)) > thr)) continue;
            const int y = cand_y(key), x = cand_x(key);
            const int c = (y / cell) * gw + (x / cell);
            const int pos = cell_start[c] + atomicAdd(&cell_fill[c], 1);
            cell_cand[pos] = key;
            state[pos] = 0;
        }
    }
}

// Relaxation.  A thread owns one candidate.  Its first look scans the 3x3 cells and keeps the indices of the
// stronger candidates within minDistance that are still undecided (its "blockers") in LDS; after that it only
// polls those.  States are read and written with L1-bypassing (system-scope relaxed) accesses and only ever
// move 0 -> 1 or 0 -> 2 on final facts, so progress made by other workgroups is seen as it happens and a stale
// read merely costs another poll.  Spins are bounded; launch_counters[r] = candidates still undecided after
// launch r, and launch r+1 picks them up (it returns at once when that count is zero).
constexpr int SUP_K = 24;
constexpr int SUP_SPINS = 48;
__global__ __launch_bounds__(CT) void k_suppress(const unsigned long long* __restrict__ cell_cand,
                                                  const int* __restrict__ n_ptr, int cell, int gw, int gh,
                                                  const int* __restrict__ cell_start, uint8_t* state, double md2,
                                                  int* __restrict__ launch_counters, int r)
{
    __shared__ int blockers[SUP_K * CT];
    if (r > 0 && launch_counters[r - 1] == 0) return;
    const int n = *n_ptr;
    int* mine = blockers + threadIdx.x;   // entry q at mine[q * CT]: conflict-free
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (__atomic_load_n(&state[i], __ATOMIC_RELAXED)) continue;
        const unsigned long long key = cell_cand[i];
        const int y = cand_y(key), x = cand_x(key);
        const int xc = x / cell, yc = y / cell;
        const int x1 = max(0, xc - 1), y1 = max(0, yc - 1), x2 = min(gw - 1, xc + 1), y2 = min(gh - 1, yc + 1);
        int cnt = 0;
        bool rejected = false, overflow = false;
        for (int yy = y1; yy <= y2 && !rejected; yy++) {
            const int b = cell_start[yy * gw + x1], e = cell_start[yy * gw + x2 + 1];  // the 3 cells are contiguous
            for (int j = b; j < e; j++) {
                const unsigned long long kj = cell_cand[j];
                if (kj <= key) continue;  // only stronger candidates matter (keys are unique)
                const int yj = cand_y(kj), xj = cand_x(kj);
                const float dx = (float)(x - xj), dy = (float)(y - yj);
                if (!((double)(dx * dx + dy * dy) < md2)) continue;
                const uint8_t sj = __atomic_load_n(&state[j], __ATOMIC_RELAXED);
                if (sj == 1) { rejected = true; break; }
                if (sj == 0) {
                    if (cnt < SUP_K) mine[CT * cnt++] = j;
                    else overflow = true;
                }
            }
        }
        bool decided = false;
        if (rejected) { __atomic_store_n(&state[i], (uint8_t)2, __ATOMIC_RELAXED); decided = true; }
        else if (cnt == 0 && !overflow) { __atomic_store_n(&state[i], (uint8_t)1, __ATOMIC_RELAXED); decided = true; }
        for (int spin = 0; spin < SUP_SPINS && !decided && !overflow; spin++) {
            __builtin_amdgcn_s_sleep(8);
            int k = 0;
            for (int q = 0; q < cnt; q++) {
                const int j = mine[CT * q];
                const uint8_t sj = __atomic_load_n(&state[j], __ATOMIC_RELAXED);
                if (sj == 1) { rejected = true; break; }
                if (sj == 0) mine[CT * k++] = j;
            }
            cnt = k;
            if (rejected) { __atomic_store_n(&state[i], (uint8_t)2, __ATOMIC_RELAXED); decided = true; }
            else if (cnt == 0) { __atomic_store_n(&state[i], (uint8_t)1, __ATOMIC_RELAXED); decided = true; }
        }
        if (!decided) atomicAdd(&launch_counters[r], 1);
    }
}

// zero every counter a detection uses, in one launch (each hipMemsetAsync is a ~5 us kernel of its own)
__global__ void k_detect_reset(DetectCounters dc, int mode)
{
    reset_counters(dc, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, mode);
}

__global__ __launch_bounds__(CT) void k_gather_accepted(const unsigned long long* __restrict__ cell_cand,
                                                         const int* __restrict__ n_ptr,
                                                         const uint8_t* __restrict__ state,
                                                         unsigned long long* __restrict__ acc,
                                                         int* __restrict__ acc_count)
{
    __shared__ int s_cnt, s_base;
    const int n = *n_ptr;
    for (int i0 = blockIdx.x * CT; i0 < n; i0 += gridDim.x * CT) {
        const int i = i0 + threadIdx.x;
        const bool keep = i < n && state[i] == 1;
        block_append(keep, keep ? cell_cand[i] : 0ull, acc, acc_count, &s_cnt, &s_base);
    }
}

__global__ void k_emit(const unsigned long long* __restrict__ keys, int n, int w, float* __restrict__ xy)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    xy[2 * i] = (float)cand_x(key);
    xy[2 * i + 1] = (float)cand_y(key);
}

// The tail of a detection whose corners start a segment, in ONE launch instead of three (k_emit, k_detect_reset,
// k_seg_init): every launch of the tail has to find room beside a tracker launch -- or beside a corner kernel that has the
// chip to itself -- and the next tracker launch waits for the last of them.  Blocks [0, emit_blocks): corner i from its
// sorted key -> the corner list AND the new segment's tables (position, alive flag, vertex 0 of its track); the blocks
// behind them: the counters of the detector set for its next detection (mode as launch_detect_reset).
__global__ __launch_bounds__(CT) void k_tail(const unsigned long long* __restrict__ keys, int n, float* __restrict__ corners,
                                             float* __restrict__ seg_xy, uint8_t* __restrict__ seg_alive,
                                             float* __restrict__ seg_tracks, int max_vert, int emit_blocks, DetectCounters dc,
                                             int mode)
{
    if ((int)blockIdx.x < emit_blocks) {
        const int i = blockIdx.x * CT + threadIdx.x;
        if (i >= n) return;
        const unsigned long long key = keys[i];
        const float x = (float)cand_x(key), y = (float)cand_y(key);
        corners[2 * i] = x; corners[2 * i + 1] = y;
        seg_xy[2 * i] = x; seg_xy[2 * i + 1] = y;
        seg_alive[i] = 1;
        seg_tracks[((size_t)i * max_vert) * 2] = x;
        seg_tracks[((size_t)i * max_vert) * 2 + 1] = y;
        return;
    }
    reset_counters(dc, ((int)blockIdx.x - emit_blocks) * CT + threadIdx.x, ((int)gridDim.x - emit_blocks) * CT, mode);
}

// one-wave workgroups that reset the counters of a grid of ncell cells (and the key histogram, mode & 1)
int reset_blocks(int ncell, int mode)
{
    int blocks = (ncell + CT) / CT;
    if ((mode & 1) && blocks < KEY_BINS / CT) blocks = KEY_BINS / CT;
    return blocks > 2048 ? 2048 : blocks;
}

}  // namespace

// the counters of the detector set D belongs to, for a grid of ncell cells
DetectCounters tail_reset_of(DetectScratch& D, int ncell)
{
    DetectCounters r{};
    r.cell_count = D.cell_count;
    r.cell_fill = D.cell_fill;
    r.ncell = ncell;
    r.chunk_tot = D.chunk_tot;
    r.undecided = D.undecided;
    r.acc_count = D.acc_count;
    r.cand_count = D.cand_count;
    r.max_key = D.cb.max_key;
    r.key_hist = D.key_hist;
    r.prune_key = D.prune_key;
    return r;
}

// First launch of every detection: zero the counters (ncell = 0 when minDistance < 1).
// full = also the response maximum and the key histogram (i.e. everything a NEW detection needs); !full = only
// what a re-run of the min-distance stage on the same candidates needs.
void launch_detect_reset(hipStream_t s, DetectScratch& D, int ncell, int mode)
{
    hipLaunchKernelGGL(k_detect_reset, dim3(reset_blocks(ncell, mode)), dim3(CT), 0, s, tail_reset_of(D, ncell), mode);
}

// minDistance < 1: every candidate above the threshold, flat in D.cand / D.cand_count
void launch_flatten(hipStream_t s, DetectScratch& D, double quality)
{
    hipLaunchKernelGGL(k_flatten, dim3(512), dim3(256), 0, s, cand_src_of(D.cb), D.cb.max_key, quality, D.cand, D.cand_count);
}

// Greedy-equivalent min-distance selection, fully enqueued (no host round trip): candidate regions ->
// D.acc (unsorted accepted keys), D.acc_count; the number of thresholded candidates ends in
// D.cell_start[ncell].  D.undecided[kSuppressLaunches-1] != 0 afterwards means "not converged, call
// continue_min_distance".
// Three launches since round 4 (two before): one detection in a hundred left one or two candidates undecided after the
// second (their blockers were decided in the same launch, after the last poll) and went through the host's tail
// (detect_finish: more launches, a host round trip each, rocPRIM's sort) instead of the device's -- 300 us, and 8 ms the
// first time in a process (profiles/r04_c3_stall.txt).  A third launch picks up what the second left and returns at once
// when that is nothing; the follow-up launches use a small grid (a handful of candidates, every workgroup scans the list).
constexpr int kSuppressLaunches = 3;
static void suppress_launches(hipStream_t s, DetectScratch& D, int w, int h, double min_distance)
{
    const int cell = (int)lrint(min_distance);
    const int gw = (w + cell - 1) / cell, gh = (h + cell - 1) / cell;
    const double md2 = min_distance * min_distance;
    for (int r = 0; r < kSuppressLaunches; r++)
        hipLaunchKernelGGL(k_suppress, dim3(r < 2 ? 4096 : 512), dim3(CT), 0, s, D.cell_cand, D.cell_start + gw * gh, cell, gw, gh,
                           D.cell_start, D.state, md2, D.undecided, r);
}

static void gather_launch(hipStream_t s, DetectScratch& D, int ncell)
{
    hipLaunchKernelGGL(k_gather_accepted, dim3(1024), dim3(CT), 0, s, D.cell_cand, D.cell_start + ncell, D.state, D.acc,
                       D.acc_count);
}

void launch_min_distance(hipStream_t s, DetectScratch& D, int w, int h, double min_distance, double quality,
                         int prune_want, bool no_gather)
{
    const int cell = (int)lrint(min_distance);
    const int gw = (w + cell - 1) / cell, gh = (h + cell - 1) / cell;
    const int ncell = gw * gh;
    const CandSrc src = cand_src_of(D.cb);
    if (prune_want > 0) {
        hipLaunchKernelGGL(k_key_hist, dim3(256), dim3(CT), 0, s, src, D.cb.max_key, quality, D.key_hist);
        hipLaunchKernelGGL(k_key_select, dim3(1), dim3(CT), 0, s, D.key_hist, (unsigned)prune_want, D.cb.max_key, D.prune_key);
    }
    hipLaunchKernelGGL(k_cell_count, dim3(4096), dim3(CT), 0, s, src, D.cb.max_key, quality, D.prune_key, w, cell, gw,
                       D.cell_count, D.chunk_tot);
    hipLaunchKernelGGL(k_scan, dim3((ncell + SCAN_CHUNK - 1) / SCAN_CHUNK), dim3(CT), 0, s, D.cell_count, D.chunk_tot,
                       D.cell_start, ncell);
    hipLaunchKernelGGL(k_cell_fill, dim3(4096), dim3(CT), 0, s, src, D.cb.max_key, quality, D.prune_key, w, cell, gw,
                       D.cell_start, D.cell_fill, D.cell_cand, D.state);
    suppress_launches(s, D, w, h, min_distance);
    if (!no_gather) gather_launch(s, D, ncell);
}

// more relaxation launches + a fresh gather (only when the first batch left candidates undecided)
void continue_min_distance(hipStream_t s, DetectScratch& D, int w, int h, double min_distance)
{
    const int cell = (int)lrint(min_distance);
    const int ncell = ((w + cell - 1) / cell) * ((h + cell - 1) / cell);
    hipMemsetAsync(D.undecided, 0, sizeof(int) * 8, s);
    hipMemsetAsync(D.acc_count, 0, sizeof(int), s);
    suppress_launches(s, D, w, h, min_distance);
    gather_launch(s, D, ncell);
}

int suppress_launch_count() { return kSuppressLaunches; }

void launch_tail_fused(hipStream_t s, const unsigned long long* keys, int n, float* corners, float* seg_xy,
                       uint8_t* seg_alive, float* seg_tracks, int max_vert, DetectScratch& D, int ncell, int mode)
{
    const int emit_blocks = (n + CT - 1) / CT;
    hipLaunchKernelGGL(k_tail, dim3(emit_blocks + reset_blocks(ncell, mode)), dim3(CT), 0, s, keys, n, corners, seg_xy, seg_alive,
                       seg_tracks, max_vert, emit_blocks, tail_reset_of(D, ncell), mode);
}

void launch_emit_corners(hipStream_t s, const unsigned long long* keys, int n, int w, float* xy)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_emit, dim3((n + CT - 1) / CT), dim3(CT), 0, s, keys, n, w, xy);
}

}  // namespace icelk
