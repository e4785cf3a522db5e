// k_jpeg_huff.hip -- Huffman decoding of a baseline JPEG's scan on gfx950: the file's bytes -> quantised DCT
// coefficients in the layout k_jpeg_idct reads.  The algorithm (self-synchronising lanes) and every function that
// touches the stream are jpeg_lanes.h, which the host runs too; this file is who calls them where.
//
//   k_jpeg_huff_sync    phase 1.  One workgroup = one group of 256 lanes = 256 consecutive subsequences; the group's entry
//                       states and block counts live in LDS for the launch.  Round 0: every lane decodes its own
//                       subsequence from its guess and carries on into the following ones, in lockstep steps with a
//                       workgroup barrier between them, until it falls in step.  Round r > 0: a group whose first entry
//                       state the group in front has changed runs ONE chain from its first lane; every other workgroup
//                       returns after two loads.  Rounds are launches: no workgroup waits for another inside one.
//   k_jpeg_huff_scan    phase 2.  Exclusive prefix sum of the blocks completed per lane (one workgroup).
//   k_jpeg_huff_write   phase 3.  Every lane decodes its subsequence once more from its true state and scatters the
//                       non-zero coefficients as 2-byte stores, DC as the difference.
//   k_jpeg_dc_*         the DC differences summed up in scan order inside every restart interval: per-chunk sums, a
//                       prefix sum of the chunk sums, and the pass that writes the values.
//   k_jpeg_huff_verdict the asynchronous ingest only (abi_jpeg_job.hip): what the host reads from ctl[] between the
//                       phases of a synchronous file, worked out at the end of the chain and published to pinned words.
//
// Divergence.  Lanes of a wave decode different bits, so they diverge at every symbol by nature; what is kept uniform
// is everything around it.  The Huffman tables (8 x 1416 B) sit in LDS; a lane's bit window is refilled with one
// 4-byte load at whatever byte it stands (byte by byte only next to an FF); the by-value arguments are indexed by no
// lane's own value, so nothing goes through scratch.  A larger S means fewer lanes (less occupancy, longer serial
// stretches), a smaller one more lanes out of step and more hops.
#include "icelk_internal.h"

namespace icelk {

using namespace lanes;

__device__ __forceinline__ void tables_to_lds(HuffTable* dst, const HuffTable* src)
{
    static_assert(sizeof(HuffTable) % 4 == 0, "copied as dwords");
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(dst);
    for (uint32_t k = threadIdx.x; k < sizeof(HuffTable) * kTables / 4; k += blockDim.x) d[k] = s[k];
}

__global__ __launch_bounds__(kGroup) void k_jpeg_huff_sync(JpegHuffArgs H, int round)
{
    __shared__ HuffTable tabs[kTables];
    __shared__ uint64_t T[kGroup];
    __shared__ uint32_t cnt[kGroup];
    __shared__ uint64_t x_out;
    __shared__ uint32_t red[3];   // bound, max hops, total hops
    const uint32_t g = blockIdx.x, g0 = g * kGroup, g1 = min(H.A.nlanes, g0 + kGroup);
    const uint32_t t = threadIdx.x, i = g0 + t;
    uint64_t* Xprev = H.X + (size_t)((round + 1) & 1) * H.ngroups;
    uint64_t* Xcur = H.X + (size_t)(round & 1) * H.ngroups;
    Chain c;
    c.s = 0;
    c.seg = 0;
    c.hops = 0;
    c.active = c.bound = false;
    if (round == 0) {
        if (i < g1) {
            c.s = initial_state(H.A, H.data, H.seg, i, &c.seg);
            c.active = true;
            T[t] = c.s;
            cnt[t] = 0;
        }
        if (t == 0) x_out = kNoState;
    } else {
        // the same for the whole workgroup: has the group in front handed over another state than the one in place?
        const uint64_t e = g ? Xprev[g - 1] : kNoState;
        if (e == kNoState || e == H.T[g0]) {
            if (t == 0) Xcur[g] = Xprev[g];
            return;
        }
        if (i < g1) {
            T[t] = H.T[i];
            cnt[t] = H.cnt[i];
        }
        if (t == 0) {
            x_out = Xprev[g];
            c.s = e;
            c.seg = segment_of(H.seg, H.A.nseg, g0);
            c.active = true;
            H.ctl[JH_ROUND0 + round] = 1;
        }
    }
    if (t < 3) red[t] = 0;
    tables_to_lds(tabs, H.tabs);
    __syncthreads();
    if (round != 0 && t == 0) T[0] = c.s;
    for (uint32_t h = 0; h < (uint32_t)kGroup; h++) {
        // the barrier between two steps: an entry written in step h is read by another lane in step h + 1
        if (!__syncthreads_or(c.active)) break;
        sync_step(H.A, tabs, H.data, H.seg, g0, g1, T, cnt, &x_out, i, h, c);
    }
    if (c.hops) {
        atomicMax(&red[1], c.hops);
        atomicAdd(&red[2], c.hops);
    }
    if (c.bound) red[0] = 1;
    __syncthreads();
    if (i < g1) {
        H.T[i] = T[t];
        H.cnt[i] = cnt[t];
    }
    if (t == 0) {
        Xcur[g] = x_out;
        if (red[0]) H.ctl[JH_BOUND] = 1;
        if (red[1]) atomicMax(&H.ctl[JH_MAX_HOPS], red[1]);
        if (red[2]) atomicAdd(&H.ctl[JH_TOTAL_HOPS], red[2]);
    }
}

// inclusive prefix sum of one value per thread over the workgroup; `buf` holds blockDim.x values
__device__ __forceinline__ uint32_t group_inclusive_sum(uint32_t v, uint32_t* buf)
{
    const uint32_t t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < blockDim.x; d <<= 1) {
        const uint32_t add = t >= d ? buf[t - d] : 0;
        __syncthreads();
        v += add;
        buf[t] = v;
        __syncthreads();
    }
    return v;
}

constexpr int kScanThreads = 1024;

// P[j] = cnt[0] + ... + cnt[j - 1], j = 0 .. nlanes: every thread takes a stretch of consecutive lanes
__global__ __launch_bounds__(kScanThreads) void k_jpeg_huff_scan(JpegHuffArgs H)
{
    __shared__ uint32_t buf[kScanThreads];
    const uint32_t n = H.A.nlanes, per = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t a = min(n, threadIdx.x * per), b = min(n, a + per);
    uint32_t sum = 0;
    for (uint32_t j = a; j < b; j++) sum += H.cnt[j];
    uint32_t run = group_inclusive_sum(sum, buf) - sum;
    for (uint32_t j = a; j < b; j++) {
        H.P[j] = run;
        run += H.cnt[j];
    }
    if (b == n && a < n) H.P[n] = run;
    if (n == 0 && threadIdx.x == 0) H.P[0] = 0;
}

__global__ __launch_bounds__(kGroup) void k_jpeg_huff_write(JpegHuffArgs H)
{
    __shared__ HuffTable tabs[kTables];
    __shared__ uint32_t red[3];   // irregular, in step, spans
    if (threadIdx.x < 3) red[threadIdx.x] = 0;
    tables_to_lds(tabs, H.tabs);
    __syncthreads();
    const uint32_t j = blockIdx.x * kGroup + threadIdx.x;
    if (j < H.A.nlanes) {
        const uint32_t s = segment_of(H.seg, H.A.nseg, j);
        const LaneReport r = write_lane(H.A, tabs, H.data, H.seg, j, H.T[j], H.P[j] - H.P[H.seg[s].lane0], H.coef);
        if (r.irregular) red[0] = 1;
        if (r.in_step) atomicAdd(&red[1], 1u);
        if (r.spans) atomicAdd(&red[2], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (red[0]) H.ctl[JH_IRREGULAR] = 1;
        if (red[1]) atomicAdd(&H.ctl[JH_IN_STEP], red[1]);
        if (red[2]) atomicAdd(&H.ctl[JH_SPANS], red[2]);
    }
}

// ---- DC ----------------------------------------------------------------------------------------------------------------
// Restart interval s holds the MCUs [s * ri_mcus, (s + 1) * ri_mcus) and is cut into cps chunks of kJpegDcChunk MCUs;
// chunk t = s * cps + q.  A thread walks the blocks of its chunk in scan order.
__device__ __forceinline__ bool dc_chunk_range(const JpegHuffArgs& H, uint32_t t, uint32_t* m0, uint32_t* m1)
{
    const uint32_t s = t / H.cps, q = t - s * H.cps;
    const uint32_t seg0 = s * H.ri_mcus, seg1 = min((uint32_t)H.A.nmcu, seg0 + H.ri_mcus);
    *m0 = min(seg1, seg0 + q * kJpegDcChunk);
    *m1 = min(seg1, *m0 + kJpegDcChunk);
    return s < H.A.nseg;
}

template <bool kApply>
__global__ __launch_bounds__(256) void k_jpeg_dc_walk(JpegHuffArgs H)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t m0, m1;
    if (!dc_chunk_range(H, t, &m0, &m1)) return;
    int32_t p0 = 0, p1 = 0, p2 = 0;
    if (kApply && H.cps > 1) {
        p0 = H.dc[3 * t];
        p1 = H.dc[3 * t + 1];
        p2 = H.dc[3 * t + 2];
    }
    for (uint32_t m = m0; m < m1; m++) {
        // the MCU's differences are loaded before any of its values is stored: the loads do not wait for the stores
        int16_t* p[6];
        int32_t v[6];
#pragma unroll
        for (int b = 0; b < 6; b++) {
            p[b] = H.coef + block_base(H.A, m * (uint32_t)H.A.bpm + (uint32_t)(b < H.A.bpm ? b : 0));
            v[b] = b < H.A.bpm ? *p[b] : 0;
        }
#pragma unroll
        for (int b = 0; b < 6; b++) {
            if (b >= H.A.bpm) break;
            const uint32_t c = (H.A.comp_pack >> (2 * b)) & 3;
            int32_t sum;
            if (c == 0) sum = p0 += v[b];
            else if (c == 1) sum = p1 += v[b];
            else sum = p2 += v[b];
            if (kApply) *p[b] = (int16_t)sum;
        }
    }
    if (!kApply) {
        H.dc[3 * t] = p0;
        H.dc[3 * t + 1] = p1;
        H.dc[3 * t + 2] = p2;
    }
}

// the chunk sums of one restart interval -> their exclusive prefix, in place; one workgroup per interval
__global__ __launch_bounds__(256) void k_jpeg_dc_scan(JpegHuffArgs H)
{
    __shared__ uint32_t buf[256];
    int32_t* d = H.dc + (size_t)blockIdx.x * H.cps * 3;
    uint32_t carry[3] = {0, 0, 0};
    for (uint32_t base = 0; base < H.cps; base += 256) {
        const uint32_t q = base + threadIdx.x;
        for (int c = 0; c < 3; c++) {
            const uint32_t v = q < H.cps ? (uint32_t)d[3 * q + c] : 0;
            const uint32_t inc = group_inclusive_sum(v, buf);
            if (q < H.cps) d[3 * q + c] = (int32_t)(carry[c] + inc - v);
            carry[c] += buf[255];
            __syncthreads();
        }
    }
}

// ---- the verdict ----------------------------------------------------------------------------------------------------
// One wave behind everything else of a file that went out without the host looking in between: rounds 0 .. max_rounds,
// scan, write, DC.  The verdict is the synchronous call's: the host decoder takes the file when a chain hit the work
// bound or no round in 1 .. max_rounds changed nothing (then the later phases ran on untrue states and what they wrote
// and counted means nothing), or when the write phase met a stream that contradicts itself.  A round that changed
// nothing is followed only by such rounds, so the first one is both the fixed point and the count of rounds.
// Publication as k_publish_counts (abi_detect.hip): plain stores to the pinned words, a system-scope fence, the sequence
// word last -- the host polls that word and reads the others only behind it.
__global__ __launch_bounds__(64) void k_jpeg_huff_verdict(const uint32_t* __restrict__ ctl, int max_rounds, uint32_t* __restrict__ out,
                                                          uint32_t seq)
{
    jpeg_huff_verdict_words(ctl, max_rounds, out);
    if (threadIdx.x != 0) return;
    __threadfence_system();
    __hip_atomic_store(out + JV_SEQ, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

void launch_jpeg_huff_verdict(hipStream_t s, const uint32_t* ctl, int max_rounds, uint32_t* host_words, uint32_t seq)
{
    hipLaunchKernelGGL(k_jpeg_huff_verdict, dim3(1), dim3(64), 0, s, ctl, max_rounds, host_words, seq);
}

void launch_jpeg_huff_sync(hipStream_t s, const JpegHuffArgs& H, int round)
{
    if (H.ngroups) hipLaunchKernelGGL(k_jpeg_huff_sync, dim3(H.ngroups), dim3(kGroup), 0, s, H, round);
}

void launch_jpeg_huff_scan(hipStream_t s, const JpegHuffArgs& H)
{
    hipLaunchKernelGGL(k_jpeg_huff_scan, dim3(1), dim3(kScanThreads), 0, s, H);
}

void launch_jpeg_huff_write(hipStream_t s, const JpegHuffArgs& H)
{
    if (H.ngroups) hipLaunchKernelGGL(k_jpeg_huff_write, dim3(H.ngroups), dim3(kGroup), 0, s, H);
}

void launch_jpeg_huff_dc(hipStream_t s, const JpegHuffArgs& H)
{
    const uint32_t chunks = H.A.nseg * H.cps;
    if (!chunks) return;
    const dim3 grid((chunks + 255) / 256), block(256);
    if (H.cps > 1) {
        hipLaunchKernelGGL(k_jpeg_dc_walk<false>, grid, block, 0, s, H);
        hipLaunchKernelGGL(k_jpeg_dc_scan, dim3(H.A.nseg), block, 0, s, H);
    }
    hipLaunchKernelGGL(k_jpeg_dc_walk<true>, grid, block, 0, s, H);
}

}  // namespace icelk
