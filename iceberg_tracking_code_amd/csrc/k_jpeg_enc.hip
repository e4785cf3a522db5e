// k_jpeg_enc.hip -- the entropy coder of the JPEG writer for gfx950: quantised coefficients on the device (the layout of
// icelk_jpeg_info_t) -> the bytes of the interleaved scan, Huffman coded with the Annex K tables, FF bytes stuffed.  The
// arithmetic of a block is jpeg_enc.h, shared with the host statement (jpeg_enc_host.h); nothing here decides a bit on
// its own.  Unlike the decoder (k_jpeg_huff.hip) nothing has to be guessed: a block's length depends on the block and on
// one DC value whose address is known, so the stream is a prefix sum and a pack.
//
//   count   one lane per block in scan order, one wave (kJpegEncGroup = 64 blocks) per workgroup.  The lane loads its 128
//           contiguous bytes with eight 16-byte loads and writes them to its LDS row in ZIGZAG order (the permutation is a
//           compile-time constant per register), reads the DC of its predecessor straight from the plane, walks the row
//           (encode_block into a CountSink) and stores the length as 16 bits; a wave scan gives the group's sum.  A
//           coefficient without a code sets JE_INVALID with an integer OR
//   scan    an exclusive prefix sum over the groups' sums (in place) and its total, one workgroup of 1024 lanes that loops
//           over kJpegEncScanPass entries at a time with a carry.  Bit offsets are 32 bits wide: the launcher's caller has
//           checked blocks * 1660 < 2^32
//   pack    the same groups again: a lane's bit offset is its group's plus the wave scan of the stored lengths.  The
//           group's stretch of the stream is assembled in LDS, zeroed first, with ds_or (most significant bit first,
//           a lane flushes a dword when it has 32 bits); the lane of the scan's last block adds the 1-bits that fill the
//           last byte.  Then the stretch is stored as whole dwords in byte order; only its first and last dword can be
//           shared with a neighbour, and those go into the zero-filled buffer with an integer atomic OR -- which does not
//           depend on order, so the bytes are the same from run to run
//   ff      64 bytes of the packed stream per lane, 16 KiB per workgroup: the FF bytes of every workgroup's stretch
//   (scan   again, over those counts)
//   stuff   the same chunks: a workgroup scan of the lanes' FF counts, then every lane copies its bytes to their final
//           place, a 00 behind every FF.  Byte stores: a lane's output has no alignment to speak of
// Lanes diverge per coefficient in count and pack (zero or not, ZRL or not), as the decoder's lanes do per symbol; the
// loop counter, the table addresses and everything between the walks are uniform.  No scratch in any kernel.
//
// The device-sized forms (k_jpeg_enc_pack_budget, _ff_budget, _stuff_budget; the jobs with a file of abi_jpeg_job.hip) run the
// same bodies with the sizes read from the control words instead of from the host: packed and stuffed stream are
// allocated to a capacity of `cap` bytes beforehand, and each of the three leaves the whole grid -- a uniform branch on
// two loaded words -- when the stream does not fit it (jpeg_enc.h: packed_fits, live_bytes, stuffed_fits).  Behind them
// k_jpeg_crop_verdict, one wave, publishes the decoder's and the coder's verdict and the stuffed length to pinned words.
#include "icelk_internal.h"

namespace icelk {

namespace {

constexpr int kGroup = kJpegEncGroup;
constexpr int kTilePitch = 66;   // halfwords per lane: 33 dwords, so the lanes of a wave fall on different banks
// dwords of a group's stretch at most: up to 31 bits of the dword it begins in, its blocks, the 7 bits of padding
constexpr int kStretchDwords = (31 + kGroup * enc::kMaxBlockBits + 7 + 31) / 32;
constexpr int kChunk = kJpegEncChunk;   // bytes of the packed stream per lane of ff / stuff
static_assert(kChunk == enc::kChunkBytes && enc::kChunksPerGroup == 256, "jpeg_enc.h sizes the capacity by these");

constexpr uint8_t kZz[64] = ICELK_ENC_ZIGZAG;
constexpr int zigzag_of(int natural)
{
    for (int k = 0; k < 64; k++)
        if (kZz[k] == natural) return k;
    return 0;
}

// coefficient N of the block (natural order, two per loaded dword) -> its place in zigzag order in the lane's LDS row
template <int N>
__device__ __forceinline__ void scatter(uint16_t* row, const uint32_t (&w)[32])
{
    constexpr int k = zigzag_of(N);
    row[k] = (uint16_t)(w[N >> 1] >> (16 * (N & 1)));
    if constexpr (N + 1 < 64) scatter<N + 1>(row, w);
}

__device__ __forceinline__ void load_row(uint16_t* row, const int16_t* blk)
{
    const uint4* p = reinterpret_cast<const uint4*>(blk);   // a block is 128 bytes at a multiple of 128 from hipMalloc's pointer
    uint32_t w[32];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const uint4 q = p[r];
        w[4 * r] = q.x;
        w[4 * r + 1] = q.y;
        w[4 * r + 2] = q.z;
        w[4 * r + 3] = q.w;
    }
    scatter<0>(row, w);
}

struct RowBlock {
    const uint16_t* row;
    __device__ __forceinline__ int operator()(int k) const { return (int)(int16_t)row[k]; }
};

__device__ __forceinline__ void stage_codes(uint32_t* dst, const uint32_t* src, int t, int nthreads)
{
    for (int i = t; i < enc::kCodeWords; i += nthreads) dst[i] = src[i];
}

__device__ __forceinline__ uint32_t wave_inclusive(uint32_t x, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// bits into the group's LDS stream, most significant first; the stream was zeroed, every dword is OR-ed in
struct LdsSink {
    uint32_t* w;
    uint32_t d;      // the dword the next 32 bits go to
    uint64_t acc;
    int n;           // bits waiting in acc, < 32 between puts
    __device__ __forceinline__ void put(uint32_t v, int k)
    {
        acc = acc << k | v;
        n += k;
        if (n >= 32) {
            n -= 32;
            atomicOr(&w[d++], (uint32_t)(acc >> n));
            acc &= ((uint64_t)1 << n) - 1;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (n) atomicOr(&w[d], (uint32_t)(acc << (32 - n)));
    }
};

__device__ __forceinline__ uint32_t ff_bytes(uint32_t w)
{
    return (uint32_t)((w & 0xffu) == 0xffu) + (uint32_t)((w & 0xff00u) == 0xff00u) + (uint32_t)((w & 0xff0000u) == 0xff0000u) +
           (uint32_t)(w >= 0xff000000u);
}

// the lane's chunk of the packed stream (whole chunks are allocated and zero behind the stream's end) and its FF bytes
__device__ __forceinline__ uint32_t load_chunk(const uint32_t* packed, uint32_t chunk, uint32_t (&w)[kChunk / 4])
{
    const uint4* p = reinterpret_cast<const uint4*>(packed) + (size_t)chunk * (kChunk / 16);
    uint32_t ff = 0;
#pragma unroll
    for (int r = 0; r < kChunk / 16; r++) {
        const uint4 q = p[r];
        w[4 * r] = q.x;
        w[4 * r + 1] = q.y;
        w[4 * r + 2] = q.z;
        w[4 * r + 3] = q.w;
        ff += ff_bytes(q.x) + ff_bytes(q.y) + ff_bytes(q.z) + ff_bytes(q.w);
    }
    return ff;
}

}  // namespace

__global__ __launch_bounds__(kJpegEncGroup) void k_jpeg_enc_count(JpegEncArgs A)
{
    __shared__ uint16_t tile[kGroup][kTilePitch];
    __shared__ uint32_t codes[enc::kCodeWords];
    const int lane = threadIdx.x;
    const uint32_t s = blockIdx.x * kGroup + lane;
    const bool live = s < A.L.blocks;
    stage_codes(codes, A.codes, lane, kGroup);
    enc::Place P{};
    int pred = 0;
    if (live) {
        P = enc::place(A.L, s);
        load_row(tile[lane], A.coef + P.at);
        if (P.pred != enc::kNoPred) pred = A.coef[P.pred];
    }
    __syncthreads();
    uint32_t bits = 0;
    if (live) {
        enc::CountSink n;
        const enc::Codes* C = reinterpret_cast<const enc::Codes*>(codes);
        if (!enc::encode_block(RowBlock{tile[lane]}, pred, C->dc[P.table], C->ac[P.table], n)) atomicOr(&A.ctl[JE_INVALID], 1u);
        bits = n.bits;
        A.bits[s] = (uint16_t)bits;
    }
    const uint32_t sum = wave_inclusive(bits, lane);
    if (lane == kGroup - 1) A.group[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kJpegEncScanPass) void k_jpeg_enc_scan(uint32_t* v, uint32_t n, uint32_t* total)
{
    __shared__ uint32_t wave_sum[kJpegEncScanPass / 64];
    __shared__ uint32_t carry_s;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += kJpegEncScanPass) {
        const uint32_t i = base + t;
        const uint32_t x = i < n ? v[i] : 0u;
        const uint32_t inc = wave_inclusive(x, lane);
        if (lane == 63) wave_sum[wv] = inc;
        __syncthreads();
        uint32_t before = carry_s;
        for (int k = 0; k < wv; k++) before += wave_sum[k];
        if (i < n) v[i] = before + inc - x;
        __syncthreads();   // every lane has read the carry
        if (t == kJpegEncScanPass - 1) carry_s = before + inc;
        __syncthreads();
    }
    if (t == 0) *total = carry_s;
}

// the body of pack.  Budget: the workgroup leaves before any store when its stretch does not end inside `cap` bytes --
// with control words that the chain itself wrote the grid's exit in k_jpeg_enc_pack_budget has decided that already
template <bool Budget>
__device__ __forceinline__ void pack_group(const JpegEncArgs& A, uint32_t cap)
{
    __shared__ uint16_t tile[kGroup][kTilePitch];
    __shared__ uint32_t codes[enc::kCodeWords];
    __shared__ uint32_t stream[kStretchDwords];
    const int lane = threadIdx.x;
    const uint32_t s = blockIdx.x * kGroup + lane;
    const bool live = s < A.L.blocks;
    stage_codes(codes, A.codes, lane, kGroup);
    enc::Place P{};
    int pred = 0;
    uint32_t bits = 0;
    if (live) {
        P = enc::place(A.L, s);
        load_row(tile[lane], A.coef + P.at);
        if (P.pred != enc::kNoPred) pred = A.coef[P.pred];
        bits = A.bits[s];
    }
    const uint32_t inc = wave_inclusive(bits, lane);
    const uint32_t start = A.group[blockIdx.x];                    // the group's first bit
    uint32_t end = start + __shfl(inc, kGroup - 1, 64);            // one past its last
    const bool last_group = blockIdx.x == gridDim.x - 1;
    const uint32_t fill = last_group ? (0u - end) & 7u : 0u;       // the 1-bits that complete the stream's last byte
    end += fill;
    if (Budget && !enc::stretch_inside(start, end, cap)) return;   // uniform: start and end are the workgroup's
    const uint32_t first_dw = start >> 5, ndw = ((end + 31u) >> 5) - first_dw;   // <= kStretchDwords; >= 1: a block has bits
    for (uint32_t i = lane; i < ndw; i += kGroup) stream[i] = 0u;
    __syncthreads();
    if (live) {
        const uint32_t o = start + inc - bits;
        LdsSink out{stream, (o >> 5) - first_dw, 0, (int)(o & 31u)};
        const enc::Codes* C = reinterpret_cast<const enc::Codes*>(codes);
        enc::encode_block(RowBlock{tile[lane]}, pred, C->dc[P.table], C->ac[P.table], out);
        if (fill && s == A.L.blocks - 1) out.put((1u << fill) - 1u, (int)fill);
        out.flush();
    }
    __syncthreads();
    for (uint32_t i = lane; i < ndw; i += kGroup) {
        const uint32_t v = __builtin_bswap32(stream[i]);           // the stream's bytes in memory order
        if (i == 0 || i == ndw - 1)
            atomicOr(&A.packed[first_dw + i], v);
        else
            A.packed[first_dw + i] = v;
    }
}

__global__ __launch_bounds__(kJpegEncGroup) void k_jpeg_enc_pack(JpegEncArgs A) { pack_group<false>(A, 0u); }

__global__ __launch_bounds__(kJpegEncGroup) void k_jpeg_enc_pack_budget(JpegEncArgs A, uint32_t cap)
{
    if (!enc::packed_fits(A.ctl[JE_TOTAL_BITS], A.ctl[JE_INVALID], cap)) return;   // the whole grid: nothing is stored
    pack_group<true>(A, cap);
}

__device__ __forceinline__ void ff_group(const uint32_t* packed, uint32_t nchunks, uint32_t* wg_ff)
{
    __shared__ uint32_t wave_sum[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t chunk = blockIdx.x * 256u + t;
    uint32_t w[kChunk / 4];
    const uint32_t ff = chunk < nchunks ? load_chunk(packed, chunk, w) : 0u;
    const uint32_t inc = wave_inclusive(ff, lane);
    if (lane == 63) wave_sum[wv] = inc;
    __syncthreads();
    if (t == 0) wg_ff[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

__global__ __launch_bounds__(256) void k_jpeg_enc_ff(const uint32_t* packed, uint32_t nchunks, uint32_t* wg_ff) { ff_group(packed, nchunks, wg_ff); }

// the grid covers the capacity; a workgroup behind the live chunks (all of them when pack left) counts 0
__global__ __launch_bounds__(256) void k_jpeg_enc_ff_budget(const uint32_t* packed, const uint32_t* ctl, uint32_t cap, uint32_t* wg_ff)
{
    ff_group(packed, enc::chunks_of(enc::live_bytes(ctl[JE_TOTAL_BITS], ctl[JE_INVALID], cap)), wg_ff);
}

// the body of stuff.  Budget: a lane leaves when its bytes would not end inside `cap` -- as in pack_group, with control
// words of the chain's own the grid's exit has decided that already
template <bool Budget>
__device__ __forceinline__ void stuff_group(const uint32_t* packed, uint32_t nbytes, uint32_t nchunks, const uint32_t* wg_off, uint8_t* out,
                                            uint32_t cap)
{
    __shared__ uint32_t wave_sum[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t chunk = blockIdx.x * 256u + t;
    const bool live = chunk < nchunks;
    uint32_t w[kChunk / 4];
    const uint32_t ff = live ? load_chunk(packed, chunk, w) : 0u;
    const uint32_t inc = wave_inclusive(ff, lane);
    if (lane == 63) wave_sum[wv] = inc;
    __syncthreads();
    if (!live) return;
    uint32_t before = wg_off[blockIdx.x] + inc - ff;
    for (int k = 0; k < wv; k++) before += wave_sum[k];
    const uint32_t at = chunk * (uint32_t)kChunk;
    if (Budget && !enc::bytes_inside((uint64_t)at + before, min((uint32_t)kChunk, nbytes - at) + ff, cap)) return;   // live: at < nbytes
    uint8_t* dst = out + (size_t)at + before;
#pragma unroll
    for (int j = 0; j < kChunk; j++) {
        if (at + j < nbytes) {
            const uint8_t b = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
            *dst++ = b;
            if (b == 0xffu) *dst++ = 0;
        }
    }
}

__global__ __launch_bounds__(256) void k_jpeg_enc_stuff(const uint32_t* packed, uint32_t nbytes, uint32_t nchunks, const uint32_t* wg_off,
                                                        uint8_t* out)
{
    stuff_group<false>(packed, nbytes, nchunks, wg_off, out, 0u);
}

__global__ __launch_bounds__(256) void k_jpeg_enc_stuff_budget(const uint32_t* packed, const uint32_t* ctl, uint32_t cap, const uint32_t* wg_off,
                                                               uint8_t* out)
{
    const uint32_t bits = ctl[JE_TOTAL_BITS];
    if (!enc::stuffed_fits(bits, ctl[JE_INVALID], ctl[JE_FF_TOTAL], cap)) return;   // the whole grid: nothing is stored
    const uint32_t nbytes = enc::packed_bytes(bits);
    stuff_group<true>(packed, nbytes, enc::chunks_of(nbytes), wg_off, out, cap);
}

// One wave behind the whole chain of a crop job: the decoder's verdict and statistics as k_jpeg_huff_verdict publishes
// them, the coder's verdict and the stuffed length, then the sequence word -- plain stores to the pinned words, a
// system-scope fence, a release store.
__global__ __launch_bounds__(64) void k_jpeg_crop_verdict(const uint32_t* __restrict__ huff_ctl, int max_rounds, const uint32_t* __restrict__ enc_ctl,
                                                          uint32_t cap, uint32_t* __restrict__ out, uint32_t seq)
{
    jpeg_huff_verdict_words(huff_ctl, max_rounds, out);
    if (threadIdx.x != 0) return;
    uint32_t verdict = enc::kNotAsked, len = 0;
    if (enc_ctl) {   // uniform: a kernel argument
        const uint32_t bits = enc_ctl[JE_TOTAL_BITS], invalid = enc_ctl[JE_INVALID], ff = enc_ctl[JE_FF_TOTAL];
        verdict = enc::budget_verdict(bits, invalid, ff, cap);
        if (verdict == enc::kCoded) len = enc::packed_bytes(bits) + ff;
    }
    out[JV_ENC_VERDICT] = verdict;
    out[JV_ENC_LEN] = len;
    __threadfence_system();
    __hip_atomic_store(out + JV_SEQ, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

void launch_jpeg_enc_count(hipStream_t s, const JpegEncArgs& A)
{
    hipLaunchKernelGGL(k_jpeg_enc_count, dim3((A.L.blocks + kGroup - 1) / kGroup), dim3(kGroup), 0, s, A);
}

void launch_jpeg_enc_scan(hipStream_t s, uint32_t* v, uint32_t n, uint32_t* total)
{
    hipLaunchKernelGGL(k_jpeg_enc_scan, dim3(1), dim3(kJpegEncScanPass), 0, s, v, n, total);
}

void launch_jpeg_enc_pack(hipStream_t s, const JpegEncArgs& A)
{
    hipLaunchKernelGGL(k_jpeg_enc_pack, dim3((A.L.blocks + kGroup - 1) / kGroup), dim3(kGroup), 0, s, A);
}

void launch_jpeg_enc_ff(hipStream_t s, const uint32_t* packed, uint32_t nchunks, uint32_t* wg_ff)
{
    hipLaunchKernelGGL(k_jpeg_enc_ff, dim3((nchunks + 255) / 256), dim3(256), 0, s, packed, nchunks, wg_ff);
}

void launch_jpeg_enc_stuff(hipStream_t s, const uint32_t* packed, uint32_t nbytes, uint32_t nchunks, const uint32_t* wg_off, uint8_t* out)
{
    hipLaunchKernelGGL(k_jpeg_enc_stuff, dim3((nchunks + 255) / 256), dim3(256), 0, s, packed, nbytes, nchunks, wg_off, out);
}

// ---- the device-sized forms: grids by the capacity `cap`, sizes from A.ctl --------------------------------------------
void launch_jpeg_enc_pack_budget(hipStream_t s, const JpegEncArgs& A, uint32_t cap)
{
    hipLaunchKernelGGL(k_jpeg_enc_pack_budget, dim3((A.L.blocks + kGroup - 1) / kGroup), dim3(kGroup), 0, s, A, cap);
}

void launch_jpeg_enc_ff_budget(hipStream_t s, const uint32_t* packed, const uint32_t* ctl, uint32_t cap, uint32_t* wg_ff)
{
    hipLaunchKernelGGL(k_jpeg_enc_ff_budget, dim3(enc::groups_of(enc::chunks_of(cap))), dim3(256), 0, s, packed, ctl, cap, wg_ff);
}

void launch_jpeg_enc_stuff_budget(hipStream_t s, const uint32_t* packed, const uint32_t* ctl, uint32_t cap, const uint32_t* wg_off, uint8_t* out)
{
    hipLaunchKernelGGL(k_jpeg_enc_stuff_budget, dim3(enc::groups_of(enc::chunks_of(cap))), dim3(256), 0, s, packed, ctl, cap, wg_off, out);
}

void launch_jpeg_crop_verdict(hipStream_t s, const uint32_t* huff_ctl, int max_rounds, const uint32_t* enc_ctl, uint32_t cap, uint32_t* host_words,
                              uint32_t seq)
{
    hipLaunchKernelGGL(k_jpeg_crop_verdict, dim3(1), dim3(64), 0, s, huff_ctl, max_rounds, enc_ctl, cap, host_words, seq);
}

}  // namespace icelk
