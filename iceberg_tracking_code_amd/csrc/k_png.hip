// k_png.hip -- the PNG writer for gfx950: a tightly packed (or strided) R G B picture on the device -> the bytes of ONE
// fixed-Huffman deflate block over its filtered rows, and their Adler-32.  The arithmetic of a byte, a token and a code is
// png_enc.h, shared with the host statement (png_enc_host.h); nothing here decides a bit on its own.  The shape is the JPEG
// writer's (k_jpeg_enc.hip): count -> exclusive prefix sum (k_jpeg_enc_scan) -> pack, with no host look in between.
//
//   filter  one workgroup of 256 lanes per row.  Pass 1: a lane takes every 256th byte of the row, computes all five
//           filtered values and adds their absolute values (signed 8-bit) to five sums, which the workgroup adds up
//           (3 W * 128 < 2^23); lane 0 picks the type (pick_filter) and stores it.  Pass 2: the same bytes, the chosen type,
//           one byte store each into F.  Rows are independent: they read the UNFILTERED row above
//   parse   one workgroup per segment of kSegment = 4096 bytes of F, 16 positions per lane.  The segment and the four
//           bytes in front of it go to LDS as dwords, the bytes one row pitch earlier byte by byte (only where the pitch
//           counts as a distance).  The greedy parse is serial, the match lengths are not: per distance a lane makes the
//           16-bit mask of its positions that equal the byte `distance` before, publishes how many leading positions do
//           (head), and finds the run that continues behind its chunk by walking the following heads -- at most 17 of them,
//           since a match ends at 258.  From the back of its chunk it then knows every position's run for every distance and
//           has the token that WOULD begin there (best_of).  Which of them do begin is the serial part, and it is cut in three:
//           on the way back through its chunk a lane also notes, for each of the 16 places the parse may enter the chunk at,
//           where it leaves it again (exit: the chunk's own tokens, followed in LDS); lane 0 then hops from chunk to chunk
//           from the segment's first byte -- one dependent LDS read per chunk entered, 256 at most, where a walk over the
//           tokens took up to 4096 -- and leaves every chunk its entry; every lane follows its own 16 tokens from there.
//           It then stores its 16 token words (0: none begins here), and the workgroup adds up the tokens' bit lengths and
//           the segment's Adler piece
//   (scan   k_jpeg_enc_scan over the segments' bit counts, total into the control words)
//   pack    the same segments: a lane's bit offset is 3 + its segment's + the workgroup scan of its tokens' lengths.  The
//           segment's stretch of the stream is assembled in LDS, zeroed first, with ds_or (LSB first, a lane flushes a dword
//           when it has 32 bits), then stored as whole dwords; only its first and last dword can be shared with a
//           neighbour, and those go into the zero-filled buffer with an integer atomic OR, which does not depend on order.
//           Segment 0 adds the three header bits; the end-of-block is seven zero bits and the padding is zero: the buffer
//           has them already
//   adler   one workgroup: a lane joins a contiguous range of the segments' pieces in order (adler_join), then the 256
//           results are joined pairwise in eight steps, the earlier stretch always on the left
// Lanes diverge per token in pack (literal or match) and nowhere else in a way that depends on data, apart from lane 0's
// walk.  No scratch, no inline assembly, plain vector stores.
#include "icelk_internal.h"

namespace icelk {

namespace {

constexpr int kLanes = kPngLanes;
constexpr int kPer = png::kSegment / kLanes;   // positions of a segment per lane
static_assert(kPer == 16 && kLanes == 256, "a lane's chunk is one 16-byte load and one 16-bit mask");
constexpr int kLook = (png::kMaxMatch + kPer - 1) / kPer;   // chunks behind its own a lane has to look at
// dwords of a segment's stretch at most: up to 31 bits of the dword it begins in, 9 bits a byte
constexpr int kStretchDwords = (31 + png::kSegment * 9 + 31) / 32 + 1;

__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// the sum over the workgroup's four waves; `slot` is four words of LDS nobody else uses until the next barrier pair
__device__ __forceinline__ uint32_t group_sum(uint32_t x, uint32_t* slot, int t)
{
    x = wave_sum(x);
    __syncthreads();
    if ((t & 63) == 0) slot[t >> 6] = x;
    __syncthreads();
    return slot[0] + slot[1] + slot[2] + slot[3];
}

__device__ __forceinline__ void unpack16(const uint4& q, uint8_t* b)
{
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 16; j++) b[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
}

// bits into the segment's LDS stretch, least significant first; the stretch was zeroed, every dword is OR-ed in
struct LdsSink {
    uint32_t* w;
    uint32_t d;      // the dword the next bits go to
    uint64_t acc;
    int n;           // bits of acc taken, < 32 between puts
    __device__ __forceinline__ void put(uint32_t v, int k)
    {
        acc |= (uint64_t)v << n;
        n += k;
        if (n >= 32) {
            atomicOr(&w[d++], (uint32_t)acc);
            acc >>= 32;
            n -= 32;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (n) atomicOr(&w[d], (uint32_t)acc);
    }
};

}  // namespace

__global__ __launch_bounds__(kPngLanes) void k_png_filter(PngArgs A)
{
    __shared__ uint32_t part[5][4];
    __shared__ int type_s;
    const int t = threadIdx.x, y = blockIdx.x, n = 3 * A.w;
    const uint8_t* cur = A.rgb + (size_t)y * A.stride;
    const uint8_t* up = cur - A.stride;   // read only when y > 0
    uint8_t* out = A.F + (size_t)y * A.pitch;
    uint32_t sum[5] = {0, 0, 0, 0, 0};
    for (int x = t; x < n; x += kLanes) {
        const int v = cur[x], a = x >= 3 ? cur[x - 3] : 0, b = y > 0 ? up[x] : 0, c = y > 0 && x >= 3 ? up[x - 3] : 0;
#pragma unroll
        for (int k = 0; k < 5; k++) sum[k] += png::abs8(png::filter_value(k, v, a, b, c));
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const uint32_t s = wave_sum(sum[k]);
        if ((t & 63) == 0) part[k][t >> 6] = s;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t total[5];
        for (int k = 0; k < 5; k++) total[k] = part[k][0] + part[k][1] + part[k][2] + part[k][3];
        const int type = png::pick_filter(total);
        type_s = type;
        out[0] = (uint8_t)type;
    }
    __syncthreads();
    const int type = type_s;
    for (int x = t; x < n; x += kLanes) {
        const int v = cur[x], a = x >= 3 ? cur[x - 3] : 0, b = y > 0 ? up[x] : 0, c = y > 0 && x >= 3 ? up[x - 3] : 0;
        out[1 + x] = png::filter_value(type, v, a, b, c);
    }
}

__global__ __launch_bounds__(kPngLanes) void k_png_parse(PngArgs A)
{
    __shared__ uint32_t cur_w[1 + png::kSegment / 4];   // F[s - 4 .. s + kSegment)
    __shared__ uint32_t up_w[png::kSegment / 4];        // F[s - pitch .. s - pitch + kSegment), where that exists
    __shared__ uint16_t head[png::kCandidates][kLanes];
    __shared__ uint16_t exit_s[png::kSegment];          // entering a chunk at this position, the parse leaves it at chunk + this
    __shared__ uint32_t entry[kLanes];                  // where the parse enters the chunk, kPer: it does not
    __shared__ uint32_t slot[4];
    const int t = threadIdx.x;
    const uint32_t s = blockIdx.x * (uint32_t)png::kSegment;
    const uint32_t here = A.n - s < (uint32_t)png::kSegment ? A.n - s : (uint32_t)png::kSegment;   // bytes of F in the segment
    const bool use_pitch = A.pitch <= (uint32_t)png::kMaxDistance;   // uniform
    const uint32_t* F32 = reinterpret_cast<const uint32_t*>(A.F);    // F is allocated in whole segments
    uint8_t* up_b = reinterpret_cast<uint8_t*>(up_w);
    for (int i = t; i < png::kSegment / 4; i += kLanes) cur_w[1 + i] = F32[s / 4 + i];
    if (t == 0) cur_w[0] = s > 0 ? F32[s / 4 - 1] : 0u;
    entry[t] = kPer;
    if (use_pitch)
        for (int i = t; i < png::kSegment; i += kLanes) up_b[i] = s + i >= A.pitch ? A.F[s + i - A.pitch] : (uint8_t)0;
    __syncthreads();

    // the lane's 16 bytes, the 4 in front of them, the 16 a row earlier
    uint8_t b[4 + kPer], u[kPer];
    {
        const uint32_t w = cur_w[4 * t];
        b[0] = (uint8_t)w, b[1] = (uint8_t)(w >> 8), b[2] = (uint8_t)(w >> 16), b[3] = (uint8_t)(w >> 24);
        unpack16(make_uint4(cur_w[4 * t + 1], cur_w[4 * t + 2], cur_w[4 * t + 3], cur_w[4 * t + 4]), b + 4);
        unpack16(make_uint4(up_w[4 * t], up_w[4 * t + 1], up_w[4 * t + 2], up_w[4 * t + 3]), u);
    }
    uint32_t mask[png::kCandidates] = {0, 0, 0};
    uint32_t sumA = 0, sumB = 0;
#pragma unroll
    for (int j = 0; j < kPer; j++) {
        const uint32_t i = kPer * t + j, pos = s + i;
        if (i < here) {   // past N nothing equals anything: every run ends there
            if (png::distance_ok(1, pos) && b[4 + j] == b[3 + j]) mask[0] |= 1u << j;
            if (png::distance_ok(3, pos) && b[4 + j] == b[1 + j]) mask[1] |= 1u << j;
            if (png::distance_ok(A.pitch, pos) && b[4 + j] == u[j]) mask[2] |= 1u << j;
            sumA += b[4 + j];
            sumB += (here - i) * b[4 + j];
        }
    }
#pragma unroll
    for (int k = 0; k < png::kCandidates; k++) head[k][t] = (uint16_t)__builtin_ctz(~mask[k] | 1u << kPer);
    __syncthreads();
    uint32_t run[png::kCandidates];   // the run that begins right behind the lane's chunk, as far as a match can use it
#pragma unroll
    for (int k = 0; k < png::kCandidates; k++) {
        uint32_t r = 0;
        for (int j = t + 1; j < kLanes && j <= t + kLook; j++) {
            const uint32_t h = head[k][j];
            r += h;
            if (h < (uint32_t)kPer) break;
        }
        run[k] = r;
    }
    uint16_t tok[kPer];
#pragma unroll
    for (int j = kPer - 1; j >= 0; j--) {
#pragma unroll
        for (int k = 0; k < png::kCandidates; k++) run[k] = (mask[k] >> j) & 1u ? run[k] + 1 : 0u;
        tok[j] = png::best_of(run, b[4 + j]);
        const uint32_t next = j + png::token_advance(tok[j]);   // > j; the lane reads what it has just stored itself
        exit_s[kPer * t + j] = (uint16_t)(next >= (uint32_t)kPer ? next : exit_s[kPer * t + next]);
    }
    __syncthreads();

    if (t == 0) {   // the greedy parse, a chunk a step: exit_s is at least kPer
        for (uint32_t pos = 0; pos < here; pos = (pos & ~(uint32_t)(kPer - 1)) + exit_s[pos]) entry[pos / kPer] = pos % kPer;
    }
    __syncthreads();

    uint32_t next = entry[t], bits = 0;
#pragma unroll
    for (int j = 0; j < kPer; j++) {
        if ((uint32_t)j == next && kPer * t + j < here)
            next = j + png::token_advance(tok[j]);
        else
            tok[j] = 0;
        if (tok[j]) bits += (uint32_t)png::token_code(tok[j], A.pitch).n;
    }
    uint4* dst = reinterpret_cast<uint4*>(A.tok + s + kPer * t);   // tok is allocated in whole segments
    dst[0] = make_uint4((uint32_t)tok[0] | (uint32_t)tok[1] << 16, (uint32_t)tok[2] | (uint32_t)tok[3] << 16, (uint32_t)tok[4] | (uint32_t)tok[5] << 16,
                   (uint32_t)tok[6] | (uint32_t)tok[7] << 16);
    dst[1] = make_uint4((uint32_t)tok[8] | (uint32_t)tok[9] << 16, (uint32_t)tok[10] | (uint32_t)tok[11] << 16,
                   (uint32_t)tok[12] | (uint32_t)tok[13] << 16, (uint32_t)tok[14] | (uint32_t)tok[15] << 16);
    bits = group_sum(bits, slot, t);
    sumA = group_sum(sumA, slot, t);
    sumB = group_sum(sumB, slot, t);
    if (t == 0) {
        A.seg[blockIdx.x] = bits;
        const png::Adler p = png::adler_piece(sumA, sumB, here);
        A.adler[3 * blockIdx.x] = p.A, A.adler[3 * blockIdx.x + 1] = p.B, A.adler[3 * blockIdx.x + 2] = p.n;
    }
}

__global__ __launch_bounds__(kPngLanes) void k_png_pack(PngArgs A)
{
    __shared__ uint32_t stream[kStretchDwords];
    __shared__ uint32_t wave_total[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t s = blockIdx.x * (uint32_t)png::kSegment;
    uint16_t tok[kPer];
    {
        const uint4* src = reinterpret_cast<const uint4*>(A.tok + s + kPer * t);
        const uint4 q0 = src[0], q1 = src[1];
        const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
        for (int j = 0; j < kPer; j++) tok[j] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
    }
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < kPer; j++)
        if (tok[j]) bits += (uint32_t)png::token_code(tok[j], A.pitch).n;
    uint32_t inc = bits;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(inc, d, 64);
        if (lane >= d) inc += y;
    }
    if (lane == 63) wave_total[wv] = inc;
    __syncthreads();
    uint32_t before = inc - bits;
    for (int k = 0; k < wv; k++) before += wave_total[k];
    const uint32_t start = png::kHeaderBits + A.seg[blockIdx.x];   // the segment's first bit
    const uint32_t end = start + wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
    const uint32_t first_dw = start >> 5, ndw = ((end + 31u) >> 5) - first_dw;   // <= kStretchDwords; a segment has a token
    for (uint32_t i = t; i < ndw; i += kLanes) stream[i] = 0u;
    __syncthreads();
    if (blockIdx.x == 0 && t == 0) atomicOr(&stream[0], png::kHeaderValue);
    if (bits) {
        const uint32_t o = start + before;
        LdsSink out{stream, (o >> 5) - first_dw, 0, (int)(o & 31u)};
#pragma unroll
        for (int j = 0; j < kPer; j++)
            if (tok[j]) {
                const png::Code c = png::token_code(tok[j], A.pitch);
                out.put(c.bits, c.n);
            }
        out.flush();
    }
    __syncthreads();
    for (uint32_t i = t; i < ndw; i += kLanes) {
        const uint32_t v = stream[i];   // LSB first: the dword's bytes are the stream's in memory order
        if (i == 0 || i == ndw - 1)
            atomicOr(&A.stream[first_dw + i], v);
        else
            A.stream[first_dw + i] = v;
    }
}

__global__ __launch_bounds__(kPngLanes) void k_png_adler(const uint32_t* pieces, uint32_t n, uint32_t* value)
{
    __shared__ uint32_t part[kLanes][3];
    const int t = threadIdx.x;
    const uint32_t per = (n + kLanes - 1) / kLanes;
    png::Adler sum{0, 0, 0};
    for (uint32_t i = t * per; i < n && i < (t + 1) * per; i++) sum = png::adler_join(sum, png::Adler{pieces[3 * i], pieces[3 * i + 1], pieces[3 * i + 2]});
    part[t][0] = sum.A, part[t][1] = sum.B, part[t][2] = sum.n;
    for (int step = 1; step < kLanes; step <<= 1) {   // joining is associative, not commutative: the left part is the earlier one
        __syncthreads();
        if (t % (2 * step) == 0) {
            const png::Adler both = png::adler_join(png::Adler{part[t][0], part[t][1], part[t][2]}, png::Adler{part[t + step][0], part[t + step][1], part[t + step][2]});
            part[t][0] = both.A, part[t][1] = both.B, part[t][2] = both.n;
        }
    }
    if (t == 0) *value = png::adler_value(png::Adler{part[0][0], part[0][1], part[0][2]});
}

void launch_png_filter(hipStream_t s, const PngArgs& A) { hipLaunchKernelGGL(k_png_filter, dim3(A.h), dim3(kPngLanes), 0, s, A); }

void launch_png_parse(hipStream_t s, const PngArgs& A)
{
    hipLaunchKernelGGL(k_png_parse, dim3(png::segments_of(A.n)), dim3(kPngLanes), 0, s, A);
}

void launch_png_pack(hipStream_t s, const PngArgs& A)
{
    hipLaunchKernelGGL(k_png_pack, dim3(png::segments_of(A.n)), dim3(kPngLanes), 0, s, A);
}

void launch_png_adler(hipStream_t s, const uint32_t* pieces, uint32_t n, uint32_t* value)
{
    hipLaunchKernelGGL(k_png_adler, dim3(1), dim3(kPngLanes), 0, s, pieces, n, value);
}

}  // namespace icelk
