// k_resize.hip -- the movie's scaler on the device: an 8-bit R G B picture resampled to any size, larger or smaller, in two
// separable passes.  The arithmetic is resize.h (sample, clip8), which the host statement runs as well; the tables are made
// on the host (resize::make_axis) and the device does integer work only.
//
//   k_resize_rows  the horizontal pass.  A workgroup makes 256 neighbouring pixels of one output row, a lane one pixel with its
//                  three channels.  Neighbouring outputs share taps: where the source pixels under the workgroup's outputs
//                  are few (kStage = 1024 or fewer: every enlargement, and reductions short of a quarter) their bytes are
//                  staged in LDS once, read as dwords from the dword boundary below them, and every tap is an LDS byte read;
//                  otherwise (4099 -> 16 has 1025 taps per output) a lane walks its own taps in global memory.  The choice is
//                  the workgroup's, so no lane diverges on it.  No limit on the tap count.  A lane stores its own three
//                  bytes: gathering the workgroup's 768 bytes in LDS for dword stores was measured and gained nothing
//                  (19.1 against 19.8 us at 1200 x 800 -> 2000 wide)
//   k_resize_cols  the vertical pass.  Lanes run along the row, four bytes of it each, whatever the channel: every tap is one
//                  coalesced row read (a dword per lane where the address is aligned), the row's first index, count and
//                  weights are the same for the whole workgroup and sit in scalar registers
//
// Bounds, load by load and store by store (X, Y: tables as icelk_internal.h states them).
//   k_resize_rows  grid (ceil(ow / 256), rows): row r = blockIdx.y < rows, outputs x0 .. xl <= ow - 1.  Table loads at
//                  x0, xl and x < ow, weights at x pitch + j, j < count[x] <= pitch.  Source: pixels s0 = first[x0] ..
//                  s1 - 1 = first[xl] + count[xl] - 1 <= in - 1 of row r, bytes g0 = row + 3 s0 .. g1 - 1; a staged dword
//                  is loaded whole only where all four bytes lie in [g0, g1), byte by byte inside [g0, g1) otherwise.
//                  LDS: dword d < ceil((shift + 3 span) / 4) <= (3 + 3 kStage + 3) / 4 < kStageWords; a tap reads byte
//                  shift + 3 (first[x] - s0 + j) + c < shift + 3 span, because first[x] + count[x] <= s1.  The global form
//                  reads row + 3 (first[x] + j) + c, first[x] + j < in.  Stores: dst + r dst_pitch + 3 x + c, x < ow, c < 3,
//                  dst_pitch >= 3 ow
//   k_resize_cols  grid (ceil(ceil(3 ow / 4) / 256), oh): y = blockIdx.y < oh, bytes b .. b + nv - 1 <= 3 ow - 1 of a row.
//                  Loads: src + (first[y] - lo + j) src_pitch + b, 0 <= first[y] - lo + j < the rows src holds (lo <= first[y],
//                  first[y] + count[y] <= hi), a dword only where nv == 4 and the address is aligned.  Stores likewise at
//                  dst + y dst_pitch + b
#include "icelk_internal.h"

namespace icelk {

namespace {

constexpr int kResizeThreads = 256;
constexpr int kStage = 1024;                            // source pixels a workgroup stages
constexpr int kStageWords = (3 * kStage + 6 + 3) / 4 + 1;

// n bytes (1 .. 4) at p as one little-endian word; one load where p is aligned and all four are wanted
__device__ __forceinline__ uint32_t load_bytes(const uint8_t* p, int n)
{
    if (n == 4 && ((uintptr_t)p & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = 0;
    for (int i = 0; i < n; i++) v |= (uint32_t)p[i] << (8 * i);
    return v;
}
__device__ __forceinline__ void store_bytes(uint8_t* p, int n, uint32_t v)
{
    if (n == 4 && ((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<uint32_t*>(p) = v;
        return;
    }
    for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i));
}

__global__ __launch_bounds__(kResizeThreads) void k_resize_rows(const uint8_t* __restrict__ src, size_t src_pitch, ResizeAxis X, int ow,
                                                                uint8_t* __restrict__ dst, size_t dst_pitch)
{
    __shared__ uint32_t stage[kStageWords];
    const int x0 = blockIdx.x * kResizeThreads, xl = x0 + kResizeThreads - 1 < ow - 1 ? x0 + kResizeThreads - 1 : ow - 1;
    const int x = x0 + (int)threadIdx.x;
    const int s0 = X.first[x0], s1 = X.first[xl] + X.count[xl], span = s1 - s0;
    const uint8_t* row = src + (size_t)blockIdx.y * src_pitch;
    const bool staged = span <= kStage;   // the same for the whole workgroup
    int shift = 0;
    if (staged) {
        const uint8_t *g0 = row + 3 * (size_t)s0, *g1 = g0 + 3 * (size_t)span;
        shift = (int)((uintptr_t)g0 & 3);
        const uint8_t* ga = g0 - shift;
        const int words = (shift + 3 * span + 3) / 4;
        for (int d = threadIdx.x; d < words; d += kResizeThreads) {
            const uint8_t* p = ga + 4 * (size_t)d;
            uint32_t v = 0;
            if (p >= g0 && p + 4 <= g1) {
                v = *reinterpret_cast<const uint32_t*>(p);
            } else {
                for (int i = 0; i < 4; i++)
                    if (p + i >= g0 && p + i < g1) v |= (uint32_t)p[i] << (8 * i);
            }
            stage[d] = v;
        }
        __syncthreads();
    }
    if (x >= ow) return;
    const int first = X.first[x], n = X.count[x];
    const int32_t* k = X.k + (size_t)x * X.pitch;
    uint8_t* out = dst + (size_t)blockIdx.y * dst_pitch + 3 * (size_t)x;
    if (staged) {
        const uint8_t* s = reinterpret_cast<const uint8_t*>(stage) + shift + 3 * (first - s0);
        for (int c = 0; c < 3; c++) out[c] = resize::sample(s + c, 3, k, n);
    } else {
        const uint8_t* s = row + 3 * (size_t)first;
        int32_t acc[3] = {1 << (resize::kBits - 1), 1 << (resize::kBits - 1), 1 << (resize::kBits - 1)};
        for (int j = 0; j < n; j++)
            for (int c = 0; c < 3; c++) acc[c] += k[j] * (int32_t)s[3 * (size_t)j + c];
        for (int c = 0; c < 3; c++) out[c] = resize::clip8(acc[c]);
    }
}

__global__ __launch_bounds__(kResizeThreads) void k_resize_cols(const uint8_t* __restrict__ src, size_t src_pitch, int lo, ResizeAxis Y,
                                                                int row_bytes, uint8_t* __restrict__ dst, size_t dst_pitch)
{
    const int y = blockIdx.y;
    const int first = Y.first[y] - lo, n = Y.count[y];   // the same for the whole workgroup
    const int32_t* k = Y.k + (size_t)y * Y.pitch;
    const int b = 4 * (int)(blockIdx.x * kResizeThreads + threadIdx.x);
    if (b >= row_bytes) return;
    const int nv = row_bytes - b < 4 ? row_bytes - b : 4;
    int32_t acc[4];
    for (int i = 0; i < 4; i++) acc[i] = 1 << (resize::kBits - 1);
    const uint8_t* s = src + (size_t)first * src_pitch + b;
    for (int j = 0; j < n; j++) {
        const uint32_t v = load_bytes(s + (size_t)j * src_pitch, nv);
        const int32_t kj = k[j];
        for (int i = 0; i < 4; i++) acc[i] += kj * (int32_t)((v >> (8 * i)) & 255u);
    }
    uint32_t v = 0;
    for (int i = 0; i < 4; i++) v |= (uint32_t)resize::clip8(acc[i]) << (8 * i);
    store_bytes(dst + (size_t)y * dst_pitch + b, nv, v);
}

}  // namespace

void launch_resize_rows(hipStream_t s, const uint8_t* src, size_t src_pitch, int rows, const ResizeAxis& X, int ow, uint8_t* dst, size_t dst_pitch)
{
    const dim3 grid((ow + kResizeThreads - 1) / kResizeThreads, rows);
    hipLaunchKernelGGL(k_resize_rows, grid, dim3(kResizeThreads), 0, s, src, src_pitch, X, ow, dst, dst_pitch);
}

void launch_resize_cols(hipStream_t s, const uint8_t* src, size_t src_pitch, int lo, const ResizeAxis& Y, int ow, int oh, uint8_t* dst,
                        size_t dst_pitch)
{
    const int row_bytes = 3 * ow, lanes = (row_bytes + 3) / 4;
    const dim3 grid((lanes + kResizeThreads - 1) / kResizeThreads, oh);
    hipLaunchKernelGGL(k_resize_cols, grid, dim3(kResizeThreads), 0, s, src, src_pitch, lo, Y, row_bytes, dst, dst_pitch);
}

}  // namespace icelk
