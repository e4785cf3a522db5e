// k_thumb.hip -- the inset photographs of the velocity map on the device: the arithmetic is thumb_raster.h (and jpeg_rgb.h
// for the photo's pixels), which the host statements run as well.
//
//   k_jpeg_thumb   a decoded file's component planes -> its Wt x Ht thumbnail, interleaved R G B; the full-size R G B is
//                  never stored.  A workgroup makes `per` neighbouring pixels of one output row, `per` chosen by the
//                  launcher so that the source columns under them fill one pass of 256 columns (at 4000 -> 267 columns:
//                  16 pixels, 17 workgroups per output row).  Each quarter of the workgroup takes every fourth source row of
//                  that output row, each of its 64 lanes four neighbouring columns through rgbpx::rgb4<mode>, every group of
//                  samples ONE dword load: a source row is read coalesced and once for all the output pixels above it, and
//                  the chain of dependent loads a lane walks is a quarter of the rows -- with one lane per four columns
//                  walking all fifteen rows of a 4000 x 3000 photo the kernel waits for memory latency, 44 against 29 us
//                  for k_jpeg_out on the same planes.  The quarters' column sums, weighted with the rows' vertical weights,
//                  go to LDS, 4 x 3 x 256 words; then one lane per (pixel, channel) adds up, with the horizontal weights,
//                  the few columns under its pixel.  A 4:2:0 file's far chroma row is the near row of the luma row's
//                  neighbour: it comes from cache.
//                  Exact: integer weights; a column sum is at most H 255 < 2^24 (the vertical weights of an output row add
//                  up to H <= 65535) in uint32, a pixel's sum at most W H 255 < 2^40 (the horizontal weights add up to
//                  W <= 65535) in uint64.  Columns rgb4 returns beyond W lie beyond every output pixel: their overlap is 0,
//                  and the sums stop at last_source <= W - 1 anyway.  mode 5: a one-component file, R = G = B
//   k_map_inset    one inset into the map's R G B: a thread per pixel of the rectangle thumbnail and label cover, clipped
//                  to the picture; three byte stores where the inset changes the pixel.  One launch per inset, in array
//                  order on the one stream: a later inset covers an earlier one
// Bounds are stated store by store in abi_thumb.hip's header.
#include "icelk_internal.h"
#include "jpeg_rgb.h"

namespace icelk {

namespace {

constexpr int kThumbThreads = thumb::kThreads, kThumbChunk = thumb::kChunk, kThumbRowGroups = thumb::kRowGroups;
constexpr int kThumbLanes = kThumbThreads / kThumbRowGroups;   // lanes of a quarter: four columns each

template <int mode>
__global__ __launch_bounds__(kThumbThreads) void k_jpeg_thumb(JpegOutArgs A, int Wt, int Ht, int per)
{
    constexpr int NC = mode == 5 ? 1 : 3, G = NC == 3 ? 1 : 0, B = NC == 3 ? 2 : 0;   // one component: the three channels are one
    // per quarter and channel, the sum over the quarter's rows of wy * channel: the quarters' sums add up to at most H * 255 < 2^24
    __shared__ uint32_t col[kThumbRowGroups][NC][kThumbChunk];
    const int W = A.ow, H = A.oh;
    // a quarter is a wave: saying so keeps the row, its weight and the rows' addresses in scalar registers
    static_assert(kThumbLanes == 64, "a quarter of the workgroup is one wave of gfx950");
    const int quarter = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kThumbLanes), lane = (int)threadIdx.x % kThumbLanes;
    const int j = blockIdx.y, i_first = blockIdx.x * per;
    const int i_last = i_first + per - 1 < Wt - 1 ? i_first + per - 1 : Wt - 1;   // i_first < Wt: the grid is ceil(Wt / per) wide
    const int y0 = plot::first_source(j, H, Ht), y1 = plot::last_source(j, H, Ht);
    // the columns this workgroup's pixels draw on, from a dword boundary; xe <= W
    const int xs = plot::first_source(i_first, W, Wt) & ~3, xe = plot::last_source(i_last, W, Wt) + 1;
    rgbpx::Planes P;
    for (int k = 0; k < 3; k++) P.plane[k] = A.plane[k], P.pitch[k] = A.pitch[k];
    P.W = W, P.cw = A.cw, P.ch = A.ch, P.mode = A.mode;
    // the (pixel, channel) pairs of the workgroup, at most 3 kMaxPer <= 256: a lane has one
    const int pair = (int)threadIdx.x, pairs = (i_last - i_first + 1) * NC;
    const int i = i_first + pair / NC, c = pair % NC;
    uint64_t acc = 0;
    for (int base = xs; base < xe; base += kThumbChunk) {
        const int x4 = base + 4 * lane;
        if (x4 < xe) {   // x4 < W
            uint32_t s[NC][4];
#pragma unroll
            for (int c = 0; c < NC; c++)
#pragma unroll
                for (int k = 0; k < 4; k++) s[c][k] = 0;
            for (int y = y0 + quarter; y <= y1; y += kThumbRowGroups) {
                const uint32_t wy = (uint32_t)plot::overlap(y, j, H, Ht);
                if constexpr (mode == 5) {
                    int lum[4];
                    rgbpx::load4(P.plane[0] + (size_t)y * P.pitch[0], x4, W, lum);
#pragma unroll
                    for (int k = 0; k < 4; k++) s[0][k] += wy * (uint32_t)lum[k];
                } else {
                    rgbpx::Rgb px[4];
                    rgbpx::rgb4<mode>(P, x4, y, px);
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        s[0][k] += wy * (uint32_t)px[k].r;
                        s[G][k] += wy * (uint32_t)px[k].g;
                        s[B][k] += wy * (uint32_t)px[k].b;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NC; c++) *reinterpret_cast<uint4*>(&col[quarter][c][4 * lane]) = make_uint4(s[c][0], s[c][1], s[c][2], s[c][3]);
        }
        __syncthreads();
        if (pair < pairs) {
            const int my0 = plot::first_source(i, W, Wt), my1 = plot::last_source(i, W, Wt);
            const int lo = my0 > base ? my0 : base, hi = my1 < base + kThumbChunk - 1 ? my1 : base + kThumbChunk - 1;
            acc += thumb::row_sum(&col[0][c][0], kThumbRowGroups, NC * kThumbChunk, base, lo, hi, i, W, Wt);
        }
        __syncthreads();
    }
    if (pair < pairs) {
        uint8_t* d = A.dst + (size_t)j * A.dst_pitch + 3 * (size_t)i;
        const uint8_t v = (uint8_t)plot::average(acc, W, H);
        if (NC == 1) d[0] = d[1] = d[2] = v;
        else d[c] = v;
    }
}

__global__ __launch_bounds__(256) void k_map_inset(thumb::Inset I, int k, int bx0, int by0, int bw, int bh, int Wo, uint8_t* __restrict__ rgb)
{
    const int t = blockIdx.x * 256 + threadIdx.x;   // bw * bh <= 16384^2 = 2^28
    if (t >= bw * bh) return;
    const int py = by0 + t / bw, px = bx0 + t % bw;
    uint8_t out[3];
    if (!thumb::inset_pixel(I, k, px, py, out)) return;
    uint8_t* d = rgb + 3 * ((size_t)py * Wo + px);
    d[0] = out[0], d[1] = out[1], d[2] = out[2];
}

}  // namespace

// A: the planes of the whole file (left = top = 0, ow x oh the image), dst / dst_pitch the thumbnail; ncomp 1 or 3
void launch_jpeg_thumb(hipStream_t s, const JpegOutArgs& A, int ncomp, int Wt, int Ht)
{
    const int per = thumb::pixels_per_group(A.ow, Wt);
    const dim3 grid((Wt + per - 1) / per, Ht), block(kThumbThreads);
    switch (ncomp == 1 ? 5 : A.mode) {
    case 0: hipLaunchKernelGGL(k_jpeg_thumb<0>, grid, block, 0, s, A, Wt, Ht, per); break;
    case 1: hipLaunchKernelGGL(k_jpeg_thumb<1>, grid, block, 0, s, A, Wt, Ht, per); break;
    case 2: hipLaunchKernelGGL(k_jpeg_thumb<2>, grid, block, 0, s, A, Wt, Ht, per); break;
    case 3: hipLaunchKernelGGL(k_jpeg_thumb<3>, grid, block, 0, s, A, Wt, Ht, per); break;
    case 4: hipLaunchKernelGGL(k_jpeg_thumb<4>, grid, block, 0, s, A, Wt, Ht, per); break;
    default: hipLaunchKernelGGL(k_jpeg_thumb<5>, grid, block, 0, s, A, Wt, Ht, per); break;
    }
}

void launch_map_inset(hipStream_t s, const thumb::Inset& I, int Wo, int Ho, uint8_t* rgb)
{
    const int k = map::text_scale(Wo);
    int bx0, by0, bx1, by1;
    thumb::inset_box(I, k, Wo, Ho, &bx0, &by0, &bx1, &by1);
    if (bx1 <= bx0 || by1 <= by0) return;
    const int bw = bx1 - bx0, bh = by1 - by0;
    hipLaunchKernelGGL(k_map_inset, dim3((unsigned)(((size_t)bw * bh + 255) / 256)), dim3(256), 0, s, I, k, bx0, by0, bw, bh, Wo, rgb);
}

}  // namespace icelk
