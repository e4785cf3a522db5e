// k_plot.hip -- the segment picture on the device: the arithmetic is plot_raster.h, which the host statement
// (icelk_plot_overlay_host) runs as well.
//
//   k_plot_background   gray level 0 of a slot -> the Wo x Ho area-averaged gray plane.  The only kernel here that
//                       touches full-frame data.  One workgroup makes 256 neighbouring pixels of one output row: its
//                       lanes first sum, column by column with the rows' vertical weights, the source rows of that output
//                       row -- each lane four neighbouring columns from one dword per row, so a row is read coalesced and
//                       once for all the output pixels above it -- into LDS, 1024 columns at a time; then every lane
//                       adds up, with the horizontal weights, the few column sums of its own pixel.  Exact: the weights
//                       are integers and the sums are products of sums.
//   k_picture_clear     zeroes the two count planes (and the three planes of the velocity map: abi_map.hip)
//   k_plot_scatter      one thread per pair of consecutive vertices and one per track for the dot; the walk is bounded
//                       by max(Wo, Ho) steps whatever the coordinates, hits are counted with integer atomics, so the
//                       result does not depend on the order of arrival
//   k_plot_resolve      counts + background + tables + stamp -> interleaved R G B, rows 3 Wo bytes apart (what the
//                       picture writer reads); a thread makes four pixels and stores three dwords (picture_raster.h)
#include "icelk_internal.h"
#include "picture_raster.h"

namespace icelk {

namespace {

constexpr int kBgThreads = 256;
constexpr int kBgChunk = 4 * kBgThreads;   // source columns summed per pass

__global__ __launch_bounds__(kBgThreads) void k_plot_background(Level src, int Wo, int Ho, uint8_t* __restrict__ bg)
{
    __shared__ uint32_t col[kBgChunk];   // sum over the rows of wy * g: at most H * 255 < 2^24
    const int W = src.w, H = src.h;
    const int j = blockIdx.y, i_first = blockIdx.x * kBgThreads, i = i_first + (int)threadIdx.x;
    const int i_last = i_first + kBgThreads - 1 < Wo - 1 ? i_first + kBgThreads - 1 : Wo - 1;
    const int y0 = plot::first_source(j, H, Ho), y1 = plot::last_source(j, H, Ho);
    // the columns this workgroup's pixels draw on, from a dword boundary; xe <= W
    const int xs = plot::first_source(i_first, W, Wo) & ~3, xe = plot::last_source(i_last, W, Wo) + 1;
    int my0 = 0, my1 = -1;
    if (i < Wo) {
        my0 = plot::first_source(i, W, Wo);
        my1 = plot::last_source(i, W, Wo);
    }
    uint64_t acc = 0;
    for (int base = xs; base < xe; base += kBgChunk) {
        const int x4 = base + 4 * (int)threadIdx.x;
        if (x4 < xe) {
            // x4 is a multiple of 4 below W, rows start 64-byte aligned and are a multiple of 64 bytes long: the dword lies
            // inside the row.  Columns at or beyond W in it carry no weight below
            uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
            for (int y = y0; y <= y1; y++) {
                const uint32_t wy = (uint32_t)plot::overlap(y, j, H, Ho);
                const uint32_t v = *reinterpret_cast<const uint32_t*>(src.ptr + (size_t)y * src.pitch + x4);
                s0 += wy * (v & 255u);
                s1 += wy * ((v >> 8) & 255u);
                s2 += wy * ((v >> 16) & 255u);
                s3 += wy * (v >> 24);
            }
            *reinterpret_cast<uint4*>(&col[4 * threadIdx.x]) = make_uint4(s0, s1, s2, s3);
        }
        __syncthreads();
        const int lo = my0 > base ? my0 : base, hi = my1 < base + kBgChunk - 1 ? my1 : base + kBgChunk - 1;
        for (int x = lo; x <= hi; x++) acc += (uint64_t)plot::overlap(x, i, W, Wo) * col[x - base];
        __syncthreads();
    }
    if (i < Wo) bg[(size_t)j * Wo + i] = (uint8_t)plot::average(acc, W, H);
}

__global__ __launch_bounds__(256) void k_picture_clear(uint4* __restrict__ planes, size_t n16)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n16) planes[k] = make_uint4(0, 0, 0, 0);
}

struct CountHit {
    uint32_t* plane;
    int Wo;
    __device__ __forceinline__ void operator()(int px, int py) const { atomicAdd(plane + (size_t)py * Wo + px, 1u); }
};

__global__ __launch_bounds__(256) void k_plot_scatter(const float* __restrict__ tracks, int n, int nv, int W, int H, int Wo, int Ho,
                                                      uint32_t* __restrict__ lines, uint32_t* __restrict__ dots)
{
    const int pairs = n * (nv - 1);
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= pairs + n) return;
    const bool dot = t >= pairs;
    const int track = dot ? t - pairs : t / (nv - 1);
    const float* v = tracks + (size_t)track * nv * 2;
    for (int k = 0; k < nv; k++)
        if (!plot::vertex_ok(v[2 * k], v[2 * k + 1])) return;   // the track is left out whole
    if (dot) {
        plot::walk_dot(plot::coord(v[2 * nv - 2], Wo, W), plot::coord(v[2 * nv - 1], Ho, H), Wo, Ho, CountHit{dots, Wo});
        return;
    }
    const int k = t - track * (nv - 1);
    plot::walk_pair(plot::coord(v[2 * k], Wo, W), plot::coord(v[2 * k + 1], Ho, H), plot::coord(v[2 * k + 2], Wo, W),
                    plot::coord(v[2 * k + 3], Ho, H), Wo, Ho, CountHit{lines, Wo});
}

struct PlotTables {
    uint32_t TL[plot::kTable], TD[plot::kTable];
};

// bg, lines and dots are padded to a multiple of four pixels (the padding is never resolved)
__global__ __launch_bounds__(256) void k_plot_resolve(const uint8_t* __restrict__ bg, const uint32_t* __restrict__ lines,
                                                      const uint32_t* __restrict__ dots, const PlotTables* __restrict__ tab, plot::Stamp stamp,
                                                      int Wo, int Ho, uint8_t* __restrict__ rgb)
{
    __shared__ PlotTables T;
    if (threadIdx.x < plot::kTable) {
        T.TL[threadIdx.x] = tab->TL[threadIdx.x];
        T.TD[threadIdx.x] = tab->TD[threadIdx.x];
    }
    __syncthreads();
    const size_t total = (size_t)Wo * Ho, p0 = 4 * ((size_t)blockIdx.x * 256 + threadIdx.x);
    if (p0 >= total) return;
    const uint32_t g4 = *reinterpret_cast<const uint32_t*>(bg + p0);
    const uint4 l4 = *reinterpret_cast<const uint4*>(lines + p0), d4 = *reinterpret_cast<const uint4*>(dots + p0);
    const uint32_t l[4] = {l4.x, l4.y, l4.z, l4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w};
    picture::resolve_quad(p0, total, Wo, rgb, [&](int k, int px, int py, uint8_t* out) {
        plot::resolve_pixel((int)((g4 >> (8 * k)) & 255u), l[k], d[k], T.TL, T.TD, stamp, px, py, Wo, Ho, out);
    });
}

}  // namespace

void launch_plot_background(hipStream_t s, const Level& src, int Wo, int Ho, uint8_t* bg)
{
    hipLaunchKernelGGL(k_plot_background, dim3((Wo + kBgThreads - 1) / kBgThreads, Ho), dim3(kBgThreads), 0, s, src, Wo, Ho, bg);
}

// words: a multiple of four, from an allocation's start
void launch_picture_clear(hipStream_t s, uint32_t* planes, size_t words)
{
    const size_t n16 = words / 4;
    if (!n16) return;
    hipLaunchKernelGGL(k_picture_clear, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<uint4*>(planes), n16);
}

void launch_plot_scatter(hipStream_t s, const float* tracks, int n, int nv, int W, int H, int Wo, int Ho, uint32_t* lines, uint32_t* dots)
{
    if (n <= 0) return;
    const int threads = n * nv;   // n (nv - 1) pairs + n dots
    hipLaunchKernelGGL(k_plot_scatter, dim3((threads + 255) / 256), dim3(256), 0, s, tracks, n, nv, W, H, Wo, Ho, lines, dots);
}

void launch_plot_resolve(hipStream_t s, const uint8_t* bg, const uint32_t* lines, const uint32_t* dots, const uint32_t* tables,
                         const plot::Stamp& stamp, int Wo, int Ho, uint8_t* rgb)
{
    const size_t quads = ((size_t)Wo * Ho + 3) / 4;
    hipLaunchKernelGGL(k_plot_resolve, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, bg, lines, dots,
                       reinterpret_cast<const PlotTables*>(tables), stamp, Wo, Ho, rgb);
}

}  // namespace icelk
