// k_map.hip -- the velocity map of a gridded window on the device: the arithmetic is map_raster.h, which the host statement
// (icelk_map_overlay_host) runs as well.
//
//   k_map_cells      one thread per cell: the interior of an unmeasured cell row by row over its rectangle clipped to the
//                    view, the four sides through walk_pair; atomicMax of the code into `base`
//   k_map_polyline   one thread per pair of consecutive outline vertices, atomicMax of code 3 into `base`
//   k_map_arrows     one thread per arrow: shaft walk and head fill, each hit atomicMax(top, index + 1) and
//                    atomicAdd(count, 1).  With a group array a thread whose arrow is not of the wanted group returns at
//                    once: one resident upload of a day's vectors serves every window's picture.  The work of a thread is
//                    bounded by 7 max(vw, vh) + 97^2 hits whatever the arrow's numbers
//   k_map_resolve    planes + scene (views, cameras, tables, texts, colour table) -> interleaved R G B, rows 3 Wo bytes
//                    apart (what the picture writer reads); a thread makes four pixels and stores three dwords
//                    (picture_raster.h).  The arrow's speed is gathered through `top`
// The three planes (base | top | count) are zeroed by k_picture_clear (k_plot.hip).
// Every atomic goes to plane[(y0 + q) Wo + x0 + p] with 0 <= p < vw, 0 <= q < vh -- map_raster.h hands out no other
// pixel -- and the view lies inside the Wo x Ho picture (abi_map.hip checks it before anything is enqueued).
#include "icelk_internal.h"
#include "picture_raster.h"

namespace icelk {

namespace {

struct BaseHit {
    uint32_t* base;
    int Wo, x0, y0;
    uint32_t code;
    __device__ __forceinline__ void operator()(int p, int q) const { atomicMax(base + (size_t)(y0 + q) * Wo + (x0 + p), code); }
};

struct ArrowHit {
    uint32_t *top, *count;
    int Wo, x0, y0;
    uint32_t id;   // index + 1
    __device__ __forceinline__ void operator()(int p, int q) const
    {
        const size_t o = (size_t)(y0 + q) * Wo + (x0 + p);
        atomicMax(top + o, id);
        atomicAdd(count + o, 1u);
    }
};

__global__ __launch_bounds__(256) void k_map_cells(map::View V, const double* __restrict__ cells, const uint8_t* __restrict__ measured, int n,
                                                   int Wo, uint32_t* __restrict__ base)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    map::walk_cell(V, cells[3 * (size_t)t], cells[3 * (size_t)t + 1], cells[3 * (size_t)t + 2], measured[t] != 0, BaseHit{base, Wo, V.x0, V.y0, 1u},
                   BaseHit{base, Wo, V.x0, V.y0, 2u});
}

__global__ __launch_bounds__(256) void k_map_polyline(map::View V, const double* __restrict__ xy, int n, int Wo, uint32_t* __restrict__ base)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t + 1 >= n) return;
    map::walk_segment(V, xy[2 * (size_t)t], xy[2 * (size_t)t + 1], xy[2 * (size_t)t + 2], xy[2 * (size_t)t + 3], BaseHit{base, Wo, V.x0, V.y0, 3u});
}

__global__ __launch_bounds__(256) void k_map_arrows(map::View V, int w, int pivot_mid, const double* __restrict__ arrows,
                                                    const int32_t* __restrict__ group, int want, int n, int Wo, uint32_t* __restrict__ top,
                                                    uint32_t* __restrict__ count)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    if (group && group[t] != want) return;
    const double* a = arrows + 5 * (size_t)t;
    map::walk_arrow(V, w, pivot_mid != 0, a[0], a[1], a[2], a[3], a[4], ArrowHit{top, count, Wo, V.x0, V.y0, (uint32_t)t + 1u});
}

// the planes are padded to a multiple of four pixels (the padding is never resolved)
__global__ __launch_bounds__(256) void k_map_resolve(const map::Scene* __restrict__ scene, const uint32_t* __restrict__ base,
                                                     const uint32_t* __restrict__ top, const uint32_t* __restrict__ count, uint8_t* __restrict__ rgb)
{
    const map::Scene& S = *scene;
    const int Wo = S.Wo;
    const size_t total = (size_t)Wo * S.Ho, p0 = 4 * ((size_t)blockIdx.x * 256 + threadIdx.x);
    if (p0 >= total) return;
    const uint4 b4 = *reinterpret_cast<const uint4*>(base + p0), t4 = *reinterpret_cast<const uint4*>(top + p0),
                c4 = *reinterpret_cast<const uint4*>(count + p0);
    const uint32_t b[4] = {b4.x, b4.y, b4.z, b4.w}, t[4] = {t4.x, t4.y, t4.z, t4.w}, c[4] = {c4.x, c4.y, c4.z, c4.w};
    picture::resolve_quad(p0, total, Wo, rgb, [&](int k, int px, int py, uint8_t* out) { map::resolve_pixel(S, b[k], t[k], c[k], px, py, out); });
}

}  // namespace

void launch_map_cells(hipStream_t s, const map::View& V, const double* cells, const uint8_t* measured, int n, int Wo, uint32_t* base)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_map_cells, dim3((n + 255) / 256), dim3(256), 0, s, V, cells, measured, n, Wo, base);
}

void launch_map_polyline(hipStream_t s, const map::View& V, const double* xy, int n, int Wo, uint32_t* base)
{
    if (n < 2) return;
    hipLaunchKernelGGL(k_map_polyline, dim3((n - 1 + 255) / 256), dim3(256), 0, s, V, xy, n, Wo, base);
}

void launch_map_arrows(hipStream_t s, const map::View& V, int w, bool pivot_mid, const double* arrows, const int32_t* group, int want, int n,
                       int Wo, uint32_t* top, uint32_t* count)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_map_arrows, dim3((n + 255) / 256), dim3(256), 0, s, V, w, pivot_mid ? 1 : 0, arrows, group, want, n, Wo, top, count);
}

void launch_map_resolve(hipStream_t s, const map::Scene* d_scene, int Wo, int Ho, const uint32_t* base, const uint32_t* top,
                        const uint32_t* count, uint8_t* rgb)
{
    const size_t quads = ((size_t)Wo * Ho + 3) / 4;
    hipLaunchKernelGGL(k_map_resolve, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, d_scene, base, top, count, rgb);
}

}  // namespace icelk
