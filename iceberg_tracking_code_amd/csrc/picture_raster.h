// picture_raster.h -- what the resolve kernels of the segment picture (k_plot.hip) and of the velocity map (k_map.hip)
// share: the walk of one thread over its four pixels and the store of their interleaved R G B.  What a pixel looks like
// stays with plot_raster.h and map_raster.h; it comes in as a functor, the way walk_pair takes its Hit.
#pragma once
#include <stdint.h>

namespace icelk {
namespace picture {

// Pixels p0 .. p0 + 3 (p0 a multiple of four below total) of a picture Wo wide and `total` pixels large at rgb.
// pixel(k, px, py, out) writes the three bytes of pixel p0 + k, which lies at (px, py), carried across a row end.  Four live
// pixels leave as three packed dwords -- rgb + 3 p0 is a 12-byte step from an allocation's start: dword aligned --, the
// picture's last one to three byte by byte: nothing is stored at or beyond rgb + 3 total
template <typename Pixel>
__device__ __forceinline__ void resolve_quad(size_t p0, size_t total, int Wo, uint8_t* __restrict__ rgb, Pixel pixel)
{
    uint8_t out[12] = {0};
    int py = (int)(p0 / (size_t)Wo), px = (int)(p0 - (size_t)py * Wo);
    const int live = total - p0 < 4 ? (int)(total - p0) : 4;
    for (int k = 0; k < live; k++) {
        pixel(k, px, py, out + 3 * k);
        if (++px == Wo) px = 0, py++;
    }
    uint8_t* dst = rgb + 3 * p0;
    if (live == 4) {
        uint32_t* q = reinterpret_cast<uint32_t*>(dst);
        for (int k = 0; k < 3; k++)
            q[k] = (uint32_t)out[4 * k] | (uint32_t)out[4 * k + 1] << 8 | (uint32_t)out[4 * k + 2] << 16 | (uint32_t)out[4 * k + 3] << 24;
    } else {
        for (int k = 0; k < 3 * live; k++) dst[k] = out[k];
    }
}

}  // namespace picture
}  // namespace icelk
