// jpeg_crop_fwd_host.h -- the host statement of the fused crop-and-forward kernel (k_jpeg_crop_fwd, k_jpeg_fwd.hip): phase 1
// from a decoded file's component planes -- jpeg_rgb.h, the code the kernel runs, walked as the kernel walks it: four
// neighbouring pixels of a crop row per rgbpx::crop_row4 call, from columns that are multiples of 4, the right-edge clamp
// inside that call -- followed by the host statement of the forward half as it stands (jpeg_resave_host.h).  Plain C++ without the HIP runtime:
// tests/jpeg_crop_fwd_host_main.cpp runs it under the host's sanitizers on planes exactly as large as jpeg_plane_args
// (abi_jpeg_ingest.hip) makes them.
#pragma once
#include "jpeg_resave_host.h"
#include "jpeg_rgb.h"

namespace icelk {
namespace resave {

// The coefficients of the file Pillow would write for `Image.open(file).crop(box)`: P are the file's planes, the box is
// w x h pixels whose pixel (0, 0) is image pixel (left, top); it must lie inside the image (the callers' crop check).
inline int coefficients_from_planes(const rgbpx::Planes& P, int left, int top, int w, int h, int quality, icelk_jpeg_info_t* info,
                                    int16_t* coef, uint64_t capacity)
{
    if (left < 0 || top < 0 || w < 1 || left + w > P.W) return ICELK_EARG;
    // the four pixels made last: coefficients_from asks for neighbours of a row one after the other
    rgbpx::Rgb four[4];
    int at_row = -1, at_x0 = -1;
    return coefficients_from(
        [&](int y, int x) {
            const int x0 = x & ~3;
            if (y != at_row || x0 != at_x0) {
                rgbpx::crop_row4_any(P, left, top, w, x0, y, four);
                at_row = y, at_x0 = x0;
            }
            const rgbpx::Rgb& p = four[x & 3];
            return Pixel{p.r, p.g, p.b};
        },
        w, h, quality, info, coef, capacity);
}

}  // namespace resave
}  // namespace icelk
