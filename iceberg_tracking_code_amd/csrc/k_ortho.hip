// k_ortho.hip -- the orthophoto on the device: the arithmetic is ortho.h, which the host statement runs as well.
//
//   k_ortho_fill   a mosaic begun: one thread per raster pixel -- the fill colour, cover 0, best +inf
//   k_ortho_add    a camera's photograph gathered into the raster: one thread per raster pixel, workgroups of 256 as
//                  16 x 16 tiles of the raster, so that a tile's footprint in the source is compact and its neighbours'
//                  samples come out of L1 / L2 (a gather is uncoalesced by nature; the tile shape is what keeps it local).
//                  Camera, raster, source and options travel by value in the kernel arguments: they are wave-uniform and
//                  sit in scalar registers; the three quotients by H are formed per thread from them, two double divisions
//                  by den remain per pixel.  No trigonometry, no libm, no atomics: additions are launches on one stream
//                  and a pixel belongs to one thread.  A thread that does not change its pixel stores nothing
//
// Bounds, load by load and store by store.  The raster is R.width x R.height with 1 <= R.width, R.height <= 16384 (checked by
// icelk_ortho_begin); rgb holds at least 3 R.width R.height bytes (picture_grow), cover R.width R.height bytes and best
// R.width R.height doubles (abi_ortho.hip sizes both at begin).  The source is S.w x S.h samples of S.channels (1 | 3) bytes,
// rows S.pitch >= S.w S.channels bytes apart, in an allocation of at least S.h S.pitch bytes (abi_ortho.hip: the upload, the
// decoder's R G B or luma plane, a frame slot's level 0); 1 <= S.w, S.h <= 65535.
//   k_ortho_fill   grid ceil(width height / 256): thread t < width height
//       stores     rgb + 3 t .. + 2 < 3 width height; cover + t; best + t
//   k_ortho_add    grid (ceil(width / 16), ceil(height / 16)), block (16, 16): pixel i = 16 blockIdx.x + threadIdx.x,
//                  j = 16 blockIdx.y + threadIdx.y; a thread with i >= width or j >= height returns before any access.
//                  t = j width + i < width height
//       loads      best + t; then, only where ortho::locate says seen, i.e. 0 <= xs <= S.w - 1 and 0 <= ys <= S.h - 1 in
//                  doubles (a NaN is not seen), the samples of ortho::sample: fx = (int)(256 xs) in 0 .. 256 (S.w - 1), so
//                  0 <= ix = fx >> 8 <= S.w - 1, ix1 = min(ix + 1, S.w - 1), nearest (fx + 128) >> 8 <= S.w - 1, rows
//                  likewise below S.h; a sample is the S.channels bytes at px + row pitch + column channels, the last of
//                  them at most (S.h - 1) pitch + (S.w - 1) channels + channels - 1 < S.h pitch
//       stores     only where the pixel changes: rgb + 3 t .. + 2, cover + t, best + t, as above
#include "icelk_internal.h"

namespace icelk {

namespace {

constexpr int kOrthoThreads = 256;

struct OrthoFill {
    uint8_t c[3];
};

__global__ __launch_bounds__(kOrthoThreads) void k_ortho_fill(int n, OrthoFill fill, uint8_t* __restrict__ rgb, uint8_t* __restrict__ cover,
                                                               double* __restrict__ best)
{
    const int t = blockIdx.x * kOrthoThreads + threadIdx.x;
    if (t >= n) return;
    uint8_t* o = rgb + 3 * (size_t)t;
    o[0] = fill.c[0], o[1] = fill.c[1], o[2] = fill.c[2];
    cover[t] = 0;
    best[t] = ortho::infinity();
}

__global__ __launch_bounds__(kOrthoThreads) void k_ortho_add(icelk_camera_t cam, icelk_ortho_raster_t R, ortho::Source S, double max_range,
                                                              int sampling, int index, uint8_t* __restrict__ rgb, uint8_t* __restrict__ cover,
                                                              double* __restrict__ best)
{
    const int i = blockIdx.x * ortho::kTile + threadIdx.x, j = blockIdx.y * ortho::kTile + threadIdx.y;
    if (i >= R.width || j >= R.height) return;
    const size_t t = (size_t)j * R.width + i;
    uint8_t px[3];
    double d2;
    if (!ortho::add_pixel(cam, R, S, max_range, sampling, i, j, best[t], px, &d2)) return;
    uint8_t* o = rgb + 3 * t;
    o[0] = px[0], o[1] = px[1], o[2] = px[2];
    cover[t] = (uint8_t)(index + 1);
    best[t] = d2;
}

}  // namespace

void launch_ortho_fill(hipStream_t s, int width, int height, const uint8_t* fill, uint8_t* rgb, uint8_t* cover, double* best)
{
    const int n = width * height;   // <= 2^28
    OrthoFill f{{fill[0], fill[1], fill[2]}};
    hipLaunchKernelGGL(k_ortho_fill, dim3((n + kOrthoThreads - 1) / kOrthoThreads), dim3(kOrthoThreads), 0, s, n, f, rgb, cover, best);
}

void launch_ortho_add(hipStream_t s, const icelk_camera_t& cam, const icelk_ortho_raster_t& R, const ortho::Source& S, double max_range,
                      int sampling, int index, uint8_t* rgb, uint8_t* cover, double* best)
{
    static_assert(ortho::kTile * ortho::kTile == kOrthoThreads, "a tile is a workgroup");
    const dim3 grid((R.width + ortho::kTile - 1) / ortho::kTile, (R.height + ortho::kTile - 1) / ortho::kTile);
    hipLaunchKernelGGL(k_ortho_add, grid, dim3(ortho::kTile, ortho::kTile), 0, s, cam, R, S, max_range, sampling, index, rgb, cover, best);
}

}  // namespace icelk
