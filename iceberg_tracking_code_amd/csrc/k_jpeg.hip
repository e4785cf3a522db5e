// k_jpeg.hip -- the device half of the JPEG ingest path for gfx950: quantised DCT coefficients -> pixels.
//
//   k_jpeg_idct   dequantise + 8x8 inverse DCT of the blocks a crop needs, into 8-bit component planes
//   k_jpeg_out    chroma upsampling + YCbCr -> RGB + crop, then either gray into a slot's level 0 or interleaved RGB
//
// Arithmetic: libjpeg's default decoder restated from its published description (tests/jpeg_restatement.py is the
// same in numpy, and is what Pillow's output is compared with): the "islow" inverse DCT -- the factorisation of
// Loeffler, Ligtenberg and Moschytz in 13-bit fixed point, the column pass keeping 2 extra bits --, "fancy" upsampling
// (a 3:1 triangle filter in each subsampled direction, edge samples repeated at the TRUE plane edges), and the 16-bit
// fixed-point colour matrix.  All integer, so equality with the host library is bit for bit.
//
// The planes go through HBM between the two kernels (18 MB at 12 MP 4:2:0); each is one pass over its data.
#include "icelk_internal.h"
#include "jpeg_rgb.h"

namespace icelk {

// 8-point inverse DCT of x[0..7] in place, descaled by `shift` with rounding.  32 bits are enough for a BLOCK an encoder
// makes: the forward DCT of 64 8-bit samples, give or take half a quantiser step per coefficient, which is what
// libjpeg's own analysis of its 32-bit "islow" transform assumes, and there the result equals libjpeg's bit for bit.
// No bound on the single coefficient says the same: a file may hold any 16-bit value, and +-255 at a table entry of 16
// (4080, well below 2^18) in every coefficient already carries the row pass's sums past 2^31.  So the products and
// sums are taken in uint32_t, where they wrap by definition instead of overflowing a signed int, and only the final
// shift is the arithmetic one of a signed value.  Inside an encoder's range nothing changes; outside it the result is
// that of two's complement 32-bit arithmetic, which no longer is what libjpeg (or its SIMD paths, which differ from
// its C code there) makes of the file.
template <int shift>
__device__ __forceinline__ void idct8(int (&xs)[8])
{
    uint32_t x[8];
#pragma unroll
    for (int k = 0; k < 8; k++) x[k] = (uint32_t)xs[k];
    // even part
    const uint32_t z = (x[2] + x[6]) * 4433u;
    const uint32_t e2 = z - x[6] * 15137u;
    const uint32_t e3 = z + x[2] * 6270u;
    const uint32_t e0 = (x[0] + x[4]) * 8192u;
    const uint32_t e1 = (x[0] - x[4]) * 8192u;
    const uint32_t a0 = e0 + e3, a3 = e0 - e3, a1 = e1 + e2, a2 = e1 - e2;
    // odd part
    const uint32_t z5 = (x[7] + x[3] + x[5] + x[1]) * 9633u;
    const uint32_t z3 = z5 - (x[7] + x[3]) * 16069u;
    const uint32_t z4 = z5 - (x[5] + x[1]) * 3196u;
    const uint32_t z1 = 0u - (x[7] + x[1]) * 7373u;
    const uint32_t z2 = 0u - (x[5] + x[3]) * 20995u;
    const uint32_t o0 = x[7] * 2446u + z1 + z3;
    const uint32_t o1 = x[5] * 16819u + z2 + z4;
    const uint32_t o2 = x[3] * 25172u + z2 + z3;
    const uint32_t o3 = x[1] * 12299u + z1 + z4;
    constexpr uint32_t half = 1u << (shift - 1);
    xs[0] = (int)(a0 + o3 + half) >> shift;
    xs[7] = (int)(a0 - o3 + half) >> shift;
    xs[1] = (int)(a1 + o2 + half) >> shift;
    xs[6] = (int)(a1 - o2 + half) >> shift;
    xs[2] = (int)(a2 + o1 + half) >> shift;
    xs[5] = (int)(a2 - o1 + half) >> shift;
    xs[3] = (int)(a3 + o0 + half) >> shift;
    xs[4] = (int)(a3 - o0 + half) >> shift;
}

using rgbpx::clamp255;

// ------------------------------------------------------------------------------------------------
// Inverse DCT.  8 lanes per block, 32 blocks per 256-thread workgroup.  Lane r of a block loads row r of the
// coefficients (16 B: a block is 128 contiguous bytes, a wave reads 1 KiB), dequantises, and writes it to the block's
// LDS tile; the same lane then owns COLUMN r for the column pass (which has to come first: its rounding is part of the
// result), writes the column back, and owns row r again for the row pass and the 8-byte store into the plane.
// The tile rows are padded to 9 dwords: 8 lanes x 4 blocks of a half wave then touch 32 different banks in both
// directions.  The 8 lanes of a block sit in one wave, but the tile is handed over with workgroup barriers all the same.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_jpeg_idct(JpegIdctArgs A)
{
    __shared__ int tile[32][8][9];
    __shared__ uint16_t quant[3][64];
    if (threadIdx.x < 192) quant[threadIdx.x >> 6][threadIdx.x & 63] = A.quant[threadIdx.x >> 6][threadIdx.x & 63];
    __syncthreads();
    const int g = threadIdx.x >> 3, r = threadIdx.x & 7;
    const int blk = blockIdx.x * 32 + g;
    const bool live = blk < A.first[3];
    int c = 0, bx = 0, by = 0;
    if (live) {
        c = blk >= A.first[2] ? 2 : (blk >= A.first[1] ? 1 : 0);
        const int k = blk - A.first[c];
        by = A.by0[c] + k / A.nbx[c];
        bx = A.bx0[c] + k % A.nbx[c];
        const int16_t* src = A.coef[c] + ((size_t)by * A.blocks_x[c] + bx) * 64 + r * 8;
        const uint4 raw = *reinterpret_cast<const uint4*>(src);
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int k2 = 0; k2 < 4; k2++) {
            tile[g][r][2 * k2] = (int)(int16_t)(w[k2] & 0xffffu) * (int)quant[c][r * 8 + 2 * k2];
            tile[g][r][2 * k2 + 1] = ((int)w[k2] >> 16) * (int)quant[c][r * 8 + 2 * k2 + 1];
        }
    }
    __syncthreads();
    int x[8];
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = tile[g][k][r];
        idct8<11>(x);
#pragma unroll
        for (int k = 0; k < 8; k++) tile[g][k][r] = x[k];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = tile[g][r][k];
        idct8<18>(x);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            lo |= (uint32_t)clamp255(x[k] + 128) << (8 * k);
            hi |= (uint32_t)clamp255(x[k + 4] + 128) << (8 * k);
        }
        uint8_t* dst = A.plane[c] + (size_t)(by * 8 + r) * A.pitch[c] + bx * 8;
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
    }
}

void launch_jpeg_idct(hipStream_t s, const JpegIdctArgs& A)
{
    const int nblk = A.first[3];
    if (nblk <= 0) return;
    hipLaunchKernelGGL(k_jpeg_idct, dim3((nblk + 31) / 32), dim3(256), 0, s, A);
}

// ------------------------------------------------------------------------------------------------
// Upsampling + colour + crop (+ gray).  The pixels are jpeg_rgb.h's (chroma modes, edge rules and the colour matrix are
// stated there, and the fused crop-and-forward kernel of k_jpeg_fwd.hip runs the same functions): a lane makes 4 neighbouring
// output pixels from 4 luma samples and at most 4 neighbouring chroma samples per row, each group ONE dword load.
// ------------------------------------------------------------------------------------------------
using rgbpx::chroma4;
using rgbpx::load4;
typedef rgbpx::u32_a1 u32_a1;

// gray: one dword stored per lane (256 B per wave and row); rgb: 12 bytes
template <int mode, bool rgb>
__global__ __launch_bounds__(256) void k_jpeg_out(JpegOutArgs A)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (4 * q >= A.ow || y >= A.oh) return;
    const int X0 = 4 * q + A.left, Y = y + A.top;
    const int nx = min(4, A.ow - 4 * q);
    int lum[4], cb[4], cr[4];
    load4(A.plane[0] + (size_t)Y * A.pitch[0], X0, A.W, lum);
    chroma4<mode>(A.plane[1], A.pitch[1], A.cw, A.ch, X0, Y, cb);
    chroma4<mode>(A.plane[2], A.pitch[2], A.cw, A.ch, X0, Y, cr);
    const int half = 1 << (A.shift - 1);
    uint32_t px[4];   // gray: px[0] holds the 4 pixels; rgb: R | G << 8 | B << 16 each
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const rgbpx::Rgb c = rgbpx::colour(lum[i], cb[i], cr[i]);
        const int R = c.r, G = c.g, B = c.b;
        // gray: channel 0 (R) takes the "B" weight, as k_bgr2gray gives it to the first byte of PIL's RGB pixels
        if (rgb) px[i] = (uint32_t)R | (uint32_t)G << 8 | (uint32_t)B << 16;
        else px[i] = (uint32_t)((R * A.k0 + G * A.k1 + B * A.k2 + half) >> A.shift);
    }
    uint8_t* d = A.dst + (size_t)y * A.dst_pitch;
    if (rgb) {
        if (nx == 4) {
            u32_a1* o = reinterpret_cast<u32_a1*>(d + 12 * q);   // a row of 3 * width bytes starts anywhere
            o[0] = px[0] | px[1] << 24;
            o[1] = px[1] >> 8 | px[2] << 16;
            o[2] = px[2] >> 16 | px[3] << 8;
        } else {
            for (int i = 0; i < nx; i++) {
                d[12 * q + 3 * i] = (uint8_t)px[i];
                d[12 * q + 3 * i + 1] = (uint8_t)(px[i] >> 8);
                d[12 * q + 3 * i + 2] = (uint8_t)(px[i] >> 16);
            }
        }
    } else {
        if (nx == 4) *reinterpret_cast<uint32_t*>(d + 4 * q) = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;   // level rows are 64-B aligned
        else
            for (int i = 0; i < nx; i++) d[4 * q + i] = (uint8_t)px[i];
    }
}

template <bool rgb>
static void launch_out(hipStream_t s, const JpegOutArgs& A)
{
    dim3 block(256);
    dim3 grid(((A.ow + 3) / 4 + 255) / 256, A.oh);
    switch (A.mode) {
    case 0: hipLaunchKernelGGL((k_jpeg_out<0, rgb>), grid, block, 0, s, A); break;
    case 1: hipLaunchKernelGGL((k_jpeg_out<1, rgb>), grid, block, 0, s, A); break;
    case 2: hipLaunchKernelGGL((k_jpeg_out<2, rgb>), grid, block, 0, s, A); break;
    case 3: hipLaunchKernelGGL((k_jpeg_out<3, rgb>), grid, block, 0, s, A); break;
    default: hipLaunchKernelGGL((k_jpeg_out<4, rgb>), grid, block, 0, s, A); break;
    }
}

void launch_jpeg_gray(hipStream_t s, JpegOutArgs A, int variant)
{
    if (variant == ICELK_GRAY_CV4) { A.k0 = 3735; A.k1 = 19235; A.k2 = 9798; A.shift = 15; }
    else { A.k0 = 1868; A.k1 = 9617; A.k2 = 4899; A.shift = 14; }
    launch_out<false>(s, A);
}

void launch_jpeg_rgb(hipStream_t s, JpegOutArgs A)
{
    A.shift = 1;
    launch_out<true>(s, A);
}

}  // namespace icelk
