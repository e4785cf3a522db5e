// k_jpeg_fwd.hip -- the forward half of the re-save for gfx950: interleaved R G B pixels -> the quantised DCT coefficients
// of the 4:2:0 baseline file Pillow's `img.save` would write, in the layout of icelk_jpeg_info_t.  From there k_jpeg_idct
// and k_jpeg_out (k_jpeg.hip) decode them as they decode a file's.  The arithmetic is jpeg_fwd.h, shared with the host
// statement (abi_jpeg_resave.hip); nothing here rounds on its own.
//
// One workgroup of 256 threads makes a strip of 16 MCUs: 256 x 16 pixels, 64 luma and 2 x 16 chroma blocks.
//   phase 1  a thread takes 2x2 pixel quads (4 of them, 2 quad rows apart): colour conversion, 4 luma samples and the
//            downsampled Cb / Cr sample into LDS, with the edge rules of jpeg_fwd.h (fwd::quad_rows) -- padding is a
//            clamped coordinate, never a stored copy
//   phase 2  three passes over 32 blocks (luma block row 0, luma block row 1, Cb + Cr), 8 lanes per block as in
//            k_jpeg_idct: lane r transforms row r, the block's tile (rows padded to 9 dwords) turns it, the lane
//            transforms and quantises column r, the tile turns it back, and the lane stores row r of the coefficients
//            as one 16-byte store (a block is 128 contiguous bytes, a wave writes 1 KiB).  The DC of every luma block
//            stays in LDS
//   tail     the dummy luma blocks of the strip (a block column or row of the MCU grid that holds no sample): AC 0, DC
//            from the block fwd::dummy_source names, which lies in the same MCU, so in this workgroup's LDS
// Reads 3 bytes and writes 3 bytes (1.5 int16) per pixel; no scratch.
//
// k_jpeg_crop_fwd is the same kernel with another phase 1: it takes the crop box of a decoded file's component PLANES
// (what k_jpeg_idct left) instead of R G B bytes, so the cropped image never goes through HBM.  Output pixel (x, y) of the
// crop is image pixel (x + left, y + top), made by jpeg_rgb.h exactly as k_jpeg_out makes it -- upsampling with neighbours
// clamped at the TRUE plane edges, the 16-bit colour matrix, clamped to 8 bits, which is the rounding Pillow puts between
// its decoder and its encoder -- and from there on phase 1 is the one above (fwd_quad), fwd::quad_rows and the right-edge
// clamp taken in CROP coordinates; only the walk differs: a thread takes two neighbouring quads at a time, so that the four
// samples of a dword load serve four pixels.  Phase 2 and the tail are shared code (fwd_blocks).  No scratch.
// What it touches.  Every plane read goes through rgbpx::crop_row4 (jpeg_rgb.h, which states the read set exactly): luma
// rows top .. top + h - 1 at four neighbouring columns from inside left .. left + w - 1 -- at the crop's right edge the
// crop's last four, which for a 3-wide crop reach one column past it -- clamped to the true width W; chroma at the four
// samples of the window chroma4 names for those columns, one sample wider than the crop's own on each subsampled side, in
// mode 2 in a near and a far row, every index clamped into the cw x ch true samples.  load4 never leaves a row's true
// samples, so all of it lies inside the planes as jpeg_plane_args sizes them.  Samples beyond what the crop's pixels need
// may lie in blocks the source's inverse DCT did not transform (it transforms the box's blocks and the filter's
// neighbours): they hold whatever the buffer held, are computed with, and are never picked.  Stores are blocks of the
// re-saved file's layout only, walked by the grid, not by the data.  So the kernel is safe on whatever a decode that did
// not settle left in the planes (abi_jpeg_job.hip): it turns garbage samples into bounded coefficients.
#include "icelk_internal.h"
#include "jpeg_fwd.h"
#include "jpeg_rgb.h"

namespace icelk {

namespace {

constexpr int kStripMcus = 16;
constexpr int kLumaPitch = 16 * kStripMcus + 4;    // bytes per LDS row of luma: 65 dwords
constexpr int kChromaPitch = 8 * kStripMcus + 4;   // 33 dwords

typedef uint32_t fwd_u32_a1 __attribute__((aligned(1)));
typedef uint16_t fwd_u16_a1 __attribute__((aligned(1)));

struct Pixels2 {
    int r[2], g[2], b[2];
};

// the pixels at columns 2 qx and 2 qx + 1 of a row, the column clamped to the image: 6 neighbouring bytes at whatever
// address 3 * width puts them (gfx950 under HSA takes unaligned vector loads), or byte by byte at the right edge
__device__ __forceinline__ Pixels2 load_pair(const uint8_t* __restrict__ row, int qx, int w)
{
    Pixels2 p;
    if (2 * qx + 1 < w) {
        const uint32_t lo = *reinterpret_cast<const fwd_u32_a1*>(row + 6 * qx);
        const uint32_t hi = *reinterpret_cast<const fwd_u16_a1*>(row + 6 * qx + 4);
        p.r[0] = lo & 255;
        p.g[0] = (lo >> 8) & 255;
        p.b[0] = (lo >> 16) & 255;
        p.r[1] = lo >> 24;
        p.g[1] = hi & 255;
        p.b[1] = hi >> 8;
    } else {
        const uint8_t* q = row + 3 * (w - 1);
        p.r[0] = p.r[1] = q[0];
        p.g[0] = p.g[1] = q[1];
        p.b[0] = p.b[1] = q[2];
    }
    return p;
}

}  // namespace

// the workgroup's LDS: the strip's samples, the blocks' tiles, the tables, the DC of the strip's luma blocks
struct FwdLds {
    __attribute__((aligned(16))) uint8_t lum[16][kLumaPitch];   // read a dword at a time
    __attribute__((aligned(16))) uint8_t chr[2][8][kChromaPitch];
    int tile[32][8][9];
    uint16_t quant[2][64];
    uint32_t recip[2][64];
    int16_t dc[2][2 * kStripMcus];
};

__device__ __forceinline__ void fwd_tables(const JpegFwdArgs& A, FwdLds& S)
{
    const int t = threadIdx.x;
    if (t < 128) {
        S.quant[t >> 6][t & 63] = A.quant[t >> 6][t & 63];
        S.recip[t >> 6][t & 63] = A.recip[t >> 6][t & 63];
    }
}

// one 2x2 quad of the padded grid: rows a / b are its luma rows, ca / cb the rows its chroma sample is made of
__device__ __forceinline__ void fwd_quad(FwdLds& S, int qr, int qc, int qx, const Pixels2& a, const Pixels2& b, const Pixels2& ca,
                                         const Pixels2& cb)
{
    const uint32_t y0 = (uint32_t)fwd::luma(a.r[0], a.g[0], a.b[0]) | (uint32_t)fwd::luma(a.r[1], a.g[1], a.b[1]) << 8;
    const uint32_t y1 = (uint32_t)fwd::luma(b.r[0], b.g[0], b.b[0]) | (uint32_t)fwd::luma(b.r[1], b.g[1], b.b[1]) << 8;
    *reinterpret_cast<uint16_t*>(&S.lum[2 * qr][2 * qc]) = (uint16_t)y0;
    *reinterpret_cast<uint16_t*>(&S.lum[2 * qr + 1][2 * qc]) = (uint16_t)y1;
    S.chr[0][qr][qc] = (uint8_t)fwd::downsample(fwd::chroma_b(ca.r[0], ca.g[0], ca.b[0]), fwd::chroma_b(ca.r[1], ca.g[1], ca.b[1]),
                                                fwd::chroma_b(cb.r[0], cb.g[0], cb.b[0]), fwd::chroma_b(cb.r[1], cb.g[1], cb.b[1]), qx);
    S.chr[1][qr][qc] = (uint8_t)fwd::downsample(fwd::chroma_r(ca.r[0], ca.g[0], ca.b[0]), fwd::chroma_r(ca.r[1], ca.g[1], ca.b[1]),
                                                fwd::chroma_r(cb.r[0], cb.g[0], cb.b[0]), fwd::chroma_r(cb.r[1], cb.g[1], cb.b[1]), qx);
}

// phase 1 over the strip: `pair(row, qx)` gives the pixels at columns 2 qx and 2 qx + 1 of image row `row`, the column clamped
template <typename Pair>
__device__ __forceinline__ void fwd_samples(FwdLds& S, int mcu0, int my, int nmcu, int h, Pair pair)
{
    const int t = threadIdx.x;
    const int qc = t & 127, qx = mcu0 * 8 + qc;
    if (qc < 8 * nmcu) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int qr = (t >> 7) + 2 * k;
            const fwd::QuadRows R = fwd::quad_rows(my * 8 + qr, h);
            const Pixels2 a = pair(R.y0, qx);
            const Pixels2 b = pair(R.y1, qx);
            Pixels2 ca = a, cb = b;
            if (R.c0 != R.y0 || R.c1 != R.y1) {   // a chroma row below the last one: the rows of that one
                ca = pair(R.c0, qx);
                cb = pair(R.c1, qx);
            }
            fwd_quad(S, qr, qc, qx, a, b, ca, cb);
        }
    }
}

// phase 2 and the tail
__device__ __forceinline__ void fwd_blocks(const JpegFwdArgs& A, FwdLds& S, int mcu0, int my, int nmcu)
{
    auto& lum = S.lum;
    auto& chr = S.chr;
    auto& tile = S.tile;
    auto& quant = S.quant;
    auto& recip = S.recip;
    auto& dc = S.dc;
    const int t = threadIdx.x;
    // ---- phase 2
    const int g = t >> 3, r = t & 7;
#pragma unroll 1
    for (int pass = 0; pass < 3; pass++) {
        // pass 0 / 1: luma block row `pass`, block column g; pass 2: Cb blocks 0 .. 15, Cr blocks 0 .. 15
        const int comp = pass < 2 ? 0 : 1 + (g >> 4);
        const int lbx = pass < 2 ? g : (g & 15);           // block column inside the strip
        const int bx = (pass < 2 ? 2 * mcu0 : mcu0) + lbx;
        const int by = pass < 2 ? 2 * my + pass : my;
        bool live = lbx < (pass < 2 ? 2 * nmcu : nmcu);
        if (pass < 2) live = live && bx < A.real_bx && by < A.real_by;   // dummies: the tail
        const int tab = comp ? 1 : 0;
        int x[8];
        if (live) {
            const uint8_t* src = pass < 2 ? &lum[8 * pass + r][8 * lbx] : &chr[comp - 1][r][8 * lbx];
            const uint32_t lo = *reinterpret_cast<const uint32_t*>(src), hi = *reinterpret_cast<const uint32_t*>(src + 4);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                x[k] = (int)((lo >> (8 * k)) & 255) - 128;
                x[k + 4] = (int)((hi >> (8 * k)) & 255) - 128;
            }
            fwd::fdct8<true>(x);
#pragma unroll
            for (int k = 0; k < 8; k++) tile[g][r][k] = x[k];
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int k = 0; k < 8; k++) x[k] = tile[g][k][r];
            fwd::fdct8<false>(x);
#pragma unroll
            for (int k = 0; k < 8; k++) x[k] = fwd::quantise(x[k], quant[tab][k * 8 + r], recip[tab][k * 8 + r]);
            if (pass < 2 && r == 0) dc[pass][lbx] = (int16_t)x[0];
        }
        __syncthreads();   // every lane has read its column
        if (live) {
#pragma unroll
            for (int k = 0; k < 8; k++) tile[g][k][r] = x[k];
        }
        __syncthreads();
        if (live) {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = ((uint32_t)tile[g][r][2 * k] & 0xffffu) | (uint32_t)tile[g][r][2 * k + 1] << 16;
            const int blocks_x = comp ? A.mcus_x : 2 * A.mcus_x;
            int16_t* base = comp == 0 ? A.coef[0] : (comp == 1 ? A.coef[1] : A.coef[2]);   // no lane-indexed kernel argument
            int16_t* dst = base + ((size_t)by * blocks_x + bx) * 64 + r * 8;
            *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        __syncthreads();   // the next pass writes the tile again
    }

    // ---- tail: the strip's dummy luma blocks (dc[][] is complete: the loop's last barrier)
    const bool col_tail = 2 * (mcu0 + nmcu) > A.real_bx, row_tail = 2 * my + 1 >= A.real_by;
    if (col_tail || row_tail) {
        // at most the bottom block row and, of the top one, the last block column: 8 lanes each
        for (int s = g; s < 2 * 2 * nmcu; s += 32) {
            const int v = s / (2 * nmcu), lbx = s % (2 * nmcu);
            const int bx = 2 * mcu0 + lbx, by = 2 * my + v;
            const bool col_real = bx < A.real_bx, row_real = by < A.real_by;
            if (col_real && row_real) continue;
            const bool col1_real = (bx | 1) < A.real_bx;
            const int from = fwd::dummy_source(v, col1_real, row_real);
            const int16_t d = dc[from >> 1][(lbx & ~1) | (from & 1)];
            int16_t* dst = A.coef[0] + ((size_t)by * 2 * A.mcus_x + bx) * 64 + r * 8;
            *reinterpret_cast<uint4*>(dst) = make_uint4(r == 0 ? (uint32_t)(uint16_t)d : 0u, 0u, 0u, 0u);
        }
    }
}


__global__ __launch_bounds__(256) void k_jpeg_fwd(JpegFwdArgs A)
{
    __shared__ FwdLds S;
    fwd_tables(A, S);
    const int mcu0 = blockIdx.x * kStripMcus, my = blockIdx.y;
    const int nmcu = min(kStripMcus, A.mcus_x - mcu0);   // MCUs of this strip: >= 1 by the launch's grid
    fwd_samples(S, mcu0, my, nmcu, A.h, [&](int row, int qx) { return load_pair(A.rgb + (size_t)row * A.pitch, qx, A.w); });
    __syncthreads();
    fwd_blocks(A, S, mcu0, my, nmcu);
}

using rgbpx::crop_row4;

__device__ __forceinline__ Pixels2 pixels2(const rgbpx::Rgb (&px)[4], int j)
{
    Pixels2 p;
    p.r[0] = px[2 * j].r, p.g[0] = px[2 * j].g, p.b[0] = px[2 * j].b;
    p.r[1] = px[2 * j + 1].r, p.g[1] = px[2 * j + 1].g, p.b[1] = px[2 * j + 1].b;
    return p;
}

// F.rgb / F.pitch are not read; F.w x F.h is the crop, whose pixel (0, 0) is image pixel (left, top) of P.
// Phase 1 here: a thread takes two neighbouring quads (4 x 2 pixels, 2 of them, 4 quad rows apart), so that every group of 4
// samples jpeg_rgb.h loads with one dword serves 4 pixels, as in k_jpeg_out: 1.25 loads per pixel at 4:2:0.
template <int mode>
__global__ __launch_bounds__(256) void k_jpeg_crop_fwd(rgbpx::Planes P, int left, int top, JpegFwdArgs A)
{
    __shared__ FwdLds S;
    fwd_tables(A, S);
    const int mcu0 = blockIdx.x * kStripMcus, my = blockIdx.y;
    const int nmcu = min(kStripMcus, A.mcus_x - mcu0);
    {
        const int t = threadIdx.x;
        const int qc = 2 * (t & 63), qx = mcu0 * 8 + qc;   // the first of the two quad columns
        if (qc < 8 * nmcu) {
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int qr = (t >> 6) + 4 * k;
                const fwd::QuadRows R = fwd::quad_rows(my * 8 + qr, A.h);
                rgbpx::Rgb a[4], b[4], ca[4], cb[4];
                crop_row4<mode>(P, left, top, A.w, 2 * qx, R.y0, a);
                crop_row4<mode>(P, left, top, A.w, 2 * qx, R.y1, b);
                if (R.c0 != R.y0 || R.c1 != R.y1) {   // a chroma row below the last one: the rows of that one
                    crop_row4<mode>(P, left, top, A.w, 2 * qx, R.c0, ca);
                    crop_row4<mode>(P, left, top, A.w, 2 * qx, R.c1, cb);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) ca[j] = a[j], cb[j] = b[j];
                }
#pragma unroll
                for (int j = 0; j < 2; j++) fwd_quad(S, qr, qc + j, qx + j, pixels2(a, j), pixels2(b, j), pixels2(ca, j), pixels2(cb, j));
            }
        }
    }
    __syncthreads();
    fwd_blocks(A, S, mcu0, my, nmcu);
}

void launch_jpeg_fwd(hipStream_t s, const JpegFwdArgs& A)
{
    if (A.mcus_x <= 0 || A.mcus_y <= 0) return;
    hipLaunchKernelGGL(k_jpeg_fwd, dim3((A.mcus_x + kStripMcus - 1) / kStripMcus, A.mcus_y), dim3(256), 0, s, A);
}

void launch_jpeg_crop_fwd(hipStream_t s, const JpegOutArgs& O, const JpegFwdArgs& A)
{
    if (A.mcus_x <= 0 || A.mcus_y <= 0) return;
    rgbpx::Planes P;
    for (int k = 0; k < 3; k++) P.plane[k] = O.plane[k], P.pitch[k] = O.pitch[k];
    P.W = O.W, P.cw = O.cw, P.ch = O.ch, P.mode = O.mode;
    const dim3 grid((A.mcus_x + kStripMcus - 1) / kStripMcus, A.mcus_y), block(256);
    switch (O.mode) {
    case 0: hipLaunchKernelGGL(k_jpeg_crop_fwd<0>, grid, block, 0, s, P, O.left, O.top, A); break;
    case 1: hipLaunchKernelGGL(k_jpeg_crop_fwd<1>, grid, block, 0, s, P, O.left, O.top, A); break;
    case 2: hipLaunchKernelGGL(k_jpeg_crop_fwd<2>, grid, block, 0, s, P, O.left, O.top, A); break;
    case 3: hipLaunchKernelGGL(k_jpeg_crop_fwd<3>, grid, block, 0, s, P, O.left, O.top, A); break;
    default: hipLaunchKernelGGL(k_jpeg_crop_fwd<4>, grid, block, 0, s, P, O.left, O.top, A); break;
    }
}

}  // namespace icelk
