// jpeg_resave_host.h -- the host statement of the re-save's forward half: jpeg_fwd.h (the code the device kernel runs)
// called pixel by pixel and block by block on the CPU, plus the tables and the descriptor of the file Pillow would
// write.  Plain C++ without the HIP runtime: abi_jpeg_resave.hip exports it (icelk_jpeg_resave_tables,
// icelk_jpeg_resave_coefficients_host), and a stand-alone program can include it as it is.  No global state that is
// written: re-entrant.
#pragma once
#include <string.h>

#include <vector>

#include "../../include/icelk.h"
#include "jpeg_fwd.h"

namespace icelk {
namespace resave {

// ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), natural order
static const uint8_t kAnnexK[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// libjpeg's quality scaling, entries kept in 1 .. 255 (a baseline file)
inline void quality_tables(int quality, uint16_t* luma, uint16_t* chroma)
{
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; t++)
        for (int i = 0; i < 64; i++) {
            const int v = (kAnnexK[t][i] * scale + 50) / 100;
            (t ? chroma : luma)[i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
}

inline bool size_ok(int w, int h, int quality) { return quality >= 1 && quality <= 100 && w >= 1 && h >= 1 && w <= 65535 && h <= 65535; }

// what icelk_jpeg_describe says about the file Pillow would write: 4:2:0, no restart markers
inline void resave_info(int w, int h, int quality, icelk_jpeg_info_t* I)
{
    memset(I, 0, sizeof(*I));
    I->width = w;
    I->height = h;
    I->ncomp = 3;
    I->hmax = I->vmax = 2;
    I->mcus_x = (w + 15) / 16;
    I->mcus_y = (h + 15) / 16;
    uint64_t off = 0;
    for (int k = 0; k < 3; k++) {
        I->comp_w[k] = k ? (w + 1) / 2 : w;
        I->comp_h[k] = k ? (h + 1) / 2 : h;
        I->blocks_x[k] = I->mcus_x * (k ? 1 : 2);
        I->blocks_y[k] = I->mcus_y * (k ? 1 : 2);
        I->coef_offset[k] = off;
        off += (uint64_t)I->blocks_x[k] * I->blocks_y[k] * 64;
    }
    I->coef_count = off;
    quality_tables(quality, I->quant[0], I->quant[1]);
    memcpy(I->quant[2], I->quant[1], sizeof(I->quant[2]));
}

// one 8x8 block of a padded sample plane -> quantised coefficients, natural order
inline void block_host(const uint8_t* s, size_t pitch, const uint16_t* q, int16_t* out)
{
    int t[8][8];
    for (int r = 0; r < 8; r++) {
        int x[8];
        for (int k = 0; k < 8; k++) x[k] = (int)s[r * pitch + k] - 128;
        fwd::fdct8<true>(x);
        for (int k = 0; k < 8; k++) t[r][k] = x[k];
    }
    for (int col = 0; col < 8; col++) {
        int x[8];
        for (int k = 0; k < 8; k++) x[k] = t[k][col];
        fwd::fdct8<false>(x);
        for (int k = 0; k < 8; k++) out[k * 8 + col] = (int16_t)fwd::quantise(x[k], q[k * 8 + col], fwd::reciprocal((uint32_t)q[k * 8 + col] << 3));
    }
}

struct Pixel {
    int r, g, b;
};

// The coefficients of the file Pillow would write for a w x h image, and its descriptor.  px(y, x): the 8-bit R G B of image
// pixel (x, y), 0 <= x < w and 0 <= y < h -- interleaved bytes (coefficients_host below) or the crop box of a decoded file's
// planes (jpeg_crop_fwd_host.h); the padding of jpeg_fwd.h is a clamped coordinate here, as in the kernels.
template <typename Px>
inline int coefficients_from(Px px_of, int w, int h, int quality, icelk_jpeg_info_t* info, int16_t* coef, uint64_t capacity)
{
    if (!info || !size_ok(w, h, quality)) return ICELK_EARG;
    resave_info(w, h, quality, info);
    if (!coef) return ICELK_OK;   // the descriptor only
    if (capacity < info->coef_count) return ICELK_ECAP;
    const icelk_jpeg_info_t& I = *info;
    // the padded sample planes: luma over its real blocks, chroma over its whole grid
    const int rbx = (w + 7) / 8, rby = (h + 7) / 8;
    const size_t lp = (size_t)rbx * 8, cp = (size_t)I.mcus_x * 8;
    std::vector<uint8_t> Y, Cb, Cr;
    try {
        Y.resize(lp * rby * 8);
        Cb.resize(cp * I.mcus_y * 8);
        Cr.resize(cp * I.mcus_y * 8);
    } catch (...) {
        return ICELK_ENOMEM;
    }
    auto px = [&](int y, int x) { return px_of(y, x < w ? x : w - 1); };
    for (int qy = 0; qy < I.mcus_y * 8; qy++) {
        const fwd::QuadRows R = fwd::quad_rows(qy, h);
        for (int qx = 0; qx < I.mcus_x * 8; qx++) {
            for (int k = 0; k < 4; k++) {
                const int ly = 2 * qy + (k >> 1), lx = 2 * qx + (k & 1);
                if (ly >= rby * 8 || lx >= rbx * 8) continue;
                const Pixel p = px((k >> 1) ? R.y1 : R.y0, lx);
                Y[ly * lp + lx] = (uint8_t)fwd::luma(p.r, p.g, p.b);
            }
            const Pixel a = px(R.c0, 2 * qx), b = px(R.c0, 2 * qx + 1), d = px(R.c1, 2 * qx), e = px(R.c1, 2 * qx + 1);
            Cb[qy * cp + qx] = (uint8_t)fwd::downsample(fwd::chroma_b(a.r, a.g, a.b), fwd::chroma_b(b.r, b.g, b.b),
                                                        fwd::chroma_b(d.r, d.g, d.b), fwd::chroma_b(e.r, e.g, e.b), qx);
            Cr[qy * cp + qx] = (uint8_t)fwd::downsample(fwd::chroma_r(a.r, a.g, a.b), fwd::chroma_r(b.r, b.g, b.b),
                                                        fwd::chroma_r(d.r, d.g, d.b), fwd::chroma_r(e.r, e.g, e.b), qx);
        }
    }
    int16_t* L = coef + I.coef_offset[0];
    const size_t lbx = (size_t)I.blocks_x[0];
    for (int by = 0; by < rby; by++)
        for (int bx = 0; bx < rbx; bx++) block_host(Y.data() + (size_t)by * 8 * lp + bx * 8, lp, I.quant[0], L + (by * lbx + bx) * 64);
    for (int k = 1; k < 3; k++) {
        const std::vector<uint8_t>& P = k == 1 ? Cb : Cr;
        for (int by = 0; by < I.mcus_y; by++)
            for (int bx = 0; bx < I.mcus_x; bx++)
                block_host(P.data() + (size_t)by * 8 * cp + bx * 8, cp, I.quant[k], coef + I.coef_offset[k] + ((size_t)by * I.mcus_x + bx) * 64);
    }
    // dummy luma blocks, MCU by MCU in the encoder's block order (a source may be a dummy written just before)
    for (int my = 0; my < I.mcus_y; my++)
        for (int mx = 0; mx < I.mcus_x; mx++)
            for (int v = 0; v < 2; v++)
                for (int u = 0; u < 2; u++) {
                    const int bx = 2 * mx + u, by = 2 * my + v;
                    if (bx < rbx && by < rby) continue;
                    const int from = fwd::dummy_source(v, 2 * mx + 1 < rbx, by < rby);
                    int16_t* dst = L + (by * lbx + bx) * 64;
                    memset(dst, 0, 64 * sizeof(int16_t));
                    dst[0] = L[((2 * my + (from >> 1)) * lbx + 2 * mx + (from & 1)) * 64];
                }
    return ICELK_OK;
}

// the coefficients of the file Pillow would write for the w x h image at rgb, and its descriptor: icelk.h says the rest
inline int coefficients_host(const uint8_t* rgb, int w, int h, int stride, int quality, icelk_jpeg_info_t* info, int16_t* coef,
                             uint64_t capacity)
{
    if (!rgb || stride < 3 * w) return ICELK_EARG;
    return coefficients_from(
        [&](int y, int x) {
            const uint8_t* p = rgb + (size_t)y * stride + 3 * (size_t)x;
            return Pixel{p[0], p[1], p[2]};
        },
        w, h, quality, info, coef, capacity);
}

}  // namespace resave
}  // namespace icelk
