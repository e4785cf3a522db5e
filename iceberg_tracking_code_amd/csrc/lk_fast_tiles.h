// lk_fast_tiles.h -- building blocks shared by the window-size-specialised Lucas-Kanade kernels
// (k_lk_fast.hip: one feature per wave; k_lk_multi.hip: several features per wave): compile-time window
// geometry, staging of image tiles in LDS as aligned dwords, byte -> 16-bit-pair widening for v_dot2_i32_i16.
#pragma once
#include <type_traits>

#include "lk_common.h"

namespace icelk {
namespace lkf {

using namespace lk;

// Search-tile margin R: the estimate may move +-R px from where the tile was staged before it is staged again.  Results
// do not depend on it.  Measured (C2 / REF / C5 pairs/s): R = 6: 5 040 / 611 / 470; 3: 5 300 / 640 / 530; 2: 5 280 / 652 /
// 547; 1: 5 360 / 654 / 552; 0: 5 240 / 645 / 534.  A level's first guess comes from the level above and lands within a
// pixel of the answer, so a wide tile is loaded (and its addresses computed, and its registers held) for nothing; with
// R = 1 the 21x21 search tile is 24x24 B = 3 rounds of loads instead of 6 (34x34).
constexpr int kMargin = kLkTileMargin;

constexpr int pick_seg(int ww, int wh)
{
    int best = 8, best_cost = 1 << 30;
    for (int s = 5; s <= 8; s++) {
        const int nseg = (ww + s - 1) / s;
        const int tpl = (nseg * wh + 63) / 64;
        const int cost = tpl * (s + 3);
        if (cost < best_cost) { best_cost = cost; best = s; }
    }
    return best;
}

template <int WW, int WH>
struct Cfg {
    static constexpr int S = pick_seg(WW, WH);       // pixels per row segment
    static constexpr int NSEG = (WW + S - 1) / S;    // segments per window row
    static constexpr int NTASK = NSEG * WH;
    static constexpr int TPL = (NTASK + 63) / 64;    // segments per lane
    static constexpr int ITW = WW + 3, ITH = WH + 3;  // template source patch (1-px ring for Scharr + bilinear)
    static constexpr int IPD = (ITW + 2) / 4 + 1;     // LDS row pitch in dwords (any 4-byte phase)
    static constexpr int JTW = WW + 1 + 2 * kMargin, JTH = WH + 1 + 2 * kMargin;
    static constexpr int JPD = (JTW + 2) / 4 + 1;
    static constexpr int I_DW = IPD * ITH, J_DW = JPD * JTH;
    static constexpr int LDS_DW = I_DW + J_DW + 8;    // +8: realignment reads may run 3 dwords past a row
};

// ---- tile staging ---------------------------------------------------------------------------------
// A tile whose top-left image pixel is (x0, y0) is kept in LDS as the aligned dwords that cover each of
// its rows: LDS byte (r*PD*4 + (x0 & 3) + tx) holds image pixel (x0 + tx, y0 + r).
template <int PD, int TH>
struct TileRegs {
    static constexpr int N = (PD * TH + 63) / 64;
    uint32_t v[N];
};

template <int PD, int TH>
__device__ __forceinline__ void tile_issue(TileRegs<PD, TH>& t, const Level& L, int x0, int y0, int lane)
{
    // uniform 64-bit base + per-lane 32-bit offset (r * pitch + 4c < 2^24): one 24-bit mad per load, and no
    // predication -- surplus lanes of the last round re-load the tile's last dword
    const uint8_t* base = L.ptr + (size_t)y0 * L.pitch + (x0 & ~3);
#pragma unroll
    for (int m = 0; m < TileRegs<PD, TH>::N; m++) {
        int i = lane + 64 * m;
        i = i < PD * TH ? i : PD * TH - 1;
        const int r = i / PD, c = i - r * PD;
        const unsigned off = (unsigned)__mul24(r, L.pitch) + 4u * (unsigned)c;
        t.v[m] = *reinterpret_cast<const uint32_t*>(base + off);
    }
}

template <int PD, int TH>
__device__ __forceinline__ void tile_commit(const TileRegs<PD, TH>& t, uint32_t* lds, int lane)
{
#pragma unroll
    for (int m = 0; m < TileRegs<PD, TH>::N; m++) {
        int i = lane + 64 * m;
        i = i < PD * TH ? i : PD * TH - 1;   // same value written twice: harmless
        lds[i] = t.v[m];
    }
}

// Tiles that reach over the image border (features within a window of the frame edge at this level): the same
// aligned dwords, fetched with reflection (BORDER_REFLECT_101).  Rows reflect as a whole; a dword whose four columns
// lie inside the row is one load as usual; the few dwords that straddle the left or right edge are put together
// from four reflected byte loads.  Two rounds of loads in flight per tile, whatever its size -- the byte-wise loop
// this replaces paid the memory latency TW*TH/64 times in a row and made the border features (9 % of them at
// 4000x3000, 21x21, 4 levels) the stragglers of every launch: 92 us against 50 us for an interior feature.
template <int PD, int TH>
__device__ __forceinline__ void tile_issue_reflect(TileRegs<PD, TH>& t, const Level& L, int x0, int y0, int lane)
{
    constexpr int N = TileRegs<PD, TH>::N;
    const int xa = x0 & ~3;
    const uint8_t* row[N];
    int gx[N];
    bool edge[N];
#pragma unroll
    for (int m = 0; m < N; m++) {
        int i = lane + 64 * m;
        i = i < PD * TH ? i : PD * TH - 1;
        const int r = i / PD, c = i - r * PD;
        row[m] = L.ptr + (size_t)reflect101(y0 + r, L.h) * L.pitch;
        gx[m] = xa + 4 * c;
        edge[m] = !(L.w >= 4 && (unsigned)gx[m] <= (unsigned)(L.w - 4));
        t.v[m] = edge[m] ? 0u : *reinterpret_cast<const uint32_t*>(row[m] + gx[m]);
    }
    bool any = false;
#pragma unroll
    for (int m = 0; m < N; m++) any |= edge[m];
    if (__builtin_amdgcn_ballot_w64(any) == 0) return;
    uint8_t q[N][4];
#pragma unroll
    for (int m = 0; m < N; m++)
#pragma unroll
        for (int k = 0; k < 4; k++) q[m][k] = edge[m] ? row[m][reflect101(gx[m] + k, L.w)] : (uint8_t)0;
#pragma unroll
    for (int m = 0; m < N; m++)
        if (edge[m]) t.v[m] = (uint32_t)q[m][0] | ((uint32_t)q[m][1] << 8) | ((uint32_t)q[m][2] << 16) | ((uint32_t)q[m][3] << 24);
}

template <int PD, int TW, int TH>
__device__ __forceinline__ void tile_border(uint32_t* lds, const Level& L, int x0, int y0, int lane)
{
    TileRegs<PD, TH> t;
    tile_issue_reflect(t, L, x0, y0, lane);
    tile_commit(t, lds, lane);
}

__device__ __forceinline__ bool tile_inside(const Level& L, int x0, int y0, int tw, int th)
{
    // 0 <= x0 <= w - tw and 0 <= y0 <= h - th, as two unsigned compares (a level smaller than the tile fails)
    return L.w >= tw && L.h >= th && (unsigned)x0 <= (unsigned)(L.w - tw) && (unsigned)y0 <= (unsigned)(L.h - th);
}

// OpenCV's bounds test of a window origin: !(x < -W || x >= cols || y < -H || y >= rows)
template <int WW, int WH>
__device__ __forceinline__ bool origin_ok(const Level& L, int x, int y)
{
    return (unsigned)(x + WW) < (unsigned)(L.w + WW) && (unsigned)(y + WH) < (unsigned)(L.h + WH);
}

// the staged search tile (origin jx0, jy0, margin R on every side) still covers a window at (x, y); an origin of kUnstaged
// (no tile staged) covers none
constexpr int kUnstaged = -(1 << 29);
__device__ __forceinline__ bool tile_covers(int jx0, int jy0, int x, int y)
{
    return (unsigned)(x - jx0) <= 2u * kMargin && (unsigned)(y - jy0) <= 2u * kMargin;
}

typedef short v2s __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2s as_v2s(uint32_t x) { return __builtin_bit_cast(v2s, x); }
__device__ __forceinline__ uint32_t as_u32(v2s x) { return __builtin_bit_cast(uint32_t, x); }

// NX stream-aligned dwords (bytes 0 .. 4*NX-1) starting at byte offset `off` of an LDS row
template <int NX>
__device__ __forceinline__ void row_dwords(const uint32_t* row, int off, uint32_t (&X)[NX])
{
    const uint32_t* p = row + (off >> 2);
    const int sh = off & 3;
    uint32_t d[NX + 1];
#pragma unroll
    for (int i = 0; i <= NX; i++) d[i] = p[i];
#pragma unroll
    for (int i = 0; i < NX; i++) X[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
}

// bytes (M, M+1) of the stream widened to a pair of 16-bit lanes: (byte M) | (byte M+1) << 16
template <int M, int NX>
__device__ __forceinline__ v2s byte_pair(const uint32_t (&X)[NX])
{
    constexpr int i = M / 4, r = M % 4;
    static_assert(i < NX && (r < 3 || i + 1 < NX), "pair outside the loaded dwords");
    if constexpr (r == 0) return as_v2s(__builtin_amdgcn_perm(0u, X[i], 0x0c010c00u));
    else if constexpr (r == 1) return as_v2s(__builtin_amdgcn_perm(0u, X[i], 0x0c020c01u));
    else if constexpr (r == 2) return as_v2s(__builtin_amdgcn_perm(0u, X[i], 0x0c030c02u));
    else return as_v2s(__builtin_amdgcn_perm(X[i + 1 < NX ? i + 1 : i], X[i], 0x0c040c03u));
}

// byte M of two streams as a pair of 16-bit lanes: (byte M of X0) | (byte M of X1) << 16 -- one column of two rows
template <int M, int NX>
__device__ __forceinline__ v2s col_pair(const uint32_t (&X0)[NX], const uint32_t (&X1)[NX])
{
    constexpr int i = M / 4, r = M % 4;
    static_assert(i < NX, "column outside the loaded dwords");
    return as_v2s(__builtin_amdgcn_perm(X1[i], X0[i], 0x0c000c00u | ((4u + r) << 16) | (uint32_t)r));
}

// (a.y, b.x): the pair one 16-bit lane further along
__device__ __forceinline__ v2s pair_shift(v2s a, v2s b)
{
    return as_v2s(__builtin_amdgcn_alignbit(as_u32(b), as_u32(a), 16));
}

__device__ __forceinline__ int dot2(v2s a, v2s b, int c) { return __builtin_amdgcn_sdot2(a, b, c, false); }

template <int N, int I = 0, typename F>
__device__ __forceinline__ void static_for(F&& f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

// packed weight pairs (w00 | w01 << 16), (w10 | w11 << 16) for v_dot2_i32_i16 against row pairs (template_pixels)
__device__ __forceinline__ uint32_t pack_weights_lo(const Weights& w) { return ((uint32_t)w.w00 & 0xffffu) | ((uint32_t)w.w01 << 16); }
__device__ __forceinline__ uint32_t pack_weights_hi(const Weights& w) { return ((uint32_t)w.w10 & 0xffffu) | ((uint32_t)w.w11 << 16); }
// the same weights by column, (w00 | w10 << 16), (w01 | w11 << 16), against column pairs (residual_pixels)
__device__ __forceinline__ uint32_t pack_weights_c0(const Weights& w) { return ((uint32_t)w.w00 & 0xffffu) | ((uint32_t)w.w10 << 16); }
__device__ __forceinline__ uint32_t pack_weights_c1(const Weights& w) { return ((uint32_t)w.w01 & 0xffffu) | ((uint32_t)w.w11 << 16); }

// bilinear_weights' four values, bit for bit, already packed: the x / y float work two to an instruction (v_pk_*_f32), and
// cvRound as one addition of 1.5 * 2^23: for 0 <= v < 2^22 the sum rounds v to the nearest integer, ties to even (the
// constant is even), and its low 22 bits are that integer.  BY_COLUMN: pack_weights_c0 / _c1, else pack_weights_lo / _hi.
template <bool BY_COLUMN>
__device__ __forceinline__ void packed_weights(float a, float b, uint32_t& p0, uint32_t& p1)
{
    typedef float f2 __attribute__((ext_vector_type(2)));
    constexpr float kMagic = 12582912.f;                       // 1.5 * 2^23, bit pattern 0x4b400000
    constexpr uint32_t kMagicBits = 0x4b400000u;
    const f2 f = {a, b};
    const f2 g = 1.f - f;                                      // (1 - a, 1 - b)
    const f2 fg = f * g.yx;                                    // (a * (1 - b), b * (1 - a))
    const f2 r = fg * (float)(1 << W_BITS) + kMagic;           // two roundings, as written: -ffp-contract=off
    const float r00 = (g.x * g.y) * (float)(1 << W_BITS) + kMagic;
    const uint32_t x00 = __float_as_uint(r00), x01 = __float_as_uint(r.x), x10 = __float_as_uint(r.y);
    const uint32_t x11 = 3u * kMagicBits + (1u << W_BITS) - x00 - x01 - x10;   // low 16 bits: w11 = 2^14 - w00 - w01 - w10
    if (BY_COLUMN) {
        p0 = __builtin_amdgcn_perm(x10, x00, 0x05040100u);
        p1 = __builtin_amdgcn_perm(x11, x01, 0x05040100u);
    } else {
        p0 = __builtin_amdgcn_perm(x01, x00, 0x05040100u);
        p1 = __builtin_amdgcn_perm(x11, x10, 0x05040100u);
    }
}

// ---- pixel work shared by the one-feature-per-wave and the several-features-per-wave kernels ---------------------------
// The template of a feature: I as a dot2 accumulator seed, Ix / Iy as packed 16-bit pairs of neighbouring pixels.
template <int WW, int WH, int F>
struct Template {
    using C = Cfg<WW, WH>;
    int Ineg[F][C::TPL][C::S];                       // 256 - (I << 9): dot2 accumulator seed of the residual
    uint32_t Ixp[F][C::TPL][(C::S + 1) / 2];         // (Ix[2q], Ix[2q+1]) as 16-bit pairs
    uint32_t Iyp[F][C::TPL][(C::S + 1) / 2];
};

__device__ __forceinline__ uint32_t pack16(int lo, int hi)
{
    return __builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, 0x05040100u);
}

// v_perm selector that packs the HIGH 16-bit halves of two dwords, perm(hi, lo, sel) = (lo >> 16) | (hi >> 16) << 16, and
// clears the halves of pixels a segment of `len` pixels does not have (selector byte 0x0c gives 0x00).  Pixel pair q of the
// segment: template_pixels takes the derivative samples' rounding shift, their packing and the window mask in this one
// instruction.
__device__ __forceinline__ uint32_t pair_sel(int q, int len)
{
    return (2 * q < len ? 0x0302u : 0x0c0cu) | (2 * q + 1 < len ? 0x07060000u : 0x0c0c0000u);
}

// v_dot2_i32_i16 in its three-address (VOP3P) form.  The compiler only ever selects the two-address v_dot2c, which
// overwrites its accumulator: with a seed that is needed again (the template value of the residual, a rounding
// constant) that costs a v_mov per dot product.  b and c may be scalars (weights, constants): at most one of them is.
__device__ __forceinline__ int dot2_vsv(v2s a, uint32_t b_scalar, int c)
{
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(as_u32(a)), "s"(b_scalar), "v"(c));
    return d;
}
__device__ __forceinline__ int dot2_vvs(v2s a, uint32_t b, int c_scalar)
{
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(as_u32(a)), "v"(b), "s"(c_scalar));
    return d;
}
// the first term of a sum: accumulator 0 as an inline constant, not a v_mov of a zero register in front of v_dot2c
__device__ __forceinline__ int dot2_vv0(v2s a, v2s b)
{
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(d) : "v"(as_u32(a)), "v"(as_u32(b)));
    return d;
}

// ---- pixel phase: template of ONE feature -------------------------------------------------------------------
// Everything that is the same for all lanes arrives as a scalar (readlane of the owning block's registers).
// psel: the lane's pair selectors (pair_sel of each segment's pixel pairs and its pixel count in the window).
// fsum != nullptr (the "lk_sums" variants, LKParams::sum_mode): every window pixel's three products also go to LDS as
// floats, in raster order, for the lane-ordered float sums of chain_sums (k_lk_fast.hip); tlen = pixels of each segment
// that lie inside the window.
template <int WW, int WH, int F, int FI>
__device__ __forceinline__ void template_pixels(Template<WW, WH, F>& T, const uint32_t* ldsI, uint32_t W0u, uint32_t W1u, int ics,
                                                bool i_inside, int ipx, int ipy, int liw, int lih,
                                                const int (&trow)[Cfg<WW, WH>::TPL], const int (&tcol)[Cfg<WW, WH>::TPL],
                                                const uint32_t (&psel)[Cfg<WW, WH>::TPL][(Cfg<WW, WH>::S + 1) / 2], int& a11,
                                                int& a12, int& a22, float* fsum = nullptr, const int* tlen = nullptr)
{
    using C = Cfg<WW, WH>;
    constexpr int S = C::S;
    // the second weight pair as a VGPR (a three-address dot2 takes one scalar), the rounding constants as scalars.
    // The derivatives are formed 4 times too large (|4 Ix| <= 16 320 still fits a 16-bit lane), so that
    // (4 dx * w + 2^15) >> 16 == (dx * w + 2^13) >> 14 lands in the high half of the dot2 result: one v_perm then
    // shifts, packs and masks a pixel pair (pair_sel) where two shifts, a pack and a mask AND were needed.
    const uint32_t W1v = W1u;
    const int kRoundI = 1 << (W_BITS - 6), kRoundD4 = 1 << (W_BITS + 1);
#pragma unroll
    for (int k = 0; k < C::TPL; k++) {
        constexpr int NP = (S + 4) / 2;   // even-aligned column pairs covering columns 0 .. S+2
        constexpr int ND = (S + 2) / 2;   // derivative pairs covering derivative columns 0 .. S
        // The pairs come straight out of the dwords as they lie in LDS: pair kk is bytes 2 kk + sh, 2 kk + sh + 1 of the
        // row, i.e. of the dword pair (d[kk / 2], d[kk / 2 + 1]) at a byte offset below 7, so one v_perm with a per-lane
        // selector takes them out (no v_alignbyte realignment of the row first)
        const int off = ics + tcol[k], sh = off & 3;
        const uint32_t selA = 0x0c010c00u + (uint32_t)sh * 0x00010001u;   // bytes sh, sh + 1 of the pair -> 16-bit lanes
        const uint32_t selB = selA + 0x00020002u;                          // bytes sh + 2, sh + 3
        v2s E[4][NP];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t* p = ldsI + (trow[k] + r) * C::IPD + (off >> 2);
            uint32_t d[(NP - 1) / 2 + 2];
#pragma unroll
            for (int i = 0; i < (NP - 1) / 2 + 2; i++) d[i] = p[i];
            static_for<NP>([&](auto kk) {
                E[r][kk] = as_v2s(__builtin_amdgcn_perm(d[kk / 2 + 1], d[kk / 2], kk % 2 ? selB : selA));
            });
        }
        // I samples first (they need source rows 1 and 2 only): columns (j+1, j+2) are the pair E[.][(j+1)/2] for odd j
        // and the pair one 16-bit lane further along for even j
        static_for<S>([&](auto jj) {
            constexpr int j = jj;
            v2s s1, s2;
            if constexpr (j % 2 == 1) {
                s1 = E[1][(j + 1) / 2]; s2 = E[2][(j + 1) / 2];
            } else {
                s1 = pair_shift(E[1][j / 2], E[1][j / 2 + 1]); s2 = pair_shift(E[2][j / 2], E[2][j / 2 + 1]);
            }
            const int iv = dot2(s2, as_v2s(W1v), dot2_vvs(s1, W0u, kRoundI)) >> (W_BITS - 5);
            T.Ineg[FI][k][j] = (1 << (W_BITS - 6)) - (iv << (W_BITS - 5));
        });
        // Scharr x 4, two columns per instruction: t0 = 12*(a + c) + 40*b, t1 = c - a down the rows, then
        // dx = t0[i+2] - t0[i], dy = 12*(t1[i+2] + t1[i]) + 40*t1[i+1] along the row
        v2s dxp[2][ND], dyp[2][ND];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            v2s t0[NP], t1[NP];
#pragma unroll
            for (int q = 0; q < NP; q++) {
                t0[q] = (E[r][q] + E[r + 2][q]) * (short)12 + E[r + 1][q] * (short)40;
                t1[q] = E[r + 2][q] - E[r][q];
            }
#pragma unroll
            for (int d = 0; d < ND; d++) {
                dxp[r][d] = t0[d + 1] - t0[d];
                dyp[r][d] = (t1[d + 1] + t1[d]) * (short)12 + pair_shift(t1[d], t1[d + 1]) * (short)40;
            }
        }
        if (!i_inside) {
            // derivative image is zero outside the frame (BORDER_CONSTANT), SURVEY.md A.4.  Both derivative rows under one
            // branch: with a branch per row the compiler hoisted their shared column tests into the interior path.
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const int gy = ipy + trow[k] + r;
                const bool row_in = gy >= 0 && gy < lih;
#pragma unroll
                for (int d = 0; d < ND; d++) {
                    const int gx = ipx + tcol[k] + 2 * d;
                    const bool in0 = row_in && gx >= 0 && gx < liw, in1 = row_in && gx + 1 >= 0 && gx + 1 < liw;
                    const uint32_t m = (in0 ? 0xffffu : 0u) | (in1 ? 0xffff0000u : 0u);
                    dxp[r][d] = as_v2s(as_u32(dxp[r][d]) & m);
                    dyp[r][d] = as_v2s(as_u32(dyp[r][d]) & m);
                }
            }
        }
        // derivative samples, x 2^16: the sample itself is the high half
        int ixw[S], iyw[S];
        static_for<S>([&](auto jj) {
            constexpr int j = jj;
            // derivative columns (j, j+1) of derivative rows 0 and 1
            v2s gx0, gx1, gy0, gy1;
            if constexpr (j % 2 == 0) {
                gx0 = dxp[0][j / 2]; gx1 = dxp[1][j / 2]; gy0 = dyp[0][j / 2]; gy1 = dyp[1][j / 2];
            } else {
                gx0 = pair_shift(dxp[0][j / 2], dxp[0][j / 2 + 1]); gx1 = pair_shift(dxp[1][j / 2], dxp[1][j / 2 + 1]);
                gy0 = pair_shift(dyp[0][j / 2], dyp[0][j / 2 + 1]); gy1 = pair_shift(dyp[1][j / 2], dyp[1][j / 2 + 1]);
            }
            ixw[j] = dot2(gx1, as_v2s(W1v), dot2_vvs(gx0, W0u, kRoundD4));
            iyw[j] = dot2(gy1, as_v2s(W1v), dot2_vvs(gy0, W0u, kRoundD4));
        });
        if (fsum) {
            constexpr int NPX = WW * WH;
            static_for<S>([&](auto jj) {
                constexpr int j = jj;
                if (j < tlen[k]) {
                    const int idx = trow[k] * WW + tcol[k] + j;
                    const int ix = ixw[j] >> 16, iy = iyw[j] >> 16;
                    fsum[idx] = (float)(ix * ix);
                    fsum[NPX + idx] = (float)(ix * iy);
                    fsum[2 * NPX + idx] = (float)(iy * iy);
                }
            });
        }
        // gradient pairs for the dot2 form of the residual sums (pixels beyond the window's right edge and the
        // surplus lanes' pixels are cleared here, once, by the lane's pair selectors), and the 2x2 matrix sums on
        // the same pairs
        static_for<(S + 1) / 2>([&](auto qq) {
            constexpr int q = qq, q1 = 2 * q + 1 < S ? 2 * q + 1 : 2 * q;   // a lone last pixel: its partner half is cleared
            const uint32_t px2 = __builtin_amdgcn_perm((uint32_t)ixw[q1], (uint32_t)ixw[2 * q], psel[k][q]);
            const uint32_t py2 = __builtin_amdgcn_perm((uint32_t)iyw[q1], (uint32_t)iyw[2 * q], psel[k][q]);
            T.Ixp[FI][k][q] = px2;
            T.Iyp[FI][k][q] = py2;
            if (k == 0 && q == 0) {
                a11 = dot2_vv0(as_v2s(px2), as_v2s(px2));
                a12 = dot2_vv0(as_v2s(px2), as_v2s(py2));
                a22 = dot2_vv0(as_v2s(py2), as_v2s(py2));
            } else {
                a11 = dot2(as_v2s(px2), as_v2s(px2), a11);
                a12 = dot2(as_v2s(px2), as_v2s(py2), a12);
                a22 = dot2(as_v2s(py2), as_v2s(py2), a22);
            }
        });
    }
}

// ---- pixel phase: residual of ONE feature at the window origin encoded in `jb` ------------------------------------
// jb = byte offset of the window's first pixel inside the feature's staged search tile (wave-uniform).
// V0u, V1u = the weights by column (pack_weights_c0 / _c1).  A sample is taken from the COLUMN pairs (J[y][x], J[y+1][x])
// and (J[y][x+1], J[y+1][x+1]): neighbouring samples share one, so S + 1 v_perm widen a segment's two rows instead of the
// 2 S of row pairs.  The four products and the seed are added in another order, exactly (32-bit integers, no overflow).
// ERR = false: b1 = sum diff*Ix, b2 = sum diff*Iy.   ERR = true: b1 = sum |diff| over the real window pixels.
// fsum != nullptr: the two products of every window pixel also go to LDS as floats (int32 -> float, as _mm_cvtepi32_ps),
// in raster order (trow, tcol = the segments' window rows / first columns).
//
// Its two halves, for one segment.  fetch + widen: the segment's two tile rows out of LDS (row_dwords x 2)
// and its S + 1 column pairs.  They depend on the byte offset `off` (= jb + the segment's own offset) and on what the tile
// holds, not on the weights: an iteration whose window origin lies in the same pixel cell as the one before it, with
// nothing restaged in between, gets the same pairs (k_lk_fast.hip keeps them for the windows with one segment per lane).
template <int WW, int WH>
__device__ __forceinline__ void segment_pairs(const uint32_t* ldsJ, int off, v2s (&cp)[Cfg<WW, WH>::S + 1])
{
    using C = Cfg<WW, WH>;
    constexpr int S = C::S, NXJ = (S + 1 + 3) / 4;
    uint32_t Y0[NXJ], Y1[NXJ];
    row_dwords<NXJ>(ldsJ, off, Y0);
    row_dwords<NXJ>(ldsJ + C::JPD, off, Y1);
    static_for<S + 1>([&](auto qq) {
        constexpr int q = qq;
        cp[q] = col_pair<q, NXJ>(Y0, Y1);
    });
}

// samples + products of segment k from its column pairs: added to b1, b2 (the caller zeroes them)
template <int WW, int WH, int F, int FI, bool ERR>
__device__ __forceinline__ void segment_residual(const Template<WW, WH, F>& T, int k, const v2s (&cp)[Cfg<WW, WH>::S + 1],
                                                 uint32_t V0u, uint32_t V1v, int tlen_k, int& b1, int& b2,
                                                 float* fsum = nullptr, int trow_k = 0, int tcol_k = 0)
{
    using C = Cfg<WW, WH>;
    constexpr int S = C::S;
    int diff[S];
    static_for<S>([&](auto qq) {
        constexpr int q = qq;
        // ((J bilinear + 256) >> 9) - I, with 256 - (I << 9) as the accumulator seed
        diff[q] = dot2(cp[q + 1], as_v2s(V1v), dot2_vsv(cp[q], V0u, T.Ineg[FI][k][q])) >> (W_BITS - 5);
    });
    if constexpr (ERR) {
        static_for<S>([&](auto qq) {
            constexpr int q = qq;
            b1 += q < tlen_k ? (diff[q] < 0 ? -diff[q] : diff[q]) : 0;
        });
    } else {
        if (fsum) {
            constexpr int NPX = WW * WH;
            static_for<S>([&](auto qq) {
                constexpr int q = qq;
                if (q < tlen_k) {
                    const uint32_t gx = T.Ixp[FI][k][q / 2], gy = T.Iyp[FI][k][q / 2];
                    const int ix = (q & 1) ? ((int)gx >> 16) : (int)(short)(gx & 0xffffu);
                    const int iy = (q & 1) ? ((int)gy >> 16) : (int)(short)(gy & 0xffffu);
                    const int idx = trow_k * WW + tcol_k + q;
                    fsum[idx] = (float)(diff[q] * ix);
                    fsum[NPX + idx] = (float)(diff[q] * iy);
                }
            });
        }
        static_for<(S + 1) / 2>([&](auto qq) {
            constexpr int q = qq;
            uint32_t dp;
            if constexpr (2 * q + 1 < S) dp = pack16(diff[2 * q], diff[2 * q + 1]);
            else dp = (uint32_t)diff[2 * q];   // the partner half of the gradient pair is zero
            b1 = dot2(as_v2s(dp), as_v2s(T.Ixp[FI][k][q]), b1);
            b2 = dot2(as_v2s(dp), as_v2s(T.Iyp[FI][k][q]), b2);
        });
    }
}

template <int WW, int WH, int F, int FI, bool ERR>
__device__ __forceinline__ void residual_pixels(const Template<WW, WH, F>& T, const uint32_t* ldsJ, int jb, uint32_t V0u,
                                                uint32_t V1u, const int (&joff)[Cfg<WW, WH>::TPL],
                                                const int (&tlen)[Cfg<WW, WH>::TPL], int& b1, int& b2, float* fsum = nullptr,
                                                const int* trow = nullptr, const int* tcol = nullptr)
{
    using C = Cfg<WW, WH>;
    const uint32_t V1v = V1u;   // one weight pair rides as a scalar, the other in a VGPR
    b1 = 0; b2 = 0;
#pragma unroll
    for (int k = 0; k < C::TPL; k++) {
        v2s cp[C::S + 1];
        segment_pairs<WW, WH>(ldsJ, jb + joff[k], cp);
        segment_residual<WW, WH, F, FI, ERR>(T, k, cp, V0u, V1v, tlen[k], b1, b2, fsum, fsum ? trow[k] : 0,
                                             fsum ? tcol[k] : 0);
    }
}

}  // namespace lkf
}  // namespace icelk
