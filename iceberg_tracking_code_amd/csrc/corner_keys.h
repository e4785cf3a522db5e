// corner_keys.h -- what the corner detector's sources exchange, each stated once: the order-preserving response key, the
// 64-bit candidate key, the quality threshold, the constants of the counters a detection uses and their reset.
// Included by k_corners.hip (candidates, K6/K7), k_corners_fast.hip (the two-pass form of the same), k_min_distance.hip
// (selection, K8) and k_tail.hip (the device-driven tail).  A stage that needs any of this includes the header; it does
// not restate it: every stage must cut at the same float and unpack the same bits, or a candidate is binned by one stage
// and dropped by the next.
// The key, its accessors and the threshold are plain C++ for the host and the device alike: tests/corner_keys_main.cpp
// runs this text on the CPU against the numpy statement of tests/strip_arm_frames.py.
// Everything sits in the unnamed namespace, as it did when each source had its own copy: no symbol is shared.
#pragma once
#if defined(__HIPCC__)
#include "icelk_internal.h"
#define ICELK_KEYS_FN __host__ __device__ __forceinline__
#define ICELK_KEYS_CAST_FN __host__ __device__ inline
#else
#define ICELK_KEYS_FN inline
#define ICELK_KEYS_CAST_FN inline
#endif

namespace icelk {

namespace {

// the bits of a float and back, on either side (not forced inline: the device code is then what __float_as_uint /
// __uint_as_float gave, instruction for instruction)
ICELK_KEYS_CAST_FN unsigned float_bits(float v)
{
    unsigned b;
    __builtin_memcpy(&b, &v, sizeof(b));
    return b;
}
ICELK_KEYS_CAST_FN float bits_float(unsigned b)
{
    float v;
    __builtin_memcpy(&v, &b, sizeof(v));
    return v;
}

// order-preserving map float -> uint32 (larger float <=> larger key); 0 is below every float
ICELK_KEYS_FN unsigned ordered_key(float v)
{
    const unsigned b = float_bits(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
ICELK_KEYS_FN float key_to_float(unsigned k)
{
    const unsigned b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return bits_float(b);
}

// low half of a candidate key: (y << 16) | x orders exactly like the raster address y*w + x (the tie-break of
// OpenCV's greaterThanPtr) and needs no division to unpack; frames are < 65536 px on either side
ICELK_KEYS_FN unsigned pack_xy(int x, int y) { return ((unsigned)y << 16) | (unsigned)x; }
ICELK_KEYS_FN int xy_x(unsigned xy) { return (int)(xy & 0xffffu); }
ICELK_KEYS_FN int xy_y(unsigned xy) { return (int)(xy >> 16); }

// the candidate key: response key << 32 | y << 16 | x.  Keys are unique, and their order is OpenCV's: by response, ties
// by raster address
ICELK_KEYS_FN unsigned long long cand_key(float response, int x, int y)
{
    return ((unsigned long long)ordered_key(response) << 32) | pack_xy(x, y);
}
ICELK_KEYS_FN unsigned cand_response_key(unsigned long long key) { return (unsigned)(key >> 32); }
ICELK_KEYS_FN unsigned cand_xy(unsigned long long key) { return (unsigned)key; }
ICELK_KEYS_FN int cand_x(unsigned long long key) { return xy_x(cand_xy(key)); }
ICELK_KEYS_FN int cand_y(unsigned long long key) { return xy_y(cand_xy(key)); }

// max * qualityLevel as the float every stage cuts at; max_key: the published key of the masked maximum, 0 = none
ICELK_KEYS_FN float quality_threshold(unsigned max_key, double quality)
{
    const double max_val = max_key ? (double)key_to_float(max_key) : 0.0;
    return (float)(max_val * quality);
}

// Sobel (ksize 3) taps scaled as cornerEigenValsVecs does
inline void sobel_scale(int block_size, float* k0, float* k1)
{
    double scale = (double)(1 << 2) * block_size;
    scale *= 255.0;
    scale = 1.0 / scale;
    *k1 = (float)(1.0 * scale);
    *k0 = (float)(2.0 * scale);
}

#if defined(__HIPCC__)
__device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

__device__ __forceinline__ float threshold_of(const unsigned* max_key, double quality)
{
    return quality_threshold(*max_key, quality);
}

// Candidate source: nblk regions of `region` keys each, blk_count[b] valid keys in region b.
struct CandSrc {
    const unsigned long long* keys;
    const int* blk_count;
    int nblk;
    int region;
};
inline CandSrc cand_src_of(const CandBuf& cb) { return CandSrc{cb.raw, cb.blk_count, cb.nblk, cb.region}; }

// Every kernel of the min-distance stage and of the tail is launched as ONE-WAVE workgroups (k_min_distance.hip: why)
constexpr int CT = 64;
constexpr int SCAN_CHUNK = 2048;   // cells per workgroup of k_scan; k_cell_count also keeps per-chunk totals
// The chunk totals are hot atomic targets: one per 128-byte line (atomics on one line serialise in its L2 channel,
// ~90 per us), and a wave adds its contributions to a chunk with one atomic.
constexpr int CHUNK_TOT_STRIDE = 32;
constexpr int KEY_BINS = 2048;                // bins counted DOWN from the bin of the maximum: 64 octaves

// What a detection leaves zeroed for the next one of its set, by threads i0, i0 + stride, ...; mode as
// launch_detect_reset documents it: | 1 = the key histogram too, | 2 = and the masked maximum
__device__ __forceinline__ void reset_counters(const DetectCounters& dc, int i0, int stride, int mode)
{
    for (int i = i0; i <= dc.ncell; i += stride) {
        dc.cell_count[i] = 0;
        if (i < dc.ncell) dc.cell_fill[i] = 0;
        if (i % SCAN_CHUNK == 0) dc.chunk_tot[(i / SCAN_CHUNK) * CHUNK_TOT_STRIDE] = 0;
    }
    if (mode & 1)
        for (int i = i0; i < KEY_BINS; i += stride) dc.key_hist[i] = 0;
    if (i0 < 8) dc.undecided[i0] = 0;
    if (i0 == 0) {
        *dc.acc_count = 0;
        *dc.cand_count = 0;
        *dc.prune_key = 0;
        if (mode & 2) *dc.max_key = 0;
    }
}
#endif

}  // namespace

}  // namespace icelk
