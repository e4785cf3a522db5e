// resize.h -- the arithmetic of the movie's scaler as plain C++ for the host and the device alike: an 8-bit R G B picture
// resampled to any size, larger or smaller, as Pillow's Image.resize(size, Image.BICUBIC) resamples it, byte for byte.
// The host statement (resize_host below, exported by abi_movie.hip), the kernels (k_resize.hip) and
// tests/movie_restatement.py (numpy, written independently) all compute what is stated here.  DESIGN.md 7.11 has the rule.
//
//   axis      `in` source samples -> `out` output samples: scale = in / out (double), fs = max(scale, 1), support = 2 fs.
//             Output xx: center = (xx + 0.5) scale, first = max(0, (int)(center - support + 0.5)),
//             end = min(in, (int)(center + support + 0.5)), count = end - first ((int) truncates).  Weight j is
//             B((j + first - center + 0.5) (1 / fs)) with the cubic B of a = -0.5 (bicubic); the weights are divided by
//             their sum, taken in index order, when it is not 0, and k_j = (int)(w_j 2^22 +- 0.5), the sign w_j's.
//             The tables are made on the host in double, with no contraction (-ffp-contract=off): the device gets integers
//   sample    clip(0, 255, (2^21 + sum k_j s[first + j]) >> 22) in 32-bit signed arithmetic, the shift arithmetic
//   passes    the horizontal pass first, over the source rows the vertical pass reads (rows lo .. hi - 1 of its table), then
//             the vertical pass on that 8-bit result.  A pass with in == out is skipped
//   limits    every side in 1 .. 16384
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef ICELK_RESIZE_FN
#define ICELK_RESIZE_FN __host__ __device__ __forceinline__
#endif

#include <vector>

namespace icelk {
namespace resize {

constexpr int kMaxSide = 16384;
constexpr int kBits = 22;   // of the fixed-point weights: 32 - 8 - 2

ICELK_RESIZE_FN bool side_ok(int v) { return v >= 1 && v <= kMaxSide; }

// the 8-bit sample of an accumulator that started at 1 << (kBits - 1): clip(0, 255, acc >> kBits).  Clamped first and shifted
// then, which gives the same value.  The other order is not used: where two such bytes are packed side by side hipcc
// (ROCm 7.2) makes one v_ashr_pk_u8_i32 of them and takes the upper half of its result for zero, while the MI355X left the
// register's old upper half there -- k_resize_cols wrote bytes 2 and 3 of every dword wrong (tests/test_gpu_movie.py)
ICELK_RESIZE_FN uint8_t clip8(int32_t acc)
{
    constexpr int32_t top = (256 << kBits) - 1;
    const int32_t v = acc < 0 ? 0 : acc > top ? top : acc;
    return (uint8_t)(v >> kBits);
}

// one output sample: n taps k over samples `step` bytes apart
ICELK_RESIZE_FN uint8_t sample(const uint8_t* s, size_t step, const int32_t* k, int n)
{
    int32_t acc = 1 << (kBits - 1);
    for (int j = 0; j < n; j++) acc += k[j] * (int32_t)s[(size_t)j * step];
    return clip8(acc);
}

// mencoder's scale=W:-10 as this project states it: the width asked for, the height that keeps the proportions rounded to
// the nearest multiple of 16, at least 16.  movie_width <= 0: the picture's own width.  False for a picture or a width
// outside the limits; the height is plain arithmetic (at most 2^28 + 8) and may be more than a frame can have
inline bool movie_size(int w, int h, int movie_width, int* mw, int* mh)
{
    if (!side_ok(w) || !side_ok(h) || movie_width > kMaxSide) return false;
    const int W = movie_width <= 0 ? w : movie_width;
    const int64_t H = ((int64_t)W * h / w + 8) / 16 * 16;
    *mw = W, *mh = H < 16 ? 16 : (int)H;
    return true;
}

// ---- host only: an axis' table
struct Axis {
    int in = 0, out = 0, pitch = 0;   // pitch: the largest count
    int lo = 0, hi = 0;               // the source samples the axis reads: first[0] .. first[out - 1] + count[out - 1] - 1
    std::vector<int32_t> first, count, k;   // out, out, out * pitch (a row's unused tail is 0)
};

inline double bicubic(double x)
{
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

inline void make_axis(int in, int out, Axis* A)
{
    const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale, support = 2.0 * fs, ss = 1.0 / fs;
    A->in = in, A->out = out, A->pitch = 0;
    A->first.assign((size_t)out, 0), A->count.assign((size_t)out, 0);
    for (int xx = 0; xx < out; xx++) {
        const double center = (xx + 0.5) * scale;
        int first = (int)(center - support + 0.5), end = (int)(center + support + 0.5);
        if (first < 0) first = 0;
        if (end > in) end = in;
        A->first[xx] = first, A->count[xx] = end - first;
        if (end - first > A->pitch) A->pitch = end - first;
    }
    A->lo = A->first[0], A->hi = A->first[out - 1] + A->count[out - 1];
    A->k.assign((size_t)out * A->pitch, 0);
    std::vector<double> w((size_t)A->pitch);
    for (int xx = 0; xx < out; xx++) {
        const double center = (xx + 0.5) * scale;
        const int first = A->first[xx], n = A->count[xx];
        double ww = 0.0;
        for (int j = 0; j < n; j++) ww += w[j] = bicubic((j + first - center + 0.5) * ss);
        for (int j = 0; j < n; j++) {
            if (ww != 0.0) w[j] /= ww;
            const double f = w[j] * (double)(1 << kBits);
            A->k[(size_t)xx * A->pitch + j] = w[j] < 0 ? (int32_t)(-0.5 + f) : (int32_t)(0.5 + f);
        }
    }
}

// the w x h picture at rgb (stride bytes per row) -> ow x oh at out (out_stride bytes per row); every side in 1 .. kMaxSide
inline void resize_host(const uint8_t* rgb, int w, int h, size_t stride, int ow, int oh, uint8_t* out, size_t out_stride)
{
    Axis X, Y;
    if (w != ow) make_axis(w, ow, &X);
    if (h != oh) make_axis(h, oh, &Y);
    const int lo = h != oh ? Y.lo : 0, hi = h != oh ? Y.hi : h;   // the rows the vertical pass reads
    std::vector<uint8_t> mid;
    const uint8_t* src = rgb + (size_t)lo * stride;   // row lo of what the vertical pass reads, rows src_stride apart
    size_t src_stride = stride;
    if (w != ow) {
        uint8_t* dst = out;
        size_t dst_stride = out_stride;
        if (h != oh) {
            mid.resize((size_t)(hi - lo) * 3 * ow);
            dst = mid.data(), dst_stride = 3 * (size_t)ow;
        }
        for (int y = lo; y < hi; y++)
            for (int x = 0; x < ow; x++)
                for (int c = 0; c < 3; c++)
                    dst[(size_t)(y - lo) * dst_stride + 3 * (size_t)x + c] =
                        sample(rgb + (size_t)y * stride + 3 * (size_t)X.first[x] + c, 3, &X.k[(size_t)x * X.pitch], X.count[x]);
        src = dst, src_stride = dst_stride;
    }
    if (h != oh) {
        for (int y = 0; y < oh; y++)
            for (size_t b = 0; b < 3 * (size_t)ow; b++)
                out[(size_t)y * out_stride + b] = sample(src + (size_t)(Y.first[y] - lo) * src_stride + b, src_stride, &Y.k[(size_t)y * Y.pitch], Y.count[y]);
    } else if (w == ow) {
        for (int y = 0; y < h; y++)
            for (size_t b = 0; b < 3 * (size_t)w; b++) out[(size_t)y * out_stride + b] = rgb[(size_t)y * stride + b];
    }
}

}  // namespace resize
}  // namespace icelk
