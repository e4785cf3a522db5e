// resize_main.cpp -- the movie's scaler (csrc/resize.h: the code the host statement runs and the device's tables come from)
// as a program of its own under the host's sanitizers (test_resize_sanitizers_host.py builds and runs it; nothing of the
// library is linked).
//
// Every picture is a heap allocation of exactly height * stride bytes and every result one of exactly oh * out_stride, so
// a read or a store outside them is AddressSanitizer's to find.  Per case and per fill (random, random 0 / 255, all 0, all
// 255): the tables are checked against what the kernels rely on (0 <= first, first + count <= in, neither ever decreasing,
// the weights of an output adding up to 2^22 within a tap's rounding each), the picture is resized, resized again from a
// copy with a wider stride that is no multiple of 4 into a result with a wider stride, and the two must agree; a constant
// picture must come out constant.  One line per case, then the count.
#define ICELK_RESIZE_FN inline
#include "../iceberg_tracking_code_amd/csrc/resize.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace icelk;

namespace {

[[noreturn]] void die(const char* what, int a = 0, int b = 0)
{
    fprintf(stderr, "resize_main: %s (%d, %d)\n", what, a, b);
    exit(2);
}

uint32_t g_state = 2024;
uint32_t rnd() { return g_state = g_state * 1664525u + 1013904223u, g_state >> 8; }

struct Buffer {   // exactly n bytes
    uint8_t* p;
    explicit Buffer(size_t n) : p((uint8_t*)malloc(n ? n : 1)) {}
    ~Buffer() { free(p); }
};

void check_axis(int in, int out)
{
    resize::Axis A;
    resize::make_axis(in, out, &A);
    if ((int)A.first.size() != out || (int)A.count.size() != out || A.k.size() != (size_t)out * A.pitch) die("table sizes", in, out);
    int last_first = 0, last_end = 0;
    for (int o = 0; o < out; o++) {
        const int first = A.first[o], n = A.count[o];
        if (first < 0 || n < 1 || n > A.pitch || first + n > in) die("taps outside the axis", in, out);
        if (first < last_first || first + n < last_end) die("taps that go backwards", in, out);
        last_first = first, last_end = first + n;
        int64_t sum = 0;
        for (int j = 0; j < n; j++) sum += A.k[(size_t)o * A.pitch + j];
        if (sum < (1 << resize::kBits) - n || sum > (1 << resize::kBits) + n) die("weights that do not add up to one", in, out);
    }
    if (A.lo != A.first[0] || A.hi != last_end) die("lo / hi", in, out);
}

const int kCases[][4] = {{1, 1, 16, 16},    {2, 3, 16, 16},     {5, 7, 3, 16},       {37, 23, 64, 48},   {64, 48, 37, 23},
                         {33, 17, 33, 32},  {257, 130, 31, 16}, {1200, 13, 2000, 16}, {1400, 40, 2000, 64}, {4099, 5, 16, 16},
                         {16, 16, 16, 16}};

}  // namespace

int main()
{
    int done = 0;
    for (const auto& q : kCases) {
        const int w = q[0], h = q[1], ow = q[2], oh = q[3];
        if (w != ow) check_axis(w, ow);
        if (h != oh) check_axis(h, oh);
        for (int fill = 0; fill < 4; fill++) {
            const size_t stride = 3 * (size_t)w, wide = stride + 5 - (stride + 5) % 4 + 1;   // wide % 4 == 1
            Buffer a(stride * h), b(wide * h), out(3 * (size_t)ow * oh), out2((3 * (size_t)ow + 7) * oh);
            for (int y = 0; y < h; y++)
                for (size_t x = 0; x < stride; x++) {
                    const uint8_t v = fill == 0 ? (uint8_t)rnd() : fill == 1 ? (uint8_t)((rnd() & 1) * 255) : fill == 2 ? 0 : 255;
                    a.p[y * stride + x] = b.p[y * wide + x] = v;
                }
            for (int y = 0; y < h; y++) memset(b.p + y * wide + stride, 0x5a, wide - stride);
            memset(out2.p, 0xa5, (3 * (size_t)ow + 7) * oh);
            resize::resize_host(a.p, w, h, stride, ow, oh, out.p, 3 * (size_t)ow);
            resize::resize_host(b.p, w, h, wide, ow, oh, out2.p, 3 * (size_t)ow + 7);
            for (int y = 0; y < oh; y++) {
                if (memcmp(out.p + (size_t)y * 3 * ow, out2.p + (size_t)y * (3 * ow + 7), 3 * (size_t)ow)) die("the strided copy differs", w, ow);
                for (int k = 0; k < 7; k++)
                    if (out2.p[(size_t)y * (3 * ow + 7) + 3 * ow + k] != 0xa5) die("a store between the rows", w, ow);
            }
            if (fill >= 2)
                for (size_t i = 0; i < 3 * (size_t)ow * oh; i++)
                    if (out.p[i] != (fill == 2 ? 0 : 255)) die("a constant picture that does not stay constant", w, ow);
        }
        int mw = 0, mh = 0;
        if (!resize::movie_size(w, h, 2000, &mw, &mh) || mw != 2000 || mh % 16 || mh < 16) die("movie_size", w, h);
        printf("%d x %d -> %d x %d\n", w, h, ow, oh);
        done++;
    }
    printf("%d cases\ndone\n", done);
    return 0;
}
