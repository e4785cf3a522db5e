// thumb_main.cpp -- csrc/thumb_raster.h under the host's sanitizers, as a program of its own (nothing of the library in it):
// the size rule, the host statement of the thumbnail on images and thumbnails of exactly the stated sizes, k_jpeg_thumb's
// decomposition walked lane by lane with a column-sum array of exactly one pass per quarter of the workgroup (every index it
// forms is checked, every sum is held against its bound, nothing is read that no lane stored, and the pixels must equal
// the host statement's), and the inset paste at the picture's edges into a picture of exactly width x height pixels.  tests/test_thumb_sanitizers_host.py builds and runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../iceberg_tracking_code_amd/csrc/thumb_raster.h"

using namespace icelk;

#define REQUIRE(x)                                                   \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("line %d: %s\n", __LINE__, #x);                   \
            exit(1);                                                 \
        }                                                            \
    } while (0)

static uint32_t rnd_state = 97531;
static uint32_t rnd()
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

// the kernel's walk of one channel: workgroups of `per` pixels, passes of kChunk columns, quarters of the workgroup taking
// every fourth row, lanes of four columns, the columns beyond W a lane's four reach repeating the last one (what
// rgbpx::rgb4 returns there)
static void walk_as_the_kernel(const std::vector<uint8_t>& img, int W, int H, int channels, int c, int Wt, int Ht, std::vector<uint8_t>& out)
{
    const int per = thumb::pixels_per_group(W, Wt), lanes = thumb::kThreads / thumb::kRowGroups;
    REQUIRE(per >= 1 && 3 * per <= thumb::kThreads && 4 * lanes == thumb::kChunk);
    std::vector<uint32_t> col((size_t)thumb::kRowGroups * thumb::kChunk);
    for (int j = 0; j < Ht; j++) {
        const int y0 = plot::first_source(j, H, Ht), y1 = plot::last_source(j, H, Ht);
        REQUIRE(y0 >= 0 && y1 < H && y0 <= y1);
        for (int i_first = 0; i_first < Wt; i_first += per) {
            const int i_last = i_first + per - 1 < Wt - 1 ? i_first + per - 1 : Wt - 1;
            const int xs = plot::first_source(i_first, W, Wt) & ~3, xe = plot::last_source(i_last, W, Wt) + 1;
            REQUIRE(xs >= 0 && xe <= W);
            if ((int64_t)thumb::kSpan * Wt >= W) REQUIRE(xe - xs <= thumb::kChunk);   // one pass, but for pixels wider than one
            std::vector<uint64_t> acc(per, 0);
            for (int base = xs; base < xe; base += thumb::kChunk) {
                std::fill(col.begin(), col.end(), 0xdeadbeefu);   // what no lane stored must not be read
                for (int t = 0; t < thumb::kThreads; t++) {
                    const int quarter = t / lanes, lane = t % lanes, x4 = base + 4 * lane;
                    if (x4 >= xe) continue;
                    REQUIRE(x4 < W);
                    for (int k = 0; k < 4; k++) {
                        const int x = x4 + k < W - 1 ? x4 + k : W - 1;
                        uint32_t s = 0;
                        for (int y = y0 + quarter; y <= y1; y += thumb::kRowGroups)
                            s += (uint32_t)plot::overlap(y, j, H, Ht) * img.at(((size_t)y * W + x) * channels + c);
                        REQUIRE(s <= (uint32_t)H * 255u && s < (1u << 24));
                        col.at((size_t)quarter * thumb::kChunk + 4 * lane + k) = s;
                    }
                }
                for (int t = 0; t < per && i_first + t <= i_last; t++) {
                    const int i = i_first + t;
                    const int my0 = plot::first_source(i, W, Wt), my1 = plot::last_source(i, W, Wt);
                    const int lo = my0 > base ? my0 : base, hi = my1 < base + thumb::kChunk - 1 ? my1 : base + thumb::kChunk - 1;
                    if (lo <= hi) REQUIRE(lo - base >= 0 && hi - base < thumb::kChunk && hi < xe);
                    for (int x = lo; x <= hi; x++)
                        for (int q = 0; q < thumb::kRowGroups; q++) REQUIRE(col[(size_t)q * thumb::kChunk + x - base] != 0xdeadbeefu);
                    acc[t] += thumb::row_sum(col.data(), thumb::kRowGroups, thumb::kChunk, base, lo, hi, i, W, Wt);
                    REQUIRE(acc[t] <= (uint64_t)W * H * 255u);
                }
            }
            for (int t = 0; t < per && i_first + t <= i_last; t++) out.at(((size_t)j * Wt + i_first + t) * 3 + (channels == 1 ? 0 : c)) = (uint8_t)plot::average(acc[t], W, H);
        }
    }
}

static void reduce(int W, int H, int channels, int Wt, int Ht)
{
    std::vector<uint8_t> img((size_t)W * H * channels), out((size_t)Wt * Ht * 3, 0xAA), again((size_t)Wt * Ht * 3, 0xAA);
    for (auto& v : img) v = (uint8_t)(rnd() % 5 == 0 ? 255 : rnd());
    thumb::reduce_host(img.data(), W, H, channels, (size_t)W * channels, Wt, Ht, out.data(), (size_t)Wt * 3);
    for (int c = 0; c < channels; c++) walk_as_the_kernel(img, W, H, channels, c, Wt, Ht, again);
    if (channels == 1)
        for (size_t p = 0; p < (size_t)Wt * Ht; p++) again[3 * p + 1] = again[3 * p + 2] = again[3 * p];
    REQUIRE(out == again);
    if (Wt == W && Ht == H)
        for (size_t p = 0; p < (size_t)W * H; p++)
            for (int c = 0; c < 3; c++) REQUIRE(out[3 * p + c] == img[p * channels + (channels == 1 ? 0 : c)]);
    printf("%d x %d x %d -> %d x %d, %d pixel(s) per workgroup\n", W, H, channels, Wt, Ht, thumb::pixels_per_group(W, Wt));
}

static void sizes()
{
    int tw = -1, th = -1;
    const int bad[][4] = {{0, 1, 1, 1}, {1, 0, 1, 1}, {65536, 1, 1, 1}, {1, 65536, 1, 1}, {1, 1, 0, 1}, {1, 1, 1, 0}, {1, 1, 16385, 1}, {1, 1, 1, 16385}};
    for (const auto& b : bad) REQUIRE(!thumb::size(b[0], b[1], b[2], b[3], &tw, &th) && tw == -1 && th == -1);
    long n = 0;
    const int edge[] = {1, 2, 3, 255, 256, 1023, 1024, 16383, 16384, 16385, 65534, 65535};
    for (int W : edge)
        for (int H : edge)
            for (int bw : edge)
                for (int bh : edge) {
                    if (bw > thumb::kMaxBox || bh > thumb::kMaxBox) continue;
                    REQUIRE(thumb::size(W, H, bw, bh, &tw, &th));
                    REQUIRE(tw >= 1 && tw <= W && tw <= bw && th >= 1 && th <= H && th <= bh);
                    const int per = thumb::pixels_per_group(W, tw);
                    REQUIRE(per >= 1 && 3 * per <= thumb::kThreads);
                    n++;
                }
    printf("%ld sizes\n", n);
}

static void paste(int Wo, int Ho)
{
    std::vector<uint8_t> rgb((size_t)Wo * Ho * 3, 200);
    const int k = map::text_scale(Wo);
    const int tw = Wo < 40 ? Wo : 13, th = Ho < 40 ? Ho : 9;
    std::vector<uint8_t> px((size_t)tw * th * 3);
    for (auto& v : px) v = (uint8_t)(1 + rnd() % 199);
    const int at[][2] = {{0, 0}, {Wo - tw, 0}, {0, Ho - th}, {Wo - tw, Ho - th}};
    const int label_at[][2] = {{-5, -3}, {Wo - 4 * k, Ho - 3 * k}, {-1048576, -1048576}, {1048576, 1048576}, {Wo - 1, 0}, {0, Ho - 1}, {Wo, Ho}, {2, 2}};
    const char* text = "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-:./ ,()abcd";   // 48 characters
    long changed = 0;
    for (const auto& a : at)
        for (const auto& l : label_at) {
            thumb::Inset I[2];
            I[0].x0 = a[0], I[0].y0 = a[1], I[0].w = tw, I[0].h = th, I[0].px = px.data(), I[0].pitch = 3 * tw;
            REQUIRE(map::make_text(text, l[0], l[1], &I[0].label));
            I[1] = I[0];
            I[1].x0 = at[3][0], I[1].y0 = at[3][1];
            REQUIRE(map::make_text("", 0, 0, &I[1].label));
            std::fill(rgb.begin(), rgb.end(), 200);
            thumb::paste_host(I, 2, Wo, Ho, rgb.data(), (size_t)Wo * 3);
            for (int y = 0; y < th; y++)
                for (int x = 0; x < 3 * tw; x++) {
                    const uint8_t v = rgb[((size_t)(at[3][1] + y) * Wo + at[3][0]) * 3 + x];
                    REQUIRE(v == px[(size_t)y * 3 * tw + x]);   // the later inset, which has no label, covers what came before
                }
            for (uint8_t v : rgb) changed += v != 200;
        }
    REQUIRE(changed > 0);
    printf("picture %d x %d, thumbnail %d x %d, text scale %d\n", Wo, Ho, tw, th, k);
}

int main()
{
    sizes();
    const int shapes[][4] = {{67, 45, 67, 45}, {67, 45, 66, 44}, {67, 45, 1, 1}, {67, 45, 9, 7}, {64, 48, 8, 6}, {2100, 9, 260, 1}, {9, 2100, 1, 260},
                             {2100, 9, 1, 1}, {2100, 9, 2100, 9}, {2100, 9, 2099, 8}, {4000, 24, 250, 2}, {65535, 1, 65535, 1}, {65535, 1, 16384, 1},
                             {65535, 1, 1, 1}, {65535, 1, 63, 1}, {1, 65535, 1, 65535}, {1, 65535, 1, 16384}, {1, 65535, 1, 1}, {3, 5, 2, 3}};
    for (const auto& s : shapes)
        for (int channels = 1; channels <= 3; channels += 2) reduce(s[0], s[1], channels, s[2], s[3]);
    paste(64, 1);
    paste(64, 48);
    paste(1400, 40);
    paste(16384, 3);
    printf("done\n");
    return 0;
}
