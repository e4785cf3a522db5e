// plot_raster_main.cpp -- csrc/plot_raster.h under the host's sanitizers, as a program of its own (nothing of the library in
// it): the walks of k_plot_scatter over coordinates at and beyond the limits into count planes of exactly Wo x Ho words, the
// stamp over every pixel, and the index arithmetic of k_plot_background -- its chunks of 1024 columns, the dword each lane
// reads, the LDS entry each lane adds -- replayed lane by lane on rows of exactly `pitch` bytes and an array of exactly
// one chunk.  tests/test_plot_sanitizers_host.py builds and runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../iceberg_tracking_code_amd/csrc/plot_raster.h"

using namespace icelk;

#define REQUIRE(x)                                                   \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("line %d: %s\n", __LINE__, #x);                   \
            exit(1);                                                 \
        }                                                            \
    } while (0)

static uint32_t rnd_state = 12345;
static uint32_t rnd()
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

// the background kernel's workgroup (blockIdx.x = bx, blockIdx.y = j), lane by lane; returns the pixels it made
static int background_group(const std::vector<uint8_t>& frame, int W, int H, int pitch, int Wo, int Ho, int bx, int j, std::vector<uint8_t>& bg)
{
    const int kThreads = 256, kChunk = 1024;
    std::vector<uint32_t> col(kChunk);
    const int i_first = bx * kThreads, i_last = i_first + kThreads - 1 < Wo - 1 ? i_first + kThreads - 1 : Wo - 1;
    const int y0 = plot::first_source(j, H, Ho), y1 = plot::last_source(j, H, Ho);
    REQUIRE(y0 >= 0 && y1 < H && y0 <= y1);
    const int xs = plot::first_source(i_first, W, Wo) & ~3, xe = plot::last_source(i_last, W, Wo) + 1;
    REQUIRE(xs >= 0 && xe <= W);
    std::vector<uint64_t> acc(kThreads, 0);
    for (int base = xs; base < xe; base += kChunk) {
        for (int t = 0; t < kThreads; t++) {
            const int x4 = base + 4 * t;
            if (x4 >= xe) continue;
            uint32_t s[4] = {0, 0, 0, 0};
            for (int y = y0; y <= y1; y++) {
                const uint32_t wy = (uint32_t)plot::overlap(y, j, H, Ho);
                uint32_t v;
                REQUIRE(x4 + 4 <= pitch);
                memcpy(&v, &frame.at((size_t)y * pitch + x4 + 3) - 3, 4);
                for (int k = 0; k < 4; k++) s[k] += wy * ((v >> (8 * k)) & 255u);
            }
            for (int k = 0; k < 4; k++) col.at(4 * t + k) = s[k];
        }
        for (int t = 0; t < kThreads; t++) {
            const int i = i_first + t;
            if (i >= Wo) continue;
            const int my0 = plot::first_source(i, W, Wo), my1 = plot::last_source(i, W, Wo);
            const int lo = my0 > base ? my0 : base, hi = my1 < base + kChunk - 1 ? my1 : base + kChunk - 1;
            for (int x = lo; x <= hi; x++) {
                REQUIRE(x < xe);   // a column phase 1 has summed
                acc[t] += (uint64_t)plot::overlap(x, i, W, Wo) * col.at(x - base);
            }
        }
    }
    int made = 0;
    for (int t = 0; t < kThreads && i_first + t < Wo; t++, made++) bg.at((size_t)j * Wo + i_first + t) = (uint8_t)plot::average(acc[t], W, H);
    return made;
}

static void background(int W, int H, int out_width)
{
    const int Wo = plot::out_width_of(W, out_width), Ho = plot::out_height_of(W, H, Wo), pitch = (W + 63) / 64 * 64;
    REQUIRE(Ho >= 1 && Ho <= H);
    std::vector<uint8_t> frame((size_t)pitch * H), bg((size_t)Wo * Ho);
    for (auto& v : frame) v = (uint8_t)rnd();
    int made = 0;
    for (int j = 0; j < Ho; j++)
        for (int bx = 0; bx < (Wo + 255) / 256; bx++) made += background_group(frame, W, H, pitch, Wo, Ho, bx, j, bg);
    REQUIRE(made == Wo * Ho);
    // against the plain double sum
    for (int n = 0; n < 200; n++) {
        const int i = (int)(rnd() % (uint32_t)Wo), j = (int)(rnd() % (uint32_t)Ho);
        uint64_t sum = 0, wsum = 0;
        for (int y = 0; y < H; y++)
            for (int x = plot::first_source(i, W, Wo); x <= plot::last_source(i, W, Wo); x++) {
                const uint64_t wgt = (uint64_t)plot::overlap(x, i, W, Wo) * plot::overlap(y, j, H, Ho);
                sum += wgt * frame[(size_t)y * pitch + x];
                wsum += wgt;
            }
        REQUIRE(wsum == (uint64_t)W * H);
        REQUIRE(bg[(size_t)j * Wo + i] == plot::average(sum, W, H));
    }
    printf("background %d x %d -> %d x %d\n", W, H, Wo, Ho);
}

static void walks(int W, int H, int out_width)
{
    const int Wo = plot::out_width_of(W, out_width), Ho = plot::out_height_of(W, H, Wo);
    std::vector<uint32_t> lines((size_t)Wo * Ho, 0), dots((size_t)Wo * Ho, 0);
    long steps = 0;
    auto line = [&](int px, int py) {
        REQUIRE(px >= 0 && px < Wo && py >= 0 && py < Ho);
        lines.at((size_t)py * Wo + px)++;
        steps++;
    };
    auto dot = [&](int px, int py) {
        REQUIRE(px >= 0 && px < Wo && py >= 0 && py < Ho);
        dots.at((size_t)py * Wo + px)++;
    };
    const float edge[] = {0.0f, -0.5f, -0.49f, (float)W - 0.5f, (float)W - 0.51f, (float)H - 0.5f, 1048575.0f, -1048575.0f, 1048575.9f, 3.0f, -7.25f, 1e-30f};
    const int ne = (int)(sizeof(edge) / sizeof(edge[0]));
    int pairs = 0;
    for (int a = 0; a < ne; a++)
        for (int b = 0; b < ne; b++)
            for (int c = 0; c < ne; c++)
                for (int d = 0; d < ne; d++) {
                    REQUIRE(plot::vertex_ok(edge[a], edge[b]) && plot::vertex_ok(edge[c], edge[d]));
                    const long before = steps;
                    plot::walk_pair(plot::coord(edge[a], Wo, W), plot::coord(edge[b], Ho, H), plot::coord(edge[c], Wo, W), plot::coord(edge[d], Ho, H), Wo,
                                    Ho, line);
                    REQUIRE(steps - before <= (Wo > Ho ? Wo : Ho));
                    plot::walk_dot(plot::coord(edge[c], Wo, W), plot::coord(edge[d], Ho, H), Wo, Ho, dot);
                    pairs++;
                }
    for (int n = 0; n < 20000; n++) {
        const float x0 = (float)(rnd() % (uint32_t)(3 * W)) - W + 0.37f, y0 = (float)(rnd() % (uint32_t)(3 * H)) - H + 0.61f;
        const float x1 = x0 + (float)(rnd() % 41) - 20, y1 = y0 + (float)(rnd() % 41) - 20;
        plot::walk_pair(plot::coord(x0, Wo, W), plot::coord(y0, Ho, H), plot::coord(x1, Wo, W), plot::coord(y1, Ho, H), Wo, Ho, line);
        plot::walk_dot(plot::coord(x1, Wo, W), plot::coord(y1, Ho, H), Wo, Ho, dot);
    }
    const float nan = nanf(""), inf = HUGE_VALF;
    REQUIRE(!plot::vertex_ok(nan, 0) && !plot::vertex_ok(0, inf) && !plot::vertex_ok(-inf, 0) && !plot::vertex_ok(1048576.0f, 0) &&
            !plot::vertex_ok(0, -1048576.0f));
    // the stamp over every pixel, the longest one
    plot::Stamp S;
    REQUIRE(plot::make_stamp("0123456789-:./ 0123456789-:./ 0123456789-:./ 012", &S) && S.n == plot::kMaxStamp);
    REQUIRE(!plot::make_stamp("0123456789-:./ 0123456789-:./ 0123456789-:./ 0123", &S) && !plot::make_stamp("12h30", &S));
    REQUIRE(plot::make_stamp("0123456789-:./ 0123456789-:./ 0123456789-:./ 012", &S));
    uint32_t TL[plot::kTable], TD[plot::kTable];
    plot::make_tables(TL, TD);
    std::vector<uint8_t> rgb((size_t)3 * Wo * Ho);
    long stamped = 0;
    for (int j = 0; j < Ho; j++)
        for (int i = 0; i < Wo; i++) {
            const size_t p = (size_t)j * Wo + i;
            plot::resolve_pixel((int)(rnd() & 255), lines[p], dots[p], TL, TD, S, i, j, Wo, Ho, &rgb.at(3 * p + 2) - 2);
            stamped += plot::stamp_hit(S, i, j, Wo, Ho);
        }
    printf("walks %d x %d -> %d x %d: %d edge pairs, %ld hits, %ld stamped pixels\n", W, H, Wo, Ho, pairs, steps, stamped);
}

int main()
{
    const int shapes[][3] = {{64, 48, 24}, {37, 29, 16}, {50, 37, 50}, {4000, 8, 1200}, {3000, 7, 8}, {1031, 5, 1030}, {65535, 2, 8}, {9, 65535 / 64, 8}, {2053, 3, 1200}};
    for (const auto& s : shapes) background(s[0], s[1], s[2]);
    for (const auto& s : shapes) walks(s[0], s[1], s[2]);
    printf("done\n");
    return 0;
}
