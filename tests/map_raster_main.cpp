// map_raster_main.cpp -- csrc/map_raster.h under the host's sanitizers, as a program of its own (nothing of the library in
// it): the walks of k_map_cells, k_map_polyline and k_map_arrows over coordinates at and beyond the limits into planes of
// exactly width x height words, with the hit bound of one arrow (7 max(vw, vh) + 97^2) asserted for every arrow drawn, and
// every pixel resolved under 16 texts of 48 characters, 8 cameras and a colour bar per view.
// tests/test_map_sanitizers_host.py builds and runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../iceberg_tracking_code_amd/csrc/map_raster.h"

using namespace icelk;

#define REQUIRE(x)                                                   \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("line %d: %s\n", __LINE__, #x);                   \
            exit(1);                                                 \
        }                                                            \
    } while (0)

static uint32_t rnd_state = 4321;
static uint32_t rnd()
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 8;
}

struct Planes {
    int W, H;
    std::vector<uint32_t> base, top, count;
    Planes(int w, int h) : W(w), H(h), base((size_t)w * h, 0), top((size_t)w * h, 0), count((size_t)w * h, 0) {}
};

static void picture(int W, int H, int n_views, double metres_per_pixel)
{
    Planes P(W, H);
    map::Scene* S = new map::Scene;
    memset(S, 0, sizeof(*S));
    S->Wo = W, S->Ho = H, S->n_views = n_views;
    const int pw = W / n_views;
    std::vector<std::vector<double>> kept(n_views);
    long arrows_drawn = 0, most = 0;
    for (int v = 0; v < n_views; v++) {
        map::View V;
        V.x0 = v * pw + 1, V.y0 = 2, V.w = pw - 8, V.h = H - 3, V.bar_x0 = V.x0 + V.w + 1, V.bar_w = 4;
        V.xmin = 500000.0, V.xmax = V.xmin + metres_per_pixel * V.w, V.ymin = 7000000.0, V.ymax = V.ymin + metres_per_pixel * V.h;
        REQUIRE(V.x0 >= 0 && V.x0 + V.w <= W && V.y0 + V.h <= H && V.bar_x0 + V.bar_w <= W);
        S->P[v].V = V;
        const double m = metres_per_pixel, far = m * 1048575.0;
        const double xs[] = {V.xmin, V.xmax, V.xmin - 0.5 * m, V.xmax + 0.49 * m, V.xmin + far, V.xmin - far, V.xmin + m * 1048576.0,
                             V.xmin + 3.3 * m, V.xmax - 7.25 * m, (V.xmin + V.xmax) / 2, nan(""), HUGE_VAL, -HUGE_VAL, 1e300, -1e300};
        const double ys[] = {V.ymin, V.ymax, V.ymin - 0.5 * m, V.ymax + 0.49 * m, V.ymax - far, V.ymax + far, V.ymax - m * 1048576.0,
                             V.ymin + 2.7 * m, V.ymax - 5.5 * m, (V.ymin + V.ymax) / 2, nan(""), HUGE_VAL, -HUGE_VAL, 1e300, -1e300};
        const int ne = (int)(sizeof(xs) / sizeof(xs[0]));
        auto at = [&](int p, int q) {
            REQUIRE(p >= 0 && p < V.w && q >= 0 && q < V.h);
            return (size_t)(V.y0 + q) * W + (V.x0 + p);
        };
        auto code = [&](uint32_t c) {
            return [&P, at, c](int p, int q) {
                uint32_t& b = P.base.at(at(p, q));
                if (b < c) b = c;
            };
        };
        // cells and outline pairs between every two of the edge coordinates
        const double sizes[] = {m * 3.0, m * 0.3, -m * 2.0, far, 2 * far, 0.0, nan(""), HUGE_VAL};
        for (int a = 0; a < ne; a++)
            for (int b = 0; b < ne; b++) {
                for (double size : sizes) map::walk_cell(V, xs[a], ys[b], size, (a + b) & 1, code(1), code(2));
                for (int c = 0; c < ne; c += 2)
                    for (int d = 1; d < ne; d += 2) map::walk_segment(V, xs[a], ys[b], xs[c], ys[d], code(3));
            }
        // arrows: every pair of edge coordinates as position and as tip, both pivots, widths from hair to beam
        const double widths[] = {m * 0.01, m, m * 2.4, m * 6.6, m * 30.0, m * 1e6, 1e300};
        const long bound = 7L * (V.w > V.h ? V.w : V.h) + 97L * 97L;
        std::vector<double>& A = kept[v];
        auto draw = [&](double x, double y, double dx, double dy, double speed, double width, bool mid) {
            const int w = map::arrow_width(V, width);
            REQUIRE(w >= 256 && map::shaft_thickness(w) >= 1 && map::shaft_thickness(w) <= map::kMaxThick);
            const double a5[5] = {x, y, dx, dy, speed};
            A.insert(A.end(), a5, a5 + 5);
            const uint32_t id = (uint32_t)(A.size() / 5);
            long hits = 0;
            map::walk_arrow(V, w, mid, x, y, dx, dy, speed, [&](int p, int q) {
                const size_t o = at(p, q);
                if (P.top.at(o) < id) P.top.at(o) = id;
                P.count.at(o)++;
                hits++;
            });
            REQUIRE(hits <= bound);
            if (hits > most) most = hits;
            arrows_drawn++;
        };
        int k = 0;
        for (int a = 0; a < ne; a++)
            for (int b = 0; b < ne; b++)
                for (int c = 0; c < ne; c++)
                    for (int d = 0; d < ne; d++, k++) {
                        const double width = widths[k % 7];
                        draw(xs[a], ys[b], xs[c] - xs[a], ys[d] - ys[b], 0.1 + 0.001 * (k % 500), width, (k / 7) & 1);
                    }
        for (int n = 0; n < 20000; n++) {
            const double x = V.xmin + m * ((double)(rnd() % (uint32_t)(3 * V.w)) - V.w + 0.37), y = V.ymin + m * ((double)(rnd() % (uint32_t)(3 * V.h)) - V.h + 0.61);
            const double dx = m * ((double)(rnd() % 161) - 80), dy = m * ((double)(rnd() % 161) - 80);
            const double speeds[] = {0.0, 0.3, 0.5, 0.7, -0.1, nan(""), HUGE_VAL};
            draw(x, y, dx, dy, speeds[n % 7], widths[n % 5], n & 1);
        }
        S->P[v].arrows = A.data();
        S->P[v].vmax = 0.5;
        map::make_table(v ? 0.75 : 1.0, S->P[v].T);
        const double cams[][2] = {{V.xmin, V.ymin}, {V.xmax, V.ymax}, {V.xmin + far, V.ymin}, {nan(""), V.ymin}, {V.xmin + 5 * m, V.ymax - 4 * m},
                                  {V.xmin - 1.9 * m, V.ymin + 6 * m}, {1e300, 0.0}, {(V.xmin + V.xmax) / 2, (V.ymin + V.ymax) / 2}};
        for (const auto& c : cams)
            if (map::to_fixed(V, c[0], c[1], &S->P[v].cam_x[S->P[v].n_cameras], &S->P[v].cam_y[S->P[v].n_cameras])) S->P[v].n_cameras++;
        REQUIRE(S->P[v].n_cameras == 6);   // all but the NaN and the 1e300
    }
    // 16 texts of 48 characters, at and beyond every edge
    const char* line48 = "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-:./ ,()abcd";
    REQUIRE(strlen(line48) == 48);
    const int pos[16][2] = {{0, 0}, {-5, -5}, {W - 3, 0}, {0, H - 3}, {W - 1, H - 1}, {W, H}, {-300, 3}, {3, -7}, {-1048576, -1048576}, {1048576, 1048576},
                            {W / 2, H / 2}, {1, H / 3}, {W / 3, 1}, {-17, H - 9}, {W - 40, H / 4}, {2, 2}};
    for (int n = 0; n < 16; n++) REQUIRE(map::make_text(line48, pos[n][0], pos[n][1], &S->text[n]) && S->text[n].n == 48);
    S->n_texts = 16;
    map::Text T;
    REQUIRE(!map::make_text("ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-:./ ,()abcde", 0, 0, &T) && !map::make_text("50%", 0, 0, &T) && !map::make_text("a_b", 0, 0, &T));
    REQUIRE(map::make_text("", 0, 0, &T) && T.n == 0);
    for (int ch = 0; ch < 256; ch++) {
        const int g = map::glyph_index(ch);
        REQUIRE(g >= -1 && g < map::kGlyphs);
        if (g >= 0)
            for (int r = 0; r < plot::kGlyphH; r++) REQUIRE(map::glyph_row(g, r) < 32u);
    }
    for (int c = 0; c < 768; c++) S->table[c] = (uint8_t)rnd();
    std::vector<uint8_t> rgb((size_t)3 * W * H);
    long black = 0, red = 0;
    for (int j = 0; j < H; j++)
        for (int i = 0; i < W; i++) {
            const size_t o = (size_t)j * W + i;
            uint8_t* out = &rgb.at(3 * o + 2) - 2;
            map::resolve_pixel(*S, P.base[o], P.top[o], P.count[o], i, j, out);
            black += out[0] == 0 && out[1] == 0 && out[2] == 0;
            red += out[0] == 255 && out[1] == 0 && out[2] == 0;
        }
    REQUIRE(black > 0 && red > 0);
    printf("picture %d x %d, %d view(s), %g m/pixel: %ld arrows, at most %ld hits each, %ld black and %ld red pixels\n", W, H, n_views, metres_per_pixel,
           arrows_drawn, most, black, red);
    delete S;
}

int main()
{
    REQUIRE(map::colour_index(0.0, 0.5) == 0 && map::colour_index(0.5, 0.5) == 255 && map::colour_index(1e308, 1e-308) == 255 &&
            map::colour_index(0.49, 0.5) == 250);
    REQUIRE(!map::speed_ok(nan("")) && !map::speed_ok(-0.1) && !map::speed_ok(HUGE_VAL) && map::speed_ok(0.0));
    picture(64, 48, 1, 10.0);
    picture(64, 11, 2, 10.0);
    picture(97, 61, 2, 0.25);
    picture(160, 120, 1, 1000.0);
    picture(1400, 40, 2, 5.0);
    picture(70, 700, 1, 3.0);
    printf("done\n");
    return 0;
}
