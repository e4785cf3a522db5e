// png_main.cpp -- the arithmetic and the host statement of the PNG writer (csrc/png_enc.h, csrc/png_enc_host.h: the code the
// kernels of k_png.hip run) as a program of its own under the host's sanitizers (test_png_sanitizers_host.py builds and
// runs it; nothing of the library is linked).
//
// Every picture is a heap allocation of exactly height * stride bytes, the filtered rows one of exactly N = H (1 + 3 W),
// the file one of exactly the length the coder reports, so a read or a store outside them is AddressSanitizer's to find.
// Per picture: the length is asked for with no buffer, the file is written into a buffer of exactly that size and refused
// for one a byte short (nothing written), the length is within the bound, a second run gives the same bytes, a strided
// copy of the picture gives the same file, and the file's frame is checked byte by byte (signature, chunk lengths, CRCs
// recomputed bit by bit, the zlib header, the block header bits).  Then the codes: every length 3 .. 258 and every
// distance 1 .. 32768 is coded and decoded again by a table-free reading of RFC 1951 3.2.5, and the Adler-32 by pieces is
// compared with the byte-by-byte definition across piece lengths that do not divide the stream.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../iceberg_tracking_code_amd/csrc/png_enc_host.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace icelk;

namespace {

[[noreturn]] void die(const char* what, const char* arg = "")
{
    fprintf(stderr, "png_main: %s %s\n", what, arg);
    exit(2);
}

uint32_t g_state = 12345;
uint32_t rnd() { return g_state = g_state * 1664525u + 1013904223u, g_state >> 8; }

struct Picture {
    int w, h;
    uint8_t* px;   // exactly h * 3 w bytes
    Picture(int w_, int h_) : w(w_), h(h_), px((uint8_t*)malloc((size_t)h_ * 3 * w_)) {}
    ~Picture() { free(px); }
    uint8_t& at(int y, int x) { return px[(size_t)y * 3 * w + x]; }
};

uint32_t crc_slow(const uint8_t* p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = c & 1u ? 0xedb88320u ^ (c >> 1) : c >> 1;
    }
    return c ^ 0xffffffffu;
}

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

uint32_t adler_slow(const uint8_t* p, size_t n)
{
    uint32_t a = 1, b = 0;
    for (size_t i = 0; i < n; i++) a = (a + p[i]) % 65521u, b = (b + a) % 65521u;
    return b << 16 | a;
}

void check_frame(const Picture& P, const uint8_t* f, uint64_t len, const uint8_t* F, uint32_t N, const char* name)
{
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (memcmp(f, sig, 8)) die("signature", name);
    if (be32(f + 8) != 13 || memcmp(f + 12, "IHDR", 4) || be32(f + 16) != (uint32_t)P.w || be32(f + 20) != (uint32_t)P.h || f[24] != 8 || f[25] != 2 ||
        f[26] || f[27] || f[28] || be32(f + 29) != crc_slow(f + 12, 17))
        die("IHDR", name);
    const uint32_t n = be32(f + 33);
    if (memcmp(f + 37, "IDAT", 4) || (uint64_t)n + png::kFileFixed - 6 != len || f[41] != 0x78 || f[42] != 0x01 || (f[43] & 7) != 3) die("IDAT", name);
    if (be32(f + 41 + n) != crc_slow(f + 37, 4 + (size_t)n)) die("IDAT's CRC", name);
    if (be32(f + 41 + n - 4) != adler_slow(F, N)) die("Adler-32", name);
    const uint8_t* e = f + 45 + n;
    if (be32(e) != 0 || memcmp(e + 4, "IEND", 4) || be32(e + 8) != crc_slow(e + 4, 4) || e + 12 != f + len) die("IEND", name);
}

int g_pictures = 0;

void run(Picture& P, const char* name)
{
    const uint32_t N = png::stream_of(P.w, P.h);
    uint8_t* F = (uint8_t*)malloc(N);
    if (png::filter_host(P.px, P.w, P.h, 3 * P.w, F)) die("filter_host", name);
    for (int y = 0; y < P.h; y++)
        if (F[(size_t)y * png::pitch_of(P.w)] > 4) die("a filter type above 4", name);
    uint64_t len = 0, again = 0;
    if (png::encode_host(P.px, P.w, P.h, 3 * P.w, nullptr, 0, &len) != ICELK_ECAP || len < (uint64_t)png::kFileFixed + 2) die("length", name);
    if (len > png::bound_of(P.w, P.h)) die("above the bound", name);
    uint8_t* file = (uint8_t*)malloc(len);
    if (png::encode_host(P.px, P.w, P.h, 3 * P.w, file, len, &again) || again != len) die("encode_host", name);
    uint8_t* small = (uint8_t*)malloc(len - 1);
    memset(small, 0x5a, len - 1);
    if (png::encode_host(P.px, P.w, P.h, 3 * P.w, small, len - 1, &again) != ICELK_ECAP || again != len) die("a buffer a byte short", name);
    for (uint64_t i = 0; i + 1 < len; i++)
        if (small[i] != 0x5a) die("a refused call wrote", name);
    check_frame(P, file, len, F, N, name);
    // rows farther apart: the same file
    const int stride = 3 * P.w + 5;
    uint8_t* wide = (uint8_t*)malloc((size_t)P.h * stride);
    memset(wide, 0xee, (size_t)P.h * stride);
    for (int y = 0; y < P.h; y++) memcpy(wide + (size_t)y * stride, P.px + (size_t)y * 3 * P.w, 3 * (size_t)P.w);
    uint8_t* file2 = (uint8_t*)malloc(len);
    if (png::encode_host(wide, P.w, P.h, stride, file2, len, &again) || again != len || memcmp(file, file2, len)) die("strided rows", name);
    printf("%s: %d x %d, N %u -> %llu bytes\n", name, P.w, P.h, N, (unsigned long long)len);
    g_pictures++;
    free(file2), free(wide), free(small), free(file), free(F);
}

void noise(Picture& P)
{
    for (size_t i = 0; i < (size_t)P.h * 3 * P.w; i++) P.px[i] = (uint8_t)rnd();
}
void flat(Picture& P, int r, int g, int b)
{
    for (size_t i = 0; i < (size_t)P.h * P.w; i++) P.px[3 * i] = (uint8_t)r, P.px[3 * i + 1] = (uint8_t)g, P.px[3 * i + 2] = (uint8_t)b;
}

// ---- RFC 1951 3.2.5 read back: the symbol and the extra bits of a code as token_code made it -----------------------
struct Reader {
    uint32_t bits;
    int at;
    uint32_t take(int n)
    {
        const uint32_t v = (bits >> at) & ((1u << n) - 1u);
        at += n;
        return v;
    }
    uint32_t huff(int n)   // a Huffman code: most significant bit first
    {
        uint32_t v = 0;
        for (int k = 0; k < n; k++) v = v << 1 | take(1);
        return v;
    }
};

uint32_t read_symbol(Reader& r)
{
    uint32_t v = r.huff(7);
    if (v <= 0x17) return 256 + v;                    // 0000000 .. 0010111
    v = v << 1 | r.take(1);
    if (v >= 0x30 && v <= 0xbf) return v - 0x30;      // 00110000 .. 10111111
    if (v >= 0xc0 && v <= 0xc7) return 280 + (v - 0xc0);
    v = v << 1 | r.take(1);
    return 144 + (v - 0x190);
}

void check_codes()
{
    static const int lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const int lextra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const int dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const int dextra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    for (int v = 0; v < 256; v++) {
        const png::Code c = png::token_code((uint16_t)(png::kLiteral | v), 4);
        Reader r{c.bits, 0};
        if (read_symbol(r) != (uint32_t)v || r.at != c.n || c.n != (v < 144 ? 8 : 9) || c.bits >> c.n) die("a literal's code");
    }
    for (uint32_t pitch = 4; pitch <= 32770; pitch += 3)
        for (int sel = 0; sel < (pitch <= 32768 ? 3 : 2); sel++)   // a pitch above 32768 is no candidate: never coded
            for (int len = 3; len <= 258; len += (pitch % 97 == 4 || len < 12 || len > 250) ? 1 : 37) {
                const png::Code c = png::token_code((uint16_t)(len | sel << 9), pitch);
                Reader r{c.bits, 0};
                const uint32_t s = read_symbol(r);
                if (s < 257 || s > 285) die("a length symbol");
                const uint32_t l = lbase[s - 257] + r.take(lextra[s - 257]);
                const uint32_t ds = r.huff(5);
                if (ds > 29) die("a distance symbol");
                const uint32_t d = dbase[ds] + r.take(dextra[ds]);
                if (l != (uint32_t)len || d != png::distance_of(sel, pitch) || r.at != c.n || c.n > png::kMaxTokenBits || (c.n < 32 && c.bits >> c.n)) die("a match's code");
            }
    printf("codes: 256 literals, lengths 3 .. 258, distances 1 .. 32768\n");
}

void check_adler()
{
    std::vector<uint8_t> v(3 * png::kSegment + 1234);
    for (auto& b : v) b = (uint8_t)(rnd() | 0x80);
    for (uint32_t piece : {1u, 7u, 4095u, 4096u}) {
        png::Adler sum{0, 0, 0};
        for (size_t s = 0; s < v.size(); s += piece) {
            const size_t end = s + piece < v.size() ? s + piece : v.size();
            uint32_t A = 0, B = 0;
            for (size_t i = s; i < end; i++) A += v[i], B += (uint32_t)(end - i) * v[i];
            sum = png::adler_join(sum, png::adler_piece(A, B, (uint32_t)(end - s)));
        }
        if (png::adler_value(sum) != adler_slow(v.data(), v.size())) die("Adler-32 by pieces");
    }
    std::vector<uint8_t> ff(png::kSegment, 0xff);   // the largest raw sums a piece can have
    uint32_t A = 0, B = 0;
    for (int i = 0; i < png::kSegment; i++) A += 0xff, B += (uint32_t)(png::kSegment - i) * 0xff;
    if (png::adler_value(png::adler_piece(A, B, png::kSegment)) != adler_slow(ff.data(), ff.size())) die("a piece of FF bytes");
    printf("adler: pieces of 1, 7, 4095, 4096 bytes\n");
}

}  // namespace

int main()
{
    {
        Picture a(1, 1), b(1, 7), c(7, 1);
        noise(a), noise(b), noise(c);
        run(a, "1 x 1"), run(b, "1 x 7"), run(c, "7 x 1");
    }
    {
        Picture z(512, 64), k(512, 64);
        flat(z, 0, 0, 0), flat(k, 17, 200, 93);
        run(z, "zero"), run(k, "one colour");
    }
    {
        Picture n(64, 48);
        noise(n);
        run(n, "noise");
    }
    {
        Picture hr(101, 37), vr(37, 101), ck(47, 33);
        for (int y = 0; y < hr.h; y++)
            for (int x = 0; x < 3 * hr.w; x++) hr.at(y, x) = (uint8_t)((x / 3) * (1 + x % 3) + 50 * (x % 3));
        for (int y = 0; y < vr.h; y++)
            for (int x = 0; x < 3 * vr.w; x++) vr.at(y, x) = (uint8_t)(y * (1 + x % 3) + 50 * (x % 3));
        for (int y = 0; y < ck.h; y++)
            for (int x = 0; x < 3 * ck.w; x++) ck.at(y, x) = (uint8_t)(((y / 2 + x / 6) & 1) ? 200 - 70 * (x % 3) : 20 + 110 * (x % 3));
        run(hr, "horizontal ramp"), run(vr, "vertical ramp"), run(ck, "checkerboard");
    }
    for (int length : {2, 3, 257, 258, 259, 516}) {
        Picture r(200, 1);
        for (int x = 0; x < 600; x++) r.at(0, x) = x % 2 ? 226 : 30;
        for (int x = 31; x < 31 + length; x++) r.at(0, x) = 0;
        char name[32];
        snprintf(name, sizeof name, "zero run %d", length);
        run(r, name);
    }
    {
        Picture a(85, 16), b(30, 45), c(80, 17), d(85, 32), e(1366, 5);
        noise(a), noise(b), noise(c);
        flat(d, 9, 9, 200);
        for (int y = 0; y < e.h; y++)
            for (int x = 0; x < 3 * e.w; x++) e.at(y, x) = (uint8_t)(x / 3);
        run(a, "N = segment"), run(b, "N = segment - 1"), run(c, "N = segment + 1"), run(d, "N = 2 segments"), run(e, "rows straddle segments");
    }
    for (int w : {10922, 10923}) {
        Picture p(w, 2);
        int sum[3] = {0, 0, 0};
        for (int x = 0; x < 3 * w; x++) {
            const int r = (int)(rnd() % 8 + 1) * (rnd() & 1 ? 1 : -1);
            sum[x % 3] += r;
            p.at(0, x) = (uint8_t)sum[x % 3], p.at(1, x) = (uint8_t)(sum[x % 3] + 100);
        }
        run(p, w == 10922 ? "pitch 32767" : "pitch 32770");
    }
    {   // the limits
        uint8_t px[3] = {1, 2, 3};
        uint64_t len = 0;
        if (png::size_ok(0, 1) || png::size_ok(1, 0) || png::size_ok(16385, 1) || png::size_ok(1, 16385) || png::size_ok(16384, 5462) || !png::size_ok(16384, 5461) ||
            !png::size_ok(16384, 1) || !png::size_ok(1, 16384))
            die("size_ok");
        if (png::encode_host(px, 0, 1, 3, nullptr, 0, &len) != ICELK_EARG || png::encode_host(px, 1, 1, 2, nullptr, 0, &len) != ICELK_EARG ||
            png::encode_host(nullptr, 1, 1, 3, nullptr, 0, &len) != ICELK_EARG || png::encode_host(px, 1, 1, 3, nullptr, 0, nullptr) != ICELK_EARG ||
            png::filter_host(px, 1, 1, 3, nullptr) != ICELK_EARG)
            die("a refusal");
        if (png::bound_of(16384, 5461) != 63 + ((uint64_t)9 * 5461 * 49153 + 10 + 7) / 8) die("the bound");
        Picture tall(1, 16384), wide(16384, 1);
        noise(tall), noise(wide);
        run(tall, "1 x 16384"), run(wide, "16384 x 1");
    }
    check_codes();
    check_adler();
    printf("%d pictures\ndone\n", g_pictures);
    return 0;
}
