// jpeg_enc_budget_main.cpp -- the budgeted chain of a crop job (csrc/jpeg_enc_host.h: encode_budgeted_host, which takes
// every decision with the functions of csrc/jpeg_enc.h that the device-sized kernels of k_jpeg_enc.hip take them with) as a
// program of its own under the host's sanitizers (test_jpeg_crop_sanitizers_host.py builds and runs it; nothing of the
// library is linked).
//
// The chain runs in the kernels' order -- count, scan, pack, ff, scan, stuff, verdict -- with `packed` and `out` as heap
// allocations of exactly cap = bytes per block x blocks bytes, so a read or a store outside the capacity is
// AddressSanitizer's to find.  Per image:
//   fits        the least bytes per block that hold the stuffed scan: the scan must equal encode_host's, byte for byte
//   over        one byte per block less (where its capacity is below the scan): the verdict is "over budget", stuff stores nothing
//   packed fits but stuffed does not: every bytes-per-block value between the two sizes -- pack stores, stuff does not
//   arbitrary control words: each of the three words forced to edge values and pseudo-random ones, alone and together
// and a coefficient without a code (JE_INVALID): pack and stuff store nothing.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../iceberg_tracking_code_amd/csrc/jpeg_resave_host.h"
#include "../iceberg_tracking_code_amd/csrc/jpeg_enc_host.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

namespace {

using namespace icelk;

[[noreturn]] void die(const char* what, const char* arg = "")
{
    fprintf(stderr, "jpeg_enc_budget_main: %s %s\n", what, arg);
    exit(2);
}

uint32_t g_rng = 12345u;
uint32_t rnd()
{
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

std::vector<uint8_t> image(const char* kind, int w, int h)
{
    static const uint8_t colours[6][3] = {{255, 0, 0}, {0, 255, 0}, {0, 0, 255}, {0, 255, 255}, {255, 0, 255}, {255, 255, 0}};
    std::vector<uint8_t> rgb((size_t)3 * w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            for (int c = 0; c < 3; c++) {
                uint8_t v = 0;
                if (kind[0] == 'n') v = (uint8_t)rnd();
                else if (kind[0] == 's') v = colours[((x / 8) + 2 * (y / 8)) % 6][c];
                else if (kind[0] == 'r') v = (uint8_t)((3 + 2 * c) * x + (1 + c) * y);
                rgb[((size_t)y * w + x) * 3 + c] = v;
            }
    return rgb;
}

struct Run {
    enc::BudgetWalk W;
    std::unique_ptr<uint8_t[]> packed, out;   // exactly W.cap bytes each
};

Run walk(const icelk_jpeg_info_t& info, const std::vector<int16_t>& coef, uint32_t blocks, int bpb, const uint32_t* force, uint32_t mask)
{
    Run R;
    const uint32_t cap = enc::budget_cap(blocks, bpb);
    R.packed.reset(new uint8_t[cap]);
    R.out.reset(new uint8_t[cap]);
    if (enc::encode_budgeted_host(&info, coef.data(), bpb, force, mask, R.packed.get(), R.out.get(), &R.W) != ICELK_OK) die("walk");
    if (R.W.cap != cap) die("capacity");
    return R;
}

void run(const char* kind, int w, int h, int quality)
{
    const std::vector<uint8_t> rgb = image(kind, w, h);
    icelk_jpeg_info_t info;
    if (resave::coefficients_host(rgb.data(), w, h, 3 * w, quality, &info, nullptr, 0) != ICELK_OK) die("descriptor", kind);
    std::vector<int16_t> coef((size_t)info.coef_count);
    if (resave::coefficients_host(rgb.data(), w, h, 3 * w, quality, &info, coef.data(), coef.size()) != ICELK_OK) die("coefficients", kind);
    enc::Layout L;
    if (enc::layout_of(&info, &L) != ICELK_OK) die("layout", kind);
    uint64_t len = 0, hlen = 0;
    if (enc::encode_host(&info, coef.data(), nullptr, 0, nullptr, 0, &len) != ICELK_ECAP) die("size", kind);
    std::vector<uint8_t> file((size_t)len);
    if (enc::encode_host(&info, coef.data(), nullptr, 0, file.data(), len, &len) != ICELK_OK) die("file", kind);
    if (enc::header_host(&info, nullptr, 0, nullptr, 0, &hlen) != ICELK_ECAP) die("header", kind);
    const uint32_t S = (uint32_t)(len - hlen - 2);                      // the stuffed scan
    uint32_t ff = 0;
    for (uint32_t i = 0; i + 1 < S; i++) ff += file[hlen + i] == 0xFF && file[hlen + i + 1] == 0x00;
    const uint32_t P = S - ff;                                          // the packed scan
    const int fit = (int)((S + L.blocks - 1) / L.blocks);
    if (fit > enc::kMaxBytesPerBlock) die("a block above its bound", kind);
    // fits
    {
        const Run R = walk(info, coef, L.blocks, fit, nullptr, 0);
        if (R.W.verdict != enc::kCoded || R.W.stuffed != S || R.W.ff_total != ff || enc::packed_bytes(R.W.total_bits) != P) die("fit: sizes", kind);
        if (memcmp(R.out.get(), file.data() + hlen, S)) die("fit: the scan differs from encode_host's", kind);
        if (R.W.out_stores != S) die("fit: stores", kind);
    }
    // over, at the first exit (packed does not fit) or the second
    int over_cases = 0, second_exit = 0;
    for (int bpb = fit - 1; bpb >= 1 && bpb >= fit - 3; bpb--) {
        const uint32_t cap = enc::budget_cap(L.blocks, bpb);
        if (cap >= S) continue;
        const Run R = walk(info, coef, L.blocks, bpb, nullptr, 0);
        if (R.W.verdict != enc::kOverBudget || R.W.stuffed != 0 || R.W.out_stores != 0) die("over: verdict or stores", kind);
        if (cap >= P) {
            second_exit++;
            if (R.W.packed_stores == 0) die("over: pack did not run though the packed scan fits", kind);
        } else if (R.W.packed_stores != 0) die("over: pack stored", kind);
        over_cases++;
    }
    // arbitrary control words
    const uint32_t capf = enc::budget_cap(L.blocks, fit);
    const uint32_t edges[] = {0u, 1u, 7u, 8u, 9u, P * 8u - 8u, P * 8u, P * 8u + 1u, capf * 8u, capf * 8u + 1u, capf, capf + 1u, S, ff, 0x7fffffffu,
                              0xfffffff8u, 0xffffffffu};
    int forced = 0;
    for (int bpb : {fit, fit > 1 ? fit - 1 : fit, fit + 1 <= enc::kMaxBytesPerBlock ? fit + 1 : fit})
        for (uint32_t mask = 1; mask < 8; mask++)
            for (int k = 0; k < 24; k++) {
                uint32_t f[3];
                for (int i = 0; i < 3; i++) f[i] = k < 17 ? edges[(k + 5 * i) % 17] : rnd() >> (rnd() % 24);
                if (k & 1) f[1] &= 1u;
                const Run R = walk(info, coef, L.blocks, bpb, f, mask);
                if (R.W.out_stores > R.W.cap || R.W.stuffed > R.W.cap) die("forced: more than the capacity", kind);
                if (R.W.verdict == enc::kCoded && (uint64_t)enc::packed_bytes(R.W.total_bits) + R.W.ff_total > R.W.cap) die("forced: coded beyond the capacity", kind);
                forced++;
            }
    // a coefficient without a code
    std::vector<int16_t> bad = coef;
    bad[bad.size() - 1] = 1024;
    const Run R = walk(info, bad, L.blocks, enc::kMaxBytesPerBlock, nullptr, 0);
    if (R.W.verdict != enc::kInvalid || R.W.packed_stores != 0 || R.W.out_stores != 0 || R.W.stuffed != 0) die("invalid: verdict or stores", kind);
    printf("%s %d x %d quality %d: %u blocks, packed %u, stuffed %u, %d per block; over %d (behind the FF count %d), forced %d\n", kind, w, h, quality,
           L.blocks, P, S, fit, over_cases, second_exit, forced);
}

}  // namespace

int main()
{
    run("zeros", 3, 3, 100);          // 6 blocks, a scan of a few bytes
    run("noise", 3, 3, 100);
    run("stripes", 200, 9, 95);       // 78 blocks: 13 bytes per block hold the packed scan and not the stuffed one
    run("noise", 176, 16, 100);       // 66 blocks, two past a workgroup of count and pack
    run("noise", 176, 16, 1);
    run("ramp", 99, 131, 75);
    run("noise", 250, 333, 100);      // 672 x 84 bytes: several workgroups of ff and stuff
    run("stripes", 640, 480, 95);
    printf("done\n");
    return 0;
}
