// jpeg_resave_host_main.cpp -- the host statement of the re-save's forward half (csrc/jpeg_resave_host.h, which runs
// csrc/jpeg_fwd.h, the code of the device kernel) as a program of its own under the host's sanitizers
// (test_jpeg_resave_sanitizers_host.py builds and runs it; nothing of the library is linked).
//
//   jpeg_resave_host_main BLOB...
//
// A blob is four int32 (width, height, stride in bytes, quality) and height * stride bytes of interleaved R G B.  The
// pixels and the coefficients are heap allocations of exactly the size the call is told, so a read or a store outside
// them is AddressSanitizer's to find, and the integer arithmetic is UndefinedBehaviorSanitizer's.  The coefficients go to
// BLOB.coef (the test compares them with the library's and with Pillow's file).  Then the quantiser's multiply-shift is
// compared with division for every table entry and every numerator up to 2^17.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../iceberg_tracking_code_amd/csrc/jpeg_resave_host.h"

#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

[[noreturn]] void die(const char* what, const char* arg = "")
{
    fprintf(stderr, "jpeg_resave_host_main: %s %s\n", what, arg);
    exit(2);
}

void run(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) die("cannot open", path);
    int32_t head[4];
    if (fread(head, sizeof(head), 1, f) != 1) die("short blob", path);
    const int w = head[0], h = head[1], stride = head[2], quality = head[3];
    const size_t bytes = (size_t)h * stride;
    std::vector<uint8_t> rgb(bytes);
    if (fread(rgb.data(), 1, bytes, f) != bytes) die("short blob", path);
    fclose(f);
    icelk_jpeg_info_t info;
    if (icelk::resave::coefficients_host(rgb.data(), w, h, stride, quality, &info, nullptr, 0) != ICELK_OK) die("descriptor", path);
    std::vector<int16_t> coef((size_t)info.coef_count, (int16_t)0x7777);
    if (icelk::resave::coefficients_host(rgb.data(), w, h, stride, quality, &info, coef.data(), coef.size()) != ICELK_OK) die("coefficients", path);
    if (coef.size() > 1 && icelk::resave::coefficients_host(rgb.data(), w, h, stride, quality, &info, coef.data(), coef.size() - 1) != ICELK_ECAP)
        die("capacity not checked", path);
    const std::string out = std::string(path) + ".coef";
    FILE* g = fopen(out.c_str(), "wb");
    if (!g || fwrite(coef.data(), sizeof(int16_t), coef.size(), g) != coef.size()) die("cannot write", out.c_str());
    fclose(g);
    printf("%s: %d x %d quality %d, %llu coefficients\n", path, w, h, quality, (unsigned long long)info.coef_count);
}

}  // namespace

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; i++) run(argv[i]);
    unsigned long long checked = 0;
    for (uint32_t q = 1; q <= 255; q++) {
        const uint32_t qv = q << 3, m = icelk::fwd::reciprocal(qv);
        for (uint32_t n = 0; n <= (1u << 17); n++, checked++)
            if (icelk::fwd::divide(n, m) != n / qv) die("multiply-shift differs from division");
    }
    printf("divisions checked: %llu\n", checked);
    return 0;
}
