// jpeg_enc_host_main.cpp -- the host statement of the JPEG writer (csrc/jpeg_enc_host.h, which walks the scan with
// csrc/jpeg_enc.h, the code of the device kernels) as a program of its own under the host's sanitizers
// (test_jpeg_encode_sanitizers_host.py builds and runs it; nothing of the library is linked).
//
//   jpeg_enc_host_main BLOB...
//
// A blob is four int32 (width, height, stride in bytes, quality) and height * stride bytes of interleaved R G B, as for
// jpeg_resave_host_main.  The coefficients, the header and the file are heap allocations of exactly the size the calls
// report, so a read or a store outside them is AddressSanitizer's to find; the file goes to BLOB.jpg with the comment
// "blob" (the test compares it with the library's and with Pillow's).  Then the longest blocks the tables can code -- all
// AC coefficients at +-1023, DC differences of +-2047 -- are written into a buffer of exactly their size, and a
// coefficient without a code is refused.  Every file is also put together again by the assembler the library's finish calls
// use (enc::file_into: header, a scan from host memory, EOI), from a scan of exactly its size into a buffer of exactly the
// file's length, and into one a byte short of it, which must be refused with the length.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../iceberg_tracking_code_amd/csrc/jpeg_resave_host.h"
#include "../iceberg_tracking_code_amd/csrc/jpeg_enc_host.h"

#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

[[noreturn]] void die(const char* what, const char* arg = "")
{
    fprintf(stderr, "jpeg_enc_host_main: %s %s\n", what, arg);
    exit(2);
}

const uint8_t kComment[] = {'b', 'l', 'o', 'b'};

int assembled = 0;

// `file` (its header takes hlen bytes) once more, from its scan alone
void assemble_again(const icelk_jpeg_info_t& info, const std::vector<uint8_t>& file, uint64_t hlen, const char* what)
{
    const std::vector<uint8_t> scan(file.begin() + (size_t)hlen, file.end() - 2);
    if (icelk::enc::file_len(info, kComment, sizeof(kComment), scan.size()) != file.size()) die("assembler: length", what);
    uint64_t len = 0;
    std::vector<uint8_t> shorter(file.size() - 1, 0xAA), exact(file.size());
    if (icelk::enc::file_into(info, kComment, sizeof(kComment), scan.data(), scan.size(), shorter.data(), shorter.size(), &len) != ICELK_ECAP ||
        len != file.size())
        die("assembler: capacity not checked", what);
    for (uint8_t b : shorter)
        if (b != 0xAA) die("assembler: wrote into a buffer it refused", what);
    len = 0;
    if (icelk::enc::file_into(info, kComment, sizeof(kComment), scan.data(), scan.size(), nullptr, file.size(), &len) != ICELK_ECAP || len != file.size())
        die("assembler: null buffer taken", what);
    len = 0;
    if (icelk::enc::file_into(info, kComment, sizeof(kComment), scan.data(), scan.size(), exact.data(), exact.size(), &len) != ICELK_OK ||
        len != file.size() || exact != file)
        die("assembler: file", what);
    assembled++;
}

// the file of (info, coef) in a buffer of exactly its size; every smaller capacity is refused with the size
std::vector<uint8_t> file_of(const icelk_jpeg_info_t& info, const std::vector<int16_t>& coef, const char* what)
{
    uint64_t len = 0, again = 0;
    if (icelk::enc::encode_host(&info, coef.data(), kComment, sizeof(kComment), nullptr, 0, &len) != ICELK_ECAP || len == 0) die("size", what);
    std::vector<uint8_t> out((size_t)len);
    if (icelk::enc::encode_host(&info, coef.data(), kComment, sizeof(kComment), out.data(), len - 1, &again) != ICELK_ECAP || again != len)
        die("capacity not checked", what);
    if (icelk::enc::encode_host(&info, coef.data(), kComment, sizeof(kComment), out.data(), len, &again) != ICELK_OK || again != len)
        die("file", what);
    uint64_t hlen = 0;
    if (icelk::enc::header_host(&info, kComment, sizeof(kComment), nullptr, 0, &hlen) != ICELK_ECAP || hlen == 0 || hlen >= len) die("header size", what);
    std::vector<uint8_t> head((size_t)hlen);
    if (icelk::enc::header_host(&info, kComment, sizeof(kComment), head.data(), hlen, &again) != ICELK_OK || again != hlen) die("header", what);
    if (memcmp(head.data(), out.data(), (size_t)hlen)) die("header differs from the file's", what);
    assemble_again(info, out, hlen, what);
    return out;
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
    std::vector<int16_t> coef((size_t)info.coef_count);
    if (icelk::resave::coefficients_host(rgb.data(), w, h, stride, quality, &info, coef.data(), coef.size()) != ICELK_OK) die("coefficients", path);
    const std::vector<uint8_t> out = file_of(info, coef, path);
    const std::string name = std::string(path) + ".jpg";
    FILE* g = fopen(name.c_str(), "wb");
    if (!g || fwrite(out.data(), 1, out.size(), g) != out.size()) die("cannot write", name.c_str());
    fclose(g);
    printf("%s: %d x %d quality %d, %zu bytes\n", path, w, h, quality, out.size());
}

void extremes()
{
    icelk_jpeg_info_t info;
    icelk::resave::resave_info(40, 24, 100, &info);
    std::vector<int16_t> coef((size_t)info.coef_count);
    for (size_t i = 0; i < coef.size(); i++) {
        const size_t blk = i / 64, k = i % 64;
        coef[i] = k == 0 ? (blk % 2 ? 1023 : -1024) : (int16_t)((k + blk) % 2 ? 1023 : -1023);
    }
    const std::vector<uint8_t> out = file_of(info, coef, "extremes");
    printf("extremes: %zu bytes\n", out.size());
    uint64_t len = 0;
    std::vector<uint8_t> buf(out.size());
    coef[coef.size() - 1] = 1024;
    if (icelk::enc::encode_host(&info, coef.data(), nullptr, 0, buf.data(), buf.size(), &len) != ICELK_EARG) die("AC 1024 taken");
    coef[coef.size() - 1] = -32768;
    if (icelk::enc::encode_host(&info, coef.data(), nullptr, 0, buf.data(), buf.size(), &len) != ICELK_EARG) die("AC -32768 taken");
    coef[coef.size() - 1] = 0;
    coef[0] = 32767;
    coef[64] = -32768;
    if (icelk::enc::encode_host(&info, coef.data(), nullptr, 0, buf.data(), buf.size(), &len) != ICELK_EARG) die("DC difference 65535 taken");
    info.restart_interval = 4;
    if (icelk::enc::encode_host(&info, coef.data(), nullptr, 0, buf.data(), buf.size(), &len) != ICELK_EUNSUP) die("restart interval taken");
}

}  // namespace

int main(int argc, char** argv)
{
    for (int i = 1; i < argc; i++) run(argv[i]);
    extremes();
    printf("assembled: %d of %d\n", assembled, argc);
    printf("done\n");
    return 0;
}
