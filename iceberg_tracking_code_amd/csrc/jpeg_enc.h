// jpeg_enc.h -- the entropy coder of a baseline JPEG file (ITU-T T.81 F.1.2) as plain C++ for the host and the device
// alike: quantised coefficients in the layout of icelk_jpeg_info_t -> the bits of the interleaved scan, coded with the
// four "typical" Huffman tables of T.81 Annex K.3, the ones libjpeg (so Pillow's `img.save` without optimize=True) puts
// into every file.  The file is a pure function of the coefficients, so the re-saved crop of the reference
// (camtools.py:64-104) can be written from the coefficients k_jpeg_fwd leaves on the device.  The host statement
// (jpeg_enc_host.h, exported by abi_jpeg_enc.hip) and the device kernels (k_jpeg_enc.hip) both run the functions below.
//
//   tables    BITS / HUFFVAL of tables K.3 - K.6; the codes follow by Annex C (build_codes): (code << 8 | length) per
//             symbol, 0 where the table has no code
//   layout    where the s-th block of the interleaved scan lies in the coefficient planes, and where the block lies whose
//             DC it is predicted from (place): 1 component, or 3 with luma 1x1, 2x1 or 2x2 over chroma 1x1
//   a block   DC difference, then (run, size) symbols with ZRL for runs above 15 and EOB unless coefficient 63 is non-zero
//             (encode_block), into a sink: one that adds up lengths (CountSink), or one that places bits
//   bounds    a block is at most 22 + 63 * 26 = 1660 bits (kMaxBlockBits): a count fits 16 bits.  A DC difference of
//             category above 11 and an AC value of category above 10 have no code: encode_block says so and codes a
//             harmless stand-in, so that both passes over a block always agree on its length
// No restart intervals: the re-save has none.
#pragma once
#include <stdint.h>

#define ICELK_ENC_FN __host__ __device__ __forceinline__

namespace icelk {
namespace enc {

constexpr int kMaxBlockBits = 22 + 63 * 26;
constexpr int kMaxPutBits = 26;   // the longest code with its value bits: AC, 16 + 10

// natural (row-major) index of the k-th coefficient in zigzag order (T.81 Figure A.6)
#define ICELK_ENC_ZIGZAG                                                                                                              \
    {                                                                                                                                 \
        0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, \
            49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63    \
    }

// ---- T.81 Annex K.3: tables K.3 (DC luminance), K.4 (DC chrominance), K.5 (AC luminance), K.6 (AC chrominance) -------
struct HuffSpec {
    uint8_t bits[16];    // codes of length 1 .. 16
    int nval;
    uint8_t val[162];    // the symbols by increasing code length
};
static const HuffSpec kSpec[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
     162,
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
      0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
      0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
      0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
      0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
      0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
      0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
      0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
     162,
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
      0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
      0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
      0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
      0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
      0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
      0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
      0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}},
};
enum { SPEC_DC0 = 0, SPEC_DC1 = 1, SPEC_AC0 = 2, SPEC_AC1 = 3 };

// The tables as the coder looks symbols up: code << 8 | length, 0: the table has no code for the symbol.  Table 0 is
// luminance, 1 chrominance.  2176 bytes: the device kernels stage them in LDS.
struct Codes {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
constexpr int kCodeWords = sizeof(Codes) / sizeof(uint32_t);

// T.81 Annex C: Generate_size_table, Generate_code_table, Order_codes in one walk
inline void build_codes(Codes* C)
{
    for (int t = 0; t < 2; t++) {
        for (int i = 0; i < 16; i++) C->dc[t][i] = 0;
        for (int i = 0; i < 256; i++) C->ac[t][i] = 0;
    }
    for (int t = 0; t < 4; t++) {
        const HuffSpec& S = kSpec[t];
        uint32_t* dst = t < 2 ? C->dc[t] : C->ac[t - 2];
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; len++) {
            for (int i = 0; i < S.bits[len - 1]; i++, k++, code++) dst[S.val[k]] = code << 8 | (uint32_t)len;
            code <<= 1;
        }
    }
}

// ---- where the blocks of the scan lie -----------------------------------------------------------------------------------
struct Layout {
    int32_t ncomp, hs, vs;      // hs x vs luma blocks per MCU (1 x 1 for one component), then one block per further component
    int32_t mcus_x;
    uint32_t bpm, blocks;       // blocks per MCU, blocks of the scan
    uint32_t luma_bx;           // blocks per row of the luma plane; a chroma plane has mcus_x
    uint32_t off0, off1, off2;  // first coefficient of every component (three names: no lane-indexed array in a kernel argument)
};
struct Place {
    uint32_t at;      // index of the block's first coefficient
    uint32_t pred;    // ... of the block whose DC is the prediction; kNoPred: the prediction is 0
    int table;        // 0 luminance, 1 chrominance
};
constexpr uint32_t kNoPred = 0xffffffffu;

ICELK_ENC_FN uint32_t luma_at(const Layout& L, uint32_t m, int j)
{
    const uint32_t my = m / (uint32_t)L.mcus_x, mx = m - my * (uint32_t)L.mcus_x;
    const uint32_t v = (uint32_t)j / (uint32_t)L.hs, u = (uint32_t)j - v * (uint32_t)L.hs;
    return L.off0 + ((my * (uint32_t)L.vs + v) * L.luma_bx + mx * (uint32_t)L.hs + u) * 64u;
}

// s < L.blocks
ICELK_ENC_FN Place place(const Layout& L, uint32_t s)
{
    Place P;
    const uint32_t m = s / L.bpm;
    const int j = (int)(s - m * L.bpm), nl = L.hs * L.vs;
    if (j < nl) {
        P.table = 0;
        P.at = luma_at(L, m, j);
        P.pred = j > 0 ? luma_at(L, m, j - 1) : (m > 0 ? luma_at(L, m - 1, nl - 1) : kNoPred);
    } else {
        P.table = 1;
        P.at = (j == nl ? L.off1 : L.off2) + m * 64u;
        P.pred = m > 0 ? P.at - 64u : kNoPred;
    }
    return P;
}

// ---- one block ---------------------------------------------------------------------------------------------------------
ICELK_ENC_FN int category(int v)   // SSSS of T.81 tables F.1 / F.2: the bits of |v|
{
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}
ICELK_ENC_FN uint32_t value_bits(int v, int s) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u); }

struct CountSink {
    uint32_t bits = 0;
    ICELK_ENC_FN void put(uint32_t, int n) { bits += (uint32_t)n; }
};

// get(k): the block's coefficient number k in zigzag order; pred: the DC of the block before it in its component;
// dc / ac: one table of Codes each.  Every put has 1 .. kMaxPutBits bits.  false: a coefficient has no code.
template <class Get, class Sink>
ICELK_ENC_FN bool encode_block(Get get, int pred, const uint32_t* dc, const uint32_t* ac, Sink& out)
{
    bool ok = true;
    int diff = get(0) - pred;
    int s = category(diff);
    if (s > 11) {
        ok = false;
        diff = 0;
        s = 0;
    }
    uint32_t e = dc[s];
    out.put((e >> 8) << s | value_bits(diff, s), (int)(e & 255u) + s);
    const uint32_t zrl = ac[0xF0], eob = ac[0x00];
    int run = 0;
#pragma unroll 1
    for (int k = 1; k < 64; k++) {
        int v = get(k);
        if (v == 0) {
            run++;
            continue;
        }
        for (; run > 15; run -= 16) out.put(zrl >> 8, (int)(zrl & 255u));
        s = category(v);
        if (s > 10) {
            ok = false;
            v = 1;
            s = 1;
        }
        e = ac[run << 4 | s];
        out.put((e >> 8) << s | value_bits(v, s), (int)(e & 255u) + s);
        run = 0;
    }
    if (run) out.put(eob >> 8, (int)(eob & 255u));
    return ok;
}

// ---- the budget of a scan whose sizes stay on the device (jobs with a file: abi_jpeg_job.hip) ----------------------------
// Such a job may take `cap` = bytes per block x blocks bytes for the stuffed scan; the packed and the stuffed stream are
// allocated to that before anything is enqueued, and the kernels read the sizes the count and the scans left in the
// control words.  Every decision they take on those words is one of the functions below, which the host walk
// (jpeg_enc_host.h: encode_budgeted_host) takes too.
constexpr int kChunkBytes = 64;          // bytes of the packed stream one lane of ff / stuff takes
constexpr int kChunksPerGroup = 256;     // lanes of a workgroup of ff / stuff: 16 KiB of the packed stream
constexpr int kMinBytesPerBlock = 1, kMaxBytesPerBlock = 2 * ((kMaxBlockBits + 7) / 8);   // 416: every byte of a block stuffed
constexpr int kDefaultBytesPerBlock = 48;
enum Verdict : uint32_t { kNotAsked = 0, kCoded = 1, kOverBudget = 2, kInvalid = 3 };

// blocks * kMaxBlockBits < 2^32 (layout_of) and bytes_per_block <= 416: below 2^31
ICELK_ENC_FN uint32_t budget_cap(uint32_t blocks, int bytes_per_block) { return blocks * (uint32_t)bytes_per_block; }
ICELK_ENC_FN uint32_t packed_bytes(uint32_t bits) { return (uint32_t)(((uint64_t)bits + 7u) >> 3); }
ICELK_ENC_FN uint32_t chunks_of(uint32_t bytes) { return (uint32_t)(((uint64_t)bytes + (kChunkBytes - 1)) / kChunkBytes); }
ICELK_ENC_FN uint32_t groups_of(uint32_t chunks) { return (chunks + (kChunksPerGroup - 1)) / kChunksPerGroup; }
// pack runs: every coefficient has a code and the packed stream is inside the capacity
ICELK_ENC_FN bool packed_fits(uint32_t total_bits, uint32_t invalid, uint32_t cap) { return !invalid && packed_bytes(total_bits) <= cap; }
// bytes of the packed stream that ff and stuff walk: none of a stream that pack did not write
ICELK_ENC_FN uint32_t live_bytes(uint32_t total_bits, uint32_t invalid, uint32_t cap)
{
    return packed_fits(total_bits, invalid, cap) ? packed_bytes(total_bits) : 0u;
}
// stuff runs: the stream with its stuffed bytes is inside the capacity
ICELK_ENC_FN bool stuffed_fits(uint32_t total_bits, uint32_t invalid, uint32_t ff_total, uint32_t cap)
{
    return packed_fits(total_bits, invalid, cap) && (uint64_t)packed_bytes(total_bits) + ff_total <= cap;
}
// the stretch of bits that ends at `end_bits` lies in the first `cap` bytes (pack: per workgroup)
ICELK_ENC_FN bool stretch_inside(uint32_t start_bits, uint32_t end_bits, uint32_t cap) { return end_bits >= start_bits && packed_bytes(end_bits) <= cap; }
// `n` output bytes from `at` on lie in the first `cap` bytes (stuff: per lane)
ICELK_ENC_FN bool bytes_inside(uint64_t at, uint32_t n, uint32_t cap) { return at + n <= cap; }
ICELK_ENC_FN uint32_t budget_verdict(uint32_t total_bits, uint32_t invalid, uint32_t ff_total, uint32_t cap)
{
    return invalid ? (uint32_t)kInvalid : (stuffed_fits(total_bits, 0, ff_total, cap) ? (uint32_t)kCoded : (uint32_t)kOverBudget);
}

}  // namespace enc
}  // namespace icelk
