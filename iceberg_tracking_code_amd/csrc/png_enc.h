// png_enc.h -- the arithmetic of the PNG writer as plain C++ for the host and the device alike: an 8-bit R G B picture ->
// the file the reference's `plt.savefig(...png)` stands for (s3:630-637), with the pixels exact.  The host statement
// (png_enc_host.h, exported by abi_png.hip) and the kernels (k_png.hip) both run the functions below; nothing there decides
// a byte on its own.
//
//   file      signature, IHDR (8 bits, colour type 2, no interlace), one IDAT, IEND.  IDAT holds a zlib stream: 78 01, ONE
//             fixed-Huffman deflate block (BFINAL = 1, BTYPE = 01), the Adler-32 of the filtered bytes, big-endian
//   filters   row y -> 1 + 3 W bytes: the type, then the filtered row (PNG 1.2 section 6, bpp = 3, the row above row 0 is
//             zeros).  All five types are computed; the one with the smallest sum of the bytes' absolute values taken as
//             signed 8-bit is kept, ties to the lowest type (filter_value, abs8).  The filtered stream F has
//             N = H (1 + 3 W) bytes
//   tokens    F is cut into segments of kSegment = 4096 bytes, each parsed greedily from its first byte: at a position the
//             longest match among the distances 1, 3 and 1 + 3 W (the byte before, the pixel before, the row above), a
//             distance counting only if it is <= 32768 and <= the position; lengths 3 .. 258, cut at the segment's end and
//             at N; a match may reach back across segment starts; ties go to the smallest distance (best_of); no match of
//             3 or more: a literal.  No lazy matching, no hash search
//   bits      the fixed codes of RFC 1951 3.2.6, most significant bit first into the LSB-first stream, extra bits plain
//             (token_code): a token is at most 31 bits.  The stream is the 3 header bits, the segments' tokens, the 7-bit
//             end-of-block (all zero), zero padding to a byte
//   checksum  Adler-32 by pieces of kSegment bytes: a piece's (A, B) = (sum d_i, sum (n - i) d_i) fit 32 bits
//             (255 * 4096 * 4097 / 2 < 2^31), pieces compose with adler_join; CRC-32 by table, on the host
//   limits    1 <= W, H <= 16384 and N <= 2^28: 3 + 9 N + 7 bits fit 32 bits (size_ok)
#pragma once
#include <stddef.h>
#include <stdint.h>

#define ICELK_PNG_FN __host__ __device__ __forceinline__

namespace icelk {
namespace png {

constexpr int kSegment = 4096;          // bytes of F per greedy parse (and per Adler piece)
constexpr int kMaxSide = 16384;
constexpr uint64_t kMaxStream = (uint64_t)1 << 28;   // N at most
constexpr int kMinMatch = 3, kMaxMatch = 258, kMaxDistance = 32768;
constexpr int kCandidates = 3;          // distances tried: 1, 3, the row pitch
constexpr int kHeaderBits = 3, kEndBits = 7;
constexpr uint32_t kHeaderValue = 3;    // BFINAL = 1, then BTYPE = 01 LSB first
constexpr int kMaxTokenBits = 31;       // 8 + 5 + 5 + 13
constexpr uint32_t kAdlerMod = 65521;
constexpr int kFileFixed = 8 + 25 + 12 + 2 + 4 + 12;   // signature, IHDR, IDAT's frame, zlib header, Adler-32, IEND
constexpr int kStreamAt = 8 + 25 + 8 + 2;               // where the deflate bytes begin in the file

ICELK_PNG_FN bool size_ok(int w, int h)
{
    return w >= 1 && h >= 1 && w <= kMaxSide && h <= kMaxSide && (uint64_t)h * (1 + 3 * (uint64_t)w) <= kMaxStream;
}
ICELK_PNG_FN uint32_t pitch_of(int w) { return 1u + 3u * (uint32_t)w; }
ICELK_PNG_FN uint32_t stream_of(int w, int h) { return (uint32_t)h * pitch_of(w); }   // N; size_ok
ICELK_PNG_FN uint32_t segments_of(uint32_t n) { return (n + kSegment - 1) / kSegment; }
ICELK_PNG_FN uint32_t deflate_bytes(uint32_t token_bits) { return (uint32_t)(((uint64_t)token_bits + kHeaderBits + kEndBits + 7) / 8); }
// the largest file: every byte a 9-bit literal
ICELK_PNG_FN uint64_t bound_of(int w, int h) { return (uint64_t)kFileFixed + deflate_bytes(9u * stream_of(w, h)); }

// ---- row filters ----------------------------------------------------------------------------------------------------
ICELK_PNG_FN int paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
}
// x: the byte; a: the byte 3 to its left, b: the byte above, c: the byte above a (0 outside the picture)
ICELK_PNG_FN uint8_t filter_value(int type, int x, int a, int b, int c)
{
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (uint8_t)(x - pred);
}
ICELK_PNG_FN uint32_t abs8(uint8_t v) { return v < 128 ? v : 256u - v; }
// the type of the smallest sum, ties to the lowest
ICELK_PNG_FN int pick_filter(const uint32_t (&sum)[5])
{
    int best = 0;
    for (int t = 1; t < 5; t++)
        if (sum[t] < sum[best]) best = t;
    return best;
}

// ---- tokens ---------------------------------------------------------------------------------------------------------
// 16 bits per position of F: 0 no token begins here; kLiteral | byte; or length | selector << 9 (0: distance 1, 1: 3,
// 2: the pitch)
constexpr uint16_t kLiteral = 0x8000;
ICELK_PNG_FN uint32_t distance_of(int sel, uint32_t pitch) { return sel == 0 ? 1u : sel == 1 ? 3u : pitch; }
ICELK_PNG_FN bool distance_ok(uint32_t d, uint32_t pos) { return d <= (uint32_t)kMaxDistance && d <= pos; }
// run[k]: how many bytes from the position on equal the byte `distance k` before them (0 for a distance that does not
// count), already cut at the segment's end and at N.  The token that begins at the position, `byte` being F there
ICELK_PNG_FN uint16_t best_of(const uint32_t (&run)[kCandidates], uint8_t byte)
{
    uint32_t len = 0;
    int sel = 0;
    for (int k = 0; k < kCandidates; k++) {
        const uint32_t l = run[k] < (uint32_t)kMaxMatch ? run[k] : (uint32_t)kMaxMatch;
        if (l > len) len = l, sel = k;
    }
    return len >= (uint32_t)kMinMatch ? (uint16_t)(len | (uint32_t)sel << 9) : (uint16_t)(kLiteral | byte);
}
ICELK_PNG_FN uint32_t token_advance(uint16_t t) { return t & kLiteral ? 1u : (uint32_t)(t & 511u); }

// ---- the fixed codes ------------------------------------------------------------------------------------------------
ICELK_PNG_FN uint32_t reverse_bits(uint32_t v, int n)
{
    uint32_t r = 0;
    for (int k = 0; k < n; k++) r |= ((v >> k) & 1u) << (n - 1 - k);
    return r;
}
ICELK_PNG_FN int top_bit(uint32_t v)   // v >= 1
{
    int m = 0;
    while (v >> (m + 1)) m++;
    return m;
}
struct Code {
    uint32_t bits;   // as they go into the LSB-first stream
    int n;
};
// a literal / length symbol 0 .. 287
ICELK_PNG_FN Code symbol_code(uint32_t s)
{
    if (s < 144) return Code{reverse_bits(0x30u + s, 8), 8};
    if (s < 256) return Code{reverse_bits(0x190u + (s - 144), 9), 9};
    if (s < 280) return Code{reverse_bits(s - 256, 7), 7};
    return Code{reverse_bits(0xc0u + (s - 280), 8), 8};
}
ICELK_PNG_FN Code token_code(uint16_t t, uint32_t pitch)
{
    if (t & kLiteral) return symbol_code(t & 255u);
    const uint32_t len = t & 511u, l = len - kMinMatch;
    uint32_t sym, extra = 0;
    int ne = 0;
    if (len == (uint32_t)kMaxMatch)
        sym = 285;
    else if (l < 4)
        sym = 257 + l;
    else {
        ne = top_bit(l) - 2;
        sym = 261 + 4 * (uint32_t)ne + ((l >> ne) & 3u);
        extra = l & ((1u << ne) - 1u);
    }
    Code c = symbol_code(sym);
    c.bits |= extra << c.n;
    c.n += ne;
    const uint32_t x = distance_of(t >> 9, pitch) - 1;
    uint32_t dsym = x, dextra = 0;
    int nd = 0;
    if (x >= 4) {
        const int m = top_bit(x);
        nd = m - 1;
        dsym = 2 * (uint32_t)m + ((x >> nd) & 1u);
        dextra = x & ((1u << nd) - 1u);
    }
    c.bits |= reverse_bits(dsym, 5) << c.n;
    c.n += 5;
    c.bits |= dextra << c.n;
    c.n += nd;
    return c;
}

// ---- Adler-32 -------------------------------------------------------------------------------------------------------
// A stretch of n bytes acts on the running (a, b) as a += A, b += n a + B.  Of two stretches in a row:
struct Adler {
    uint32_t A, B, n;   // all below kAdlerMod
};
ICELK_PNG_FN Adler adler_piece(uint32_t sum, uint32_t weighted, uint32_t n)   // n <= kSegment: the raw sums fit
{
    return Adler{sum % kAdlerMod, weighted % kAdlerMod, n % kAdlerMod};
}
ICELK_PNG_FN Adler adler_join(const Adler& p, const Adler& q)
{
    return Adler{(p.A + q.A) % kAdlerMod, (uint32_t)((p.B + q.B + (uint64_t)q.n * p.A) % kAdlerMod), (p.n + q.n) % kAdlerMod};
}
// from the start value a = 1, b = 0
ICELK_PNG_FN uint32_t adler_value(const Adler& p) { return ((p.B + p.n) % kAdlerMod) << 16 | (1u + p.A) % kAdlerMod; }

}  // namespace png
}  // namespace icelk
