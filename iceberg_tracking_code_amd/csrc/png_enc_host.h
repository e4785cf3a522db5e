// png_enc_host.h -- the host statement of the PNG writer: the whole file, serially, with the functions of png_enc.h that
// the kernels of k_png.hip run.  Exported by abi_png.hip (icelk_png_filter_host, icelk_png_encode_host); the device's file
// equals this one byte for byte.  Also what both share on the host: the CRC-32 table and the file's frame around the
// deflate bytes (file_frame, file_finish), which the device call fills with the stream it copies down.
#pragma once
#include <string.h>

#include <new>

#include "../../include/icelk.h"
#include "png_enc.h"

namespace icelk {
namespace png {

// ---- CRC-32 (ISO 3309, PNG 1.2 annex D): by table, eight bytes a step ("slicing by 8": t[k][b] is the CRC of byte b
// followed by k zero bytes, so the eight look-ups of a step are independent) -------------------------------------------
struct CrcTable {
    uint32_t t[8][256];
    CrcTable()
    {
        for (uint32_t n = 0; n < 256; n++) {
            uint32_t c = n;
            for (int k = 0; k < 8; k++) c = c & 1u ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[0][n] = c;
        }
        for (uint32_t n = 0; n < 256; n++)
            for (int k = 1; k < 8; k++) t[k][n] = t[0][t[k - 1][n] & 0xffu] ^ (t[k - 1][n] >> 8);
    }
};
inline uint32_t crc_update(uint32_t crc, const uint8_t* p, size_t n)
{
    static const CrcTable T;
    for (; n >= 8; n -= 8, p += 8) {
        const uint32_t lo = crc ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
        crc = T.t[7][lo & 0xffu] ^ T.t[6][(lo >> 8) & 0xffu] ^ T.t[5][(lo >> 16) & 0xffu] ^ T.t[4][lo >> 24] ^ T.t[3][p[4]] ^ T.t[2][p[5]] ^
              T.t[1][p[6]] ^ T.t[0][p[7]];
    }
    for (size_t i = 0; i < n; i++) crc = T.t[0][(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
    return crc;
}
inline uint32_t crc_of(const uint8_t* p, size_t n) { return crc_update(0xffffffffu, p, n) ^ 0xffffffffu; }

inline void put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }

// length and type in front of `n` bytes of data at p + 8 that are there already, the CRC behind them; returns the end
inline uint8_t* close_chunk(uint8_t* p, const char* type, uint32_t n)
{
    put32(p, n);
    memcpy(p + 4, type, 4);
    put32(p + 8 + n, crc_of(p + 4, 4 + (size_t)n));
    return p + 12 + n;
}

// The file around `nbytes` deflate bytes.  ICELK_ECAP with nothing written when it does not fit (or out is NULL); *len is
// what the file takes either way.  Otherwise signature, IHDR and the zlib header are written and *at is where the deflate
// bytes go; file_finish then adds the Adler-32, IDAT's frame and IEND
inline int file_frame(int w, int h, uint32_t nbytes, uint8_t* out, uint64_t capacity, uint64_t* len, uint8_t** at)
{
    *len = (uint64_t)kFileFixed + nbytes;
    if (!out || capacity < *len) return ICELK_ECAP;
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    memcpy(out, sig, 8);
    uint8_t* p = out + 8;
    put32(p + 8, (uint32_t)w);
    put32(p + 12, (uint32_t)h);
    p[16] = 8, p[17] = 2, p[18] = 0, p[19] = 0, p[20] = 0;
    p = close_chunk(p, "IHDR", 13);
    p[8] = 0x78, p[9] = 0x01;
    *at = p + 10;   // == out + kStreamAt
    return ICELK_OK;
}
inline void file_finish(uint8_t* out, uint32_t nbytes, uint32_t adler)
{
    uint8_t* idat = out + 8 + 25;
    put32(idat + 8 + 2 + nbytes, adler);
    uint8_t* p = close_chunk(idat, "IDAT", 2 + nbytes + 4);
    close_chunk(p, "IEND", 0);
}

// ---- the filtered stream ----------------------------------------------------------------------------------------------
// row y of the picture (rows `stride` bytes apart) -> F + y (1 + 3 w)
inline void filter_row(const uint8_t* rgb, int w, size_t stride, int y, uint8_t* out)
{
    const uint8_t* cur = rgb + (size_t)y * stride;
    const uint8_t* up = y > 0 ? cur - stride : nullptr;
    const int n = 3 * w;
    uint32_t sum[5] = {0, 0, 0, 0, 0};
    for (int pass = 0, type = 0; pass < 2; pass++) {
        for (int x = 0; x < n; x++) {
            const int a = x >= 3 ? cur[x - 3] : 0, b = up ? up[x] : 0, c = up && x >= 3 ? up[x - 3] : 0;
            if (pass == 0)
                for (int t = 0; t < 5; t++) sum[t] += abs8(filter_value(t, cur[x], a, b, c));
            else
                out[1 + x] = filter_value(type, cur[x], a, b, c);
        }
        if (pass == 0) out[0] = (uint8_t)(type = pick_filter(sum));
    }
}

// F, h (1 + 3 w) bytes
inline int filter_host(const uint8_t* rgb, int w, int h, int stride, uint8_t* out)
{
    if (!rgb || !out || !size_ok(w, h) || stride < 3 * w) return ICELK_EARG;
    for (int y = 0; y < h; y++) filter_row(rgb, w, (size_t)stride, y, out + (size_t)y * pitch_of(w));
    return ICELK_OK;
}

// the token that begins at `pos` of F (n bytes) in a segment that ends at `end`
inline uint16_t token_at(const uint8_t* F, uint32_t pos, uint32_t end, uint32_t pitch)
{
    uint32_t run[kCandidates];
    for (int k = 0; k < kCandidates; k++) {
        const uint32_t d = distance_of(k, pitch);
        run[k] = 0;
        if (!distance_ok(d, pos)) continue;
        while (pos + run[k] < end && run[k] < (uint32_t)kMaxMatch && F[pos + run[k]] == F[pos + run[k] - d]) run[k]++;
    }
    return best_of(run, F[pos]);
}

struct BitSink {   // LSB first into zeroed bytes
    uint8_t* p;
    uint64_t at;
    void put(uint32_t v, int n)
    {
        for (int k = 0; k < n; k++, at++) p[at >> 3] |= (uint8_t)(((v >> k) & 1u) << (at & 7));
    }
};

// the file.  ICELK_EARG, ICELK_ENOMEM, ICELK_ECAP (with *len) or ICELK_OK
inline int encode_host(const uint8_t* rgb, int w, int h, int stride, uint8_t* out, uint64_t capacity, uint64_t* len)
{
    if (!rgb || !len || !size_ok(w, h) || stride < 3 * w) return ICELK_EARG;
    const uint32_t N = stream_of(w, h), pitch = pitch_of(w);
    uint8_t* F = new (std::nothrow) uint8_t[N];
    if (!F) return ICELK_ENOMEM;
    filter_host(rgb, w, h, stride, F);
    // the bits are counted first: the file's length is known before a byte of it is written
    uint32_t bits = 0;
    for (uint32_t s = 0; s < N; s += kSegment) {
        const uint32_t end = N - s < (uint32_t)kSegment ? N : s + kSegment;
        for (uint32_t pos = s; pos < end;) {
            const uint16_t t = token_at(F, pos, end, pitch);
            bits += (uint32_t)token_code(t, pitch).n;
            pos += token_advance(t);
        }
    }
    const uint32_t nbytes = deflate_bytes(bits);
    uint8_t* at = nullptr;
    int rc = file_frame(w, h, nbytes, out, capacity, len, &at);
    if (rc == ICELK_OK) {
        memset(at, 0, nbytes);
        BitSink sink{at, 0};
        sink.put(kHeaderValue, kHeaderBits);
        Adler sum{0, 0, 0};
        for (uint32_t s = 0; s < N; s += kSegment) {
            const uint32_t end = N - s < (uint32_t)kSegment ? N : s + kSegment;
            for (uint32_t pos = s; pos < end;) {
                const uint16_t t = token_at(F, pos, end, pitch);
                const Code c = token_code(t, pitch);
                sink.put(c.bits, c.n);
                pos += token_advance(t);
            }
            uint32_t A = 0, B = 0;
            for (uint32_t i = s; i < end; i++) A += F[i], B += (end - i) * F[i];
            sum = adler_join(sum, adler_piece(A, B, end - s));
        }
        file_finish(out, nbytes, adler_value(sum));   // the end-of-block's seven bits and the padding are the zeros there
    }
    delete[] F;
    return rc;
}

}  // namespace png
}  // namespace icelk
