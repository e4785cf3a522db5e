// jpeg_enc_host.h -- the host statement of the JPEG writer: the header Pillow's `img.save(path)` writes, and the scan
// coded serially with jpeg_enc.h, the code the device kernels run.  Plain C++ without the HIP runtime: abi_jpeg_enc.hip
// exports it (icelk_jpeg_encode_header, icelk_jpeg_encode_coefficients_host, icelk_jpeg_resave_file_host), and a
// stand-alone program can include it as it is (tests/jpeg_enc_host_main.cpp).  No global state that is written after the
// tables are built once: re-entrant.
//
// The file, in libjpeg's order: SOI, APP0 (JFIF 1.01, density 1 : 1 without a unit -- what `crop().save()` writes whatever
// the source said), one COM segment if a comment is given, a DQT segment per table slot (0, and 1 with three components),
// SOF0, a DHT segment per table in the order DC0, AC0, DC1, AC1 (the first two only with one component), SOS, the scan
// with a 00 stuffed behind every FF and the last byte filled with 1-bits, EOI.
#pragma once
#include <string.h>

#include <new>

#include "../../include/icelk.h"
#include "jpeg_enc.h"

namespace icelk {
namespace enc {

static const uint8_t kZigzag[64] = ICELK_ENC_ZIGZAG;

inline const Codes& codes()
{
    static const Codes C = [] {
        Codes c;
        build_codes(&c);
        return c;
    }();
    return C;
}

// The scan's layout of a descriptor, which must be laid out as icelk_jpeg_describe lays files out.  ICELK_EARG: not such a
// descriptor; ICELK_EUNSUP: restart intervals, or a third quantisation table; ICELK_ECAP: blocks * 1660 bits do not fit
// 32 bits (bit offsets are carried in 32 bits, on the host as on the device)
inline int layout_of(const icelk_jpeg_info_t* I, Layout* L)
{
    if (!I) return ICELK_EARG;
    if (I->ncomp != 1 && I->ncomp != 3) return ICELK_EARG;
    if (I->width < 1 || I->height < 1 || I->width > 65535 || I->height > 65535) return ICELK_EARG;
    const int hs = I->hmax, vs = I->vmax;
    if (I->ncomp == 1 ? (hs != 1 || vs != 1) : !((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return ICELK_EARG;
    const int mx = (I->width + 8 * hs - 1) / (8 * hs), my = (I->height + 8 * vs - 1) / (8 * vs);
    if (I->mcus_x != mx || I->mcus_y != my) return ICELK_EARG;
    uint64_t off = 0;
    for (int c = 0; c < 3; c++) {
        const bool on = c < I->ncomp;
        const int bx = on ? mx * (c ? 1 : hs) : 0, by = on ? my * (c ? 1 : vs) : 0;
        if (I->blocks_x[c] != bx || I->blocks_y[c] != by || I->coef_offset[c] != off) return ICELK_EARG;
        off += (uint64_t)bx * by * 64;
        if (on)
            for (int i = 0; i < 64; i++)
                if (I->quant[c][i] < 1 || I->quant[c][i] > 255) return ICELK_EARG;   // an 8-bit DQT
    }
    if (I->coef_count != off) return ICELK_EARG;
    if (I->restart_interval != 0) return ICELK_EUNSUP;
    if (I->ncomp == 3 && memcmp(I->quant[1], I->quant[2], sizeof(I->quant[1]))) return ICELK_EUNSUP;   // slots 0 and 1 only
    const uint64_t bpm = (uint64_t)(I->ncomp == 1 ? 1 : hs * vs + 2), blocks = bpm * mx * my;
    if (blocks * kMaxBlockBits >= ((uint64_t)1 << 32)) return ICELK_ECAP;
    L->ncomp = I->ncomp;
    L->hs = hs;
    L->vs = vs;
    L->mcus_x = mx;
    L->bpm = (uint32_t)bpm;
    L->blocks = (uint32_t)blocks;
    L->luma_bx = (uint32_t)I->blocks_x[0];
    L->off0 = (uint32_t)I->coef_offset[0];
    L->off1 = (uint32_t)I->coef_offset[1];
    L->off2 = (uint32_t)I->coef_offset[2];
    return ICELK_OK;
}

// bytes that are written only while they fit; `n` counts them all the same
struct Bytes {
    uint8_t* out;
    uint64_t cap, n = 0;
    Bytes(uint8_t* o, uint64_t c) : out(o), cap(o ? c : 0) {}
    void put(uint8_t b)
    {
        if (n < cap) out[n] = b;
        n++;
    }
    void put16(unsigned v)
    {
        put((uint8_t)(v >> 8));
        put((uint8_t)v);
    }
    void put(const void* p, size_t k)
    {
        for (size_t i = 0; i < k; i++) put(((const uint8_t*)p)[i]);
    }
};

inline bool comment_ok(const uint8_t* comment, uint64_t comment_len) { return comment_len <= 65533 && (comment || comment_len == 0); }

// SOI .. the end of SOS into B (the descriptor has passed layout_of)
inline void header_bytes(const icelk_jpeg_info_t& I, const uint8_t* comment, uint64_t comment_len, Bytes& B)
{
    static const uint8_t app0[] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    B.put16(0xFFD8);
    B.put(app0, sizeof(app0));
    if (comment) {   // an empty comment is a segment too
        B.put16(0xFFFE);
        B.put16((unsigned)comment_len + 2);
        B.put(comment, (size_t)comment_len);
    }
    const int nt = I.ncomp == 1 ? 1 : 2;
    for (int t = 0; t < nt; t++) {
        B.put16(0xFFDB);
        B.put16(67);
        B.put((uint8_t)t);
        for (int k = 0; k < 64; k++) B.put((uint8_t)I.quant[t][kZigzag[k]]);
    }
    B.put16(0xFFC0);
    B.put16(8 + 3 * I.ncomp);
    B.put(8);
    B.put16((unsigned)I.height);
    B.put16((unsigned)I.width);
    B.put((uint8_t)I.ncomp);
    for (int c = 0; c < I.ncomp; c++) {
        B.put((uint8_t)(c + 1));
        B.put((uint8_t)(c ? 0x11 : I.hmax << 4 | I.vmax));
        B.put((uint8_t)(c ? 1 : 0));
    }
    for (int t = 0; t < nt; t++)
        for (int ac = 0; ac < 2; ac++) {
            const HuffSpec& S = kSpec[ac ? SPEC_AC0 + t : SPEC_DC0 + t];
            B.put16(0xFFC4);
            B.put16(19 + S.nval);
            B.put((uint8_t)(ac << 4 | t));
            B.put(S.bits, 16);
            B.put(S.val, (size_t)S.nval);
        }
    B.put16(0xFFDA);
    B.put16(6 + 2 * I.ncomp);
    B.put((uint8_t)I.ncomp);
    for (int c = 0; c < I.ncomp; c++) {
        B.put((uint8_t)(c + 1));
        B.put((uint8_t)(c ? 0x11 : 0x00));
    }
    B.put(0);
    B.put(63);
    B.put(0);
}

inline int header_host(const icelk_jpeg_info_t* info, const uint8_t* comment, uint64_t comment_len, uint8_t* out, uint64_t capacity,
                       uint64_t* len)
{
    Layout L;
    if (!len || !comment_ok(comment, comment_len)) return ICELK_EARG;
    if (int rc = layout_of(info, &L)) return rc;
    Bytes B(out, capacity);
    header_bytes(*info, comment, comment_len, B);
    *len = B.n;
    return out && B.n <= capacity ? ICELK_OK : ICELK_ECAP;
}

// ---- the file around a scan: header | scan | EOI ------------------------------------------------------------------------------
// the file's length
inline uint64_t file_len(const icelk_jpeg_info_t& I, const uint8_t* comment, uint64_t comment_len, uint64_t scan_len)
{
    Bytes H(nullptr, 0);
    header_bytes(I, comment, comment_len, H);
    return H.n + scan_len + 2;
}

// Header and EOI of a file whose scan takes scan_len bytes into `out`; *scan_at: where the scan goes, which the caller
// fills (from host memory: file_into; from the device: jpeg_deliver_file, abi_jpeg_enc.hip; as it is coded: encode_host).
// ICELK_ECAP with nothing written: out is too small (or NULL); *len says what the file takes in either case
inline int file_frame(const icelk_jpeg_info_t& I, const uint8_t* comment, uint64_t comment_len, uint64_t scan_len, uint8_t* out,
                      uint64_t capacity, uint64_t* len, uint8_t** scan_at)
{
    *len = file_len(I, comment, comment_len, scan_len);
    if (!out || capacity < *len) return ICELK_ECAP;
    Bytes B(out, capacity);
    header_bytes(I, comment, comment_len, B);
    *scan_at = out + B.n;
    out[B.n + scan_len] = 0xFF;
    out[B.n + scan_len + 1] = 0xD9;
    return ICELK_OK;
}

// the whole file around a scan in host memory
inline int file_into(const icelk_jpeg_info_t& I, const uint8_t* comment, uint64_t comment_len, const uint8_t* scan, uint64_t scan_len,
                     uint8_t* out, uint64_t capacity, uint64_t* len)
{
    uint8_t* at = nullptr;
    if (int rc = file_frame(I, comment, comment_len, scan_len, out, capacity, len, &at)) return rc;
    if (scan_len) memcpy(at, scan, (size_t)scan_len);
    return ICELK_OK;
}

// bits -> bytes, most significant first, a 00 behind every FF
struct ByteSink {
    Bytes& B;
    uint64_t acc = 0;
    int n = 0;
    explicit ByteSink(Bytes& b) : B(b) {}
    void put(uint32_t v, int k)
    {
        acc = acc << k | v;
        n += k;
        while (n >= 8) {
            n -= 8;
            const uint8_t b = (uint8_t)(acc >> n);
            B.put(b);
            if (b == 0xFF) B.put(0);
        }
        acc &= ((uint64_t)1 << n) - 1;
    }
    void pad()
    {
        if (n) put((1u << (8 - n)) - 1u, 8 - n);
    }
};

struct HostBlock {
    const int16_t* blk;
    int operator()(int k) const { return blk[kZigzag[k]]; }
};

// the whole file.  ICELK_ECAP: out is too small (or NULL), *len says what it takes; ICELK_EARG: a coefficient without a
// code -- found by the measuring pass before anything is written
inline int encode_host(const icelk_jpeg_info_t* info, const int16_t* coef, const uint8_t* comment, uint64_t comment_len, uint8_t* out,
                       uint64_t capacity, uint64_t* len)
{
    Layout L;
    if (!len || !coef || !comment_ok(comment, comment_len)) return ICELK_EARG;
    if (int rc = layout_of(info, &L)) return rc;
    const Codes& C = codes();
    // the scan twice: measured (into no buffer), then written where file_frame says
    auto scan_into = [&](Bytes& B) {
        ByteSink S(B);
        for (uint32_t s = 0; s < L.blocks; s++) {
            const Place P = place(L, s);
            if (!encode_block(HostBlock{coef + P.at}, P.pred == kNoPred ? 0 : coef[P.pred], C.dc[P.table], C.ac[P.table], S)) return false;
        }
        S.pad();
        return true;
    };
    Bytes N(nullptr, 0);
    if (!scan_into(N)) return ICELK_EARG;
    uint8_t* at = nullptr;
    if (int rc = file_frame(*info, comment, comment_len, N.n, out, capacity, len, &at)) return rc;
    Bytes B(at, N.n);
    scan_into(B);
    return ICELK_OK;
}

// ---- the budgeted chain of a job with a file (abi_jpeg_job.hip), in the kernels' order --------------------------------------------
// count, scan, pack, ff, scan, stuff and the verdict as k_jpeg_enc.hip runs them when the sizes stay on the device, with
// the decisions of jpeg_enc.h: `packed` and `out` hold exactly cap = bytes_per_block x blocks bytes and nothing is read
// or written outside them, whatever the control words say.  force / force_mask: words of ctl (bit JE_* of the mask) that
// are overwritten after the scan that writes them -- what a test uses to show that no contents of ctl lead outside.
struct BudgetWalk {
    uint32_t cap, chunks, groups;            // capacity in bytes, in chunks, in workgroups of ff / stuff
    uint32_t total_bits, invalid, ff_total;  // the control words as the verdict saw them
    uint32_t verdict;                        // enc::Verdict
    uint32_t stuffed;                        // bytes in `out` when the verdict is kCoded, else 0
    uint32_t packed_stores, out_stores;      // bytes pack / stuff stored
};

// bits OR-ed into a zeroed byte buffer at a bit offset, most significant first
struct PackSink {
    uint8_t* p;
    uint64_t at;
    void put(uint32_t v, int k)
    {
        for (int i = k - 1; i >= 0; i--, at++)
            if (v >> i & 1u) p[at >> 3] |= (uint8_t)(0x80u >> (at & 7u));
    }
};

// ICELK_OK with W filled (the verdict is in W, not in the code); ICELK_EARG / _EUNSUP / _ECAP as layout_of; ICELK_ENOMEM
inline int encode_budgeted_host(const icelk_jpeg_info_t* info, const int16_t* coef, int bytes_per_block, const uint32_t* force,
                                uint32_t force_mask, uint8_t* packed, uint8_t* out, BudgetWalk* W)
{
    constexpr uint32_t kGroupBlocks = 64;    // blocks per workgroup of count and pack
    enum { TOTAL_BITS = 0, INVALID = 1, FF_TOTAL = 2 };   // JpegEncCtl (icelk_internal.h)
    Layout L;
    if (!coef || !W || !packed || !out || bytes_per_block < kMinBytesPerBlock || bytes_per_block > kMaxBytesPerBlock) return ICELK_EARG;
    if (force_mask && !force) return ICELK_EARG;
    if (int rc = layout_of(info, &L)) return rc;
    const Codes& C = codes();
    const uint32_t cap = budget_cap(L.blocks, bytes_per_block), chunks = chunks_of(cap), groups = groups_of(chunks);
    *W = BudgetWalk{};
    W->cap = cap;
    W->chunks = chunks;
    W->groups = groups;
    uint32_t ctl[3] = {0, 0, 0};
    auto forced = [&](int k) {
        if (force_mask >> k & 1u) ctl[k] = force[k];
    };
    // count
    const uint32_t ngroups = (L.blocks + kGroupBlocks - 1) / kGroupBlocks;
    uint16_t* bits = new (std::nothrow) uint16_t[L.blocks];
    uint32_t* group = new (std::nothrow) uint32_t[ngroups];
    uint32_t* wg_ff = new (std::nothrow) uint32_t[groups ? groups : 1];
    struct Drop {
        uint16_t* a;
        uint32_t *b, *c;
        ~Drop()
        {
            delete[] a;
            delete[] b;
            delete[] c;
        }
    } drop{bits, group, wg_ff};
    if (!bits || !group || !wg_ff) return ICELK_ENOMEM;
    for (uint32_t g = 0; g < ngroups; g++) group[g] = 0;
    for (uint32_t s = 0; s < L.blocks; s++) {
        const Place P = place(L, s);
        CountSink n;
        if (!encode_block(HostBlock{coef + P.at}, P.pred == kNoPred ? 0 : coef[P.pred], C.dc[P.table], C.ac[P.table], n)) ctl[INVALID] |= 1u;
        bits[s] = (uint16_t)n.bits;
        group[s / kGroupBlocks] += n.bits;
    }
    // scan: exclusive, in place; the total
    uint32_t run = 0;
    for (uint32_t g = 0; g < ngroups; g++) {
        const uint32_t x = group[g];
        group[g] = run;
        run += x;
    }
    ctl[TOTAL_BITS] = run;
    forced(TOTAL_BITS);
    forced(INVALID);
    // pack: the packed stream is zeroed over its whole capacity first
    memset(packed, 0, cap);
    if (packed_fits(ctl[TOTAL_BITS], ctl[INVALID], cap)) {
        for (uint32_t g = 0; g < ngroups; g++) {
            const uint32_t s0 = g * kGroupBlocks, s1 = s0 + kGroupBlocks < L.blocks ? s0 + kGroupBlocks : L.blocks;
            uint32_t sum = 0;
            for (uint32_t s = s0; s < s1; s++) sum += bits[s];
            const uint32_t start = group[g];
            uint32_t end = start + sum;
            const uint32_t fill = g == ngroups - 1 ? (0u - end) & 7u : 0u;
            end += fill;
            if (!stretch_inside(start, end, cap)) continue;
            PackSink S{packed, start};
            for (uint32_t s = s0; s < s1; s++) {
                const Place P = place(L, s);
                encode_block(HostBlock{coef + P.at}, P.pred == kNoPred ? 0 : coef[P.pred], C.dc[P.table], C.ac[P.table], S);
            }
            if (fill) S.put((1u << fill) - 1u, (int)fill);
            W->packed_stores += packed_bytes(end) - packed_bytes(start);   // a byte two stretches share counts for the first
        }
    }
    // ff: per workgroup of the capacity, over the live bytes only
    const uint32_t live = live_bytes(ctl[TOTAL_BITS], ctl[INVALID], cap);
    const uint32_t wg_bytes = (uint32_t)kChunkBytes * kChunksPerGroup;
    for (uint32_t g = 0; g < groups; g++) {
        uint32_t n = 0;
        for (uint64_t i = (uint64_t)g * wg_bytes; i < (uint64_t)(g + 1) * wg_bytes && i < live; i++) n += packed[i] == 0xFF;
        wg_ff[g] = n;
    }
    // scan
    run = 0;
    for (uint32_t g = 0; g < groups; g++) {
        const uint32_t x = wg_ff[g];
        wg_ff[g] = run;
        run += x;
    }
    ctl[FF_TOTAL] = run;
    forced(FF_TOTAL);
    // stuff: a lane per chunk
    if (stuffed_fits(ctl[TOTAL_BITS], ctl[INVALID], ctl[FF_TOTAL], cap)) {
        const uint32_t nbytes = packed_bytes(ctl[TOTAL_BITS]), nchunks = chunks_of(nbytes);
        uint32_t before = 0;
        for (uint32_t ch = 0; ch < nchunks; ch++) {
            if (ch % kChunksPerGroup == 0) before = wg_ff[ch / kChunksPerGroup];
            const uint32_t at = ch * (uint32_t)kChunkBytes, n = nbytes - at < (uint32_t)kChunkBytes ? nbytes - at : (uint32_t)kChunkBytes;
            uint32_t ff = 0;
            for (uint32_t j = 0; j < n; j++) ff += packed[at + j] == 0xFF;
            if (bytes_inside((uint64_t)at + before, n + ff, cap)) {
                uint8_t* dst = out + at + before;
                for (uint32_t j = 0; j < n; j++) {
                    *dst++ = packed[at + j];
                    if (packed[at + j] == 0xFF) *dst++ = 0;
                }
                W->out_stores += n + ff;
            }
            before += ff;
        }
    }
    // verdict
    W->total_bits = ctl[TOTAL_BITS];
    W->invalid = ctl[INVALID];
    W->ff_total = ctl[FF_TOTAL];
    W->verdict = budget_verdict(ctl[TOTAL_BITS], ctl[INVALID], ctl[FF_TOTAL], cap);
    W->stuffed = W->verdict == kCoded ? packed_bytes(ctl[TOTAL_BITS]) + ctl[FF_TOTAL] : 0u;
    return ICELK_OK;
}

}  // namespace enc
}  // namespace icelk
