// abi_jpeg.hip -- the host half of the JPEG ingest path: headers and Huffman decoding of a baseline file into quantised
// DCT coefficients (icelk_jpeg_describe, icelk_jpeg_read_coefficients).  Host code only, no handle, no global state that
// is written after start-up: the decode-ahead threads of sequence.py run it side by side.  The device half is k_jpeg.hip,
// reached through icelk_upload_jpeg / icelk_jpeg_decode_rgb (abi_jpeg_ingest.hip).
//
// For Huffman decoding on the device (k_jpeg_huff.hip) this file also locates the entropy-coded segments and packs the
// tables (icelk_jpeg_index), and states the parallel algorithm of jpeg_lanes.h serially, phase by phase, on the CPU
// (icelk_jpeg_read_coefficients_lanes).
//
// The stream is outside input: every byte is fetched through a bounds check, every table index is checked before use,
// and anything that does not add up returns ICELK_EARG.  Nothing here throws or aborts.
//
// Format: ITU-T T.81 (markers B.1, frame header B.2.2, scan header B.2.3, tables B.2.4, Huffman procedures Annex C and
// F.2.2).  What counts as "YCbCr" follows libjpeg's guess (JFIF marker / Adobe transform / component ids), because the
// result has to equal Pillow's.
#include <new>
#include <vector>

#include "icelk_ctx.h"
#include "jpeg_lanes.h"

namespace icelk {

namespace {

constexpr int kLookBits = 9;

// natural (row-major) index of the k-th coefficient in zigzag order (T.81 Figure A.6): walked along the diagonals
struct Zigzag {
    uint8_t nat[64];
    Zigzag()
    {
        int k = 0;
        for (int s = 0; s < 15; s++) {
            // odd diagonals run downwards (row grows), even ones upwards
            for (int i = 0; i < 8; i++) {
                const int r = (s & 1) ? i : 7 - i;
                const int c = s - r;
                if (c >= 0 && c < 8) nat[k++] = (uint8_t)(r * 8 + c);
            }
        }
    }
};
const Zigzag kZigzag;

struct Huff {
    bool set = false;
    uint16_t look[1 << kLookBits];   // code length << 8 | symbol for codes of up to kLookBits bits, 0: a longer code
    int32_t maxcode[17];             // largest code of each length, -1: none
    int32_t valoff[17];              // index of a length's first symbol minus its first code
    uint8_t vals[256];
};

struct Parsed {
    icelk_jpeg_info_t I;
    Huff dc[4], ac[4];
    uint16_t qt[4][64];
    bool qt_set[4] = {false, false, false, false};
    int td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    int comp_hs[3] = {1, 1, 1}, comp_vs[3] = {1, 1, 1};
    size_t scan = 0;                 // first byte of the entropy-coded data
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

int build_huff(Huff& H, const uint8_t* counts, const uint8_t* symbols, int nsym)
{
    memset(H.look, 0, sizeof(H.look));
    memcpy(H.vals, symbols, nsym);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; len++) {
        const int n = counts[len - 1];
        H.maxcode[len] = -1;
        H.valoff[len] = k - code;
        if (n) {
            if (code + n > (1 << len)) return ICELK_EARG;   // more codes than the length has
            if (len <= kLookBits) {
                for (int j = 0; j < n; j++) {
                    const int first = (code + j) << (kLookBits - len);
                    for (int f = 0; f < (1 << (kLookBits - len)); f++) H.look[first + f] = (uint16_t)(len << 8 | symbols[k + j]);
                }
            }
            H.maxcode[len] = code + n - 1;
            code += n;
            k += n;
        }
        code <<= 1;
    }
    H.set = true;
    return ICELK_OK;
}

// sizes and offsets that follow from width, height, ncomp and the luma sampling factors
void fill_layout(icelk_jpeg_info_t& I)
{
    I.mcus_x = (I.width + 8 * I.hmax - 1) / (8 * I.hmax);
    I.mcus_y = (I.height + 8 * I.vmax - 1) / (8 * I.vmax);
    uint64_t off = 0;
    for (int c = 0; c < 3; c++) {
        const int hs = c == 0 ? I.hmax : 1, vs = c == 0 ? I.vmax : 1;
        const bool on = c < I.ncomp;
        I.comp_w[c] = on ? (I.width * hs + I.hmax - 1) / I.hmax : 0;
        I.comp_h[c] = on ? (I.height * vs + I.vmax - 1) / I.vmax : 0;
        I.blocks_x[c] = on ? I.mcus_x * hs : 0;
        I.blocks_y[c] = on ? I.mcus_y * vs : 0;
        I.coef_offset[c] = off;
        off += (uint64_t)I.blocks_x[c] * I.blocks_y[c] * 64;
    }
    I.coef_count = off;
}

// the component counts and luma sampling factors the decoder takes (chroma is 1 x 1)
bool sampling_ok(int ncomp, int hs, int vs)
{
    if (ncomp == 1) return hs == 1 && vs == 1;
    return ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
}

int parse_headers(const uint8_t* d, size_t len, Parsed& P)
{
    memset(&P.I, 0, sizeof(P.I));
    if (len < 4 || d[0] != 0xFF || d[1] != 0xD8) return ICELK_EARG;
    size_t pos = 2;
    bool sof = false, jfif = false, adobe = false;
    int adobe_transform = 0, comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
    for (;;) {
        if (pos + 2 > len || d[pos] != 0xFF) return ICELK_EARG;
        while (pos + 2 <= len && d[pos + 1] == 0xFF) pos++;   // fill bytes in front of a marker
        if (pos + 2 > len) return ICELK_EARG;
        const int m = d[pos + 1];
        if (m == 0xD8 || m == 0xD9 || m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) return ICELK_EARG;   // no frame, no scan
        if (pos + 4 > len) return ICELK_EARG;
        const size_t n = (size_t)be16(d + pos + 2);
        if (n < 2 || pos + 2 + n > len) return ICELK_EARG;
        const uint8_t* b = d + pos + 4;
        const size_t bn = n - 2;
        pos += 2 + n;
        if (m == 0xC0) {
            if (sof || bn < 6) return ICELK_EARG;
            const int nc = b[5];
            if (bn != (size_t)(6 + 3 * nc)) return ICELK_EARG;
            if (b[0] != 8) return ICELK_EUNSUP;
            P.I.height = be16(b + 1);
            P.I.width = be16(b + 3);
            if (P.I.width == 0) return ICELK_EARG;
            if (P.I.height == 0) return ICELK_EUNSUP;   // the height comes in a DNL marker
            if (nc != 1 && nc != 3) return nc == 0 ? ICELK_EARG : ICELK_EUNSUP;
            P.I.ncomp = nc;
            for (int c = 0; c < nc; c++) {
                comp_id[c] = b[6 + 3 * c];
                P.comp_hs[c] = b[7 + 3 * c] >> 4;
                P.comp_vs[c] = b[7 + 3 * c] & 15;
                comp_tq[c] = b[8 + 3 * c];
                if (P.comp_hs[c] < 1 || P.comp_hs[c] > 4 || P.comp_vs[c] < 1 || P.comp_vs[c] > 4 || comp_tq[c] > 3) return ICELK_EARG;
            }
            sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
            return ICELK_EUNSUP;     // extended, progressive, lossless, differential, arithmetic (SOFn, DAC)
        } else if (m == 0xDC) {
            return ICELK_EUNSUP;     // DNL
        } else if (m == 0xC4) {
            size_t k = 0;
            while (k < bn) {
                if (k + 17 > bn) return ICELK_EARG;
                const int tc = b[k] >> 4, th = b[k] & 15;
                if (tc > 1 || th > 3) return ICELK_EARG;
                int nsym = 0;
                for (int i = 0; i < 16; i++) nsym += b[k + 1 + i];
                if (nsym > 256 || k + 17 + nsym > bn) return ICELK_EARG;
                if (int rc = build_huff(tc ? P.ac[th] : P.dc[th], b + k + 1, b + k + 17, nsym)) return rc;
                k += 17 + nsym;
            }
        } else if (m == 0xDB) {
            size_t k = 0;
            while (k < bn) {
                const int pq = b[k] >> 4, tq = b[k] & 15;
                if (tq > 3 || pq > 1) return ICELK_EARG;
                if (pq == 1) return ICELK_EUNSUP;
                if (k + 65 > bn) return ICELK_EARG;
                for (int i = 0; i < 64; i++) P.qt[tq][kZigzag.nat[i]] = b[k + 1 + i];
                P.qt_set[tq] = true;
                k += 65;
            }
        } else if (m == 0xDD) {
            if (bn != 2) return ICELK_EARG;
            P.I.restart_interval = be16(b);
        } else if (m == 0xE0) {
            if (bn >= 5 && !memcmp(b, "JFIF", 5)) jfif = true;
        } else if (m == 0xEE) {
            if (bn >= 12 && !memcmp(b, "Adobe", 5)) {
                adobe = true;
                adobe_transform = b[11];
            }
        } else if (m == 0xDA) {
            if (!sof) return ICELK_EARG;
            const int nc = P.I.ncomp;
            if (bn < 1) return ICELK_EARG;
            const int ns = b[0];
            if (ns < 1 || ns > 4 || bn != (size_t)(4 + 2 * ns)) return ICELK_EARG;
            if (ns != nc) return ICELK_EUNSUP;                      // one scan per component: several scans
            for (int c = 0; c < nc; c++) {
                if (b[1 + 2 * c] != comp_id[c]) return ICELK_EUNSUP;   // another component order
                P.td[c] = b[2 + 2 * c] >> 4;
                P.ta[c] = b[2 + 2 * c] & 15;
                if (P.td[c] > 3 || P.ta[c] > 3 || !P.dc[P.td[c]].set || !P.ac[P.ta[c]].set) return ICELK_EARG;
                if (!P.qt_set[comp_tq[c]]) return ICELK_EARG;
            }
            if (b[1 + 2 * ns] != 0 || b[2 + 2 * ns] != 63 || b[3 + 2 * ns] != 0) return ICELK_EUNSUP;   // a progressive scan's parameters
            P.scan = pos;
            break;
        }
        // everything else (APPn, COM, ...) is skipped
    }
    icelk_jpeg_info_t& I = P.I;
    if (I.ncomp == 3) {
        // libjpeg's colour-space guess must come out as YCbCr
        if (adobe && adobe_transform != 1) return ICELK_EUNSUP;
        if (!jfif && !adobe && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return ICELK_EUNSUP;
        if (P.comp_hs[1] != 1 || P.comp_vs[1] != 1 || P.comp_hs[2] != 1 || P.comp_vs[2] != 1) return ICELK_EUNSUP;
    }
    if (!sampling_ok(I.ncomp, P.comp_hs[0], P.comp_vs[0])) return ICELK_EUNSUP;
    I.hmax = P.comp_hs[0];
    I.vmax = P.comp_vs[0];
    if (I.width < 3) return ICELK_EUNSUP;   // libjpeg's own result depends on its padding when a chroma plane is one sample wide
    fill_layout(I);
    for (int c = 0; c < I.ncomp; c++) memcpy(I.quant[c], P.qt[comp_tq[c]], sizeof(I.quant[c]));
    return ICELK_OK;
}

// The bit reader.  `acc` holds `n` valid bits at its top.  Behind the end of the data or in front of a marker zero bits
// are fed (`pad` counts them); whoever consumes one of those has run off the stream: ok() says so.
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;
    int n = 0, pad = 0;

    void refill()   // called with n < 32
    {
        if (end - p >= 4) {
            const uint32_t w = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
            const uint32_t inv = ~w;   // a byte 0xFF in w is a zero byte in inv
            if (!((inv - 0x01010101u) & ~inv & 0x80808080u)) {
                acc |= (uint64_t)w << (32 - n);
                n += 32;
                p += 4;
                return;
            }
        }
        while (n <= 56) {
            if (pad == 0 && p < end) {
                const uint8_t b = *p;
                if (b != 0xFF) {
                    p++;
                    acc |= (uint64_t)b << (56 - n);
                    n += 8;
                    continue;
                }
                if (end - p >= 2 && p[1] == 0) {   // a stuffed zero behind a data byte 0xFF
                    p += 2;
                    acc |= (uint64_t)0xFF << (56 - n);
                    n += 8;
                    continue;
                }
            }
            pad += 8;   // a marker, or the end of the data: stay in front of it
            n += 8;
        }
    }
    inline void need32()
    {
        if (n < 32) refill();
    }
    inline uint32_t peek(int k) const { return (uint32_t)(acc >> (64 - k)); }   // 1 <= k <= 32
    inline void drop(int k)
    {
        acc <<= k;
        n -= k;
    }
    inline bool ok() const { return n >= pad; }
    void reset(const uint8_t* at)
    {
        p = at;
        acc = 0;
        n = pad = 0;
    }
};

// one Huffman symbol; at least 16 bits are in the accumulator.  < 0: no such code
inline int symbol(Bits& B, const Huff& H)
{
    const uint32_t e = H.look[B.peek(kLookBits)];
    if (e) {
        B.drop(e >> 8);
        return e & 255;
    }
    const int32_t v = (int32_t)B.peek(16);
    for (int len = kLookBits + 1; len <= 16; len++) {
        const int32_t code = v >> (16 - len);
        if (code <= H.maxcode[len]) {
            const int idx = H.valoff[len] + code;
            if (idx < 0 || idx > 255) return -1;
            B.drop(len);
            return H.vals[idx];
        }
    }
    return -1;
}

// s more bits as a signed value (T.81 F.2.2.1 EXTEND); 1 <= s <= 15
inline int receive_extend(Bits& B, int s)
{
    const int v = (int)B.peek(s);
    B.drop(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

int decode_block(Bits& B, const Huff& dc, const Huff& ac, int& pred, int16_t* blk)
{
    memset(blk, 0, 64 * sizeof(int16_t));
    B.need32();
    int s = symbol(B, dc);
    if (s < 0 || s > 15) return ICELK_EARG;
    if (s) pred += receive_extend(B, s);
    blk[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        B.need32();
        const int rs = symbol(B, ac);
        if (rs < 0) return ICELK_EARG;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;   // end of block
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) return ICELK_EARG;
        blk[kZigzag.nat[k]] = (int16_t)receive_extend(B, s);
        k++;
    }
    return B.ok() ? ICELK_OK : ICELK_EARG;
}

int decode_scan(const uint8_t* d, size_t len, const Parsed& P, int16_t* coef)
{
    const icelk_jpeg_info_t& I = P.I;
    Bits B;
    B.end = d + len;
    B.reset(d + P.scan);
    int pred[3] = {0, 0, 0};
    int left = I.restart_interval, nrst = 0;
    for (int my = 0; my < I.mcus_y; my++) {
        for (int mx = 0; mx < I.mcus_x; mx++) {
            if (I.restart_interval && left == 0) {
                // the bits left over in front of the marker are padding; the marker itself was never consumed
                const uint8_t* q = B.p;
                while (B.end - q >= 2 && q[0] == 0xFF && q[1] == 0xFF) q++;
                if (B.end - q < 2 || q[0] != 0xFF || q[1] != 0xD0 + (nrst & 7)) return ICELK_EARG;
                B.reset(q + 2);
                nrst++;
                left = I.restart_interval;
                pred[0] = pred[1] = pred[2] = 0;
            }
            left--;
            for (int c = 0; c < I.ncomp; c++) {
                const int hs = c == 0 ? I.hmax : 1, vs = c == 0 ? I.vmax : 1;
                for (int v = 0; v < vs; v++) {
                    for (int u = 0; u < hs; u++) {
                        const size_t blk = (size_t)(my * vs + v) * I.blocks_x[c] + (size_t)(mx * hs + u);
                        if (int rc = decode_block(B, P.dc[P.td[c]], P.ac[P.ta[c]], pred[c], coef + I.coef_offset[c] + blk * 64)) return rc;
                    }
                }
            }
        }
    }
    return ICELK_OK;
}


// ---- the scan as the lanes see it ---------------------------------------------------------------------------------------
// the next marker at or behind `from`: the first FF that is not followed by a stuffed zero; len: none
size_t next_marker(const uint8_t* d, size_t len, size_t from)
{
    size_t q = from;
    while (q < len) {
        const void* f = memchr(d + q, 0xFF, len - q);
        if (!f) return len;
        q = (size_t)((const uint8_t*)f - d);
        if (q + 1 < len && d[q + 1] == 0) {
            q += 2;
            continue;
        }
        return q;
    }
    return len;
}

void pack_table(const Huff& H, lanes::HuffTable& T)
{
    memset(&T, 0, sizeof(T));
    for (int i = 0; i < 17; i++) T.maxcode[i] = -1;
    if (!H.set) return;
    memcpy(T.look, H.look, sizeof(T.look));
    for (int len = 1; len <= 16; len++) {
        T.maxcode[len] = H.maxcode[len];
        T.valoff[len] = H.valoff[len];
    }
    memcpy(T.vals, H.vals, sizeof(T.vals));
}

}  // namespace

static_assert(sizeof(lanes::HuffTable) * lanes::kTables == ICELK_JPEG_TABLE_BYTES, "the header states the packed tables' size");

// Headers, segments and tables of a file.  The RSTn markers must come in the order D0 .. D7, D0 ... and be as many as
// the restart interval and the number of MCUs imply; what follows the last segment is not looked at.
int jpeg_index(const uint8_t* d, size_t len, JpegIndex& X)
{
    if (len >= ((size_t)1 << 28)) return ICELK_EUNSUP;   // positions are 32-bit bit offsets
    Parsed* P = new (std::nothrow) Parsed;
    if (!P) return ICELK_ENOMEM;
    int rc = parse_headers(d, len, *P);
    if (rc) {
        delete P;
        return rc;
    }
    X.info = P->I;
    for (int t = 0; t < 4; t++) {
        pack_table(P->dc[t], X.tabs[t]);
        pack_table(P->ac[t], X.tabs[4 + t]);
    }
    const icelk_jpeg_info_t& I = X.info;
    lanes::Scan& A = X.scan;
    memset(&A, 0, sizeof(A));
    int b = 0;
    for (int c = 0; c < I.ncomp; c++) {
        const int hs = c == 0 ? I.hmax : 1, vs = c == 0 ? I.vmax : 1;
        for (int v = 0; v < vs; v++)
            for (int u = 0; u < hs; u++, b++) {
                A.comp_pack |= (uint32_t)c << (2 * b);
                A.dc_pack |= (uint32_t)P->td[c] << (2 * b);
                A.ac_pack |= (uint32_t)P->ta[c] << (2 * b);
                A.u_pack |= (uint32_t)u << (2 * b);
                A.v_pack |= (uint32_t)v << (2 * b);
            }
    }
    const size_t scan = P->scan;
    delete P;
    A.bpm = b;
    A.nmcu = I.mcus_x * I.mcus_y;
    A.mcus_x = I.mcus_x;
    A.total_blocks = (uint32_t)A.nmcu * (uint32_t)b;
    const uint32_t ri = I.restart_interval > 0 && I.restart_interval < A.nmcu ? (uint32_t)I.restart_interval : 0;
    A.seg_blocks = ri * (uint32_t)b;
    A.nseg = ri ? ((uint32_t)A.nmcu + ri - 1) / ri : 1;
    A.hs = I.hmax;
    A.vs = I.vmax;
    A.blocks_x0 = I.blocks_x[0];
    A.blocks_x1 = I.blocks_x[1];
    A.off0 = I.coef_offset[0];
    A.off1 = I.coef_offset[1];
    A.off2 = I.coef_offset[2];
    try {
        X.seg.assign(A.nseg + 1, lanes::Seg{0, 0, 0});
    } catch (...) {
        return ICELK_ENOMEM;
    }
    size_t pos = scan;
    for (uint32_t s = 0; s < A.nseg; s++) {
        const size_t end = next_marker(d, len, pos);
        X.seg[s].begin = (uint32_t)pos;
        X.seg[s].end = (uint32_t)end;
        if (s + 1 < A.nseg) {
            size_t m = end;
            while (m + 1 < len && d[m] == 0xFF && d[m + 1] == 0xFF) m++;   // fill bytes in front of the marker
            if (m + 1 >= len || d[m] != 0xFF || d[m + 1] != 0xD0 + (s & 7)) return ICELK_EARG;
            pos = m + 2;
        }
    }
    return ICELK_OK;
}

// jpeg_index, or the news that only the serial decoder takes the file: the lanes' positions are 32 bits, so for a file of
// 256 MiB or more *host_only is set and *info alone is filled (icelk_jpeg_describe)
int jpeg_open_core(const uint8_t* data, uint64_t len, JpegIndex& X, icelk_jpeg_info_t* info, bool* host_only)
{
    int rc = jpeg_index(data, (size_t)len, X);
    *host_only = rc == ICELK_EUNSUP && len >= ((uint64_t)1 << 28);
    if (*host_only) return icelk_jpeg_describe(data, len, info);
    if (!rc) *info = X.info;
    return rc;
}

// cuts the segments into lanes of S bits
void jpeg_index_lanes(JpegIndex& X, uint32_t S, int max_hops)
{
    uint32_t lane = 0;
    for (uint32_t s = 0; s < X.scan.nseg; s++) {
        X.seg[s].lane0 = lane;
        const uint64_t bits = (uint64_t)(X.seg[s].end - X.seg[s].begin) * 8;
        lane += bits ? (uint32_t)((bits + S - 1) / S) : 1;
    }
    X.seg[X.scan.nseg].lane0 = lane;
    X.scan.nlanes = lane;
    X.scan.S = S;
    X.scan.max_hops = max_hops;
}

bool jpeg_huff_config_ok(int subseq_bits, int max_hops, int max_rounds)
{
    return subseq_bits >= 32 && subseq_bits % 32 == 0 && subseq_bits <= (1 << 20) && max_hops >= 1 && max_rounds >= 1 &&
           max_rounds <= kJpegMaxRounds;
}

int jpeg_host_decode(const uint8_t* data, size_t len, int16_t* coef, uint64_t capacity)
{
    return icelk_jpeg_read_coefficients(data, (uint64_t)len, coef, capacity);
}

namespace {

// the DC differences of every component summed up in scan order, from zero at every restart interval
void dc_pass_host(const lanes::Scan& A, int16_t* coef)
{
    const uint32_t ri = A.seg_blocks ? A.seg_blocks / (uint32_t)A.bpm : (uint32_t)A.nmcu;
    int32_t pred[3] = {0, 0, 0};
    uint32_t g = 0;
    for (uint32_t mcu = 0; mcu < (uint32_t)A.nmcu; mcu++) {
        if (mcu % ri == 0) pred[0] = pred[1] = pred[2] = 0;
        for (int b = 0; b < A.bpm; b++, g++) {
            const int c = (A.comp_pack >> (2 * b)) & 3;
            int16_t* p = coef + lanes::block_base(A, g);
            pred[c] += *p;
            *p = (int16_t)pred[c];
        }
    }
}

// The phases of k_jpeg_huff.hip, one lane after the other.  false: the work bound was hit, nothing was written.
bool lanes_decode_host(const uint8_t* data, JpegIndex& X, int max_rounds, int16_t* coef, icelk_jpeg_huff_stats_t& st, bool* irregular)
{
    using namespace lanes;
    const Scan& A = X.scan;
    const Seg* seg = X.seg.data();
    const uint32_t n = A.nlanes, ngroups = (n + kGroup - 1) / kGroup;
    std::vector<uint64_t> T(n), Xs[2];
    std::vector<uint32_t> cnt(n, 0), P(n + 1, 0);
    std::vector<Chain> ch(kGroup);
    Xs[0].assign(ngroups, kNoState);
    Xs[1].assign(ngroups, kNoState);
    st.segments = A.nseg;
    st.subsequences = n;
    bool bound = false;
    auto run_steps = [&](uint32_t g, uint32_t first_active, uint32_t last_active, uint64_t* x_out) {
        const uint32_t g0 = g * kGroup, g1 = std::min(n, g0 + kGroup);
        for (uint32_t h = 0; h < (uint32_t)kGroup; h++) {
            bool any = false;
            for (uint32_t i = first_active; i < last_active; i++) any |= ch[i - g0].active;
            if (!any) break;
            for (uint32_t i = first_active; i < last_active; i++)
                sync_step(A, X.tabs, data, seg, g0, g1, T.data() + g0, cnt.data() + g0, x_out, i, h, ch[i - g0]);
        }
        for (uint32_t i = first_active; i < last_active; i++) {
            const Chain& c = ch[i - g0];
            st.total_hops += c.hops;
            st.max_hops = std::max(st.max_hops, c.hops);
            bound |= c.bound;
        }
    };
    // round 0: every lane from its guess
    for (uint32_t g = 0; g < ngroups; g++) {
        const uint32_t g0 = g * kGroup, g1 = std::min(n, g0 + kGroup);
        for (uint32_t i = g0; i < g1; i++) {
            Chain& c = ch[i - g0];
            c.s = T[i] = initial_state(A, data, seg, i, &c.seg);
            c.hops = 0;
            c.active = true;
            c.bound = false;
        }
        run_steps(g, g0, g1, &Xs[0][g]);
    }
    st.rounds = 1;
    // rounds 1 ..: a group whose entry the group in front has changed runs one chain from its first lane
    bool settled = false;
    for (int r = 1; r <= max_rounds && !bound; r++) {
        std::vector<uint64_t>&prev = Xs[(r - 1) & 1], &cur = Xs[r & 1];
        bool changed = false;
        cur[0] = prev[0];
        for (uint32_t g = 1; g < ngroups; g++) {
            const uint32_t g0 = g * kGroup;
            cur[g] = prev[g];
            const uint64_t e = prev[g - 1];
            if (e == kNoState || e == T[g0]) continue;
            changed = true;
            Chain& c = ch[0];
            c.s = T[g0] = e;
            c.seg = segment_of(seg, A.nseg, g0);
            c.hops = 0;
            c.active = true;
            c.bound = false;
            run_steps(g, g0, g0 + 1, &cur[g]);
        }
        if (!changed) {
            settled = true;
            break;
        }
        st.rounds++;
    }
    if (bound || !settled) return false;
    // phase 2: blocks completed in front of every lane
    for (uint32_t j = 0; j < n; j++) P[j + 1] = P[j] + cnt[j];
    // phase 3
    *irregular = false;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t s = segment_of(seg, A.nseg, j);
        const LaneReport rep = write_lane(A, X.tabs, data, seg, j, T[j], P[j] - P[seg[s].lane0], coef);
        *irregular |= rep.irregular;
        st.lanes_in_step += rep.in_step;
        st.spanning_blocks += rep.spans;
    }
    if (!*irregular) dc_pass_host(A, coef);
    return true;
}

}  // namespace

// the descriptor a caller hands to the device entry points is checked against what its first five fields imply
bool jpeg_info_ok(const icelk_jpeg_info_t& in)
{
    if (in.width < 3 || in.height < 1 || in.width > 65535 || in.height > 65535) return false;
    if (!sampling_ok(in.ncomp, in.hmax, in.vmax)) return false;
    icelk_jpeg_info_t t = in;
    fill_layout(t);
    if (t.mcus_x != in.mcus_x || t.mcus_y != in.mcus_y || t.coef_count != in.coef_count) return false;
    for (int c = 0; c < 3; c++)
        if (t.comp_w[c] != in.comp_w[c] || t.comp_h[c] != in.comp_h[c] || t.blocks_x[c] != in.blocks_x[c] ||
            t.blocks_y[c] != in.blocks_y[c] || t.coef_offset[c] != in.coef_offset[c])
            return false;
    return true;
}

}  // namespace icelk

using namespace icelk;

extern "C" {

int icelk_jpeg_describe(const uint8_t* data, uint64_t len, icelk_jpeg_info_t* info)
{
    if (!data || !info) return ICELK_EARG;
    Parsed* P = new (std::nothrow) Parsed;
    if (!P) return ICELK_ENOMEM;
    const int rc = parse_headers(data, (size_t)len, *P);
    if (!rc) *info = P->I;
    delete P;
    return rc;
}

int icelk_jpeg_read_coefficients(const uint8_t* data, uint64_t len, int16_t* coef, uint64_t capacity)
{
    if (!data || !coef) return ICELK_EARG;
    Parsed* P = new (std::nothrow) Parsed;
    if (!P) return ICELK_ENOMEM;
    int rc = parse_headers(data, (size_t)len, *P);
    if (!rc && capacity < P->I.coef_count) rc = ICELK_ECAP;
    if (!rc) rc = decode_scan(data, (size_t)len, *P, coef);
    delete P;
    return rc;
}

int icelk_jpeg_index(const uint8_t* data, uint64_t len, icelk_jpeg_info_t* info, icelk_jpeg_scan_t* scan, uint32_t* seg_begin,
                     uint32_t* seg_end, uint64_t seg_capacity, void* tables)
{
    if (!data || !info || !scan) return ICELK_EARG;
    JpegIndex* X = new (std::nothrow) JpegIndex;
    if (!X) return ICELK_ENOMEM;
    int rc = jpeg_index(data, (size_t)len, *X);
    if (!rc) {
        *info = X->info;
        memset(scan, 0, sizeof(*scan));
        scan->segments = X->scan.nseg;
        scan->blocks_per_mcu = (uint32_t)X->scan.bpm;
        scan->blocks_per_segment = X->scan.seg_blocks;
        scan->total_blocks = X->scan.total_blocks;
        for (int b = 0; b < X->scan.bpm; b++) {
            scan->component[b] = (uint8_t)((X->scan.comp_pack >> (2 * b)) & 3);
            scan->dc_table[b] = (uint8_t)((X->scan.dc_pack >> (2 * b)) & 3);
            scan->ac_table[b] = (uint8_t)((X->scan.ac_pack >> (2 * b)) & 3);
        }
        if (seg_begin && seg_end) {
            if (seg_capacity < X->scan.nseg) rc = ICELK_ECAP;
            for (uint32_t s = 0; !rc && s < X->scan.nseg; s++) {
                seg_begin[s] = X->seg[s].begin;
                seg_end[s] = X->seg[s].end;
            }
        }
        if (!rc && tables) memcpy(tables, X->tabs, sizeof(X->tabs));
    }
    delete X;
    return rc;
}

int icelk_jpeg_read_coefficients_lanes(const uint8_t* data, uint64_t len, int16_t* coef, uint64_t capacity, int subseq_bits,
                                       int max_hops, int max_rounds, icelk_jpeg_huff_stats_t* stats)
{
    if (!data || !coef || !jpeg_huff_config_ok(subseq_bits, max_hops, max_rounds)) return ICELK_EARG;
    icelk_jpeg_huff_stats_t st;
    memset(&st, 0, sizeof(st));
    JpegIndex* X = new (std::nothrow) JpegIndex;
    if (!X) return ICELK_ENOMEM;
    icelk_jpeg_info_t info;
    bool host_only = false;
    int rc = jpeg_open_core(data, len, *X, &info, &host_only);
    if (host_only) {
        delete X;
        st.fallback = ICELK_JPEG_FALLBACK_SIZE;
        if (stats) *stats = st;
        return icelk_jpeg_read_coefficients(data, len, coef, capacity);
    }
    if (!rc && capacity < X->info.coef_count) rc = ICELK_ECAP;
    if (!rc) {
        bool irregular = false, done = false;
        try {
            jpeg_index_lanes(*X, (uint32_t)subseq_bits, max_hops);
            memset(coef, 0, (size_t)X->info.coef_count * sizeof(int16_t));
            done = lanes_decode_host(data, *X, max_rounds, coef, st, &irregular);
        } catch (...) {
            rc = ICELK_ENOMEM;
        }
        if (!rc && (!done || irregular)) {
            st.fallback = done ? ICELK_JPEG_FALLBACK_STREAM : ICELK_JPEG_FALLBACK_BOUND;
            rc = icelk_jpeg_read_coefficients(data, len, coef, capacity);
        }
    }
    delete X;
    if (stats) *stats = st;
    return rc;
}

}  // extern "C"
