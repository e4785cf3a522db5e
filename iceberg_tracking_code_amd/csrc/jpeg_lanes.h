// jpeg_lanes.h -- decoding a baseline JPEG's entropy-coded data in parallel lanes by self-synchronisation (Weissenberger
// and Schmidt, "Accelerating JPEG Decompression on GPUs"), as plain C++ for the host and the device alike.  The device
// kernels (k_jpeg_huff.hip) and the serial host statement (icelk_jpeg_read_coefficients_lanes, abi_jpeg.hip) both run
// exactly the functions below; only who calls them in which order differs.
//
// Segments and lanes.  A segment is the entropy-coded data between two markers: the whole scan, or one restart interval.
// It is cut into subsequences of S bits of the RAW stream (stuffed zeros included), one lane each; the lanes of all
// segments are numbered through.  The state of a decoder between two symbols is (p, b, k): p the raw bit position of the
// next symbol inside the segment, b the block's index inside the MCU (it selects the tables), k the zigzag position
// (0: a DC code comes next).  A position never stands inside a stuffed zero: passing the last bit of a data byte FF
// also passes the zero behind it.
//
// F = decode<false>: from a state, every symbol that starts in front of a limit; returns the state behind them and the
// blocks completed.  It is total: an impossible code consumes one bit and changes nothing else, a DC category above 15
// counts as 0, a run past coefficient 63 ends the block, bits behind the segment's end are zeros.  Every step consumes
// at least one bit, so the loop ends.
//
// Synchronisation (sync_step).  Lanes are grouped by kGroup consecutive lanes.  Entry state T[j] of lane j: known for
// the first lane of a segment, a guess (its own first bit, b = k = 0) for the others.  In lockstep step h lane i decodes
// subsequence i + h from the state its chain has reached and compares what comes out with T[i + h + 1]: equal, and the
// chain has fallen in step with the one in front and stops; different, and it overwrites the entry and goes on.  In one
// step every entry is touched by one chain only.  A chain that reaches the group's end leaves its state as the group's
// exit X; the next ROUND hands it to the following group, where one chain starts again from the first lane if the entry
// changes.  When a round changes nothing, every T is the true state, by induction from the first lane of the segment,
// whatever F made of the garbage in between.
#pragma once
#include <stdint.h>

#define ICELK_LANES_FN __host__ __device__ __forceinline__

namespace icelk {
namespace lanes {

constexpr int kLookBits = 9;
constexpr int kGroup = 256;            // lanes per synchronisation group = threads per workgroup
constexpr uint64_t kNoState = ~0ull;

// one Huffman table in the form both decoders read: 1416 bytes
struct HuffTable {
    uint16_t look[1 << kLookBits];   // code length << 8 | symbol for codes of up to kLookBits bits, 0: a longer code
    int32_t maxcode[17];             // largest code of each length, -1: none
    int32_t valoff[17];              // index of a length's first symbol minus its first code
    uint8_t vals[256];
};
constexpr int kTables = 8;             // DC 0..3, AC 0..3

struct Seg {
    uint32_t begin, end;   // bytes of the file: [begin, end) holds the segment's data, a marker or the file's end follows
    uint32_t lane0;        // its first lane; the table ends with a sentinel {0, 0, lanes in all}
};

// what a lane has to know about the scan; small fields packed 2 bits per block of the MCU so that nothing is indexed
// by a lane's own value in a by-value kernel argument
struct Scan {
    uint32_t S;                 // bits per subsequence
    uint32_t nlanes, nseg;
    int32_t bpm;                // blocks per MCU (1, 3, 4 or 6)
    uint32_t seg_blocks;        // blocks per restart interval, 0: one segment
    uint32_t total_blocks;
    int32_t mcus_x, nmcu;
    uint32_t comp_pack, dc_pack, ac_pack, u_pack, v_pack;   // per block of the MCU: component, tables, place in the MCU
    int32_t hs, vs;             // luma blocks per MCU across and down
    int32_t blocks_x0, blocks_x1;
    uint64_t off0, off1, off2;  // coef_offset of the three components
    int32_t max_hops;
};

// natural (row-major) index of the k-th coefficient in zigzag order
ICELK_LANES_FN int natural(int k)
{
    const uint8_t nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return nat[k & 63];
}

ICELK_LANES_FN uint64_t pack_state(uint32_t p, int b, int k) { return (uint64_t)p | (uint64_t)b << 32 | (uint64_t)k << 40; }

// the segment of lane j: the last one whose lane0 <= j (binary search; seg[nseg] is the sentinel)
ICELK_LANES_FN uint32_t segment_of(const Seg* seg, uint32_t nseg, uint32_t j)
{
    uint32_t lo = 0, hi = nseg;   // seg[lo].lane0 <= j < seg[hi].lane0
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg[mid].lane0 <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// element index of coefficient 0 of block g (scan order over the whole image)
ICELK_LANES_FN uint64_t block_base(const Scan& A, uint32_t g)
{
    const uint32_t mcu = g / (uint32_t)A.bpm, b = g - mcu * (uint32_t)A.bpm;
    const uint32_t my = mcu / (uint32_t)A.mcus_x, mx = mcu - my * (uint32_t)A.mcus_x;
    const uint32_t c = (A.comp_pack >> (2 * b)) & 3, u = (A.u_pack >> (2 * b)) & 3, v = (A.v_pack >> (2 * b)) & 3;
    const uint32_t hs = c == 0 ? A.hs : 1, vs = c == 0 ? A.vs : 1;
    const uint64_t blk = (uint64_t)(my * vs + v) * (uint32_t)(c == 0 ? A.blocks_x0 : A.blocks_x1) + (mx * hs + u);
    return (c == 0 ? A.off0 : (c == 1 ? A.off1 : A.off2)) + blk * 64;
}

typedef uint32_t u32_a1 __attribute__((aligned(1)));

// The bit reader of one lane, on the raw bytes d[0 .. end) of its segment.  `acc` holds n valid bits at its top, `sm`
// moves with it and has a one at the last bit of every data byte FF whose stuffed zero was skipped: `head`, the raw
// position of the next bit, jumps 8 further when such a bit is dropped.  Behind the end zeros are fed.
struct Reader {
    const uint8_t* d;
    uint32_t bp, end, head;
    uint64_t acc, sm;
    int n;

    ICELK_LANES_FN void fill()   // afterwards n >= 32
    {
        if (n >= 32) return;
        if (bp + 4 <= end) {
            const uint32_t w = __builtin_bswap32(*reinterpret_cast<const u32_a1*>(d + bp));
            const uint32_t inv = ~w;   // a byte FF in w is a zero byte in inv
            if (!((inv - 0x01010101u) & ~inv & 0x80808080u)) {
                acc |= (uint64_t)w << (32 - n);
                n += 32;
                bp += 4;
                return;
            }
        }
        while (n <= 56) {
            if (bp < end) {
                const uint32_t b = d[bp];
                if (b != 0xFF) {
                    bp++;
                    acc |= (uint64_t)b << (56 - n);
                    n += 8;
                    continue;
                }
                if (bp + 1 < end && d[bp + 1] == 0) {
                    bp += 2;
                    acc |= (uint64_t)0xFF << (56 - n);
                    sm |= (uint64_t)1 << (56 - n);
                    n += 8;
                    continue;
                }
                bp = end;   // an FF without its zero: the segment's data ends in front of it
            }
            n += 8;
        }
    }
    ICELK_LANES_FN uint32_t peek(int k) const { return (uint32_t)(acc >> (64 - k)); }   // 1 <= k <= 32
    ICELK_LANES_FN void drop(int k)                                                    // 1 <= k <= 32, k <= n
    {
        head += (uint32_t)k + 8u * (uint32_t)__builtin_popcountll(sm >> (64 - k));
        acc <<= k;
        sm <<= k;
        n -= k;
    }
    ICELK_LANES_FN void start(const uint8_t* seg, uint32_t nbytes, uint32_t p)   // p: a position outside stuffed zeros
    {
        d = seg;
        end = nbytes;
        bp = p >> 3;
        if (bp > end) bp = end;
        head = p & ~7u;
        acc = sm = 0;
        n = 0;
        if (p & 7) {
            fill();
            drop((int)(p & 7));
        }
    }
};

// the guess a lane starts from: the first bit of its subsequence, or of the next byte when that one is a stuffed zero
ICELK_LANES_FN uint64_t guess_state(const uint8_t* seg, uint32_t nbytes, uint32_t first_bit)
{
    const uint32_t q = first_bit >> 3;
    if (q > 0 && q < nbytes && seg[q] == 0 && seg[q - 1] == 0xFF) first_bit += 8;
    return pack_state(first_bit, 0, 0);
}

// one Huffman symbol; at least 16 bits are in the accumulator.  -1: no such code, one bit consumed
ICELK_LANES_FN int symbol(Reader& R, const HuffTable& H)
{
    const uint32_t e = H.look[R.peek(kLookBits)];
    if (e) {
        R.drop((int)(e >> 8));
        return (int)(e & 255);
    }
    const int32_t v = (int32_t)R.peek(16);
    for (int len = kLookBits + 1; len <= 16; len++) {
        const int32_t code = v >> (16 - len);
        if (code <= H.maxcode[len]) {
            const int idx = H.valoff[len] + code;
            if (idx < 0 || idx > 255) break;
            R.drop(len);
            return H.vals[idx];
        }
    }
    R.drop(1);
    return -1;
}

// s more bits as a signed value (T.81 F.2.2.1 EXTEND); 1 <= s <= 15
ICELK_LANES_FN int receive_extend(Reader& R, int s)
{
    const int v = (int)R.peek(s);
    R.drop(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// what the write phase of one lane adds to the decode loop
struct Writer {
    int16_t* coef;         // the whole zero-filled buffer
    uint32_t g, g_end;     // the block in progress, the first block behind the lane's segment
    uint32_t seg_bits;
    uint32_t done_at;      // where the segment's last block ended (valid once g == g_end)
    bool bad;              // an impossible code, category or run, or bits taken from behind the segment's end
    bool began;            // the block in progress began in this lane
};

// Decodes from state `st` every symbol that starts in front of raw bit `limit` of the segment; returns the state behind
// them, *completed = blocks ended.  Writing: non-zero coefficients go to their place (DC as the difference), and the
// lane stops at the block its segment ends with.
template <bool kWrite>
ICELK_LANES_FN uint64_t decode(const Scan& A, const HuffTable* tabs, const uint8_t* seg, uint32_t nbytes, uint32_t limit,
                               uint64_t st, uint32_t* completed, Writer* W)
{
    uint32_t p = (uint32_t)st;
    int b = (int)((st >> 32) & 7), k = (int)((st >> 40) & 63);
    if (b >= A.bpm) b = 0;
    uint32_t done = 0;
    if (p < limit && (!kWrite || W->g < W->g_end)) {
        Reader R;
        R.start(seg, nbytes, p);
        int16_t* blk = nullptr;
        if (kWrite) blk = W->coef + block_base(A, W->g);
        while (R.head < limit) {
            R.fill();
            bool ends = false;
            if (k == 0) {
                int s = symbol(R, tabs[(A.dc_pack >> (2 * b)) & 3]);
                if (s < 0 || s > 15) {
                    if (kWrite) W->bad = true;
                    s = 0;
                }
                const int v = s ? receive_extend(R, s) : 0;
                if (kWrite) {
                    if (v) blk[0] = (int16_t)v;
                    W->began = true;
                }
                k = 1;
            } else {
                const int rs = symbol(R, tabs[4 + ((A.ac_pack >> (2 * b)) & 3)]);
                if (rs < 0) {
                    if (kWrite) W->bad = true;
                } else {
                    const int r = rs >> 4, s = rs & 15;
                    if (s == 0) {
                        if (r == 15) {
                            k += 16;
                            ends = k >= 64;
                        } else {
                            ends = true;
                        }
                    } else {
                        k += r;
                        if (k > 63) {
                            if (kWrite) W->bad = true;
                            ends = true;
                        } else {
                            const int v = receive_extend(R, s);
                            if (kWrite) blk[natural(k)] = (int16_t)v;
                            k++;
                            ends = k == 64;
                        }
                    }
                }
            }
            if (ends) {
                k = 0;
                b = b + 1 == A.bpm ? 0 : b + 1;
                done++;
                if (kWrite) {
                    if (R.head > W->seg_bits) W->bad = true;
                    W->began = false;
                    W->g++;
                    if (W->g >= W->g_end) {
                        W->done_at = R.head;
                        p = R.head;
                        *completed = done;
                        return pack_state(p, b, k);
                    }
                    blk = W->coef + block_base(A, W->g);
                }
            }
        }
        p = R.head;
    }
    *completed = done;
    return pack_state(p, b, k);
}

// raw bits of segment s, and the limit of lane j inside it
ICELK_LANES_FN uint32_t seg_bits_of(const Seg& s) { return (s.end - s.begin) * 8u; }
ICELK_LANES_FN uint32_t lane_limit(const Scan& A, const Seg& s, uint32_t j)
{
    const uint64_t e = (uint64_t)(j - s.lane0 + 1) * A.S;
    const uint32_t bits = seg_bits_of(s);
    return e < bits ? (uint32_t)e : bits;
}

// ---- phase 1 ---------------------------------------------------------------------------------------------------------
// the chain a lane carries through the steps of a round
struct Chain {
    uint64_t s;
    uint32_t seg;        // its segment
    uint32_t hops;       // entries overwritten
    bool active, bound;  // bound: it stopped at max_hops without falling in step
};

// T and cnt are the group's own: T[j - g0], cnt[j - g0] for the lanes g0 <= j < g1 (LDS on the device).  Step h of lane i.
ICELK_LANES_FN void sync_step(const Scan& A, const HuffTable* tabs, const uint8_t* data, const Seg* seg, uint32_t g0, uint32_t g1,
                              uint64_t* T, uint32_t* cnt, uint64_t* x_out, uint32_t i, uint32_t h, Chain& c)
{
    if (!c.active) return;
    const uint32_t j = i + h;
    const Seg sg = seg[c.seg];
    uint32_t n = 0;
    const uint64_t e = decode<false>(A, tabs, data + sg.begin, sg.end - sg.begin, lane_limit(A, sg, j), c.s, &n, nullptr);
    cnt[j - g0] = n;
    const uint32_t nx = j + 1;
    c.active = false;
    if (nx == seg[c.seg + 1].lane0) return;   // the end of the segment (the sentinel ends the last one)
    if (nx == g1) {
        *x_out = e;                               // the next round hands it to the following group
        return;
    }
    if (T[nx - g0] == e) return;                  // in step with the chain in front
    T[nx - g0] = e;
    c.s = e;
    c.hops++;
    if ((int32_t)c.hops >= A.max_hops) c.bound = true;
    else c.active = true;
}

// the state lane j starts round 0 from
ICELK_LANES_FN uint64_t initial_state(const Scan& A, const uint8_t* data, const Seg* seg, uint32_t j, uint32_t* seg_out)
{
    const uint32_t s = segment_of(seg, A.nseg, j);
    *seg_out = s;
    if (j == seg[s].lane0) return pack_state(0, 0, 0);
    const uint64_t first = (uint64_t)(j - seg[s].lane0) * A.S;
    return guess_state(data + seg[s].begin, seg[s].end - seg[s].begin, (uint32_t)first);
}

// ---- phase 3 ---------------------------------------------------------------------------------------------------------
struct LaneReport {
    bool irregular;      // the stream contradicts itself here: the host decoder has the last word on this file
    bool in_step;        // the lane's guess was the true state
    bool spans;          // a block began here and did not end here
};

// first: blocks completed by the lanes of the same segment in front of this one (phase 2)
ICELK_LANES_FN LaneReport write_lane(const Scan& A, const HuffTable* tabs, const uint8_t* data, const Seg* seg, uint32_t j, uint64_t st,
                                     uint32_t first, int16_t* coef)
{
    const uint32_t s = segment_of(seg, A.nseg, j);
    const Seg sg = seg[s];
    const bool last_lane = j + 1 == seg[s + 1].lane0;
    Writer W;
    W.coef = coef;
    const uint64_t g_seg = (uint64_t)s * A.seg_blocks;
    const uint64_t g_end = A.seg_blocks && g_seg + A.seg_blocks < A.total_blocks ? g_seg + A.seg_blocks : A.total_blocks;
    const uint64_t g = g_seg + first;
    W.g_end = (uint32_t)g_end;
    W.g = g < g_end ? (uint32_t)g : (uint32_t)g_end;
    W.seg_bits = seg_bits_of(sg);
    W.done_at = 0;
    W.bad = false;
    W.began = false;
    const bool was_open = W.g < W.g_end;
    uint32_t n = 0;
    const uint64_t e = decode<true>(A, tabs, data + sg.begin, sg.end - sg.begin, lane_limit(A, sg, j), st, &n, &W);
    LaneReport r;
    r.irregular = was_open && W.bad;
    if (was_open && W.g >= W.g_end) {
        // the segment's blocks end here.  Behind them only padding may stand in front of the marker; what the file's last
        // segment is followed by, nobody looks at
        // (padding ones can fill a byte to FF: its stuffed zero is no data either)
        const uint32_t nbytes = sg.end - sg.begin;
        const bool stuffed_end = nbytes >= 2 && data[sg.end - 1] == 0 && data[sg.end - 2] == 0xFF;
        if (W.done_at > W.seg_bits) r.irregular = true;
        else if (s + 1 < A.nseg && W.done_at + 8 + (stuffed_end ? 8 : 0) <= W.seg_bits) r.irregular = true;
    }
    if (last_lane && W.g < W.g_end) r.irregular = true;   // the data ends in front of the blocks
    uint32_t sx;
    r.in_step = initial_state(A, data, seg, j, &sx) == st;
    r.spans = W.g < W.g_end && W.began && ((e >> 40) & 63) != 0;
    return r;
}

}  // namespace lanes
}  // namespace icelk
