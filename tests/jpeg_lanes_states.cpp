// jpeg_lanes_states.cpp -- the functions of csrc/jpeg_lanes.h called from states that are not the true ones, as plain C++
// under the host's sanitizers (test_jpeg_lanes_states_host.py builds and runs this program; nothing of the library is
// linked).  The asynchronous JPEG ingest (csrc/abi_jpeg_job.hip) cannot stop its chain of kernels when a file hits the
// work bound or does not settle: scan, write and DC pass then run on whatever phase 1 left.  That this stores nothing
// outside the coefficient buffer, reads nothing outside the file and ends is a property of jpeg_lanes.h alone, so it is
// shown here, where an overrun lands in a redzone, and never on a device.
//
//   jpeg_lanes_states PAIRS BLOB...
//
// A blob is what the test writes per file from icelk_jpeg_index (the layout is `Blob::load` below).  Every buffer is a
// heap allocation of exactly the size the device's is.  Per blob and S in {32, 512}:
//   1. the harness as the device's caller: phase 1 under generous bounds, prefix sum, write_lane per lane, DC sums; the
//      coefficients go to BLOB.S<S>.coef and the test compares them with icelk_jpeg_read_coefficients_lanes';
//   2. the device's order on a file that does not settle: phase 1 under max_hops 1 and max_rounds 1, and no stop;
//   3. PAIRS arbitrary (state, first block) pairs per lane through write_lane and decode<false>.
// Prints one line per blob and S and the number of calls of write_lane and decode<false> made; the test knows how many
// that has to be.
#define __host__
#define __device__
#define __forceinline__ inline
#include "../iceberg_tracking_code_amd/csrc/jpeg_lanes.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace icelk::lanes;

namespace {

[[noreturn]] void die(const char* what, const char* arg = "")
{
    fprintf(stderr, "jpeg_lanes_states: %s %s\n", what, arg);
    exit(2);
}

// a heap block of exactly n elements: whatever goes past either end lands in a redzone
template <class T>
T* exact(size_t n)
{
    T* p = static_cast<T*>(malloc(std::max<size_t>(n, 1) * sizeof(T)));
    if (!p) die("no memory");
    return p;
}

struct Blob {
    enum { LEN, NSEG, BPM, SEG_BLOCKS, TOTAL_BLOCKS, MCUS_X, MCUS_Y, HMAX, VMAX, BLOCKS_X0, BLOCKS_X1, OFF0, OFF1, OFF2, COEF_COUNT,
           NCOMP, COMPONENT, DC_TABLE = COMPONENT + 8, AC_TABLE = DC_TABLE + 8, WORDS = AC_TABLE + 8 };
    uint64_t h[WORDS];
    Scan A;                // S, nlanes, max_hops are set per run (set_lanes)
    uint8_t* file;         // h[LEN] bytes
    Seg* seg;              // nseg + 1
    HuffTable* tabs;       // kTables
    uint64_t coef_count;

    // uint64 h[WORDS] | uint32 begin[nseg] | uint32 end[nseg] | the packed tables | the file
    void load(const char* path)
    {
        FILE* f = fopen(path, "rb");
        if (!f) die("cannot open", path);
        std::vector<uint8_t> raw;
        uint8_t buf[1 << 16];
        for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) raw.insert(raw.end(), buf, buf + n);
        fclose(f);
        if (raw.size() < sizeof(h)) die("short blob", path);
        memcpy(h, raw.data(), sizeof(h));
        const size_t nseg = (size_t)h[NSEG], len = (size_t)h[LEN];
        if (raw.size() != sizeof(h) + 8 * nseg + sizeof(HuffTable) * kTables + len) die("blob of the wrong size", path);
        const uint8_t* q = raw.data() + sizeof(h);
        seg = exact<Seg>(nseg + 1);
        for (size_t s = 0; s < nseg; s++) {
            memcpy(&seg[s].begin, q + 4 * s, 4);
            memcpy(&seg[s].end, q + 4 * (nseg + s), 4);
            seg[s].lane0 = 0;
            if (seg[s].begin > seg[s].end || seg[s].end > len) die("segment outside the file", path);
        }
        seg[nseg] = Seg{0, 0, 0};
        q += 8 * nseg;
        tabs = exact<HuffTable>(kTables);
        memcpy(tabs, q, sizeof(HuffTable) * kTables);
        q += sizeof(HuffTable) * kTables;
        file = exact<uint8_t>(len);
        memcpy(file, q, len);
        coef_count = h[COEF_COUNT];
        // the Scan as jpeg_index (csrc/abi_jpeg.hip) fills it
        memset(&A, 0, sizeof(A));
        int b = 0;
        for (int c = 0; c < (int)h[NCOMP]; c++) {
            const int hs = c == 0 ? (int)h[HMAX] : 1, vs = c == 0 ? (int)h[VMAX] : 1;
            for (int v = 0; v < vs; v++)
                for (int u = 0; u < hs; u++, b++) {
                    if (b >= 8 || (int)h[COMPONENT + b] != c) die("the blocks of the MCU are not as the sampling says", path);
                    A.comp_pack |= (uint32_t)c << (2 * b);
                    A.dc_pack |= (uint32_t)h[DC_TABLE + b] << (2 * b);
                    A.ac_pack |= (uint32_t)h[AC_TABLE + b] << (2 * b);
                    A.u_pack |= (uint32_t)u << (2 * b);
                    A.v_pack |= (uint32_t)v << (2 * b);
                }
        }
        if (b != (int)h[BPM]) die("blocks per MCU", path);
        A.bpm = b;
        A.nseg = (uint32_t)nseg;
        A.seg_blocks = (uint32_t)h[SEG_BLOCKS];
        A.total_blocks = (uint32_t)h[TOTAL_BLOCKS];
        A.mcus_x = (int32_t)h[MCUS_X];
        A.nmcu = (int32_t)(h[MCUS_X] * h[MCUS_Y]);
        A.hs = (int32_t)h[HMAX];
        A.vs = (int32_t)h[VMAX];
        A.blocks_x0 = (int32_t)h[BLOCKS_X0];
        A.blocks_x1 = (int32_t)h[BLOCKS_X1];
        A.off0 = h[OFF0];
        A.off1 = h[OFF1];
        A.off2 = h[OFF2];
        if (A.total_blocks != (uint32_t)A.nmcu * (uint32_t)b) die("total blocks", path);
    }

    // jpeg_index_lanes
    void set_lanes(uint32_t S, int max_hops)
    {
        uint32_t lane = 0;
        for (uint32_t s = 0; s < A.nseg; s++) {
            seg[s].lane0 = lane;
            const uint64_t bits = (uint64_t)(seg[s].end - seg[s].begin) * 8;
            lane += bits ? (uint32_t)((bits + S - 1) / S) : 1;
        }
        seg[A.nseg].lane0 = lane;
        A.nlanes = lane;
        A.S = S;
        A.max_hops = max_hops;
    }

    void drop()
    {
        free(file);
        free(seg);
        free(tabs);
    }
};

// the working set of one file on the device (jpeg_huff_setup): T, cnt of nlanes, P of nlanes + 1, X of two rows of groups
struct Work {
    uint32_t n, ngroups;
    uint64_t *T, *X;
    uint32_t *cnt, *P;
    int16_t* coef;
    uint64_t coef_count;

    Work(const Blob& B) : n(B.A.nlanes), ngroups((B.A.nlanes + kGroup - 1) / kGroup), coef_count(B.coef_count)
    {
        T = exact<uint64_t>(n);
        X = exact<uint64_t>(2 * (size_t)ngroups);
        cnt = exact<uint32_t>(n);
        P = exact<uint32_t>((size_t)n + 1);
        coef = exact<int16_t>((size_t)coef_count);
        memset(cnt, 0, n * sizeof(uint32_t));
        memset(coef, 0, (size_t)coef_count * sizeof(int16_t));
    }
    ~Work()
    {
        free(T);
        free(X);
        free(cnt);
        free(P);
        free(coef);
    }
    Work(const Work&) = delete;
    Work& operator=(const Work&) = delete;
};

struct Phase1 {
    uint32_t rounds;
    bool bound, settled;
};

// Phase 1 as lanes_decode_host (csrc/abi_jpeg.hip) runs it.  `as_device`: as the rounds go out in one piece on the device,
// where a chain at the work bound stops nothing: every round 1 .. max_rounds that has something to do runs.
Phase1 phase1(const Blob& B, Work& W, int max_rounds, bool as_device)
{
    const Scan& A = B.A;
    const uint32_t n = W.n;
    std::vector<Chain> ch(kGroup);
    uint64_t* Xs[2] = {W.X, W.X + W.ngroups};
    for (uint32_t g = 0; g < 2 * W.ngroups; g++) W.X[g] = kNoState;
    Phase1 out{1, false, false};
    auto run_steps = [&](uint32_t g, uint32_t first_active, uint32_t last_active, uint64_t* x_out) {
        const uint32_t g0 = g * kGroup, g1 = std::min(n, g0 + kGroup);
        for (uint32_t h = 0; h < (uint32_t)kGroup; h++) {
            bool any = false;
            for (uint32_t i = first_active; i < last_active; i++) any |= ch[i - g0].active;
            if (!any) break;
            for (uint32_t i = first_active; i < last_active; i++)
                sync_step(A, B.tabs, B.file, B.seg, g0, g1, W.T + g0, W.cnt + g0, x_out, i, h, ch[i - g0]);
        }
        for (uint32_t i = first_active; i < last_active; i++) out.bound |= ch[i - g0].bound;
    };
    for (uint32_t g = 0; g < W.ngroups; g++) {
        const uint32_t g0 = g * kGroup, g1 = std::min(n, g0 + kGroup);
        for (uint32_t i = g0; i < g1; i++) {
            Chain& c = ch[i - g0];
            c.s = W.T[i] = initial_state(A, B.file, B.seg, i, &c.seg);
            c.hops = 0;
            c.active = true;
            c.bound = false;
        }
        run_steps(g, g0, g1, &Xs[0][g]);
    }
    for (int r = 1; r <= max_rounds && (as_device || !out.bound); r++) {
        uint64_t *prev = Xs[(r - 1) & 1], *cur = Xs[r & 1];
        bool changed = false;
        if (W.ngroups) cur[0] = prev[0];
        for (uint32_t g = 1; g < W.ngroups; g++) {
            const uint32_t g0 = g * kGroup;
            cur[g] = prev[g];
            const uint64_t e = prev[g - 1];
            if (e == kNoState || e == W.T[g0]) continue;
            changed = true;
            Chain& c = ch[0];
            c.s = W.T[g0] = e;
            c.seg = segment_of(B.seg, A.nseg, g0);
            c.hops = 0;
            c.active = true;
            c.bound = false;
            run_steps(g, g0, g0 + 1, &cur[g]);
        }
        if (!changed) {
            out.settled = true;
            break;
        }
        out.rounds++;
    }
    return out;
}

// phase 2, phase 3 and the DC sums from whatever T and cnt hold (k_jpeg_huff_scan, k_jpeg_huff_write, k_jpeg_dc_*)
uint64_t later_phases(const Blob& B, Work& W)
{
    const Scan& A = B.A;
    W.P[0] = 0;
    for (uint32_t j = 0; j < W.n; j++) W.P[j + 1] = W.P[j] + W.cnt[j];
    uint64_t calls = 0;
    for (uint32_t j = 0; j < W.n; j++) {
        const uint32_t s = segment_of(B.seg, A.nseg, j);
        (void)write_lane(A, B.tabs, B.file, B.seg, j, W.T[j], W.P[j] - W.P[B.seg[s].lane0], W.coef);
        calls++;
    }
    const uint32_t ri = A.seg_blocks ? A.seg_blocks / (uint32_t)A.bpm : (uint32_t)A.nmcu;
    uint32_t pred[3] = {0, 0, 0}, g = 0;   // the device's 32-bit sums wrap; so do these
    for (uint32_t mcu = 0; mcu < (uint32_t)A.nmcu; mcu++) {
        if (mcu % ri == 0) pred[0] = pred[1] = pred[2] = 0;
        for (int b = 0; b < A.bpm; b++, g++) {
            const int c = (A.comp_pack >> (2 * b)) & 3;
            int16_t* p = W.coef + block_base(A, g);
            pred[c] += (uint32_t)(int32_t)*p;
            *p = (int16_t)(uint16_t)pred[c];
        }
    }
    return calls;
}

struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next()
    {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    uint64_t below(uint64_t n) { return n ? next() % n : 0; }   // 0 .. n - 1
};

uint64_t drawn[8];   // how often each kind of p (0..3), kNoState (4) and each kind of `first` (5..7) was drawn

// arbitrary (state, first block) pairs: what no run of phase 1 may ever leave, too
uint64_t arbitrary_states(const Blob& B, Work& W, int pairs, Rng& rng)
{
    const Scan& A = B.A;
    uint64_t calls = 0;
    for (uint32_t j = 0; j < W.n; j++) {
        const uint32_t s = segment_of(B.seg, A.nseg, j);
        const Seg sg = B.seg[s];
        const uint32_t bits = seg_bits_of(sg), limit = lane_limit(A, sg, j);
        const uint64_t lane_first = (uint64_t)(j - sg.lane0) * A.S;
        for (int q = 0; q < pairs; q++) {
            uint32_t p;
            const int kind_p = (int)((j + (uint32_t)q) & 3);
            if (kind_p == 0) p = (uint32_t)(lane_first + rng.below(limit > lane_first ? limit - lane_first : 1));
            else if (kind_p == 1) p = (uint32_t)rng.below((uint64_t)bits + 64);
            else if (kind_p == 2) p = bits - (uint32_t)rng.below(std::min<uint32_t>(bits, 64) + 1);
            else p = (uint32_t)rng.next();
            drawn[kind_p]++;
            uint64_t st = pack_state(p, (int)rng.below(8), (int)rng.below(64));
            if (rng.below(16) == 0) {
                st = kNoState;
                drawn[4]++;
            }
            uint32_t first;
            const int kind_f = (int)rng.below(3);
            if (kind_f == 0) first = (uint32_t)rng.below(2 * (uint64_t)A.total_blocks + 1);
            else if (kind_f == 1) first = A.total_blocks - (uint32_t)rng.below(std::min<uint32_t>(A.total_blocks, 8) + 1);
            else first = (uint32_t)rng.next();
            drawn[5 + kind_f]++;
            (void)write_lane(A, B.tabs, B.file, B.seg, j, st, first, W.coef);
            uint32_t n = 0;
            (void)decode<false>(A, B.tabs, B.file + sg.begin, sg.end - sg.begin, limit, st, &n, nullptr);
            calls += 2;
        }
    }
    return calls;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) die("usage: jpeg_lanes_states PAIRS BLOB...");
    const int pairs = atoi(argv[1]);
    if (pairs < 1) die("PAIRS");
    Rng rng{20191018};
    uint64_t total = 0;
    for (int f = 2; f < argc; f++) {
        Blob B;
        B.load(argv[f]);
        for (uint32_t S : {32u, 512u}) {
            uint64_t calls = 0;
            // 1. the device's caller, as lanes_decode_host
            B.set_lanes(S, 256);
            Phase1 a;
            {
                Work W(B);
                a = phase1(B, W, 255, false);
                calls += later_phases(B, W);
                const std::string path = std::string(argv[f]) + ".S" + std::to_string(S) + ".coef";
                FILE* o = fopen(path.c_str(), "wb");
                if (!o || fwrite(W.coef, sizeof(int16_t), (size_t)W.coef_count, o) != W.coef_count || fclose(o)) die("cannot write", path.c_str());
            }
            // 2. the device's order on a file that does not settle
            B.set_lanes(S, 1);
            Phase1 b;
            {
                Work W(B);
                b = phase1(B, W, 1, true);
                calls += later_phases(B, W);
            }
            // 3. arbitrary states
            B.set_lanes(S, 256);
            {
                Work W(B);
                calls += arbitrary_states(B, W, pairs, rng);
            }
            printf("%s S %u lanes %u rounds %u settled %d | bounds 1, 1: bound %d settled %d | calls %llu\n", argv[f], S, B.A.nlanes,
                   a.rounds, (int)(a.settled && !a.bound), (int)b.bound, (int)b.settled, (unsigned long long)calls);
            total += calls;
        }
        B.drop();
    }
    printf("drawn");
    for (uint64_t d : drawn) printf(" %llu", (unsigned long long)d);
    printf("\ncalls %llu\n", (unsigned long long)total);
    return 0;
}
