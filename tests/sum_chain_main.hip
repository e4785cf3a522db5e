// sum_chain_main.hip -- a program of its own (nothing of the library in it but csrc/lk_common.h): the tracker's pair chain
// (dpp_pair_steps and the converting read-outs lanes31_63_float_i32 / _u32, "two guarded sums as one chain") on the device,
// one wave per case, against 64-bit sums formed on the host.  Per case and per input four things are compared: the integer
// in lane 31 / 63 with the 64-bit total, the float read out with (float)total * 2^-20 (the host's int64 -> float conversion
// rounds once, to nearest even), and both again for the six-step chain the pair chain stands in for (dpp_all_steps,
// lane63_float_*), so that a difference between the two forms shows as such.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -I<csrc> sum_chain_main.hip -o sum_chain_main
// Cases, all inside the guard of lk_common.h (signed: [-2^25, 2^25) per lane; unsigned: [0, 2^26)):
//   * one lane holds the value, the other 63 and the whole other input hold 0: every lane in turn, either input, signed
//     (2^25 - 1 and -2^25) and unsigned (2^26 - 1): a lane dropped, counted twice or credited to the other sum shows
//   * every lane at -2^25, every lane at 2^25 - 1, one input at each (both ways round); unsigned: every lane at 2^26 - 1
//     (total above 2^31), and one input at that with the other at 0
//   * random vectors: every lane uniform in a range of 2^k, k drawn per input and case (small totals convert exactly,
//     large ones round), 3000 signed and 3000 unsigned
// Prints the counts of cases, of values compared and of mismatches; exit status 0 only if there is no mismatch.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>
#include "lk_common.h"

using namespace icelk::lk;

constexpr float kScale = 1.f / (1 << 20);   // FLT_SCALE of the kernels

// case c: lanes x[64 c ..], y[64 c ..]; out[8 c ..]: pair chain int x, int y, float x, float y, then the same of the six steps
__global__ __launch_bounds__(64) void k_chain(const int* __restrict__ x, const int* __restrict__ y, int is_unsigned, uint32_t* __restrict__ out)
{
    const int lane = threadIdx.x;
    const size_t c = blockIdx.x;
    const int a = x[c * 64 + lane], b = y[c * 64 + lane];
    const int p = dpp_pair_steps(a, b);
    const int sa = dpp_all_steps(a), sb = dpp_all_steps(b);
    float f0, f1, g0, g1;
    if (is_unsigned) {
        lanes31_63_float_u32(p, kScale, f0, f1);
        g0 = lane63_float_u32(sa) * kScale;
        g1 = lane63_float_u32(sb) * kScale;
    } else {
        lanes31_63_float_i32(p, kScale, f0, f1);
        g0 = lane63_float_i32(sa) * kScale;
        g1 = lane63_float_i32(sb) * kScale;
    }
    const int p31 = __builtin_amdgcn_readlane(p, 31), p63 = __builtin_amdgcn_readlane(p, 63);
    const int a63 = __builtin_amdgcn_readlane(sa, 63), b63 = __builtin_amdgcn_readlane(sb, 63);
    if (lane == 0) {
        uint32_t* o = out + c * 8;
        o[0] = (uint32_t)p31; o[1] = (uint32_t)p63; o[2] = __float_as_uint(f0); o[3] = __float_as_uint(f1);
        o[4] = (uint32_t)a63; o[5] = (uint32_t)b63; o[6] = __float_as_uint(g0); o[7] = __float_as_uint(g1);
    }
}

struct Cases {
    std::vector<int> x, y;
    size_t n = 0;
    void add(const int* a, const int* b)
    {
        x.insert(x.end(), a, a + 64);
        y.insert(y.end(), b, b + 64);
        n++;
    }
    void constant(int a, int b)
    {
        int u[64], v[64];
        for (int l = 0; l < 64; l++) { u[l] = a; v[l] = b; }
        add(u, v);
    }
    void single_lanes(int value)
    {
        for (int which = 0; which < 2; which++)
            for (int l = 0; l < 64; l++) {
                int u[64] = {0}, v[64] = {0};
                (which ? v : u)[l] = value;
                add(u, v);
            }
    }
};

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static uint32_t float_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// runs the cases; returns the number of values that differ (negative: a HIP error)
static long long run(const Cases& cs, bool is_unsigned, unsigned long long& values)
{
    int *dx = nullptr, *dy = nullptr;
    uint32_t* dout = nullptr;
    const size_t bytes = cs.n * 64 * sizeof(int);
    std::vector<uint32_t> out(cs.n * 8);
#define CHECKR(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return -1; } } while (0)
    CHECKR(hipMalloc(&dx, bytes));
    CHECKR(hipMalloc(&dy, bytes));
    CHECKR(hipMalloc(&dout, out.size() * sizeof(uint32_t)));
    CHECKR(hipMemcpy(dx, cs.x.data(), bytes, hipMemcpyHostToDevice));
    CHECKR(hipMemcpy(dy, cs.y.data(), bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_chain, dim3((unsigned)cs.n), dim3(64), 0, 0, dx, dy, is_unsigned ? 1 : 0, dout);
    CHECKR(hipGetLastError());
    CHECKR(hipDeviceSynchronize());
    CHECKR(hipMemcpy(out.data(), dout, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CHECKR(hipFree(dx)); CHECKR(hipFree(dy)); CHECKR(hipFree(dout));
#undef CHECKR
    long long bad = 0;
    for (size_t c = 0; c < cs.n; c++) {
        long long t[2] = {0, 0};
        for (int l = 0; l < 64; l++) {
            t[0] += is_unsigned ? (long long)(uint32_t)cs.x[c * 64 + l] : (long long)cs.x[c * 64 + l];
            t[1] += is_unsigned ? (long long)(uint32_t)cs.y[c * 64 + l] : (long long)cs.y[c * 64 + l];
        }
        const uint32_t* o = &out[c * 8];
        for (int k = 0; k < 2; k++) {
            const uint32_t want_i = (uint32_t)(unsigned long long)t[k];      // the total fits 32 bits (signed or unsigned) by the guard
            const uint32_t want_f = float_bits((float)t[k] * kScale);
            const uint32_t got[4] = {o[k], o[2 + k], o[4 + k], o[6 + k]};
            const uint32_t want[4] = {want_i, want_f, want_i, want_f};
            for (int q = 0; q < 4; q++) {
                values++;
                if (got[q] != want[q]) {
                    if (bad < 10)
                        printf("mismatch: %s case %zu input %d %s: got 0x%08x want 0x%08x (total %lld)\n", is_unsigned ? "unsigned" : "signed",
                               c, k, q == 0 ? "pair int" : q == 1 ? "pair float" : q == 2 ? "six-step int" : "six-step float", got[q], want[q], t[k]);
                    bad++;
                }
            }
        }
    }
    return bad;
}

int main()
{
    constexpr int kLo = -(1 << 25), kHi = (1 << 25) - 1, kTop = (1 << 26) - 1;
    Cases s, u;
    s.single_lanes(kHi);
    s.single_lanes(kLo);
    s.constant(kLo, kLo);
    s.constant(kHi, kHi);
    s.constant(kLo, kHi);
    s.constant(kHi, kLo);
    u.single_lanes(kTop);
    u.constant(kTop, kTop);
    u.constant(kTop, 0);
    u.constant(0, kTop);
    for (int i = 0; i < 3000; i++) {
        int a[64], b[64];
        const int ka = 1 + (int)(rng() % 26), kb = 1 + (int)(rng() % 26);      // signed range 2^k around 0, k = 1 .. 26
        for (int l = 0; l < 64; l++) {
            a[l] = (int)(rng() & ((1u << ka) - 1)) - (1 << (ka - 1));
            b[l] = (int)(rng() & ((1u << kb) - 1)) - (1 << (kb - 1));
        }
        s.add(a, b);
        const int ja = 1 + (int)(rng() % 26), jb = 1 + (int)(rng() % 26);      // unsigned range [0, 2^k), k = 1 .. 26
        for (int l = 0; l < 64; l++) {
            a[l] = (int)(rng() & ((1u << ja) - 1));
            b[l] = (int)(rng() & ((1u << jb) - 1));
        }
        u.add(a, b);
    }
    unsigned long long values = 0;
    const long long bs = run(s, false, values);
    if (bs < 0) return 2;
    const long long bu = run(u, true, values);
    if (bu < 0) return 2;
    printf("sum chain: %zu signed cases, %zu unsigned cases, %llu values, mismatches %lld\n", s.n, u.n, values, bs + bu);
    return bs + bu == 0 ? 0 : 1;
}
