// recip_exact_main.hip -- a program of its own (nothing of the library in it but csrc/lk_uniform_math.h): runs recip_exact
// and __fdiv_rn(1.f, x) on the device over EVERY float bit pattern of the range the tracker's D can lie in, and
// floor_to_int against (int)floorf(x) over every bit pattern that is not a NaN, and counts the results that differ bit for
// bit.  (On a NaN the two differ, and the tracker relies on the one instruction's value failing its origin test:
// tests/test_gpu_lk_floors.py judges that against the oracle.  What it makes of the quiet NaN 0x7fc00000 is printed here
// for the record.)
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-fast-math -I<csrc> recip_exact_main.hip -o recip_exact_main
// Prints the ranges and the counts; exit status 0 only if both counts are 0.
#include <cstdio>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "lk_uniform_math.h"

using namespace icelk::lk;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

// out[0]: mismatches, out[1]: the first mismatching bit pattern + 1 (the smallest one, by atomicMin on its complement)
__global__ void k_recip(uint32_t lo, uint32_t hi, unsigned long long* out)
{
    const unsigned long long n = (unsigned long long)hi - lo + 1ull;
    unsigned long long bad = 0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n;
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const float x = __uint_as_float(lo + (uint32_t)i);
        if (__float_as_uint(recip_exact(x)) != __float_as_uint(__fdiv_rn(1.f, x))) {
            bad++;
            atomicMin(&out[1], (unsigned long long)(lo + (uint32_t)i));
        }
    }
    if (bad) atomicAdd(&out[0], bad);
}

__global__ void k_floor(unsigned long long* out)
{
    unsigned long long bad = 0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < (1ull << 32);
         i += (unsigned long long)gridDim.x * blockDim.x) {
        const float x = __uint_as_float((uint32_t)i);
        if (x != x) {
            if ((uint32_t)i == 0x7fc00000u) out[2] = (unsigned long long)(uint32_t)floor_to_int(x);
            continue;
        }
        if (floor_to_int(x) != (int)floorf(x)) {
            bad++;
            atomicMin(&out[1], i);
        }
    }
    if (bad) atomicAdd(&out[0], bad);
}

int main()
{
    unsigned long long* d = nullptr;
    unsigned long long h[5] = {0ull, ~0ull, 0ull, ~0ull, 0ull};
    CHECK(hipMalloc(&d, sizeof(h)));
    CHECK(hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_recip, dim3(4096), dim3(256), 0, 0, RECIP_LO_BITS, RECIP_HI_BITS, d);
    hipLaunchKernelGGL(k_floor, dim3(4096), dim3(256), 0, 0, d + 2);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
    CHECK(hipFree(d));
    printf("reciprocal: bits 0x%08x .. 0x%08x (2^-23 .. 2^32), %llu values, mismatches %llu", RECIP_LO_BITS, RECIP_HI_BITS,
           (unsigned long long)RECIP_HI_BITS - RECIP_LO_BITS + 1ull, h[0]);
    if (h[0]) printf(" (first at 0x%08llx)", h[1]);
    printf("\nfloor: bits 0x00000000 .. 0xffffffff without the NaNs, %llu values, mismatches %llu", (1ull << 32) - (1ull << 24) + 2ull, h[2]);
    if (h[2]) printf(" (first at 0x%08llx)", h[3]);
    printf("\nfloor of the quiet NaN: %d\n", (int)(uint32_t)h[4]);
    return h[0] == 0 && h[2] == 0 ? 0 : 1;
}
