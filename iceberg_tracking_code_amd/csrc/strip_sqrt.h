// strip_sqrt.h -- the correctly rounded float32 square root from a seed within one ulp of it, for radicands in a stated band.
//
// k_eig_strip (k_corners.hip) takes the root of (a - c)^2 + b^2 once per pixel.  sqrtf on gfx950 is v_sqrt_f32 (accurate to
// 1 ulp) followed by a correction, wrapped in a range scaling for radicands below 2^-96 and a test for 0 and infinity.
// In the band the wrapping does nothing, and the correction alone is the whole of it:
//
//     s  = seed, within 1 ulp of sqrt(x);  sd, su = the floats next below and above s
//     rd = fma(-sd, s, x),  ru = fma(-su, s, x)          each rounded once
//     rd <= 0  ->  sd;   ru > 0  ->  su;   otherwise s
//
// rd <= 0 says x <= sd * s, the square of the geometric mean of sd and s, which lies below their midpoint by less than any float32
// x can resolve: sqrt(x) rounds to sd (or lower: excluded by the seed's accuracy).  ru > 0 likewise says it rounds to su.
//
// The band [2^-96, 2^64]:
//   lower end  the residuals are about s * ulp(s) ~ x * 2^-23.  For x >= 2^-96 that is >= 2^-119, a normal float, so the sign of
//              a residual is never lost to underflow, and x, s, sd, su are normal too (s >= 2^-48).  It is the threshold below
//              which the compiler's own expansion scales the radicand; v_sqrt_f32 keeps its accuracy far below it.
//   upper end  s * su must not overflow: any x < 2^127 would do.  2^64 is far above the map's range (the box sums are <= 1,
//              the radicand <= 1.25).
// 0, denormals, infinity, NaN and negative radicands are outside; the caller sends them to sqrtf.
// Host and device: tests/strip_sqrt_host_main.cpp feeds sqrt_from_seed every seed the hardware may return.
#pragma once
#include <cmath>
#include <cstdint>

namespace icelk {

constexpr uint32_t SQRT_BAND_LO = 0x0f800000u;   // bits of 2^-96f
constexpr uint32_t SQRT_BAND_HI = 0x5f800000u;   // bits of 2^64f

__host__ __device__ __forceinline__ uint32_t sqrt_bits(float v)
{
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    return b;
}
__host__ __device__ __forceinline__ float sqrt_float(uint32_t b)
{
    float v;
    __builtin_memcpy(&v, &b, 4);
    return v;
}

// x in the band, s within one ulp of sqrt(x): the correctly rounded root.  The two fmaf are explicit (-ffp-contract=off).
__host__ __device__ __forceinline__ float sqrt_from_seed(float x, float s)
{
    const float sd = sqrt_float(sqrt_bits(s) - 1u), su = sqrt_float(sqrt_bits(s) + 1u);
    const float rd = fmaf(-sd, s, x), ru = fmaf(-su, s, x);
    float out = rd <= 0.f ? sd : s;
    out = ru > 0.f ? su : out;
    return out;
}

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ float sqrt_in_band(float x) { return sqrt_from_seed(x, __builtin_amdgcn_sqrtf(x)); }
#else
__device__ __forceinline__ float sqrt_in_band(float x) { return sqrtf(x); }   // host pass of a .hip file: never called
#endif

}  // namespace icelk
