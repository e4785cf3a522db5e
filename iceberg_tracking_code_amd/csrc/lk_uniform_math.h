// lk_uniform_math.h -- the short forms of the tracker's wave-uniform scalar math (k_lk_fast.hip), in a header of their own
// so that a stand-alone program (tests/recip_exact_main.hip) can run them over every float they can meet.
#pragma once
#include <hip/hip_runtime.h>

namespace icelk {
namespace lk {

// 1 / d, correctly rounded, for a NORMAL d whose reciprocal is normal too and far from both ends of the exponent range:
// the tracker divides by D only after `D < FLT_EPSILON` has failed, so D >= 2^-23, and D = A11 A22 - A12^2 < 2^32 because
// every sum is below 2^36 (tests/test_lk_limits.py) and carries FLT_SCALE = 2^-20.  In that range neither the scaling
// (v_div_scale x 2, v_div_fmas) nor the fix-up (v_div_fixup) of the compiler's division does anything, and with a numerator
// of 1 its multiply is the identity.  What is left is v_rcp_f32 and Newton steps whose residual 1 - d y is exact (fma).
// v_rcp_f32 alone is the correctly rounded reciprocal for 89 % of the range (49 372 125 of its 461 373 441 floats are
// one ulp off); since it is never further off, ONE step y + (1 - d y) y rounds to the correct float for every one of
// them (Markstein: a reciprocal estimate within an ulp, corrected once with an exact residual, is correctly rounded
// unless the divisor's significand is all ones -- and those come out right here as well).  The exhaustive run on the
// device decides, not the theorem: tests/recip_exact_main.hip counts 0 mismatches against __fdiv_rn(1.f, d) over every
// float of the range.  Three instructions for eleven.
constexpr unsigned RECIP_LO_BITS = 0x34000000u;   // 2^-23
constexpr unsigned RECIP_HI_BITS = 0x4f800000u;   // 2^32
__device__ __forceinline__ float recip_exact(float d)
{
    float y = __builtin_amdgcn_rcpf(d);
    const float e = __builtin_fmaf(-d, y, 1.f);
    return __builtin_fmaf(e, y, y);
}

// (int)floorf(x) in one instruction (v_cvt_flr_i32_f32) for the two the compiler forms (v_floor_f32, v_cvt_i32_f32).  The
// two agree on every float that is not a NaN (tests/recip_exact_main.hip runs all 2^32 - 2^24 + 2 of them): +-inf and
// everything outside int saturate to INT_MAX / INT_MIN, which origin_ok (lk_fast_tiles.h) rejects.  On a NaN they do
// NOT agree (INT_MAX here, 0 there), and only INT_MAX fails the origin test as the oracle's x86 conversion (INT_MIN) does:
// the tracker therefore takes every origin from this one (k_lk_fast.hip, floor_uni), and a NaN point is skipped at every
// level as the oracle skips it.
__device__ __forceinline__ int floor_to_int(float x)
{
    int i;
    asm volatile("v_cvt_flr_i32_f32 %0, %1" : "=v"(i) : "v"(x));
    return i;
}

}  // namespace lk
}  // namespace icelk
