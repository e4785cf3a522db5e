// k_corners.hip -- corner detection for gfx950: the Shi-Tomasi response (smaller eigenvalue) or, under icelk_set_detector,
// the Harris response det - k tr^2 of the same covariance sums (harris_of below: the two forms).
//
// Replaces cv2.goodFeaturesToTrack(frame_gray, mask=mask, **feature_params) at
// s1_lucaskanade_tracking.py:437 (s0_1_test_lucaskanade_tracking.py:167).  Arithmetic restated from OpenCV's
// cornerMinEigenVal / goodFeaturesToTrack (OpenCV is not part of /root/reference).
//
// Stages
//   K6+K7 fused (k_eig_strip<BS>, blockSize 3/5/7/10): a workgroup walks down a strip of the frame, one thread per
//         covariance column: Sobel -> covariance products -> blockSize^2 box sums (double sums: column sums
//         rolled down in registers, row sums through LDS) -> min eigenvalue -> 3x3 non-max test, mask, 1-px border ->
//         local maxima appended as 64-bit keys (response key << 32 | y << 16 | x), plus the masked maximum of the map
//         (order-preserving atomicMax).  Neither OpenCV's f32 Dx/Dy/covariance images (5 x 4 B/px) nor the
//         eigenvalue map itself ever exist in HBM unless the map is asked for (icelk_min_eig_map): 1 B/px is read,
//         ~8 B per local maximum written.
//         The quality threshold (max * qualityLevel) is applied to the candidate list afterwards
//         (k_filter): for max > 0,  v > thr && v == dilate3x3(threshold_tozero(eig))  <=>  v > thr && v >= its
//         8 raw neighbours; for max <= 0 OpenCV finds no corner either.  With the Harris response that case is an
//         ordinary one (about half of a textured frame is negative, a pure ramp everywhere) and the cut
//         quality_threshold() returns for it is negative, so it is the candidate kernels that keep it empty: the
//         non-max test of the strip kernel -- one test for its FAST and non-FAST row phases -- lists v > 0 only, and
//         k_nms_collect compares v with a dilated value that is never below 0.
//         (k_corners_fast.hip: the same candidates in two passes, ICELK_TWO_PASS_CORNERS=1.)
//   K6, K7 separate (k_min_eig, k_nms_collect): any other blockSize, ICELK_GENERIC_CORNERS=1 and the arithmetic
//         variants of icelk_set_variant.
//   K8, the selection among these candidates (min distance, top-K pruning, the corner list): k_min_distance.hip.
// Candidates live in per-workgroup regions (region b = the local maxima of a 16-row band of a strip, or of a workgroup's
// band of k_nms_collect; count in blk_count[b]):
// no single-address atomics anywhere on the image-sized passes (one word saturates at ~90 atomics/us on
// gfx950), and the masked maximum is published with a read-guarded atomicMax.
// The key format, the quality threshold and the constants the stages share: corner_keys.h.
#include <algorithm>
#include <climits>
#include <cstdlib>

#include "corner_keys.h"
#include "strip_sqrt.h"

namespace icelk {

namespace {

// Sobel (ksize 3) pair scaled as cornerEigenValsVecs does, in OpenCV's operation order:
//   Dx: row pass [-1 0 1] (exact), column pass (r0 + r2)*k1 + r1*k0
//   Dy: row pass k1*a + k0*b + k1*c left to right, column pass t2 - t0
// `variant` (icelk_set_variant, the generic kernel only): bit 0 = the symmetric column pass fused, fmaf(r0 + r2, k1, r1 k0)
// (OpenCV 4.x SymmColumnSmallVec_32f in an FMA3 build); bit 1 = the row pass with its two additions fused (a RowFilter loop
// contracted by a compiler that targets FMA); bit 2 = calcMinEigenVal's (a-c)^2 + b^2 as fmaf(b, b, t t).  0 = what every
// other kernel computes.  oracle/icelk_oracle.c names the same switches (orc_set_variant).
__device__ __forceinline__ float row_smooth(float a, float b, float c, float k0, float k1, int variant)
{
    if (variant & 2) return fmaf(k1, c, fmaf(k0, b, __fmul_rn(k1, a)));
    return __fadd_rn(__fadd_rn(__fmul_rn(k1, a), __fmul_rn(k0, b)), __fmul_rn(k1, c));
}

__device__ __forceinline__ void sobel_cov(float a0, float b0, float c0, float a1, float c1, float a2, float b2,
                                          float c2, float k0, float k1, float& xx, float& xy, float& yy, int variant = 0)
{
    const float dx = (variant & 1) ? fmaf(__fadd_rn(__fsub_rn(c0, a0), __fsub_rn(c2, a2)), k1, __fmul_rn(__fsub_rn(c1, a1), k0))
                                   : __fadd_rn(__fmul_rn(__fadd_rn(__fsub_rn(c0, a0), __fsub_rn(c2, a2)), k1),
                                               __fmul_rn(__fsub_rn(c1, a1), k0));
    const float t0 = row_smooth(a0, b0, c0, k0, k1, variant);
    const float t2 = row_smooth(a2, b2, c2, k0, k1, variant);
    const float dy = __fsub_rn(t2, t0);
    xx = __fmul_rn(dx, dx);
    xy = __fmul_rn(dx, dy);
    yy = __fmul_rn(dy, dy);
}

// the same for two horizontally adjacent positions at once, on packed f32 math (v_pk_add/mul_f32: two lanes of
// work per issue slot); every operation rounds exactly like its scalar counterpart
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void sobel_cov2(f2 a0, f2 b0, f2 c0, f2 a1, f2 c1, f2 a2, f2 b2, f2 c2, float k0, float k1,
                                           f2& xx, f2& xy, f2& yy)
{
    const f2 dx = ((c0 - a0) + (c2 - a2)) * k1 + (c1 - a1) * k0;
    const f2 t0 = (a0 * k1 + b0 * k0) + c0 * k1;
    const f2 t2 = (a2 * k1 + b2 * k0) + c2 * k1;
    const f2 dy = t2 - t0;
    xx = dx * dx;
    xy = dx * dy;
    yy = dy * dy;
}

// N consecutive window sums of BS terms each over v[0 .. N+BS-2]: a sliding sum (drop the oldest term, add the next), 2
// additions per output instead of BS - 1.  NOT the order of the oracle, the restatement and k_min_eig, which add term by
// term.  Where every derivative is integer * scale the products lie in [2^-30, 2^-4] with 24-bit mantissas and any sum of a few
// hundred of them is exact in double (tests/test_oracle_kat.py::test_box_sums_of_the_covariance_planes_are_exact_in_double),
// so the order cannot show.  Real dy values are not all of that form: where two pixel rows nearly cancel, dy is a rounding
// residue down to 2^-28, its products reach below 2^-60, and a sum that also holds ordinary products rounds.  The sliding
// sum then differs from the term-by-term one by at most N_add * 2^-53 * (largest sum), which the float32 map shows in a few
// pixels per frame at the 1e-12 level (the bound, its derivation, the measured counts;
// tests/box_sum_frames.py, tests/test_gpu_box_sums.py).  OpenCV's own RowSum / ColumnSum are running sums too: their
// result depends on their history in the same way, and is not the term-by-term value either.
template <int N, int BS>
__device__ __forceinline__ void window_sums(const double (&v)[N + BS - 1], double (&out)[N])
{
    if constexpr (BS <= 3) {
#pragma unroll
        for (int i = 0; i < N; i++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < BS; k++) s += v[i + k];
            out[i] = s;
        }
    } else {
        double s = v[0];
#pragma unroll
        for (int k = 1; k < BS; k++) s += v[k];
        out[0] = s;
#pragma unroll
        for (int i = 1; i < N; i++) {
            s = (s - v[i - 1]) + v[i + BS - 1];
            out[i] = s;
        }
    }
}

__device__ __forceinline__ float min_eig_of(double s0, double s1, double s2, int variant = 0)
{
    const float a = __fmul_rn((float)s0, 0.5f), b = (float)s1, c = __fmul_rn((float)s2, 0.5f);
    const float d = __fsub_rn(a, c);
    const float r = (variant & 4) ? fmaf(b, b, __fmul_rn(d, d)) : __fadd_rn(__fmul_rn(d, d), __fmul_rn(b, b));
    return __fsub_rn(__fadd_rn(a, c), sqrtf(r));
}

// The Harris response of the same three box sums, which are NOT halved as calcMinEigenVal halves them.  Every operation
// is rounded to float32 and nothing is fused: calcHarris' float lanes,
//     t = a + c;  R = (a c - b b) - (kf t) t;   kf = (float)k
// tail (icelk_set_variant "harris_tail" 1, the any-blockSize kernel only): OpenCV's scalar tail, where k stays a double,
//     R = (float)((double)(fl(a c) - fl(b b)) - (k (double)fl(a + c)) (double)fl(a + c))
// Both are written from knowledge of upstream OpenCV; like the rest of the detector, parity with OpenCV is unpinned
// (DESIGN.md 2).  tests/harris_restatement.py states both in numpy.
__device__ __forceinline__ float harris_of(float a, float b, float c, float kf)
{
    const float t = __fadd_rn(a, c);
    return __fsub_rn(__fsub_rn(__fmul_rn(a, c), __fmul_rn(b, b)), __fmul_rn(__fmul_rn(kf, t), t));
}
__device__ __forceinline__ float harris_tail_of(float a, float b, float c, double k)
{
    const double t = (double)__fadd_rn(a, c);
    const double det = (double)__fsub_rn(__fmul_rn(a, c), __fmul_rn(b, b));
    return (float)__dsub_rn(det, __dmul_rn(__dmul_rn(k, t), t));
}
// what the any-blockSize kernel computes at a pixel: resp.kind picks the response, resp.tail the Harris form
__device__ __forceinline__ float response_of(double s0, double s1, double s2, int variant, const Response& resp)
{
    if (resp.kind != ICELK_DETECTOR_HARRIS) return min_eig_of(s0, s1, s2, variant);
    return resp.tail ? harris_tail_of((float)s0, (float)s1, (float)s2, resp.k)
                     : harris_of((float)s0, (float)s1, (float)s2, (float)resp.k);
}

// wave-reduce `best` and publish it; the atomic is skipped when the published maximum is already as large
// (the value only grows, so a stale read can only cause a redundant atomic, never a lost one)
__device__ __forceinline__ void publish_max(unsigned* max_key, unsigned best, int tid)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned other = __shfl_xor(best, o);
        best = other > best ? other : best;
    }
    if ((tid & 63) == 0 && best > __atomic_load_n(max_key, __ATOMIC_RELAXED)) atomicMax(max_key, best);
}

// ------------------------------------------------------------------------------------------------
// K6+K7 in STRIPS (round 3; blockSize 3/5/7/10).  Round 2's tile kernel (removed) paid for its 64x16 tile twice: the Sobel
// stage ran on 27x75 positions and the row sums on 27x66 for 16x64 outputs (1.98x / 1.74x), and its column pass and
// eigenvalue stage occupied 198 of 256 threads.  Here a workgroup walks DOWN a strip 245 outputs wide (blockSize 10) and 62 high:
//   * one thread per covariance column.  The Sobel pair rolls down the column in registers (row difference and row
//     smooth of the two pixel rows above are kept; three byte loads per new row, issued one row ahead; BORDER_REFLECT_101
//     in x costs nothing: the three column offsets of a thread are fixed).  The COLUMN sums come first: a running double
//     sum per plane, + the new product, - the one blockSize rows up, kept as f32 in a register ring (static indices: the
//     row loop is unrolled by lcm(blockSize, 4)).  These sums are exact for derivatives of the form integer * scale and
//     round where a dy is a rounding residue (window_sums' note): the running sum carries such an error down the strip
//     until the strip ends (over an exactly constant band, where every later term is 0, it stays visible as a map value of
//     ~1e-19 in place of 0), so columns-first-and-sliding equals the term-by-term sum, and OpenCV's row-then-column running
//     sums, only up to the bound of DESIGN.md 4.2: (blockSize - 1) + 2 EH additions here, (blockSize - 1) + 2 (RX - 1) in
//     the row window.
//   * every 4 rows: the column sums of the 4 rows (LDS, 24 KB) -> row sums by threads that own 4 consecutive outputs of
//     one row (sliding window, 15 additions per plane) -> min eigenvalue -> an 8-row ring of the eigenvalue map (LDS);
//     then the 3x3 non-max test, one thread per column, for the 4 rows whose lower neighbour now exists.
// Strips that touch the top or bottom of the image (FRESH) reflect rows: the covariance row at a reflected position is
// the one AT that position with its own neighbours, so the roll does not apply there and each row loads its 3x3 afresh.
// Round 8 took out per-pixel work the results do not need: pixels are read through a buffer descriptor (no vector
// address arithmetic), the square root is taken at the range the radicand has (strip_sqrt.h), and a strip that lies inside the
// frame, unmasked, with no map asked for, runs a row phase that tests nothing per pixel (FAST).  Results are bit for bit as before.
// Halo: 1.045 in x, 69 covariance rows for 58 output rows.  Regions: 4 per workgroup (16 output rows each).
// Measured and dropped: a form that stays within the 72 VGPRs the tracker's five waves leave free on a SIMD (ring in
// LDS, the running sums and the roll parked in LDS during the row-sum phase, s_setprio 3), so that its workgroups are
// resident the moment they are dispatched instead of waiting for tracker waves to retire on all four SIMDs of a CU.
// It does what it was built for -- the gaps between tracker launches shrink from 11-200 us to 13-20 us -- but the
// tracker launch beside it takes 318 us instead of 282 and the kernel alone 154 us instead of 75 (53 KB of LDS, two
// workgroups per CU): 5 630-5 690 pairs/s against 5 910-5 920 on the same box.  The pipeline is bound by the
// instructions the SIMDs issue, not by when they issue them.
// ------------------------------------------------------------------------------------------------
constexpr int gcd_c(int a, int b) { return b == 0 ? a : gcd_c(b, a % b); }

template <int BS>
struct StripCfg {
    static constexpr int NT = 256;                 // threads = covariance columns; four waves, one row of a batch each
    static constexpr int AN = BS / 2;
    static constexpr int EW = NT - (BS - 1);       // eigenvalue columns
    static constexpr int TW = EW - 2;              // output columns
    static constexpr int R = 4;                    // rows per batch = waves
    static constexpr int UNROLL = BS * R / gcd_c(BS, R);   // rows per trip of the row loop: ring slots and batch rows static
    // eigenvalue rows: whole trips -- an exit from inside the unrolled trip would meet the register ring in a different
    // rotation at every batch (measured: 230 VGPRs instead of 146)
    static constexpr int EH = (64 / UNROLL) * UNROLL;
    static constexpr int SH = EH - 2;              // output rows
    static constexpr int NROWS = EH + BS - 1;      // covariance rows walked
    static constexpr int RX = 4;                   // outputs per row task
    static constexpr int NG = (EW + RX - 1) / RX;  // row tasks per row
    static constexpr int VP = NT + 2;              // doubles per row of column sums (the last task reads 2 beyond)
    static constexpr int SUB = 16, NSUB = (SH + SUB - 1) / SUB;
    static constexpr int V_BYTES = R * 3 * VP * 8;
    static constexpr int E_BYTES = 8 * NT * 4;
    static constexpr int LDS_BYTES = V_BYTES + E_BYTES;
    static_assert(EH % R == 0 && NG <= 64 && RX * NG <= NT + RX - 1, "one wave per row of a batch");
    static_assert(RX * (NG - 1) + RX + BS - 2 < VP, "row tasks stay inside a row of column sums");
    static_assert((VP * 8) % 16 == 0, "16-byte reads of the column sums");
};

// a frame's pixels behind a raw buffer descriptor (no stride, pitch * h bytes, the 32-bit data format word of gfx9); a row is
// the descriptor and a scalar byte offset, a pixel of it one buffer_load_ubyte at a lane offset
struct PixelRow {
    __amdgpu_buffer_rsrc_t rsrc;
    unsigned at;
    __device__ __forceinline__ unsigned operator[](unsigned x) const { return __builtin_amdgcn_raw_buffer_load_b8(rsrc, x, at, 0); }
};
struct PixelRows {
    __amdgpu_buffer_rsrc_t rsrc;
    unsigned pitch;
    __device__ __forceinline__ PixelRow row(int y) const { return PixelRow{rsrc, (unsigned)y * pitch}; }
};

struct SobelRoll {
    float d1, d2, t1, t2;   // row difference / row smooth of pixel rows yc (1) and yc - 1 (2)
};

__device__ __forceinline__ float smooth3(float a, float b, float c, float k0, float k1)
{
    return __fadd_rn(__fadd_rn(__fmul_rn(k1, a), __fmul_rn(k0, b)), __fmul_rn(k1, c));
}

// min_eig_of for the N outputs of a row task, with the square root taken at the range this kernel has.  sqrtf, as the
// compiler expands it, scales the radicand into range, corrects the hardware's root by the two-sided residual test, scales
// back and tests for 0 and infinity: about 16 instructions.  The radicand here, (a - c)^2 + b^2 of box sums that are at
// most 1, lies between ~1e-20 and 1.25 wherever the ground has texture, so only the residual test does anything
// (strip_sqrt.h: the band and why the result is sqrtf's bit for bit).  One wave-uniform test guards it: if any radicand of
// the wave is outside the band -- 0 over flat ground, above all -- the whole wave takes sqrtf.  A real branch.  BAND = false:
// min_eig_of as it is, for the block size that is faster with it.
template <int N, bool BAND>
__device__ __forceinline__ void min_eig_strip(const double (&Sm)[3][N], float (&e)[N])
{
    if constexpr (!BAND) {
#pragma unroll
        for (int k = 0; k < N; k++) e[k] = min_eig_of(Sm[0][k], Sm[1][k], Sm[2][k]);
        return;
    }
    float tr[N], r[N];
    unsigned lo = 0xffffffffu, hi = 0u;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const float a = __fmul_rn((float)Sm[0][k], 0.5f), b = (float)Sm[1][k], c = __fmul_rn((float)Sm[2][k], 0.5f);
        const float d = __fsub_rn(a, c);
        r[k] = __fadd_rn(__fmul_rn(d, d), __fmul_rn(b, b));
        tr[k] = __fadd_rn(a, c);
        const unsigned rb = __float_as_uint(r[k]);   // non-negative floats order like their bits; -0, negatives and NaN lie above
        lo = rb < lo ? rb : lo;
        hi = rb > hi ? rb : hi;
    }
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(lo < SQRT_BAND_LO || hi > SQRT_BAND_HI) == 0, 1)) {
#pragma unroll
        for (int k = 0; k < N; k++) e[k] = __fsub_rn(tr[k], sqrt_in_band(r[k]));
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) e[k] = __fsub_rn(tr[k], sqrtf(r[k]));
    }
}

// HARRIS: the row task takes harris_of (four multiplications, three additions or subtractions, no square root, so no band
// and no wave-wide test) in place of the smaller eigenvalue; kf is read by that arm only.  Everything else -- the roll, the
// sums, the map, the masked maximum, the non-max test -- is the same text for both responses, and the !HARRIS
// instantiations are the code they were before the parameter existed.
template <int BS, bool FRESH, bool FAST, bool HARRIS>
__device__ __forceinline__ void strip_body(const uint8_t* __restrict__ img, int w, int h, int pitch, float k0, float k1, float kf,
                                           const uint8_t* __restrict__ mask, int mask_pitch, unsigned* __restrict__ max_key,
                                           unsigned long long* __restrict__ raw, int* __restrict__ blk_count,
                                           float* __restrict__ eig_out, uint8_t* smem, int* s_cnt)
{
    using C = StripCfg<BS>;
    double* Vb = reinterpret_cast<double*>(smem);                 // [R][3][VP]
    float* Er = reinterpret_cast<float*>(smem + C::V_BYTES);      // [8][NT]
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * C::TW, y0 = blockIdx.y * C::SH;
    const int xs = x0 - 1 - C::AN, ys = y0 - 1 - C::AN;           // image position of covariance column / row 0
    const int rx = reflect101(xs + tid, w);
    // Pixels are read through a buffer descriptor of the frame: a load is then (descriptor, 32-bit lane offset, scalar row
    // offset), and a row costs no vector address arithmetic at all -- a pointer plus a lane index is a 64-bit vector add per
    // load.  The three column offsets of a thread are fixed; only the scalar row offset moves.  (The descriptor is no
    // safety net: the hardware compares only the lane offset with pitch * h, not the scalar row offset.  Every read is inside
    // the frame because rows and columns are reflected or clamped into it, as before.)
    const unsigned xm = (unsigned)reflect101(rx - 1, w), xc = (unsigned)rx, xp = (unsigned)reflect101(rx + 1, w);
    const PixelRows px{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(img), 0, pitch * h, 0x00020000), (unsigned)pitch};
    const int bid = blockIdx.y * gridDim.x + blockIdx.x;
    if (tid < C::NSUB) s_cnt[tid] = 0;
    // the two doubles per row of column sums that the last row task reads beyond the NT columns: no thread writes them and no
    // output uses them, but their radicands take part in the wave's test of the square root's band.  Zero, they give ordinary
    // values; left as the LDS was found, a NaN or an infinity there would send every wave to sqrtf.
    if (tid < C::R * 3 * (C::VP - C::NT)) Vb[(tid / (C::VP - C::NT)) * C::VP + C::NT + tid % (C::VP - C::NT)] = 0.0;

    float ring[3][BS];
#pragma unroll
    for (int k = 0; k < BS; k++) ring[0][k] = ring[1][k] = ring[2][k] = 0.f;
    double V[3] = {0.0, 0.0, 0.0};
    SobelRoll S{};
    unsigned pa = 0, pb = 0, pc = 0;   // the pixel row one ahead of the roll
    if (!FRESH) {
        const PixelRow r2 = px.row(ys - 1), r1 = px.row(ys), r0 = px.row(ys + 1);
        const float a2 = (float)r2[xm], b2 = (float)r2[xc], c2 = (float)r2[xp];
        const float a1 = (float)r1[xm], b1 = (float)r1[xc], c1 = (float)r1[xp];
        S.d2 = __fsub_rn(c2, a2); S.t2 = smooth3(a2, b2, c2, k0, k1);
        S.d1 = __fsub_rn(c1, a1); S.t1 = smooth3(a1, b1, c1, k0, k1);
        pa = r0[xm]; pb = r0[xc]; pc = r0[xp];
    }
    // products of covariance row r (image row ys + r)
    auto cov_row = [&](int r, float& xx, float& xy, float& yy) {
        float dtop, dmid, dbot, ttop, tbot;
        if (FRESH) {
            const int ry = reflect101(ys + r, h);
            const PixelRow q0 = px.row(reflect101(ry - 1, h)), q1 = px.row(ry), q2 = px.row(reflect101(ry + 1, h));
            const float a0 = (float)q0[xm], b0 = (float)q0[xc], c0 = (float)q0[xp];
            const float a1 = (float)q1[xm], c1 = (float)q1[xp];
            const float a2 = (float)q2[xm], b2 = (float)q2[xc], c2 = (float)q2[xp];
            dtop = __fsub_rn(c0, a0); dmid = __fsub_rn(c1, a1); dbot = __fsub_rn(c2, a2);
            ttop = smooth3(a0, b0, c0, k0, k1); tbot = smooth3(a2, b2, c2, k0, k1);
        } else {
            float a = (float)pa, b = (float)pb, c = (float)pc;
            // a and c are needed as floats for the smooth anyway: kept opaque here, c - a is one subtraction of them and not an
            // integer subtraction of the bytes plus a conversion of its own (the same value either way: both are exact).  This
            // steers one compiler's choice; with another the asm costs nothing and the kernel computes the same
            asm("" : "+v"(a), "+v"(c));
            int nr = ys + r + 2;                  // next pixel row; past the last row needed it is only kept inside the image
            nr = nr < h ? nr : h - 1;
            const PixelRow q = px.row(nr);
            pa = q[xm]; pb = q[xc]; pc = q[xp];
            dtop = S.d2; dmid = S.d1; dbot = __fsub_rn(c, a);
            ttop = S.t2; tbot = smooth3(a, b, c, k0, k1);
            S.d2 = S.d1; S.d1 = dbot; S.t2 = S.t1; S.t1 = tbot;
        }
        const float dx = __fadd_rn(__fmul_rn(__fadd_rn(dtop, dbot), k1), __fmul_rn(dmid, k0));
        const float dy = __fsub_rn(tbot, ttop);
        xx = __fmul_rn(dx, dx); xy = __fmul_rn(dx, dy); yy = __fmul_rn(dy, dy);
    };

    // the first blockSize - 1 covariance rows only fill the window
#pragma unroll
    for (int r = 0; r < BS - 1; r++) {
        float p[3];
        cov_row(r, p[0], p[1], p[2]);
#pragma unroll
        for (int q = 0; q < 3; q++) { V[q] += (double)p[q]; ring[q][r] = p[q]; }
    }

    unsigned best = 0;
    // FAST: the masked maximum without a key per pixel.  Of the RX outputs of a task, output 0 lies outside the strip for the
    // first task of a row and outputs KL + 1 .. RX - 1 for the last; nothing else is ever left out.  So three classes of
    // outputs (0 | 1 .. KL | KL + 1 .. RX - 1) each keep what they have seen down the strip, and which classes count is
    // decided once per thread after the loop.  Kept per class: the largest and the smallest of the values' bits as SIGNED
    // integers.  If any value is >= +0 the largest is the maximum (such floats order like their bits, and every float with the
    // sign set, -0 included, is a negative integer); if none is, the values order against their bits and the smallest is the
    // maximum.  That is the order of ordered_key, -0 below +0 included, with no assumption about the values.
    constexpr int KL = C::TW - C::RX * (C::NG - 1);
    static_assert(KL >= 0 && KL < C::RX && C::RX * C::NG - 1 >= C::TW, "the last row task holds the strip's last output column");
    int top_hi[3], top_lo[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { top_hi[k] = INT_MIN; top_lo[k] = INT_MAX; }
    // row-sum phase: which row of the batch (= wave) / which group of RX outputs this thread takes
    const int wr = __builtin_amdgcn_readfirstlane(tid >> 6), g = tid & 63;   // wr is the wave: row tests on it are scalar
    for (int base = 0; base < C::EH; base += C::UNROLL) {
#pragma unroll
        for (int j = 0; j < C::UNROLL; j++) {
            const int i = base + j;                   // eigenvalue row this covariance row completes
            const int K = (BS - 1 + j) % BS;          // ring slot: holds the product blockSize rows up
            float p[3];
            cov_row(BS - 1 + i, p[0], p[1], p[2]);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                V[q] = (V[q] + (double)p[q]) - (double)ring[q][K];
                ring[q][K] = p[q];
                Vb[((j % C::R) * 3 + q) * C::VP + tid] = V[q];
            }
            __builtin_amdgcn_sched_barrier(0);           // rows stay in order: the loads of 20 unrolled rows are not hoisted
            if (j % C::R != C::R - 1) continue;
            const int eb = i / C::R;                  // batch: eigenvalue rows eb*R .. eb*R + R-1
            __syncthreads();
            if (g < C::NG && wr < C::R) {
                double Sm[3][C::RX];
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    double v[C::RX + BS - 1];
                    const double* src = Vb + (wr * 3 + q) * C::VP + C::RX * g;
#pragma unroll
                    for (int k = 0; k < C::RX + BS - 1; k++) v[k] = src[k];
                    window_sums<C::RX, BS>(v, Sm[q]);
                    __builtin_amdgcn_sched_barrier(0);   // one plane's 13 doubles at a time, not all three
                }
                const int er = eb * C::R + wr;
                float e[C::RX];
                // blockSize 3 keeps sqrtf: measured alone, its kernel is 69-71 us with sqrtf and 75-77 with the band form (the
                // parent: 75-76), though the band form issues fewer instructions -- its row phase is the short one (two additions
                // per output and plane) and the wave-wide test and branch sit in the middle of it
                if constexpr (HARRIS) {
#pragma unroll
                    for (int k = 0; k < C::RX; k++) e[k] = harris_of((float)Sm[0][k], (float)Sm[1][k], (float)Sm[2][k], kf);
                } else {
                    min_eig_strip<C::RX, BS != 3>(Sm, e);
                }
                *reinterpret_cast<float4*>(Er + (er & 7) * C::NT + C::RX * g) = make_float4(e[0], e[1], e[2], e[3]);
                const int y = y0 - 1 + er;
                if constexpr (FAST) {
                    // every output of the strip is inside the frame, unmasked, and no map is asked for: nothing to test per
                    // pixel.  The first and last eigenvalue row are left out here (per wave), the first and last column
                    // after the loop (per thread).
                    if (er >= 1 && er <= C::SH) {
#pragma unroll
                        for (int k = 0; k < C::RX; k++) {
                            const int cls = k == 0 ? 0 : (k <= KL ? 1 : 2), bits = __float_as_int(e[k]);
                            top_hi[cls] = max(top_hi[cls], bits);
                            top_lo[cls] = min(top_lo[cls], bits);
                        }
                    }
                } else if (er >= 1 && er <= C::SH && y < h) {
#pragma unroll
                    for (int k = 0; k < C::RX; k++) {
                        const int ce = C::RX * g + k, x = x0 - 1 + ce;
                        if (ce >= 1 && ce <= C::TW && x < w) {
                            if (eig_out) eig_out[(size_t)y * w + x] = e[k];
                            if (!mask || mask[(size_t)y * mask_pitch + x]) {
                                const unsigned key = ordered_key(e[k]);
                                best = key > best ? key : best;
                            }
                        }
                    }
                }
            }
            __syncthreads();
            {
                // 3x3 non-max test of eigenvalue rows eb*R - 1 .. eb*R + 2, column tid
                const int x = x0 - 1 + tid;
                if (tid >= 1 && tid <= C::TW && x >= 1 && x < w - 1) {
                    float m3[6], mid[6], side[6];
#pragma unroll
                    for (int k = 0; k < 6; k++) {
                        const float* row = Er + ((eb * C::R - 2 + k) & 7) * C::NT + tid;
                        const float l = row[-1], c = row[0], r = row[1];
                        mid[k] = c;
                        side[k] = fmaxf(l, r);
                        m3[k] = fmaxf(side[k], c);
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int c = eb * C::R - 1 + q, y = y0 - 1 + c;
                        if (c < 1 || c > C::SH || y < 1 || y >= h - 1) continue;
                        const float v = mid[q + 1];
                        if (!(v > 0.f)) continue;
                        const float m = fmaxf(fmaxf(m3[q], m3[q + 2]), side[q + 1]);
                        if (v < m) continue;
                        if (mask && !mask[(size_t)y * mask_pitch + x]) continue;
                        const int sub = (c - 1) / C::SUB;
                        const int pos = atomicAdd(&s_cnt[sub], 1);
                        raw[((size_t)bid * C::NSUB + sub) * (C::TW * C::SUB) + pos] = cand_key(v, x, y);
                    }
                }
            }
        }
    }
    if constexpr (FAST) {
        // one key per thread: class 0 counts unless this is the first task of a row, class 2 unless it is the last
        const bool counts[3] = {g >= 1 && g < C::NG, g < C::NG, g < C::NG - 1};
        int hi = INT_MIN, lo = INT_MAX;
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (counts[k]) { hi = max(hi, top_hi[k]); lo = min(lo, top_lo[k]); }
        if (lo <= hi) best = ordered_key(__int_as_float(hi >= 0 ? hi : lo));   // lo > hi: the thread has seen no output
    }
    publish_max(max_key, best, tid);
    __syncthreads();
    if (tid < C::NSUB) blk_count[bid * C::NSUB + tid] = s_cnt[tid];
}

// Registers: what the kernel needs at blockSize 10 is 144 VGPRs.  Until late in round 4 it was held to 128 for a fourth wave
// per SIMD -- 18 spilled VGPRs, 76 B of scratch per lane: 19 MB of scratch written per launch (WRITE_SIZE) -- which is
// faster ALONE (81 against 98 us) and slower where it counts: beside a tracker launch the tracker decides how many of its
// waves fit, and without scratch C2 runs at 6 900-6 940 pairs/s instead of 6 620-6 650 (same-box A/B,
// profiles/r04_ab_corner_kernel_registers.txt; REF equal, C5 +1 %).  blockSize 3 / 5 / 7 need 87 / 110 / 124 and keep four waves.
// Round 8 (profiles/r08_corner_resources.json): 148 at blockSize 10, three waves, no scratch; blockSize 7 now needs exactly the 128
// of a fourth wave, so a change of compiler or of this body can cost blockSize 7 that wave -- look at the resource remarks
// (-Rpass-analysis=kernel-resource-usage) after either.
// The response is a compile-time parameter of the body, and each response has an entry point of its own: k_eig_strip keeps its
// name, its argument list and with them its kernel-argument layout, so its code object is the one it was before the Harris
// response existed (tools/isa_compare.py against the parent); k_harris_strip, below, is the same text with kf = (float)k
// behind the same arguments.  TWO COPIES of the dispatch (rolling / inside_x / the three arms): a change to one is a change
// to both.  (One helper for both was tried: the Shi-Tomasi instantiations then came out with another register allocation.)
template <int BS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_eig_strip(const uint8_t* __restrict__ img, int w, int h, int pitch, float k0,
                                                    float k1, const uint8_t* __restrict__ mask, int mask_pitch,
                                                    unsigned* __restrict__ max_key,
                                                    unsigned long long* __restrict__ raw, int* __restrict__ blk_count,
                                                    float* __restrict__ eig_out)
{
    using C = StripCfg<BS>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int s_cnt[C::NSUB];
    const int ys = (int)blockIdx.y * C::SH - 1 - C::AN;
    // pixel rows ys - 1 .. ys + NROWS are read by the rolling form: such a strip has all its output rows inside the frame
    const bool rolling = ys - 1 >= 0 && ys + C::NROWS <= h - 1;
    // all TW output columns of the strip are inside the frame (every strip but a narrower last one)
    const bool inside_x = ((int)blockIdx.x + 1) * C::TW <= w;
    if (rolling && inside_x && !mask && !eig_out)
        strip_body<BS, false, true, false>(img, w, h, pitch, k0, k1, 0.f, mask, mask_pitch, max_key, raw, blk_count, eig_out, smem, s_cnt);
    else if (rolling)
        strip_body<BS, false, false, false>(img, w, h, pitch, k0, k1, 0.f, mask, mask_pitch, max_key, raw, blk_count, eig_out, smem, s_cnt);
    else
        strip_body<BS, true, false, false>(img, w, h, pitch, k0, k1, 0.f, mask, mask_pitch, max_key, raw, blk_count, eig_out, smem, s_cnt);
}

// Registers (the compiler's resource remarks, profiles/harris_strip_resources.json): 84 / 112 / 134 / 148 VGPRs at blockSize
// 3 / 5 / 7 / 10 against k_eig_strip's 83 / 110 / 128 / 148, no scratch, no spill.  blockSize 7 is over the 128 of a fourth
// wave per SIMD, which k_eig_strip<7> holds exactly: three waves here.  The body below is k_eig_strip's, copied: keep the
// two in step.
template <int BS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void k_harris_strip(const uint8_t* __restrict__ img, int w, int h, int pitch, float k0,
                                                    float k1, const uint8_t* __restrict__ mask, int mask_pitch,
                                                    unsigned* __restrict__ max_key,
                                                    unsigned long long* __restrict__ raw, int* __restrict__ blk_count,
                                                    float* __restrict__ eig_out, float kf)
{
    using C = StripCfg<BS>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ int s_cnt[C::NSUB];
    const int ys = (int)blockIdx.y * C::SH - 1 - C::AN;
    // pixel rows ys - 1 .. ys + NROWS are read by the rolling form: such a strip has all its output rows inside the frame
    const bool rolling = ys - 1 >= 0 && ys + C::NROWS <= h - 1;
    // all TW output columns of the strip are inside the frame (every strip but a narrower last one)
    const bool inside_x = ((int)blockIdx.x + 1) * C::TW <= w;
    if (rolling && inside_x && !mask && !eig_out)
        strip_body<BS, false, true, true>(img, w, h, pitch, k0, k1, kf, mask, mask_pitch, max_key, raw, blk_count, eig_out, smem, s_cnt);
    else if (rolling)
        strip_body<BS, false, false, true>(img, w, h, pitch, k0, k1, kf, mask, mask_pitch, max_key, raw, blk_count, eig_out, smem, s_cnt);
    else
        strip_body<BS, true, false, true>(img, w, h, pitch, k0, k1, kf, mask, mask_pitch, max_key, raw, blk_count, eig_out, smem, s_cnt);
}

// ------------------------------------------------------------------------------------------------
// K6 generic: any blockSize, writes the eigenvalue map.  LDS: cov[3][eh][ew] f32, hs[3][eh][TW] f64.
// ------------------------------------------------------------------------------------------------
constexpr int EIG_TW = 64;
constexpr int EIG_TH = 16;

__global__ __launch_bounds__(256) void k_min_eig(const uint8_t* __restrict__ img, int w, int h, int pitch, int bs,
                                                 float k0, float k1, float* __restrict__ eig,
                                                 const uint8_t* __restrict__ mask, int mask_pitch,
                                                 unsigned* __restrict__ max_key, int variant, Response resp)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int anchor = bs / 2;
    const int ew = EIG_TW + bs - 1, eh = EIG_TH + bs - 1;
    double* hs = reinterpret_cast<double*>(smem);
    float* cov = reinterpret_cast<float*>(smem + sizeof(double) * 3 * eh * EIG_TW);
    const int x0 = blockIdx.x * EIG_TW, y0 = blockIdx.y * EIG_TH;
    const int tid = threadIdx.x;
    for (int i = tid; i < ew * eh; i += 256) {
        const int ey = i / ew, ex = i - ey * ew;
        const int rx = reflect101(x0 - anchor + ex, w), ry = reflect101(y0 - anchor + ey, h);
        const int xm = reflect101(rx - 1, w), xp = reflect101(rx + 1, w);
        const int ym = reflect101(ry - 1, h), yp = reflect101(ry + 1, h);
        const uint8_t* r0 = img + (size_t)ym * pitch;
        const uint8_t* r1 = img + (size_t)ry * pitch;
        const uint8_t* r2 = img + (size_t)yp * pitch;
        float xx, xy, yy;
        sobel_cov((float)r0[xm], (float)r0[rx], (float)r0[xp], (float)r1[xm], (float)r1[xp], (float)r2[xm],
                  (float)r2[rx], (float)r2[xp], k0, k1, xx, xy, yy, variant);
        cov[i] = xx;
        cov[ew * eh + i] = xy;
        cov[2 * ew * eh + i] = yy;
    }
    __syncthreads();
    for (int i = tid; i < eh * EIG_TW; i += 256) {
        const int ey = i / EIG_TW, ox = i - ey * EIG_TW;
        const float* c = cov + ey * ew + ox;
        double s0 = 0, s1 = 0, s2 = 0;
        for (int k = 0; k < bs; k++) {
            s0 += (double)c[k];
            s1 += (double)c[ew * eh + k];
            s2 += (double)c[2 * ew * eh + k];
        }
        hs[i] = s0;
        hs[eh * EIG_TW + i] = s1;
        hs[2 * eh * EIG_TW + i] = s2;
    }
    __syncthreads();
    unsigned best = 0;
    for (int i = tid; i < EIG_TH * EIG_TW; i += 256) {
        const int oy = i / EIG_TW, ox = i - oy * EIG_TW;
        const int x = x0 + ox, y = y0 + oy;
        if (x >= w || y >= h) continue;
        const double* r = hs + oy * EIG_TW + ox;
        double s0 = 0, s1 = 0, s2 = 0;
        for (int k = 0; k < bs; k++) {
            s0 += r[k * EIG_TW];
            s1 += r[eh * EIG_TW + k * EIG_TW];
            s2 += r[2 * eh * EIG_TW + k * EIG_TW];
        }
        const float v = response_of(s0, s1, s2, variant, resp);
        eig[(size_t)y * w + x] = v;
        if (!mask || mask[(size_t)y * mask_pitch + x]) {
            const unsigned k = ordered_key(v);
            best = k > best ? k : best;
        }
    }
    publish_max(max_key, best, tid);
}

// K7 generic: threshold + 3x3 dilate equality on the materialised map; a workgroup covers a 256 x 8 pixel band
// and owns region (blockIdx) of the candidate buffer.
constexpr int NMS_ROWS = 8;
__global__ __launch_bounds__(256) void k_nms_collect(const float* __restrict__ eig, int w, int h,
                                                     const uint8_t* __restrict__ mask, int mask_pitch,
                                                     const unsigned* __restrict__ max_key, double quality,
                                                     unsigned long long* __restrict__ raw, int* __restrict__ blk_count)
{
    __shared__ int list_n;
    const int tid = threadIdx.x;
    if (tid == 0) list_n = 0;
    __syncthreads();
    const int bid = blockIdx.y * gridDim.x + blockIdx.x;
    unsigned long long* region = raw + (size_t)bid * (256 * NMS_ROWS);
    const float thr = threshold_of(max_key, quality);
    const int x = blockIdx.x * 256 + tid + 1;
    for (int r = 0; r < NMS_ROWS; r++) {
        const int y = blockIdx.y * NMS_ROWS + r + 1;
        if (x >= w - 1 || y >= h - 1) continue;
        const float v = eig[(size_t)y * w + x];
        if (!(v > thr) || v == 0.f) continue;
        if (mask && !mask[(size_t)y * mask_pitch + x]) continue;
        // m >= 0 whatever the map holds, so a negative v -- which passes v > thr when the masked maximum, and with it thr, is
        // negative (the Harris response over a ramp) -- never equals it: max <= 0 lists nothing
        float m = 0.f;  // dilate of the TOZERO-thresholded map (includes the centre)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                float q = eig[(size_t)(y + dy) * w + (x + dx)];
                q = q > thr ? q : 0.f;
                m = q > m ? q : m;
            }
        if (v != m) continue;
        region[atomicAdd(&list_n, 1)] = cand_key(v, x, y);
    }
    __syncthreads();
    if (tid == 0) blk_count[bid] = list_n;
}

template <int BS>
void launch_strip(hipStream_t s, const Level& img, float k0, float k1, const uint8_t* mask, int mask_pitch, CandBuf& cb,
                  float* eig_out, const Response& resp)
{
    using C = StripCfg<BS>;
    dim3 grid((img.w + C::TW - 1) / C::TW, (img.h + C::SH - 1) / C::SH);
    if (resp.kind == ICELK_DETECTOR_HARRIS)
        hipLaunchKernelGGL((k_harris_strip<BS>), grid, dim3(C::NT), C::LDS_BYTES, s, img.ptr, img.w, img.h, img.pitch, k0, k1,
                           mask, mask_pitch, cb.max_key, cb.raw, cb.blk_count, eig_out, (float)resp.k);
    else
        hipLaunchKernelGGL((k_eig_strip<BS>), grid, dim3(C::NT), C::LDS_BYTES, s, img.ptr, img.w, img.h, img.pitch, k0, k1, mask,
                           mask_pitch, cb.max_key, cb.raw, cb.blk_count, eig_out);
    cb.nblk = (int)(grid.x * grid.y) * C::NSUB;
    cb.region = C::TW * C::SUB;
}

// regions / keys the strip layout needs, whichever blockSize is asked for later
template <int BS>
void strip_geometry(int w, int h, size_t* regions, size_t* keys)
{
    using C = StripCfg<BS>;
    const size_t r = (size_t)((w + C::TW - 1) / C::TW) * ((h + C::SH - 1) / C::SH) * C::NSUB;
    const size_t k = r * (size_t)(C::TW * C::SUB);
    *regions = r > *regions ? r : *regions;
    *keys = k > *keys ? k : *keys;
}
void strip_layout(int w, int h, size_t* regions, size_t* keys)
{
    *regions = *keys = 0;
    strip_geometry<3>(w, h, regions, keys); strip_geometry<5>(w, h, regions, keys);
    strip_geometry<7>(w, h, regions, keys); strip_geometry<10>(w, h, regions, keys);
}

// k_nms_collect: a workgroup per 256 x NMS_ROWS band of the frame's interior
dim3 nms_grid(int w, int h) { return dim3((w - 2 + 255) / 256, (h - 2 + NMS_ROWS - 1) / NMS_ROWS); }

}  // namespace

size_t min_eig_lds_bytes(int block_size)
{
    const int ew = EIG_TW + block_size - 1, eh = EIG_TH + block_size - 1;
    return sizeof(double) * 3 * eh * EIG_TW + sizeof(float) * 3 * eh * ew;
}

bool fused_block_size(int bs) { return bs == 3 || bs == 5 || bs == 7 || bs == 10; }

// capacity (in keys) and regions (blk_count entries) the region layout needs for a w x h frame, whichever kernel produces
// the candidates: k_eig_strip, k_nms_collect or the two-pass form
size_t candidate_capacity(int w, int h)
{
    size_t strip_r, strip_k;
    strip_layout(w, h, &strip_r, &strip_k);
    const size_t generic = (size_t)((w + 255) / 256) * ((h + NMS_ROWS - 1) / NMS_ROWS) * (256 * NMS_ROWS);
    const size_t m = std::max({generic, fast_key_capacity(w, h), strip_k});
    return m + 1024;
}
size_t candidate_blocks(int w, int h)
{
    size_t strip_r, strip_k;
    strip_layout(w, h, &strip_r, &strip_k);
    const dim3 g = nms_grid(w, h);
    const size_t m = std::max({(size_t)g.x * g.y, fast_regions(w, h), strip_r});
    return m + 16;
}

// K6 alone, writing the map with the any-blockSize kernel.
void launch_min_eig(hipStream_t s, const Level& img, int block_size, float* eig, const uint8_t* mask,
                    int mask_pitch, unsigned* max_key, int variant, const Response& resp)
{
    float k0, k1;
    sobel_scale(block_size, &k0, &k1);
    const size_t lds = min_eig_lds_bytes(block_size);
    static size_t attr_lds = 0;
    if (lds > attr_lds) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_min_eig), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
        attr_lds = lds;
    }
    dim3 grid((img.w + EIG_TW - 1) / EIG_TW, (img.h + EIG_TH - 1) / EIG_TH);
    hipLaunchKernelGGL(k_min_eig, grid, dim3(256), lds, s, img.ptr, img.w, img.h, img.pitch, block_size, k0, k1, eig,
                       mask, mask_pitch, max_key, variant, resp);
}

// Candidate collection (K6+K7) into regions of D.cb.raw (stream order, no host sync).
void launch_candidates(hipStream_t s, DetectScratch& D, const Level& img, int block_size, const uint8_t* mask,
                       int mask_pitch, double quality, bool use_generic, float* eig_out_or_null, int variant, const Response& resp)
{
    const bool harris = resp.kind == ICELK_DETECTOR_HARRIS;
    if (variant || (harris && resp.tail)) use_generic = true;     // the named variants live in the any-blockSize kernel only
    // ICELK_TWO_PASS_CORNERS=1: the two-pass form (k_corners_fast.hip: integer bracket of the map + exact arithmetic at the
    // possible maxima) -- a third statement of the arithmetic, bit-identical, measured and not the default
    const bool two_pass = D.cb.acand != nullptr && getenv("ICELK_TWO_PASS_CORNERS") != nullptr;   // scratch: at icelk_create, under the same switch
    // its bracket eps(p) is derived for the smaller eigenvalue and does not hold for det - k tr^2: with the Harris response
    // the switch is ignored and the one-pass strip kernel runs
    if (two_pass && !harris && !use_generic && fused_block_size(block_size) && !eig_out_or_null &&
        launch_candidates_fast(s, D, img, block_size, mask, mask_pitch, quality))
        return;
    if (!use_generic && fused_block_size(block_size)) {
        float k0, k1;
        sobel_scale(block_size, &k0, &k1);
        switch (block_size) {
            case 3: launch_strip<3>(s, img, k0, k1, mask, mask_pitch, D.cb, eig_out_or_null, resp); break;
            case 5: launch_strip<5>(s, img, k0, k1, mask, mask_pitch, D.cb, eig_out_or_null, resp); break;
            case 7: launch_strip<7>(s, img, k0, k1, mask, mask_pitch, D.cb, eig_out_or_null, resp); break;
            default: launch_strip<10>(s, img, k0, k1, mask, mask_pitch, D.cb, eig_out_or_null, resp); break;
        }
    } else {
        launch_min_eig(s, img, block_size, D.eig, mask, mask_pitch, D.cb.max_key, variant, resp);
        D.cb.nblk = 0;
        D.cb.region = 256 * NMS_ROWS;
        if (img.w >= 3 && img.h >= 3) {
            const dim3 grid = nms_grid(img.w, img.h);
            hipLaunchKernelGGL(k_nms_collect, grid, dim3(256), 0, s, D.eig, img.w, img.h, mask, mask_pitch, D.cb.max_key,
                               quality, D.cb.raw, D.cb.blk_count);
            D.cb.nblk = (int)(grid.x * grid.y);
        }
    }
}

}  // namespace icelk
