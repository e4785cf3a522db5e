// k_calib.hip -- the misfit of the camera calibration (s0_2_camera_calibration.py:117-152 photo_to_utm, 231-238
// closest_node, 240-275 optimizefun_calibration): every shoreline point of the photo projected to the map with a
// candidate's (theta, phi, psi, sigma, H), and its distance to the nearest waterline vertex, brute force.
//
// A candidate is 11 doubles prepared on the host: X[3], U[3], V[3] (the direction vectors, products in the order of
// s0_2:124-136), sigma scaled to pixels, H.  The arithmetic is the reference's, unfused (-ffp-contract=off):
//   den = (sigma * X2 + xi * U2) + yi * V2;  tx = H * ((sigma * X0 + xi * U0) + yi * V0) / den + E;  ty likewise + N
//   d2 = dx * dx + dy * dy with dx = wx - tx, dy = wy - ty;  the minimum over all vertices;  sqrt at the end
// (sqrt is monotonic and correctly rounded, so sqrt(min d2) is np.min(d2 ** 0.5) bit for bit; the minimum does not
// depend on the order it is taken in).  np.min propagates NaN and fmin drops it: a NaN tx or ty gives NaN in the
// epilogue; with finite vertices -- icelk_calib_set accepts no others -- nothing else can make a NaN, and an infinite
// tx or ty gives d2 = inf for every vertex, so inf, as numpy.
//
// Every lane of a wave works on the same vertex: the vertices come through scalar loads (a uniform index into a
// restrict const pointer), eight vertices a batch, and the subtraction takes them as scalar operands.  Per pair
// the vector unit runs two v_add_f64 (the differences), two v_mul_f64, one v_add_f64 and one v_min_f64, plus one
// v_max_f64 per batch of eight.
#include <math.h>

#include <algorithm>

#include "icelk_internal.h"
#include "np_sums.h"

namespace icelk {

namespace {

constexpr int kCand = 11;          // doubles per candidate
constexpr int kCostLds = 4096;     // doubles of squared residuals a workgroup of k_calib_cost holds (32 KiB)

__device__ __forceinline__ void calib_project(const double* __restrict__ c, double xi, double yi, double E, double N,
                                              double& tx, double& ty)
{
    const double sigma = c[9], H = c[10];
    const double den = (sigma * c[2] + xi * c[5]) + yi * c[8];
    tx = H * ((sigma * c[0] + xi * c[3]) + yi * c[6]) / den + E;
    ty = H * ((sigma * c[1] + xi * c[4]) + yi * c[7]) / den + N;
}

// distance from (tx, ty) to the nearest of the W vertices water[2 k], water[2 k + 1]
__device__ __forceinline__ double calib_nearest(const double* __restrict__ water, int W, double tx, double ty)
{
    // the eight fresh d2 of a batch are reduced among themselves before they meet the running minimum: the compiler
    // canonicalises a loop-carried operand of fmin (one v_max_f64), and this way does so once per batch
    double best = HUGE_VAL;
    int k = 0;
    for (; k + 8 <= W; k += 8) {
        double d[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const double dx = water[2 * (k + j)] - tx, dy = water[2 * (k + j) + 1] - ty;
            d[j] = dx * dx + dy * dy;
        }
        best = fmin(best, fmin(fmin(fmin(d[0], d[1]), fmin(d[2], d[3])), fmin(fmin(d[4], d[5]), fmin(d[6], d[7]))));
    }
    for (; k < W; k++) {
        const double dx = water[2 * k] - tx, dy = water[2 * k + 1] - ty;
        best = fmin(best, dx * dx + dy * dy);
    }
    const double d2 = best;
    return (tx != tx || ty != ty) ? __builtin_nan("") : sqrt(d2);
}

// one thread per (candidate, point), point fastest: out_dist (P, M), and tx, ty where asked for
__global__ __launch_bounds__(256) void k_calib_residuals(const double* __restrict__ cand, int P,
                                                         const double* __restrict__ shore, int M,
                                                         const double* __restrict__ water, int W, double E, double N,
                                                         double* __restrict__ out_dist, double* __restrict__ out_tx,
                                                         double* __restrict__ out_ty)
{
    const int i = blockIdx.x * 256 + threadIdx.x;   // P * M fits 31 bits (checked by the caller)
    if (i >= P * M) return;
    const int p = i / M, m = i - p * M;
    double tx, ty;
    calib_project(cand + (size_t)p * kCand, shore[2 * m], shore[2 * m + 1], E, N, tx, ty);
    out_dist[i] = calib_nearest(water, W, tx, ty);
    if (out_tx) out_tx[i] = tx;
    if (out_ty) out_ty[i] = ty;
}

struct SquaresAt {
    const double* sq;
    __device__ __forceinline__ double operator()(int t) const { return sq[t]; }
};

// the lattice form: a workgroup takes `cpb` consecutive candidates (cpb * M <= kCostLds), leaves the squared
// residuals in LDS, and one thread per candidate adds them in numpy's pairwise order: np.mean(res ** 2)
__global__ __launch_bounds__(256) void k_calib_cost(const double* __restrict__ cand, int P,
                                                    const double* __restrict__ shore, int M,
                                                    const double* __restrict__ water, int W, double E, double N,
                                                    int cpb, double* __restrict__ out_meansq)
{
    __shared__ double sq[kCostLds];
    const int c0 = blockIdx.x * cpb;
    const int nc = min(cpb, P - c0);
    const int items = nc * M;
    for (int i = threadIdx.x; i < items; i += 256) {
        const int pl = i / M, m = i - pl * M;
        double tx, ty;
        calib_project(cand + (size_t)(c0 + pl) * kCand, shore[2 * m], shore[2 * m + 1], E, N, tx, ty);
        const double d = calib_nearest(water, W, tx, ty);
        sq[i] = d * d;
    }
    __syncthreads();
    if ((int)threadIdx.x < nc)
        out_meansq[c0 + threadIdx.x] = np_pairwise_sum(SquaresAt{sq + threadIdx.x * M}, M) / (double)M;
}

}  // namespace

int calib_cost_max_points() { return kCostLds; }

void launch_calib_residuals(hipStream_t s, const double* cand, int P, const double* shore, int M, const double* water,
                            int W, double E, double N, double* out_dist, double* out_tx, double* out_ty)
{
    const long long n = (long long)P * M;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_calib_residuals, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cand, P, shore, M, water,
                       W, E, N, out_dist, out_tx, out_ty);
}

void launch_calib_cost(hipStream_t s, const double* cand, int P, const double* shore, int M, const double* water, int W,
                       double E, double N, double* out_meansq)
{
    if (P <= 0 || M <= 0 || M > kCostLds) return;
    const int cpb = std::min(256, kCostLds / M);
    hipLaunchKernelGGL(k_calib_cost, dim3((unsigned)((P + cpb - 1) / cpb)), dim3(256), 0, s, cand, P, shore, M, water, W,
                       E, N, cpb, out_meansq);
}

}  // namespace icelk
