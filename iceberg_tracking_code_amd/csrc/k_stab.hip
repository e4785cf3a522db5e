// k_stab.hip -- camera shake fitted to land anchors on the device.  The rules are stab.h's, which the host
// statement runs as well; the five kernels go out on one stream with no host look between them (abi_stab.hip):
//   k_stab_flags    one thread per row: the row's flag (the caller's byte, or the anchor mask under vertex 0) and whether it is
//                   an anchor (flag and all 2 V coordinates finite)
//   k_stab_compact  ONE workgroup of 1024: thread x counts the anchors of its contiguous run of rows, an exclusive scan of the
//                   counts, then it writes its run's row numbers behind those of the threads before it -- idx is ascending,
//                   *n_a the total.  Every later kernel reads n_a from there
//   k_stab_median   one workgroup of 256 per (vertex, component): X - x or Y - y staged as order keys, wg_median of
//                   grid_select_wg.h.  The anchors are finite floats, so no term is a NaN
//   k_stab_rounds   one workgroup of 256 per vertex runs stab.h's fit_vertex to its end; all threads carry the same values.
//                   An inlier pass is a strided loop with the count and the "differs" flag joined in LDS.  A sum is np_sum's
//                   additions dealt out: per chunk of at most 8192 terms thread 0 walks np_pairwise_sum's stack machine once
//                   to list the leaves (np_pairwise_walk with ListLeaves; the list depends on the chunk's length alone and is
//                   kept while that stays), the threads compute np_leaf_sum of (sum, leaf) pairs -- cut along its eight
//                   accumulators, a thread per chain, then joined (np_leaf_lane, np_leaf_join) --, and thread s walks the
//                   same machine again for sum s with the leaves' values handed out in order (ReplayLeaves) and adds the
//                   chunk to its accumulator as np_sum_onto does.  The machine decides which values are added and in which
//                   order, and it is the same text in all three uses, so the additions are np_sum's
//   k_stab_apply    one thread per (row, vertex), in place; vertex 0 and vertices under TOO_FEW or LOST are left as they are
// The table has A.n rows, or, with A.n_ptr set, the *n_ptr <= A.n rows a gather on the same stream has just counted: the
// grids are sized for A.n and the kernels clamp what they read to it.
// Bounds: tracks holds n V 2 floats; flags, anchor and idx n entries; keys (V - 1) 2 stretches of `stride` >= n entries;
// w (V - 1) stretches of `stride` >= n bytes; med 2 (V - 1) doubles; res V - 1 entries.  n_a <= n by construction (each
// thread of k_stab_compact writes as many entries as it counted, inside [0, n)).  The mask is mw x mh bytes, rows mw apart,
// and mask_flag reads it only inside.
#include "icelk_internal.h"
#include "grid_select_wg.h"
#include "stab.h"

namespace icelk {

namespace {

using namespace stab;

// the table's rows: n_max where the host knows them, *n_ptr <= n_max where only the device does (a segment's gather)
__device__ __forceinline__ int rows_of(int n_max, const int* __restrict__ n_ptr)
{
    if (!n_ptr) return n_max;
    const int n = *n_ptr;
    return n < 0 ? 0 : (n < n_max ? n : n_max);
}

__global__ __launch_bounds__(256) void k_stab_flags(const float* __restrict__ tracks, int n_max, const int* __restrict__ n_ptr, int V,
                                                    const uint8_t* in_flags, const uint8_t* __restrict__ mask, int mw, int mh,
                                                    uint8_t* flags, uint8_t* __restrict__ anchor)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows_of(n_max, n_ptr)) return;
    const float* row = tracks + (size_t)i * V * 2;
    const uint8_t f = in_flags ? (in_flags[i] != 0 ? 1 : 0) : mask_flag(row[0], row[1], mask, mw, mh, (size_t)mw);
    flags[i] = f;
    anchor[i] = f && row_finite(row, V) ? 1 : 0;
}

constexpr int kCompactThreads = 1024;

__global__ __launch_bounds__(kCompactThreads) void k_stab_compact(const uint8_t* __restrict__ anchor, int n_max,
                                                                  const int* __restrict__ n_ptr, int* __restrict__ idx,
                                                                  int* __restrict__ n_a)
{
    __shared__ int scan[kCompactThreads];
    const int tid = threadIdx.x;
    const int n = rows_of(n_max, n_ptr);
    const int per = (n + kCompactThreads - 1) / kCompactThreads;
    const int b = tid * per < n ? tid * per : n, e = b + per < n ? b + per : n;
    int mine = 0;
    for (int i = b; i < e; i++) mine += anchor[i];
    scan[tid] = mine;
    __syncthreads();
    for (int o = 1; o < kCompactThreads; o <<= 1) {
        const int add = tid >= o ? scan[tid - o] : 0;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    int at = scan[tid] - mine;
    for (int i = b; i < e; i++)
        if (anchor[i]) idx[at++] = i;
    if (tid == kCompactThreads - 1) *n_a = scan[tid];
}

__global__ __launch_bounds__(256) void k_stab_median(const float* __restrict__ tracks, const int* __restrict__ idx,
                                                     const int* __restrict__ n_a_ptr, int V, int min_anchors,
                                                     unsigned long long* __restrict__ keys, size_t stride, double* __restrict__ med)
{
    __shared__ SelectLds lds;
    const int n_a = *n_a_ptr;
    if (n_a < min_anchors) return;   // TOO_FEW: nobody reads a median (min_anchors >= 2, so wg_median sees n >= 1)
    const int comp = blockIdx.y;
    unsigned long long* __restrict__ sk = keys + ((size_t)blockIdx.x * 2 + comp) * stride;
    const ShiftAt at{Anchors{tracks, idx, V, (int)blockIdx.x + 1}, comp};
    // thread x stages and later reads terms x, x + 256, ... only, as in k_grid_select
    for (int t = threadIdx.x; t < n_a; t += 256) sk[t] = order_key(at(t));
    const double m = wg_median(sk, n_a, &lds);
    if (threadIdx.x == 0) med[blockIdx.x * 2 + comp] = m;
}

constexpr int kMaxSums = 7;   // the sums fit() asks for at once
constexpr int kRoundsThreads = 256;   // k_stab_rounds' workgroup

constexpr int kLeafBatch = 32;   // leaves whose accumulators are in LDS at a time

struct RoundsLds {
    LeafSpan leaf[kMaxLeaves];
    double vals[kMaxSums][kMaxLeaves];
    double lane[kMaxSums][kLeafBatch][8];
    double out[T_COUNT];
    int nleaf, listed_len, count, differ;
};

struct WgEngine {
    TermCtx C;
    uint8_t* w;
    int n_a;
    const double* med;
    RoundsLds* L;

    __device__ double median(int comp) const { return med[comp]; }

    __device__ int inliers(const Model& m, double g, bool* same)
    {
        if (threadIdx.x == 0) L->count = 0, L->differ = 0;
        __syncthreads();
        const double gg = g * g;
        int count = 0, differ = 0;
        for (int t = threadIdx.x; t < n_a; t += kRoundsThreads) {
            const uint8_t v = residual2(m, C.A.x(t), C.A.y(t), C.A.X(t), C.A.Y(t)) <= gg ? 1 : 0;
            differ |= v != w[t];
            w[t] = v;
            count += v;
        }
        if (count) atomicAdd(&L->count, count);
        if (differ) atomicOr(&L->differ, 1);
        __syncthreads();   // the count is whole, and every w[t] is written before a sum's leaf reads it
        const int total = L->count;
        *same = L->differ == 0;
        __syncthreads();   // read by all before the next pass resets them
        return total;
    }

    __device__ void sums(unsigned terms, const Means& c, const Model& m, double* out)
    {
        C.c = c, C.m = m;
        int which[kMaxSums], ns = 0;
        for (int T = 0; T < T_COUNT; T++)
            if ((terms >> T & 1) && ns < kMaxSums) which[ns++] = T;
        const int tid = threadIdx.x;
        double acc = 0.0;
        for (int first = 0; first < n_a; first += kNpBufferSize) {
            const int len = n_a - first < kNpBufferSize ? n_a - first : kNpBufferSize;
            if (tid == 0 && L->listed_len != len) {
                ListLeaves list{L->leaf, 0};
                np_pairwise_walk(list, len, 0);
                L->nleaf = list.count, L->listed_len = len;
            }
            __syncthreads();
            const int nleaf = L->nleaf;
            if (nleaf <= kMaxLeaves) {
                for (int l0 = 0; l0 < nleaf; l0 += kLeafBatch) {
                    const int nb = nleaf - l0 < kLeafBatch ? nleaf - l0 : kLeafBatch;
                    // a thread per (sum, leaf, accumulator): the eight chains of np_leaf_sum side by side
                    for (int item = tid; item < ns * nb * 8; item += kRoundsThreads) {
                        const int j = item & 7, sl = item >> 3, s = sl / nb, l = sl - s * nb;
                        const LeafSpan leaf = L->leaf[l0 + l];
                        if (leaf.len >= 8) L->lane[s][l][j] = with_term(which[s], C, LaneSum{first + leaf.start, leaf.len, j});
                    }
                    __syncthreads();
                    // a thread per (sum, leaf): the accumulators joined and the tail added; a leaf below 8 terms as it is
                    for (int item = tid; item < ns * nb; item += kRoundsThreads) {
                        const int s = item / nb, l = item - s * nb;
                        const LeafSpan leaf = L->leaf[l0 + l];
                        L->vals[s][l0 + l] = leaf.len >= 8 ? with_term(which[s], C, JoinSum{L->lane[s][l], first + leaf.start, leaf.len})
                                                           : leaf_of(which[s], C, first + leaf.start, leaf.len);
                    }
                    __syncthreads();
                }
                if (tid < ns) {
                    ReplayLeaves replay{L->vals[tid], 0};
                    acc = acc + np_pairwise_walk(replay, len, 0);
                }
            } else if (tid < ns) {   // (more leaves than the table holds: no chunk of at most 8192 terms has them)
                ComputeLeaves compute{which[tid], C};
                acc = acc + np_pairwise_walk(compute, len, first);
            }
            __syncthreads();   // vals and the list are free again
        }
        if (tid < ns) L->out[which[tid]] = acc;
        __syncthreads();
        for (int T = 0; T < T_COUNT; T++)
            if (terms >> T & 1) out[T] = L->out[T];
        __syncthreads();
    }
};

__global__ __launch_bounds__(kRoundsThreads) void k_stab_rounds(const float* __restrict__ tracks, const int* __restrict__ idx,
                                                     const int* __restrict__ n_a_ptr, int V, icelk_stab_params_t P,
                                                     const double* __restrict__ med, uint8_t* w, size_t stride, VertexResult* __restrict__ res)
{
    __shared__ RoundsLds lds;
    const int n_a = *n_a_ptr;
    uint8_t* wk = w + (size_t)blockIdx.x * stride;
    for (int t = threadIdx.x; t < n_a; t += kRoundsThreads) wk[t] = 0;
    if (threadIdx.x == 0) lds.listed_len = -1;
    __syncthreads();
    const Means none{0.0, 0.0, 0.0, 0.0};
    WgEngine E{TermCtx{Anchors{tracks, idx, V, (int)blockIdx.x + 1}, wk, none, Model{1.0, 0.0, 0.0, 0.0}}, wk, n_a, med + blockIdx.x * 2, &lds};
    const VertexResult R = fit_vertex(E, n_a, P);
    if (threadIdx.x == 0) res[blockIdx.x] = R;
}

__global__ __launch_bounds__(256) void k_stab_apply(float* tracks, int n_max, const int* __restrict__ n_ptr, int V,
                                                    const VertexResult* __restrict__ res)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (size_t)rows_of(n_max, n_ptr) * V) return;
    const int k = (int)(g % V);
    if (k == 0) return;
    const VertexResult R = res[k - 1];
    if (is_identity(R.status)) return;
    float* p = tracks + g * 2;
    apply_point(R.m, p[0], p[1], p, p + 1);
}

}  // namespace

void launch_stab_step(hipStream_t s, const StabArgs& A, int step)
{
    const size_t items = (size_t)A.n * A.V;
    switch (step) {
    case STAB_FLAGS:
        if (A.n > 0)
            hipLaunchKernelGGL(k_stab_flags, dim3((A.n + 255) / 256), dim3(256), 0, s, A.tracks, A.n, A.n_ptr, A.V, A.in_flags, A.mask,
                               A.mask_w, A.mask_h, A.flags, A.anchor);
        break;
    case STAB_COMPACT:
        hipLaunchKernelGGL(k_stab_compact, dim3(1), dim3(kCompactThreads), 0, s, A.anchor, A.n, A.n_ptr, A.idx, A.n_a);
        break;
    case STAB_MEDIAN:
        hipLaunchKernelGGL(k_stab_median, dim3(A.V - 1, 2), dim3(256), 0, s, A.tracks, A.idx, A.n_a, A.V, A.P.min_anchors, A.keys, A.stride,
                           A.med);
        break;
    case STAB_ROUNDS:
        hipLaunchKernelGGL(k_stab_rounds, dim3(A.V - 1), dim3(kRoundsThreads), 0, s, A.tracks, A.idx, A.n_a, A.V, A.P, A.med, A.w, A.stride, A.res);
        break;
    default:
        if (A.n > 0)
            hipLaunchKernelGGL(k_stab_apply, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, A.tracks, A.n, A.n_ptr, A.V, A.res);
        break;
    }
}

}  // namespace icelk
