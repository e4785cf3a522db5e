// k_validate.hip -- the normalised median test on the device (the rules are validate.h's, the host's
// statement of them validate::run_host).
//
//   assign   one thread per point: the judged points get the key ((g * ncells + j * cols + i) << 32) | p, slots from one
//            workgroup scan and one atomic per workgroup (key_slots); the others get status 3 and a NaN r2.  The group is
//            the caller's (k_validate_assign) or the point's window of the day tables (k_validate_day_assign: day_window,
//            the gridder's rule, unchanged).
//   sort     the gridder's (k_sort.hip), by the caller.
//   pools    one workgroup of 256 per (group, cell) and velocity component.  Eight threads find the pool's three runs and
//            the cell's own by binary search; a cell without a point of its own writes its empty record and returns.  The
//            median and the MAD are wg_median_of's eight-pass select over the pool's order keys: a pool of at most
//            kPoolLds terms stages them in LDS once (the MAD's overwrite them in place), a larger one computes them from
//            global memory on every pass.  Both are one code shape (pool_median_mad) with two fetchers.
//   judge    one thread per sorted key: status and r2 of its point, the time of a rejected point set to NaN where the day
//            form asks for it, and the group's rejected count, combined within the wave before the atomic.
//
// kPoolLds = 2048: 16 KB of keys beside the select's 1 KB.  A CU holds 32 waves, eight workgroups of 256, and 160 KB of LDS,
// 20 KB per workgroup at that occupancy: 2048 keys is the largest power of two at which LDS does not cost a wave.  A pool
// of a 3 x 3 neighbourhood with the ~40-400 points per cell met here stays well below it.
//
// Memory besides the caller's arrays: the keys and the sorted keys (8 n bytes each) and the sort's own scratch; the pool
// kernel needs none -- 16 n bytes plus the sort's, whatever the pools' sizes.  The per-(group, cell) record is 36 bytes.
// Bounds: a key slot is below the number of judged points <= n (one key per point at most, and checked); every index into
// the sorted keys is below `total`, the judged count read back by the caller; a segment is below ngroups * ncells < 2^31
// (validate::check); a staged term is below pool.n <= kPoolLds.
#include "icelk_internal.h"
#include "grid_keys.h"
#include "grid_select_wg.h"
#include "validate.h"

namespace icelk {

namespace {

using validate::Pool;
using validate::PoolAt;

constexpr int kPoolLds = 2048;

__device__ __forceinline__ void assign_point(const ValidateArgs& A, int p, int g)
{
    int i = 0, j = 0;
    const bool live = p < A.n;
    const bool judged = live && g >= 0 && g < A.ngroups && validate::cell_of(A.L, A.x[p], A.y[p], A.u[p], A.v[p], &i, &j);
    const int at = key_slots(judged ? 1 : 0, A.key_count);
    if (judged) {
        const unsigned ncells = (unsigned)A.L.cols * (unsigned)A.L.rows;
        if (at >= 0 && at < A.n) A.keys[at] = validate::make_key((unsigned)g * ncells + (unsigned)j * (unsigned)A.L.cols + (unsigned)i, p);
    } else if (live) {
        A.status[p] = validate::kNotJudged;
        A.r2[p] = __builtin_nan("");
    }
}

__global__ __launch_bounds__(256) void k_validate_assign(ValidateArgs A)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    assign_point(A, p, p < A.n && A.group ? A.group[p] : 0);
}

__global__ __launch_bounds__(256) void k_validate_day_assign(ValidateArgs A, const double* __restrict__ t, DayTables D)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    int cam = 0;
    double tp = 0.0;
    assign_point(A, p, day_window(D, t, p, A.n, &cam, &tp));
}

struct PoolShared {
    SelectLds sel;
    int bound[8];
    unsigned long long keys[kPoolLds];
};

// The two fetchers of the pool kernel.  load(at, n, med, dev): what the select is to see from now on -- the terms at(t), or
// with `dev` fabs(at(t) - med); every thread calls it.  operator[](t): term t's order key.
struct StagedKeys {   // n <= kPoolLds: staged once; thread x stages and re-stages terms x, x + 256, ... only
    unsigned long long* lds;
    __device__ __forceinline__ void load(const PoolAt& at, int n, double med, bool dev)
    {
        for (int t = threadIdx.x; t < n; t += 256) lds[t] = order_key(dev ? fabs(from_order_key(lds[t]) - med) : at(t));
        __syncthreads();
    }
    __device__ __forceinline__ unsigned long long operator[](int t) const { return lds[t]; }
};

struct WalkedKeys {   // any n: gathered through the sorted keys whenever asked
    PoolAt at;
    double med;
    bool dev;
    __device__ __forceinline__ void load(const PoolAt& at_, int, double med_, bool dev_) { at = at_, med = med_, dev = dev_; }
    __device__ __forceinline__ unsigned long long operator[](int t) const
    {
        const double a = at(t);
        return order_key(dev ? fabs(a - med) : a);
    }
};

template <typename Keys>
__device__ __forceinline__ void pool_median_mad(Keys& keys, const PoolAt& at, int n, SelectLds* L, double* med, double* mad)
{
    keys.load(at, n, 0.0, false);
    *med = wg_median_of(keys, n, L);
    keys.load(at, n, *med, true);
    *mad = wg_median_of(keys, n, L);
}

__global__ __launch_bounds__(256) void k_validate_pools(ValidateArgs A, int total)
{
    __shared__ PoolShared S;
    const unsigned seg = blockIdx.x;
    if (threadIdx.x < 8) S.bound[threadIdx.x] = validate::pool_bound(A.L, A.sorted, total, seg, (int)threadIdx.x);
    __syncthreads();
    const Pool pool = validate::pool_from_bounds(S.bound);
    double* const out_med = blockIdx.y ? A.cells.med_v : A.cells.med_u;
    double* const out_mad = blockIdx.y ? A.cells.mad_v : A.cells.mad_u;
    if (pool.own_count <= 0) {   // the whole workgroup alike
        if (threadIdx.x == 0) {
            if (blockIdx.y == 0) A.cells.pool_n[seg] = 0;
            out_med[seg] = out_mad[seg] = __builtin_nan("");
        }
        return;
    }
    const PoolAt at{A.sorted, blockIdx.y ? A.v : A.u, pool};
    double med, mad;
    if (pool.n <= kPoolLds) {
        StagedKeys keys{S.keys};
        pool_median_mad(keys, at, pool.n, &S.sel, &med, &mad);
    } else {
        WalkedKeys keys{at, 0.0, false};
        pool_median_mad(keys, at, pool.n, &S.sel, &med, &mad);
    }
    if (threadIdx.x == 0) {
        if (blockIdx.y == 0) A.cells.pool_n[seg] = pool.n;
        out_med[seg] = med;
        out_mad[seg] = mad;
    }
}

// one more rejected point in group g (-1: none), the lanes of one group combined first: the keys are sorted by group, so
// nearly always one group per wave and one atomic.  Called by every lane of the wave.
__device__ __forceinline__ void count_rejected(int g, int32_t* __restrict__ rejected)
{
    unsigned long long pending = __ballot(g >= 0);
    while (pending) {
        const int leader = __ffsll((long long)pending) - 1;
        const int g0 = __shfl(g, leader);
        const unsigned long long mine = __ballot(g == g0);
        if ((threadIdx.x & 63) == leader) atomicAdd(&rejected[g0], (int32_t)__popcll(mine));
        pending &= ~mine;
    }
}

__global__ __launch_bounds__(256) void k_validate_judge(ValidateArgs A, int total)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    int g = -1;
    if (k < total) {
        const unsigned long long key = A.sorted[k];
        const unsigned seg = (unsigned)(key >> 32), p = (unsigned)key;
        double r2;
        const uint8_t st = validate::judge(A.u[p], A.v[p], A.cells.pool_n[seg], A.cells.med_u[seg], A.cells.mad_u[seg], A.cells.med_v[seg],
                                           A.cells.mad_v[seg], A.P, &r2);
        A.status[p] = st;
        A.r2[p] = r2;
        if (st == validate::kRejected) {
            g = (int)(seg / ((unsigned)A.L.cols * (unsigned)A.L.rows));
            if (A.t_kill) A.t_kill[p] = __builtin_nan("");
        }
    }
    count_rejected(g, A.rejected);
}

}  // namespace

void launch_validate_assign(hipStream_t s, const ValidateArgs& A)
{
    if (A.n <= 0) return;
    hipLaunchKernelGGL(k_validate_assign, dim3((A.n + 255) / 256), dim3(256), 0, s, A);
}

void launch_validate_day_assign(hipStream_t s, const ValidateArgs& A, const double* t, const long long* file_off, const int* file_cam,
                                const int* win_f0, const int* win_f1, int nfiles, const long long* t_lo, const long long* t_hi, int ncam,
                                int nw)
{
    if (A.n <= 0) return;
    const DayTables D{file_off, file_cam, win_f0, win_f1, t_lo, t_hi, nfiles, ncam, nw};
    hipLaunchKernelGGL(k_validate_day_assign, dim3((A.n + 255) / 256), dim3(256), 0, s, A, t, D);
}

void launch_validate_pools(hipStream_t s, const ValidateArgs& A, int total)
{
    const long long nseg = (long long)A.ngroups * A.L.cols * A.L.rows;
    if (nseg <= 0) return;
    hipLaunchKernelGGL(k_validate_pools, dim3((unsigned)nseg, 2), dim3(256), 0, s, A, total);
}

void launch_validate_judge(hipStream_t s, const ValidateArgs& A, int total)
{
    if (total <= 0) return;
    hipLaunchKernelGGL(k_validate_judge, dim3((total + 255) / 256), dim3(256), 0, s, A, total);
}

int validate_pool_lds_terms() { return kPoolLds; }

}  // namespace icelk
