// join_kernels.hip -- the hash join of two accumulators (dnagpu_acc_join): for every group of `left` the
// count its key has in `right` (0: none), the rows of the asked kind compacted to three arrays, six statistics over them.
//
// Both tables hash alike -- partition = the top pbits bits of h = splitmix64(key), home slot = the low 12 bits -- so
// partition q of a table of b bits holds, by key, a subset of partition q >> (b - a) of any table of a <= b bits: the two
// sides line up partition by partition with no binning pass.  Two kernels find a left group's partner and share one body
// (JoinRows / join_emit) for what follows:
//   partition path: one workgroup per partition q of the FINER side (f = max(s, t) bits).  It loads right's partition
//     q >> (f - t) into LDS, streams left's partition q >> (f - s) and probes LDS for the groups whose hash says q.
//   direct path: one workgroup per tile of left's slots; every group probes right's table in global memory.
// The body ranks the workgroup's result rows with a block scan, takes ONE returning atomic on the cursor for all of them,
// stores the rows below `cap`, and adds the statistics with one global atomic per statistic per workgroup.  No kernel
// writes to a table, and a partition with occ == 0 (its slots hold nothing defined) is never read.
#include <hip/hip_runtime.h>

#include "acc_device.hpp"

namespace dnagpu {

namespace {

constexpr int JOIN_PER_T = 8;                              // left slots per thread, in both kernels
constexpr int DIRECT_NT = 256;
constexpr int DIRECT_TILE = DIRECT_NT * JOIN_PER_T;        // QAccSrc's tiling: a tile lies inside one partition
static_assert(ACC_PER_T == JOIN_PER_T, "the partition path streams a partition eight slots per thread");
static_assert(ACC_SLOTS % DIRECT_TILE == 0, "a tile must lie inside one accumulator partition");
constexpr int JOIN_SUMS = JOIN_RES_WORDS - 1;              // the statistics that are not the cursor

// a thread's left groups: mask bit j = slot j is live (count != 0, and this workgroup's to handle)
struct JoinRows {
    u64 key[JOIN_PER_T], cl[JOIN_PER_T], cr[JOIN_PER_T];
    u32 mask;
};

template <int NT>
struct JoinShared {
    u32 arr[NT];
    u32 wtmp[NT / 64];
    u64 base;
    u64 part[JOIN_SUMS][NT / 64];
};

// the shared body: which live rows are result rows of a.kind, their places, their statistics
template <int NT>
__device__ __forceinline__ void join_emit(const JoinArgs &a, const JoinRows &r, JoinShared<NT> &sh)
{
    const int tid = threadIdx.x;
    u32 res = 0;
    u64 sum[JOIN_SUMS] = {0, 0, 0, 0, 0};                  // res[1 ..]: sum_left, sum_right, sum_min, checksum_left, checksum_right
#pragma unroll
    for (int j = 0; j < JOIN_PER_T; j++) {
        if (!(r.mask & (1u << j)))
            continue;
        const bool hit = r.cr[j] != 0;
        if (a.kind == JOIN_KIND_INNER ? !hit : a.kind == JOIN_KIND_ANTI ? hit : false)
            continue;
        res |= 1u << j;
        sum[0] += r.cl[j];
        sum[1] += r.cr[j];
        sum[2] += r.cl[j] < r.cr[j] ? r.cl[j] : r.cr[j];
        sum[3] += pair_mix(r.key[j], r.cl[j]);
        if (hit)
            sum[4] += pair_mix(r.key[j], r.cr[j]);
    }
    const u32 total = block_scan_value<NT>((u32)__builtin_popcount(res), sh.arr, NT, sh.wtmp, tid);
    if (total == 0)
        return;
    if (tid == 0)
        sh.base = atomicAdd(a.res, (unsigned long long)total);
#pragma unroll
    for (int i = 0; i < JOIN_SUMS; i++) {
        u64 v = sum[i];
        for (int off = 32; off > 0; off >>= 1)
            v += __shfl_down(v, off);
        if ((tid & 63) == 0)
            sh.part[i][tid >> 6] = v;
    }
    __syncthreads();
    if (tid < JOIN_SUMS) {
        u64 v = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; w++)
            v += sh.part[tid][w];
        if (v)
            atomicAdd(a.res + 1 + tid, (unsigned long long)v);
    }
    u64 at = sh.base + sh.arr[tid];                        // (>= a.out_base: the cursor only grows)
#pragma unroll
    for (int j = 0; j < JOIN_PER_T; j++) {
        if (!(res & (1u << j)))
            continue;
        if (at < a.cap) {
            const u64 o = at - a.out_base;
            if (a.out_keys)
                a.out_keys[o] = r.key[j];
            if (a.out_left)
                a.out_left[o] = r.cl[j];
            if (a.out_right)
                a.out_right[o] = r.cr[j];
        }
        at++;
    }
}

}  // namespace

// One workgroup per partition q0 + blockIdx.x of the finer side.
__global__ __launch_bounds__(ACC_NT) void join_partition_kernel(JoinArgs a, u64 q0)
{
    __shared__ u64 lds[2 * ACC_SLOTS];
    __shared__ JoinShared<ACC_NT> sh;
    const int f = a.s > a.t ? a.s : a.t;
    const u64 q = q0 + blockIdx.x;
    const u64 ps = q >> (f - a.s);
    if (a.l_occ[ps] == 0)
        return;
    bool have_right = false;
    if (a.r_table) {
        const u64 pt = q >> (f - a.t);
        have_right = a.r_occ[pt] != 0;
        if (have_right)
            load_region(lds, a.r_table + 2 * pt * ACC_SLOTS, true);
    }
    __syncthreads();
    const u64 *src = a.l_table + 2 * ps * ACC_SLOTS;
    JoinRows r;
    r.mask = 0;
#pragma unroll
    for (int j = 0; j < JOIN_PER_T; j++) {
        ld_slot(src + 2 * ((u64)j * ACC_NT + threadIdx.x), r.key[j], r.cl[j]);
        r.cr[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < JOIN_PER_T; j++) {
        if (r.cl[j] == 0)
            continue;
        const u64 h = splitmix64(r.key[j]);
        if ((h >> (64 - f)) != q)                          // (never when f == s: the group lives in ps == q)
            continue;
        r.mask |= 1u << j;
        if (!have_right)
            continue;
        u32 sl = acc_home(h);
        for (int probe = 0; probe < ACC_SLOTS; probe++) {
            const u64 c = lds[2 * sl + 1];
            if (c == 0)
                break;
            if (lds[2 * sl] == r.key[j]) {
                r.cr[j] = c;
                break;
            }
            sl = (sl + 1) & (ACC_SLOTS - 1);
        }
    }
    join_emit<ACC_NT>(a, r, sh);
}

// One workgroup per tile tile0 + blockIdx.x of DIRECT_TILE slots of left.
__global__ __launch_bounds__(DIRECT_NT) void join_direct_kernel(JoinArgs a, u64 tile0)
{
    __shared__ JoinShared<DIRECT_NT> sh;
    const u64 t = tile0 + blockIdx.x;
    if (a.l_occ[(t * DIRECT_TILE) / ACC_SLOTS] == 0)
        return;
    const u64 *src = a.l_table + 2 * t * DIRECT_TILE;
    JoinRows r;
    r.mask = 0;
#pragma unroll
    for (int j = 0; j < JOIN_PER_T; j++) {
        ld_slot(src + 2 * ((u64)j * DIRECT_NT + threadIdx.x), r.key[j], r.cl[j]);
        r.cr[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < JOIN_PER_T; j++) {
        if (r.cl[j] == 0)
            continue;
        r.mask |= 1u << j;
        if (!a.r_table)
            continue;
        const u64 h = splitmix64(r.key[j]);
        const u64 pt = h >> (64 - a.t);
        if (a.r_occ[pt] == 0)
            continue;
        const u64 *region = a.r_table + 2 * pt * ACC_SLOTS;
        u32 sl = acc_home(h);
        for (int probe = 0; probe < ACC_SLOTS; probe++) {
            u64 k, c;
            ld_slot(region + 2 * (u64)sl, k, c);
            if (c == 0)
                break;
            if (k == r.key[j]) {
                r.cr[j] = c;
                break;
            }
            sl = (sl + 1) & (ACC_SLOTS - 1);
        }
    }
    join_emit<DIRECT_NT>(a, r, sh);
}

hipError_t launch_join_partition(const JoinArgs &a, u64 p_lo, u64 n_parts, hipStream_t st)
{
    const int f = a.s > a.t ? a.s : a.t;
    const u64 n = n_parts << (f - a.s);
    if (n == 0)
        return hipSuccess;
    if (n > 0x7fffffffull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(join_partition_kernel, dim3((unsigned)n), dim3(ACC_NT), 0, st, a, p_lo << (f - a.s));
    return hipGetLastError();
}

hipError_t launch_join_direct(const JoinArgs &a, u64 p_lo, u64 n_parts, hipStream_t st)
{
    const u64 per = ACC_SLOTS / DIRECT_TILE, n = n_parts * per;
    if (n == 0)
        return hipSuccess;
    if (n > 0x7fffffffull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(join_direct_kernel, dim3((unsigned)n), dim3(DIRECT_NT), 0, st, a, p_lo * per);
    return hipGetLastError();
}

}  // namespace dnagpu
