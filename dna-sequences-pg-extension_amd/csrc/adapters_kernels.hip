// adapters_kernels.hip -- the kernels of dnagpu_dna_adapters: the 3' adapter cut of every segment of a
// packed stream, the verdicts with the report, and the passing list.  The window arithmetic, the hit key and the sixteen
// positions of one lane are adapters_math.hpp's.  Integer VALU only; no atomic per position.
//
// Every kernel begins with `if (*bad) return`: the validation of the caller's lists (launch_take_segments) runs before them
// on the same stream and sets that word, so that a list with a segment that leaves the stream reads nothing through it and
// writes nothing to the caller's arrays, without a read-back in between.
#include <hip/hip_runtime.h>

#include "adapters_math.hpp"
#include "kernels.hpp"

namespace dnagpu {

namespace {

__device__ __forceinline__ void seg_of(const AdapterSegs &g, u64 i, u64 *first, u64 *n)
{
    if (g.first) {
        *first = g.first[i];
        *n = g.len[i];
    } else {
        *first = g.starts[i];
        *n = g.starts[i + 1] - *first;
    }
}

// the descriptors into LDS, by the whole workgroup; synchronises
__device__ __forceinline__ void ads_to_lds(const AdapterDesc *__restrict__ ads, u32 n_ads, AdapterDesc *s_ads)
{
    const u64 *src = reinterpret_cast<const u64 *>(ads);
    u64 *dst = reinterpret_cast<u64 *>(s_ads);
    for (u32 i = threadIdx.x; i < n_ads * (u32)(sizeof(AdapterDesc) / 8); i += ADAPTERS_THREADS)
        dst[i] = src[i];
    __syncthreads();
}

// the minimum over a team of LANES lanes of one wave, in every lane of it
template <u32 LANES>
__device__ __forceinline__ u64 team_min(u64 v)
{
#pragma unroll
    for (u32 off = LANES / 2; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(v, off, LANES);
        v = o < v ? o : v;
    }
    return v;
}

}  // namespace

// ---- a group of ADAPTERS_GROUP_LANES lanes per segment, segment = the group's index in the grid.  A segment of more than
// ADAPTERS_GROUP_BASES bases is handed on by id: into the wave list or the workgroup list (lists[0 .. n) and lists[n .. 2 n);
// counts[0], counts[1] zero before the launch), one atomic per such segment.  keys[i] = the segment's cut, or ADAPTERS_NONE.
__global__ __launch_bounds__(ADAPTERS_THREADS) void adapters_group_kernel(const u64 *__restrict__ words, const AdapterSegs g,
                                                                         const AdapterDesc *__restrict__ ads, u32 n_ads,
                                                                         const unsigned long long *__restrict__ bad,
                                                                         u64 *__restrict__ keys, u32 *__restrict__ lists,
                                                                         u32 *__restrict__ counts)
{
    __shared__ AdapterDesc s_ads[ADAPTERS_MAX];
    if (*bad)
        return;
    ads_to_lds(ads, n_ads, s_ads);
    const u64 i = ((u64)blockIdx.x * ADAPTERS_THREADS + threadIdx.x) / ADAPTERS_GROUP_LANES;
    const u32 rank = threadIdx.x & (ADAPTERS_GROUP_LANES - 1);
    u64 first = 0, n = 0;
    if (i < g.n)
        seg_of(g, i, &first, &n);
    const bool longer = n > ADAPTERS_GROUP_BASES;
    if (longer && rank == 0) {
        const u32 cls = n > ADAPTERS_WAVE_BASES ? 1u : 0u;
        lists[(u64)cls * g.n + atomicAdd(&counts[cls], 1u)] = (u32)i;
    }
    const u64 mine = adapter_lane_best([&](u64 w) { return words[w]; }, first, longer ? 0 : n, (u64)rank * ADAPTERS_LANE_POS, s_ads, n_ads);
    const u64 key = team_min<ADAPTERS_GROUP_LANES>(mine);
    if (i < g.n && !longer && rank == 0)
        keys[i] = key;
}

// ---- the segments of the wave list: one wave each, the waves of the grid stride over the list
__global__ __launch_bounds__(ADAPTERS_THREADS) void adapters_wave_kernel(const u64 *__restrict__ words, const AdapterSegs g,
                                                                        const AdapterDesc *__restrict__ ads, u32 n_ads,
                                                                        const unsigned long long *__restrict__ bad,
                                                                        u64 *__restrict__ keys, const u32 *__restrict__ list,
                                                                        const u32 *__restrict__ count)
{
    __shared__ AdapterDesc s_ads[ADAPTERS_MAX];
    if (*bad)
        return;
    ads_to_lds(ads, n_ads, s_ads);
    const u32 waves = gridDim.x * (ADAPTERS_THREADS / 64), m = *count, lane = threadIdx.x & 63;
    for (u32 j = blockIdx.x * (ADAPTERS_THREADS / 64) + (threadIdx.x >> 6); j < m; j += waves) {     // (uniform in the wave)
        const u64 i = list[j];
        u64 first, n;
        seg_of(g, i, &first, &n);
        const u64 mine = adapter_lane_best([&](u64 w) { return words[w]; }, first, n, (u64)lane * ADAPTERS_LANE_POS, s_ads, n_ads);
        const u64 key = team_min<64>(mine);
        if (lane == 0)
            keys[i] = key;
    }
}

// ---- the segments of the workgroup list: one workgroup each, tile after tile from the front; the first tile that holds a
// hit ends the walk, because the lowest position wins
__global__ __launch_bounds__(ADAPTERS_THREADS) void adapters_block_kernel(const u64 *__restrict__ words, const AdapterSegs g,
                                                                         const AdapterDesc *__restrict__ ads, u32 n_ads,
                                                                         const unsigned long long *__restrict__ bad,
                                                                         u64 *__restrict__ keys, const u32 *__restrict__ list,
                                                                         const u32 *__restrict__ count)
{
    __shared__ AdapterDesc s_ads[ADAPTERS_MAX];
    __shared__ u64 wmin[ADAPTERS_THREADS / 64];
    if (*bad)
        return;
    ads_to_lds(ads, n_ads, s_ads);
    const u32 m = *count;
    for (u32 j = blockIdx.x; j < m; j += gridDim.x) {                        // (uniform in the workgroup)
        const u64 i = list[j];
        u64 first, n;
        seg_of(g, i, &first, &n);
        u64 key = ADAPTERS_NONE;
        for (u64 t0 = 0; t0 < n && key == ADAPTERS_NONE; t0 += ADAPTERS_TILE_BASES) {
            const u64 mine = adapter_lane_best([&](u64 w) { return words[w]; }, first, n, t0 + (u64)threadIdx.x * ADAPTERS_LANE_POS, s_ads,
                                               n_ads);
            const u64 wave = team_min<64>(mine);
            __syncthreads();                         // (the words of the tile before have been read)
            if ((threadIdx.x & 63) == 0)
                wmin[threadIdx.x >> 6] = wave;
            __syncthreads();
            key = wmin[0];
#pragma unroll
            for (u32 w = 1; w < ADAPTERS_THREADS / 64; w++)
                key = wmin[w] < key ? wmin[w] : key;
        }
        if (threadIdx.x == 0)
            keys[i] = key;
    }
}

// ---- the verdicts: one thread per segment (grid-stride).  out_len / out_adapter / out_mismatch (any may be null) and
// flags[i] = the segment passes; res[ADAPTERS_R_*] += the report's sums, one atomic per wave and word; the segments cut by
// each adapter are counted in LDS and added with at most n_ads atomics per workgroup.
__global__ __launch_bounds__(ADAPTERS_THREADS) void adapters_verdict_kernel(const AdapterSegs g, const u64 *__restrict__ keys,
                                                                           u64 min_bases, u32 opt_flags, u64 *__restrict__ out_len,
                                                                           u64 *__restrict__ out_adapter, u64 *__restrict__ out_mismatch,
                                                                           u32 *__restrict__ flags, unsigned long long *__restrict__ res)
{
    __shared__ u32 hist[ADAPTERS_MAX];
    if (res[ADAPTERS_R_BAD])
        return;
    if (threadIdx.x < ADAPTERS_MAX)
        hist[threadIdx.x] = 0;
    __syncthreads();
    constexpr u32 SUMS = ADAPTERS_R_ADAPTER - ADAPTERS_R_PASSED;
    u64 acc[SUMS] = {};
    for (u64 i = (u64)blockIdx.x * ADAPTERS_THREADS + threadIdx.x; i < g.n; i += (u64)gridDim.x * ADAPTERS_THREADS) {
        u64 first, n;
        seg_of(g, i, &first, &n);
        const u64 key = keys[i], kept = adapter_kept(key, n);
        const bool hit = key != ADAPTERS_NONE;
        const u32 v = adapter_verdict(key, n, min_bases, opt_flags);
        if (out_len)
            out_len[i] = kept;
        if (out_adapter)
            out_adapter[i] = hit ? adapter_key_adapter(key) : ~(u64)0;
        if (out_mismatch)
            out_mismatch[i] = hit ? adapter_key_mismatch(key) : 0;
        flags[i] = v == ADAPTERS_PASS;
        if (hit)
            atomicAdd(&hist[adapter_key_adapter(key)], 1u);
        acc[ADAPTERS_R_PASSED - ADAPTERS_R_PASSED] += v == ADAPTERS_PASS;
        acc[ADAPTERS_R_TRIMMED - ADAPTERS_R_PASSED] += hit;
        acc[ADAPTERS_R_BASES_IN - ADAPTERS_R_PASSED] += n;
        acc[ADAPTERS_R_BASES_KEPT - ADAPTERS_R_PASSED] += kept;
        acc[ADAPTERS_R_SHORT - ADAPTERS_R_PASSED] += v == ADAPTERS_FAIL_SHORT;
        acc[ADAPTERS_R_DISCARDED - ADAPTERS_R_PASSED] += v == ADAPTERS_FAIL_DISCARDED;
    }
#pragma unroll
    for (u32 k = 0; k < SUMS; k++) {
        u64 v = acc[k];
        for (u32 off = 32; off > 0; off >>= 1)
            v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v)
            atomicAdd(&res[ADAPTERS_R_PASSED + k], (unsigned long long)v);
    }
    __syncthreads();
    if (threadIdx.x < ADAPTERS_MAX && hist[threadIdx.x])
        atomicAdd(&res[ADAPTERS_R_ADAPTER + threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

// ---- the passing segments in input order: rank = the scanned flags; at most cap entries; any list may be null.  seg_seq
// (may be null: the id is i) is carried through.
__global__ __launch_bounds__(ADAPTERS_THREADS) void adapters_pass_kernel(const AdapterSegs g, const u64 *__restrict__ seg_seq,
                                                                        const u64 *__restrict__ keys, const u32 *__restrict__ flags,
                                                                        const u32 *__restrict__ rank, u64 cap,
                                                                        const unsigned long long *__restrict__ bad,
                                                                        u64 *__restrict__ pass_seq, u64 *__restrict__ pass_first,
                                                                        u64 *__restrict__ pass_len)
{
    if (*bad)
        return;
    const u64 i = (u64)blockIdx.x * ADAPTERS_THREADS + threadIdx.x;
    if (i >= g.n || !flags[i] || rank[i] >= cap)
        return;
    const u32 at = rank[i];
    u64 first, n;
    seg_of(g, i, &first, &n);
    if (pass_seq)
        pass_seq[at] = seg_seq ? seg_seq[i] : i;
    if (pass_first)
        pass_first[at] = first;
    if (pass_len)
        pass_len[at] = adapter_kept(keys[i], n);
}

hipError_t launch_adapters_find(const u64 *words, const AdapterSegs &g, const AdapterDesc *ads, u32 n_ads, const unsigned long long *bad,
                                u64 *keys, u32 *lists, u32 *counts2, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(counts2, 0, 2 * sizeof(u32), s);
    if (e != hipSuccess || g.n == 0)
        return e;
    const u64 groups_per_block = ADAPTERS_THREADS / ADAPTERS_GROUP_LANES;
    hipLaunchKernelGGL(adapters_group_kernel, dim3((unsigned)((g.n + groups_per_block - 1) / groups_per_block)), dim3(ADAPTERS_THREADS), 0,
                       s, words, g, ads, n_ads, bad, keys, lists, counts2);
    // (the longer segments: grids of a fixed size that stride over the lists, whose lengths only the device knows)
    const u64 waves = (g.n + ADAPTERS_THREADS / 64 - 1) / (ADAPTERS_THREADS / 64);
    hipLaunchKernelGGL(adapters_wave_kernel, dim3((unsigned)(waves < 1024 ? waves : 1024)), dim3(ADAPTERS_THREADS), 0, s, words, g, ads,
                       n_ads, bad, keys, lists, counts2);
    hipLaunchKernelGGL(adapters_block_kernel, dim3((unsigned)(g.n < 1024 ? g.n : 1024)), dim3(ADAPTERS_THREADS), 0, s, words, g, ads,
                       n_ads, bad, keys, lists + g.n, counts2 + 1);
    return hipGetLastError();
}

hipError_t launch_adapters_verdict(const AdapterSegs &g, const u64 *keys, u64 min_bases, u32 flags, u64 *out_len, u64 *out_adapter,
                                   u64 *out_mismatch, u32 *pass_flags, unsigned long long *res, hipStream_t s)
{
    if (g.n == 0)
        return hipSuccess;
    const u64 blocks = (g.n + ADAPTERS_THREADS - 1) / ADAPTERS_THREADS;
    hipLaunchKernelGGL(adapters_verdict_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(ADAPTERS_THREADS), 0, s, g, keys,
                       min_bases, flags, out_len, out_adapter, out_mismatch, pass_flags, res);
    return hipGetLastError();
}

hipError_t launch_adapters_pass(const AdapterSegs &g, const u64 *seg_seq, const u64 *keys, const u32 *pass_flags, const u32 *rank, u64 cap,
                                const unsigned long long *bad, u64 *pass_seq, u64 *pass_first, u64 *pass_len, hipStream_t s)
{
    if (g.n == 0 || cap == 0 || (!pass_seq && !pass_first && !pass_len))
        return hipSuccess;
    hipLaunchKernelGGL(adapters_pass_kernel, dim3((unsigned)((g.n + ADAPTERS_THREADS - 1) / ADAPTERS_THREADS)), dim3(ADAPTERS_THREADS), 0, s,
                       g, seg_seq, keys, pass_flags, rank, cap, bad, pass_seq, pass_first, pass_len);
    return hipGetLastError();
}

}  // namespace dnagpu
