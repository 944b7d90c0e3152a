// names_kernels.hip -- the kernels of the names column (dnagpu_names_*): the sweep over a text that marks the
// bytes which end a name, the suffix minimum over its tiles, the span of every sequence's name, the check of a caller's
// offsets, and the validation of a column's bytes.  The bytes themselves are moved by quals_copy_kernel (quals_kernels.hip),
// the named image is formed by export_read_named_kernel (export_kernels.hip).  The arithmetic is names_math.hpp's; the chunk
// load and the error minimum are text_device.hpp's.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "names_math.hpp"
#include "take_math.hpp"
#include "text_device.hpp"

namespace dnagpu {

// the minimum of v over the workgroup's threads, in every thread; wmin: one word of LDS per wave.  Synchronises.
__device__ __forceinline__ u32 names_block_min(u32 v, u32 *wmin)
{
#pragma unroll
    for (u32 off = 32; off > 0; off >>= 1) {
        const u32 o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    if ((threadIdx.x & 63) == 0)
        wmin[threadIdx.x >> 6] = v;
    __syncthreads();
    u32 r = wmin[0];
#pragma unroll
    for (u32 w = 1; w < NAMES_THREADS / 64; w++)
        r = wmin[w] < r ? wmin[w] : r;
    __syncthreads();
    return r;
}

// the minimum of v over this thread and the threads behind it in the workgroup (NAMES_THREADS entries of LDS).  Synchronises.
__device__ __forceinline__ u32 names_block_suffix_min(u32 v, u32 *arr)
{
    const u32 tid = threadIdx.x;
    arr[tid] = v;
    __syncthreads();
#pragma unroll
    for (u32 off = 1; off < NAMES_THREADS; off <<= 1) {
        const u32 o = tid + off < NAMES_THREADS ? arr[tid + off] : NAMES_NONE;
        __syncthreads();
        v = o < v ? o : v;
        arr[tid] = v;
        __syncthreads();
    }
    return v;
}

// ---- the sweep: TEXT_CHUNK bytes per lane, TEXT_TILE_BYTES per workgroup (the loaders' shape).  mask has names_chunks(n)
// words, each written once; tile_first one word per tile.
static_assert(NAMES_THREADS == TEXT_THREADS, "the sweep's reductions are sized for the loaders' workgroup");
__global__ __launch_bounds__(TEXT_THREADS) void names_ends_kernel(const unsigned char *__restrict__ text, u64 n, bool first_word,
                                                                  u32 *__restrict__ mask, u32 *__restrict__ tile_first,
                                                                  unsigned long long *__restrict__ res)
{
    __shared__ u32 wmin[TEXT_THREADS / 64];
    const u32 tid = threadIdx.x, tile = blockIdx.x;
    const u64 b = (u64)tile * TEXT_TILE_BYTES + (u64)tid * TEXT_CHUNK;
    u32 first = NAMES_NONE;
    bool lone = false;
    if (b < n) {
        u32 w[8];
        const u32 valid = text_low_bits(text_load_words(text, n, b, w));
        u32 ends = 0, nl = 0, cr = 0;
#pragma unroll
        for (u32 j = 0; j < TEXT_CHUNK; j++) {
            const u32 byte = (w[j >> 2] >> (8 * (j & 3))) & 0xff;
            ends |= (u32)names_ends_here(byte, first_word) << j;
            nl |= (u32)(byte == '\n') << j;
            cr |= (u32)(byte == '\r') << j;
        }
        ends &= valid;
        const bool next_nl = n - b > TEXT_CHUNK && text[b + TEXT_CHUNK] == '\n';
        lone = (cr & valid & ~((nl >> 1) | ((u32)next_nl << 31))) != 0;
        mask[b / TEXT_CHUNK] = ends;
        if (ends)
            first = (u32)(b + (u32)__builtin_ctz(ends));
    }
    first = names_block_min(first, wmin);
    if (tid == 0)
        tile_first[tile] = first;
    if (__syncthreads_or(lone) && tid == 0)
        atomicOr(&res[NAMES_R_LONE_CR], 1ull);
}

// ---- the suffix minimum, first inside groups of NAMES_GROUP_TILES tiles
__global__ __launch_bounds__(NAMES_THREADS) void names_suffix_local_kernel(const u32 *__restrict__ tile_first, u32 n_tiles,
                                                                           u32 *__restrict__ local, u32 *__restrict__ group_min)
{
    __shared__ u32 arr[NAMES_THREADS];
    const u64 t = (u64)blockIdx.x * NAMES_GROUP_TILES + threadIdx.x;
    const u32 v = names_block_suffix_min(t < n_tiles ? tile_first[t] : NAMES_NONE, arr);
    if (t < n_tiles)
        local[t] = v;
    if (threadIdx.x == 0)
        group_min[blockIdx.x] = v;
}

// ---- then over the groups, by one workgroup from the last batch of groups to the first: after[g] = the minimum of the
// groups behind g
__global__ __launch_bounds__(NAMES_THREADS) void names_suffix_groups_kernel(const u32 *__restrict__ group_min, u32 n_groups,
                                                                            u32 *__restrict__ after)
{
    __shared__ u32 arr[NAMES_THREADS];
    u32 carry = NAMES_NONE;                          // the minimum of the batches behind this one
    const u32 batches = (n_groups + NAMES_THREADS - 1) / NAMES_THREADS;
    for (u32 bt = batches; bt-- > 0;) {              // uniform
        const u32 g = bt * NAMES_THREADS + threadIdx.x;
        names_block_suffix_min(g < n_groups ? group_min[g] : NAMES_NONE, arr);
        const u32 behind = threadIdx.x + 1 < NAMES_THREADS ? arr[threadIdx.x + 1] : NAMES_NONE;
        const u32 whole = arr[0];
        if (g < n_groups)
            after[g] = behind < carry ? behind : carry;
        carry = whole < carry ? whole : carry;
        __syncthreads();                             // (arr is written again by the next batch)
    }
}

// ---- one thread per sequence
__global__ __launch_bounds__(NAMES_THREADS) void names_spans_kernel(const NamesSpans A)
{
    __shared__ u64 wsum[NAMES_THREADS / 64];
    const u64 s = (u64)blockIdx.x * NAMES_THREADS + threadIdx.x;
    u64 len = 0;
    int bad = 0;
    if (s < A.n_seqs) {
        const u64 r = A.src_record ? A.src_record[s] : s;
        u64 start = 0;
        if (r < A.n_records) {
            const u64 p = A.record_pos[r];
            if (p < A.n && A.text[p] == A.marker) {
                start = p + 1;
                const u64 e = names_end_from(
                    start, A.n, [&](u64 c) { return A.mask[c]; }, [&](u64 t) { return A.local[t]; },
                    [&](u64 g) { return A.after[g]; });
                len = names_strip(start, e, A.n, [&](u64 i) { return (u32)A.text[i]; }) - start;
            } else {
                bad = 1;
            }
        } else {
            bad = 1;
        }
        A.first[s] = start;
        A.len32[s] = (u32)len;                       // (below the text's bytes)
    }
    u64 sum = len;
    for (int off = 32; off > 0; off >>= 1)
        sum += __shfl_down(sum, off);
    if ((threadIdx.x & 63) == 0)
        wsum[threadIdx.x >> 6] = sum;
    const int any_bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        u64 total = 0;
#pragma unroll
        for (u32 w = 0; w < NAMES_THREADS / 64; w++)
            total += wsum[w];
        if (total)
            atomicAdd(&A.res[NAMES_R_TOTAL], (unsigned long long)total);
        if (any_bad)
            atomicOr(&A.res[NAMES_R_BAD], 1ull);
    }
}

// ---- a caller's offsets: one thread per entry
__global__ __launch_bounds__(NAMES_THREADS) void names_offsets_check_kernel(const u64 *__restrict__ off, u64 n,
                                                                            unsigned long long *__restrict__ res)
{
    const u64 i = (u64)blockIdx.x * NAMES_THREADS + threadIdx.x;
    int bad = 0;
    if (i < n)
        bad = off[i] > off[i + 1];
    if (i == 0)
        bad |= off[0] != 0;
    if (i == n)
        res[NAMES_R_TOTAL] = off[n];
    if (__syncthreads_or(bad) && threadIdx.x == 0)
        atomicOr(&res[NAMES_R_BAD], 1ull);
}

// ---- a column's bytes: one lane per 16-byte chunk (quals_validate_kernel's pattern: one 64-bit minimum of error words;
// the word is the offset itself).  Nothing is written.
__global__ __launch_bounds__(NAMES_THREADS) void names_validate_kernel(const unsigned char *__restrict__ col, u64 total,
                                                                       unsigned long long *__restrict__ res)
{
    const u64 c = (u64)blockIdx.x * NAMES_THREADS + threadIdx.x, p = c * QUALS_CHUNK;
    u64 err = NAMES_NO_ERROR;
    if (p < total) {
        const uint4 w = *reinterpret_cast<const uint4 *>(col + p);
        QualsBytes v;
        v.lo = (u64)w.x | ((u64)w.y << 32);
        v.hi = (u64)w.z | ((u64)w.w << 32);
        const u32 have = total - p < QUALS_CHUNK ? (u32)(total - p) : QUALS_CHUNK;
        for (u32 k = have; k-- > 0;)
            if (names_forbidden(quals_get(v, k)))
                err = p + k;
    }
    text_error_min(err, res);
}

// ---- where an invalid byte of a column made from a text lies in that text: one thread
__global__ void names_locate_kernel(const u64 *__restrict__ off, u64 n, u64 pos, const u64 *__restrict__ first,
                                    const u64 *__restrict__ src_record, u64 *__restrict__ out3)
{
    const u64 s = take_segment_of(off, 0, n - 1, pos);
    out3[0] = s;
    out3[1] = first[s] + (pos - off[s]);
    out3[2] = src_record ? src_record[s] : s;
}

hipError_t launch_names_ends(const unsigned char *text, u64 n, u32 n_tiles, bool first_word, u32 *mask, u32 *tile_first,
                             unsigned long long *res, hipStream_t s)
{
    hipLaunchKernelGGL(names_ends_kernel, dim3(n_tiles), dim3(TEXT_THREADS), 0, s, text, n, first_word, mask, tile_first, res);
    return hipGetLastError();
}

hipError_t launch_names_suffix_min(const u32 *tile_first, u32 n_tiles, u32 *local, u32 *group_min, u32 *after, hipStream_t s)
{
    const u32 groups = (u32)names_groups(n_tiles);
    hipLaunchKernelGGL(names_suffix_local_kernel, dim3(groups), dim3(NAMES_THREADS), 0, s, tile_first, n_tiles, local, group_min);
    hipLaunchKernelGGL(names_suffix_groups_kernel, dim3(1), dim3(NAMES_THREADS), 0, s, group_min, groups, after);
    return hipGetLastError();
}

hipError_t launch_names_spans(const NamesSpans &a, hipStream_t s)
{
    if (a.n_seqs == 0)
        return hipSuccess;
    hipLaunchKernelGGL(names_spans_kernel, dim3((unsigned)((a.n_seqs + NAMES_THREADS - 1) / NAMES_THREADS)), dim3(NAMES_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_names_offsets_check(const u64 *off, u64 n, unsigned long long *res, hipStream_t s)
{
    hipLaunchKernelGGL(names_offsets_check_kernel, dim3((unsigned)((n + 1 + NAMES_THREADS - 1) / NAMES_THREADS)), dim3(NAMES_THREADS), 0,
                       s, off, n, res);
    return hipGetLastError();
}

hipError_t launch_names_validate(const unsigned char *col, u64 total, unsigned long long *res, hipStream_t s)
{
    if (total == 0)
        return hipSuccess;
    const u64 blocks = (quals_chunks(total) + NAMES_THREADS - 1) / NAMES_THREADS;
    hipLaunchKernelGGL(names_validate_kernel, dim3((unsigned)blocks), dim3(NAMES_THREADS), 0, s, col, total, res);
    return hipGetLastError();
}

hipError_t launch_names_locate(const u64 *off, u64 n, u64 pos, const u64 *first, const u64 *src_record, u64 *out3, hipStream_t s)
{
    hipLaunchKernelGGL(names_locate_kernel, dim3(1), dim3(1), 0, s, off, n, pos, first, src_record, out3);
    return hipGetLastError();
}

}  // namespace dnagpu
