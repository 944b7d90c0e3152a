// take_kernels.hip -- the bit-granular gather of segments of a packed stream into a new packed stream (dnagpu_dna_gather,
// dnagpu_dna_take): the pass that builds and validates the segment list, the widening of the scanned lengths
// into the result's starts, and the output-centric sweep.  The piece arithmetic is take_math.hpp's.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "take_math.hpp"

namespace dnagpu {

// ---- the segment list.  One thread per entry (grid-stride).  ids != nullptr (take): entry i is sequence ids[i] of the table
// -- seg_first[i] = seq_starts[id], its length the difference to the next start; an id >= n_seqs is an error.  Else
// (gather): entry i is (in_first[i], in_len[i]) as the caller gave them; one that leaves [0, n_bases] is an error and
// seg_first is not written (the sweep reads in_first itself).  len32[i] = the length (what the scan takes: it is only run
// once the total is known to fit 32 bits); res[0] += the lengths (take_len_clamped), res[1] |= 1 on any error: a block
// reduce, then one atomic per workgroup and word.  An entry in error counts as empty.
__global__ __launch_bounds__(TAKE_THREADS) void take_segments_kernel(const u64 *__restrict__ ids, const u64 *__restrict__ seq_starts,
                                                                     u64 n_seqs, const u64 *__restrict__ in_first,
                                                                     const u64 *__restrict__ in_len, u64 n_bases, u64 n,
                                                                     u64 *__restrict__ seg_first, u32 *__restrict__ len32,
                                                                     unsigned long long *__restrict__ res)
{
    __shared__ u64 wsum[TAKE_THREADS / 64];
    u64 sum = 0;
    int bad = 0;
    for (u64 i = (u64)blockIdx.x * TAKE_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * TAKE_THREADS) {
        u64 len = 0;
        if (ids) {
            const u64 id = ids[i];
            u64 a = 0;
            if (id < n_seqs) {
                a = seq_starts[id];
                len = seq_starts[id + 1] - a;
            } else {
                bad = 1;
            }
            seg_first[i] = a;
        } else {
            const u64 a = in_first[i], l = in_len[i];
            if (a <= n_bases && l <= n_bases - a)
                len = l;
            else
                bad = 1;
        }
        len32[i] = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)len;
        sum += take_len_clamped(len);
    }
    for (int off = 32; off > 0; off >>= 1)
        sum += __shfl_down(sum, off);
    if ((threadIdx.x & 63) == 0)
        wsum[threadIdx.x >> 6] = sum;
    const int any_bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        u64 total = 0;
#pragma unroll
        for (u32 w = 0; w < TAKE_THREADS / 64; w++)
            total += wsum[w];
        if (total)
            atomicAdd(&res[0], (unsigned long long)total);
        if (any_bad)
            atomicOr(&res[1], 1ull);
    }
}

// out_starts[i] = scan[i] (the exclusive scan of the lengths) for i < n, out_starts[n] = total
__global__ __launch_bounds__(TAKE_THREADS) void take_starts_kernel(const u32 *__restrict__ scan, u64 n, u64 total,
                                                                   u64 *__restrict__ out_starts)
{
    const u64 i = (u64)blockIdx.x * TAKE_THREADS + threadIdx.x;
    if (i < n)
        out_starts[i] = scan[i];
    else if (i == n)
        out_starts[i] = total;
}

// Index of the first entry of a[lo .. hi) that is > p (hi when there is none), a ascending; by the whole workgroup, every
// thread gets the answer (the 256-ary search of filter_kernels.hip's block_upper_bound: every round the threads test the
// last entries of 256 equal chunks and the answer's chunk becomes the range).  wc: one word of LDS per wave.
__device__ __forceinline__ u64 take_block_upper_bound(const u64 *__restrict__ a, u64 lo, u64 hi, u64 p, u32 *wc)
{
    const u32 tid = threadIdx.x;
    while (hi > lo) {                                // uniform
        const u64 step = (hi - lo + TAKE_THREADS - 1) / TAKE_THREADS;
        const u64 c0 = lo + (u64)tid * step;
        bool le = false;
        if (c0 < hi) {
            const u64 c1 = c0 + step < hi ? c0 + step : hi;
            le = a[c1 - 1] <= p;
        }
        const u32 wcnt = (u32)__popcll(__ballot(le));
        if ((tid & 63) == 0)
            wc[tid >> 6] = wcnt;
        __syncthreads();
        u32 cnt = 0;
#pragma unroll
        for (u32 w = 0; w < TAKE_THREADS / 64; w++)
            cnt += wc[w];
        __syncthreads();
        // chunks [0, cnt) lie at or below p; chunk cnt, if it has entries, ends above p
        u64 nlo = lo + (u64)cnt * step;
        if (nlo > hi)
            nlo = hi;
        u64 nhi = nlo + step < hi ? nlo + step : hi;
        if (nhi > nlo)
            nhi--;
        lo = nlo;
        hi = nhi;
    }
    return lo;
}

// The words of one tile: thread t forms words t, t + 256, .. of the tile; the segment of every word's first base lies in
// [lo, hi] of the three lists (global memory, or the tile's part of them in LDS).  The searches first, all of them, so that
// their loads overlap; then the words.
__device__ __forceinline__ void take_tile_words(const u64 *starts, const u64 *first, const uint8_t *flip, u64 lo, u64 hi,
                                                const u64 *__restrict__ src, u64 total, u64 w_tile, u64 n_out_words,
                                                u64 *__restrict__ out)
{
    const u32 tid = threadIdx.x;
    u64 seg[TAKE_WORDS_PER_THREAD];
#pragma unroll
    for (u32 j = 0; j < TAKE_WORDS_PER_THREAD; j++) {
        const u64 w = w_tile + j * TAKE_THREADS + tid;
        seg[j] = w < n_out_words ? take_segment_of(starts, lo, hi, 32 * w) : lo;
    }
#pragma unroll
    for (u32 j = 0; j < TAKE_WORDS_PER_THREAD; j++) {
        const u64 w = w_tile + j * TAKE_THREADS + tid;
        if (w < n_out_words)
            out[w] = take_word(starts, first, flip, total, seg[j], w, [&](u64 i) { return src[i]; });
    }
}

// ---- the sweep.  A workgroup owns the TAKE_TILE_WORDS output words from word blockIdx.x * TAKE_TILE_WORDS on; thread t forms
// words t, t + 256, .. of the tile in registers and stores each once, whole (consecutive lanes, consecutive words).  The
// workgroup finds the segments of its tile's first and last base once -- the first by a block search over out_starts, the
// last among the 256 starts that follow (another block search only when all of them lie inside the tile: segments shorter
// than 128 bases on average) -- and every thread searches for the segment of its word's first base between the two; the
// pieces of the word follow from there (take_word).  A tile of at most TAKE_LDS_SEGS segments (segments of 32 bases or more
// on average) first brings their starts, source bases and flags into LDS, and searches and walks there; a tile of more
// reads them where they are.  No word of src is read that holds no base of a piece; total > 0.
__global__ __launch_bounds__(TAKE_THREADS) void take_copy_kernel(const u64 *__restrict__ src, const u64 *__restrict__ seg_first,
                                                                 const uint8_t *__restrict__ seg_flip,
                                                                 const u64 *__restrict__ out_starts, u64 n, u64 total,
                                                                 u64 n_out_words, u64 *__restrict__ out)
{
    __shared__ u32 wc[TAKE_THREADS / 64], wle[TAKE_THREADS / 64];
    __shared__ u64 s_starts[TAKE_LDS_SEGS + 1], s_first[TAKE_LDS_SEGS];
    __shared__ uint8_t s_flip[TAKE_LDS_SEGS];
    const u32 tid = threadIdx.x;
    const u64 w_tile = (u64)blockIdx.x * TAKE_TILE_WORDS;
    const u64 p_first = 32 * w_tile;
    const u64 tile_end = 32 * (w_tile + TAKE_TILE_WORDS);
    const u64 p_last = (tile_end < total ? tile_end : total) - 1;
    // out_starts[0 .. ub_lo) lie at or below the tile's first base: entry 0 is 0, entry n = total is above every base
    const u64 ub_lo = take_block_upper_bound(out_starts, 1, n, p_first, wc);
    const u64 sv = ub_lo + tid < n ? out_starts[ub_lo + tid] : ~(u64)0;
    const u32 nle = (u32)__popcll(__ballot(sv <= p_last));
    if ((tid & 63) == 0)
        wle[tid >> 6] = nle;
    __syncthreads();
    u32 n_le = 0;
#pragma unroll
    for (u32 w = 0; w < TAKE_THREADS / 64; w++)
        n_le += wle[w];
    u64 ub_hi = ub_lo + n_le;
    if (n_le == TAKE_THREADS && ub_hi < n)           // uniform
        ub_hi = take_block_upper_bound(out_starts, ub_hi, n, p_last, wc);
    const u64 seg_lo = ub_lo - 1, seg_hi = ub_hi - 1;

    const u64 m = seg_hi - seg_lo + 1;               // the tile's segments: seg_lo .. seg_hi
    if (m <= TAKE_LDS_SEGS) {                        // uniform
        for (u32 i = tid; i <= (u32)m; i += TAKE_THREADS)
            s_starts[i] = out_starts[seg_lo + i];
        for (u32 i = tid; i < (u32)m; i += TAKE_THREADS) {
            s_first[i] = seg_first[seg_lo + i];
            s_flip[i] = seg_flip ? seg_flip[seg_lo + i] : (uint8_t)0;
        }
        __syncthreads();
        take_tile_words(s_starts, s_first, s_flip, (u64)0, m - 1, src, total, w_tile, n_out_words, out);
    } else {
        take_tile_words(out_starts, seg_first, seg_flip, seg_lo, seg_hi, src, total, w_tile, n_out_words, out);
    }
}

hipError_t launch_take_segments(const u64 *ids, const u64 *seq_starts, u64 n_seqs, const u64 *in_first, const u64 *in_len,
                                u64 n_bases, u64 n, u64 *seg_first, u32 *len32, unsigned long long *res2, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(res2, 0, 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess || n == 0)
        return e;
    const u64 blocks = (n + TAKE_THREADS - 1) / TAKE_THREADS;
    hipLaunchKernelGGL(take_segments_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(TAKE_THREADS), 0, s, ids,
                       seq_starts, n_seqs, in_first, in_len, n_bases, n, seg_first, len32, res2);
    return hipGetLastError();
}

hipError_t launch_take_starts(const u32 *scan, u64 n, u64 total, u64 *out_starts, hipStream_t s)
{
    hipLaunchKernelGGL(take_starts_kernel, dim3((unsigned)((n + 1 + TAKE_THREADS - 1) / TAKE_THREADS)), dim3(TAKE_THREADS), 0, s, scan,
                       n, total, out_starts);
    return hipGetLastError();
}

hipError_t launch_take_copy(const u64 *src, const u64 *seg_first, const uint8_t *seg_flip, const u64 *out_starts, u64 n, u64 total,
                            u64 *out, hipStream_t s)
{
    const u64 n_out_words = take_words(total);
    if (n_out_words == 0)
        return hipSuccess;
    hipLaunchKernelGGL(take_copy_kernel, dim3((unsigned)take_tiles(n_out_words)), dim3(TAKE_THREADS), 0, s, src, seg_first, seg_flip,
                       out_starts, n, total, n_out_words, out);
    return hipGetLastError();
}

}  // namespace dnagpu
