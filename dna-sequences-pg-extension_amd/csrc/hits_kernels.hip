// hits_kernels.hip -- per-sequence hits of a table's k-mers in a counted set (dnagpu_table_hits):
//   SELECT d.id, count(*) FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) g JOIN counts_b b ON g.kmer = b.kmer
//   WHERE b.count BETWEEN lo AND hi GROUP BY d.id
// One sweep over the packed stream probes the accumulator's table once per row and leaves a hit BIT per stream row with
// three levels of running counts (hits_math.hpp); one thread per sequence then takes its hits as the difference of two
// prefix counts.  Sequence boundaries enter the sweep only as the bit mask of the rows that reach across one (they are not
// probed); nothing searches seq_starts per row and nothing is added to per row.
//
// The sweep is 32-rows-per-thread (filter_kernels.hip's layout), not lane-per-row.  Either way a wave-instruction of the
// probe carries 64 independent 16-byte loads; what the row-per-thread form adds is that a thread owns its mask word -- no
// ballot, no cross-lane step before the store -- and that it can put the first probes of FOUR of its rows in flight before
// it looks at any of them (the loads are unconditional for that: see the loop): 256 loads per wave between two waits
// instead of 64.
#include <hip/hip_runtime.h>

#include "acc_device.hpp"
#include "hits_math.hpp"
#include "stream_rows.hpp"
#include "strand_math.hpp"

namespace dnagpu {

namespace {

constexpr int HITS_NT = (int)HITS_TILE_WORDS;              // a sweep workgroup: one mask word per thread
constexpr int HITS_BATCH = 4;                              // rows of a thread whose first probes are in flight together
constexpr int HS_NT = 256;                                 // select: threads, sequences per thread (consecutive), per tile
constexpr int HS_PER = 8;
constexpr int HS_TILE = HS_NT * HS_PER;
static_assert(HITS_ROWS_PER_WORD % HITS_BATCH == 0, "a mask word is a whole number of batches");

// One tile of the window per workgroup: mask word blockIdx.x * HITS_TILE_WORDS + tid per thread.
template <bool CANON>
__global__ __launch_bounds__(HITS_NT) void hits_sweep_kernel(HitsWindow w, HitsSet set, u64 n_mask_words, u64 stream_rows,
                                                             u32 *__restrict__ mask, u32 *__restrict__ word_pre,
                                                             u32 *__restrict__ tile_tot)
{
    __shared__ u32 arr[HITS_NT];
    __shared__ u32 wtmp[HITS_NT / 64];
    const int tid = threadIdx.x;
    const u64 mw = (u64)blockIdx.x * HITS_TILE_WORDS + tid;
    const HitsWordAt at = hits_word_at(w.a0, mw);

    // the rows of this word that are rows of one sequence, and the 64 bases that start at the first of them
    u32 todo = mw < n_mask_words ? hits_word_valid(stream_rows, mw) : 0u;
    u64 lo = 0, hi = 0;
    if (todo) {
        const Stream4 s = stream_of(words_load(w.words, w.n_words, at.stream_word, at.fo * 2), at.fo * 2);
        lo = ((u64)s.d[1] << 32) | s.d[0];
        hi = ((u64)s.d[3] << 32) | s.d[2];
        todo &= ~spoiled_rows(marks_load(w.marks, w.n_mark_words, at.stream_word, at.fo), at.fo, (u32)w.k - 1u);
    }

    const u64 kmask = kmer_mask(w.k);
    const int pshift = 64 - set.pbits;                     // (pbits >= 1: a set without a table is never swept)
    u32 hit = 0;
#pragma unroll 1
    for (int j0 = 0; j0 < (int)HITS_ROWS_PER_WORD; j0 += HITS_BATCH) {
        if (((todo >> j0) & ((1u << HITS_BATCH) - 1u)) == 0)
            continue;
        u64 key[HITS_BATCH], fk[HITS_BATCH], fc[HITS_BATCH];
        const u64 *region[HITS_BATCH];
        u32 sl[HITS_BATCH];
        bool live[HITS_BATCH];
        // Keys and hashes of all four, then two rounds of UNCONDITIONAL loads, so that each round is four loads behind one
        // wait: the occ words (every key has a partition, also a row that is not probed), then the home slots.  A row that
        // is not probed, or whose partition holds nothing -- such a partition is never read -- loads set.idle instead, 16
        // defined bytes, and its result is dropped.
        u32 oc[HITS_BATCH];
#pragma unroll
        for (int i = 0; i < HITS_BATCH; i++) {
            key[i] = funnel(lo, hi, 2u * (unsigned)(j0 + i)) & kmask;
            if (CANON)
                key[i] = kmer_canonical(key[i], w.k);
            const u64 h = splitmix64(key[i]);
            const u64 pt = h >> pshift;
            region[i] = set.table + 2 * pt * ACC_SLOTS;
            sl[i] = acc_home(h);
            oc[i] = set.occ[pt];
        }
        const u64 *addr[HITS_BATCH];
#pragma unroll
        for (int i = 0; i < HITS_BATCH; i++) {
            live[i] = ((todo >> (j0 + i)) & 1u) != 0 && oc[i] != 0;
            addr[i] = live[i] ? region[i] + 2 * (u64)sl[i] : set.idle;
        }
#pragma unroll
        for (int i = 0; i < HITS_BATCH; i++)
            ld_slot(addr[i], fk[i], fc[i]);
        // each row's linear probe (join_direct_kernel's) goes on from its home slot: stop at an empty slot
#pragma unroll
        for (int i = 0; i < HITS_BATCH; i++) {
            if (!live[i])
                continue;
            u64 k2 = fk[i], c = fc[i];
            for (int probe = 1; c != 0; probe++) {
                if (k2 == key[i]) {
                    if (c >= set.lo && c <= set.hi)
                        hit |= 1u << (j0 + i);
                    break;
                }
                if (probe >= ACC_SLOTS)
                    break;
                sl[i] = (sl[i] + 1) & (ACC_SLOTS - 1);
                ld_slot(region[i] + 2 * (u64)sl[i], k2, c);
            }
        }
    }

    const u32 total = block_scan_value<HITS_NT>((u32)__popc(hit), arr, HITS_NT, wtmp, tid);
    if (mw < n_mask_words) {
        mask[mw] = hit;
        word_pre[mw] = arr[tid];
    }
    if (tid == 0)
        tile_tot[blockIdx.x] = total;
}

__global__ void hits_bounds_kernel(const u64 *__restrict__ seq_starts, u64 seq_first, u64 seq_count, u64 *__restrict__ out2)
{
    if (threadIdx.x < 2)
        out2[threadIdx.x] = seq_starts[seq_first + (threadIdx.x ? seq_count : 0)];
}

// sum of v over the workgroup into *dst (one atomic, none for a zero); part: HS_NT / 64 words nothing else uses meanwhile
__device__ __forceinline__ void block_add_u64(u64 v, u64 *part, unsigned long long *dst)
{
    for (int off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0)
        part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 s = 0;
        for (int wv = 0; wv < HS_NT / 64; wv++)
            s += part[wv];
        if (s)
            atomicAdd(dst, (unsigned long long)s);
    }
    __syncthreads();
}

// One thread per sequence of the window (starts = seq_starts + seq_first).  mask == nullptr: nothing was swept, no hits.
__global__ __launch_bounds__(HS_NT) void hits_gather_kernel(const u64 *__restrict__ starts, u64 seq_count, u64 a0, int k,
                                                            const u32 *__restrict__ mask, const u32 *__restrict__ word_pre,
                                                            const u32 *__restrict__ tile_base, u32 *__restrict__ out_rows,
                                                            u32 *__restrict__ out_hits, unsigned long long *totals3)
{
    __shared__ u64 part[HS_NT / 64];
    u64 t_rows = 0, t_hits = 0, t_seqs = 0;
    for (u64 i = (u64)blockIdx.x * HS_NT + threadIdx.x; i < seq_count; i += (u64)gridDim.x * HS_NT) {
        const u64 s0 = starts[i], s1 = starts[i + 1];
        const u64 rows = hits_seq_rows(s1 - s0, k);
        u32 h = 0;
        if (rows && mask) {
            const u64 r0 = s0 - a0;
            h = hits_before(mask, word_pre, tile_base, r0 + rows) - hits_before(mask, word_pre, tile_base, r0);
        }
        out_rows[i] = (u32)rows;
        out_hits[i] = h;
        t_rows += rows;
        t_hits += h;
        t_seqs += h != 0;
    }
    block_add_u64(t_rows, part, totals3);
    block_add_u64(t_hits, part, totals3 + 1);
    block_add_u64(t_seqs, part, totals3 + 2);
}

// bit j = sequence tile * HS_TILE + tid * HS_PER + j exists and passes
__device__ __forceinline__ u32 select_bits(const u32 *__restrict__ rows, const u32 *__restrict__ hits, u64 n, const HitsPredicate &p,
                                           u64 base)
{
    u32 bits = 0;
#pragma unroll
    for (int j = 0; j < HS_PER; j++) {
        const u64 i = base + j;
        if (i < n && hits_selected(rows[i], hits[i], p.min_hits, p.max_hits, p.frac_num, p.frac_den))
            bits |= 1u << j;
    }
    return bits;
}

__global__ __launch_bounds__(HS_NT) void hits_select_count_kernel(const u32 *__restrict__ rows, const u32 *__restrict__ hits, u64 n,
                                                                  HitsPredicate p, u32 *__restrict__ tile_counts)
{
    __shared__ u32 wsum[HS_NT / 64];
    const u64 base = (u64)blockIdx.x * HS_TILE + (u64)threadIdx.x * HS_PER;
    const u32 c = wave_sum((u32)__popc(select_bits(rows, hits, n, p, base)));
    if ((threadIdx.x & 63) == 0)
        wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 g = 0;
        for (int wv = 0; wv < HS_NT / 64; wv++)
            g += wsum[wv];
        tile_counts[blockIdx.x] = g;
    }
}

// the matches of a tile go out in sequence order behind those of the tiles before it (tile_offsets: the scanned counts)
__global__ __launch_bounds__(HS_NT) void hits_select_write_kernel(const u32 *__restrict__ rows, const u32 *__restrict__ hits, u64 n,
                                                                  HitsPredicate p, const u32 *__restrict__ tile_offsets,
                                                                  u64 seq_first, u64 *__restrict__ out_seq,
                                                                  u64 *__restrict__ out_rows, u64 *__restrict__ out_hits, u64 cap)
{
    __shared__ u32 arr[HS_NT];
    __shared__ u32 wtmp[HS_NT / 64];
    const int tid = threadIdx.x;
    const u64 base = (u64)blockIdx.x * HS_TILE + (u64)tid * HS_PER;
    const u32 bits = select_bits(rows, hits, n, p, base);
    block_scan_value<HS_NT>((u32)__popc(bits), arr, HS_NT, wtmp, tid);
    u64 at = (u64)tile_offsets[blockIdx.x] + arr[tid];
#pragma unroll
    for (int j = 0; j < HS_PER; j++) {
        if (!(bits & (1u << j)))
            continue;
        if (at < cap) {
            const u64 i = base + j;
            if (out_seq)
                out_seq[at] = seq_first + i;
            if (out_rows)
                out_rows[at] = rows[i];
            if (out_hits)
                out_hits[at] = hits[i];
        }
        at++;
    }
}

__global__ __launch_bounds__(HS_NT) void hits_widen_kernel(const u32 *__restrict__ in, u64 *__restrict__ out, u64 n)
{
    for (u64 i = (u64)blockIdx.x * HS_NT + threadIdx.x; i < n; i += (u64)gridDim.x * HS_NT)
        out[i] = in[i];
}

unsigned stride_grid(u64 n)
{
    const u64 g = (n + HS_NT - 1) / HS_NT;
    return (unsigned)(g < 65536 ? g : 65536);
}

}  // namespace

hipError_t launch_hits_sweep(const HitsWindow &w, const HitsSet &set, u32 *mask, u32 *word_pre, u32 *tile_tot, hipStream_t s)
{
    if (!set.table || !set.occ || !set.idle || set.pbits < 1 || set.pbits > 63 || w.k < 1 || w.k > 32 || w.n > 0xFFFFFFFFull)
        return hipErrorInvalidValue;
    const u64 n_mw = hits_mask_words(w.n), tiles = hits_tiles(w.n), rows = hits_stream_rows(w.n, w.k);
    if (w.canonical)
        hipLaunchKernelGGL(hits_sweep_kernel<true>, dim3((unsigned)tiles), dim3(HITS_NT), 0, s, w, set, n_mw, rows, mask, word_pre,
                           tile_tot);
    else
        hipLaunchKernelGGL(hits_sweep_kernel<false>, dim3((unsigned)tiles), dim3(HITS_NT), 0, s, w, set, n_mw, rows, mask, word_pre,
                           tile_tot);
    return hipGetLastError();
}

hipError_t launch_hits_bounds(const u64 *seq_starts, u64 seq_first, u64 seq_count, u64 *out2, hipStream_t s)
{
    hipLaunchKernelGGL(hits_bounds_kernel, dim3(1), dim3(64), 0, s, seq_starts, seq_first, seq_count, out2);
    return hipGetLastError();
}

hipError_t launch_hits_gather(const u64 *starts, u64 seq_count, u64 a0, int k, const u32 *mask, const u32 *word_pre,
                              const u32 *tile_base, u32 *out_rows, u32 *out_hits, unsigned long long *totals3, hipStream_t s)
{
    if (seq_count == 0)
        return hipSuccess;
    hipLaunchKernelGGL(hits_gather_kernel, dim3(stride_grid(seq_count)), dim3(HS_NT), 0, s, starts, seq_count, a0, k, mask, word_pre,
                       tile_base, out_rows, out_hits, totals3);
    return hipGetLastError();
}

u32 hits_select_tiles(u64 n)
{
    return (u32)((n + HS_TILE - 1) / HS_TILE);
}

hipError_t launch_hits_select_count(const u32 *rows, const u32 *hits, u64 n, const HitsPredicate &p, u32 *tile_counts, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(hits_select_count_kernel, dim3(hits_select_tiles(n)), dim3(HS_NT), 0, s, rows, hits, n, p, tile_counts);
    return hipGetLastError();
}

hipError_t launch_hits_select_write(const u32 *rows, const u32 *hits, u64 n, const HitsPredicate &p, const u32 *tile_offsets,
                                    u64 seq_first, u64 *out_seq, u64 *out_rows, u64 *out_hits, u64 cap, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(hits_select_write_kernel, dim3(hits_select_tiles(n)), dim3(HS_NT), 0, s, rows, hits, n, p, tile_offsets,
                       seq_first, out_seq, out_rows, out_hits, cap);
    return hipGetLastError();
}

hipError_t launch_hits_widen(const u32 *in, u64 *out, u64 n, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(hits_widen_kernel, dim3(stride_grid(n)), dim3(HS_NT), 0, s, in, out, n);
    return hipGetLastError();
}

}  // namespace dnagpu
