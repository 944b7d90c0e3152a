// index_kernels.hip -- the index over a stored kmer column (test.sql:156-270): a stable LSD radix sort of
// (r, row) pairs by 8-bit digits, the range-pruned scan behind `=`, `^@` and `@>`, the batch lookup and the window read, and
// the two updates: the merge-path merge of an appended batch and the bitmap + compaction of a delete.
// No workgroup ever waits for another inside a launch: every pass is histogram -> scan -> scatter, three launches.
#include <algorithm>

#include "index_math.hpp"
#include "kernels.hpp"

namespace dnagpu {

namespace {

constexpr int IX_THREADS = 256;
constexpr int IX_WAVES = IX_THREADS / 64;
constexpr int IX_ITEMS = INDEX_SORT_TILE / IX_THREADS;       // items per thread of a sort tile
constexpr int IX_DIGITS = 256;
static_assert(IX_ITEMS * IX_THREADS == INDEX_SORT_TILE, "a tile is a whole number of items per thread");
static_assert(IX_DIGITS == IX_THREADS, "one thread per digit scans the waves' counts");

__device__ __forceinline__ void ix_load(const IndexSortSrc &s, u64 idx, u64 *r, u32 *row)
{
    if (s.keys) {               // the first pass that moves anything: the caller's keys, row = row_base + position
        *r = index_r_of_key(s.keys[idx], s.k);
        *row = s.row_base + (u32)idx;
    } else {
        *r = s.r[idx];
        *row = s.row[idx];
    }
}
__device__ __forceinline__ u64 ix_load_r(const IndexSortSrc &s, u64 idx)
{
    return s.keys ? index_r_of_key(s.keys[idx], s.k) : s.r[idx];
}

// hist[d * n_tiles + tile] = the keys of the tile whose digit is d
__global__ __launch_bounds__(IX_THREADS) void index_hist_kernel(IndexSortSrc s, u64 n, int shift, u32 n_tiles, u32 *__restrict__ hist)
{
    __shared__ u32 bins[IX_DIGITS];
    const int tid = threadIdx.x;
    bins[tid] = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * INDEX_SORT_TILE;
#pragma unroll
    for (int i = 0; i < IX_ITEMS; i++) {
        const u64 idx = base + (u64)i * IX_THREADS + tid;
        if (idx < n)
            atomicAdd(&bins[(u32)(ix_load_r(s, idx) >> shift) & (IX_DIGITS - 1)], 1u);
    }
    __syncthreads();
    hist[(u64)tid * n_tiles + blockIdx.x] = bins[tid];
}

// *nonempty = the digits that occur at all, from the scanned matrix (digit d starts at off[d * n_tiles])
__global__ __launch_bounds__(IX_DIGITS) void index_digit_bins_kernel(const u32 *__restrict__ off, u32 n_tiles, u32 n, u32 *__restrict__ nonempty)
{
    const int d = threadIdx.x;
    const u32 start = off[(u64)d * n_tiles];
    const u32 end = d + 1 < IX_DIGITS ? off[(u64)(d + 1) * n_tiles] : n;
    const int c = __syncthreads_count(end != start);
    if (d == 0)
        *nonempty = (u32)c;
}

// Stable scatter of one tile.  Wave w owns the slice [w * 64 * IX_ITEMS, ...) of the tile, element (item i, lane l) at
// slice + 64 i + l.  A key's rank inside its digit = the keys of that digit in earlier waves (wcount after the scan over
// waves, which also adds the tile's global base) + in earlier items of its wave (wcount[wave] while the items run) + in
// lower lanes of its item (eight ballots).
__global__ __launch_bounds__(IX_THREADS) void index_scatter_kernel(IndexSortSrc s, u64 n, int shift, u32 n_tiles,
                                                                   const u32 *__restrict__ off, u64 *__restrict__ out_r,
                                                                   u32 *__restrict__ out_row)
{
    __shared__ u32 wcount[IX_WAVES][IX_DIGITS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int w = 0; w < IX_WAVES; w++)
        wcount[w][tid] = 0;
    __syncthreads();
    const u64 slice = (u64)blockIdx.x * INDEX_SORT_TILE + (u64)wave * 64 * IX_ITEMS;
    volatile u32 *wc = wcount[wave];
    u64 r[IX_ITEMS];
    u32 row[IX_ITEMS], rank[IX_ITEMS];
#pragma unroll
    for (int i = 0; i < IX_ITEMS; i++) {
        const u64 idx = slice + (u64)i * 64 + lane;
        const bool valid = idx < n;
        r[i] = 0;
        row[i] = 0;
        if (valid)
            ix_load(s, idx, &r[i], &row[i]);
        const u32 d = (u32)(r[i] >> shift) & (IX_DIGITS - 1);
        u64 same = __ballot(valid);                 // the lanes of this item that carry the same digit
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1;
            const u64 bal = __ballot(valid && bit);
            same &= bit ? bal : ~bal;
        }
        const u32 lower = (u32)__popcll(same & (((u64)1 << lane) - 1));
        const u32 prev = valid ? wc[d] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (valid && lower == 0)                    // one lane per digit of the item
            wc[d] = prev + (u32)__popcll(same);
        __builtin_amdgcn_wave_barrier();
        rank[i] = prev + lower;
    }
    __syncthreads();
    {
        u32 base = off[(u64)tid * n_tiles + blockIdx.x];
#pragma unroll
        for (int w = 0; w < IX_WAVES; w++) {
            const u32 t = wcount[w][tid];
            wcount[w][tid] = base;
            base += t;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < IX_ITEMS; i++) {
        const u64 idx = slice + (u64)i * 64 + lane;
        if (idx < n) {
            const u32 d = (u32)(r[i] >> shift) & (IX_DIGITS - 1);
            const u64 pos = (u64)wcount[wave][d] + rank[i];
            if (pos < n) {                          // (always: the histogram counted the same digits)
                out_r[pos] = r[i];
                out_row[pos] = row[i];
            }
        }
    }
}

__device__ __forceinline__ u32 block_sum_256(u32 v, u32 *sh4)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0)
        sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    const u32 t = sh4[0] + sh4[1] + sh4[2] + sh4[3];
    __syncthreads();
    return t;
}

// *distinct += the positions where a new key starts
__global__ __launch_bounds__(IX_THREADS) void index_distinct_kernel(const u64 *__restrict__ r, u64 n, unsigned long long *distinct)
{
    __shared__ u32 sh4[4];
    u32 c = 0;
    for (u64 i = (u64)blockIdx.x * IX_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * IX_THREADS)
        c += (i == 0 || r[i] != r[i - 1]) ? 1u : 0u;
    const u32 t = block_sum_256(c, sh4);
    if (threadIdx.x == 0 && t)
        atomicAdd(distinct, (unsigned long long)t);
}

// first index in [0, n) with r[i] >= v (n if none) / with r[i] > v
__device__ __forceinline__ u64 ix_lower_bound(const u64 *__restrict__ r, u64 n, u64 v)
{
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (r[mid] < v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
__device__ __forceinline__ u64 ix_upper_bound(const u64 *__restrict__ r, u64 lo, u64 n, u64 v)
{
    u64 hi = n;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (r[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// One workgroup: thread j looks up the j-th concrete prefix (ascending r: disjoint, ascending ranges), the lengths are
// scanned into off[0 .. R]; beg[j] = the range's first index slot; *visited = off[R].
__global__ __launch_bounds__(1024) void index_ranges_kernel(const u64 *__restrict__ r, u64 n, FilterBits fb, int p, u32 R,
                                                            u32 *__restrict__ off, u32 *__restrict__ beg, u64 *__restrict__ visited)
{
    __shared__ u32 arr[1024];
    __shared__ u32 wtmp[16];
    const int tid = threadIdx.x;
    u32 len = 0;
    if ((u32)tid < R) {
        u64 lo, hi;
        index_prefix_range(index_prefix_at(fb, p, (u32)tid), p, fb.k, &lo, &hi);
        const u64 b = ix_lower_bound(r, n, lo);
        const u64 e = ix_upper_bound(r, b, n, hi);
        beg[tid] = (u32)b;
        len = (u32)(e - b);
    }
    const u32 total = block_scan_value<1024>(len, arr, (int)R, wtmp, tid);
    if ((u32)tid < R)
        off[tid] = arr[tid];
    if (tid == 0) {
        off[R] = total;
        *visited = total;
    }
}

constexpr int IX_SCAN_ITEMS = INDEX_SCAN_TILE / IX_THREADS;

// The two sweeps over the candidates (the concatenation of the ranges), the shape of the filtered extraction's pair:
// WRITE = false counts the matches of every tile; WRITE = true takes the scanned counts and writes the matches in index
// order.  test == 0: every candidate matches (no residual positions), candidate j is output row j and `tiles` is unused.
template <bool WRITE>
__global__ __launch_bounds__(IX_THREADS) void index_sweep_kernel(IndexScanArgs a, u32 *__restrict__ tiles, u64 *__restrict__ out_rows,
                                                                 u64 *__restrict__ out_keys, u64 cap)
{
    __shared__ u32 s_off[INDEX_MAX_RANGES + 1];
    __shared__ u32 s_beg[INDEX_MAX_RANGES];
    __shared__ u32 arr[IX_THREADS];
    __shared__ u32 wtmp[IX_WAVES];
    const int tid = threadIdx.x;
    for (u32 i = tid; i <= a.R; i += IX_THREADS)
        s_off[i] = a.off[i];
    for (u32 i = tid; i < a.R; i += IX_THREADS)
        s_beg[i] = a.beg[i];
    __syncthreads();
    const u64 j0 = (u64)blockIdx.x * INDEX_SCAN_TILE + (u64)tid * IX_SCAN_ITEMS;
    u64 key[IX_SCAN_ITEMS];
    u32 slot[IX_SCAN_ITEMS];
    u32 hit = 0, cnt = 0;
#pragma unroll
    for (int q = 0; q < IX_SCAN_ITEMS; q++) {
        const u64 j = j0 + q;
        key[q] = 0;
        slot[q] = 0;
        if (j < a.C) {
            // the range of candidate j: the last i with off[i] <= j (off[0] = 0 <= j < C = off[R]; empty ranges repeat a value)
            u32 lo = 0, hi = a.R;
            while (lo < hi) {
                const u32 mid = (lo + hi) >> 1;
                if (s_off[mid] <= (u32)j)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            const u32 i = lo - 1;
            slot[q] = s_beg[i] + ((u32)j - s_off[i]);
            key[q] = index_key_of_r(a.r[slot[q]], a.k);
            if (!a.test || filter_match(a.fd, key[q])) {
                hit |= 1u << q;
                cnt++;
            }
        }
    }
    if (!WRITE) {
        const u32 t = block_sum_256(cnt, arr);
        if (tid == 0)
            tiles[blockIdx.x] = t;
        return;
    }
    u64 pos = j0;
    if (a.test) {
        block_scan_value<IX_THREADS>(cnt, arr, IX_THREADS, wtmp, tid);
        pos = (u64)tiles[blockIdx.x] + arr[tid];
    }
#pragma unroll
    for (int q = 0; q < IX_SCAN_ITEMS; q++)
        if (hit & (1u << q)) {
            if (pos < cap) {
                if (out_rows)
                    out_rows[pos] = a.row[slot[q]];
                if (out_keys)
                    out_keys[pos] = key[q];
            }
            pos++;
        }
}

__global__ __launch_bounds__(IX_THREADS) void index_lookup_kernel(const u64 *__restrict__ r, u64 n, int k, const u64 *__restrict__ keys,
                                                                  u64 m, u64 *__restrict__ out_first, u64 *__restrict__ out_count)
{
    const u64 j = (u64)blockIdx.x * IX_THREADS + threadIdx.x;
    if (j >= m)
        return;
    const u64 key = keys[j];
    u64 first = 0, count = 0;
    if ((key & ~kmer_mask(k)) == 0) {               // bits above 2k: no key of k bases, matches nothing
        const u64 v = index_r_of_key(key, k);
        first = ix_lower_bound(r, n, v);
        count = ix_upper_bound(r, first, n, v) - first;
    }
    out_first[j] = first;
    out_count[j] = count;
}

__global__ __launch_bounds__(IX_THREADS) void index_read_kernel(const u64 *__restrict__ r, const u32 *__restrict__ row, int k, u64 first,
                                                                u64 count, u64 *__restrict__ out_rows, u64 *__restrict__ out_keys)
{
    const u64 i = (u64)blockIdx.x * IX_THREADS + threadIdx.x;
    if (i >= count)
        return;
    if (out_rows)
        out_rows[i] = row[first + i];
    if (out_keys)
        out_keys[i] = index_key_of_r(r[first + i], k);
}


// ---- append: the stable merge of the index (A) and the sorted batch (B)

// part[t] = the split of diagonal min(t * INDEX_SORT_TILE, na + nb), t = 0 .. n_tiles: one thread per tile boundary
__global__ __launch_bounds__(IX_THREADS) void index_merge_partition_kernel(const u64 *__restrict__ ar, u64 na, const u64 *__restrict__ br,
                                                                           u64 nb, u32 n_tiles, u32 *__restrict__ part)
{
    const u64 t = (u64)blockIdx.x * IX_THREADS + threadIdx.x;
    if (t > n_tiles)
        return;
    const u64 d = std::min(t * INDEX_SORT_TILE, na + nb);
    part[t] = (u32)index_merge_split([=](u64 i) { return ar[i]; }, na, [=](u64 i) { return br[i]; }, nb, d);
}

// Where entry p of a staged tile lies in LDS: one slot of padding behind every 16.  Thread t then meets its 8 consecutive
// entries at 8 t + t / 2 + i: the 16 lanes of an LDS write group (and the 32 of a read group) on 16 (32) different 8-byte
// columns of the bank row, where the dense layout puts them on two.  Lane-consecutive accesses stay conflict-free.
constexpr int IX_MERGE_SLOTS = INDEX_SORT_TILE + INDEX_SORT_TILE / 16;
__device__ __forceinline__ u32 ix_pad(u32 p)
{
    return p + (p >> 4);
}

// One tile of INDEX_SORT_TILE outputs: its slices of A and B (part[tile] .. part[tile + 1] of A, the rest of the diagonal
// of B: together the tile's outputs, at most INDEX_SORT_TILE entries) are staged in LDS, A's slice first; thread t finds
// the split of its own diagonal 8 t there and merges 8 outputs into registers; the outputs go back into LDS in output
// order and leave as whole lines.  r compares as unsigned 64-bit; an exhausted side is never read.
__global__ __launch_bounds__(IX_THREADS) void index_merge_kernel(const u64 *__restrict__ ar, const u32 *__restrict__ arow, u64 na,
                                                                 const u64 *__restrict__ br, const u32 *__restrict__ brow, u64 nb,
                                                                 const u32 *__restrict__ part, u64 *__restrict__ out_r,
                                                                 u32 *__restrict__ out_row)
{
    __shared__ u64 s_r[IX_MERGE_SLOTS];
    __shared__ u32 s_row[IX_MERGE_SLOTS];
    const u32 tid = threadIdx.x;
    const u64 d0 = (u64)blockIdx.x * INDEX_SORT_TILE;
    const u64 d1 = std::min(d0 + INDEX_SORT_TILE, na + nb);
    const u64 a0 = part[blockIdx.x], a1 = part[blockIdx.x + 1];
    const u64 b0 = d0 - a0, b1 = d1 - a1;
    if (a1 < a0 || a1 > na || b1 < b0 || b1 > nb)       // (never: the splits ascend with the diagonal)
        return;
    const u32 ta = (u32)(a1 - a0), tb = (u32)(b1 - b0), tn = ta + tb;       // tn = d1 - d0 <= INDEX_SORT_TILE
    for (u32 i = tid; i < tn; i += IX_THREADS) {
        const u32 p = ix_pad(i);
        if (i < ta) {
            s_r[p] = ar[a0 + i];
            s_row[p] = arow[a0 + i];
        } else {
            s_r[p] = br[b0 + (i - ta)];
            s_row[p] = brow[b0 + (i - ta)];
        }
    }
    __syncthreads();
    const u32 d = std::min(tid * (u32)IX_ITEMS, tn);
    u32 a = (u32)index_merge_split([&](u64 i) { return s_r[ix_pad((u32)i)]; }, ta, [&](u64 i) { return s_r[ix_pad(ta + (u32)i)]; },
                                   tb, d);
    u32 b = d - a;
    u64 va = a < ta ? s_r[ix_pad(a)] : 0, vb = b < tb ? s_r[ix_pad(ta + b)] : 0;
    u64 r[IX_ITEMS];
    u32 row[IX_ITEMS];
#pragma unroll
    for (int i = 0; i < IX_ITEMS; i++) {
        const bool has_a = a < ta, has_b = b < tb;
        const bool take_a = has_a && (!has_b || va <= vb);      // a tie goes to A: the old entry has the smaller row id
        r[i] = take_a ? va : vb;
        row[i] = 0;
        if (take_a) {
            row[i] = s_row[ix_pad(a)];
            a++;
            if (a < ta)
                va = s_r[ix_pad(a)];
        } else if (has_b) {
            row[i] = s_row[ix_pad(ta + b)];
            b++;
            if (b < tb)
                vb = s_r[ix_pad(ta + b)];
        }
    }
    __syncthreads();                                    // every thread has read its inputs
#pragma unroll
    for (int i = 0; i < IX_ITEMS; i++) {
        const u32 o = tid * IX_ITEMS + i;
        if (o < tn) {
            s_r[ix_pad(o)] = r[i];
            s_row[ix_pad(o)] = row[i];
        }
    }
    __syncthreads();
    for (u32 i = tid; i < tn; i += IX_THREADS) {
        out_r[d0 + i] = s_r[ix_pad(i)];
        out_row[d0 + i] = s_row[ix_pad(i)];
    }
}

// ---- delete: one bit per listed row id, then a stable compaction of the entries whose bit is clear

__global__ __launch_bounds__(IX_THREADS) void index_mark_kernel(const u64 *__restrict__ ids, u64 m, u64 n_bits, u32 *__restrict__ bitmap)
{
    const u64 j = (u64)blockIdx.x * IX_THREADS + threadIdx.x;
    if (j >= m)
        return;
    const u64 id = ids[j];
    if (id < n_bits)                                    // an id the index was never given: ignored
        atomicOr(&bitmap[id >> 5], 1u << (id & 31));
}

// The two sweeps of the compaction, the tile layout of the sort's scatter: wave w owns the slice [w * 64 * IX_ITEMS, ...)
// of the tile, element (item i, lane l) at slice + 64 i + l, so that every load is a whole line and the kept entries of an
// item land side by side.  An entry's rank in its tile = the kept entries of earlier waves (wsum) + of earlier items of its
// wave (a running count) + of lower lanes of its item (one ballot).  WRITE = false: tiles[tile] = the kept entries;
// WRITE = true: tiles = their exclusive scan.
template <bool WRITE>
__global__ __launch_bounds__(IX_THREADS) void index_compact_kernel(const u64 *__restrict__ r, const u32 *__restrict__ row, u64 n,
                                                                   const u32 *__restrict__ bitmap, u32 *__restrict__ tiles,
                                                                   u64 *__restrict__ out_r, u32 *__restrict__ out_row, u64 n_out)
{
    __shared__ u32 wsum[IX_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 slice = (u64)blockIdx.x * INDEX_SORT_TILE + (u64)wave * 64 * IX_ITEMS;
    u32 id[IX_ITEMS], rank[IX_ITEMS];
    u32 kept = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < IX_ITEMS; i++) {
        const u64 idx = slice + (u64)i * 64 + lane;
        bool keep = false;
        id[i] = 0;
        if (idx < n) {
            id[i] = row[idx];
            keep = !((bitmap[id[i] >> 5] >> (id[i] & 31)) & 1u);
        }
        const u64 bal = __ballot(keep);
        rank[i] = cnt + (u32)__popcll(bal & (((u64)1 << lane) - 1));
        cnt += (u32)__popcll(bal);
        kept |= keep ? 1u << i : 0u;
    }
    if (lane == 0)
        wsum[wave] = cnt;
    __syncthreads();
    if (!WRITE) {
        if (tid == 0)
            tiles[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        return;
    }
    u64 base = tiles[blockIdx.x];
    for (int w = 0; w < wave; w++)
        base += wsum[w];
#pragma unroll
    for (int i = 0; i < IX_ITEMS; i++)
        if (kept & (1u << i)) {
            const u64 pos = base + rank[i];
            if (pos < n_out) {                          // (always: the count sweep saw the same bits)
                out_r[pos] = r[slice + (u64)i * 64 + lane];
                out_row[pos] = id[i];
            }
        }
}

}  // namespace

u32 index_sort_tiles(u64 n)
{
    return (u32)((n + INDEX_SORT_TILE - 1) / INDEX_SORT_TILE);
}

hipError_t launch_index_hist(const IndexSortSrc &src, u64 n, int shift, u32 *hist, hipStream_t s)
{
    const u32 nt = index_sort_tiles(n);
    hipLaunchKernelGGL(index_hist_kernel, dim3(nt), dim3(IX_THREADS), 0, s, src, n, shift, nt, hist);
    return hipGetLastError();
}

hipError_t launch_index_digit_bins(const u32 *off, u64 n, u32 *nonempty, hipStream_t s)
{
    hipLaunchKernelGGL(index_digit_bins_kernel, dim3(1), dim3(IX_DIGITS), 0, s, off, index_sort_tiles(n), (u32)n, nonempty);
    return hipGetLastError();
}

hipError_t launch_index_scatter(const IndexSortSrc &src, u64 n, int shift, const u32 *off, u64 *out_r, u32 *out_row, hipStream_t s)
{
    const u32 nt = index_sort_tiles(n);
    hipLaunchKernelGGL(index_scatter_kernel, dim3(nt), dim3(IX_THREADS), 0, s, src, n, shift, nt, off, out_r, out_row);
    return hipGetLastError();
}

hipError_t launch_index_distinct(const u64 *r, u64 n, u64 *distinct, hipStream_t s)
{
    const u64 nb = std::min<u64>((n + INDEX_SORT_TILE - 1) / INDEX_SORT_TILE, 2048);
    hipLaunchKernelGGL(index_distinct_kernel, dim3((unsigned)nb), dim3(IX_THREADS), 0, s, r, n,
                       reinterpret_cast<unsigned long long *>(distinct));
    return hipGetLastError();
}

hipError_t launch_index_ranges(const u64 *r, u64 n, const FilterBits &fb, int p, u32 R, u32 *off, u32 *beg, u64 *visited,
                               hipStream_t s)
{
    if (R > INDEX_MAX_RANGES)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(index_ranges_kernel, dim3(1), dim3(1024), 0, s, r, n, fb, p, R, off, beg, visited);
    return hipGetLastError();
}

u32 index_scan_tiles(u64 C)
{
    return (u32)((C + INDEX_SCAN_TILE - 1) / INDEX_SCAN_TILE);
}

hipError_t launch_index_sweep_count(const IndexScanArgs &a, u32 *tile_counts, hipStream_t s)
{
    hipLaunchKernelGGL(index_sweep_kernel<false>, dim3(index_scan_tiles(a.C)), dim3(IX_THREADS), 0, s, a, tile_counts,
                       (u64 *)nullptr, (u64 *)nullptr, (u64)0);
    return hipGetLastError();
}

hipError_t launch_index_sweep_write(const IndexScanArgs &a, const u32 *tile_offsets, u64 *out_rows, u64 *out_keys, u64 cap,
                                    hipStream_t s)
{
    hipLaunchKernelGGL(index_sweep_kernel<true>, dim3(index_scan_tiles(a.C)), dim3(IX_THREADS), 0, s, a,
                       const_cast<u32 *>(tile_offsets), out_rows, out_keys, cap);
    return hipGetLastError();
}

hipError_t launch_index_lookup(const u64 *r, u64 n, int k, const u64 *keys, u64 m, u64 *out_first, u64 *out_count, hipStream_t s)
{
    hipLaunchKernelGGL(index_lookup_kernel, dim3((unsigned)((m + IX_THREADS - 1) / IX_THREADS)), dim3(IX_THREADS), 0, s, r, n, k,
                       keys, m, out_first, out_count);
    return hipGetLastError();
}

hipError_t launch_index_read(const u64 *r, const u32 *row, int k, u64 first, u64 count, u64 *out_rows, u64 *out_keys, hipStream_t s)
{
    hipLaunchKernelGGL(index_read_kernel, dim3((unsigned)((count + IX_THREADS - 1) / IX_THREADS)), dim3(IX_THREADS), 0, s, r, row,
                       k, first, count, out_rows, out_keys);
    return hipGetLastError();
}

hipError_t launch_index_merge_partition(const u64 *ar, u64 na, const u64 *br, u64 nb, u32 *part, hipStream_t s)
{
    const u32 nt = index_sort_tiles(na + nb);
    hipLaunchKernelGGL(index_merge_partition_kernel, dim3(nt / IX_THREADS + 1), dim3(IX_THREADS), 0, s, ar, na, br, nb, nt, part);
    return hipGetLastError();
}

hipError_t launch_index_merge(const u64 *ar, const u32 *arow, u64 na, const u64 *br, const u32 *brow, u64 nb, const u32 *part,
                              u64 *out_r, u32 *out_row, hipStream_t s)
{
    hipLaunchKernelGGL(index_merge_kernel, dim3(index_sort_tiles(na + nb)), dim3(IX_THREADS), 0, s, ar, arow, na, br, brow, nb, part,
                       out_r, out_row);
    return hipGetLastError();
}

u64 index_bitmap_words(u64 n_bits)
{
    return (n_bits + 31) / 32;
}

hipError_t launch_index_mark(const u64 *ids, u64 m, u64 n_bits, u32 *bitmap, hipStream_t s)
{
    hipLaunchKernelGGL(index_mark_kernel, dim3((unsigned)((m + IX_THREADS - 1) / IX_THREADS)), dim3(IX_THREADS), 0, s, ids, m, n_bits,
                       bitmap);
    return hipGetLastError();
}

hipError_t launch_index_compact_count(const u32 *row, u64 n, const u32 *bitmap, u32 *tile_counts, hipStream_t s)
{
    hipLaunchKernelGGL(index_compact_kernel<false>, dim3(index_sort_tiles(n)), dim3(IX_THREADS), 0, s, (const u64 *)nullptr, row, n,
                       bitmap, tile_counts, (u64 *)nullptr, (u32 *)nullptr, (u64)0);
    return hipGetLastError();
}

hipError_t launch_index_compact_write(const u64 *r, const u32 *row, u64 n, const u32 *bitmap, const u32 *tile_offsets, u64 *out_r,
                                      u32 *out_row, u64 n_out, hipStream_t s)
{
    hipLaunchKernelGGL(index_compact_kernel<true>, dim3(index_sort_tiles(n)), dim3(IX_THREADS), 0, s, r, row, n, bitmap,
                       const_cast<u32 *>(tile_offsets), out_r, out_row, n_out);
    return hipGetLastError();
}

}  // namespace dnagpu
