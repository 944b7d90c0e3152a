// query_kernels.hip -- read-only queries over counted groups (dnagpu_hist_* / dnagpu_acc_* spectrum, select, top, rank;
// DESIGN.md 4.10): a digit histogram of the counts, a compaction of the groups whose count lies in a range, the
// sort of at most 2^20 selected rows, and the scatter of every group to the rows of its count class (rank).
//
// One abstraction feeds every kernel, a GROUP SOURCE cut into tiles of Q_TILE slots, eight per thread of a 256-thread
// workgroup:
//   QHistSrc  a histogram part: u64 keys[], u32 counts[], n slots, count 0 = padding.  A pass that needs only the counts
//             reads only the counts (4 bytes per slot, one dwordx4 = four slots per lane where the tile is whole).
//   QAccSrc   the accumulator's table: 16-byte {key, u64 count} slots read one dwordx4 at a time, count 0 = empty; a tile
//             lies inside one partition (Q_TILE divides ACC_SLOTS) and the tiles of a partition with occ == 0 are never
//             read (its slots hold nothing defined).
//   QDenseSrc dense rows u64 keys[], u64 counts[] (the tail of a ranking, compacted): the digit and select kernels only.
// No kernel writes to its source.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace dnagpu {

namespace {

constexpr int Q_NT = 256;
constexpr int Q_PER_T = 8;
static_assert(Q_NT * Q_PER_T == Q_TILE, "a tile is eight slots per thread");
static_assert(ACC_SLOTS % Q_TILE == 0, "a tile must lie inside one accumulator partition");
constexpr int Q_REG_BINS = 4;         // the lowest bins are counted in registers (uniform data: every group in one of them)

// ---- group sources: live(t) is uniform over the workgroup; slot(t, tid, j) = the slot thread tid's j-th count came from
struct HistTile {
    QHistSrc s;
    __device__ __forceinline__ bool live(u64) const { return true; }
    __device__ __forceinline__ u64 slot(u64 t, int tid, int j) const
    {
        return t * Q_TILE + (u64)(j >> 2) * (Q_NT * 4) + (u64)tid * 4 + (u64)(j & 3);
    }
    __device__ __forceinline__ void load(u64 t, int tid, u64 (&c)[Q_PER_T], u64 (&)[Q_PER_T]) const
    {
        const bool whole = (t + 1) * Q_TILE <= s.n && (reinterpret_cast<uintptr_t>(s.counts) & 15) == 0;
        if (whole) {
#pragma unroll
            for (int h = 0; h < Q_PER_T / 4; h++) {
                const uint4 v = *reinterpret_cast<const uint4 *>(s.counts + slot(t, tid, 4 * h));
                c[4 * h] = v.x;
                c[4 * h + 1] = v.y;
                c[4 * h + 2] = v.z;
                c[4 * h + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < Q_PER_T; j++) {
                const u64 i = slot(t, tid, j);
                c[j] = i < s.n ? s.counts[i] : 0;
            }
        }
    }
    __device__ __forceinline__ u64 key(u64 t, int tid, int j, const u64 (&)[Q_PER_T]) const { return s.keys[slot(t, tid, j)]; }
    // every slot's key beside its count (rank): two dwordx4 per four slots where the tile is whole; a padding slot's key is
    // read (it lies inside the extent) and never used
    __device__ __forceinline__ void load_keys(u64 t, int tid, u64 (&k)[Q_PER_T]) const
    {
        const bool whole = (t + 1) * Q_TILE <= s.n && (reinterpret_cast<uintptr_t>(s.keys) & 15) == 0;
        if (whole) {
#pragma unroll
            for (int h = 0; h < Q_PER_T / 2; h++) {
                const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(s.keys + slot(t, tid, 2 * h));
                k[2 * h] = v.x;
                k[2 * h + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < Q_PER_T; j++) {
                const u64 i = slot(t, tid, j);
                k[j] = i < s.n ? s.keys[i] : 0;
            }
        }
    }
};

struct AccTile {
    QAccSrc s;
    __device__ __forceinline__ bool live(u64 t) const { return s.occ[(t * Q_TILE) / ACC_SLOTS] != 0; }
    __device__ __forceinline__ u64 slot(u64 t, int tid, int j) const { return t * Q_TILE + (u64)j * Q_NT + (u64)tid; }
    __device__ __forceinline__ void load(u64 t, int tid, u64 (&c)[Q_PER_T], u64 (&k)[Q_PER_T]) const
    {
#pragma unroll
        for (int j = 0; j < Q_PER_T; j++) {
            const u64 i = slot(t, tid, j);
            ulonglong2 v;
            v.x = 0;
            v.y = 0;
            if (i < s.n)
                v = *reinterpret_cast<const ulonglong2 *>(s.table + 2 * i);
            k[j] = v.x;
            c[j] = v.y;
        }
    }
    __device__ __forceinline__ u64 key(u64, int, int j, const u64 (&k)[Q_PER_T]) const { return k[j]; }
    __device__ __forceinline__ void load_keys(u64, int, u64 (&)[Q_PER_T]) const {}       // (load brought them)
};

struct DenseTile {
    QDenseSrc s;
    __device__ __forceinline__ bool live(u64) const { return true; }
    __device__ __forceinline__ u64 slot(u64 t, int tid, int j) const { return t * Q_TILE + (u64)j * Q_NT + (u64)tid; }
    __device__ __forceinline__ void load(u64 t, int tid, u64 (&c)[Q_PER_T], u64 (&)[Q_PER_T]) const
    {
#pragma unroll
        for (int j = 0; j < Q_PER_T; j++) {
            const u64 i = slot(t, tid, j);
            c[j] = i < s.n ? s.counts[i] : 0;
        }
    }
    __device__ __forceinline__ u64 key(u64 t, int tid, int j, const u64 (&)[Q_PER_T]) const { return s.keys[slot(t, tid, j)]; }
};

__device__ __forceinline__ u64 tiles_of(u64 n) { return (n + Q_TILE - 1) / Q_TILE; }

// ---- the digit histogram.  bins[b] += the groups of bin b, where a group's bin is
//   spectrum: min(count, n_bins) - 1                      (dnagpu_*_spectrum)
//   else:     digit (count >> shift) & (Q_DIGITS - 1) of the groups with count >> prefix_shift == prefix (radix select)
// Bins below a.lds_bins are privatised per workgroup in LDS and flushed as one 64-bit global atomic per non-zero bin; of
// those the lowest Q_REG_BINS live in per-thread registers and meet in a wave sum (on uniform data every lane would
// otherwise add to one LDS address); bins from a.lds_bins on take global atomics (a spectrum wider than the LDS: its mass
// is in the low bins).  want_max: *maxc = max(*maxc, the largest count).
template <class Src>
__global__ __launch_bounds__(Q_NT) void query_digits_kernel(Src src, QDigit a, unsigned long long *__restrict__ bins,
                                                            unsigned long long *__restrict__ maxc)
{
    extern __shared__ u32 lds[];
    const int tid = threadIdx.x;
    for (u32 b = tid; b < a.lds_bins; b += Q_NT)
        lds[b] = 0;
    __syncthreads();
    u32 reg[Q_REG_BINS] = {0, 0, 0, 0};
    u64 mx = 0;
    const u64 n_tiles = tiles_of(src.s.n);
    for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        if (!src.live(t))
            continue;
        u64 c[Q_PER_T], k[Q_PER_T];
        src.load(t, tid, c, k);
#pragma unroll
        for (int j = 0; j < Q_PER_T; j++) {
            const u64 v = c[j];
            if (v == 0)
                continue;
            mx = v > mx ? v : mx;
            if (a.has_prefix && (v >> a.prefix_shift) != a.prefix)
                continue;
            const u64 bin = a.spectrum ? (v < a.n_bins ? v : a.n_bins) - 1 : (v >> a.shift) & (u64)(Q_DIGITS - 1);
            if (bin < Q_REG_BINS) {
#pragma unroll
                for (int r = 0; r < Q_REG_BINS; r++)
                    reg[r] += bin == (u64)r;
            } else if (bin < a.lds_bins) {
                atomicAdd(&lds[bin], 1u);
            } else {
                atomicAdd(&bins[bin], 1ull);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < Q_REG_BINS; r++) {
        const u32 w = wave_sum(reg[r]);
        if ((tid & 63) == 0 && w)
            atomicAdd(&lds[r], w);
    }
    if (a.want_max) {
        for (int off = 32; off > 0; off >>= 1) {
            const u64 o = __shfl_down(mx, off);
            mx = o > mx ? o : mx;
        }
        if ((tid & 63) == 0 && mx)
            atomicMax(maxc, (unsigned long long)mx);
    }
    __syncthreads();
    for (u32 b = tid; b < a.lds_bins; b += Q_NT) {
        const u32 v = lds[b];
        if (v)
            atomicAdd(&bins[b], (unsigned long long)v);
    }
}

// ---- select: the groups with lo <= count <= hi (lo >= 1), compacted.  One workgroup per tile: it counts its matches,
// takes ONE returning atomic on *cursor for all of them and stores each at base + its rank inside the workgroup -- rows
// from `cap` on are not stored, *cursor still counts them.
template <class Src>
__global__ __launch_bounds__(Q_NT) void query_select_kernel(Src src, u64 lo, u64 hi, u64 *__restrict__ out_keys,
                                                            u64 *__restrict__ out_counts, u64 cap,
                                                            unsigned long long *__restrict__ cursor)
{
    __shared__ u32 arr[Q_NT];
    __shared__ u32 wtmp[Q_NT / 64];
    __shared__ u64 base_s;
    const int tid = threadIdx.x;
    const u64 t = blockIdx.x;
    if (!src.live(t))
        return;
    u64 c[Q_PER_T], k[Q_PER_T];
    src.load(t, tid, c, k);
    u32 mask = 0;
#pragma unroll
    for (int j = 0; j < Q_PER_T; j++)
        if (c[j] >= lo && c[j] <= hi)
            mask |= 1u << j;
    const u32 total = block_scan_value<Q_NT>((u32)__builtin_popcount(mask), arr, Q_NT, wtmp, tid);
    if (total == 0)
        return;
    if (tid == 0)
        base_s = atomicAdd(cursor, (unsigned long long)total);
    __syncthreads();
    u64 at = base_s + arr[tid];
#pragma unroll
    for (int j = 0; j < Q_PER_T; j++) {
        if (!(mask & (1u << j)))
            continue;
        if (at < cap) {
            if (out_keys)
                out_keys[at] = src.key(t, tid, j, k);
            if (out_counts)
                out_counts[at] = c[j];
        }
        at++;
    }
}

// ---- rank: every group to the rows of its count class, class = min(count, n_classes) (the last class is the tail: every
// count from n_classes on, still to be sorted).  One workgroup per tile.  It ranks its rows inside every class, reserves the
// rows of a class with ONE returning global atomic per class the tile holds (cursors[class], which starts at the class's
// first row), and stores (key, 64-bit count) at the reserved base + rank: the rows one tile adds to a class are contiguous.
// Classes 1 .. R_FAST are ranked with a block scan of per-thread counts, two 16-bit fields in one word (on uniform data
// every group has count 1: 64 lanes taking a returning LDS atomic on one address would serialise); the other classes
// take a returning LDS atomic on the class's counter, and the lane that drew rank 0 makes the class's reservation.
constexpr int R_FAST = 2;

template <class Src>
__global__ __launch_bounds__(Q_NT) void query_rank_scatter_kernel(Src src, u32 n_classes, unsigned long long *__restrict__ cursors,
                                                                  u64 *__restrict__ out_keys, u64 *__restrict__ out_counts, u64 rows)
{
    __shared__ u32 cnt[Q_DIGITS + 1];
    __shared__ u64 base[Q_DIGITS + 1];
    __shared__ u32 arr[Q_NT];
    __shared__ u32 wtmp[Q_NT / 64];
    const int tid = threadIdx.x;
    const u64 t = blockIdx.x;
    if (!src.live(t))
        return;
    for (u32 b = tid; b <= n_classes; b += Q_NT)
        cnt[b] = 0;
    u64 c[Q_PER_T], k[Q_PER_T];
    src.load(t, tid, c, k);
    src.load_keys(t, tid, k);
    __syncthreads();
    u32 rank[Q_PER_T];
    u32 fast = 0;                                    // this thread's rows of class 1 (bits 0-15) and class 2 (bits 16-31)
#pragma unroll
    for (int j = 0; j < Q_PER_T; j++) {
        const u64 v = c[j];
        rank[j] = 0;
        if (v == 0)
            continue;
        if (v <= (u64)R_FAST) {
            const int sh = 16 * ((int)v - 1);
            rank[j] = (fast >> sh) & 0xFFFFu;
            fast += 1u << sh;
        } else {
            rank[j] = atomicAdd(&cnt[v < n_classes ? (u32)v : n_classes], 1u);
        }
    }
    const u32 total = block_scan_value<Q_NT>(fast, arr, Q_NT, wtmp, tid);      // (its barriers also end the LDS atomics)
    if (tid < R_FAST) {
        const u32 n = (total >> (16 * tid)) & 0xFFFFu;
        if (n)
            base[tid + 1] = atomicAdd(&cursors[tid + 1], (unsigned long long)n);
    }
#pragma unroll
    for (int j = 0; j < Q_PER_T; j++) {
        if (c[j] > (u64)R_FAST && rank[j] == 0) {
            const u32 cls = c[j] < n_classes ? (u32)c[j] : n_classes;
            base[cls] = atomicAdd(&cursors[cls], (unsigned long long)cnt[cls]);
        }
    }
    __syncthreads();
    const u32 before = arr[tid];
#pragma unroll
    for (int j = 0; j < Q_PER_T; j++) {
        const u64 v = c[j];
        if (v == 0)
            continue;
        const u32 cls = v < n_classes ? (u32)v : n_classes;
        u64 at = base[cls] + rank[j];
        if (v <= (u64)R_FAST)
            at += (before >> (16 * ((int)v - 1))) & 0xFFFFu;
        if (at < rows) {                             // (always, while the cursors were set from this source's spectrum)
            out_keys[at] = k[j];
            out_counts[at] = v;
        }
    }
}

__global__ __launch_bounds__(256) void query_reverse_kernel(u64 *__restrict__ keys, u64 *__restrict__ cnts, u64 n)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n / 2)
        return;
    const u64 p = n - 1 - i;
    const u64 ka = keys[i], ca = cnts[i], kb = keys[p], cb = cnts[p];
    keys[i] = kb;
    cnts[i] = cb;
    keys[p] = ka;
    cnts[p] = ca;
}

// ---- the sort of top's rows: a bitonic network over m = 2^x rows by (count descending, key ascending).  Steps whose
// partners are less than SORT_TILE apart run in LDS, a whole tile's steps per launch; the others are one launch each over
// global memory.  Not a hot path: at most 2^20 rows.
constexpr int SORT_TILE = 2048;
constexpr int SORT_NT = 1024;

__device__ __forceinline__ bool row_before(u64 ka, u64 ca, u64 kb, u64 cb) { return ca > cb || (ca == cb && ka < kb); }

// stages k_lo .. k_hi (sequence lengths), each from partner distance min(k / 2, tile / 2) down to 1
__global__ __launch_bounds__(SORT_NT) void query_sort_tile_kernel(u64 *__restrict__ keys, u64 *__restrict__ cnts, u32 tile,
                                                                  u32 k_lo, u32 k_hi)
{
    __shared__ u64 sk[SORT_TILE], sc[SORT_TILE];
    const u32 tid = threadIdx.x;
    const u32 base = blockIdx.x * tile;
    for (u32 i = tid; i < tile; i += SORT_NT) {
        sk[i] = keys[base + i];
        sc[i] = cnts[base + i];
    }
    __syncthreads();
    for (u32 k = k_lo; k <= k_hi; k <<= 1) {
        for (u32 j = (k / 2 < tile / 2 ? k / 2 : tile / 2); j > 0; j >>= 1) {
            if (tid < tile / 2) {
                const u32 i = (tid / j) * 2 * j + (tid % j), p = i + j;
                const bool up = ((base + i) & k) == 0;
                const u64 ka = sk[i], ca = sc[i], kb = sk[p], cb = sc[p];
                if (up ? row_before(kb, cb, ka, ca) : row_before(ka, ca, kb, cb)) {
                    sk[i] = kb;
                    sc[i] = cb;
                    sk[p] = ka;
                    sc[p] = ca;
                }
            }
            __syncthreads();
        }
        if (k == 0x80000000u)
            break;
    }
    for (u32 i = tid; i < tile; i += SORT_NT) {
        keys[base + i] = sk[i];
        cnts[base + i] = sc[i];
    }
}

__global__ __launch_bounds__(256) void query_sort_step_kernel(u64 *__restrict__ keys, u64 *__restrict__ cnts, u32 m, u32 k, u32 j)
{
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m / 2)
        return;
    const u32 i = (t / j) * 2 * j + (t % j), p = i + j;
    const bool up = (i & k) == 0;
    const u64 ka = keys[i], ca = cnts[i], kb = keys[p], cb = cnts[p];
    if (up ? row_before(kb, cb, ka, ca) : row_before(ka, ca, kb, cb)) {
        keys[i] = kb;
        cnts[i] = cb;
        keys[p] = ka;
        cnts[p] = ca;
    }
}

template <class Src, class S>
hipError_t run_digits(const S &s, const QDigit &a, u64 *bins, u64 *maxc, hipStream_t st)
{
    const u64 n_tiles = (s.n + Q_TILE - 1) / Q_TILE;
    if (n_tiles == 0)
        return hipSuccess;
    const unsigned grid = (unsigned)(n_tiles < 2048 ? n_tiles : 2048);          // eight workgroups per CU
    hipLaunchKernelGGL(query_digits_kernel<Src>, dim3(grid), dim3(Q_NT), (size_t)a.lds_bins * 4, st, Src{s}, a,
                       reinterpret_cast<unsigned long long *>(bins), reinterpret_cast<unsigned long long *>(maxc));
    return hipGetLastError();
}

template <class Src, class S>
hipError_t run_rank(const S &s, u32 n_classes, u64 *cursors, u64 *out_keys, u64 *out_counts, u64 rows, hipStream_t st)
{
    const u64 n_tiles = (s.n + Q_TILE - 1) / Q_TILE;
    if (n_tiles == 0)
        return hipSuccess;
    if (n_tiles > 0x7FFFFFFFull || n_classes < R_FAST + 1 || n_classes > (u32)Q_DIGITS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(query_rank_scatter_kernel<Src>, dim3((unsigned)n_tiles), dim3(Q_NT), 0, st, Src{s}, n_classes,
                       reinterpret_cast<unsigned long long *>(cursors), out_keys, out_counts, rows);
    return hipGetLastError();
}

template <class Src, class S>
hipError_t run_select(const S &s, u64 lo, u64 hi, u64 *out_keys, u64 *out_counts, u64 cap, u64 *cursor, hipStream_t st)
{
    const u64 n_tiles = (s.n + Q_TILE - 1) / Q_TILE;
    if (n_tiles == 0)
        return hipSuccess;
    if (n_tiles > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(query_select_kernel<Src>, dim3((unsigned)n_tiles), dim3(Q_NT), 0, st, Src{s}, lo, hi, out_keys, out_counts,
                       cap, reinterpret_cast<unsigned long long *>(cursor));
    return hipGetLastError();
}

}  // namespace

hipError_t launch_query_digits(const QHistSrc &s, const QDigit &a, u64 *bins, u64 *maxc, hipStream_t st)
{
    return run_digits<HistTile>(s, a, bins, maxc, st);
}
hipError_t launch_query_digits(const QAccSrc &s, const QDigit &a, u64 *bins, u64 *maxc, hipStream_t st)
{
    return run_digits<AccTile>(s, a, bins, maxc, st);
}
hipError_t launch_query_select(const QHistSrc &s, u64 lo, u64 hi, u64 *out_keys, u64 *out_counts, u64 cap, u64 *cursor,
                               hipStream_t st)
{
    return run_select<HistTile>(s, lo, hi, out_keys, out_counts, cap, cursor, st);
}
hipError_t launch_query_select(const QAccSrc &s, u64 lo, u64 hi, u64 *out_keys, u64 *out_counts, u64 cap, u64 *cursor,
                               hipStream_t st)
{
    return run_select<AccTile>(s, lo, hi, out_keys, out_counts, cap, cursor, st);
}

hipError_t launch_query_digits(const QDenseSrc &s, const QDigit &a, u64 *bins, u64 *maxc, hipStream_t st)
{
    return run_digits<DenseTile>(s, a, bins, maxc, st);
}
hipError_t launch_query_select(const QDenseSrc &s, u64 lo, u64 hi, u64 *out_keys, u64 *out_counts, u64 cap, u64 *cursor,
                               hipStream_t st)
{
    return run_select<DenseTile>(s, lo, hi, out_keys, out_counts, cap, cursor, st);
}

hipError_t launch_query_rank_scatter(const QHistSrc &s, u32 n_classes, u64 *cursors, u64 *out_keys, u64 *out_counts, u64 rows,
                                     hipStream_t st)
{
    return run_rank<HistTile>(s, n_classes, cursors, out_keys, out_counts, rows, st);
}
hipError_t launch_query_rank_scatter(const QAccSrc &s, u32 n_classes, u64 *cursors, u64 *out_keys, u64 *out_counts, u64 rows,
                                     hipStream_t st)
{
    return run_rank<AccTile>(s, n_classes, cursors, out_keys, out_counts, rows, st);
}

hipError_t launch_query_reverse(u64 *keys, u64 *counts, u64 n, hipStream_t st)
{
    if (n < 2)
        return hipSuccess;
    const u64 blocks = (n / 2 + 255) / 256;
    if (blocks > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(query_reverse_kernel, dim3((unsigned)blocks), dim3(256), 0, st, keys, counts, n);
    return hipGetLastError();
}

hipError_t launch_query_sort(u64 *keys, u64 *counts, u32 m, hipStream_t st)
{
    if (m < 2 || (m & (m - 1)))
        return hipErrorInvalidValue;
    const u32 tile = m < (u32)SORT_TILE ? m : (u32)SORT_TILE;
    hipLaunchKernelGGL(query_sort_tile_kernel, dim3(m / tile), dim3(SORT_NT), 0, st, keys, counts, tile, 2u, tile);
    for (u32 k = 2 * tile; k <= m && k != 0; k <<= 1) {
        for (u32 j = k / 2; j >= tile; j >>= 1)
            hipLaunchKernelGGL(query_sort_step_kernel, dim3((m / 2 + 255) / 256), dim3(256), 0, st, keys, counts, m, k, j);
        hipLaunchKernelGGL(query_sort_tile_kernel, dim3(m / tile), dim3(SORT_NT), 0, st, keys, counts, tile, k, k);
    }
    return hipGetLastError();
}

}  // namespace dnagpu
