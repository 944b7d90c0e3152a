// acc_kernels.hip -- the k-mer accumulator (dnagpu_acc_*): a hash-partitioned table of 64-bit counts whose partitions
// are merged in LDS (DESIGN.md "accumulator").
//
// Layout: P = 2^pbits partitions of ACC_SLOTS 16-byte slots {key, u64 count}; count 0 marks an empty slot, so every
// key value -- the all-ones key of 32 G's included -- is a key.  A key lives in partition h >> (64 - pbits) of
// h = splitmix64(key), probing linearly (inside its partition, wrapping) from slot h & (ACC_SLOTS - 1).  occ[p] = the
// occupied slots of partition p; a partition with occ[p] == 0 is never read, so its slots need no initialisation.
//
// An add: acc_bin scatters the histogram's groups into per-partition bins (one returning atomic per group on an
// L2-sized cursor array, one 16-byte store); acc_merge then runs one workgroup per partition that loads the partition
// into LDS, adds the bin there and writes the partition back whole.  Keys inside one histogram are distinct, so two
// groups of one bin never meet: phase A adds to the keys already present (read-only probes of slots occupied at load),
// phase B claims empty slots for the rest by LDS compare-and-swap on the count.  No per-group global atomics in the merge.
//
// The canonical add folds a histogram strand-neutrally: the bin stores the canonical form of every key, so
// x and rc(x) of one histogram arrive as the SAME key and the sentence above no longer holds.  What still holds: the
// arrivals that were not flipped are distinct among themselves, and so are the flipped ones (bit 63 of the bin's count
// word tells them apart).  The CANON instantiation of the merge therefore runs phase B class by class; see there.
#include <hip/hip_runtime.h>

#include "acc_device.hpp"
#include "strand_math.hpp"

namespace dnagpu {

namespace {

// (acc_home, ld_slot / st_slot and load_region: acc_device.hpp -- the join's partition path loads a partition the same way)
constexpr int MERGE_NT = ACC_NT;                           // threads of a partition's workgroup
constexpr int PER_T = ACC_PER_T;                           // slots (and at most bin entries) per thread: 8
constexpr u64 FLIPPED = (u64)1 << 63;                      // canonical bins: the entry's key is rc of the histogram's key

__device__ __forceinline__ void store_region(const u64 *lds, u64 *__restrict__ region)
{
#pragma unroll
    for (int j = 0; j < PER_T; j++) {
        const int s = j * MERGE_NT + (int)threadIdx.x;
        st_slot(region + 2 * (u64)s, lds[2 * s], lds[2 * s + 1]);
    }
}

// claims an empty slot for a key that is not in the partition (keys distinct: no compare needed); false when the
// partition is full, which the host's load bound rules out
__device__ __forceinline__ bool lds_claim(u64 *lds, u64 key, u64 cnt, u32 s)
{
    for (int probe = 0; probe < ACC_SLOTS; probe++) {
        unsigned long long *pc = reinterpret_cast<unsigned long long *>(&lds[2 * s + 1]);
        if (atomicCAS(pc, 0ull, (unsigned long long)cnt) == 0ull) {
            lds[2 * s] = key;
            return true;
        }
        s = (s + 1) & (ACC_SLOTS - 1);
    }
    return false;
}

__device__ __forceinline__ u32 block_sum_u32(u32 v, u32 *wtmp)
{
    const u32 w = wave_sum(v);
    if ((threadIdx.x & 63) == 0)
        wtmp[threadIdx.x >> 6] = w;
    __syncthreads();
    u32 t = 0;
#pragma unroll
    for (int i = 0; i < MERGE_NT / 64; i++)
        t += wtmp[i];
    return t;
}

}  // namespace

// one thread per histogram slot: padding (count 0) skipped, everything else to its partition's bin.  CANON: the canonical
// form of the key (k bases) goes to the partition of that form; a flipped key is marked in the count word (counts arrive
// as 32 bits, so bit 63 is free)
template <bool CANON>
__device__ __forceinline__ void acc_bin(const u64 *__restrict__ keys, const u32 *__restrict__ counts, u64 n, int pbits,
                                        u32 *__restrict__ cursor, u64 *__restrict__ bins, u32 bin_cap, int k)
{
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const u32 c = counts[i];
    if (c == 0)
        return;
    u64 key = keys[i], word = c;
    if constexpr (CANON) {
        bool flipped;
        key = kmer_canonical(key, k, &flipped);
        word |= flipped ? FLIPPED : 0;
    }
    const u64 p = splitmix64(key) >> (64 - pbits);
    const u32 at = atomicAdd(&cursor[p], 1u);
    if (at < bin_cap)
        st_slot(bins + 2 * (p * bin_cap + at), key, word);
}
__global__ __launch_bounds__(256) void acc_bin_kernel(const u64 *__restrict__ keys, const u32 *__restrict__ counts, u64 n,
                                                      int pbits, u32 *__restrict__ cursor, u64 *__restrict__ bins, u32 bin_cap)
{
    acc_bin<false>(keys, counts, n, pbits, cursor, bins, bin_cap, 0);
}
__global__ __launch_bounds__(256) void acc_bin_canonical_kernel(const u64 *__restrict__ keys, const u32 *__restrict__ counts,
                                                                u64 n, int pbits, u32 *__restrict__ cursor,
                                                                u64 *__restrict__ bins, u32 bin_cap, int k)
{
    acc_bin<true>(keys, counts, n, pbits, cursor, bins, bin_cap, k);
}

// stats[0] = max over partitions of occ + arrivals, stats[1] = max arrivals
__global__ __launch_bounds__(256) void acc_bin_stats_kernel(const u32 *__restrict__ occ, const u32 *__restrict__ cursor, u64 P,
                                                            u32 *__restrict__ stats)
{
    u32 m0 = 0, m1 = 0;
    for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (u64)gridDim.x * blockDim.x) {
        const u32 a = cursor[p];
        m0 = max(m0, occ[p] + a);
        m1 = max(m1, a);
    }
    for (int off = 32; off > 0; off >>= 1) {
        m0 = max(m0, (u32)__shfl_down((int)m0, off));
        m1 = max(m1, (u32)__shfl_down((int)m1, off));
    }
    __shared__ u32 part[2][4];
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = m0;
        part[1][threadIdx.x >> 6] = m1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const u32 *q = part[threadIdx.x];
        atomicMax(&stats[threadIdx.x], max(max(q[0], q[1]), max(q[2], q[3])));
    }
}

// One workgroup per partition with arrivals.  commit == 0: a dry run that only counts the arrivals whose key is new
// (stats: [0] max of occ + new as u32, [2..3] the sum of new as u64).  commit == 1: the merge itself; occ[p] grows by
// the new keys, stats[2..3] receives their sum, stats[1] is set if a partition ran full (never, under the host's bound).
//
// CANON (a bin of acc_bin_canonical_kernel): a key may arrive twice, unflipped and flipped.  Phase A is unchanged -- two
// arrivals for one resident key are two atomic adds.  Phase B runs class by class, each step closed by a barrier:
//   B1   the pending unflipped arrivals claim slots (distinct among themselves and from the resident keys);
//   B2a  every pending flipped arrival probes again, read-only as phase A: if B1 brought its key in, it adds and is done;
//   B2b  the flipped arrivals still pending claim slots (distinct among themselves and, now, from everything present).
// B2a and B2b are two steps because a claim publishes the slot's count before its key: a probe that ran beside the claims
// could compare against a key not yet written, and the key a fresh slot holds, 0, is a canonical key (T x k folds into it).
// Only the keys that are really new are counted: the unflipped pending and the flipped ones still pending after B2a.  The
// dry run needs that same number, so it performs B1 and B2a in LDS and skips only B2b, the store back and occ.
// One exception: a dry run can meet occ + the new unflipped keys > ACC_SLOTS (occ <= ACC_BOUND, arrivals <= ACC_SLOTS).  B1 then
// fills LDS, the claims that find no slot give up after ACC_SLOTS probes, and a flipped arrival whose partner found none
// counts as new.  The number is then too high, never too low, and it belongs to a partition whose occ + new is past the
// bound anyway: the host grows the table, from a bound that is still an upper one.
template <bool CANON>
__global__ __launch_bounds__(MERGE_NT) void acc_merge_kernel(u64 *__restrict__ table, u32 *__restrict__ occ,
                                                             const u32 *__restrict__ cursor, const u64 *__restrict__ bins,
                                                             u32 bin_cap, int commit, u32 *__restrict__ stats)
{
    __shared__ u64 lds[2 * ACC_SLOTS];
    __shared__ u32 wtmp[MERGE_NT / 64];
    const u64 p = blockIdx.x;
    const u32 n_arr = min(cursor[p], bin_cap);
    if (n_arr == 0)
        return;
    const u32 o = occ[p];
    u64 *region = table + 2 * p * ACC_SLOTS;
    load_region(lds, region, o != 0);
    __syncthreads();
    const u64 *bin = bins + 2 * p * bin_cap;
    // phase A: keys already present (slots occupied at load never change key, so the probes need no ordering)
    u64 key[PER_T], cnt[PER_T];
    u32 pending = 0, flipped = 0;
#pragma unroll
    for (int j = 0; j < PER_T; j++) {
        const u32 e = (u32)j * MERGE_NT + threadIdx.x;
        key[j] = 0;
        cnt[j] = 0;
        if (e >= n_arr)
            continue;
        ld_slot(bin + 2 * (u64)e, key[j], cnt[j]);
        if constexpr (CANON) {
            flipped |= cnt[j] & FLIPPED ? 1u << j : 0u;
            cnt[j] &= ~FLIPPED;
        }
        u32 s = acc_home(splitmix64(key[j]));
        bool found = false;
        for (int probe = 0; probe < ACC_SLOTS; probe++) {
            if (lds[2 * s + 1] == 0)
                break;
            if (lds[2 * s] == key[j]) {
                found = true;
                if (commit)
                    atomicAdd(reinterpret_cast<unsigned long long *>(&lds[2 * s + 1]), (unsigned long long)cnt[j]);
                break;
            }
            s = (s + 1) & (ACC_SLOTS - 1);
        }
        if (!found)
            pending |= 1u << j;
    }
    u32 n_mine = 0;                                // new keys of this thread that already hold a slot (CANON: B1's)
    bool full = false;
    if constexpr (CANON) {
        __syncthreads();                           // (phase A's probes are over before a claim changes a slot)
        const u32 first_class = pending & ~flipped;
#pragma unroll
        for (int j = 0; j < PER_T; j++)            // B1
            if (first_class & (1u << j))
                full |= !lds_claim(lds, key[j], cnt[j], acc_home(splitmix64(key[j])));
        n_mine = (u32)__builtin_popcount(first_class);
        pending &= flipped;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER_T; j++) {          // B2a
            if (!(pending & (1u << j)))
                continue;
            u32 s = acc_home(splitmix64(key[j]));
            for (int probe = 0; probe < ACC_SLOTS; probe++) {
                if (lds[2 * s + 1] == 0)
                    break;
                if (lds[2 * s] == key[j]) {
                    atomicAdd(reinterpret_cast<unsigned long long *>(&lds[2 * s + 1]), (unsigned long long)cnt[j]);
                    pending &= ~(1u << j);
                    break;
                }
                s = (s + 1) & (ACC_SLOTS - 1);
            }
        }
    }
    const u32 n_new = block_sum_u32(n_mine + (u32)__builtin_popcount(pending), wtmp);
    if (!commit) {
        if (threadIdx.x == 0) {
            atomicMax(&stats[0], o + n_new);
            if (n_new)
                atomicAdd(reinterpret_cast<unsigned long long *>(stats + 2), (unsigned long long)n_new);
        }
        return;
    }
    // phase B (CANON: B2b): new keys claim empty slots
#pragma unroll
    for (int j = 0; j < PER_T; j++)
        if (pending & (1u << j))
            full |= !lds_claim(lds, key[j], cnt[j], acc_home(splitmix64(key[j])));
    __syncthreads();
    store_region(lds, region);
    if (threadIdx.x == 0) {
        occ[p] = o + n_new;
        if (n_new)
            atomicAdd(reinterpret_cast<unsigned long long *>(stats + 2), (unsigned long long)n_new);
    }
    if (full)
        atomicOr(&stats[1], 1u);
}

// growth: new partition q of 2^new_bits takes the keys of old partition q >> (new_bits - old_bits) whose hash says q
__global__ __launch_bounds__(MERGE_NT) void acc_split_kernel(const u64 *__restrict__ old_table, const u32 *__restrict__ old_occ,
                                                             int old_bits, u64 *__restrict__ new_table, u32 *__restrict__ new_occ,
                                                             int new_bits, u32 *__restrict__ stats)
{
    __shared__ u64 lds[2 * ACC_SLOTS];
    __shared__ u32 wtmp[MERGE_NT / 64];
    const u64 q = blockIdx.x;
    const u64 parent = q >> (new_bits - old_bits);
    if (old_occ[parent] == 0) {
        if (threadIdx.x == 0)
            new_occ[q] = 0;
        return;
    }
    load_region(lds, nullptr, false);
    __syncthreads();
    const u64 *src = old_table + 2 * parent * ACC_SLOTS;
    u32 mine = 0;
    bool full = false;
#pragma unroll
    for (int j = 0; j < PER_T; j++) {
        const u64 s = (u64)j * MERGE_NT + threadIdx.x;
        u64 k, c;
        ld_slot(src + 2 * s, k, c);
        if (c == 0)
            continue;
        const u64 h = splitmix64(k);
        if ((h >> (64 - new_bits)) != q)
            continue;
        full |= !lds_claim(lds, k, c, acc_home(h));
        mine++;
    }
    const u32 n = block_sum_u32(mine, wtmp);   // (synchronises: every claim is in LDS)
    if (n)
        store_region(lds, new_table + 2 * q * ACC_SLOTS);
    if (threadIdx.x == 0)
        new_occ[q] = n;
    if (full)
        atomicOr(&stats[1], 1u);
}

// res[0] += sum(count), res[1] += #(count == 1), res[2] += sum(pair_mix(key, count)) over the occupied partitions
__global__ __launch_bounds__(256) void acc_summary_kernel(const u64 *__restrict__ table, const u32 *__restrict__ occ, u64 P,
                                                          u64 *__restrict__ res)
{
    __shared__ u64 part[3][4];
    u64 t = 0, u = 0, c = 0;
    for (u64 p = blockIdx.x; p < P; p += gridDim.x) {
        if (occ[p] == 0)
            continue;
        const u64 *region = table + 2 * p * ACC_SLOTS;
        for (u32 s = threadIdx.x; s < (u32)ACC_SLOTS; s += 256) {
            u64 k, n;
            ld_slot(region + 2 * (u64)s, k, n);
            if (n == 0)
                continue;
            t += n;
            u += n == 1;
            c += pair_mix(k, n);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        t += __shfl_down(t, off);
        u += __shfl_down(u, off);
        c += __shfl_down(c, off);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = t;
        part[1][threadIdx.x >> 6] = u;
        part[2][threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const u64 v = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        atomicAdd(reinterpret_cast<unsigned long long *>(res + threadIdx.x), (unsigned long long)v);
    }
}

// dense view: group r (partition order, slot order inside a partition; pre[p] = groups before partition p) goes to
// out[r - first] when r is in [first, first + count).  One workgroup per partition p_lo + blockIdx.x.
__global__ __launch_bounds__(MERGE_NT) void acc_gather_kernel(const u64 *__restrict__ table, const u32 *__restrict__ occ,
                                                              const u64 *__restrict__ pre, u64 p_lo, u64 first, u64 count,
                                                              u64 *__restrict__ out_keys, u64 *__restrict__ out_counts)
{
    __shared__ u32 arr[MERGE_NT];
    __shared__ u32 wtmp[MERGE_NT / 64];
    const u64 p = p_lo + blockIdx.x;
    if (occ[p] == 0)
        return;
    const u64 *region = table + 2 * p * ACC_SLOTS;
    const int tid = threadIdx.x;
    u64 k[PER_T], c[PER_T];
    u32 mine = 0;
#pragma unroll
    for (int j = 0; j < PER_T; j++) {              // thread tid owns slots tid * PER_T .. + PER_T (ranks in slot order)
        ld_slot(region + 2 * ((u64)tid * PER_T + j), k[j], c[j]);
        mine += c[j] != 0;
    }
    block_scan_value<MERGE_NT>(mine, arr, MERGE_NT, wtmp, tid);
    u64 r = pre[p] + arr[tid];
#pragma unroll
    for (int j = 0; j < PER_T; j++) {
        if (c[j] == 0)
            continue;
        if (r >= first && r - first < count) {
            if (out_keys)
                out_keys[r - first] = k[j];
            if (out_counts)
                out_counts[r - first] = c[j];
        }
        r++;
    }
}

hipError_t launch_acc_bin(const u64 *keys, const u32 *counts, u64 n, int pbits, u32 *cursor, u64 *bins, u32 bin_cap, int canon_k,
                          hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (canon_k)
        hipLaunchKernelGGL(acc_bin_canonical_kernel, grid, dim3(256), 0, s, keys, counts, n, pbits, cursor, bins, bin_cap, canon_k);
    else
        hipLaunchKernelGGL(acc_bin_kernel, grid, dim3(256), 0, s, keys, counts, n, pbits, cursor, bins, bin_cap);
    return hipGetLastError();
}

hipError_t launch_acc_bin_stats(const u32 *occ, const u32 *cursor, u64 P, u32 *stats, hipStream_t s)
{
    const u64 blocks = (P + 255) / 256;
    hipLaunchKernelGGL(acc_bin_stats_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, occ, cursor, P, stats);
    return hipGetLastError();
}

hipError_t launch_acc_merge(u64 *table, u32 *occ, u64 P, const u32 *cursor, const u64 *bins, u32 bin_cap, int commit, int canonical,
                            u32 *stats, hipStream_t s)
{
    if (canonical)
        hipLaunchKernelGGL(acc_merge_kernel<true>, dim3((unsigned)P), dim3(MERGE_NT), 0, s, table, occ, cursor, bins, bin_cap, commit,
                           stats);
    else
        hipLaunchKernelGGL(acc_merge_kernel<false>, dim3((unsigned)P), dim3(MERGE_NT), 0, s, table, occ, cursor, bins, bin_cap, commit,
                           stats);
    return hipGetLastError();
}

hipError_t launch_acc_split(const u64 *old_table, const u32 *old_occ, int old_bits, u64 *new_table, u32 *new_occ, int new_bits,
                            u32 *stats, hipStream_t s)
{
    hipLaunchKernelGGL(acc_split_kernel, dim3((unsigned)((u64)1 << new_bits)), dim3(MERGE_NT), 0, s, old_table, old_occ, old_bits,
                       new_table, new_occ, new_bits, stats);
    return hipGetLastError();
}

hipError_t launch_acc_summary(const u64 *table, const u32 *occ, u64 P, u64 *res3, hipStream_t s)
{
    hipLaunchKernelGGL(acc_summary_kernel, dim3((unsigned)(P < 4096 ? P : 4096)), dim3(256), 0, s, table, occ, P, res3);
    return hipGetLastError();
}

hipError_t launch_acc_gather(const u64 *table, const u32 *occ, const u64 *pre, u64 p_lo, u64 n_parts, u64 first, u64 count,
                             u64 *out_keys, u64 *out_counts, hipStream_t s)
{
    if (n_parts == 0)
        return hipSuccess;
    hipLaunchKernelGGL(acc_gather_kernel, dim3((unsigned)n_parts), dim3(MERGE_NT), 0, s, table, occ, pre, p_lo, first, count, out_keys,
                       out_counts);
    return hipGetLastError();
}

}  // namespace dnagpu
