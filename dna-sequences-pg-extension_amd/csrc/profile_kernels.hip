// profile_kernels.hip -- the k-mer profile of every sequence of a window of a table (dnagpu_table_profile):
//   SELECT d.id, k.kmer, count(*) FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k) AS k(kmer) GROUP BY d.id, k.kmer
// as a dense matrix of 4^k u32 columns per sequence, k <= 6.  Rows are counted into LDS histograms and a sequence's
// boundaries come from seq_starts alone: a wave or an item walks the rows of ONE sequence, so no k-mer spans two.
//   plan   one thread per sequence: its rows (out_rows) and its item count (0 for the wave class)
//   wave   one wave per sequence: a private LDS histogram, one ds_add per row, then the whole output row in coalesced
//          stores, zeros included -- no global atomic, no clearing.  The row of a sequence of SEVERAL items is written as
//          zeros here.
//   tile   one workgroup per item (afterwards, on the same stream): steps of 32 rows per thread into one LDS histogram,
//          then the flush -- the only item of a sequence stores the row, one of several issues one global atomicAdd per
//          non-zero column into the zeroed row
// DNAGPU_PROFILE_CANONICAL costs nothing per row: rows are counted forward and the fold (profile_math.hpp) happens when
// the histogram is read out.
//
// Small k: with 4, 16 or 64 columns the 64 adds of a wave-instruction land on a handful of LDS addresses, which the LDS
// serialises.  The histogram is therefore kept in PROFILE_COPIES copies, interleaved (counter = key * copies + lane %
// copies, so that the copies of one key lie in consecutive banks); the copies are summed when the histogram is read out.
#include <hip/hip_runtime.h>

#include "profile_math.hpp"
#include "stream_rows.hpp"

namespace dnagpu {

namespace {

constexpr int PF_NT = 256;                                 // threads of every workgroup here
constexpr int PF_WAVES = PF_NT / 64;
constexpr int PROFILE_COPIES = 16;                         // copies of a histogram of at most 64 columns
static_assert(PROFILE_CHUNK_ROWS == (u64)PF_NT * 32, "a step of an item is 32 rows per thread");

template <int K>
struct Geo {
    static constexpr int W = 1 << (2 * K);
    static constexpr int R = W <= 64 ? PROFILE_COPIES : 1;
    static constexpr int HW = W * R;                       // counters of one histogram: 64 .. 4096
    // where the counter of `key` lies (who = the lane or thread that adds: it picks the copy)
    static __device__ __forceinline__ u32 slot(u32 key, int who)
    {
        return R > 1 ? key * R + ((u32)who & (R - 1)) : key;
    }
};

// 16 bytes at an address that is only known to be 4-byte aligned (out_counts): one global_store_dwordx4
struct __attribute__((packed, aligned(4))) Quad {
    u32 x, y, z, w;
};

// LDS written by one lane and read by another of the same wave: DS operations of a wave execute in program order, so only
// the compiler has to be kept from reordering them
__device__ __forceinline__ void wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One thread per sequence of the window (starts = seq_starts + seq_first).
__global__ __launch_bounds__(PF_NT) void profile_plan_kernel(const u64 *__restrict__ starts, u64 seq_count, int k,
                                                             u64 *__restrict__ out_rows, u32 *__restrict__ items)
{
    for (u64 i = (u64)blockIdx.x * PF_NT + threadIdx.x; i < seq_count; i += (u64)gridDim.x * PF_NT) {
        const u64 rows = profile_seq_rows(starts[i + 1] - starts[i], k);
        if (out_rows)
            out_rows[i] = rows;
        items[i] = (u32)profile_items(rows);
    }
}

// column c of the output from the summed forward counts (get(x) = the rows of key x)
template <int K, typename Get>
__device__ __forceinline__ u32 folded(u32 c, bool canonical, Get get)
{
    if (!canonical)
        return get(c);
    u32 other;
    const int n = profile_fold_sources(c, K, &other);
    return n == 0 ? 0u : get(c) + (n == 2 ? get(other) : 0u);
}

// Sequence blockIdx.x * 4 + wave (grid-stride) per wave; h = 4 private histograms.
template <int K>
__global__ __launch_bounds__(PF_NT) void profile_wave_kernel(const u64 *__restrict__ words, u64 n_words,
                                                             const u64 *__restrict__ starts, u64 seq_count, int canonical,
                                                             u32 *__restrict__ out)
{
    constexpr int W = Geo<K>::W, R = Geo<K>::R, HW = Geo<K>::HW;
    __shared__ __attribute__((aligned(16))) u32 h_all[PF_WAVES * HW];
    const int lane = threadIdx.x & 63;
    u32 *h = h_all + (threadIdx.x >> 6) * HW;
    const u64 mask = kmer_mask(K);
    const u64 groups = (seq_count + PF_WAVES - 1) / PF_WAVES;

    for (u64 g = blockIdx.x; g < groups; g += gridDim.x) {
        const u64 i = g * PF_WAVES + (threadIdx.x >> 6);   // wave-uniform
        if (i >= seq_count)
            continue;
        const u64 s0 = starts[i];
        const u64 rows = profile_seq_rows(starts[i + 1] - s0, K);
        u32 *orow = out + i * (u64)W;

        if (profile_is_tiled(rows)) {                      // one item writes this row later, or several add into it
            if (!profile_is_shared(rows))
                continue;
            if (W >= 256) {
                for (int c = lane * 4; c < W; c += 256)
                    *reinterpret_cast<Quad *>(orow + c) = Quad{0u, 0u, 0u, 0u};
            } else if (lane < W) {
                orow[lane] = 0u;
            }
            continue;
        }

        for (int c = lane * 4; c < HW; c += 256)
            *reinterpret_cast<uint4 *>(h + c) = make_uint4(0u, 0u, 0u, 0u);
        wave_fence();
        // row r to lane r % 64: the position s0 + r + K - 1 is a base of this sequence, so word (s0 + r) / 32 exists
        for (u32 r = (u32)lane; r < (u32)rows; r += 64) {
            const u32 key = (u32)key_at(words, n_words, s0 + r, mask);
            atomicAdd(&h[Geo<K>::slot(key, lane)], 1u);
        }
        wave_fence();

        if (W >= 256) {
            for (int c = lane * 4; c < W; c += 256) {
                // the lane's four columns in one 16-byte read; the fold reads its second columns one by one
                const uint4 own = *reinterpret_cast<const uint4 *>(h + Geo<K>::slot((u32)c, 0));
                u32 v[4] = {own.x, own.y, own.z, own.w};
                if (canonical) {                           // (one reversal serves the quad: profile_fold_sources_quad)
                    const u32 rev_c = profile_rev_fields((u32)c, K);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        u32 other;
                        const int n_src = profile_fold_sources_quad((u32)c, rev_c, j, K, &other);
                        const u32 theirs = n_src == 2 ? h[Geo<K>::slot(other, 0)] : 0u;
                        v[j] = n_src == 0 ? 0u : v[j] + theirs;
                    }
                }
                *reinterpret_cast<Quad *>(orow + c) = Quad{v[0], v[1], v[2], v[3]};
            }
        } else {
            // lane c sums the copies of column c; the fold takes its second column from another lane
            u32 sum = 0;
            if (lane < W) {
#pragma unroll
                for (int j = 0; j < R; j += 4) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(h + lane * R + j);
                    sum += v.x + v.y + v.z + v.w;
                }
            }
            // (every lane takes part in the shuffle; lanes past the last column hold 0 and store nothing)
            u32 other;
            const int n_src = profile_fold_sources((u32)lane & (W - 1), K, &other);
            const u32 theirs = (u32)__shfl((int)sum, (int)other);
            if (canonical)
                sum = n_src == 0 ? 0u : sum + (n_src == 2 ? theirs : 0u);
            if (lane < W)
                orow[lane] = sum;
        }
        wave_fence();                                      // the next sequence clears what was just read
    }
}

// One item per workgroup: off = the exclusive scan of the sequences' item counts.
template <int K>
__global__ __launch_bounds__(PF_NT) void profile_tile_kernel(const u64 *__restrict__ words, u64 n_words,
                                                             const u64 *__restrict__ starts, u64 seq_count,
                                                             const u32 *__restrict__ off, int canonical, u32 *__restrict__ out)
{
    constexpr int W = Geo<K>::W, R = Geo<K>::R, HW = Geo<K>::HW;
    __shared__ __attribute__((aligned(16))) u32 h[HW];
    __shared__ u32 sums[R > 1 ? W : 1];
    __shared__ u64 item_at[4];                             // the item's sequence, its first stream base, its rows, shared?
    const int tid = threadIdx.x;
    if (tid == 0) {
        const u32 item = blockIdx.x;
        const u64 i = profile_item_seq(off, seq_count, item);
        const u64 s0 = starts[i];
        u64 r0, r1;
        const u64 seq_rows = profile_seq_rows(starts[i + 1] - s0, K);
        profile_item_rows(seq_rows, item - off[i], &r0, &r1);
        item_at[0] = i;
        item_at[1] = s0 + r0;
        item_at[2] = r1 - r0;
        item_at[3] = profile_is_shared(seq_rows) ? 1 : 0;
    }
    for (int c = tid * 4; c < HW; c += PF_NT * 4)
        *reinterpret_cast<uint4 *>(h + c) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const u64 i = item_at[0], p0 = item_at[1], n_rows = item_at[2];
    const bool shared = item_at[3] != 0;

    // Step by step, the thread's rows: 32 tid .. 32 tid + 31 of the step's PROFILE_CHUNK_ROWS; the 64 bases at the first of
    // them (the shift is the same for every thread and step).  A row that exists ends inside the sequence, so no bit behind
    // the last base enters a key.
    for (u64 first = (u64)tid * 32; first < n_rows; first += PROFILE_CHUNK_ROWS) {
        const int mine = n_rows - first < 32 ? (int)(n_rows - first) : 32;
        const u64 p = p0 + first;
        const unsigned sh = (unsigned)(p & 31) * 2;
        const Stream4 s = stream_of(words_load(words, n_words, p >> 5, sh), sh);
        const u64 lo = ((u64)s.d[1] << 32) | s.d[0], hi = ((u64)s.d[3] << 32) | s.d[2];
        const u64 mask = kmer_mask(K);
        for (int j = 0; j < mine; j++) {
            const u32 key = (u32)(funnel(lo, hi, 2u * (unsigned)j) & mask);
            atomicAdd(&h[Geo<K>::slot(key, tid)], 1u);
        }
    }
    __syncthreads();

    u32 *orow = out + i * (u64)W;
    if (R > 1) {
        if (tid < W) {
            u32 sum = 0;
#pragma unroll
            for (int j = 0; j < R; j += 4) {
                const uint4 v = *reinterpret_cast<const uint4 *>(h + tid * R + j);
                sum += v.x + v.y + v.z + v.w;
            }
            sums[tid] = sum;
        }
        __syncthreads();
    }
    // the only item of its sequence writes the row, zeros included; one of several adds what it has to the zeroed row
    for (int c = tid; c < W; c += PF_NT) {
        const u32 v = folded<K>((u32)c, canonical != 0, [&](u32 x) { return R > 1 ? sums[x] : h[Geo<K>::slot(x, 0)]; });
        if (!shared)
            orow[c] = v;
        else if (v)
            atomicAdd(&orow[c], v);
    }
}

unsigned stride_grid(u64 n, u64 per_block)
{
    const u64 g = (n + per_block - 1) / per_block;
    return (unsigned)(g < 65536 ? g : 65536);
}

template <int K>
void wave_launch(const u64 *words, u64 n_words, const u64 *starts, u64 seq_count, int canonical, u32 *out, hipStream_t s)
{
    hipLaunchKernelGGL(profile_wave_kernel<K>, dim3(stride_grid(seq_count, PF_WAVES)), dim3(PF_NT), 0, s, words, n_words, starts,
                       seq_count, canonical, out);
}
template <int K>
void tile_launch(const u64 *words, u64 n_words, const u64 *starts, u64 seq_count, const u32 *off, u32 n_items, int canonical,
                 u32 *out, hipStream_t s)
{
    hipLaunchKernelGGL(profile_tile_kernel<K>, dim3(n_items), dim3(PF_NT), 0, s, words, n_words, starts, seq_count, off, canonical,
                       out);
}

}  // namespace

hipError_t launch_profile_plan(const u64 *starts, u64 seq_count, int k, u64 *out_rows, u32 *items, hipStream_t s)
{
    if (seq_count == 0)
        return hipSuccess;
    if (profile_width(k) == 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(profile_plan_kernel, dim3(stride_grid(seq_count, PF_NT)), dim3(PF_NT), 0, s, starts, seq_count, k, out_rows,
                       items);
    return hipGetLastError();
}

hipError_t launch_profile_wave(const u64 *words, u64 n_words, const u64 *starts, u64 seq_count, int k, int canonical, u32 *out,
                               hipStream_t s)
{
    if (seq_count == 0)
        return hipSuccess;
    switch (k) {
    case 1: wave_launch<1>(words, n_words, starts, seq_count, canonical, out, s); break;
    case 2: wave_launch<2>(words, n_words, starts, seq_count, canonical, out, s); break;
    case 3: wave_launch<3>(words, n_words, starts, seq_count, canonical, out, s); break;
    case 4: wave_launch<4>(words, n_words, starts, seq_count, canonical, out, s); break;
    case 5: wave_launch<5>(words, n_words, starts, seq_count, canonical, out, s); break;
    case 6: wave_launch<6>(words, n_words, starts, seq_count, canonical, out, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_profile_tile(const u64 *words, u64 n_words, const u64 *starts, u64 seq_count, const u32 *off, u32 n_items, int k,
                               int canonical, u32 *out, hipStream_t s)
{
    if (n_items == 0)
        return hipSuccess;
    switch (k) {
    case 1: tile_launch<1>(words, n_words, starts, seq_count, off, n_items, canonical, out, s); break;
    case 2: tile_launch<2>(words, n_words, starts, seq_count, off, n_items, canonical, out, s); break;
    case 3: tile_launch<3>(words, n_words, starts, seq_count, off, n_items, canonical, out, s); break;
    case 4: tile_launch<4>(words, n_words, starts, seq_count, off, n_items, canonical, out, s); break;
    case 5: tile_launch<5>(words, n_words, starts, seq_count, off, n_items, canonical, out, s); break;
    case 6: tile_launch<6>(words, n_words, starts, seq_count, off, n_items, canonical, out, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace dnagpu
