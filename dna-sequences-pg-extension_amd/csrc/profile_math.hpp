// profile_math.hpp -- the arithmetic of dnagpu_table_profile, shared by the kernels (profile_kernels.hip), the
// host driver (profile_host.hip) and the host check tests/host/profile_math_check.cpp: the width of a profile, the rows of a
// sequence, its class and its items, the rows of an item, and the strand arithmetic of a column (2k <= 12 bits).
//
// A sequence of at most PROFILE_WAVE_ROWS rows is counted by one wave, which writes its whole output row (the WAVE class).
// A longer one (the TILED class) is cut into items of PROFILE_TILE_ROWS rows, one workgroup each; item t of a sequence
// holds its rows [t * PROFILE_TILE_ROWS, min(rows, (t + 1) * PROFILE_TILE_ROWS)).  A tiled sequence of ONE item has its row
// written by that item; only a sequence of several items (profile_is_shared) has its row zeroed first and added into.
#pragma once
#include "kmer_device.hpp"

namespace dnagpu {

constexpr int PROFILE_MAX_K = 6;
constexpr u64 PROFILE_WAVE_ROWS = 2048;
constexpr u64 PROFILE_CHUNK_ROWS = 8192;                   // what a workgroup takes in one step: 256 threads x 32 rows
constexpr u64 PROFILE_TILE_ROWS = 8 * PROFILE_CHUNK_ROWS;  // an item: 8 steps into one LDS histogram, then one flush
static_assert(PROFILE_WAVE_ROWS < PROFILE_TILE_ROWS && PROFILE_TILE_ROWS % 32 == 0, "the two classes, and whole words of rows");

// columns of a profile: 4^k, or 0 where no dense profile is offered
__host__ __device__ __forceinline__ u64 profile_width(int k)
{
    return k >= 1 && k <= PROFILE_MAX_K ? (u64)1 << (2 * k) : 0;
}

// rows of one sequence of len bases: the 64-bit restatement of dna.c:781
__host__ __device__ __forceinline__ u64 profile_seq_rows(u64 len, int k) { return len >= (u64)k ? len - (u64)k + 1 : 0; }

__host__ __device__ __forceinline__ bool profile_is_tiled(u64 rows) { return rows > PROFILE_WAVE_ROWS; }
// more than one item: the items share the output row
__host__ __device__ __forceinline__ bool profile_is_shared(u64 rows) { return rows > PROFILE_TILE_ROWS; }

// items of a sequence of `rows` rows: 0 for the wave class
__host__ __device__ __forceinline__ u64 profile_items(u64 rows)
{
    return profile_is_tiled(rows) ? (rows + PROFILE_TILE_ROWS - 1) / PROFILE_TILE_ROWS : 0;
}

// the rows [*r0, *r1) of item `tile` of a sequence of `rows` rows
__host__ __device__ __forceinline__ void profile_item_rows(u64 rows, u64 tile, u64 *r0, u64 *r1)
{
    *r0 = tile * PROFILE_TILE_ROWS;
    *r1 = rows - *r0 < PROFILE_TILE_ROWS ? rows : *r0 + PROFILE_TILE_ROWS;
}

// Item -> sequence.  off[0 .. n) = the exclusive scan of the sequences' item counts, item < their sum: the LAST i with
// off[i] <= item.  (off[i + 1] > item or i == n - 1, so that sequence has items and `item - off[i]` is one of them;
// sequences without items share their offset with the next one and are stepped over.)
__host__ __device__ __forceinline__ u64 profile_item_seq(const u32 *off, u64 n, u32 item)
{
    u64 lo = 0, hi = n;                                    // off[lo] <= item (off[0] == 0); off[hi] > item, or hi == n
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (off[mid] <= item)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// ---- strand arithmetic of a column c < 4^k, k <= 6 (codes A = 0, T = 1, C = 2, G = 3: the complement is code ^ 1)
// the k 2-bit fields of c in reverse order
__host__ __device__ __forceinline__ u32 profile_rev_fields(u32 c, int k)
{
    c = ((c >> 2) & 0x3333u) | ((c & 0x3333u) << 2);
    c = ((c >> 4) & 0x0F0Fu) | ((c & 0x0F0Fu) << 4);
    c = ((c >> 8) & 0x00FFu) | ((c & 0x00FFu) << 8);       // 8 fields of 16 bits reversed
    return c >> (16 - 2 * k);
}
__host__ __device__ __forceinline__ u32 profile_rc(u32 c, int k)
{
    return profile_rev_fields(c, k) ^ (0x5555u & ((1u << (2 * k)) - 1u));
}
// c comes no later than rc(c) in text order under A < T < C < G (strand_math.hpp's kmer_is_canonical: the rank of a key is
// its fields reversed, and the rank of rc(c) is c ^ M)
__host__ __device__ __forceinline__ bool profile_is_canonical(u32 c, int k)
{
    return profile_rev_fields(c, k) <= (c ^ (0x5555u & ((1u << (2 * k)) - 1u)));
}
// the column a row of key c is counted in under DNAGPU_PROFILE_CANONICAL
__host__ __device__ __forceinline__ u32 profile_fold_target(u32 c, int k)
{
    return profile_is_canonical(c, k) ? c : profile_rc(c, k);
}
// The fold as a gather: column c of the canonical profile from the forward counts T.  *other = the second column to add
// (rc(c)), valid when the function returns 2; returns the number of forward columns that land in c: 0 (c is not
// canonical), 1 (c is its own reverse complement) or 2.
__host__ __device__ __forceinline__ int profile_fold_sources(u32 c, int k, u32 *other)
{
    const u32 r = profile_rc(c, k);
    *other = r;
    if (!profile_is_canonical(c, k))
        return 0;
    return r == c ? 1 : 2;
}
// The same for column c + j of the quad c .. c + 3 (c % 4 == 0, j in 0 .. 3) from ONE reversal, rev_c =
// profile_rev_fields(c, k): the four differ in base 0 alone, which is the top field of the reversal.
__host__ __device__ __forceinline__ int profile_fold_sources_quad(u32 c, u32 rev_c, int j, int k, u32 *other)
{
    const u32 m = 0x5555u & ((1u << (2 * k)) - 1u);
    const u32 rj = rev_c | ((u32)j << (2 * k - 2));
    *other = rj ^ m;
    if (rj > ((c + (u32)j) ^ m))
        return 0;
    return *other == c + (u32)j ? 1 : 2;
}

}  // namespace dnagpu
