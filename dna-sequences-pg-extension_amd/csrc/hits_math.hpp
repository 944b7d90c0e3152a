// hits_math.hpp -- the index arithmetic of dnagpu_table_hits, shared by the kernels (hits_kernels.hip), the
// host driver (hits_host.hip) and the host check tests/host/hits_math_check.cpp.
//
// A window of a table is the stream bases [a0, a1); its rows are numbered from the window's first base: row r is the k-mer
// at stream position a0 + r.  The sweep leaves one hit bit per row, 32 rows to a u32 mask word, HITS_TILE_WORDS mask words
// to a tile, and three levels of running counts:
//   tile_base[t]  hits in the tiles before tile t          (exclusive scan of the tile totals)
//   word_pre[w]   hits in the words of w's tile before w   (exclusive, inside the tile)
//   mask[w]       bit j = row 32 w + j is a hit
// C(r) = hits among rows [0, r) = tile_base[tile] + word_pre[word] + popcount(mask[word] & low), for every r in [0, n]:
// r = n (n = a1 - a0) is asked for by a last sequence of fewer than k bases, so there is always a word for it.
#pragma once
#include "kmer_device.hpp"

namespace dnagpu {

constexpr u32 HITS_ROWS_PER_WORD = 32;
constexpr u32 HITS_TILE_WORDS = 256;                       // one mask word per thread of a sweep workgroup
constexpr u32 HITS_TILE_ROWS = HITS_TILE_WORDS * HITS_ROWS_PER_WORD;

// mask words (and word prefixes) of a window of n bases: C(n) must have a word
__host__ __device__ __forceinline__ u64 hits_mask_words(u64 n) { return n / HITS_ROWS_PER_WORD + 1; }
__host__ __device__ __forceinline__ u64 hits_tiles(u64 n) { return (hits_mask_words(n) + HITS_TILE_WORDS - 1) / HITS_TILE_WORDS; }
// stream rows of the window that exist at all: rows [0, n - k]; a sequence's own rows are among them
__host__ __device__ __forceinline__ u64 hits_stream_rows(u64 n, int k) { return n >= (u64)k ? n - (u64)k + 1 : 0; }
// rows of one sequence of len bases: the 64-bit restatement of dna.c:781
__host__ __device__ __forceinline__ u64 hits_seq_rows(u64 len, int k) { return len >= (u64)k ? len - (u64)k + 1 : 0; }

// where mask word w reads the packed stream and the marks: word index and the shift inside it (bases)
struct HitsWordAt {
    u64 stream_word;
    u32 fo;                                                // a0 % 32, the same for every word of the window
};
__host__ __device__ __forceinline__ HitsWordAt hits_word_at(u64 a0, u64 w)
{
    return HitsWordAt{(a0 >> 5) + w, (u32)(a0 & 31)};
}
// the bits of mask word w that are rows of the window's stream (rows = hits_stream_rows): the last word is partial
__host__ __device__ __forceinline__ u32 hits_word_valid(u64 rows, u64 w)
{
    const u64 r0 = w * HITS_ROWS_PER_WORD;
    if (r0 >= rows)
        return 0u;
    const u64 left = rows - r0;
    return left >= HITS_ROWS_PER_WORD ? ~0u : (1u << (u32)left) - 1u;
}

// the three places C(r) is read from
struct HitsAt {
    u64 word;                                              // mask[word], word_pre[word]
    u64 tile;                                              // tile_base[tile]
    u32 low;                                               // the bits of the word that lie before r
};
__host__ __device__ __forceinline__ HitsAt hits_at(u64 r)
{
    HitsAt a;
    a.word = r / HITS_ROWS_PER_WORD;
    a.tile = a.word / HITS_TILE_WORDS;
    a.low = (1u << (u32)(r % HITS_ROWS_PER_WORD)) - 1u;
    return a;
}
__host__ __device__ __forceinline__ u32 hits_popc(u32 x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (u32)__popc(x);
#else
    return (u32)__builtin_popcount(x);
#endif
}
__host__ __device__ __forceinline__ u32 hits_before(const u32 *mask, const u32 *word_pre, const u32 *tile_base, u64 r)
{
    const HitsAt a = hits_at(r);
    return tile_base[a.tile] + word_pre[a.word] + hits_popc(mask[a.word] & a.low);
}

// what select asks of one sequence (both factors of either product are below 2^32: exact in 64 bits)
__host__ __device__ __forceinline__ bool hits_selected(u32 rows, u32 hits, u64 min_hits, u64 max_hits, u64 frac_num, u64 frac_den)
{
    return hits >= min_hits && hits <= max_hits && (u64)hits * frac_den >= frac_num * (u64)rows;
}

}  // namespace dnagpu
