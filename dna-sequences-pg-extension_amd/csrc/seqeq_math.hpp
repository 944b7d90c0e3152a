// seqeq_math.hpp -- the arithmetic of sequence equality (dnagpu_dna_equals, dnagpu_table_classes, dnagpu_table_match; DESIGN.md
// 4.18), shared by the kernels (seqeq_kernels.hip), the host driver (seqeq_host.hip) and the host check
// tests/host/seqeq_math_check.cpp: the two sequence classes and the items of the long one, the realigned word of a sequence,
// and the fingerprint.
//
// A sequence of at most SEQEQ_WAVE_BASES bases (the SHORT class) is fingerprinted, and compared, whole by a group of
// SEQEQ_GROUP lanes of a wave -- eight sequences per wave -- lane g of the group taking words g, g + 8, ...  A longer one (the
// LONG class) is cut into items of SEQEQ_TILE_BASES bases = SEQEQ_TILE_WORDS realigned words, one workgroup each; item t
// holds the sequence's words [t * SEQEQ_TILE_WORDS, min(words, (t + 1) * SEQEQ_TILE_WORDS)).  Item -> sequence is
// profile_math.hpp's profile_item_seq over the scanned item counts.
#pragma once
#include "profile_math.hpp"

namespace dnagpu {

constexpr int SEQEQ_GROUP = 8;                             // lanes that share one short sequence
constexpr u64 SEQEQ_WAVE_BASES = 2048;                     // 64 words: eight per lane of a group
constexpr u64 SEQEQ_TILE_WORDS = 2048;                     // an item: 256 threads x 8 words
constexpr u64 SEQEQ_TILE_BASES = 32 * SEQEQ_TILE_WORDS;
static_assert(0 < SEQEQ_WAVE_BASES && SEQEQ_WAVE_BASES < SEQEQ_TILE_BASES && SEQEQ_TILE_BASES <= ((u64)1 << 20) &&
                  SEQEQ_TILE_BASES % 32 == 0,
              "the two classes, and whole words per item");

__host__ __device__ __forceinline__ u64 seqeq_words(u64 len) { return (len + 31) / 32; }
__host__ __device__ __forceinline__ bool seqeq_is_long(u64 len) { return len > SEQEQ_WAVE_BASES; }
// items of a sequence of len bases: 0 for the short class
__host__ __device__ __forceinline__ u64 seqeq_items(u64 len)
{
    return seqeq_is_long(len) ? (len + SEQEQ_TILE_BASES - 1) / SEQEQ_TILE_BASES : 0;
}
// the realigned words [*w0, *w1) of item `item` of a sequence of len bases
__host__ __device__ __forceinline__ void seqeq_item_words(u64 len, u64 item, u64 *w0, u64 *w1)
{
    const u64 nw = seqeq_words(len);
    *w0 = item * SEQEQ_TILE_WORDS;
    *w1 = nw - *w0 < SEQEQ_TILE_WORDS ? nw : *w0 + SEQEQ_TILE_WORDS;
}

// Realigned word j (j < seqeq_words(len)) of the sequence of len bases that starts at base `start` of the stream: its bases
// [32 j, 32 j + 32) at bits 0 .. 63, the bits behind the sequence's last base zero.  It comes from stream word (start + 32 j)
// / 32 and the one after it; the second is read only if it holds a base of this sequence, and never at or beyond n_words.
__host__ __device__ __forceinline__ u64 seqeq_word(const u64 *words, u64 n_words, u64 start, u64 len, u64 j)
{
    const u64 p = start + 32 * j;                          // the word's first base in the stream
    const u64 wi = p >> 5;
    const unsigned off = (unsigned)(p & 31);               // bases of stream word wi in front of it
    const u64 rem = len - 32 * j;
    const unsigned nb = rem < 32 ? (unsigned)rem : 32u;    // bases of this word: 1 .. 32
    u64 v = words[wi] >> (2 * off);
    if (off != 0 && nb > 32 - off && wi + 1 < n_words)
        v |= words[wi + 1] << (64 - 2 * off);
    return nb < 32 ? v & (((u64)1 << (2 * nb)) - 1) : v;
}

// ---- the fingerprint: a function of (length, bases) alone, fp = seqeq_fp_length(len) + the wrapping sum over j of
// seqeq_fp_word(realigned word j, j).  A sum, so the items of a long sequence add their partial sums in any order.  Every
// word counts, a word of 32 A's (0) too: splitmix64 of a per-index constant.
__host__ __device__ __forceinline__ u64 seqeq_fp_word(u64 word, u64 j)
{
    return splitmix64(word ^ splitmix64(j * 0xD6E8FEB86659FD93ull + 0x2545F4914F6CDD1Dull));
}
__host__ __device__ __forceinline__ u64 seqeq_fp_length(u64 len) { return splitmix64(len ^ 0x6a09e667f3bcc909ull); }
// the partial sum of the realigned words [w0, w1)
__host__ __device__ __forceinline__ u64 seqeq_fp_part(const u64 *words, u64 n_words, u64 start, u64 len, u64 w0, u64 w1)
{
    u64 s = 0;
    for (u64 j = w0; j < w1; j++)
        s += seqeq_fp_word(seqeq_word(words, n_words, start, len, j), j);
    return s;
}
__host__ __device__ __forceinline__ u64 seqeq_fingerprint(const u64 *words, u64 n_words, u64 start, u64 len)
{
    return seqeq_fp_length(len) + seqeq_fp_part(words, n_words, start, len, 0, seqeq_words(len));
}
// DNAGPU_DEBUG_WEAK_FINGERPRINT keeps these bits of every fingerprint
constexpr u64 SEQEQ_WEAK_MASK = 3;

}  // namespace dnagpu
