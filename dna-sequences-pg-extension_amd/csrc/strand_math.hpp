// strand_math.hpp -- the arithmetic of strand-neutral k-mers, shared by the kernels (strand_kernels.hip, the
// canonical add of acc_kernels.hip) and the host check tests/host/strand_math_check.cpp: the reverse complement of a key
// and of one packed word, and the canonical form of a key.
//
// Codes are the reference's, A = 00, T = 01, C = 10, G = 11: the complement of a base is code ^ 1.
// The canonical form of a k-mer is whichever of key and rc(key) comes first in the index order of index_math.hpp: text
// order under A < T < C < G with base 0 most significant.  This is NOT the conventional A < C < G < T.
#pragma once
#include "index_math.hpp"

namespace dnagpu {

constexpr u64 STRAND_COMPLEMENT = 0x5555555555555555ull;    // bit 0 of every field

// rc(key, k): base i of the result is the complement of base k - 1 - i of key.  Bits of key above 2k are dropped.
__host__ __device__ __forceinline__ u64 kmer_revcomp(u64 key, int k)
{
    return index_r_of_key(key, k) ^ (STRAND_COMPLEMENT & kmer_mask(k));
}

// With r = index_r_of_key(key, k) and M = 0x5555... & kmer_mask(k): rc(key) = r ^ M, and the index rank of rc(key) -- its
// fields reversed once more -- is key ^ M.  So key comes first, or is its own reverse complement, exactly when
// r <= key ^ M: one reversal serves both the test and the result.  key == rc(key) happens only at even k; such a key is
// canonical.
__host__ __device__ __forceinline__ bool kmer_is_canonical(u64 key, int k)
{
    const u64 mask = kmer_mask(k);
    return index_r_of_key(key, k) <= ((key & mask) ^ (STRAND_COMPLEMENT & mask));
}

// the canonical form of key (masked to 2k bits); *flipped = it is rc(key) and differs from key
__host__ __device__ __forceinline__ u64 kmer_canonical(u64 key, int k, bool *flipped)
{
    const u64 mask = kmer_mask(k), m = STRAND_COMPLEMENT & mask;
    const u64 r = index_r_of_key(key, k);
    key &= mask;
    *flipped = r > (key ^ m);
    return *flipped ? r ^ m : key;
}
__host__ __device__ __forceinline__ u64 kmer_canonical(u64 key, int k)
{
    bool flipped;
    return kmer_canonical(key, k, &flipped);
}

// the 32 bases of one packed word reverse-complemented: base i of the result is the complement of base 31 - i
__host__ __device__ __forceinline__ u64 word_revcomp(u64 w)
{
    return rev2(w) ^ STRAND_COMPLEMENT;
}

// ---- the reverse complement of bases [first, first + count) of a packed stream, output word by output word.
// Output word j holds nb = min(32, count - 32 j) bases, the complements of input bases q .. q + nb - 1 read backwards,
// q = first + count - 32 j - nb: always inside the window, so the last (short) output word starts at `first` and not
// before it.  The nb bases start at bit 2 (q mod 32) of word q / 32 and reach into the next word only when
// (q mod 32) + nb > 32; nothing else is read.
struct RevcompSource {
    u64 word;          // q / 32
    unsigned shift;    // 2 (q mod 32)
    unsigned nb;       // 1 .. 32
    bool two_words;
};
__host__ __device__ __forceinline__ RevcompSource revcomp_source(u64 first, u64 count, u64 j)
{
    const u64 left = count - 32 * j;
    RevcompSource s;
    s.nb = left < 32 ? (unsigned)left : 32u;
    const u64 q = first + left - s.nb;
    s.word = q >> 5;
    s.shift = (unsigned)(q & 31) * 2;
    s.two_words = (q & 31) + s.nb > 32;
    return s;
}
// w = the 64 bits at bit `shift` of the two source words (whatever lies behind the nb bases is pushed out here, so the
// result never depends on it); bits behind the last base of the result are zero
__host__ __device__ __forceinline__ u64 revcomp_finish(u64 w, unsigned nb)
{
    return word_revcomp(w << (2 * (32 - nb))) & kmer_mask((int)nb);
}

}  // namespace dnagpu
