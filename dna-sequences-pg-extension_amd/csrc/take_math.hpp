// take_math.hpp -- the piece arithmetic of dnagpu_dna_gather / dnagpu_dna_take, shared by the sweep
// (take_kernels.hip), the host driver (take_host.hip) and the host check tests/host/take_math_check.cpp.
//
// A gather is a list of n segments of a packed source stream, segment i = the len[i] bases at source base first[i], reverse-
// complemented when flip[i] != 0, laid back to back into an output stream: out_starts[0 .. n] is the exclusive scan of the
// lengths, out_starts[n] = total.  The output is formed word by word.  The non-empty segments that intersect the 32 bases of
// output word w are its PIECES: a piece is nb <= 32 consecutive bases of one segment, nb consecutive bases of the source
// (read backwards when the segment is flipped), and so at most two neighbouring source words.
#pragma once
#include "strand_math.hpp"

namespace dnagpu {

constexpr u32 TAKE_THREADS = 256;
constexpr u32 TAKE_WORDS_PER_THREAD = 4;
constexpr u32 TAKE_TILE_WORDS = TAKE_THREADS * TAKE_WORDS_PER_THREAD;      // output words of one workgroup of the sweep
constexpr u32 TAKE_LDS_SEGS = 1024;       // most segments of a tile whose starts, source bases and flags the sweep holds in LDS

__host__ __device__ __forceinline__ u64 take_words(u64 total) { return (total + 31) / 32; }
__host__ __device__ __forceinline__ u64 take_tiles(u64 n_words) { return (n_words + TAKE_TILE_WORDS - 1) / TAKE_TILE_WORDS; }

// what the validation pass adds to the 64-bit total for one segment: no more than 2^32, so that 2^32 - 1 segments cannot
// wrap the sum, and any length that alone passes the limit of a result still puts the total above it
__host__ __device__ __forceinline__ u64 take_len_clamped(u64 len) { return len > ((u64)1 << 32) ? (u64)1 << 32 : len; }

// The last segment i of [lo, hi] with out_starts[i] <= p (out_starts[lo] <= p is the caller's): of a run of equal starts --
// empty segments -- only the last has bases, and that is the one an upper bound minus one finds.
__host__ __device__ __forceinline__ u64 take_segment_of(const u64 *out_starts, u64 lo, u64 hi, u64 p)
{
    while (lo < hi) {
        const u64 mid = lo + (hi - lo + 1) / 2;
        if (out_starts[mid] <= p)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// One piece: nb bases (1 .. 32) at offset `off` of a segment (first, len, flip), to be placed at base `at` (0 .. 31) of its
// output word.  A forward piece is source bases [first + off, first + off + nb); a flipped one is the reverse complement of
// [first + len - off - nb, first + len - off) (dnagpu_dna_revcomp's definition applied to the segment).  Either way the nb
// bases start at bit `shift` of source word `word` and reach into word + 1 only when two_words -- that word then exists,
// because the piece's last base lies in it.
struct TakePiece {
    u64 word;
    unsigned shift;        // 2 (q mod 32), q = the piece's first source base
    unsigned nb;
    unsigned dst;          // 2 at
    bool two_words;
    bool flip;
};
__host__ __device__ __forceinline__ TakePiece take_piece(u64 first, u64 len, bool flip, u64 off, unsigned nb, unsigned at)
{
    const u64 q = flip ? first + len - off - nb : first + off;
    const RevcompSource s = revcomp_source(q, nb, 0);       // (the window of nb bases at q as ONE output word: word, shift, reach)
    TakePiece pc;
    pc.word = s.word;
    pc.shift = s.shift;
    pc.nb = nb;
    pc.dst = 2 * at;
    pc.two_words = s.two_words;
    pc.flip = flip;
    return pc;
}
// bits = the 64 bits at bit `shift` of the piece's two source words (funnel): masked to the piece's bases -- whatever lies
// behind them, bits behind the source's last base included, never reaches the result -- and shifted to its place
__host__ __device__ __forceinline__ u64 take_piece_bits(const TakePiece &pc, u64 bits)
{
    const u64 v = pc.flip ? revcomp_finish(bits, pc.nb) : bits & kmer_mask((int)pc.nb);
    return v << pc.dst;
}

// Output word w (w < take_words(total)), assembled from its pieces.  seg = any segment with out_starts[seg] <= 32 w that is
// not behind the word's first piece (take_segment_of gives the piece's own); load(i) = source word i, asked only for words
// that hold a base of a piece.  Bits behind the last base of the output are zero.
template <typename Load>
__host__ __device__ __forceinline__ u64 take_word(const u64 *out_starts, const u64 *first, const uint8_t *flip, u64 total, u64 seg,
                                                  u64 w, Load load)
{
    u64 p = 32 * w;
    const u64 end = p + 32 < total ? p + 32 : total;
    u64 s = out_starts[seg], acc = 0;
    while (p < end) {                                       // (out_starts[n] = total > p: the walk ends inside the list)
        const u64 e = out_starts[seg + 1];
        if (e > p) {                                        // segment seg holds output base p: the bases [p, min(e, end))
            const u64 hi = e < end ? e : end;
            const TakePiece pc = take_piece(first[seg], e - s, flip != nullptr && flip[seg] != 0, p - s, (unsigned)(hi - p),
                                            (unsigned)(p - 32 * w));
            const u64 w0 = load(pc.word);
            const u64 w1 = pc.two_words ? load(pc.word + 1) : 0;
            acc |= take_piece_bits(pc, funnel(w0, w1, pc.shift));
            p = hi;
        }
        s = e;
        seg++;
    }
    return acc;
}

}  // namespace dnagpu
