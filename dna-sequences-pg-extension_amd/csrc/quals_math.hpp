// quals_math.hpp -- what the kernels of the quality column (quals_kernels.hip), its host driver (quals_host.hip) and the host
// check tests/host/quals_math_check.cpp share: the class of a quality byte, the error word, the sixteen
// bytes one lane forms at a time, and their assembly from the pieces of the segments that lie under them.
//
// A quality column has one byte per base of a table's stream: byte b is the raw Phred+33 character of base b.  Every way a
// column is made -- from a FASTQ text, from another column by take / gather -- is the same copy: a list of n segments,
// segment i = the bytes [src_at[i], src_at[i] + len_i) of a source (read backwards when flip[i] != 0: qualities have no
// complement), laid back to back; out_starts[0 .. n] is the exclusive scan of the lengths and out_starts[n] = total.  The
// output is formed in chunks of QUALS_CHUNK bytes, aligned in the column: the non-empty segments under a chunk are its pieces.
#pragma once
#include "kmer_device.hpp"

namespace dnagpu {

constexpr u32 QUALS_THREADS = 256;
constexpr u32 QUALS_CHUNK = 16;                  // bytes one lane forms at a time: one uint4 store
constexpr u32 QUALS_TILE_BYTES = QUALS_THREADS * QUALS_CHUNK;
constexpr u32 QUALS_LDS_SEGS = 1024;             // most segments of a tile whose starts, sources and flags the copy holds in LDS

__host__ __device__ __forceinline__ u64 quals_chunks(u64 total) { return (total + QUALS_CHUNK - 1) / QUALS_CHUNK; }
__host__ __device__ __forceinline__ u64 quals_tiles(u64 total) { return (total + QUALS_TILE_BYTES - 1) / QUALS_TILE_BYTES; }
// bytes of the allocation behind a column of `total` bytes: whole chunks, so that every lane stores its chunk whole
__host__ __device__ __forceinline__ u64 quals_alloc_bytes(u64 total) { return total ? quals_chunks(total) * QUALS_CHUNK : QUALS_CHUNK; }

// a Phred+33 character: '!' .. '~'
__host__ __device__ __forceinline__ bool quals_valid(u32 byte) { return byte >= 33 && byte <= 126; }

// ---- the error word: (byte offset << 2) | kind, as text_error_key: a 64-bit minimum keeps the error with the lowest
// offset.  At one offset a length error comes before a character error (the quality line's first byte can carry both).
constexpr u64 QUALS_NO_ERROR = ~(u64)0;
constexpr u32 QUALS_ERR_LENGTH = 0;      // a quality line whose length differs from its sequence line's
constexpr u32 QUALS_ERR_CHAR = 1;        // a byte outside 33 .. 126 in a quality line
constexpr u32 QUALS_ERR_TRUNC = 3;       // the lines are no multiple of four (TEXT_ERR_TRUNC)
__host__ __device__ __forceinline__ u64 quals_error_key(u64 pos, u32 kind) { return (pos << 2) | kind; }
__host__ __device__ __forceinline__ u64 quals_error_pos(u64 key) { return key >> 2; }
__host__ __device__ __forceinline__ u32 quals_error_kind(u64 key) { return (u32)(key & 3); }

// ---- FASTQ: the four words of a record.  A line's end is the offset of its '\n', or n for a last line without one; its
// length is taken without the terminator, and a '\r' directly before the '\n' belongs to the terminator.
constexpr u32 QUALS_REC_WORDS = 4;       // start and end of the sequence line, start and end of the quality line
template <typename Byte>
__host__ __device__ __forceinline__ u32 quals_line_len(u32 start, u32 end, u64 n, Byte &&byte)
{
    if (end < n && end > start && byte(end - 1) == '\r')
        end--;
    return end - start;
}

// ---- sixteen bytes, byte k at bits 8 (k mod 8) of lo (k < 8) or hi
struct QualsBytes {
    u64 lo, hi;
};
__host__ __device__ __forceinline__ void quals_put(QualsBytes &v, u32 k, u32 byte)
{
    if (k < 8)
        v.lo |= (u64)byte << (8 * k);
    else
        v.hi |= (u64)byte << (8 * (k - 8));
}
__host__ __device__ __forceinline__ u32 quals_get(const QualsBytes &v, u32 k)
{
    return (u32)((k < 8 ? v.lo >> (8 * k) : v.hi >> (8 * (k - 8))) & 0xff);
}
__host__ __device__ __forceinline__ u64 quals_swap64(u64 x)
{
    x = ((x & 0x00FF00FF00FF00FFull) << 8) | ((x >> 8) & 0x00FF00FF00FF00FFull);
    x = ((x & 0x0000FFFF0000FFFFull) << 16) | ((x >> 16) & 0x0000FFFF0000FFFFull);
    return (x << 32) | (x >> 32);
}
// the sixteen bytes in reverse order
__host__ __device__ __forceinline__ QualsBytes quals_reverse(const QualsBytes &v)
{
    QualsBytes r;
    r.lo = quals_swap64(v.hi);
    r.hi = quals_swap64(v.lo);
    return r;
}
// sixteen bytes that begin `mis` bytes (0 .. 3) into the five little-endian 32-bit words d[0 .. 5) (d[4] is not looked at
// when mis == 0)
__host__ __device__ __forceinline__ QualsBytes quals_from_words(const u32 d[5], u32 mis)
{
    const u32 sh = 8 * mis;
    u32 w[4];
#pragma unroll
    for (u32 i = 0; i < 4; i++)
        w[i] = sh ? (d[i] >> sh) | (d[i + 1] << (32 - sh)) : d[i];
    QualsBytes v;
    v.lo = (u64)w[0] | ((u64)w[1] << 32);
    v.hi = (u64)w[2] | ((u64)w[3] << 32);
    return v;
}

// the source byte of byte `off` of a segment of len bytes at source byte `at`
__host__ __device__ __forceinline__ u64 quals_source(u64 at, u64 len, bool flip, u64 off)
{
    return flip ? at + len - 1 - off : at + off;
}

// Chunk c (c < quals_chunks(total)) of the output, assembled from its pieces.  seg = any segment with out_starts[seg] <=
// 16 c that is not behind the chunk's first piece (take_segment_of gives the piece's own).  load(i) = source byte i, asked
// only for bytes of a piece; whole(a, flip, &v) may form a piece that fills the chunk -- the sixteen source bytes from a on,
// reversed when flip -- at once and return true, or return false and leave it to load.  Bytes behind the last byte of the
// output are zero.
template <typename Load, typename Whole>
__host__ __device__ __forceinline__ QualsBytes quals_chunk(const u64 *out_starts, const u64 *src_at, const uint8_t *flip, u64 total,
                                                           u64 seg, u64 c, Load &&load, Whole &&whole)
{
    const u64 p0 = (u64)QUALS_CHUNK * c;
    const u64 end = p0 + QUALS_CHUNK < total ? p0 + QUALS_CHUNK : total;
    u64 p = p0, s = out_starts[seg];
    QualsBytes v = {0, 0};
    while (p < end) {                                       // (out_starts[n] = total > p: the walk ends inside the list)
        const u64 e = out_starts[seg + 1];
        if (e > p) {                                        // segment seg holds output byte p: the bytes [p, min(e, end))
            const u64 hi = e < end ? e : end;
            const bool f = flip != nullptr && flip[seg] != 0;
            const u64 at = src_at[seg], len = e - s;
            if (hi - p == QUALS_CHUNK && whole(quals_source(at, len, f, f ? hi - 1 - s : p - s), f, &v))
                return v;
            for (u64 q = p; q < hi; q++)
                quals_put(v, (u32)(q - p0), load(quals_source(at, len, f, q - s)));
            p = hi;
        }
        s = e;
        seg++;
    }
    return v;
}

// ================================================================ dnagpu_quals_trim
// The Phred value of a byte is byte - 33.  With Q_i = the sum of the values of a sequence's bases 0 .. i, the running sum of
// the front walk at base i is F (i + 1) - Q_i and that of the tail walk is T (n - i) - (Q_{n-1} - Q_{i-1}): both walks, their
// breaks and their maxima follow from ONE prefix sum of the values.  A team of lanes holds a tile of the sequence, every
// lane one aligned 16-byte chunk of the column; the lane functions below are what a lane does with its chunk, and the
// kernels (and the host check) join the lanes' answers: a scan of the lanes' sums, the first / last lane with a negative
// running sum, the maximum of the lanes' bests.
typedef long long i64;
constexpr i64 QUALS_NONE = 0x7FFFFFFFFFFFFFFFll;     // no negative running sum in a front walk
constexpr u32 QUALS_GROUP_LANES = 16;
// a sequence at any alignment of at most 16 L - 15 bases lies in L aligned chunks
constexpr u32 QUALS_GROUP_BASES = QUALS_CHUNK * QUALS_GROUP_LANES - (QUALS_CHUNK - 1);
constexpr u32 QUALS_WAVE_BASES = QUALS_CHUNK * 64 - (QUALS_CHUNK - 1);
constexpr u32 QUALS_TRIM_TILE_BASES = QUALS_CHUNK * QUALS_THREADS - (QUALS_CHUNK - 1);
constexpr u32 QUALS_MAX_THRESHOLD = 255;             // cut_front, cut_tail, min_mean_q, low_q: a byte's worth

struct QualsTrimOpt {
    u32 cut_front, cut_tail, min_mean_q, low_q;
    u32 low_num, low_den;
    u64 min_bases;
};
// 0: the sequence passes; 1 .. 3: the first criterion it fails, in the order short, mean, low
constexpr u32 QUALS_PASS = 0, QUALS_FAIL_SHORT = 1, QUALS_FAIL_MEAN = 2, QUALS_FAIL_LOW = 3;
__host__ __device__ __forceinline__ u32 quals_verdict(u64 len, u64 qsum, u64 low, const QualsTrimOpt &o)
{
    if (len == 0 || len < o.min_bases)
        return QUALS_FAIL_SHORT;
    if (qsum < (u64)o.min_mean_q * len)
        return QUALS_FAIL_MEAN;
    if (o.low_den != 0 && low * o.low_den > (u64)o.low_num * len)
        return QUALS_FAIL_LOW;
    return QUALS_PASS;
}

// one lane's chunk of a sequence of the column: bytes [k0, k1) of v are the sequence's bases i0 + k0 .. i0 + k1 - 1 (i0 is
// negative in the first chunk of a sequence that does not begin on a chunk)
struct QualsLane {
    QualsBytes v;
    u32 k0, k1;
    i64 i0;
};
// the chunk at column byte 16 c of a sequence of n bases at column byte base; load(c) is asked only when the chunk holds a base
template <typename Load>
__host__ __device__ __forceinline__ QualsLane quals_lane(u64 base, u64 n, u64 c, Load &&load)
{
    QualsLane l;
    l.v.lo = l.v.hi = 0;
    l.k0 = l.k1 = 0;
    const u64 p = c * QUALS_CHUNK;
    l.i0 = (i64)p - (i64)base;
    if (n == 0 || p + QUALS_CHUNK <= base || p >= base + n)
        return l;
    l.v = load(c);
    l.k0 = base > p ? (u32)(base - p) : 0u;
    l.k1 = base + n < p + QUALS_CHUNK ? (u32)(base + n - p) : QUALS_CHUNK;
    return l;
}
__host__ __device__ __forceinline__ u32 quals_phred(const QualsLane &l, u32 k) { return quals_get(l.v, k) - 33; }
__host__ __device__ __forceinline__ u32 quals_lane_sum(const QualsLane &l)
{
    u32 s = 0;
#pragma unroll
    for (u32 k = 0; k < QUALS_CHUNK; k++)
        if (k >= l.k0 && k < l.k1)
            s += quals_phred(l, k);
    return s;
}
// qex: the sum of the values of the sequence's bases before the lane's.  The first base of the lane whose front running sum
// is negative (QUALS_NONE: none)
__host__ __device__ __forceinline__ i64 quals_lane_front_neg(const QualsLane &l, u64 qex, u32 F)
{
    i64 neg = QUALS_NONE;
    u64 q = qex;
#pragma unroll
    for (u32 k = 0; k < QUALS_CHUNK; k++)
        if (k >= l.k0 && k < l.k1) {
            q += quals_phred(l, k);
            const i64 i = l.i0 + k;
            if ((i64)F * (i + 1) - (i64)q < 0 && neg == QUALS_NONE)
                neg = i;
        }
    return neg;
}
// the front walk over the lane's bases before `limit`: a running sum above *bestv becomes *bestv, its base *besti (the
// later base does not replace an equal best)
__host__ __device__ __forceinline__ void quals_lane_front_best(const QualsLane &l, u64 qex, u32 F, i64 limit, i64 *bestv, i64 *besti)
{
    u64 q = qex;
#pragma unroll
    for (u32 k = 0; k < QUALS_CHUNK; k++)
        if (k >= l.k0 && k < l.k1) {
            q += quals_phred(l, k);
            const i64 i = l.i0 + k, s = (i64)F * (i + 1) - (i64)q;
            if (i < limit && s > *bestv) {
                *bestv = s;
                *besti = i;
            }
        }
}
// qtot: the sum over the whole sequence.  The last base of the lane whose tail running sum is negative (-1: none)
__host__ __device__ __forceinline__ i64 quals_lane_tail_neg(const QualsLane &l, u64 qex, u64 qtot, u64 n, u32 T)
{
    i64 neg = -1;
    u64 q = qex;                                     // (the values before base i)
#pragma unroll
    for (u32 k = 0; k < QUALS_CHUNK; k++)
        if (k >= l.k0 && k < l.k1) {
            const i64 i = l.i0 + k;
            if ((i64)T * ((i64)n - i) - (i64)(qtot - q) < 0)
                neg = i;
            q += quals_phred(l, k);
        }
    return neg;
}
// the tail walk over the lane's bases behind `limit`, from the last to the first (of equal bests the first met, the later
// base, stays)
__host__ __device__ __forceinline__ void quals_lane_tail_best(const QualsLane &l, u64 qex, u64 qtot, u64 n, u32 T, i64 limit, i64 *bestv,
                                                              i64 *besti)
{
    u64 q = qex + quals_lane_sum(l);                 // (the values up to and including base i)
#pragma unroll
    for (u32 kk = 0; kk < QUALS_CHUNK; kk++) {
        const u32 k = QUALS_CHUNK - 1 - kk;
        if (k >= l.k0 && k < l.k1) {
            const i64 i = l.i0 + k;
            q -= quals_phred(l, k);
            const i64 s = (i64)T * ((i64)n - i) - (i64)(qtot - q);
            if (i > limit && s > *bestv) {
                *bestv = s;
                *besti = i;
            }
        }
    }
}
// the lane's bases in [start, stop): *qsum += their values, *low += those below low_q
__host__ __device__ __forceinline__ void quals_lane_range(const QualsLane &l, i64 start, i64 stop, u32 low_q, u64 *qsum, u64 *low)
{
#pragma unroll
    for (u32 k = 0; k < QUALS_CHUNK; k++)
        if (k >= l.k0 && k < l.k1) {
            const i64 i = l.i0 + k;
            if (i >= start && i < stop) {
                const u32 v = quals_phred(l, k);
                *qsum += v;
                *low += v < low_q;
            }
        }
}

}  // namespace dnagpu
