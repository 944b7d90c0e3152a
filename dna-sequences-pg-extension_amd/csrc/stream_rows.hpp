// stream_rows.hpp -- how a thread of a stream sweep reads its 32 consecutive rows (filter_kernels.hip, hits_kernels.hip): the
// packed words under them, the 64 bases that start at the thread's first row, and -- over a TABLE of sequences -- the mask
// of the rows that reach across a sequence start, from the resident marks.  Device code only.
#pragma once
#include "kmer_device.hpp"

namespace dnagpu {

// the 64 bases starting at stream word w (+ a wave-uniform shift of sh = 2 * (first % 32) bits) as 4 dwords
struct Stream4 {
    u32 d[4];
};
struct Words3 {
    u64 w0, w1, w2;
};

__device__ __forceinline__ Words3 words_load(const u64 *__restrict__ words, u64 n_words, u64 w, unsigned sh)
{
    Words3 r;
    r.w0 = w < n_words ? words[w] : 0;
    r.w1 = w + 1 < n_words ? words[w + 1] : 0;
    r.w2 = (sh && w + 2 < n_words) ? words[w + 2] : 0;
    return r;
}

__device__ __forceinline__ Stream4 stream_of(const Words3 &r, unsigned sh)
{
    u64 lo = r.w0, hi = r.w1;
    if (sh) {                                        // wave-uniform
        lo = (r.w0 >> sh) | (r.w1 << (64 - sh));
        hi = (r.w1 >> sh) | (r.w2 << (64 - sh));
    }
    Stream4 s;
    s.d[0] = (u32)lo;
    s.d[1] = (u32)(lo >> 32);
    s.d[2] = (u32)hi;
    s.d[3] = (u32)(hi >> 32);
    return s;
}

// ---- the rows of a TABLE of sequences (dnagpu_generate_kmers_table, dnagpu_table_hits) -----------
// A stream row is a table row when no sequence starts among the k - 1 bases behind its first base (batch_keys_kernel's
// rule).  For a thread's 32 rows that is one bit-sliced mask from the resident marks; it is ANDed into the match mask, so
// a row that reaches across a boundary is never counted, listed or looked up.

// the mark words under the 62 bases behind a thread's first row (mw = the word of that row's base)
struct Marks3 {
    u32 m0 = 0, m1 = 0, m2 = 0;
};

__device__ __forceinline__ Marks3 marks_load(const u32 *__restrict__ marks, u64 n_mark_words, u64 mw, u32 fo)
{
    Marks3 r;
    r.m0 = mw < n_mark_words ? marks[mw] : 0u;
    r.m1 = mw + 1 < n_mark_words ? marks[mw + 1] : 0u;
    r.m2 = (fo && mw + 2 < n_mark_words) ? marks[mw + 2] : 0u;      // bits fo + 1 .. fo + 62 end in the third word
    return r;
}

// bit j = row j of the thread's 32 reaches across a sequence start.  M = the marks of bases p0 + 1 .. p0 + 62 (p0 = the
// thread's first row); row j is spoiled when any of M's bits j .. j + span - 1 is set (span = k - 1 <= 31): M ORed with
// shifted copies of itself, the covered width doubling, then one shift for the rest.
__device__ __forceinline__ u32 spoiled_rows(const Marks3 &r, u32 fo, u32 span)
{
    if (span == 0)                                   // k = 1: a row is one base
        return 0u;
    const unsigned sh = fo + 1u;                     // 1 .. 32
    u64 M = ((((u64)r.m1 << 32) | r.m0) >> sh) | ((u64)r.m2 << (64u - sh));
    u32 c = 1;
    for (; 2u * c <= span; c *= 2u)                  // wave-uniform, at most four rounds
        M |= M >> c;
    M |= M >> (span - c);                            // span - c < c: no gap
    return (u32)M;
}

}  // namespace dnagpu
