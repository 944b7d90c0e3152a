// adapters_math.hpp -- what the kernels of dnagpu_dna_adapters (adapters_kernels.hip), its host driver (adapters_host.hip) and
// the host check tests/host/adapters_math_check.cpp share: the descriptor of one adapter, the mismatches of
// one 32-base window against it, the hit key, and the sixteen positions one lane walks.
//
// A segment is the n bases [first, first + n) of a packed stream; position p of it is a candidate for the 3' adapter a of
// L_a letters with the overlap o = min(L_a, n - p): the mismatches are the bases b[p + j], j < o, that are not in the set
// S_a[j].  (p, a) is a hit iff o >= min(min_overlap, L_a) and m * err_den <= err_num * o; the segment's cut is the hit with
// the least (p, m, a).  Hamming distance only.
#pragma once
#include "kmer_device.hpp"

namespace dnagpu {

constexpr u32 ADAPTERS_MAX = 32;                 // adapters of one call, and letters of one adapter
constexpr u32 ADAPTERS_THREADS = 256;
constexpr u32 ADAPTERS_LANE_POS = 16;            // consecutive positions one lane owns
constexpr u32 ADAPTERS_GROUP_LANES = 16;
constexpr u32 ADAPTERS_GROUP_BASES = ADAPTERS_LANE_POS * ADAPTERS_GROUP_LANES;       // a group of lanes of one wave
constexpr u32 ADAPTERS_WAVE_BASES = ADAPTERS_LANE_POS * 64;                          // a wave
constexpr u32 ADAPTERS_TILE_BASES = ADAPTERS_LANE_POS * ADAPTERS_THREADS;            // one tile of a workgroup

// One adapter.  deny[c] has bit 2j set where code c (A=0 T=1 C=2 G=3) is NOT in S_a[j] (FilterDev::deny's planes; bits at
// and behind 2 len are zero); thr[o] = the most mismatches a hit of overlap o may have, -1 where o is below the effective
// min_overlap: built on the host from the rational, so that the device never divides.
struct AdapterDesc {
    u64 deny[4];
    u32 len;
    int8_t thr[ADAPTERS_MAX + 1];
    int8_t pad[3];
};
static_assert(sizeof(AdapterDesc) % 8 == 0, "an array of descriptors is copied as 8-byte words");

// sets[j] = S_a[j] as a 4-bit mask over the codes (bit c = code c allowed); 1 <= len <= 32, err_den >= 1, err_num <= err_den
__host__ __device__ inline void adapter_build(const int *sets, u32 len, u32 err_num, u32 err_den, u32 min_overlap, AdapterDesc *d)
{
    for (int c = 0; c < 4; c++)
        d->deny[c] = 0;
    for (u32 j = 0; j < len; j++)
        for (int c = 0; c < 4; c++)
            if (!(sets[j] & (1 << c)))
                d->deny[c] |= (u64)1 << (2 * j);
    d->len = len;
    const u32 need = min_overlap < len ? min_overlap : len;
    for (u32 o = 0; o <= ADAPTERS_MAX; o++)
        d->thr[o] = o < need || o > len ? (int8_t)-1 : (int8_t)(((u64)err_num * o) / err_den);
    d->pad[0] = d->pad[1] = d->pad[2] = 0;
}

// ---- one window: the 32 bases from a position on, base j at bits 2j.  The four planes hold bit 2j where base j is that code
// (filter_match's split); they are formed once per position and serve every adapter.
struct AdapterPlanes {
    u64 is[4];
};
__host__ __device__ __forceinline__ AdapterPlanes adapter_planes(u64 window)
{
    const u64 EVEN = 0x5555555555555555ull;
    const u64 lo = window & EVEN, hi = (window >> 1) & EVEN;
    AdapterPlanes p;
    p.is[0] = ~(lo | hi) & EVEN;
    p.is[1] = lo & ~hi;
    p.is[2] = hi & ~lo;
    p.is[3] = lo & hi;
    return p;
}
// the mismatches among the window's first o bases (o <= the adapter's length)
__host__ __device__ __forceinline__ u32 adapter_mismatches(const AdapterPlanes &p, const u64 deny[4], u32 o)
{
    const u64 bad = ((p.is[0] & deny[0]) | (p.is[1] & deny[1]) | (p.is[2] & deny[2]) | (p.is[3] & deny[3])) & kmer_mask((int)o);
    return (u32)__builtin_popcountll(bad);
}

// ---- the hit key: (p, m, a) in one integer, so that a minimum is the whole rule.  p < 2^32, m <= 32, a < 32.
constexpr u64 ADAPTERS_NONE = ~(u64)0;
__host__ __device__ __forceinline__ u64 adapter_key(u64 p, u32 m, u32 a) { return (p << 11) | ((u64)m << 5) | a; }
__host__ __device__ __forceinline__ u64 adapter_key_pos(u64 key) { return key >> 11; }
__host__ __device__ __forceinline__ u32 adapter_key_mismatch(u64 key) { return (u32)(key >> 5) & 63; }
__host__ __device__ __forceinline__ u32 adapter_key_adapter(u64 key) { return (u32)key & 31; }

// ---- one lane: the least key among the positions [p0, p0 + ADAPTERS_LANE_POS) of the segment (first, n), or
// ADAPTERS_NONE.  word(w) = word w of the stream; only words that hold a base of the segment are asked for -- the two or
// three that hold the lane's 47 bases, once -- and the window then slides by a funnel shift per position.  Bits of bases
// behind the segment's end may lie in the last word: the mask of the overlap keeps them out of every count.
template <typename Word>
__host__ __device__ __forceinline__ u64 adapter_lane_best(Word &&word, u64 first, u64 n, u64 p0, const AdapterDesc *ads, u32 n_ads)
{
    if (p0 >= n)
        return ADAPTERS_NONE;
    const u64 b0 = first + p0, w0 = b0 >> 5, w_last = (first + n - 1) >> 5;
    u32 s = (u32)(b0 & 31);
    u64 lo = word(w0), hi = w0 + 1 <= w_last ? word(w0 + 1) : 0, next = w0 + 2 <= w_last ? word(w0 + 2) : 0;
    const u32 count = n - p0 < ADAPTERS_LANE_POS ? (u32)(n - p0) : ADAPTERS_LANE_POS;
    u64 best = ADAPTERS_NONE;
    for (u32 j = 0; j < count; j++) {
        const AdapterPlanes pl = adapter_planes(funnel(lo, hi, 2 * s));
        const u64 left = n - (p0 + j);
        for (u32 a = 0; a < n_ads; a++) {
            const u32 len = ads[a].len, o = left < len ? (u32)left : len;
            const u32 m = adapter_mismatches(pl, ads[a].deny, o);
            if ((int)m <= (int)ads[a].thr[o]) {
                const u64 key = adapter_key(p0 + j, m, a);
                best = key < best ? key : best;
            }
        }
        if (best != ADAPTERS_NONE)
            break;                                   // (the lowest position wins: nothing behind it can)
        if (++s == 32) {
            s = 0;
            lo = hi;
            hi = next;
            next = 0;
        }
    }
    return best;
}

// ---- the verdict of one segment of n bases whose cut is key
constexpr u32 ADAPTERS_PASS = 0, ADAPTERS_FAIL_SHORT = 1, ADAPTERS_FAIL_DISCARDED = 2;
constexpr u32 ADAPTERS_FLAG_UNTRIMMED = 1, ADAPTERS_FLAG_TRIMMED = 2;      // DNAGPU_ADAPTERS_DISCARD_*
__host__ __device__ __forceinline__ u64 adapter_kept(u64 key, u64 n) { return key == ADAPTERS_NONE ? n : adapter_key_pos(key); }
__host__ __device__ __forceinline__ u32 adapter_verdict(u64 key, u64 n, u64 min_bases, u32 flags)
{
    const u64 kept = adapter_kept(key, n);
    if (kept == 0 || kept < min_bases)
        return ADAPTERS_FAIL_SHORT;
    const bool hit = key != ADAPTERS_NONE;
    if ((hit && (flags & ADAPTERS_FLAG_TRIMMED)) || (!hit && (flags & ADAPTERS_FLAG_UNTRIMMED)))
        return ADAPTERS_FAIL_DISCARDED;
    return ADAPTERS_PASS;
}

}  // namespace dnagpu
