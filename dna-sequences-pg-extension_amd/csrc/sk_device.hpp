// sk_device.hpp -- GROUP BY kmer, count(*) for long k-mers through super-k-mer (minimizer) partitioning.
//
// The MSD radix tree of count_kernels.hip moves every 8-byte key through two partition passes
// (3.5x the algorithmic traffic at 3 Gbase).  Here the partition passes move PACKED RUNS instead:
//
//   minimizer  of a k-mer = the m-mer (m = 15) among its w = k - m + 1 with the smallest 32-bit hash; a function
//              of the k-mer's content alone, so equal k-mers share it wherever they occur
//   bucket     = three digits (d0 < C0, d1 < 2^b1, d2 < 16) cut from a multiplicative re-mix of that hash
//   record     = a run of consecutive k-mers with the same minimizer hash (on random data 9 k-mers on
//              average, never more than SK_LMAX): 16 bytes = up to 54 bases (108 bits) + length + d1 + d2.
//              A record cut from a PLAIN tile (all of random sequence) is a run of k-mers whose leftmost minimum m-mer is
//              the SAME OCCURRENCE (same hash, same position): at most w k-mers, at most 2k - m bases, and the record
//              carries that m-mer's offset (SK_POS_*); every other record (low-complexity stretches, the partial tiles at
//              a sequence's end) has SK_REC_MULTI set.  sk_count tests records instead of k-mers with this (see there).
//
//   sk_hist0 / sk_scatter0   sweep the packed dna: hashes, window minima, runs -> records scattered
//                            into C0 coarse buckets (1.8 B per k-mer instead of 8).  Long sequences: the scatter sweep
//                            alone, every chunk of rows reserving slabs sized from a sampled histogram (unused slots =
//                            NULL records, bit 63 of the second word, dropped by level 1); the exact pair is the fall-back
//   sk_hist1 / sk_scatter1   records of a coarse bucket -> 2^b1 mid buckets, every record read once; normally without
//                            the histogram: mid buckets are regions sized from their parent, tiles reserve slots from
//                            global cursors (sk_spec_*), the exact level is the fall-back
//   sk_regroup               a mid bucket's records regrouped by d2 (read once): 16 final buckets of ~2,700 k-mers
//   sk_count                 a final bucket counted from its records in an LDS hash table (fingerprint slots); its groups go
//                            to its own output range
//   sk_count_big / sk_big_merge   long final buckets of few distinct keys (repeats): one table per bucket, slices of records
//   sk_slice_kmers / sk_expand_flat   the buckets sk_count does not take (oversize; the heavy buckets of repeats) -> keys;
//                            the ordinary tree takes over at level 2 (skew handling included)
//
// Keys meet their equals because the bucket is a function of the key; which bucket that is never shows in
// the result.  Group order: nodes in bucket order, ascending inside a node -- NOT globally ascending, which
// is why this engine sits behind dnagpu_count_kmers_unordered (PostgreSQL's GROUP BY order is unspecified,
// test.sql:95-104).
//
// This header: what more than one stage uses -- the record layout, the hash and the bucket digits, the wave helpers, the
// rules host and device share.  All of it inline or constexpr.  The stages, each with its launchers at its end:
//   sk_level0_kernels.hip   the dna sweeps: front end, walks, sk_hist0 / sk_scatter0, the slabs (and sk_count_big /
//                           sk_big_merge of the tail: see there for why)
//   sk_level1_kernels.hip   sk_hist1 / sk_sample1 / sk_scatter1, the speculative regions, sk_regroup
//   sk_tail_kernels.hip     the selection of the final buckets, sk_count_clean / sk_count, the buckets that leave the
//                           record path (slices, sk_expand_flat, heavy buckets)
// The helpers here have internal linkage in device code, and the compiler fits each to the calls of ONE translation unit:
// which kernels share a file decides their instructions.  tools/isa_same.py compares two builds function by function.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "kernels.hpp"

namespace dnagpu {

constexpr int SK_NT = 256;                       // threads of a front-end workgroup: four waves, each working tile after tile on its own
constexpr int SKW_ROWS = 63 * 32;                // rows (k-mers) a WAVE tile emits records for: lane 63 only supplies hashes
constexpr int SK_TILE_ROWS = (SK_NT / 64) * SKW_ROWS;   // one round of the workgroup's waves (chunks are cut at multiples of it)
constexpr int SK_MAX_C0 = 256;                   // most coarse buckets (digits of level 0): 2^32 rows need 195
constexpr int SKW_LIST = 768;                    // records of a wave tile listed in LDS (a tile of random bases has ~225 at k = 31, ~400 at k = 21)
// a full tile of at most this many (hash, position) runs is cut into exactly those: 1.7 times what random sequence gives
// (2016 rows in runs of (w + 1) / 2)
__host__ __device__ constexpr u32 sk_plain_max(int w) { return (u32)(2 * SKW_ROWS * 17 / (10 * (w + 1))) < (u32)SKW_LIST ? (u32)(2 * SKW_ROWS * 17 / (10 * (w + 1))) : (u32)SKW_LIST; }

typedef unsigned long long ull2_t __attribute__((ext_vector_type(2)));

// Second word of a record: bases 32..53 (bits 0..43) | (len - 1) << 44 | d1 << 49 | d2 << 59 | bit 63: NULL record.
// Bit 58 (SK_REC_MULTI): the record's k-mers do NOT all have their leftmost minimum m-mer at one place (nothing is known
// about where it is).  Clear: they do, and bits 39..43 (free: such a record has at most 2k - m <= 49 bases, i.e. payload
// bits 0..97 = bits 0..33 of this word) hold that m-mer's offset from the record's first base, 0 .. w - 1 <= 17.
constexpr int SK_REC_MULTI_BIT = 58;
constexpr int SK_POS_SHIFT = 39;                 // (k-mers of the record never reach these bits: consumers mask keys with kmask)
constexpr u32 SK_POS_MASK = 31u;
constexpr u32 SK_GPOS_MASK = 63u;                // low bits of a window minimum: the position of the minimum (see sk_front)

// 32-bit hash of an m-mer value (2 m <= 30 bits; bits above them ignored: t may carry a 16th base): two full-rate 24-bit
// multiplies, t[0..24) C1 + t[24..2m) C2 -- v_mul_u32_u24 + v_mad_u32_u24 behind one v_bfe (round 3's shift / add / xor mix
// took four operations behind a mask: the sweeps of level 0 are bound by VALU issue).  Its top 25 bits order the m-mers
// (sk_front): on random sequence that order makes runs as long as the old one (8.997 k-mers per record at k = 31 against
// 8.995) and the coarse buckets as even (tools/hash_eval2.py).  Not injective on its 25 bits, and it need not be: records
// are compared by their m-mers' VALUES wherever it matters (sk_count_clean, the walks by value).
__device__ __forceinline__ u32 sk_mix_raw(u32 t, u32 hi_bits /* 2 m - 24 */)
{
    return __umul24(t, 0x9E3779u) + __umul24(__builtin_amdgcn_ubfe(t, 24u, hi_bits), 0x85EBCBu);
}
__device__ __forceinline__ u32 sk_mix(u32 v) { return sk_mix_raw(v, 8u); }       // (v < 2^30)

// The three bucket digits of a k-mer, functions of its minimum m-mer (so equal k-mers share them).
//   d0 (coarse, < c0 <= 256) comes from the m-mer's HASH as the window minima carry it (hmin = hash bits 7..31 | 64 |
//   position): the level-0 histogram needs it for every row, and the hash is what a row has.  The minimum of w hashes is
//   small -- its high bits are biased, ~21 bits of it vary -- which is plenty for 256 coarse buckets and far too little for
//   the ~10^6 final ones (tried: final buckets of ~5 hash classes each, a third of them over sk_count's stage).
//   d1 (< 2^b1) and d2 (< 16) therefore come from the m-mer's 30-bit VALUE, which a record's builder cuts from the tile's
//   words at the minimum's position (once per record, not per row).
// v_mul_u32_u24 is a full-rate instruction; the 32-bit multiply of sk_fine_word runs once per record.  (It takes 24 bits
// of each operand: of the 25 hash bits that order the m-mers, bits 7..30 enter d0 and bit 31 does not.)
struct SkDigits {
    u32 d0, d1, d2;
};
__device__ __forceinline__ u32 sk_digit_word(u32 hmin) { return __umul24(hmin >> 7, 0x9E3779u); }
__device__ __forceinline__ u32 sk_digit0(u32 g, u32 c0) { return __umul24(g >> 16, c0) >> 16; }
__device__ __forceinline__ u32 sk_fine_word(u32 v) { return v * 0x9E3779B1u; }
__device__ __forceinline__ SkDigits sk_digits(u32 hmin, u32 v, u32 c0, u32 b1mask)
{
    const u32 f = sk_fine_word(v);
    SkDigits r;
    r.d0 = sk_digit0(sk_digit_word(hmin), c0);
    r.d1 = (f >> 23) & b1mask;
    r.d2 = (f >> 19) & 15u;
    return r;
}
// the window minimum an m-mer of value v makes (its position bits clear): what sk_front computes for it
__device__ __forceinline__ u32 sk_hash_of(u32 v) { return (sk_mix(v) & ~SK_GPOS_MASK) | 64u; }

// timing ablations (results invalid) exist in the diagnostic build (make STAMPS=1) only
#ifdef DNAGPU_STAMPS
#define SK_DBG(bit) ((dbg & (bit)) != 0)
#else
#define SK_DBG(bit) false
#endif
// the launchers' `dbg` argument: DNAGPU_DEBUG_SK in that build, 0 otherwise
inline int sk_dbg()
{
#ifdef DNAGPU_STAMPS
    const char *e = getenv("DNAGPU_DEBUG_SK");
    return e ? atoi(e) : 0;
#else
    return 0;
#endif
}

__device__ __forceinline__ u32 wave_incl_max(u32 x)
{
    int v = (int)x;                               // values are row indices + 1: small and non-negative
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false));
    return (u32)v;
}

// LDS written by one lane and read by another of the same wave: DS operations of a wave execute in program
// order, so only the compiler has to be kept from reordering them
__device__ __forceinline__ void sk_wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lane i <- lane i + 1 (lane 63 <- 0) / lane i <- lane i - 1 (lane 0 <- 0): one VALU operation each
__device__ __forceinline__ u32 wave_next(u32 x) { return (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x130, 0xf, 0xf, false); }   // wave_shl:1
__device__ __forceinline__ u32 wave_prev(u32 x) { return (u32)__builtin_amdgcn_update_dpp(0, (int)x, 0x138, 0xf, 0xf, false); }   // wave_shr:1

// bits [sh, sh + 64) of hi:lo, sh in 0 .. 127
__device__ __forceinline__ u64 sk_shr128(u64 lo, u64 hi, u32 sh)
{
    return sh < 64u ? funnel(lo, hi, sh) : hi >> (sh - 64u);
}

// exclusive scan over lanes 0..15 (one DPP row); lanes >= 16 get garbage
__device__ __forceinline__ u32 row16_excl_scan(u32 x)
{
    int v = (int)x;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
    return (u32)v - x;
}

// {sum of vals[0 .. wave), sum of all n <= 16 values} from one LDS read per lane and a 16-lane DPP scan (instead of a
// loop of n LDS reads in every thread)
__device__ __forceinline__ void sk_wave_prefix16(const u32 *vals, int n, int wave, int lane, u32 &before, u32 &total)
{
    const u32 v = lane < n ? vals[lane] : 0u;
    const u32 ex = row16_excl_scan(v);             // lanes 0..15
    total = (u32)__builtin_amdgcn_readlane((int)(ex + v), 15);
    before = (u32)__builtin_amdgcn_readlane((int)ex, wave < 16 ? wave : 15);
}

// floor(sqrt(v)): the standard deviations in the slack of sampled estimates (level 0's slabs, level 1's sampled regions)
__host__ __device__ inline u32 sk_isqrt(u64 v)
{
    u64 r = 0, bit = (u64)1 << 62;
    while (bit > v)
        bit >>= 2;
    while (bit) {
        if (v >= r + bit) {
            v -= r + bit;
            r = (r >> 1) + bit;
        } else {
            r >>= 1;
        }
        bit >>= 2;
    }
    return (u32)r;
}

// sk_count's stage (sk_tail_kernels.hip), as far as others build on it: the selection sends it the buckets that fit,
// sk_count_clean has a thread per record, sk_count_big (sk_level0_kernels.hip) cuts the same quads
constexpr int SKC_NT = 1024;                     // two workgroups = 32 waves per CU: the kernel lives on hidden latency
constexpr int SKC_MAXREC = 512;                  // records of a bucket (a bucket of 3300 k-mers of random sequence has ~370)
constexpr int SKC_KPT = 4;                       // k-mers per quad
constexpr int SKC_MAXQ = SKC_NT;                 // quads of a bucket: one per thread (the selection sends buckets with more elsewhere)
constexpr u32 SKC_FREE = ~0u;                    // an empty slot

// k-mer j of a record
__device__ __forceinline__ u64 sk_record_kmer(const ull2_t rec, u32 j, u64 kmask)
{
    return funnel(rec.x, rec.y & (((u64)1 << 44) - 1), 2 * j) & kmask;
}

// The minimizer's length m: 15 for k >= 23 (windows of 9 .. 18 m-mers), 13 for k = 21 and 22 (windows of 9 and 10: runs of
// 5 - 5.5 k-mers, 3 bytes per k-mer; 4^13 / 9 ~ 7 M effective minimizer values keep the final buckets even up to 2^32
// rows).  A function of k alone, so every rank of a sharded count cuts the same records.
// (the host's sk_minimizer_len() and sk_count_clean, which finds a record's m-mer again, share this one rule)
__host__ __device__ constexpr int sk_mlen(int k) { return k >= 23 ? 15 : (k >= 21 ? 13 : 12); }

// most k-mers of a record: it holds 54 bases, and its length field counts to 32
inline u32 sk_lmax(int k) { return 54 - k + 1 > 32 ? 32u : (u32)(54 - k + 1); }

}  // namespace dnagpu
