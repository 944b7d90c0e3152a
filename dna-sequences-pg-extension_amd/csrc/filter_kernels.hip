// filter_kernels.hip -- generate_kmers fused with a WHERE operator (`=`, `^@`, `@>`), bit-sliced.
//
// The reference evaluates the operator once per row, base by base (kmer_eq dna.c:655-668,
// starts_with dna.c:842-866, contains + nucleotide_matches dna.c:1064-1135).  Here one thread tests
// 32 consecutive rows at once on the packed STREAM, never forming a key for a row that fails:
//
//   S            = the 64 bases (128 bits) starting at the thread's first row
//   x_i, y_i     = S >> 2i and S >> (2i+1): bit 2j of x_i / y_i is the low / high code bit of base j+i,
//                  i.e. of base i of the k-mer of row j
//   allowed_i    = the pattern position's set as a boolean function of (x_i, y_i): one or two
//                  32-bit operations per dword (codes A=00 T=01 C=10 G=11, dna.c:120-123)
//   match        = AND over the pattern's non-N positions of allowed_i, on the even bits
//
// ~10 VALU operations per non-N pattern position per 32 rows.  All three operators are such
// patterns: `=` is k singleton sets, `^@` is a prefix of singletons followed by N, `@>` is the IUPAC
// text itself.  Rows are produced in position order (the reference's row order, test.sql:86-92) by
// two sweeps over the (tiny) packed input: workgroup b counts the matches of its contiguous range
// of tiles; then every workgroup sums the counts of the workgroups before it (<= 2048 values),
// lists each tile's matching rows in LDS in row order and writes keys and positions with
// 16 bytes per lane, 1 KiB per wave-instruction.  Keys are formed only for matching rows.
// What a thread reads of its 32 rows -- words, stream, the marks of a table -- is in stream_rows.hpp.
#include "kernels.hpp"
#include "stream_rows.hpp"

namespace dnagpu {

constexpr int FB_THREADS = 256;
constexpr int FB_WAVES = FB_THREADS / 64;
constexpr int FB_ROWS = 32;                          // rows per thread and tile
constexpr int FB_TILE = FB_THREADS * FB_ROWS;        // 8192 rows
constexpr int FB_MAX_GROUPS = 8192;                  // workgroups of one sweep (8 per CU)
static_assert(FB_MAX_GROUPS == FILTER_MAX_GROUPS, "kernels.hpp names the group limit");

typedef unsigned long long ull2_t __attribute__((ext_vector_type(2)));

// One pattern position on both dwords of the 32 rows: a &= allowed(set; x, y), where bit 2j of x / y is the
// low / high code bit of the base the position looks at for row j (odd bit positions carry garbage that
// the caller masks off).  set: bit0 = A(00), bit1 = T(01), bit2 = C(10), bit3 = G(11) -- nucleotide_matches,
// dna.c:1064-1086.  Every case is one three-input v_bitop3_b32 per dword.
__device__ __forceinline__ void and_allowed(u32 set, u32 x0, u32 y0, u32 x1, u32 y1, u32 &a0, u32 &a1)
{
#define FB_CASE(S, EXPR0, EXPR1) case S: a0 &= (EXPR0); a1 &= (EXPR1); break;
    switch (set) {
        FB_CASE(0x1, ~(x0 | y0), ~(x1 | y1))        // A
        FB_CASE(0x2, x0 & ~y0, x1 & ~y1)            // T
        FB_CASE(0x4, ~x0 & y0, ~x1 & y1)            // C
        FB_CASE(0x8, x0 & y0, x1 & y1)              // G
        FB_CASE(0x3, ~y0, ~y1)                      // W = A,T
        FB_CASE(0xC, y0, y1)                        // S = C,G
        FB_CASE(0x5, ~x0, ~x1)                      // M = A,C
        FB_CASE(0xA, x0, x1)                        // K = G,T
        FB_CASE(0x9, ~(x0 ^ y0), ~(x1 ^ y1))        // R = A,G
        FB_CASE(0x6, x0 ^ y0, x1 ^ y1)              // Y = C,T
        FB_CASE(0xE, x0 | y0, x1 | y1)              // B = not A
        FB_CASE(0xB, x0 | ~y0, x1 | ~y1)            // D = not C
        FB_CASE(0x7, ~(x0 & y0), ~(x1 & y1))        // H = not G
        FB_CASE(0xD, ~x0 | y0, ~x1 | y1)            // V = not T
        FB_CASE(0x0, 0u, 0u)                        // U: matches nothing (dna.c:1070)
    default: break;                                 // N
    }
#undef FB_CASE
}

// the eight pattern positions 8*W .. 8*W+7 (sets in `sw`, 4 bits each); W is a compile-time constant, so the
// dwords the shifts read and the shift bases are too
template <int W>
__device__ __forceinline__ void match_word(u32 sw, const Stream4 &s, u32 &a0, u32 &a1)
{
    if (sw == 0xFFFFFFFFu)                          // eight N in a row: nothing to test
        return;
    constexpr int D = W >> 1;                       // positions 0..15 shift inside dwords 0..2, 16..31 inside 1..3
    const u32 lo = s.d[D], mid = s.d[D + 1], hi = s.d[D + 2];
#pragma unroll 1
    for (u32 j = 0; j < 8; j++, sw >>= 4) {
        const u32 set = sw & 15u;
        if (set == 15u)
            continue;
        const u32 sh = 2u * ((u32)(W & 1) * 8u + j);
        const u32 x0 = __builtin_amdgcn_alignbit(mid, lo, sh), x1 = __builtin_amdgcn_alignbit(hi, mid, sh);
        const u32 y0 = __builtin_amdgcn_alignbit(mid, lo, sh + 1), y1 = __builtin_amdgcn_alignbit(hi, mid, sh + 1);
        and_allowed(set, x0, y0, x1, y1, a0, a1);
    }
}

// Even bit 2j of the result = row j (of the thread's 32) satisfies the pattern.  s0..s3 are fb.sets[] held in
// scalar registers by the caller (positions >= k are N).
__device__ __forceinline__ u64 match_rows(const Stream4 &s, u32 s0, u32 s1, u32 s2, u32 s3)
{
    u32 a0 = ~0u, a1 = ~0u;
    match_word<0>(s0, s, a0, a1);
    match_word<1>(s1, s, a0, a1);
    match_word<2>(s2, s, a0, a1);
    match_word<3>(s3, s, a0, a1);
    return (((u64)a1 << 32) | a0) & 0x5555555555555555ull;
}

// even-bit mask of the rows of a thread that exist: `left` rows remain from the thread's first row on
__device__ __forceinline__ u64 valid_rows(long long left)
{
    const u64 EVEN = 0x5555555555555555ull;
    if (left >= FB_ROWS)
        return EVEN;
    if (left <= 0)
        return 0;
    return EVEN & (((u64)1 << (2 * (unsigned)left)) - 1);
}

// bit 2j -> bit j
__device__ __forceinline__ u32 compact_even(u64 m)
{
    u32 lo = (u32)m, hi = (u32)(m >> 32);
    lo = (lo | (lo >> 1)) & 0x33333333u;
    hi = (hi | (hi >> 1)) & 0x33333333u;
    lo = (lo | (lo >> 2)) & 0x0f0f0f0fu;
    hi = (hi | (hi >> 2)) & 0x0f0f0f0fu;
    lo = (lo | (lo >> 4)) & 0x00ff00ffu;
    hi = (hi | (hi >> 4)) & 0x00ff00ffu;
    lo = (lo | (lo >> 8)) & 0x0000ffffu;
    hi = (hi | (hi >> 8));
    return lo | (hi << 16);
}

// ================================================================================================
// The stages of the two sweeps, written once.  The single-sequence kernels (fb_*) and the table kernels (fbt_*) are
// made of them; TABLE is a compile-time switch, so a single-sequence kernel holds no trace of the marks.

// what every thread of a sweep derives once from the call's window [first, first + count)
struct Sweep {
    u32 s0, s1, s2, s3;                              // fb.sets[], held in scalar registers (positions >= k are N)
    u32 fo;                                          // first % 32: where the window starts inside its first word
    unsigned sh;                                     // the same in bits
    u32 span;                                        // k - 1 (tables)
    u64 w_first;
    u64 t0, t1;                                      // the consecutive tiles of this workgroup
};

__device__ __forceinline__ Sweep sweep_of(u64 first, u64 count, const FilterBits &fb, u32 tiles_per_group)
{
    Sweep sw;
    sw.s0 = fb.sets[0], sw.s1 = fb.sets[1], sw.s2 = fb.sets[2], sw.s3 = fb.sets[3];
    sw.fo = (u32)(first & 31);
    sw.sh = sw.fo * 2;
    sw.span = (u32)fb.k - 1u;
    sw.w_first = first >> 5;
    const u64 n_tiles = (count + FB_TILE - 1) / FB_TILE;
    sw.t0 = (u64)blockIdx.x * tiles_per_group;
    sw.t1 = sw.t0 + tiles_per_group;
    if (sw.t1 > n_tiles)
        sw.t1 = n_tiles;
    return sw;
}

// what a thread reads of tile t: the words of its 32 rows and, over a table, the marks behind them.  The sweeps ask for
// tile t + 1 before they test tile t.
struct TileIn {
    Words3 w;
    Marks3 m;
};

template <bool TABLE>
__device__ __forceinline__ TileIn tile_load(const FilterSource &src, const Sweep &sw, u64 t)
{
    const int tid = threadIdx.x;
    const u64 w = sw.w_first + t * (FB_TILE / 32) + tid;
    TileIn r;
    r.w = words_load(src.words, src.n_words, w, sw.sh);
    if (TABLE)
        r.m = marks_load(src.marks, src.n_mark_words, w, sw.fo);
    return r;
}

// even bit 2j = row j of the thread's 32 in tile t exists and satisfies the pattern
__device__ __forceinline__ u64 tile_match(const TileIn &in, const Sweep &sw, u64 count, u64 t)
{
    const int tid = threadIdx.x;
    const u64 row0 = t * FB_TILE + (u64)tid * FB_ROWS;
    return match_rows(stream_of(in.w, sw.sh), sw.s0, sw.s1, sw.s2, sw.s3) &
           valid_rows(row0 < count ? (long long)(count - row0) : 0);
}

// bit j = row j is a row of the result: it matches and, over a table, lies inside one sequence
template <bool TABLE>
__device__ __forceinline__ u32 tile_rows(const TileIn &in, const Sweep &sw, u64 count, u64 t)
{
    u32 m = compact_even(tile_match(in, sw, count, t));
    if (TABLE)
        m &= ~spoiled_rows(in.m, sw.fo, sw.span);
    return m;
}

// ---- sweep 1: rows of the result per workgroup range ------------------------------------------
template <bool TABLE>
__device__ __forceinline__ void count_sweep(const FilterSource &src, u64 first, u64 count, const FilterBits &fb,
                                            u32 tiles_per_group, u32 *__restrict__ group_counts)
{
    __shared__ u32 wsum[FB_WAVES];
    const Sweep sw = sweep_of(first, count, fb, tiles_per_group);
    u32 c = 0;
    TileIn nxt = tile_load<TABLE>(src, sw, sw.t0);
    for (u64 t = sw.t0; t < sw.t1; t++) {
        const TileIn cur = nxt;
        if (t + 1 < sw.t1)
            nxt = tile_load<TABLE>(src, sw, t + 1);
        // (without marks the even-bit mask is counted as it is)
        c += TABLE ? (u32)__popc(tile_rows<true>(cur, sw, count, t)) : (u32)__popcll(tile_match(cur, sw, count, t));
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0)
        wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 g = 0;
        for (int w = 0; w < FB_WAVES; w++)
            g += wsum[w];
        group_counts[blockIdx.x] = g;
    }
}

__global__ __launch_bounds__(FB_THREADS) void fb_count_kernel(const u64 *__restrict__ words, u64 n_words, u64 first,
                                                              u64 count, FilterBits fb, u32 tiles_per_group,
                                                              u32 *__restrict__ group_counts)
{
    count_sweep<false>(FilterSource{words, n_words, nullptr, 0, nullptr, 0}, first, count, fb, tiles_per_group, group_counts);
}

__global__ __launch_bounds__(FB_THREADS) void fbt_count_kernel(const u64 *__restrict__ words, u64 n_words,
                                                               const u32 *__restrict__ marks, u64 n_mark_words, u64 first,
                                                               u64 count, FilterBits fb, u32 tiles_per_group,
                                                               u32 *__restrict__ group_counts)
{
    count_sweep<true>(FilterSource{words, n_words, marks, n_mark_words, nullptr, 0}, first, count, fb, tiles_per_group,
                      group_counts);
}

// ---- sweep 2: the rows in position order ------------------------------------------------------
// rows of the result before this workgroup's range: the sum of the group counts before it (wtot: FB_WAVES words)
__device__ __forceinline__ u64 group_base(const u32 *__restrict__ group_counts, u32 *wtot, u64 *base_sh)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u32 part = 0;
    for (u32 g = tid; g < blockIdx.x; g += FB_THREADS)
        part += group_counts[g];
    // partial sums of up to 2^32-1 rows cannot overflow 32 bits in total
    part = wave_sum(part);
    if (lane == 0)
        wtot[wave] = part;
    __syncthreads();
    if (tid == 0) {
        u64 b = 0;
        for (int w = 0; w < FB_WAVES; w++)
            b += wtot[w];
        *base_sh = b;
    }
    __syncthreads();
    return *base_sh;
}

// Where the thread's rows m go in the tile's list, and the rows of the whole tile.  Ends behind a barrier that also says:
// the previous tile's list and words (and whatever else the caller keeps per tile in LDS) have been read.
__device__ __forceinline__ u32 tile_scan(u32 m, const Words3 &cur, u32 *wtot, u64 *wsh, u32 *tile_cnt)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 c = (u32)__popc(m);
    const u32 inc = wave_incl_scan(c);
    if (lane == 63)
        wtot[wave] = inc;
    __syncthreads();
    u32 wbase = 0, cnt = 0;
#pragma unroll
    for (int w = 0; w < FB_WAVES; w++) {
        const u32 v = wtot[w];
        wbase += w < wave ? v : 0u;
        cnt += v;
    }
    wsh[tid] = cur.w0;
    if (tid == FB_THREADS - 1) {
        wsh[FB_THREADS] = cur.w1;
        wsh[FB_THREADS + 1] = cur.w2;
    }
    *tile_cnt = cnt;
    return wbase + inc - c;
}

// The tile's packed words into wsh (keys are cut from there) and the tile-local rows of m into list from slot r on, in
// row order; ends behind a barrier.
__device__ __forceinline__ void tile_list(u32 m, u32 r, unsigned short *list)
{
    const int tid = threadIdx.x;
    const u32 row_in_tile = (u32)tid * FB_ROWS;
    while (m) {
        const u32 j = (u32)__builtin_ctz(m);
        m &= m - 1;
        list[r++] = (unsigned short)(row_in_tile + j);
    }
    __syncthreads();
}

// key of tile-local row r: bits [2q, 2q + 2k) of the tile's words, q = r + first % 32
__device__ __forceinline__ u64 tile_key(const u64 *wsh, u32 q, u64 mask)
{
    return funnel(wsh[q >> 5], wsh[(q >> 5) + 1], (q & 31u) * 2u) & mask;
}

// The store stage: listed row s of the tile goes to slot off + s of each of the N arrays that want(a) names, slots from
// `cap` on are not stored.  Array 0 holds the keys, key(r) of tile-local row r; rest(r, v) gives v[a] for the wanted
// arrays a >= 1 and is called only when there is one.  Both are called only for rows that are stored, the keys of a slot
// or pair going out before the rest is worked out.
// WIDE: the wanted arrays are 16-byte aligned at the same index parity `par`, so slot pairs (s, s + 1) with
// (off + s + par) even go out as one 16-byte store per array; the first and last slot of a tile and the slot before
// `cap` may be left over as singles.
// (A wave-granular variant -- every wave lists and writes its own 2048 rows, no workgroup barrier -- was
// measured 8-10 % slower at selectivity 1/4: four times as many, four times shorter output bursts.)
template <int N, bool WIDE, typename Want, typename Key, typename Rest>
__device__ __forceinline__ void store_listed(const unsigned short *list, u32 tile_cnt, u64 off, u32 par, u64 cap,
                                             u64 *const (&out)[N], Want want, Key key, Rest rest)
{
    const int tid = threadIdx.x;
    bool more = false;                               // an array behind the keys is wanted
#pragma unroll
    for (int a = 1; a < N; a++)
        more = more || want(a);
    auto store_one = [&](u32 r, u64 i) {
        if (want(0))
            __builtin_nontemporal_store(key(r), &out[0][i]);
        if (more) {
            u64 v[N] = {};
            rest(r, v);
#pragma unroll
            for (int a = 1; a < N; a++)
                if (want(a))
                    __builtin_nontemporal_store(v[a], &out[a][i]);
        }
    };
    if (WIDE) {
        const int lead = (int)((off + par) & 1);
        for (int s = 2 * tid - lead; s < (int)tile_cnt; s += 2 * FB_THREADS) {
            const bool v0 = s >= 0, v1 = s + 1 < (int)tile_cnt;
            // (an empty tile with lead = 1 has neither slot: both reads stay inside the list)
            const u32 r0 = list[v0 ? s : 0], r1 = list[v1 ? s + 1 : (v0 ? s : 0)];
            const u64 i0 = off + (u64)(long long)s;
            if (v0 && v1 && i0 + 1 < cap) {
                ull2_t xy;
                if (want(0)) {
                    xy.x = key(r0);
                    xy.y = key(r1);
                    __builtin_nontemporal_store(xy, reinterpret_cast<ull2_t *>(out[0] + i0));
                }
                if (more) {
                    u64 x[N] = {}, y[N] = {};
                    rest(r0, x);
                    rest(r1, y);
#pragma unroll
                    for (int a = 1; a < N; a++)
                        if (want(a)) {
                            xy.x = x[a];
                            xy.y = y[a];
                            __builtin_nontemporal_store(xy, reinterpret_cast<ull2_t *>(out[a] + i0));
                        }
                }
            } else {
                if (v0 && i0 < cap)
                    store_one(r0, i0);
                if (v1 && i0 + 1 < cap)
                    store_one(r1, i0 + 1);
            }
        }
    } else {
        for (u32 s = tid; s < tile_cnt; s += FB_THREADS) {
            const u32 r0 = list[s];
            const u64 i0 = off + s;
            if (i0 < cap)
                store_one(r0, i0);
        }
    }
}

// One sequence: keys and positions (HAS_*: compile-time, so an array not asked for costs nothing).
template <bool HAS_KEYS, bool HAS_POS, bool WIDE>
__global__ __launch_bounds__(FB_THREADS) void fb_write_kernel(const u64 *__restrict__ words, u64 n_words, u64 first,
                                                              u64 count, u64 mask, FilterBits fb, u32 tiles_per_group,
                                                              const u32 *__restrict__ group_counts,
                                                              u64 *__restrict__ out_keys, u64 *__restrict__ out_pos,
                                                              u64 cap, u32 par, u64 *__restrict__ total_out)
{
    __shared__ unsigned short list[FB_TILE];         // tile-local rows of the matches, in row order
    __shared__ u64 wsh[FB_THREADS + 2];              // the tile's packed words
    __shared__ u32 wtot[FB_WAVES];
    __shared__ u64 base_sh;
    const int tid = threadIdx.x;
    u64 off = group_base(group_counts, wtot, &base_sh);

    const FilterSource src = {words, n_words, nullptr, 0, nullptr, 0};
    const Sweep sw = sweep_of(first, count, fb, tiles_per_group);
    u64 *const out[2] = {out_keys, out_pos};
    TileIn nxt = tile_load<false>(src, sw, sw.t0);
    for (u64 t = sw.t0; t < sw.t1; t++) {
        const TileIn cur = nxt;
        if (t + 1 < sw.t1)
            nxt = tile_load<false>(src, sw, t + 1);
        const u32 m = tile_rows<false>(cur, sw, count, t);
        u32 tile_cnt;
        const u32 r = tile_scan(m, cur.w, wtot, wsh, &tile_cnt);
        tile_list(m, r, list);
        const u64 tile_pos0 = first + t * FB_TILE;
        store_listed<2, WIDE>(
            list, tile_cnt, off, par, cap, out, [](int a) { return a == 0 ? HAS_KEYS : HAS_POS; },
            [&](u32 row) { return tile_key(wsh, row + sw.fo, mask); }, [&](u32 row, u64 *v) { v[1] = tile_pos0 + row; });
        off += tile_cnt;
    }
    if (total_out && blockIdx.x == gridDim.x - 1 && tid == 0)
        *total_out = off;
}

// Index of the first entry of a[lo .. hi) that is > p (hi when there is none), a ascending; by the whole workgroup, every
// thread gets the answer.  256-ary: every round the threads test the last entries of 256 equal chunks and the answer's
// chunk becomes the range.  wc: FB_WAVES words of LDS that nothing else uses during the call.
__device__ __forceinline__ u64 block_upper_bound(const u64 *__restrict__ a, u64 lo, u64 hi, u64 p, u32 *wc)
{
    const int tid = threadIdx.x;
    while (hi > lo) {                                // uniform
        const u64 step = (hi - lo + FB_THREADS - 1) / FB_THREADS;
        const u64 c0 = lo + (u64)tid * step;
        bool le = false;
        if (c0 < hi) {
            const u64 c1 = c0 + step < hi ? c0 + step : hi;
            le = a[c1 - 1] <= p;
        }
        const u32 wcnt = (u32)__popcll(__ballot(le));
        if ((tid & 63) == 0)
            wc[tid >> 6] = wcnt;
        __syncthreads();
        u32 cnt = 0;
#pragma unroll
        for (int w = 0; w < FB_WAVES; w++)
            cnt += wc[w];
        __syncthreads();
        // chunks [0, cnt) lie at or below p; chunk cnt, if it has entries, ends above p
        u64 nlo = lo + (u64)cnt * step;
        if (nlo > hi)
            nlo = hi;
        u64 nhi = nlo + step < hi ? nlo + step : hi;
        if (nhi > nlo)
            nhi--;
        lo = nlo;
        hi = nhi;
    }
    return lo;
}

// A table of sequences (FROM dna_sequences d, LATERAL generate_kmers(d.sequence, k), test.sql:140-150, 172-176): the rows
// of every sequence's own generate_kmers, each with the sequence it came from and its ordinal inside that sequence, in
// table order; any of the three arrays may be null (a run-time test).
// The sequence of a row at stream position p is the LAST sequence that starts at or before p (an upper bound over
// seq_starts, minus one: of a run of equal starts -- empty sequences -- only the last one has bases).  Nothing searches
// all n_seqs + 1 starts per row: the workgroup finds the bound of its first position once (block_upper_bound); every tile
// then reads the 256 starts from its lower bound on into LDS, counts those at or below its last position -- that is its
// upper bound, unless all 256 are, which takes another block_upper_bound (sequences shorter than 32 bases on average) --
// and every STORED row searches between the tile's two bounds: in LDS, or in global memory when they are more than 256
// apart.  One long sequence gives equal bounds and no search.
constexpr u32 FBT_STARTS = FB_THREADS;               // starts of a tile held in LDS
template <bool WIDE>
__global__ __launch_bounds__(FB_THREADS) void fbt_write_kernel(const u64 *__restrict__ words, u64 n_words,
                                                               const u32 *__restrict__ marks, u64 n_mark_words,
                                                               const u64 *__restrict__ seq_starts, u64 n_seqs, u64 first,
                                                               u64 count, u64 mask, FilterBits fb, u32 tiles_per_group,
                                                               const u32 *__restrict__ group_counts,
                                                               u64 *__restrict__ out_keys, u64 *__restrict__ out_seq,
                                                               u64 *__restrict__ out_pos, u64 cap, u32 par,
                                                               u64 *__restrict__ total_out)
{
    __shared__ unsigned short list[FB_TILE];         // tile-local rows of the listed table rows, in row order
    __shared__ u64 wsh[FB_THREADS + 2];              // the tile's packed words
    __shared__ u64 sst[FBT_STARTS + 1];              // seq_starts[lo - 1 .. lo + 256) of the tile's lower bound lo
    __shared__ u32 wtot[FB_WAVES], wle[FB_WAVES], wub[FB_WAVES];
    __shared__ u64 base_sh;
    const int tid = threadIdx.x;
    u64 off = group_base(group_counts, wtot, &base_sh);

    const FilterSource src = {words, n_words, marks, n_mark_words, seq_starts, n_seqs};
    const Sweep sw = sweep_of(first, count, fb, tiles_per_group);
    u64 *const out[3] = {out_keys, out_seq, out_pos};
    const bool locate = out_seq || out_pos;          // uniform
    // seq_starts[0 .. ub_lo) lie at or below every position of the tile: entry 0 is 0, entry n_seqs is above every row
    u64 ub_lo = 1;
    if (locate && sw.t0 < sw.t1)
        ub_lo = block_upper_bound(seq_starts, 1, n_seqs, first + sw.t0 * FB_TILE, wub);

    TileIn nxt = tile_load<true>(src, sw, sw.t0);
    for (u64 t = sw.t0; t < sw.t1; t++) {
        const u64 tile_row0 = t * FB_TILE;
        const TileIn cur = nxt;
        if (t + 1 < sw.t1)
            nxt = tile_load<true>(src, sw, t + 1);
        // the starts from the lower bound on, and how many of them the tile's last position has reached
        const u64 p_last = first + (tile_row0 + FB_TILE < count ? tile_row0 + FB_TILE : count) - 1;
        u64 sv = ~(u64)0, sv_lo = 0;
        if (locate) {
            if (ub_lo + (u64)tid <= n_seqs)
                sv = seq_starts[ub_lo + tid];
            sv_lo = seq_starts[ub_lo - 1];
        }
        const u32 nle = (u32)__popcll(__ballot(sv <= p_last));
        if ((tid & 63) == 0)
            wle[tid >> 6] = nle;
        const u32 m = tile_rows<true>(cur, sw, count, t);
        u32 tile_cnt;
        const u32 r = tile_scan(m, cur.w, wtot, wsh, &tile_cnt);
        u32 n_le = 0;
#pragma unroll
        for (int wv = 0; wv < FB_WAVES; wv++)
            n_le += wle[wv];
        sst[1 + tid] = sv;
        if (tid == 0)
            sst[0] = sv_lo;
        u64 ub_hi = ub_lo + n_le;
        if (locate && n_le == FBT_STARTS && ub_hi <= n_seqs)     // uniform
            ub_hi = block_upper_bound(seq_starts, ub_hi, n_seqs, p_last, wub);
        const u64 n_between = ub_hi - ub_lo;
        tile_list(m, r, list);

        // sequence and ordinal of the row at stream position p
        auto locate_row = [&](u64 p, u64 &sq, u64 &ord) {
            if (n_between <= FBT_STARTS) {
                u32 lo = 0, n = (u32)n_between;
                while (n) {
                    const u32 half = n >> 1;
                    if (sst[1 + lo + half] <= p) {
                        lo += half + 1;
                        n -= half + 1;
                    } else {
                        n = half;
                    }
                }
                sq = ub_lo - 1 + lo;
                ord = p - sst[lo];
            } else {
                u64 lo = ub_lo, n = n_between;
                while (n) {
                    const u64 half = n >> 1;
                    if (seq_starts[lo + half] <= p) {
                        lo += half + 1;
                        n -= half + 1;
                    } else {
                        n = half;
                    }
                }
                sq = lo - 1;
                ord = p - seq_starts[lo - 1];
            }
        };
        store_listed<3, WIDE>(
            list, tile_cnt, off, par, cap, out, [&](int a) { return out[a] != nullptr; },
            [&](u32 row) { return tile_key(wsh, row + sw.fo, mask); },
            [&](u32 row, u64 *v) { locate_row(first + tile_row0 + row, v[1], v[2]); });
        off += tile_cnt;
        ub_lo = ub_hi;                               // at or below the next tile's first position
    }
    if (total_out && blockIdx.x == gridDim.x - 1 && tid == 0)
        *total_out = off;
}

// ---- launchers --------------------------------------------------------------------------------
// groups of the two sweeps for `count` rows: every group takes the same number of consecutive tiles
void filter_bits_geometry(u64 count, u32 *n_groups, u32 *tiles_per_group)
{
    const u64 n_tiles = (count + FB_TILE - 1) / FB_TILE;
    u64 tpg = (n_tiles + FB_MAX_GROUPS - 1) / FB_MAX_GROUPS;
    if (tpg == 0)
        tpg = 1;
    *tiles_per_group = (u32)tpg;
    *n_groups = (u32)((n_tiles + tpg - 1) / tpg);
}

hipError_t launch_filter_bits_count(const FilterSource &src, u64 first, u64 count, const FilterBits &fb, u32 *group_counts,
                                    hipStream_t s)
{
    if (count == 0)
        return hipSuccess;
    u32 groups, tpg;
    filter_bits_geometry(count, &groups, &tpg);
    if (src.marks)
        hipLaunchKernelGGL(fbt_count_kernel, dim3(groups), dim3(FB_THREADS), 0, s, src.words, src.n_words, src.marks,
                           src.n_mark_words, first, count, fb, tpg, group_counts);
    else
        hipLaunchKernelGGL(fb_count_kernel, dim3(groups), dim3(FB_THREADS), 0, s, src.words, src.n_words, first, count, fb,
                           tpg, group_counts);
    return hipGetLastError();
}

// what every write kernel takes behind its source
struct WriteArgs {
    u64 first, count, mask;
    FilterBits fb;
    u32 tpg;
    const u32 *group_counts;
    u64 *out_keys, *out_seq, *out_pos;
    u64 cap;
    u32 par;
    u64 *total_out;
};

template <bool HK, bool HP, bool WIDE>
static void launch_single_write(dim3 grid, hipStream_t s, const FilterSource &src, const WriteArgs &a)
{
    hipLaunchKernelGGL((fb_write_kernel<HK, HP, WIDE>), grid, dim3(FB_THREADS), 0, s, src.words, src.n_words, a.first, a.count,
                       a.mask, a.fb, a.tpg, a.group_counts, a.out_keys, a.out_pos, a.cap, a.par, a.total_out);
}

template <bool WIDE>
static void launch_write_variant(dim3 grid, hipStream_t s, const FilterSource &src, const WriteArgs &a)
{
    if (src.marks)
        hipLaunchKernelGGL((fbt_write_kernel<WIDE>), grid, dim3(FB_THREADS), 0, s, src.words, src.n_words, src.marks,
                           src.n_mark_words, src.seq_starts, src.n_seqs, a.first, a.count, a.mask, a.fb, a.tpg, a.group_counts,
                           a.out_keys, a.out_seq, a.out_pos, a.cap, a.par, a.total_out);
    else if (a.out_keys && a.out_pos)
        launch_single_write<true, true, WIDE>(grid, s, src, a);
    else if (a.out_keys)
        launch_single_write<true, false, WIDE>(grid, s, src, a);
    else
        launch_single_write<false, true, WIDE>(grid, s, src, a);
}

hipError_t launch_filter_bits_write(const FilterSource &src, u64 first, u64 count, const FilterBits &fb,
                                    const u32 *group_counts, u64 *out_keys, u64 *out_seq, u64 *out_pos, u64 cap,
                                    u64 *total_out, hipStream_t s)
{
    if (count == 0)
        return hipSuccess;
    u32 groups, tpg;
    filter_bits_geometry(count, &groups, &tpg);
    // 16-byte stores need every array asked for 8-byte aligned, all at the same index parity at 16-byte boundaries
    const uintptr_t a[3] = {reinterpret_cast<uintptr_t>(out_keys), reinterpret_cast<uintptr_t>(out_seq),
                            reinterpret_cast<uintptr_t>(out_pos)};
    uintptr_t ref = 0;
    bool wide = true;
    for (uintptr_t x : a) {
        if (!x)
            continue;
        if (!ref)
            ref = x;
        wide = wide && (x & 7) == 0 && ((x ^ ref) & 15) == 0;
    }
    const WriteArgs wa = {first, count, kmer_mask(fb.k), fb, tpg, group_counts, out_keys, out_seq, out_pos, cap,
                          (u32)((ref >> 3) & 1), total_out};
    if (wide)
        launch_write_variant<true>(dim3(groups), s, src, wa);
    else
        launch_write_variant<false>(dim3(groups), s, src, wa);
    return hipGetLastError();
}

}  // namespace dnagpu
