// sk_level0_kernels.hip -- level 0 of the super-k-mer engine (sk_device.hpp): the sweeps over the packed dna.  The front end
// (hashes, window minima), the walks that cut records, sk_hist0 / sk_scatter0, the slabs of the sweep without a histogram.
//
// And, at the end, sk_count_big / sk_big_merge, which belong to the tail.  They are here for the compiler's sake: the
// helpers of kmer_device.hpp and sk_device.hpp have internal linkage in device code, so the compiler fits each to the
// calls it sees in ONE translation unit.  Level 0 only calls funnel() with shifts below 64; compiled with nothing else it
// gets other instructions for every sk_hist0 / sk_scatter0 than it always had (63 ^ sh for 63 - sh, other registers).
// With a caller whose shift is not bounded in the same unit -- sk_count_big's is the cheapest to compile -- the sweeps come
// out instruction for instruction as before (tools/isa_same.py; profiles/refactor_sk_kernels.md).  Moving sk_count_big out
// is a change of level 0's device code and wants its own measurement.
#include "sk_device.hpp"

namespace dnagpu {

int sk_tile_rows() { return SK_TILE_ROWS; }
int sk_max_c0() { return SK_MAX_C0; }

// ------------------------------------------------------------------------------------------------
// Front end of both dna sweeps, ONE WAVE per tile and nothing shared between waves: a tile = rows [row0, row0 + n_rows),
// n_rows <= SKW_ROWS; lane l owns the 32 rows row0 + 32 l ... (lane 63 owns none: it supplies the hashes that complete
// lane 62's windows).  What a lane needs of its neighbours -- the next lane's first W-1 hashes, the boundary minima, the
// last run break before its rows -- moves by DPP wave shifts and a DPP scan: no LDS, no barrier (round 2's workgroup
// tile exchanged them through LDS behind five workgroup barriers; the two sweeps together took 7.9 ms at 3 Gbase).
// Every lane ends with the window minimum of each of its rows in hm[]; sk_front_open adds the state of the record
// that is open at its first row.  Records are cut at tile boundaries (one extra record per 2016 rows: +0.4 %).
//   A minimum is hash bits 7..31 | 64 | position: the m-mers' hashes carry, in their low six bits, their own position
//   relative to the lane's first row (0 .. 31 + W - 1), so the minimum of a window is its smallest 25-bit hash and, among
//   equal ones, the LEFTMOST -- a function of the k-mer's content, like the hash.  Two neighbouring rows with equal hm
//   have the same m-mer occurrence as their minimum.  (Distinct m-mers may now tie on the 25 bits: 2^-25 per pair; the
//   bucket digits use the hash part only, so equal k-mers still share their bucket.)  Bit 6 is set in every real hash, so
//   that 0 is smaller than all of them:
//   BATCH (a table of sequences in one packed stream, dnagpu_count_kmers_batch: `marks` = one bit per base, set where a
//   sequence starts): an m-mer that reaches across a sequence start hashes to 0.  A k-mer's window holds such an m-mer
//   exactly when the k-mer itself reaches across a start, so the rows that are NOT rows of the table -- and only they --
//   have a minimum below 64 (hash part 0); they form runs of their own, which are counted and stored nowhere.
template <int W>
struct SkFront {
    u32 hm[32];
    u32 next_first;        // hm[0] of the next lane, its position in THIS lane's terms (+ 32)
    u32 prev_last;         // hm[31] of the lane before, its position in this lane's terms (- 32: a position before this lane's
                           // first row borrows from the hash part -- it then equals no minimum of this lane, rightly)
    u32 n_valid;           // rows of this lane that exist (0..32)
    u32 n_rows;            // rows of the tile
    bool plain;            // wave-uniform: a full tile whose records are its natural runs (see sk_front)
    // sk_front_open:
    u32 ns0;               // start row of the natural run that is open at this lane's first row
    u32 c0;                // length so far of the record open at this lane's first row
};

template <int W, bool BATCH = false>
__device__ __forceinline__ void sk_front(SkFront<W> &f, const u64 *__restrict__ words, u64 n_words, u64 pos0, u32 n_rows,
                                         u32 lmax, u32 mmask /* 2 m ones: the m-mer */,
                                         u64 *wsh /* this wave's [66] or null: the tile's words, word 0 = the one holding pos0 */,
                                         const u32 *__restrict__ marks = nullptr, u64 n_mark_words = 0)
{
    const int lane = threadIdx.x & 63;
    // the 64 bases from this lane's first row on (pos0 + 32 lane): 4 dwords
    const u64 pos = pos0 + (u64)lane * 32;
    const u64 w = pos >> 5;
    const unsigned sh = (unsigned)(pos & 31) * 2;          // wave-uniform
    const u64 w0 = w < n_words ? words[w] : 0, w1 = w + 1 < n_words ? words[w + 1] : 0;
    u64 lo = w0, hi = w1;
    u64 w2 = 0;
    if (sh || (wsh && lane == 63)) {
        w2 = w + 2 < n_words ? words[w + 2] : 0;
        if (sh) {
            lo = (w0 >> sh) | (w1 << (64 - sh));
            hi = (w1 >> sh) | (w2 << (64 - sh));
        }
    }
    if (wsh) {                                             // (the previous tile's payload reads are this wave's own, earlier in program order)
        wsh[lane] = w0;
        if (lane == 63) {
            wsh[64] = w1;
            wsh[65] = w2;
        }
    }
    const u32 d[4] = {(u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32)};
    constexpr int B = W - 1;                               // a window = W hashes = a[i .. i + B]
    constexpr int N = 32 + B;
    static_assert(W >= 9 && W <= 18, "window lengths of k = 23 .. 32 at m = 15");
    u32 a[N];
    const u32 hi_bits = (u32)__popc(mmask) - 24u;          // (wave-uniform: 6 for m = 15, 2 for m = 13)
    // BATCH: bit j of `within` = this lane's m-mer j reaches across no sequence start (no mark among the m - 1 bases behind
    // its first): the marks of the 64 bases from the lane's first on, smeared over m - 1 places
    u32 within = ~0u;
    if (BATCH) {
        const u64 mw = pos >> 5;
        const unsigned msh = (unsigned)(pos & 31);                                 // wave-uniform
        const u32 b0 = mw < n_mark_words ? marks[mw] : 0u, b1 = mw + 1 < n_mark_words ? marks[mw + 1] : 0u,
                  b2 = mw + 2 < n_mark_words ? marks[mw + 2] : 0u;
        const u64 S = ((u64)__builtin_amdgcn_alignbit(b2, b1, msh) << 32) | __builtin_amdgcn_alignbit(b1, b0, msh);
        u64 r = S >> 1;                            // bit i: a sequence starts at base i + 1 of the lane's
        r |= r >> 1;
        r |= r >> 2;
        r |= r >> 4;                               // ... starts among bases i + 1 .. i + 8
        const unsigned mm1 = (unsigned)__popc(mmask) / 2u - 1u;                    // m - 1 (12 or 14)
        r |= r >> (mm1 - 8u);                      // ... among bases i + 1 .. i + m - 1
        within = ~(u32)r;
    }
#pragma unroll
    for (int j = 0; j < 32; j++) {
        const int q = (2 * j) >> 5, s = (2 * j) & 31;
        const u32 t = __builtin_amdgcn_alignbit(d[q + 1], d[q], s);                // 16 bases: the m-mer's and more
        a[j] = (sk_mix_raw(t, hi_bits) & ~SK_GPOS_MASK) | (64u | (u32)j);          // (one v_and_or)
        if (BATCH)
            a[j] &= (u32)((int)(within << (31 - j)) >> 31);                        // (v_bfe_i32 + v_and)
    }
    // the next lane's first W-1 hashes complete this lane's windows (their positions: 32 ... in this lane's terms)
#pragma unroll
    for (int j = 0; j < B; j++)
        a[32 + j] = wave_next(a[j]) + 32u;
    // Window minima in three operations per row whatever W (van Herk / Gil-Werman): cut a[] into blocks of B; with
    // suf[i] = min of a[i .. end of i's block] and pre[i] = min of a[start of i's block .. i], the window [i, i + B]
    // is suf[i] and pre[i + B] together (i + B sits in the next block at i's offset).  (Round 2 took the minima by
    // doubling: 4 x 47 + 32 operations for 32 rows; this is 2 x 30 + 32.)
    u32 suf[N], pre[N];
#pragma unroll
    for (int i = N - 1; i >= 0; i--)
        suf[i] = (i == N - 1 || (i + 1) % B == 0) ? a[i] : min(a[i], suf[i + 1]);
#pragma unroll
    for (int i = 0; i < N; i++)
        pre[i] = (i % B == 0) ? a[i] : min(a[i], pre[i - 1]);
#pragma unroll
    for (int j = 0; j < 32; j++)
        f.hm[j] = min(suf[j], pre[j + B]);

    const u32 r0 = (u32)lane * 32;
    f.n_valid = r0 >= n_rows ? 0u : (n_rows - r0 < 32u ? n_rows - r0 : 32u);
    f.n_rows = n_rows;
    // neighbours' boundary minima
    f.next_first = wave_next(f.hm[0]) + 32u;
    f.prev_last = wave_prev(f.hm[31]) - 32u;
    // A tile may be PLAIN if it is full.  Its records are then the runs of equal minima, hash AND position (cut at the
    // tile's end): one m-mer occurrence stays the minimum of at most W <= 18 windows, so such a record never outgrows lmax,
    // and all its k-mers have their leftmost minimum m-mer at one place.  On random sequence a tile has ~225 of them.
    // Where one m-mer repeats (low-complexity sequence) its leftmost occurrence moves on row after row: a record per row.
    // A short stretch of that costs a few short records and nothing else; a tile that is MOSTLY that -- more than
    // sk_plain_max(W) records, which its callers count -- goes through the general walk instead, which cuts by the m-mer's
    // VALUE and every lmax rows (SK_REC_MULTI records).  (Round 3 and the first half of round 4 tested for a run of one
    // hash over 21 rows on every fourth row -- 55 operations per lane and tile -- and sent every tile with ONE such stretch
    // through the general walk: on real sequence that is every tenth tile, all of its records SK_REC_MULTI.)
    f.plain = n_rows == (u32)SKW_ROWS;
}

// ---- the general walk (a partial tile, low-complexity sequence, a plain tile whose list overflowed).  Runs are cut where a
// row's RUN KEY differs from the row before; a record is a run, cut every lmax rows and at the tile's end.
//   exact keys (a plain tile whose list overflowed, a partial tile of plain sequence): the minima themselves, hash and
//     position -- the same records as the branch-free walk of a plain tile;
//   value keys (SkValueKeys: everything else): the VALUE of the row's minimum m-mer.  Where one m-mer repeats (poly-A,
//     tandem repeats) the minimum's position moves on row after row while its value stays: runs by value keep such
//     stretches in records of lmax k-mers instead of one record per row.  All k-mers of such a record still share the
//     m-mer's value -- and so all three bucket digits -- but not its place: SK_REC_MULTI.
// The keys are computed row by row as the walk goes (a value key is a 128-bit funnel shift of the lane's bases: kept as
// an array, the 32 of them cost sk_scatter0 65 spilled registers).
template <int W, bool BATCH, bool BYV>
struct SkKeys {
    const SkFront<W> &f;
    u64 lo, hi;                    // BYV: the lane's 64 bases from its first row on
    u32 mmask;
    u32 next_first, prev_last;     // the neighbouring lanes' boundary keys, comparable with this lane's

    __device__ __forceinline__ SkKeys(const SkFront<W> &f_, const u64 *__restrict__ words, u64 n_words, u64 pos0, u32 mmask_)
        : f(f_), lo(0), hi(0), mmask(mmask_)
    {
        if (BYV) {
            // (what sk_front cut its m-mers from, read again: this is the rare path)
            const u64 pos = pos0 + (u64)(threadIdx.x & 63) * 32;
            const u64 w = pos >> 5;
            const unsigned sh = (unsigned)(pos & 31) * 2;
            const u64 w0 = w < n_words ? words[w] : 0, w1 = w + 1 < n_words ? words[w + 1] : 0;
            lo = w0;
            hi = w1;
            if (sh) {
                const u64 w2 = w + 2 < n_words ? words[w + 2] : 0;
                lo = (w0 >> sh) | (w1 << (64 - sh));
                hi = (w1 >> sh) | (w2 << (64 - sh));
            }
            next_first = wave_next((*this)(0));
            prev_last = wave_prev((*this)(31));
        } else {
            next_first = f.next_first;
            prev_last = f.prev_last;
        }
    }
    // (between two sweeps over the rows: the value keys are computed again, not kept -- 32 live keys spill)
    __device__ __forceinline__ void forget()
    {
        if (BYV)
            asm volatile("" : "+v"(lo), "+v"(hi));
    }
    __device__ __forceinline__ u32 operator()(int j) const
    {
        if (!BYV)
            return f.hm[j];
        if (BATCH && f.hm[j] < 64u)
            return ~0u;                            // (a row across a sequence start: no m-mer value is all ones)
        const u32 p = f.hm[j] & SK_GPOS_MASK;     // (<= 31 + W - 1 <= 48: the m-mer lies inside the lane's 64 bases)
        return (u32)sk_shr128(lo, hi, 2u * p) & mmask;
    }
};

// what the walk needs of the lanes before this one: the last break (a row whose key differs from the row before; the
// tile's first row counts) among the lanes' rows -> ns0 = the start row of the run that reaches this lane's first row from
// the left, and c0 = the length so far of the RECORD open there (records are cut every lmax rows of a run)
template <int W, typename Keys>
__device__ __forceinline__ void sk_front_open(SkFront<W> &f, const Keys &key, u32 lmax)
{
    const int lane = threadIdx.x & 63;
    // (opaque to the compiler: else the 32 row numbers r0 + j -- and, where they are widened, their 64-bit forms -- are
    // hoisted out of the callers' tile loops as loop invariants and spilled: sk_scatter0 carried 22 spilled VGPRs and
    // 92 bytes of scratch per lane for them, 0.4 ms of its 3.9 at 3 Gbase)
    u32 r0 = (u32)lane * 32;
    asm volatile("" : "+v"(r0));
    u32 lb = 0;
    u32 kprev = key.prev_last;
    const u32 k0 = key(0);
    u32 kcur = k0;
#pragma unroll 8
    for (int j = 0; j < 32; j++) {
        const bool brk = j == 0 ? (lane == 0 || kcur != kprev) : kcur != kprev;
        if (brk)
            lb = r0 + (u32)j + 1u;
        kprev = kcur;
        if (j < 31)
            kcur = key(j + 1);
    }
    const u32 before = wave_prev(wave_incl_max(lb));       // over the lanes before this one (lane 0: 0)
    // `before` >= 1 for every lane but lane 0 (row 0 is a break); lane 0's own row 0 is a break too
    f.ns0 = before ? before - 1u : 0u;
    const bool first_break = lane == 0 || k0 != key.prev_last;
    f.c0 = first_break ? 0u : (r0 - f.ns0) % lmax;
    if (first_break)
        f.ns0 = r0;
}

// the walk with the callback at EVERY row position (end = a record ends at this thread's row j; false for rows
// that do not exist), so that the callback may use wave-wide operations: emit(j, end, row, len, hmin, key)
template <int W, typename Keys, typename Emit>
__device__ __forceinline__ void sk_records_all(const SkFront<W> &f, const Keys &key, u32 lmax, Emit &&emit)
{
    u32 r0 = (u32)(threadIdx.x & 63) * 32;
    asm volatile("" : "+v"(r0));                  // (see sk_front_open)
    u32 c = f.c0;
    u32 kprev = 0, kcur = key(0);
#pragma unroll 8
    for (int j = 0; j < 32; j++) {
        const u32 nxt = j < 31 ? key(j + 1) : key.next_first;
        bool end = false;
        if ((u32)j < f.n_valid) {
            if (j > 0 && kcur != kprev)
                c = 0;
            end = r0 + (u32)j + 1 == f.n_rows || nxt != kcur || c + 1 == lmax;
        }
        emit(j, end, r0 + (u32)j, c + 1, f.hm[j], kcur);
        c = end ? 0u : c + 1;
        kprev = kcur;
        kcur = nxt;
    }
}

// walks the thread's rows in order and calls emit(j, end_row, len, hmin, key) for every record that ENDS in them (j = the
// row's index among the thread's 32).  (These walks run out of line -- sk_hist0_general, sk_scatter0_general -- over a memory
// copy of the SkFront.  Unrolled eight rows at a time: fully rolled, every row waits for its minimum to come back from scratch
// memory -- a sequence that is half poly-A took 31 ms instead of 24 --; fully unrolled, the walks' registers cost the kernels
// around them theirs.)
template <int W, typename Keys, typename Emit>
__device__ __forceinline__ void sk_records(const SkFront<W> &f, const Keys &key, u32 lmax, Emit &&emit)
{
    u32 r0 = (u32)(threadIdx.x & 63) * 32;
    asm volatile("" : "+v"(r0));                  // (see sk_front_open)
    u32 c = f.c0;
    u32 kprev = 0, kcur = key(0);
#pragma unroll 8
    for (int j = 0; j < 32; j++) {
        const u32 nxt = j < 31 ? key(j + 1) : key.next_first;
        if ((u32)j < f.n_valid) {
            if (j > 0 && kcur != kprev)
                c = 0;                                     // (a break at j == 0 is already in c0)
            const bool last = r0 + (u32)j + 1 == f.n_rows;   // records are cut at the tile's end
            const bool end = last || nxt != kcur || c + 1 == lmax;
            if (end) {
                emit(j, r0 + (u32)j, c + 1, f.hm[j], kcur);
                c = 0;
            } else {
                c++;
            }
        }
        kprev = kcur;
        kcur = nxt;
    }
}

// A FULL tile whose rows all have ONE minimum m-mer value -- poly-A, a microsatellite (the smallest rotation of the unit is
// every window's minimum), a tandem repeat shorter than a window -- needs no walk: by value it is one run, cut every lmax
// rows from the tile's first (exactly what the general walk makes of it, at a few percent of its cost: a sequence that is
// half poly-A spent 5.5 + 7.3 ms in the two level-0 kernels' walks).  Returns that value, or ~0u where the tile is no such
// tile (no m-mer value is all ones).  Equal hashes first (cheap; unequal ones settle it), then the values themselves, cut from
// the lane's bases at every row's minimum: a hash of 25 bits does not vouch for them.  All lanes of the wave call it.
template <int W, bool BATCH>
__device__ __forceinline__ u32 sk_uniform_value(const SkFront<W> &f, const u64 *__restrict__ words, u64 n_words, u64 pos0, u32 mmask)
{
    const int lane = threadIdx.x & 63;
    // (called over the MEMORY copy of the front the general walk takes, loops rolled eight rows at a time: over the front's
    // registers, fully unrolled, it cost sk_scatter0 70 spilled registers and sk_hist0 a wave per SIMD)
    u32 x = 0, y = f.hm[0];
#pragma unroll 2
    for (int j = 1; j < 32; j++) {
        x |= f.hm[j] ^ f.hm[0];
        if (BATCH)
            y &= f.hm[j];
    }
    const u32 h0 = (u32)__builtin_amdgcn_readfirstlane((int)f.hm[0]) >> 7;
    // (BATCH: bit 6 is clear in the minimum of a row that reaches across a sequence start -- such a tile is not uniform)
    const bool same = lane == 63 || ((x >> 7) == 0 && (f.hm[0] >> 7) == h0 && (!BATCH || (y & 64u)));
    if (__ballot(!same))
        return ~0u;
    const u64 pos = pos0 + (u64)lane * 32;
    const u64 w = pos >> 5;
    const unsigned sh = (unsigned)(pos & 31) * 2;
    const u64 w0 = w < n_words ? words[w] : 0, w1 = w + 1 < n_words ? words[w + 1] : 0;
    u64 lo = w0, hi = w1;
    if (sh) {
        const u64 w2 = w + 2 < n_words ? words[w + 2] : 0;
        lo = (w0 >> sh) | (w1 << (64 - sh));
        hi = (w1 >> sh) | (w2 << (64 - sh));
    }
    const u32 v0 = (u32)sk_shr128(lo, hi, 2u * (f.hm[0] & SK_GPOS_MASK)) & mmask;
    u32 d = 0;
#pragma unroll 2
    for (int j = 1; j < 32; j++)
        d |= ((u32)sk_shr128(lo, hi, 2u * (f.hm[j] & SK_GPOS_MASK)) & mmask) ^ v0;
    const u32 V = (u32)__builtin_amdgcn_readfirstlane((int)v0);
    const bool ok = lane == 63 || (d == 0 && v0 == V);
    return __ballot(!ok) ? ~0u : V;
}

// The general walk of sk_hist0 over a MEMORY copy of the front, its loops over the rows unrolled eight at a time: non-plain
// tiles are rare (none on random sequence), and fully unrolled over the front's registers the walk's registers were the
// kernel's (85 -> 128 VGPRs with spills: one wave less per SIMD for every tile).  (As a function of its own -- tried -- every
// call saves and restores the callee-saved registers through scratch: a sequence that is half poly-A took 31 ms.)
template <int W, bool BATCH>
__device__ __forceinline__ void sk_hist0_general(SkFront<W> &f, const u64 *__restrict__ words, u64 n_words, u64 pos0, u32 lmax, u32 mmask,
                                              u32 c0n, u32 *h /* LDS */)
{
    SkKeys<W, BATCH, true> vk(f, words, n_words, pos0, mmask);
    sk_front_open<W>(f, vk, lmax);
    vk.forget();
    if ((threadIdx.x & 63) < 63)
        sk_records<W>(f, vk, lmax, [&](int, u32, u32, u32 hmin, u32 v) {
            if (!BATCH || v != ~0u)
                atomicAdd(&h[sk_digit0(sk_digit_word(hmin), c0n)], 1u);
        });
}

// ------------------------------------------------------------------------------------------------
// sk_hist0: records per coarse digit of every chunk of rows (the histogram the generic prefix kernels take).  The
// chunk's wave tiles go round the workgroup's four waves; the waves meet only at the histogram (LDS adds).
template <int W, bool BATCH>
__global__ __launch_bounds__(SK_NT, 4) void sk_hist0_kernel(const Chunk *__restrict__ chunks, u32 n_chunks,
                                                         const u64 *__restrict__ words, u64 n_words, u64 first,
                                                         u32 lmax, u32 mmask, u32 c0n, u32 b1mask, u32 r0n /* digits of the root's split */,
                                                         u32 *__restrict__ hist, u32 *__restrict__ accum /* or null */,
                                                         const u32 *__restrict__ marks, u64 n_mark_words)
{
    __shared__ u32 h[SK_MAX_C0 + 64];             // (+ a word per lane for the adds that count nothing)
    if (blockIdx.x >= n_chunks)
        return;
    const Chunk ch = chunks[blockIdx.x];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (u32 d = threadIdx.x; d < r0n; d += SK_NT)
        h[d] = 0;
    __syncthreads();
    for (u32 t0 = (u32)wave * SKW_ROWS; t0 < ch.len; t0 += SK_TILE_ROWS) {
        const u32 n_rows = ch.len - t0 < (u32)SKW_ROWS ? ch.len - t0 : (u32)SKW_ROWS;
        SkFront<W> f;
        sk_front<W, BATCH>(f, words, n_words, first + ch.off + t0, n_rows, lmax, mmask, nullptr, marks, n_mark_words);
        bool plain = f.plain;
        const u32 nf = lane == 62 ? ~f.hm[31] : f.next_first;
        if (plain) {                               // (the tile's records if it is cut as a plain tile: sk_scatter0 counts the same)
            u32 cnt = 0;
#pragma unroll
            for (int j = 0; j < 32; j++)
                cnt += ((j < 31 ? f.hm[j + 1] : nf) != f.hm[j]) ? 1u : 0u;
            plain = wave_sum(lane < 63 ? cnt : 0u) <= sk_plain_max(W);
        }
        if (plain) {
            // a record ends at every row whose successor has another minimum -- hash or position -- (lane 62's last row: the
            // tile's end).  No branch per row: a lane whose row ends nothing adds to a word of its own behind the histogram.
            if (lane < 63) {
#pragma unroll
                for (int j = 0; j < 32; j++) {
                    const u32 nxt = j < 31 ? f.hm[j + 1] : nf;
                    const u32 d0 = sk_digit0(sk_digit_word(f.hm[j]), c0n);
                    // (BATCH: a minimum below 64 is an m-mer across a sequence start -- 0 in its own lane, 32 + j seen from the
                    // lane before: such runs are counted and stored nowhere)
                    atomicAdd(&h[nxt != f.hm[j] && (!BATCH || f.hm[j] >= 64u) ? d0 : (u32)SK_MAX_C0 + (u32)lane], 1u);
                }
            }
        } else {
            SkFront<W> fm = f;                     // (a copy in memory for what follows: f itself stays in registers)
            const u32 uv = fm.plain ? sk_uniform_value<W, BATCH>(fm, words, n_words, first + ch.off + t0, mmask) : ~0u;
            if (uv != ~0u) {                       // one run of one m-mer value: its records are the cuts every lmax rows
                if (lane == 0)
                    atomicAdd(&h[sk_digit0(sk_digit_word(fm.hm[0]), c0n)], ((u32)SKW_ROWS + lmax - 1u) / lmax);
            } else {
                sk_hist0_general<W, BATCH>(fm, words, n_words, first + ch.off + t0, lmax, mmask, c0n, h);
            }
        }
    }
    __syncthreads();
    if (accum) {                                   // (the sampled histogram behind a slab sweep: one row for all chunks)
        for (u32 d = threadIdx.x; d < r0n; d += SK_NT)
            if (h[d])
                atomicAdd(&accum[d], h[d]);
        return;
    }
    u32 *row = hist + (u64)blockIdx.x * ROW_STRIDE;
    for (u32 d = threadIdx.x; d < r0n; d += SK_NT)
        row[d] = h[d];
}

// ------------------------------------------------------------------------------------------------
// What building a tile's records needs of its kernel (sk_scatter0): the wave's LDS list and words, the
// chunk's cursors, the record buffer.
struct SkBuild {
    u64 *wl;                // list entries (see sk_build)
    const u64 *wsh;         // the tile's packed words (word 0 = the one holding its first base)
    u32 *gpos;              // per coarse digit: the chunk's next slot
    const u32 *gend;        // ... and the end of its slots (slab mode; else all ones)
    ull2_t *recs;
    u32 fo, c0n, b1mask, mmask;
    int k, dbg;
};

// Every lane builds and stores the records of its share of the list.  exact: the listed records are runs of one minimum,
// hash and position (key = that minimum) -- they carry the minimum m-mer's offset, and the m-mer's value (for d1 / d2) is
// cut from the tile's words there; else (the walk by the m-mer's value: key = that value) SK_REC_MULTI.  Returns true if
// a record found its digit's slots used up (slab mode).
// mode 0: entries key << 32 | start row << 16 | end row, key = the m-mer's value (the walk by value);
// mode 1: the same, key = the minimum itself (the exact walk in four passes);
// mode 2: entries key << 32 | end row IN ROW ORDER, key = the minimum itself (a plain tile): a record starts where its
//         predecessor ended.
template <bool BATCH>
__device__ __forceinline__ bool sk_build(const SkBuild &b, u32 wrun, int mode)
{
    const bool exact = mode != 0;
    const int dbg = b.dbg;
    (void)dbg;
    bool dropped = false;
    if (SK_DBG(2))
        return false;
    for (u32 e = threadIdx.x & 63u; e < wrun; e += 64) {
        const u64 en = b.wl[e];
        const u32 key = (u32)(en >> 32);
        if (BATCH && (exact ? key < 64u : key == ~0u))
            continue;                              // (a run of rows across a sequence start: not rows of the table)
        const u32 end_row = (u32)en & 0xFFFFu;
        u32 v = key, hmin = key;
        if (exact) {                               // the minimum's position counts from the first row of the lane of end_row
            const u32 xq = (end_row & ~31u) + (key & SK_GPOS_MASK) + b.fo;
            v = (u32)funnel(b.wsh[xq >> 5], b.wsh[(xq >> 5) + 1], (xq & 31u) * 2u) & b.mmask;
        } else {
            hmin = sk_hash_of(v);
        }
        const SkDigits dg = sk_digits(hmin, v, b.c0n, b.b1mask);
        const u32 gslot = atomicAdd(&b.gpos[dg.d0], 1u);
        u32 start = ((u32)en >> 16) & 0xFFFFu;
        if (mode == 2)
            start = e ? ((u32)b.wl[e - 1] & 0xFFFFu) + 1u : 0u;
        const u32 len = end_row - start + 1u;
        // the record's 108 payload bits from bit 2 q of the tile's words: six dwords, four funnel shifts
        const u32 q = start + b.fo;                // first base of the run, relative to the tile's first word
        const u32 wi = q >> 5, sh = (q & 15u) * 2u;
        const u64 a0 = b.wsh[wi], a1 = b.wsh[wi + 1], a2 = b.wsh[wi + 2];
        const bool odd = (q & 16u) != 0;
        const u32 e0 = odd ? (u32)(a0 >> 32) : (u32)a0, e1 = odd ? (u32)a1 : (u32)(a0 >> 32),
                  e2 = odd ? (u32)(a1 >> 32) : (u32)a1, e3 = odd ? (u32)a2 : (u32)(a1 >> 32),
                  e4 = odd ? (u32)(a2 >> 32) : (u32)a2;
        u64 lo = ((u64)__builtin_amdgcn_alignbit(e2, e1, sh) << 32) | __builtin_amdgcn_alignbit(e1, e0, sh);
        u64 hi = ((u64)__builtin_amdgcn_alignbit(e4, e3, sh) << 32) | __builtin_amdgcn_alignbit(e3, e2, sh);
        const u32 nb = len + (u32)b.k - 1;
        if (nb < 32) {
            lo &= ((u64)1 << (2 * nb)) - 1;
            hi = 0;
        } else {
            hi &= ((u64)1 << (2 * (nb - 32))) - 1;
        }
        const u32 mpos = (end_row & ~31u) + (key & SK_GPOS_MASK) - start;
        const u32 tag = exact ? (mpos & SK_POS_MASK) << (SK_POS_SHIFT - 32) : 1u << (SK_REC_MULTI_BIT - 32);
        hi |= ((u64)(len - 1) << 44) | ((u64)dg.d1 << 49) | ((u64)dg.d2 << 59) | ((u64)tag << 32);
        ull2_t r;
        r.x = lo;
        r.y = hi;
        if (gslot >= b.gend[dg.d0])
            dropped = true;                        // (slab mode: the chunk's slots of this digit are used up)
        else if (!SK_DBG(1))
            b.recs[gslot] = r;
        else if (r.x == 0x1234567 && r.y == 0x89)
            b.recs[0] = r;
    }
    return dropped;
}

// The general walk of sk_scatter0 (over a memory copy of the front: see sk_hist0_general): a partial tile, or a full one of
// more than sk_plain_max(W) (hash, position) runs (low-complexity sequence) -- records = runs of one m-mer VALUE, cut every lmax
// rows (BYV; the walk by the minima themselves, !BYV, is kept for reference: nothing calls it now).  A list that overflows
// in one pass is redone in four passes of eight row positions each, which always fit.
template <int W, bool BATCH, bool BYV>
__device__ __forceinline__ bool sk_scatter0_walk(SkFront<W> &f, const SkBuild &bx, const u64 *__restrict__ words, u64 n_words,
                                                 u64 tile_pos, u32 lmax)
{
    const u64 below = ((u64)1 << (threadIdx.x & 63)) - 1;
    u64 *wl = bx.wl;
    bool dropped = false;
    SkKeys<W, BATCH, BYV> key(f, words, n_words, tile_pos, bx.mmask);
    sk_front_open<W>(f, key, lmax);
    for (int n_pass = BYV ? 1 : 4, pass = 0; pass < n_pass; pass++) {
        const int jlo = pass * (32 / n_pass), jhi = jlo + 32 / n_pass;
        u32 wrun = 0;
        key.forget();
        sk_records_all<W>(f, key, lmax, [&](int j, bool end_any, u32 end_row, u32 len, u32, u32 kj) {
            const bool end = end_any && j >= jlo && j < jhi;
            const u64 b = __ballot(end);
            if (end) {
                const u32 pos = wrun + (u32)__popcll(b & below);
                if (pos < (u32)SKW_LIST)
                    wl[pos] = ((u64)kj << 32) | ((u64)(end_row + 1 - len) << 16) | (u64)end_row;
            }
            wrun += (u32)__popcll(b);
        });
        if (wrun > (u32)SKW_LIST) {                // (only possible in a single pass)
            n_pass = 4;
            pass = -1;
            sk_wave_fence();
            continue;
        }
        sk_wave_fence();                           // list and words written by other lanes of this wave
        if (sk_build<BATCH>(bx, wrun, BYV ? 0 : 1))
            dropped = true;
        sk_wave_fence();                           // wsh / list are rewritten by the next pass / tile
    }
    return dropped;
}
template <int W, bool BATCH>
__device__ __forceinline__ bool sk_scatter0_general(SkFront<W> &f, const SkBuild &bx, const u64 *__restrict__ words, u64 n_words,
                                                    u64 tile_pos, u32 lmax)
{
    return sk_scatter0_walk<W, BATCH, true>(f, bx, words, n_words, tile_pos, lmax);
}

// ------------------------------------------------------------------------------------------------
// sk_scatter0: the same sweep; every record goes straight to its coarse bucket.  The chunk owns a range of
// every bucket (histogram prefix), so a per-digit cursor in LDS hands out consecutive slots; with at most a few
// dozen coarse digits the open cache lines of a workgroup are few and the 16-byte stores combine in L2.
//   record = lo: bases 0..31 of the run; hi: bases 32..53 (bits 0..43) | (len-1) << 44 | d1 << 49 | d2 << 59
template <int W, bool BATCH>
__global__ __launch_bounds__(SK_NT, 4) void sk_scatter0_kernel(const Chunk *__restrict__ chunks, u32 n_chunks,
                                                            const u64 *__restrict__ words, u64 n_words, u64 first, int k,
                                                            u32 lmax, u32 mmask, u32 c0n, u32 b1mask, u32 r0n,
                                                            const u32 *__restrict__ hist, const u32 *__restrict__ tot,
                                                            ull2_t *__restrict__ recs, int dbg,
                                                            u32 *__restrict__ slab /* or null: see below */,
                                                            const u32 *__restrict__ marks, u64 n_mark_words)
{
    // slab != null: level 0 WITHOUT its histogram sweep.  slab[0 .. r0n) = slots a chunk reserves of every digit's region
    // (the host's estimate from a sampled histogram + slack), slab[SK_MAX_C0 + 16 d] = the digit's global cursor (starts
    // at its region's start), slab[17 SK_MAX_C0 + d] += records the chunk stored, slab[18 SK_MAX_C0] = 1 if a chunk ran out
    // of slots (the caller then runs the exact pair).  The slots a chunk does not use are filled with NULL records (bit 63
    // of the second word), which level 1 skips.
    __shared__ u32 gpos[SK_MAX_C0];               // where the chunk's next record of each digit goes (all waves: LDS adds)
    __shared__ u32 gend[SK_MAX_C0], gbeg[SK_MAX_C0];
    __shared__ u64 wsh_all[SK_NT / 64][66];       // per wave: the tile's packed words -- record payloads are cut from here
    __shared__ u64 list_all[SK_NT / 64][SKW_LIST + 64];   // per wave: the tile's records (see below); + an entry per lane for writes that list nothing
    if (blockIdx.x >= n_chunks)
        return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const Chunk ch = chunks[blockIdx.x];
    if (slab) {
        for (u32 d = tid; d < r0n; d += SK_NT) {
            const u32 cap = slab[d];
            const u32 base = cap ? atomicAdd(&slab[SK_MAX_C0 + 16 * d], cap) : 0u;
            gpos[d] = base;
            gbeg[d] = base;
            gend[d] = base + cap;
        }
    } else {
        const u32 *hrow = hist + (u64)blockIdx.x * ROW_STRIDE;
        const u32 *trow = tot;                     // the root is node 0: its totals row is row 0
        for (u32 d = tid; d < r0n; d += SK_NT) {
            gpos[d] = trow[d] + hrow[d];
            gend[d] = ~0u;
        }
    }
    __syncthreads();
    u64 *wsh = wsh_all[wave], *wl = list_all[wave];
    bool dropped = false;
    SkBuild bx;
    bx.wl = wl;
    bx.wsh = wsh;
    bx.gpos = gpos;
    bx.gend = gend;
    bx.recs = recs;
    bx.fo = 0;
    bx.c0n = c0n;
    bx.b1mask = b1mask;
    bx.mmask = mmask;
    bx.k = k;
    bx.dbg = dbg;
    for (u32 t0 = (u32)wave * SKW_ROWS; t0 < ch.len; t0 += SK_TILE_ROWS) {
        const u32 n_rows = ch.len - t0 < (u32)SKW_ROWS ? ch.len - t0 : (u32)SKW_ROWS;
        const u64 tile_pos = first + ch.off + t0;
        const u32 fo = (u32)(tile_pos & 31);
        SkFront<W> f;
        sk_front<W, BATCH>(f, words, n_words, tile_pos, n_rows, lmax, mmask, wsh, marks, n_mark_words);
        // The records that end in this tile (usually ~225) are listed in the wave's LDS list (ballot + prefix count per
        // row position: no atomics), and every lane then builds the payloads of its share (sk_build) -- building them where
        // they end would run the payload code for all 32 row positions, ~9 times the work.  A tile that would overflow the
        // list (very short runs: low-complexity sequence) is redone in four passes of eight row positions each, which always
        // fit (8 x 63 records).
        bx.fo = fo;
        auto build = [&](u32 wrun, int mode) {
            if (sk_build<BATCH>(bx, wrun, mode))
                dropped = true;
        };
        if (f.plain) {
            // records = natural runs, listed IN ROW ORDER: every lane counts the records that end in its rows (a compare and
            // an add-with-carry per row), one wave scan gives it its first list slot, and a second sweep over its rows writes
            // the entries -- key << 32 | end row -- there; a row that ends nothing (and lane 63, which owns no rows) writes to
            // an entry of its own behind the list.  A record's first row is its predecessor's last + 1 (sk_build), so no
            // start is tracked here.  (Round 3 ranked the ends of every row position across the wave -- ballot, two mbcnt,
            // a popcount -- and tracked every lane's open run: ten vector and three scalar operations per row, seven now.)
            const u32 nf = lane == 62 ? ~f.hm[31] : f.next_first;
            u32 cnt = 0;
#pragma unroll
            for (int j = 0; j < 32; j++)
                cnt += ((j < 31 ? f.hm[j + 1] : nf) != f.hm[j]) ? 1u : 0u;
            cnt = lane < 63 ? cnt : 0u;
            const u32 incl = wave_incl_scan(cnt);
            const u32 wrun = (u32)__builtin_amdgcn_readlane((int)incl, 63);   // wave-uniform: records of the tile
            if (wrun <= sk_plain_max(W)) {
                u32 p = incl - cnt;
                const u32 dummy = (u32)SKW_LIST + (u32)lane;
                u32 r0 = (u32)lane * 32;
                asm volatile("" : "+v"(r0));       // (else the 32 row numbers are held across the tile loop: see sk_front_open)
#pragma unroll
                for (int j = 0; j < 32; j++) {
                    const bool end = ((j < 31 ? f.hm[j + 1] : nf) != f.hm[j]) && lane < 63;
                    wl[end ? p : dummy] = ((u64)f.hm[j] << 32) | (u64)(r0 + (u32)j);
                    p += end ? 1u : 0u;
                }
                sk_wave_fence();                   // list and words written by other lanes of this wave
                build(wrun, 2);
                sk_wave_fence();                   // wsh / list are rewritten by the next tile
                continue;
            }
        }
        // the general walk: a partial tile, or one of too many (hash, position) runs
        {
            SkFront<W> fm = f;                     // (a copy in memory for what follows: f itself stays in registers)
            const SkBuild bm = bx;
            const u32 uv = fm.plain ? sk_uniform_value<W, BATCH>(fm, words, n_words, tile_pos, mmask) : ~0u;
            if (uv != ~0u) {
                // one run of one m-mer value (sk_uniform_value): the records the walk by value would list -- value << 32 |
                // start row << 16 | end row, cut every lmax rows -- written directly
                const u32 n_rec = ((u32)SKW_ROWS + lmax - 1u) / lmax;
                for (u32 e = (u32)lane; e < n_rec; e += 64) {
                    const u32 s0 = e * lmax, e1 = (s0 + lmax < (u32)SKW_ROWS ? s0 + lmax : (u32)SKW_ROWS) - 1u;
                    wl[e] = ((u64)uv << 32) | (u64)((s0 << 16) | e1);
                }
                sk_wave_fence();
                if (sk_build<BATCH>(bm, n_rec, 0))
                    dropped = true;
                sk_wave_fence();
            } else if (sk_scatter0_general<W, BATCH>(fm, bm, words, n_words, tile_pos, lmax)) {
                dropped = true;
            }
        }
    }
    if (slab) {
        if (dropped)
            slab[18 * SK_MAX_C0] = 1u;
        __syncthreads();
        ull2_t null_rec;
        null_rec.x = 0;
        null_rec.y = (unsigned long long)1 << 63;
        for (u32 d = (u32)wave; d < r0n; d += SK_NT / 64) {        // (a wave per digit: four short store chains instead of one long)
            const u32 e = gend[d], u = gpos[d] < e ? gpos[d] : e;
            for (u32 i = u + (u32)lane; i < e; i += 64)
                __builtin_nontemporal_store(null_rec, &recs[i]);
            if (lane == 0 && u > gbeg[d])
                atomicAdd(&slab[17 * SK_MAX_C0 + d], u - gbeg[d]);
        }
    }
}

// the sampled chunks of a slab sweep's estimate: chunk i = rows [i * stride, i * stride + len) of the root
__global__ __launch_bounds__(256) void sk_sample_chunks_kernel(Chunk *__restrict__ chunks, u32 n_chunks, u32 stride, u32 len, u32 n)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_chunks)
        return;
    const u64 off = (u64)i * stride;
    Chunk c;
    c.node = 0;
    c.off = (u32)off;
    c.len = off >= (u64)n ? 0u : (u32)((u64)len < (u64)n - off ? (u64)len : (u64)n - off);
    c.pad = 0;
    chunks[i] = c;
}

// Slots a chunk reserves of a digit's region: the digit's share of a chunk's records by the sampled histogram (est records
// among `sampled` rows; chunks of chunk_rows rows), + 1/32 + six standard deviations + 24, whole 128-byte lines.  Host and
// device share the formula (the host sizes the buffers with it).
__host__ __device__ inline u32 sk_slab_cap_of(u32 est, u64 chunk_rows, u64 sampled)
{
    if (est == 0)
        return 0;                                  // (a digit the sample never saw: a record of it overflows at once -> exact pair)
    const u64 e = ((u64)est * chunk_rows) / sampled + 1;   // (a FULL chunk's share: the last chunk of a sequence may be shorter)
    return (u32)((e + e / 32 + 6 * (u64)sk_isqrt(e) + 24 + 7) & ~(u64)7);
}
u32 sk_slab_cap(u32 est, u64 chunk_rows, u64 sampled) { return sk_slab_cap_of(est, chunk_rows, sampled); }

// slab[] from the sampled histogram est[] (see sk_scatter0_kernel): per-chunk slots, cursors at the regions' starts, the
// counters zeroed; nodes[d] = the coarse node of digit d (its region: n_chunks slabs, NULL records included)
__global__ __launch_bounds__(SK_MAX_C0) void sk_slab_init_kernel(const u32 *__restrict__ est, u32 r0n, u32 chunk_rows, u32 sampled,
                                                                u32 n_chunks, u32 child_meta, u32 *__restrict__ slab,
                                                                Node *__restrict__ nodes)
{
    __shared__ u64 sc[SK_MAX_C0];
    const u32 d = threadIdx.x;
    const u32 cap = d < r0n ? sk_slab_cap_of(est[d], chunk_rows, sampled) : 0u;
    sc[d] = (u64)cap * n_chunks;
    __syncthreads();
    if (d == 0) {
        u64 run = 0;
        for (u32 i = 0; i < (u32)SK_MAX_C0; i++) {
            const u64 c = sc[i];
            sc[i] = run;
            run += c;
        }
        slab[18 * SK_MAX_C0] = 0;
        slab[18 * SK_MAX_C0 + 1] = (u32)(run < 0xFFFFFFFFull ? run : 0xFFFFFFFFull);
    }
    __syncthreads();
    if (d < r0n) {
        const u32 start = (u32)(sc[d] < 0xFFFFFFFFull ? sc[d] : 0xFFFFFFFFull);
        slab[d] = cap;
        slab[SK_MAX_C0 + 16 * d] = start;
        slab[17 * SK_MAX_C0 + d] = 0;
        Node o;
        o.start = start;
        o.len = cap * n_chunks;
        o.meta = child_meta;
        o.split = 0;
        o.prefix = 0;
        o.child_base = 0;
        o.chunk_base = 0;
        nodes[d] = o;
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
template <int W, bool BATCH>
static void launch_front(bool scatter, u32 n_chunks, hipStream_t s, const Chunk *chunks, const u64 *words, u64 n_words,
                         u64 first, int k, u32 lmax, u32 mmask, u32 c0n, u32 b1mask, u32 r0n, u32 *hist, const u32 *tot, void *recs,
                         u32 *aux, const u32 *marks, u64 n_mark_words)
{
    if (scatter)
        hipLaunchKernelGGL((sk_scatter0_kernel<W, BATCH>), dim3(n_chunks), dim3(SK_NT), 0, s, chunks, n_chunks, words, n_words, first,
                           k, lmax, mmask, c0n, b1mask, r0n, hist, tot, reinterpret_cast<ull2_t *>(recs), sk_dbg(), aux, marks,
                           n_mark_words);
    else
        hipLaunchKernelGGL((sk_hist0_kernel<W, BATCH>), dim3(n_chunks), dim3(SK_NT), 0, s, chunks, n_chunks, words, n_words, first,
                           lmax, mmask, c0n, b1mask, r0n, hist, aux, marks, n_mark_words);
}

// (k = 20, round 4: 12 bases, a window of 9 -- 4^12 / 5 ~ 3 M effective minimizer values: even final buckets up to ~2^28 rows,
// which is where the engine is the default for it; longer sequences of 20-mers stay on the tree)
int sk_min_k() { return 20; }
int sk_minimizer_len(int k) { return sk_mlen(k); }

hipError_t launch_sk_level0(bool scatter, const Chunk *chunks, u32 n_chunks, const u64 *words, u64 n_words, u64 first, int k,
                            u32 c0n, u32 b1bits, u32 r0bits, u32 *hist, const u32 *tot, void *recs, hipStream_t s, u32 *aux,
                            const u32 *marks, u64 n_mark_words)
{
    if (n_chunks == 0)
        return hipSuccess;
    const int m = sk_minimizer_len(k);
    const int w = k - m + 1;
    const u32 mmask = (1u << (2 * m)) - 1u;
    const u32 lmax = sk_lmax(k);
    const u32 b1mask = (1u << b1bits) - 1, r0n = 1u << r0bits;
    if (r0n > (u32)SK_MAX_C0)
        return hipErrorInvalidValue;
#define SK_CASE(W_) case W_: \
        if (marks) launch_front<W_, true>(scatter, n_chunks, s, chunks, words, n_words, first, k, lmax, mmask, c0n, b1mask, r0n, hist, tot, recs, aux, marks, n_mark_words); \
        else launch_front<W_, false>(scatter, n_chunks, s, chunks, words, n_words, first, k, lmax, mmask, c0n, b1mask, r0n, hist, tot, recs, aux, nullptr, 0); \
        break;
    switch (w) {
        SK_CASE(9) SK_CASE(10) SK_CASE(11) SK_CASE(12) SK_CASE(13) SK_CASE(14) SK_CASE(15) SK_CASE(16) SK_CASE(17) SK_CASE(18)
    default: return hipErrorInvalidValue;
    }
#undef SK_CASE
    return hipGetLastError();
}

hipError_t launch_sk_sample_chunks(Chunk *chunks, u32 n_chunks, u32 stride, u32 len, u32 n, hipStream_t s)
{
    if (n_chunks == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_sample_chunks_kernel, dim3((n_chunks + 255) / 256), dim3(256), 0, s, chunks, n_chunks, stride, len, n);
    return hipGetLastError();
}

int sk_slab_words() { return 18 * SK_MAX_C0 + 4; }

hipError_t launch_sk_slab_init(const u32 *est, u32 r0bits, u32 chunk_rows, u32 sampled, u32 n_chunks, u32 *slab, Node *nodes,
                               hipStream_t s)
{
    hipLaunchKernelGGL(sk_slab_init_kernel, dim3(1), dim3(SK_MAX_C0), 0, s, est, 1u << r0bits, chunk_rows, sampled, n_chunks,
                       (u32)(32 - r0bits), slab, nodes);
    return hipGetLastError();
}

// ================================================================================================
// Not level 0: sk_count_big, a stage of the tail (sk_tail_kernels.hip), with its launchers.  See the head of this file for
// why it is compiled here.
// ------------------------------------------------------------------------------------------------
// sk_count_big: final buckets that are too long for sk_count but hold FEW DISTINCT keys -- what repeats make: a
// minimizer of a repeated stretch brings thousands to millions of copies of a handful of k-mers into one bucket.  One
// workgroup per bucket sweeps its records tile by tile (512 records) into ONE LDS table that is kept for the whole
// bucket: 8192 eight-byte key slots with 32-bit counts.  Groups leave once, by a sweep of the table, into the
// bucket's output range (same placement rule as sk_count: the scan of the buckets' k-mer counts).  A bucket whose
// distinct keys outgrow the table raises its status: the host sends it through the expansion + tree path instead.
constexpr int SKB_NT = 1024;
constexpr int SKB_SLOTS = 8192;
constexpr int SKB_REC = 512;                     // records per tile
constexpr int SKB_MAXQ = SKB_REC * 8;            // quads of a tile (a record holds at most 32 k-mers)
constexpr u32 SKB_ROUND_CAP = SKB_SLOTS - SKB_NT * SKC_KPT - 64;   // a round of inserts (<= 4096 new keys) starts below this
constexpr u64 SKB_EMPTY = ~(u64)0;
constexpr int SKB_RTAB_BITS = 10;
static_assert((1 << SKB_RTAB_BITS) == SKB_NT, "one record-table slot per thread");

// the table's groups, compacted: eight consecutive slots per thread, wave by wave; returns the number of groups (a count
// of the all-ones key, which the table cannot hold, goes last).  All threads of the workgroup call it.
__device__ __forceinline__ u32 skb_emit(const u64 *tab, const u32 *cnt, u32 n_ones, u32 *wtot, u64 *dst_keys, u32 *dst_counts)
{
    constexpr int WAVES = SKB_NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64 myk[8];
    u32 myc[8], mine = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        myk[j] = tab[tid * 8 + j];
        myc[j] = cnt[tid * 8 + j];
        mine += myk[j] != SKB_EMPTY ? 1u : 0u;
    }
    const u32 inc = wave_incl_scan(mine);
    if (lane == 63)
        wtot[wave] = inc;
    __syncthreads();
    u32 before = 0, D = 0;
    sk_wave_prefix16(wtot, WAVES, wave, lane, before, D);
    u64 o = before + inc - mine;
#pragma unroll
    for (int j = 0; j < 8; j++)
        if (myk[j] != SKB_EMPTY) {
            dst_keys[o] = myk[j];
            dst_counts[o] = myc[j];
            o++;
        }
    if (n_ones && tid == 0) {
        dst_keys[D] = SKB_EMPTY;
        dst_counts[D] = n_ones;
    }
    return D + (n_ones ? 1u : 0u);
}

// Work item = a SLICE of a bucket (SKB_SLICE_REC records): a bucket of one slice is counted and emitted here; a longer
// one (millions of copies of a few k-mers) is swept by several workgroups at once, each leaving the groups of its slice
// in a partial area, and sk_big_merge adds the slices' groups up.
constexpr u32 SKB_SLICE_REC = 128 * SKB_REC;
constexpr u32 SKB_FAILED = ~0u;

__global__ __launch_bounds__(256) void sk_big_slices_kernel(const Node *__restrict__ fin, const u32 *__restrict__ list, u32 n_list,
                                                            u32 *__restrict__ nsl, u32 *__restrict__ msl)
{
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_list)
        return;
    const u32 ns = (fin[list[p]].len + SKB_SLICE_REC - 1) / SKB_SLICE_REC;
    nsl[p] = ns;
    msl[p] = ns > 1 ? ns : 0u;
}

__global__ __launch_bounds__(256) void sk_big_slice_fill_kernel(const u32 *__restrict__ nsl_raw, const u32 *__restrict__ sfirst,
                                                                u32 n_list, u32 *__restrict__ sl_bucket, u32 *__restrict__ sl_idx)
{
    const u32 lane = threadIdx.x & 63;
    const u32 p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n_list)
        return;
    const u32 ns = nsl_raw[p], s0 = sfirst[p];
    for (u32 j = lane; j < ns; j += 64) {
        sl_bucket[s0 + j] = p;
        sl_idx[s0 + j] = j;
    }
}

__global__ __launch_bounds__(SKB_NT) void sk_count_big_kernel(const Node *__restrict__ fin, const u32 *__restrict__ list,
                                                              const u32 *__restrict__ list_off, const u32 *__restrict__ nsl,
                                                              const u32 *__restrict__ mfirst, const u32 *__restrict__ sl_bucket,
                                                              const u32 *__restrict__ sl_idx, u32 n_slices,
                                                              const ull2_t *__restrict__ recs, int k,
                                                              unsigned long long *__restrict__ n_groups,
                                                              u64 *__restrict__ seg_off, u32 *__restrict__ seg_cnt,
                                                              u64 *__restrict__ out_keys, u32 *__restrict__ out_counts,
                                                              u32 *__restrict__ status, u64 *__restrict__ part_keys,
                                                              u32 *__restrict__ part_cnts, u32 *__restrict__ part_n)
{
    constexpr int WAVES = SKB_NT / 64, RWAVES = SKB_REC / 64;
    __shared__ __attribute__((aligned(16))) u64 tab[SKB_SLOTS];
    __shared__ u32 cnt[SKB_SLOTS];
    __shared__ __attribute__((aligned(16))) ull2_t lrec[SKB_REC];
    __shared__ unsigned short ownq[SKB_MAXQ];      // quad -> record | first k-mer / SKC_KPT << 9
    __shared__ u32 wq[RWAVES], wtot[WAVES], wnew[2][WAVES];
    __shared__ u32 mult[SKB_REC];                  // records of the tile equal to this one (counted at the first to arrive)
    __shared__ u32 rtab[SKB_NT];                   // the tile's distinct records: record indices, hashed by content
    __shared__ u32 ones;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 kmask = kmer_mask(k);
    u64 my_groups = 0;
    for (u32 sq = blockIdx.x; sq < n_slices; sq += gridDim.x) {
        const u32 lq = sl_bucket[sq], sj = sl_idx[sq], ns = nsl[lq];
        const u32 li = list[lq];
        const u64 obase = list_off[lq];
        const Node nd = fin[li];
        const u32 r_lo = sj * SKB_SLICE_REC, r_hi = nd.len - r_lo < SKB_SLICE_REC ? nd.len : r_lo + SKB_SLICE_REC;
        if (ns > 1) {
            // the padding of a sliced bucket's output range (as long as its k-mers: hundreds of MB for a bucket of a long
            // repeat) is written by all its slices, a share each, before the merge puts the groups at its start -- one
            // workgroup zeroing 800 MB alone took 13 ms
            const u64 z_lo = (u64)nd.child_base * sj / ns, z_hi = (u64)nd.child_base * (sj + 1) / ns;
            for (u64 i = z_lo + (u64)tid; i < z_hi; i += SKB_NT)
                out_counts[obase + i] = 0;
        }
        for (int q = tid; q < SKB_SLOTS; q += SKB_NT) {
            tab[q] = SKB_EMPTY;
            cnt[q] = 0;
        }
        if (tid == 0)
            ones = 0;
        __syncthreads();
        bool failed = false;
        u32 distinct = 0, rpar = 0;                // (every thread keeps the same count: no shared counter to race on)
        for (u32 t0 = r_lo; t0 < r_hi && !failed; t0 += SKB_REC) {
            // ---- the tile's records into LDS.  A repeat brings the SAME record again and again (the same stretch of
            // sequence cut at the same places): equal records of a tile are expanded once, with a multiplicity.
            u32 nq = 0, qinc = 0;
            ull2_t myr;
            myr.x = myr.y = 0;
            u32 mylen = 0;
            if (tid < SKB_REC) {
                if (t0 + (u32)tid < r_hi) {
                    myr = recs[(u64)nd.start + t0 + tid];
                    mylen = (u32)((myr.y >> 44) & 31) + 1u;
                }
                lrec[tid] = myr;
                mult[tid] = 1u;
            }
            rtab[tid] = SKC_FREE;                  // (SKB_RTAB == SKB_NT slots)
            __syncthreads();
            // equal records of the tile, wherever they stand (the copies of a repeat's records alternate when several of them
            // share a bucket): a small table of record INDICES; a record that finds an equal one ahead of it adds to
            // that one's multiplicity and is not expanded
            bool head = false;
            if (tid < SKB_REC && mylen != 0) {
                u32 hslot = (((u32)myr.x ^ (u32)(myr.x >> 32) ^ (u32)myr.y) * 0x9E3779B1u) >> (32 - SKB_RTAB_BITS);
                for (;;) {
                    const u32 old = atomicCAS(&rtab[hslot], SKC_FREE, (u32)tid);
                    if (old == SKC_FREE) {
                        head = true;
                        break;
                    }
                    const ull2_t other = lrec[old];
                    if (other.x == myr.x && other.y == myr.y) {
                        atomicAdd(&mult[old], 1u);
                        break;
                    }
                    hslot = (hslot + 1) & (u32)(SKB_NT - 1);
                }
            }
            if (tid < SKB_REC) {
                nq = head ? (mylen + SKC_KPT - 1) / SKC_KPT : 0u;
                qinc = wave_incl_scan(nq);
                if (lane == 63)
                    wq[wave] = qinc;
            }
            __syncthreads();
            u32 n_quads = 0, qb = 0;
            sk_wave_prefix16(wq, RWAVES, wave, lane, qb, n_quads);
            if (tid < SKB_REC) {
                const u32 q0 = qb + qinc - nq;
                for (u32 q = 0; q < nq; q++)
                    ownq[q0 + q] = (unsigned short)((u32)tid | (q << 9));
            }
            __syncthreads();
            // ---- rounds of one quad per thread
            for (u32 r0 = 0; r0 < n_quads; r0 += SKB_NT) {
                if (distinct > SKB_ROUND_CAP) {    // the table could fill up inside this round
                    failed = true;
                    break;
                }
                u32 claimed = 0;
                const u32 qi = r0 + (u32)tid;
                if (qi < n_quads) {
                    const u32 e = ownq[qi];
                    const ull2_t rec = lrec[e & 511u];
                    const u32 m = mult[e & 511u];
                    const u32 rl = (u32)((rec.y >> 44) & 31) + 1u;
                    const u32 j0 = (e >> 9) * SKC_KPT;
                    const u64 hi44 = rec.y & (((u64)1 << 44) - 1);
                    u64 slo = funnel(rec.x, hi44, 2 * j0), shi = hi44 >> (2 * j0);
#pragma unroll
                    for (int q = 0; q < SKC_KPT; q++) {
                        if (j0 + (u32)q < rl) {
                            const u64 kv = slo & kmask;
                            slo = (slo >> 2) | (shi << 62);
                            shi >>= 2;
                            if (kv == SKB_EMPTY) {
                                atomicAdd(&ones, m);
                            } else {
                                u32 slot = ((((u32)kv ^ (u32)(kv >> 32)) * 0x9E3779B1u) >> 19) & (u32)(SKB_SLOTS - 1);
                                for (;;) {
                                    const u64 old = atomicCAS(reinterpret_cast<unsigned long long *>(&tab[slot]),
                                                              (unsigned long long)SKB_EMPTY, (unsigned long long)kv);
                                    if (old == SKB_EMPTY || old == kv) {
                                        atomicAdd(&cnt[slot], m);
                                        claimed += old == SKB_EMPTY ? 1u : 0u;
                                        break;
                                    }
                                    slot = (slot + 1) & (u32)(SKB_SLOTS - 1);
                                }
                            }
                        }
                    }
                }
                const u32 wc = wave_sum(claimed);
                if (lane == 0)
                    wnew[rpar][wave] = wc;
                __syncthreads();
                u32 nb = 0, nt = 0;
                sk_wave_prefix16(wnew[rpar], WAVES, wave, lane, nb, nt);
                distinct += nt;
                rpar ^= 1;                         // (the next round writes the other row: slow readers of this one are safe)
            }
            __syncthreads();                       // lrec / ownq are rewritten by the next tile
        }
        if (ns == 1) {
            // ---- the whole bucket was this slice: its groups go to its output range
            if (!failed) {
                const u32 groups = skb_emit(tab, cnt, ones, wtot, out_keys + obase, out_counts + obase);
                for (u32 i = groups + (u32)tid; i < nd.child_base; i += SKB_NT)
                    out_counts[obase + i] = 0;     // padding: the range is as long as the bucket's k-mers
                if (tid == 0) {
                    seg_off[li] = obase;
                    seg_cnt[li] = groups;
                    status[lq] = 0;
                    my_groups += groups;
                }
            } else {
                for (u32 i = tid; i < nd.child_base; i += SKB_NT)
                    out_counts[obase + i] = 0;     // the whole range is padding: the bucket is counted elsewhere
                if (tid == 0) {
                    seg_off[li] = obase;
                    seg_cnt[li] = 0;
                    status[lq] = 1;
                }
            }
        } else {
            // ---- one slice of several: its groups go to its partial area
            const u64 pa = (u64)(mfirst[lq] + sj);
            u32 groups = SKB_FAILED;
            if (!failed)
                groups = skb_emit(tab, cnt, ones, wtot, part_keys + pa * SKB_SLOTS, part_cnts + pa * SKB_SLOTS);
            if (tid == 0)
                part_n[pa] = groups;
        }
        __syncthreads();                           // (tab / cnt / counters are reset by the next slice)
    }
    if (tid == 0 && my_groups)
        atomicAdd(n_groups, (unsigned long long)my_groups);
}

// the groups of a sliced bucket: the slices' partial groups added up in one table (one workgroup per bucket)
__global__ __launch_bounds__(SKB_NT) void sk_big_merge_kernel(const Node *__restrict__ fin, const u32 *__restrict__ list,
                                                              const u32 *__restrict__ list_off, const u32 *__restrict__ nsl,
                                                              const u32 *__restrict__ mfirst, u32 n_list,
                                                              unsigned long long *__restrict__ n_groups,
                                                              u64 *__restrict__ seg_off, u32 *__restrict__ seg_cnt,
                                                              u64 *__restrict__ out_keys, u32 *__restrict__ out_counts,
                                                              u32 *__restrict__ status, const u64 *__restrict__ part_keys,
                                                              const u32 *__restrict__ part_cnts, const u32 *__restrict__ part_n)
{
    constexpr int WAVES = SKB_NT / 64;
    __shared__ __attribute__((aligned(16))) u64 tab[SKB_SLOTS];
    __shared__ u32 cnt[SKB_SLOTS];
    __shared__ u32 wtot[WAVES], wnew[2][WAVES];
    __shared__ u32 ones;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 lq = blockIdx.x;
    if (lq >= n_list)
        return;
    const u32 ns = nsl[lq];
    if (ns <= 1)
        return;
    const u32 li = list[lq];
    const u64 obase = list_off[lq];
    for (int q = tid; q < SKB_SLOTS; q += SKB_NT) {
        tab[q] = SKB_EMPTY;
        cnt[q] = 0;
    }
    if (tid == 0)
        ones = 0;
    __syncthreads();
    bool failed = false;
    u32 distinct = 0, rpar = 0;
    for (u32 j = 0; j < ns && !failed; j++) {
        const u64 pa = (u64)(mfirst[lq] + j);
        const u32 n_e = part_n[pa];
        if (n_e == SKB_FAILED) {
            failed = true;
            break;
        }
        for (u32 r0 = 0; r0 < n_e; r0 += SKB_NT) {
            if (distinct > (u32)(SKB_SLOTS - SKB_NT - 64)) {
                failed = true;
                break;
            }
            u32 claimed = 0;
            const u32 e = r0 + (u32)tid;
            if (e < n_e) {
                const u64 kv = part_keys[pa * SKB_SLOTS + e];
                const u32 m = part_cnts[pa * SKB_SLOTS + e];
                if (kv == SKB_EMPTY) {
                    atomicAdd(&ones, m);
                } else {
                    u32 slot = ((((u32)kv ^ (u32)(kv >> 32)) * 0x9E3779B1u) >> 19) & (u32)(SKB_SLOTS - 1);
                    for (;;) {
                        const u64 old = atomicCAS(reinterpret_cast<unsigned long long *>(&tab[slot]), (unsigned long long)SKB_EMPTY,
                                                  (unsigned long long)kv);
                        if (old == SKB_EMPTY || old == kv) {
                            atomicAdd(&cnt[slot], m);
                            claimed = old == SKB_EMPTY ? 1u : 0u;
                            break;
                        }
                        slot = (slot + 1) & (u32)(SKB_SLOTS - 1);
                    }
                }
            }
            const u32 wc = wave_sum(claimed);
            if (lane == 0)
                wnew[rpar][wave] = wc;
            __syncthreads();
            u32 nb = 0, nt = 0;
            sk_wave_prefix16(wnew[rpar], WAVES, wave, lane, nb, nt);
            distinct += nt;
            rpar ^= 1;
        }
    }
    __syncthreads();
    if (!failed) {
        const u32 groups = skb_emit(tab, cnt, ones, wtot, out_keys + obase, out_counts + obase);   // (the rest of the range: zeroed by the slices)
        if (tid == 0) {
            seg_off[li] = obase;
            seg_cnt[li] = groups;
            status[lq] = 0;
            atomicAdd(n_groups, (unsigned long long)groups);
        }
    } else {
        if (tid == 0) {
            seg_off[li] = obase;
            seg_cnt[li] = 0;
            status[lq] = 1;
        }
    }
}

u32 sk_big_slice_records() { return SKB_SLICE_REC; }
u64 sk_big_partial_slots() { return SKB_SLOTS; }

// lens[i] = nodes[i].len (what the host needs of a node list: 4 of its 32 bytes)
__global__ __launch_bounds__(256) void sk_node_lens_kernel(const Node *__restrict__ nodes, u32 n, u32 *__restrict__ lens)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        lens[i] = nodes[i].len;
}

hipError_t launch_sk_node_lens(const Node *nodes, u32 n, u32 *lens, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_node_lens_kernel, dim3((n + 255) / 256), dim3(256), 0, s, nodes, n, lens);
    return hipGetLastError();
}

hipError_t launch_sk_big_slices(const Node *fin, const u32 *list, u32 n_list, u32 *nsl, u32 *msl, hipStream_t s)
{
    if (n_list == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_big_slices_kernel, dim3((n_list + 255) / 256), dim3(256), 0, s, fin, list, n_list, nsl, msl);
    return hipGetLastError();
}

hipError_t launch_sk_big_slice_fill(const u32 *nsl_raw, const u32 *sfirst, u32 n_list, u32 *sl_bucket, u32 *sl_idx, hipStream_t s)
{
    if (n_list == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_big_slice_fill_kernel, dim3((n_list + 3) / 4), dim3(256), 0, s, nsl_raw, sfirst, n_list, sl_bucket, sl_idx);
    return hipGetLastError();
}

hipError_t launch_sk_count_big(const Node *fin, const u32 *list, const u32 *list_off, const u32 *nsl, const u32 *mfirst,
                               const u32 *sl_bucket, const u32 *sl_idx, u32 n_slices, u32 n_list, const void *recs, int k,
                               u64 *n_groups, u64 *seg_off, u32 *seg_cnt, u64 *out_keys, u32 *out_counts, u32 *status, u64 *part_keys,
                               u32 *part_cnts, u32 *part_n, bool any_sliced, hipStream_t s)
{
    if (n_slices == 0)
        return hipSuccess;
    int dev = 0, n_cu = 256, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
        n_cu = v;
    const u32 grid = std::min<u32>(n_slices, (u32)n_cu);
    hipLaunchKernelGGL(sk_count_big_kernel, dim3(grid), dim3(SKB_NT), 0, s, fin, list, list_off, nsl, mfirst, sl_bucket, sl_idx,
                       n_slices, reinterpret_cast<const ull2_t *>(recs), k, reinterpret_cast<unsigned long long *>(n_groups), seg_off,
                       seg_cnt, out_keys, out_counts, status, part_keys, part_cnts, part_n);
    if (any_sliced)
        hipLaunchKernelGGL(sk_big_merge_kernel, dim3(n_list), dim3(SKB_NT), 0, s, fin, list, list_off, nsl, mfirst, n_list,
                           reinterpret_cast<unsigned long long *>(n_groups), seg_off, seg_cnt, out_keys, out_counts, status,
                           part_keys, part_cnts, part_n);
    return hipGetLastError();
}

}  // namespace dnagpu
