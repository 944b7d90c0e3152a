// quals_kernels.hip -- the kernels of the quality column (dnagpu_quals_*): the validation of a caller's
// bytes, the sweep over a FASTQ text that finds every record's sequence and quality line, the length check, the source of
// every sequence's qualities, the output-centric copy that forms a column from a text or from another column, and the
// overlay of a column on a window of a FASTQ image.  The byte arithmetic is quals_math.hpp's; the chunk load and the error
// minimum are text_device.hpp's, the line roles text_math.hpp's, the segment search take_math.hpp's.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "quals_math.hpp"
#include "take_math.hpp"
#include "text_device.hpp"

namespace dnagpu {

// ---- a caller's bytes, already in the column: one lane per chunk.  res[0] = the minimum of the error words.  The bytes
// behind the column's last are set to zero (the allocation holds whole chunks).
__global__ __launch_bounds__(QUALS_THREADS) void quals_validate_kernel(unsigned char *__restrict__ col, u64 n,
                                                                       unsigned long long *__restrict__ res)
{
    const u64 c = (u64)blockIdx.x * QUALS_THREADS + threadIdx.x, p = c * QUALS_CHUNK;
    u64 err = QUALS_NO_ERROR;
    if (p < n) {
        uint4 *q = reinterpret_cast<uint4 *>(col + p);
        const uint4 w = *q;
        QualsBytes v;
        v.lo = (u64)w.x | ((u64)w.y << 32);
        v.hi = (u64)w.z | ((u64)w.w << 32);
        const u32 have = n - p < QUALS_CHUNK ? (u32)(n - p) : QUALS_CHUNK;
        for (u32 k = have; k-- > 0;)
            if (!quals_valid(quals_get(v, k)))
                err = quals_error_key(p + k, QUALS_ERR_CHAR);
        if (have < QUALS_CHUNK) {
            QualsBytes z = {0, 0};
            for (u32 k = 0; k < have; k++)
                quals_put(z, k, quals_get(v, k));
            *q = make_uint4((u32)z.lo, (u32)(z.lo >> 32), (u32)z.hi, (u32)(z.hi >> 32));
        }
    }
    text_error_min(err, res);
}

// ---- FASTQ, the sweep: TEXT_CHUNK bytes per lane, TEXT_TILE_BYTES per workgroup.  A byte's line index is the number of
// '\n' before it (nl_base: the scanned per-tile counts, *total their sum); a '\n' ends its line and the byte behind it
// begins the next, so every '\n' writes up to two of the four words of a record -- rec[4 r ..] = start and end of the
// sequence line, start and end of the quality line -- and the lane of the text's last byte closes a last line that has no
// '\n'.  Only whole records (r < records) are written, each of them completely.  res[0] = the minimum of the error words: a
// byte of a quality line that is neither a Phred+33 character nor part of the terminator.
__global__ __launch_bounds__(TEXT_THREADS) void quals_lines_kernel(const unsigned char *__restrict__ text, u64 n,
                                                                   const u32 *__restrict__ nl_base, const u32 *__restrict__ total,
                                                                   u32 *__restrict__ rec, unsigned long long *__restrict__ res)
{
    __shared__ u32 before[TEXT_THREADS], wtmp[TEXT_THREADS / 64];
    const u32 tid = threadIdx.x, tile = blockIdx.x;
    const u64 b = (u64)tile * TEXT_TILE_BYTES + (u64)tid * TEXT_CHUNK;
    const u64 records = fastq_lines(*total, text[n - 1] == '\n') / 4;
    u32 valid = 0, nl = 0, cr = 0, bad = 0;
    bool next_nl = false;
    if (b < n) {
        u32 w[8];
        valid = text_low_bits(text_load_words(text, n, b, w));
#pragma unroll
        for (u32 j = 0; j < TEXT_CHUNK; j++) {
            const u32 byte = (w[j >> 2] >> (8 * (j & 3))) & 0xff;
            nl |= (u32)(byte == '\n') << j;
            cr |= (u32)(byte == '\r') << j;
            bad |= (u32)!quals_valid(byte) << j;
        }
        nl &= valid;
        next_nl = n - b > TEXT_CHUNK && text[b + TEXT_CHUNK] == '\n';
    }
    block_scan_value<TEXT_THREADS>((u32)__popc(nl), before, (int)TEXT_THREADS, wtmp, (int)tid);
    const u64 line0 = (u64)nl_base[tile] + before[tid];
    u64 err = QUALS_NO_ERROR;
    if (valid) {
        u32 role[4];
        reads_roles(nl, (u32)line0, role);
        const u32 term = nl | (cr & ((nl >> 1) | ((u32)next_nl << 31)));
        const u32 badq = valid & role[3] & ~term & bad;               // (a truncated record has no quality line)
        if (badq)
            err = quals_error_key(b + (u32)__builtin_ctz(badq), QUALS_ERR_CHAR);
        u64 line = line0;
        u32 m = nl;
        while (m) {
            const u32 j = (u32)__builtin_ctz(m);
            const u64 p = b + j, r = line >> 2, r1 = (line + 1) >> 2;
            const u32 q = (u32)(line & 3), q1 = (u32)((line + 1) & 3);
            if (r < records && (q & 1))
                rec[QUALS_REC_WORDS * r + q] = (u32)p;                       // q = 1: word 1, q = 3: word 3
            if (p + 1 < n && r1 < records && (q1 & 1))
                rec[QUALS_REC_WORDS * r1 + q1 - 1] = (u32)(p + 1);           // q1 = 1: word 0, q1 = 3: word 2
            line++;
            m &= m - 1;
        }
        if (n - b <= TEXT_CHUNK && !((nl >> (u32)(n - 1 - b)) & 1)) {        // the last line has no '\n': it ends at n
            const u64 r = line >> 2;
            if (r < records && (line & 3) == 3)
                rec[QUALS_REC_WORDS * r + 3] = (u32)n;
        }
    }
    text_error_min(err, res);
}

// ---- one thread per record: the two lengths
__global__ __launch_bounds__(QUALS_THREADS) void quals_lengths_kernel(const unsigned char *__restrict__ text, u64 n,
                                                                      const u32 *__restrict__ total, const u32 *__restrict__ rec,
                                                                      unsigned long long *__restrict__ res)
{
    const u64 records = fastq_lines(*total, text[n - 1] == '\n') / 4;
    const u64 r = (u64)blockIdx.x * QUALS_THREADS + threadIdx.x;
    u64 err = QUALS_NO_ERROR;
    if (r < records) {
        const u32 *w = rec + QUALS_REC_WORDS * r;
        const auto byte = [&](u32 i) { return (u32)text[i]; };
        if (quals_line_len(w[0], w[1], n, byte) != quals_line_len(w[2], w[3], n, byte))
            err = quals_error_key(w[2], QUALS_ERR_LENGTH);
    }
    text_error_min(err, res);
}

// ---- one thread per sequence of the table: src_at[s] = where its qualities begin in the text -- src_offset[s] bytes into
// the quality line of record src_record[s] (both null: record s, offset 0).  res[1] = the records; res[2] |= 1 where a record
// is not below them or the sequence's bytes leave its line (such a sequence reads from byte 0 on, and nothing is copied).
__global__ __launch_bounds__(QUALS_THREADS) void quals_sources_kernel(const unsigned char *__restrict__ text, u64 n,
                                                                      const u32 *__restrict__ total, const u32 *__restrict__ rec,
                                                                      const u64 *__restrict__ starts, u64 n_seqs,
                                                                      const u64 *__restrict__ src_record,
                                                                      const u64 *__restrict__ src_offset, u64 *__restrict__ src_at,
                                                                      unsigned long long *__restrict__ res)
{
    const u64 records = fastq_lines(*total, text[n - 1] == '\n') / 4;
    const u64 s = (u64)blockIdx.x * QUALS_THREADS + threadIdx.x;
    if (s == 0)
        res[1] = records;
    bool bad = false;
    if (s < n_seqs) {
        const u64 r = src_record ? src_record[s] : s, off = src_offset ? src_offset[s] : 0, len = starts[s + 1] - starts[s];
        u64 at = 0;
        if (r < records) {
            const u32 *w = rec + QUALS_REC_WORDS * r;
            const u64 line = quals_line_len(w[2], w[3], n, [&](u32 i) { return (u32)text[i]; });
            if (off <= line && len <= line - off)
                at = w[2] + off;
            else
                bad = true;
        } else {
            bad = true;
        }
        src_at[s] = at;
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0)
        atomicOr(&res[2], 1ull);
}

// The chunks of one tile: thread t forms chunk t of the tile; the segment of every chunk's first byte lies in [lo, hi] of the
// three lists (global memory, or the tile's part of them in LDS).  A piece that fills its chunk is loaded as words where
// the words lie inside the source; every other piece byte by byte.
__device__ __forceinline__ void quals_tile_chunks(const u64 *starts, const u64 *src_at, const uint8_t *flip, u64 lo, u64 hi,
                                                  const unsigned char *__restrict__ src, u64 src_n, u64 total,
                                                  unsigned char *__restrict__ out)
{
    const u64 c = (u64)blockIdx.x * QUALS_THREADS + threadIdx.x;
    if (c * QUALS_CHUNK >= total)
        return;
    const u64 seg = take_segment_of(starts, lo, hi, c * QUALS_CHUNK);
    const QualsBytes v = quals_chunk(
        starts, src_at, flip, total, seg, c, [&](u64 i) { return (u32)src[i]; },
        [&](u64 a, bool f, QualsBytes *o) {
            const u32 mis = (u32)(reinterpret_cast<uintptr_t>(src + a) & 3);
            if (a < mis || a - mis + (mis ? 20 : 16) > src_n)
                return false;
            const u32 *q = reinterpret_cast<const u32 *>(src + a - mis);
            u32 d[5];
#pragma unroll
            for (u32 i = 0; i < 4; i++)
                d[i] = q[i];
            d[4] = mis ? q[4] : 0u;
            const QualsBytes w = quals_from_words(d, mis);
            *o = f ? quals_reverse(w) : w;
            return true;
        });
    *reinterpret_cast<uint4 *>(out + c * QUALS_CHUNK) = make_uint4((u32)v.lo, (u32)(v.lo >> 32), (u32)v.hi, (u32)(v.hi >> 32));
}

// ---- the copy.  A workgroup owns the QUALS_TILE_BYTES output bytes from byte blockIdx.x * QUALS_TILE_BYTES on; every lane
// forms one aligned chunk in registers and stores it once, whole.  The workgroup's threads all find the segments of the tile's
// first and last byte (the same loads for every lane); a tile of at most QUALS_LDS_SEGS segments brings their starts,
// sources and flags into LDS and searches there, a tile of more reads them where they are (take_copy_kernel's split).  No
// atomic; no byte of out is assumed to hold anything; no byte of src outside [0, src_n) is read.  n > 0 and total > 0.
__global__ __launch_bounds__(QUALS_THREADS) void quals_copy_kernel(const unsigned char *__restrict__ src, u64 src_n,
                                                                   const u64 *__restrict__ src_at,
                                                                   const uint8_t *__restrict__ seg_flip,
                                                                   const u64 *__restrict__ out_starts, u64 n, u64 total,
                                                                   unsigned char *__restrict__ out)
{
    __shared__ u64 s_starts[QUALS_LDS_SEGS + 1], s_at[QUALS_LDS_SEGS];
    __shared__ uint8_t s_flip[QUALS_LDS_SEGS];
    const u32 tid = threadIdx.x;
    const u64 p_first = (u64)blockIdx.x * QUALS_TILE_BYTES;
    const u64 tile_end = p_first + QUALS_TILE_BYTES;
    const u64 p_last = (tile_end < total ? tile_end : total) - 1;
    const u64 seg_lo = take_segment_of(out_starts, 0, n - 1, p_first);
    const u64 seg_hi = take_segment_of(out_starts, seg_lo, n - 1, p_last);
    const u64 m = seg_hi - seg_lo + 1;
    if (m <= QUALS_LDS_SEGS) {                       // uniform
        for (u32 i = tid; i <= (u32)m; i += QUALS_THREADS)
            s_starts[i] = out_starts[seg_lo + i];
        for (u32 i = tid; i < (u32)m; i += QUALS_THREADS) {
            s_at[i] = src_at[seg_lo + i];
            s_flip[i] = seg_flip ? seg_flip[seg_lo + i] : (uint8_t)0;
        }
        __syncthreads();
        quals_tile_chunks(s_starts, s_at, s_flip, (u64)0, m - 1, src, src_n, total, out);
    } else {
        quals_tile_chunks(out_starts, src_at, seg_flip, seg_lo, seg_hi, src, src_n, total, out);
    }
}

// ---- the overlay on a window of a FASTQ image that export_read_kernel has formed at dst: the bytes of quality lines are
// replaced by the column's.  One lane per 16 bytes of dst, aligned at dst's address: a chunk that lies whole inside the window
// is loaded, changed in registers and stored once; the window's first and last partial chunk store byte by byte, so that no
// byte outside the window is touched.  The quality line of record s is the len_s bytes before its last terminator.
__global__ __launch_bounds__(QUALS_THREADS) void quals_overlay_kernel(const unsigned char *__restrict__ quals,
                                                                      const u64 *__restrict__ starts, const u64 *__restrict__ pos,
                                                                      u64 n, u32 term, u64 first, u64 count,
                                                                      unsigned char *__restrict__ dst)
{
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(dst) & (QUALS_CHUNK - 1));
    const u64 c = (u64)blockIdx.x * QUALS_THREADS + threadIdx.x;
    const u64 lo = c * QUALS_CHUNK, hi = lo + QUALS_CHUNK;           // (offsets from dst - mis)
    const u64 w0 = lo > mis ? lo - mis : 0, w1 = hi - mis < count ? hi - mis : count;
    if (hi <= mis || w0 >= w1)
        return;
    const bool whole = w1 - w0 == QUALS_CHUNK;
    QualsBytes v = {0, 0};
    if (whole) {
        const uint4 w = *reinterpret_cast<const uint4 *>(dst + w0);
        v.lo = (u64)w.x | ((u64)w.y << 32);
        v.hi = (u64)w.z | ((u64)w.w << 32);
    }
    bool changed = false;
    u64 x = first + w0;
    const u64 x1 = first + w1;
    u64 s = take_segment_of(pos, 0, n - 1, x);
    while (x < x1) {
        const u64 next = pos[s + 1], qend = next - term, len = starts[s + 1] - starts[s], qstart = qend - len;
        const u64 a = x > qstart ? x : qstart, e = x1 < qend ? x1 : qend;
        for (u64 y = a; y < e; y++) {
            const u32 byte = quals[starts[s] + (y - qstart)];
            if (whole) {
                const u32 k = (u32)(y - first - w0);
                if (k < 8)
                    v.lo = (v.lo & ~((u64)0xff << (8 * k))) | ((u64)byte << (8 * k));
                else
                    v.hi = (v.hi & ~((u64)0xff << (8 * (k - 8)))) | ((u64)byte << (8 * (k - 8)));
                changed = true;
            } else {
                dst[y - first] = (unsigned char)byte;
            }
        }
        x = next;
        s++;
    }
    if (changed)
        *reinterpret_cast<uint4 *>(dst + w0) = make_uint4((u32)v.lo, (u32)(v.lo >> 32), (u32)v.hi, (u32)(v.hi >> 32));
}

// ================================================================ dnagpu_quals_trim
// A TEAM of lanes handles one sequence: a group of QUALS_GROUP_LANES lanes of one wave, a wave, or a workgroup.  Every lane
// holds one aligned 16-byte chunk of the column in registers (quals_math.hpp's QualsLane); what the lanes know is joined by
// the team: an exclusive scan of the lanes' sums, the first / last lane that has something, a maximum, a sum.  The sub-wave
// teams do it with a ballot and shuffles of their width, the workgroup through LDS.
template <u32 LANES>
struct TrimSub {
    static constexpr u32 lanes = LANES;
    static constexpr bool loops = false;
    __device__ __forceinline__ u32 rank() const { return threadIdx.x & (LANES - 1); }
    __device__ __forceinline__ u32 scan(u32 v, u32 *total) const
    {
        u32 inc = v;
#pragma unroll
        for (u32 off = 1; off < LANES; off <<= 1) {
            const u32 o = __shfl_up(inc, off, LANES);
            if (rank() >= off)
                inc += o;
        }
        *total = __shfl(inc, LANES - 1, LANES);
        return inc - v;
    }
    __device__ __forceinline__ u64 mine(bool has) const      // the team's lanes that have something, lane 0 of the team at bit 0
    {
        const u32 gbase = (threadIdx.x & 63) & ~(LANES - 1);
        const u64 m = __ballot(has) >> gbase;
        return LANES == 64 ? m : m & (((u64)1 << (LANES & 63)) - 1);
    }
    // v of the first / last lane that has one (lanes hold ascending bases), else none
    __device__ __forceinline__ i64 first(bool has, i64 v, i64 none) const
    {
        const u64 m = mine(has);
        const i64 got = __shfl(v, m ? (int)__builtin_ctzll(m) : 0, LANES);
        return m ? got : none;
    }
    __device__ __forceinline__ i64 last(bool has, i64 v, i64 none) const
    {
        const u64 m = mine(has);
        const i64 got = __shfl(v, m ? 63 - (int)__builtin_clzll(m) : 0, LANES);
        return m ? got : none;
    }
    __device__ __forceinline__ i64 max(i64 v) const
    {
#pragma unroll
        for (u32 off = LANES / 2; off > 0; off >>= 1) {
            const i64 o = __shfl_xor(v, off, LANES);
            v = o > v ? o : v;
        }
        return v;
    }
    __device__ __forceinline__ u64 sum(u64 v) const
    {
#pragma unroll
        for (u32 off = LANES / 2; off > 0; off >>= 1)
            v += __shfl_xor(v, off, LANES);
        return v;
    }
};

struct TrimBlock {
    static constexpr u32 lanes = QUALS_THREADS;
    static constexpr bool loops = true;
    u64 *w;                                          // LDS: one word per wave
    u32 *arr, *wtmp;                                 // LDS of block_scan_value
    __device__ __forceinline__ u32 rank() const { return threadIdx.x; }
    __device__ __forceinline__ u32 scan(u32 v, u32 *total) const
    {
        *total = block_scan_value<QUALS_THREADS>(v, arr, (int)QUALS_THREADS, wtmp, (int)threadIdx.x);
        return arr[threadIdx.x];
    }
    template <typename F>
    __device__ __forceinline__ i64 join(i64 v, F &&f) const   // f over the workgroup; synchronises
    {
#pragma unroll
        for (u32 off = 32; off > 0; off >>= 1)
            v = f(v, (i64)__shfl_xor(v, off, 64));
        __syncthreads();                             // (the words of the join before have been read)
        if ((threadIdx.x & 63) == 0)
            w[threadIdx.x >> 6] = (u64)v;
        __syncthreads();
        i64 r = (i64)w[0];
#pragma unroll
        for (u32 i = 1; i < QUALS_THREADS / 64; i++)
            r = f(r, (i64)w[i]);
        return r;
    }
    __device__ __forceinline__ i64 max(i64 v) const
    {
        return join(v, [](i64 a, i64 b) { return a > b ? a : b; });
    }
    __device__ __forceinline__ i64 first(bool has, i64 v, i64 none) const
    {
        const i64 r = -max(has ? -v : -QUALS_NONE);  // (the minimum)
        return r == QUALS_NONE ? none : r;
    }
    __device__ __forceinline__ i64 last(bool has, i64 v, i64 none) const
    {
        const i64 r = max(has ? v : -QUALS_NONE);
        return r == -QUALS_NONE ? none : r;
    }
    __device__ __forceinline__ u64 sum(u64 v) const
    {
        return (u64)join((i64)v, [](i64 a, i64 b) { return (i64)((u64)a + (u64)b); });
    }
};

// what a team makes of one sequence
struct TrimCut {
    i64 start, stop;
    u64 qsum, low;
};

// One tile of the front walk: the lanes' chunks l with qex values before each; (*bestv, *besti) carried in and out.  Returns
// the first base with a negative running sum (QUALS_NONE: none in the tile).
template <typename Team>
__device__ __forceinline__ i64 trim_front_tile(const Team &team, const QualsLane &l, u64 qex, u32 F, i64 *bestv, i64 *besti)
{
    const i64 mine = quals_lane_front_neg(l, qex, F);
    const i64 neg = team.first(mine != QUALS_NONE, mine, QUALS_NONE);
    i64 bv = *bestv, bi = *besti;
    quals_lane_front_best(l, qex, F, neg, &bv, &bi);
    const i64 top = team.max(bv);
    *besti = team.first(bv == top, bi, *besti);
    *bestv = top;
    return neg;
}
// One tile of the tail walk; returns the last base with a negative running sum (-1: none in the tile)
template <typename Team>
__device__ __forceinline__ i64 trim_tail_tile(const Team &team, const QualsLane &l, u64 qex, u64 qtot, u64 n, u32 T, i64 *bestv,
                                              i64 *besti)
{
    const i64 mine = quals_lane_tail_neg(l, qex, qtot, n, T);
    const i64 neg = team.last(mine >= 0, mine, -1);
    i64 bv = *bestv, bi = *besti;
    quals_lane_tail_best(l, qex, qtot, n, T, neg, &bv, &bi);
    const i64 top = team.max(bv);
    *besti = team.last(bv == top, bi, *besti);
    *bestv = top;
    return neg;
}

// The sequence of n bases at column byte base, by the whole team (every lane of it calls; every lane gets the answer).  A
// sequence that lies in one tile of the team -- always so for the sub-wave teams -- is loaded once and stays in registers;
// a longer one (the workgroup only) is swept tile by tile: once for the sum of its values, from the front until the walk
// breaks, from the end until that walk breaks, and over [start, stop) for the sums, each with its carried state.
template <typename Team>
__device__ __forceinline__ TrimCut trim_sequence(const Team &team, const unsigned char *__restrict__ col, u64 base, u64 n,
                                                 const QualsTrimOpt &o)
{
    const u64 c0 = base / QUALS_CHUNK, c_end = (base + n + QUALS_CHUNK - 1) / QUALS_CHUNK;
    const u64 tiles = (c_end - c0 + Team::lanes - 1) / Team::lanes;
    const auto load = [&](u64 c) {
        const uint4 w = *reinterpret_cast<const uint4 *>(col + c * QUALS_CHUNK);
        QualsBytes v;
        v.lo = (u64)w.x | ((u64)w.y << 32);
        v.hi = (u64)w.z | ((u64)w.w << 32);
        return v;
    };
    const auto lane_of = [&](u64 tile) {
        const u64 c = c0 + tile * Team::lanes + team.rank();
        return quals_lane(base, c < c_end ? n : 0, c, load);
    };
    TrimCut r;
    i64 fv = 0, fi = -1, tv = 0, ti = (i64)n;
    if (!Team::loops || tiles <= 1) {
        const QualsLane l = lane_of(0);
        u32 tot = 0;
        const u64 qex = team.scan(quals_lane_sum(l), &tot);
        if (o.cut_front)
            trim_front_tile(team, l, qex, o.cut_front, &fv, &fi);
        if (o.cut_tail)
            trim_tail_tile(team, l, qex, tot, n, o.cut_tail, &tv, &ti);
        r.start = fi + 1;
        r.stop = ti;
        if (r.start >= r.stop)
            r.start = r.stop = 0;
        u64 qs = 0, lw = 0;
        quals_lane_range(l, r.start, r.stop, o.low_q, &qs, &lw);
        r.qsum = team.sum(qs);
        r.low = team.sum(lw);
        return r;
    }
    u64 qtot = 0;
    for (u64 t = 0; t < tiles; t++)
        qtot += quals_lane_sum(lane_of(t));
    qtot = team.sum(qtot);
    if (o.cut_front) {
        u64 before = 0;
        for (u64 t = 0; t < tiles; t++) {
            const QualsLane l = lane_of(t);
            u32 tot = 0;
            const u64 qex = before + team.scan(quals_lane_sum(l), &tot);
            if (trim_front_tile(team, l, qex, o.cut_front, &fv, &fi) != QUALS_NONE)
                break;                               // (uniform: every lane has the team's answer)
            before += tot;
        }
    }
    if (o.cut_tail) {
        u64 behind = 0;                              // the values of the tiles behind this one
        for (u64 t = tiles; t-- > 0;) {
            const QualsLane l = lane_of(t);
            u32 tot = 0;
            const u64 in_tile = team.scan(quals_lane_sum(l), &tot);
            const u64 qex = qtot - behind - tot + in_tile;
            if (trim_tail_tile(team, l, qex, qtot, n, o.cut_tail, &tv, &ti) >= 0)
                break;
            behind += tot;
        }
    }
    r.start = fi + 1;
    r.stop = ti;
    if (r.start >= r.stop)
        r.start = r.stop = 0;
    u64 qs = 0, lw = 0;
    if (r.stop > r.start) {
        const u64 t0 = ((base + (u64)r.start) / QUALS_CHUNK - c0) / Team::lanes;
        const u64 t1 = ((base + (u64)r.stop - 1) / QUALS_CHUNK - c0) / Team::lanes;
        for (u64 t = t0; t <= t1; t++)
            quals_lane_range(lane_of(t), r.start, r.stop, o.low_q, &qs, &lw);
    }
    r.qsum = team.sum(qs);
    r.low = team.sum(lw);
    return r;
}

struct TrimOut {
    u64 *first, *len, *qsum, *low;                   // per sequence, none null
};
__device__ __forceinline__ void trim_store(const TrimOut &out, u64 s, u64 base, const TrimCut &r)
{
    out.first[s] = base + (u64)r.start;
    out.len[s] = (u64)(r.stop - r.start);
    out.qsum[s] = r.qsum;
    out.low[s] = r.low;
}

// ---- the reads: a group of QUALS_GROUP_LANES lanes per sequence, sequence = the group's index in the grid.  A sequence of
// more than QUALS_GROUP_BASES bases is handed on: its id goes into the wave list or the workgroup list (lists[0 .. n_seqs)
// and lists[n_seqs .. 2 n_seqs); counts[0], counts[1] zero before the launch), one atomic per such sequence.
__global__ __launch_bounds__(QUALS_THREADS) void quals_trim_group_kernel(const unsigned char *__restrict__ col,
                                                                         const u64 *__restrict__ starts, u64 n_seqs,
                                                                         const QualsTrimOpt o, const TrimOut out,
                                                                         u32 *__restrict__ lists, u32 *__restrict__ counts)
{
    const TrimSub<QUALS_GROUP_LANES> team;
    const u64 s = ((u64)blockIdx.x * QUALS_THREADS + threadIdx.x) / QUALS_GROUP_LANES;
    u64 base = 0, n = 0;
    if (s < n_seqs) {
        base = starts[s];
        n = starts[s + 1] - base;
    }
    const bool longer = n > QUALS_GROUP_BASES;
    if (longer && team.rank() == 0) {
        const u32 cls = n > QUALS_WAVE_BASES ? 1u : 0u;
        lists[(u64)cls * n_seqs + atomicAdd(&counts[cls], 1u)] = (u32)s;
    }
    const TrimCut r = trim_sequence(team, col, base, longer ? 0 : n, o);     // (every lane of the wave takes part in the joins)
    if (s < n_seqs && !longer && team.rank() == 0)
        trim_store(out, s, base, r);
}

// ---- the sequences of the wave list: one wave each, the waves of the grid stride over the list
__global__ __launch_bounds__(QUALS_THREADS) void quals_trim_wave_kernel(const unsigned char *__restrict__ col,
                                                                        const u64 *__restrict__ starts, const QualsTrimOpt o,
                                                                        const TrimOut out, const u32 *__restrict__ list,
                                                                        const u32 *__restrict__ count)
{
    const TrimSub<64> team;
    const u32 waves = gridDim.x * (QUALS_THREADS / 64), m = *count;
    for (u32 j = blockIdx.x * (QUALS_THREADS / 64) + (threadIdx.x >> 6); j < m; j += waves) {      // (uniform in the wave)
        const u64 s = list[j], base = starts[s], n = starts[s + 1] - base;
        const TrimCut r = trim_sequence(team, col, base, n, o);
        if (team.rank() == 0)
            trim_store(out, s, base, r);
    }
}

// ---- the sequences of the workgroup list: one workgroup each, of any length
__global__ __launch_bounds__(QUALS_THREADS) void quals_trim_block_kernel(const unsigned char *__restrict__ col,
                                                                         const u64 *__restrict__ starts, const QualsTrimOpt o,
                                                                         const TrimOut out, const u32 *__restrict__ list,
                                                                         const u32 *__restrict__ count)
{
    __shared__ u64 w[QUALS_THREADS / 64];
    __shared__ u32 arr[QUALS_THREADS], wtmp[QUALS_THREADS / 64];
    const TrimBlock team = {w, arr, wtmp};
    const u32 m = *count;
    for (u32 j = blockIdx.x; j < m; j += gridDim.x) {                        // (uniform in the workgroup)
        const u64 s = list[j], base = starts[s], n = starts[s + 1] - base;
        const TrimCut r = trim_sequence(team, col, base, n, o);
        if (threadIdx.x == 0)
            trim_store(out, s, base, r);
    }
}

// ---- the verdicts: one thread per sequence (grid-stride).  flags[s] = the sequence passes; res += {passed, bases kept,
// bases cut in front, bases cut at the tail, failed short, failed mean, failed low}, one atomic per wave and word.
constexpr u32 QUALS_TRIM_RES = 7;
__global__ __launch_bounds__(QUALS_THREADS) void quals_verdict_kernel(const u64 *__restrict__ starts, u64 n_seqs, const QualsTrimOpt o,
                                                                      const TrimOut out, u32 *__restrict__ flags,
                                                                      unsigned long long *__restrict__ res)
{
    u64 acc[QUALS_TRIM_RES] = {};
    for (u64 s = (u64)blockIdx.x * QUALS_THREADS + threadIdx.x; s < n_seqs; s += (u64)gridDim.x * QUALS_THREADS) {
        const u64 a = starts[s], n = starts[s + 1] - a, first = out.first[s], len = out.len[s];
        const u32 v = quals_verdict(len, out.qsum[s], out.low[s], o);
        flags[s] = v == QUALS_PASS;
        acc[0] += v == QUALS_PASS;
        acc[1] += len;
        acc[2] += first - a;
        acc[3] += n - (first - a) - len;
        acc[4] += v == QUALS_FAIL_SHORT;
        acc[5] += v == QUALS_FAIL_MEAN;
        acc[6] += v == QUALS_FAIL_LOW;
    }
#pragma unroll
    for (u32 i = 0; i < QUALS_TRIM_RES; i++) {
        u64 v = acc[i];
        for (u32 off = 32; off > 0; off >>= 1)
            v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v)
            atomicAdd(&res[i], (unsigned long long)v);
    }
}

// ---- the passing sequences in table order: rank = the scanned flags; at most cap entries; any list may be null
__global__ __launch_bounds__(QUALS_THREADS) void quals_segments_kernel(const u32 *__restrict__ flags, const u32 *__restrict__ rank,
                                                                       const TrimOut out, u64 n_seqs, u64 cap,
                                                                       u64 *__restrict__ seg_seq, u64 *__restrict__ seg_first,
                                                                       u64 *__restrict__ seg_len)
{
    const u64 s = (u64)blockIdx.x * QUALS_THREADS + threadIdx.x;
    if (s >= n_seqs || !flags[s] || rank[s] >= cap)
        return;
    const u32 at = rank[s];
    if (seg_seq)
        seg_seq[at] = s;
    if (seg_first)
        seg_first[at] = out.first[s];
    if (seg_len)
        seg_len[at] = out.len[s];
}

hipError_t launch_quals_trim(const unsigned char *col, const u64 *starts, u64 n_seqs, const QualsTrimOpt &o, u64 *first, u64 *len,
                             u64 *qsum, u64 *low, u32 *lists, u32 *counts2, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(counts2, 0, 2 * sizeof(u32), s);
    if (e != hipSuccess || n_seqs == 0)
        return e;
    const TrimOut out = {first, len, qsum, low};
    const u64 groups_per_block = QUALS_THREADS / QUALS_GROUP_LANES;
    hipLaunchKernelGGL(quals_trim_group_kernel, dim3((unsigned)((n_seqs + groups_per_block - 1) / groups_per_block)), dim3(QUALS_THREADS),
                       0, s, col, starts, n_seqs, o, out, lists, counts2);
    // (the longer sequences: grids of a fixed size that stride over the lists, whose lengths only the device knows)
    const u64 waves = (n_seqs + QUALS_THREADS / 64 - 1) / (QUALS_THREADS / 64);
    hipLaunchKernelGGL(quals_trim_wave_kernel, dim3((unsigned)(waves < 1024 ? waves : 1024)), dim3(QUALS_THREADS), 0, s, col, starts, o,
                       out, lists, counts2);
    hipLaunchKernelGGL(quals_trim_block_kernel, dim3((unsigned)(n_seqs < 1024 ? n_seqs : 1024)), dim3(QUALS_THREADS), 0, s, col, starts, o,
                       out, lists + n_seqs, counts2 + 1);
    return hipGetLastError();
}

hipError_t launch_quals_verdict(const u64 *starts, u64 n_seqs, const QualsTrimOpt &o, const u64 *first, const u64 *len, const u64 *qsum,
                                const u64 *low, u32 *flags, unsigned long long *res7, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(res7, 0, QUALS_TRIM_RES * sizeof(unsigned long long), s);
    if (e != hipSuccess || n_seqs == 0)
        return e;
    const TrimOut out = {const_cast<u64 *>(first), const_cast<u64 *>(len), const_cast<u64 *>(qsum), const_cast<u64 *>(low)};
    const u64 blocks = (n_seqs + QUALS_THREADS - 1) / QUALS_THREADS;
    hipLaunchKernelGGL(quals_verdict_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(QUALS_THREADS), 0, s, starts, n_seqs, o,
                       out, flags, res7);
    return hipGetLastError();
}

hipError_t launch_quals_segments(const u32 *flags, const u32 *rank, const u64 *first, const u64 *len, u64 n_seqs, u64 cap, u64 *seg_seq,
                                 u64 *seg_first, u64 *seg_len, hipStream_t s)
{
    if (n_seqs == 0 || cap == 0 || (!seg_seq && !seg_first && !seg_len))
        return hipSuccess;
    const TrimOut out = {const_cast<u64 *>(first), const_cast<u64 *>(len), nullptr, nullptr};
    hipLaunchKernelGGL(quals_segments_kernel, dim3((unsigned)((n_seqs + QUALS_THREADS - 1) / QUALS_THREADS)), dim3(QUALS_THREADS), 0, s,
                       flags, rank, out, n_seqs, cap, seg_seq, seg_first, seg_len);
    return hipGetLastError();
}

hipError_t launch_quals_validate(unsigned char *col, u64 n, unsigned long long *res, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    const u64 blocks = (quals_chunks(n) + QUALS_THREADS - 1) / QUALS_THREADS;
    hipLaunchKernelGGL(quals_validate_kernel, dim3((unsigned)blocks), dim3(QUALS_THREADS), 0, s, col, n, res);
    return hipGetLastError();
}

hipError_t launch_quals_lines(const unsigned char *text, u64 n, u32 n_tiles, const u32 *nl_base, const u32 *total, u32 *rec,
                              unsigned long long *res, hipStream_t s)
{
    hipLaunchKernelGGL(quals_lines_kernel, dim3(n_tiles), dim3(TEXT_THREADS), 0, s, text, n, nl_base, total, rec, res);
    return hipGetLastError();
}

hipError_t launch_quals_lengths(const unsigned char *text, u64 n, const u32 *total, const u32 *rec, u64 records_cap,
                                unsigned long long *res, hipStream_t s)
{
    if (records_cap == 0)
        return hipSuccess;
    const u64 blocks = (records_cap + QUALS_THREADS - 1) / QUALS_THREADS;
    hipLaunchKernelGGL(quals_lengths_kernel, dim3((unsigned)blocks), dim3(QUALS_THREADS), 0, s, text, n, total, rec, res);
    return hipGetLastError();
}

hipError_t launch_quals_sources(const unsigned char *text, u64 n, const u32 *total, const u32 *rec, const u64 *starts, u64 n_seqs,
                                const u64 *src_record, const u64 *src_offset, u64 *src_at, unsigned long long *res, hipStream_t s)
{
    const u64 blocks = n_seqs ? (n_seqs + QUALS_THREADS - 1) / QUALS_THREADS : 1;      // (thread 0 hands the records back)
    hipLaunchKernelGGL(quals_sources_kernel, dim3((unsigned)blocks), dim3(QUALS_THREADS), 0, s, text, n, total, rec, starts, n_seqs,
                       src_record, src_offset, src_at, res);
    return hipGetLastError();
}

hipError_t launch_quals_copy(const unsigned char *src, u64 src_n, const u64 *src_at, const uint8_t *seg_flip, const u64 *out_starts,
                             u64 n, u64 total, unsigned char *out, hipStream_t s)
{
    if (n == 0 || total == 0)
        return hipSuccess;
    hipLaunchKernelGGL(quals_copy_kernel, dim3((unsigned)quals_tiles(total)), dim3(QUALS_THREADS), 0, s, src, src_n, src_at, seg_flip,
                       out_starts, n, total, out);
    return hipGetLastError();
}

hipError_t launch_quals_overlay(const unsigned char *quals, const u64 *starts, const u64 *pos, u64 n, u32 term, u64 first,
                                u64 count, unsigned char *dst, hipStream_t s)
{
    if (n == 0 || count == 0)
        return hipSuccess;
    const u64 mis = reinterpret_cast<uintptr_t>(dst) & (QUALS_CHUNK - 1);
    const u64 chunks = (mis + count + QUALS_CHUNK - 1) / QUALS_CHUNK;
    hipLaunchKernelGGL(quals_overlay_kernel, dim3((unsigned)((chunks + QUALS_THREADS - 1) / QUALS_THREADS)), dim3(QUALS_THREADS), 0, s,
                       quals, starts, pos, n, term, first, count, dst);
    return hipGetLastError();
}

}  // namespace dnagpu
