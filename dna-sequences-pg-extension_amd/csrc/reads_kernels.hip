// reads_kernels.hip -- the kernels of dnagpu_reads_from_text: FASTQ and real FASTA into a resident table.
// The shape is dnagpu_table_from_text's (text_kernels.hip): TEXT_CHUNK bytes per lane, TEXT_TILE_BYTES per workgroup, two
// sweeps over the text with scans between them, and no lane ever walks a line or a record.  The bit arithmetic of one lane's
// bytes is text_math.hpp's, the load, the FASTA record closing and the LDS packing are text_device.hpp's.
//
// What the general entry adds to the state a byte's meaning depends on:
//   FASTQ   the role of a line is its index mod 4, and a byte's line index is the number of '\n' before it:
//           reads_newlines_kernel counts them per tile, an additive scan over the tiles and one inside the tile do the rest.
//           The cut of DNAGPU_TEXT_MORE and the truncated record come from the same counts (reads_fastq_cut_kernel).
//   SPLIT   a kept base begins a piece iff no kept base lies between it and the last break (an ambiguity letter of a sequence
//           line, or a record opener) at or before it: two "last ... before" keys, inside the tile by text_block_max_before,
//           across tiles by a maximum scan.  The one start per tile that the tile cannot decide is added to its count by
//           reads_finish_kernel and decided again, from the same scans, by the pack sweep.
//   DROP and min_bases leave sequences out after the pack: reads_select_kernel / reads_move_kernel make the segment list
//           that take_kernels.hip's copy gathers.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "text_device.hpp"

namespace dnagpu {

__device__ __forceinline__ ReadsChunk reads_load(const unsigned char *__restrict__ text, u64 n, u64 b, bool fold)
{
    ReadsChunk r = {};
    if (b >= n)
        return r;
    u32 w[8];
    const u32 have = text_load_words(text, n, b, w);
    r.c.valid = text_low_bits(have);
#pragma unroll
    for (u32 j = 0; j < TEXT_CHUNK; j++)
        reads_chunk_byte(r, j, (w[j >> 2] >> (8 * (j & 3))) & 0xff, fold);
    r.c.prev_nl = b == 0 || text[b - 1] == '\n';
    r.c.next_nl = n - b > TEXT_CHUNK && text[b + TEXT_CHUNK] == '\n';
    return r;
}

// What the two sweeps make of a lane's chunk, alike.
struct ReadsLane {
    ReadsChunk c;
    u32 starts, headers;      // line starts; those of header lines (FASTA)
    u32 keep, amb;            // bases of the result; ambiguity letters of sequence lines (none under DNAGPU_AMBIG_ERROR)
    u32 rec;                  // first bytes of records (LINES: line starts, FASTA: header starts, FASTQ: starts of role 0)
    u32 invalid, empty;       // invalid characters of sequence lines; sequence lines that begin with their terminator
    u32 bad_open;             // FASTQ: a role-0 line without '@', a role-2 line without '+'
    u32 keep_before, rec_before, keep_tile, rec_tile;     // exclusive ranks inside the tile, and the tile's totals
};
struct ReadsLds {
    u32 keep[TEXT_THREADS], rec[TEXT_THREADS], aux[TEXT_THREADS];
    u32 wk[TEXT_THREADS / 64], wr[TEXT_THREADS / 64], wa[TEXT_THREADS / 64], wmax[TEXT_THREADS / 64];
    u32 sum[4];
};

template <int FORMAT>
__device__ __forceinline__ ReadsLane reads_lane(const ReadsSweep &a, u64 n, u64 b, ReadsLds &s)
{
    const u32 tid = threadIdx.x, tile = blockIdx.x;
    ReadsLane l;
    l.c = reads_load(a.text, n, b, a.fold != 0);
    const TextChunk &c = l.c.c;
    l.starts = text_line_starts(c);
    l.headers = 0;
    l.bad_open = 0;
    u32 seqline = c.valid;                           // the bytes of sequence lines
    if (FORMAT == TEXT_FORMAT_FASTA) {
        l.headers = l.starts & c.gt;
        const u32 key = l.starts ? ((tid + 1) << 1) | ((l.headers >> text_top_bit(l.starts)) & 1) : 0u;
        const u32 before = text_block_max_before(key, s.wmax);
        const bool in_header = before ? (before & 1) != 0 : (a.in_state[tile] & 1) != 0;
        seqline &= ~text_header_bytes(l.starts, l.headers, in_header);
        l.rec = l.headers;
    } else if (FORMAT == TEXT_FORMAT_FASTQ) {
        block_scan_value<TEXT_THREADS>((u32)__popc(c.nl), s.aux, (int)TEXT_THREADS, s.wa, (int)tid);
        u32 role[4];
        reads_roles(c.nl, a.line_base[tile] + s.aux[tid], role);
        l.rec = l.starts & role[0];
        l.bad_open = (l.rec & ~l.c.at) | (l.starts & role[2] & ~l.c.plus);
        seqline &= role[1];
    } else {
        l.rec = l.starts;
    }
    const u32 term = text_terminators(c);
    l.keep = c.base & seqline;
    l.amb = a.ambiguous != READS_AMBIG_ERROR ? l.c.amb & seqline : 0u;
    l.invalid = seqline & ~c.base & ~term & ~l.amb;
    l.empty = FORMAT == TEXT_FORMAT_FASTA ? 0u : l.starts & seqline & term;
    l.keep_tile = block_scan_value<TEXT_THREADS>((u32)__popc(l.keep), s.keep, (int)TEXT_THREADS, s.wk, (int)tid);
    l.rec_tile = block_scan_value<TEXT_THREADS>((u32)__popc(l.rec), s.rec, (int)TEXT_THREADS, s.wr, (int)tid);
    l.keep_before = s.keep[tid];
    l.rec_before = s.rec[tid];
    return l;
}

// *acc (LDS, zero before, read after a __syncthreads) += the sum of v over the workgroup
__device__ __forceinline__ void reads_block_add(u32 v, u32 *acc)
{
#pragma unroll
    for (u32 off = 32; off > 0; off >>= 1)
        v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0 && v)
        atomicAdd(acc, v);
}

// SPLIT: the piece starts of the lane's chunk that the tile decides, *und the one it cannot; *kkey / *bkey / *k_before /
// *b_before: the lane's last kept base / break and those before it (positions inside the tile + 1).  Synchronises.
__device__ __forceinline__ u32 reads_lane_pieces(const ReadsLane &l, ReadsLds &s, u32 *und, u32 *kkey, u32 *bkey, u32 *k_before,
                                                 u32 *b_before)
{
    const u32 at = threadIdx.x * TEXT_CHUNK + 1, brk = l.amb | l.rec;
    *kkey = l.keep ? at + text_top_bit(l.keep) : 0u;
    *bkey = brk ? at + text_top_bit(brk) : 0u;
    *k_before = text_block_max_before(*kkey, s.wmax);
    *b_before = text_block_max_before(*bkey, s.wmax);
    return reads_piece_starts(l.keep, brk, at, *k_before, *b_before, und);
}

// ---- FASTQ, before everything: nl_t[tile] = the '\n' of the tile
__global__ __launch_bounds__(TEXT_THREADS) void reads_newlines_kernel(const unsigned char *__restrict__ text, u64 n, u32 *__restrict__ nl_t)
{
    __shared__ u32 sum;
    if (threadIdx.x == 0)
        sum = 0;
    __syncthreads();
    const TextChunk c = text_load(text, n, (u64)blockIdx.x * TEXT_TILE_BYTES + (u64)threadIdx.x * TEXT_CHUNK);
    reads_block_add((u32)__popc(c.nl), &sum);
    __syncthreads();
    if (threadIdx.x == 0)
        nl_t[blockIdx.x] = sum;
}

// ---- FASTQ: one past the '\n' that ends the last whole record (fastq_cut_newline; 0: there is none).  With `more` it
// becomes *lim; without, it is where a truncated record is reported (lines no multiple of four).  nl_base: the scanned
// nl_t, *total their sum.  One workgroup per tile; only the tile that holds that '\n' reads the text.
__global__ __launch_bounds__(TEXT_THREADS) void reads_fastq_cut_kernel(const unsigned char *__restrict__ text, u64 n,
                                                                       const u32 *__restrict__ nl_t, const u32 *__restrict__ nl_base,
                                                                       const u32 *__restrict__ total, int more, u64 *__restrict__ lim,
                                                                       unsigned long long *__restrict__ res)
{
    __shared__ u32 arr[TEXT_THREADS], wtmp[TEXT_THREADS / 64];
    const u32 tid = threadIdx.x, tile = blockIdx.x;
    const u64 newlines = *total;
    const bool ends = text[n - 1] == '\n';
    if (!more && fastq_lines(newlines, ends) % 4 == 0)
        return;
    const u64 want = fastq_cut_newline(newlines, ends, more != 0);
    u64 cut = ~(u64)0;
    if (want == 0) {
        if (tile == 0 && tid == 0)
            cut = 0;
    } else {
        if (!(nl_base[tile] < want && want <= (u64)nl_base[tile] + nl_t[tile]))
            return;                                  // (uniform)
        const u64 b = (u64)tile * TEXT_TILE_BYTES + (u64)tid * TEXT_CHUNK;
        const TextChunk c = text_load(text, n, b);
        const u32 cnt = (u32)__popc(c.nl);
        block_scan_value<TEXT_THREADS>(cnt, arr, (int)TEXT_THREADS, wtmp, (int)tid);
        const u64 before = (u64)nl_base[tile] + arr[tid];
        if (before < want && want <= before + cnt)
            cut = b + text_nth_bit(c.nl, (u32)(want - before)) + 1;
    }
    if (cut == ~(u64)0)
        return;
    if (more)
        *lim = cut;
    else
        atomicMin(res, (unsigned long long)text_error_key(cut, TEXT_ERR_TRUNC));
}

// ---- FASTQ, after an error at byte e: out3[0] = the record e belongs to (its line / 4), out3[1] = the byte, out3[2] = the
// role of its line.  One workgroup, over e's tile.
__global__ __launch_bounds__(TEXT_THREADS) void reads_fastq_rank_kernel(const unsigned char *__restrict__ text, u64 n,
                                                                        const u32 *__restrict__ nl_base, u64 e, u64 *__restrict__ out3)
{
    __shared__ u32 count;
    if (threadIdx.x == 0)
        count = 0;
    __syncthreads();
    const u64 tile = e / TEXT_TILE_BYTES, b = tile * TEXT_TILE_BYTES + (u64)threadIdx.x * TEXT_CHUNK;
    const TextChunk c = text_load(text, n, b);
    u32 nl = c.nl;
    if (b > e)
        nl = 0;
    else if (e - b < TEXT_CHUNK)
        nl &= text_low_bits((u32)(e - b));           // the '\n' before e
    if (nl)
        atomicAdd(&count, (u32)__popc(nl));
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 line = (u64)nl_base[tile] + count;
        out3[0] = line / 4;
        out3[1] = text[e];
        out3[2] = line & 3;
    }
}

// ---- the first sweep.  Per tile: keep_t = bases kept, rec_t = records begun; res[0] = the minimum of the error words,
// res[4] += the ambiguity letters of sequence lines.  FASTA: text_sweep_kernel's per-tile words for text_finish_kernel, where
// an ambiguity letter that the policy admits makes a record non-empty.  SPLIT: piece_t = the piece starts the tile decides,
// sc_t = its sequence characters (kept bases and ambiguity letters), last_keep / last_brk = its last kept base / break
// (offset + 1, 0: none), undecided = it holds a start that the tiles before decide.
template <int FORMAT, bool SPLIT>
__global__ __launch_bounds__(TEXT_THREADS) void reads_sweep_kernel(const ReadsSweep a)
{
    __shared__ ReadsLds s;
    const u32 tid = threadIdx.x, tile = blockIdx.x;
    if (tid < 4)
        s.sum[tid] = 0;
    const u64 n = *a.lim, tile_at = (u64)tile * TEXT_TILE_BYTES, b = tile_at + (u64)tid * TEXT_CHUNK;
    const ReadsLane l = reads_lane<FORMAT>(a, n, b, s);                  // (synchronises: sum is zero)
    u64 err = TEXT_NO_ERROR;
    if (FORMAT != TEXT_FORMAT_FASTA) {
        const u32 m = l.bad_open | l.empty | l.invalid;
        if (m) {
            const u32 j = (u32)__builtin_ctz(m);
            err = text_error_key(b + j, (l.bad_open >> j) & 1 ? TEXT_ERR_ORPHAN : (l.invalid >> j) & 1 ? TEXT_ERR_CHAR : TEXT_ERR_EMPTY);
        }
    } else {
        const u32 body = l.keep | l.amb;
        err = text_fasta_records(l.headers, body, body | l.invalid, l.invalid, b, tile_at, tile, a.header_before[tile] != 0, s.wmax,
                                 a.last_seq, a.first_header, a.seq_before);
    }
    if (SPLIT) {
        u32 und, kkey, bkey, k_before, b_before;
        const u32 pieces = reads_lane_pieces(l, s, &und, &kkey, &bkey, &k_before, &b_before);
        reads_block_add((u32)__popc(pieces), &s.sum[0]);
        reads_block_add((u32)__popc(l.keep | l.amb), &s.sum[1]);
        if (und)
            atomicOr(&s.sum[2], 1u);
        if (tid == TEXT_THREADS - 1) {
            const u32 k = k_before > kkey ? k_before : kkey, q = b_before > bkey ? b_before : bkey;
            a.last_keep[tile] = k ? (u32)(tile_at + k) : 0u;
            a.last_brk[tile] = q ? (u32)(tile_at + q) : 0u;
        }
    }
    reads_block_add((u32)__popc(l.amb), &s.sum[3]);
    __syncthreads();
    if (tid == 0) {
        a.keep_t[tile] = l.keep_tile;
        a.rec_t[tile] = l.rec_tile;
        if (SPLIT) {
            a.piece_t[tile] = s.sum[0];
            a.sc_t[tile] = s.sum[1];
            a.undecided[tile] = s.sum[2];
        }
        if (s.sum[3])
            atomicAdd(reinterpret_cast<unsigned long long *>(a.res + 4), (unsigned long long)s.sum[3]);
    }
    text_error_min(err, reinterpret_cast<unsigned long long *>(a.res));
}

// ---- SPLIT, across tiles: the start that a tile could not decide is one iff the last kept base before the tile lies before
// the last break before it (keep_before_t / brk_before_t: the maximum scans of last_keep / last_brk).  One thread per tile.
__global__ __launch_bounds__(TEXT_THREADS) void reads_finish_kernel(const u32 *__restrict__ undecided, const u32 *__restrict__ keep_before_t,
                                                                    const u32 *__restrict__ brk_before_t, u32 *__restrict__ piece_t,
                                                                    u32 n_tiles)
{
    const u32 t = blockIdx.x * TEXT_THREADS + threadIdx.x;
    if (t < n_tiles && undecided[t] && keep_before_t[t] < brk_before_t[t])
        piece_t[t] += 1;
}

// ---- the second sweep; a.keep_t / rec_t / piece_t / sc_t: scanned in place.  The bases are packed as text_pack_kernel packs
// them.  Every record opener writes record_pos (below record_cap).  Not SPLIT: a sequence is a record, starts[r] = the base
// record r begins at.  SPLIT: a sequence is a piece: starts, src_record (the last record opened at or before its first base)
// and src_offset (here: the sequence characters of the text before it; rec_sc[r]: those before record r's opener --
// reads_offsets_kernel subtracts).  rec_amb (DROP; zero before the launch): the ambiguity letters of every record.
template <int FORMAT, bool SPLIT>
__global__ __launch_bounds__(TEXT_THREADS) void reads_pack_kernel(const ReadsSweep a, const ReadsPack p)
{
    __shared__ ReadsLds s;
    __shared__ unsigned long long packed[TEXT_PACKED_WORDS];
    const u32 tid = threadIdx.x, tile = blockIdx.x;
    const u64 n = *a.lim, b = (u64)tile * TEXT_TILE_BYTES + (u64)tid * TEXT_CHUNK;
    for (u32 i = tid; i < TEXT_PACKED_WORDS; i += TEXT_THREADS)
        packed[i] = 0;
    const ReadsLane l = reads_lane<FORMAT>(a, n, b, s);                  // (synchronises: packed is zero)
    const u64 out_at = a.keep_t[tile];
    text_pack_lane(packed, out_at, l.keep_before, l.c.c.codes, l.keep);
    const u64 base_at = out_at + l.keep_before, rec_at = (u64)a.rec_t[tile] + l.rec_before;
    const u32 sc = l.keep | l.amb;
    u64 sc_at = 0;
    if (SPLIT) {
        block_scan_value<TEXT_THREADS>((u32)__popc(sc), s.aux, (int)TEXT_THREADS, s.wa, (int)tid);
        sc_at = (u64)a.sc_t[tile] + s.aux[tid];
    }
    u32 rec = l.rec, r = 0;
    while (rec) {
        const u32 j = (u32)__builtin_ctz(rec);
        const u64 id = rec_at + r++;
        if (!SPLIT)
            p.starts[id] = base_at + (u32)__popc(l.keep & text_low_bits(j));
        else
            p.rec_sc[id] = (u32)(sc_at + (u32)__popc(sc & text_low_bits(j)));
        if (p.record_pos && id < p.record_cap)
            p.record_pos[id] = b + j;
        rec &= rec - 1;
    }
    if (SPLIT) {
        u32 und, kkey, bkey, k_before, b_before;
        u32 pieces = reads_lane_pieces(l, s, &und, &kkey, &bkey, &k_before, &b_before);
        if (und && a.keep_before_t[tile] < a.brk_before_t[tile])
            pieces |= und;
        block_scan_value<TEXT_THREADS>((u32)__popc(pieces), s.aux, (int)TEXT_THREADS, s.wa, (int)tid);
        u64 id = (u64)a.piece_t[tile] + s.aux[tid];
        while (pieces) {
            const u32 j = (u32)__builtin_ctz(pieces);
            p.starts[id] = base_at + (u32)__popc(l.keep & text_low_bits(j));
            p.src_record[id] = rec_at + (u32)__popc(l.rec & text_low_bits(j + 1)) - 1;
            p.src_offset[id] = sc_at + (u32)__popc(sc & text_low_bits(j));
            id++;
            pieces &= pieces - 1;
        }
    }
    if (p.rec_amb) {                                 // (rare: only lanes whose chunk holds an ambiguity letter)
        u32 m = l.amb;
        while (m) {
            const u32 j = (u32)__builtin_ctz(m);
            const u64 id = rec_at + (u32)__popc(l.rec & text_low_bits(j + 1)) - 1;
            if (id < p.n_records)                    // (always, in a text without error: a record opens before the letter)
                atomicAdd(&p.rec_amb[id], 1u);
            m &= m - 1;
        }
    }
    if (tile == 0 && tid == 0)
        p.starts[p.n_seqs] = p.n_bases;
    __syncthreads();
    text_pack_flush(packed, out_at, l.keep_tile, p.words);
}

// ---- over the sequences.  SPLIT: src_offset[i] -= the sequence characters before the opener of its record
__global__ __launch_bounds__(256) void reads_offsets_kernel(const u64 *__restrict__ src_record, u64 *__restrict__ src_offset,
                                                            const u32 *__restrict__ rec_sc, u64 n)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        src_offset[i] -= rec_sc[src_record[i]];
}
// not SPLIT: sequence i is record i from its first character on
__global__ __launch_bounds__(256) void reads_identity_kernel(u64 *__restrict__ src_record, u64 *__restrict__ src_offset, u64 n)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        src_record[i] = i;
        src_offset[i] = 0;
    }
}

// flags[i] = sequence i stays: its record holds no ambiguity letter (rec_amb, null: not asked) and it has min_bases bases;
// res2[0] += the sequences left out for the first reason, res2[1] += those for the second
__global__ __launch_bounds__(256) void reads_select_kernel(const u64 *__restrict__ starts, const u32 *__restrict__ rec_amb, u64 n,
                                                           u64 min_bases, u32 *__restrict__ flags, unsigned long long *__restrict__ res2)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    bool drop = false, cut = false;
    if (i < n) {
        drop = rec_amb && rec_amb[i] != 0;
        cut = !drop && starts[i + 1] - starts[i] < min_bases;
        flags[i] = !(drop || cut);
    }
    const u32 nd = (u32)__popcll(__ballot(drop)), nc = (u32)__popcll(__ballot(cut));
    if ((threadIdx.x & 63) == 0) {
        if (nd)
            atomicAdd(&res2[0], (unsigned long long)nd);
        if (nc)
            atomicAdd(&res2[1], (unsigned long long)nc);
    }
}
// the sequences that stay, closed up, in their order: rank = the scanned flags.  seg_first / len32: the segment list of
// launch_take_copy (len32: zero before the launch, so that a scan over all n entries sums the kept ones)
__global__ __launch_bounds__(256) void reads_move_kernel(const u64 *__restrict__ starts, const u64 *__restrict__ src_record,
                                                         const u64 *__restrict__ src_offset, const u32 *__restrict__ flags,
                                                         const u32 *__restrict__ rank, u64 n, u64 *__restrict__ seg_first,
                                                         u32 *__restrict__ len32, u64 *__restrict__ src_record_out,
                                                         u64 *__restrict__ src_offset_out)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !flags[i])
        return;
    const u32 r = rank[i];
    seg_first[r] = starts[i];
    len32[r] = (u32)(starts[i + 1] - starts[i]);
    src_record_out[r] = src_record[i];
    src_offset_out[r] = src_offset[i];
}

// ---------------------------------------------------------------- launchers
hipError_t launch_reads_newlines(const unsigned char *text, u64 n, u32 n_tiles, u32 *nl_t, hipStream_t s)
{
    hipLaunchKernelGGL(reads_newlines_kernel, dim3(n_tiles), dim3(TEXT_THREADS), 0, s, text, n, nl_t);
    return hipGetLastError();
}

hipError_t launch_reads_fastq_cut(const unsigned char *text, u64 n, u32 n_tiles, const u32 *nl_t, const u32 *nl_base, const u32 *total,
                                  bool more, u64 *lim, u64 *res, hipStream_t s)
{
    hipLaunchKernelGGL(reads_fastq_cut_kernel, dim3(n_tiles), dim3(TEXT_THREADS), 0, s, text, n, nl_t, nl_base, total, more ? 1 : 0, lim,
                       reinterpret_cast<unsigned long long *>(res));
    return hipGetLastError();
}

hipError_t launch_reads_fastq_rank(const unsigned char *text, u64 n, const u32 *nl_base, u64 e, u64 *out3, hipStream_t s)
{
    hipLaunchKernelGGL(reads_fastq_rank_kernel, dim3(1), dim3(TEXT_THREADS), 0, s, text, n, nl_base, e, out3);
    return hipGetLastError();
}

template <int FORMAT>
static void reads_sweep_launch(const ReadsSweep &a, hipStream_t s)
{
    if (a.ambiguous == READS_AMBIG_SPLIT)
        hipLaunchKernelGGL((reads_sweep_kernel<FORMAT, true>), dim3(a.n_tiles), dim3(TEXT_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL((reads_sweep_kernel<FORMAT, false>), dim3(a.n_tiles), dim3(TEXT_THREADS), 0, s, a);
}
hipError_t launch_reads_sweep(const ReadsSweep &a, hipStream_t s)
{
    if (a.format == TEXT_FORMAT_FASTA)
        reads_sweep_launch<TEXT_FORMAT_FASTA>(a, s);
    else if (a.format == TEXT_FORMAT_FASTQ)
        reads_sweep_launch<TEXT_FORMAT_FASTQ>(a, s);
    else
        reads_sweep_launch<TEXT_FORMAT_LINES>(a, s);
    return hipGetLastError();
}

hipError_t launch_reads_finish(const ReadsSweep &a, hipStream_t s)
{
    hipLaunchKernelGGL(reads_finish_kernel, dim3((a.n_tiles + TEXT_THREADS - 1) / TEXT_THREADS), dim3(TEXT_THREADS), 0, s, a.undecided,
                       a.keep_before_t, a.brk_before_t, a.piece_t, a.n_tiles);
    return hipGetLastError();
}

template <int FORMAT>
static void reads_pack_launch(const ReadsSweep &a, const ReadsPack &p, hipStream_t s)
{
    if (a.ambiguous == READS_AMBIG_SPLIT)
        hipLaunchKernelGGL((reads_pack_kernel<FORMAT, true>), dim3(a.n_tiles), dim3(TEXT_THREADS), 0, s, a, p);
    else
        hipLaunchKernelGGL((reads_pack_kernel<FORMAT, false>), dim3(a.n_tiles), dim3(TEXT_THREADS), 0, s, a, p);
}
hipError_t launch_reads_pack(const ReadsSweep &a, const ReadsPack &p, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(p.words, 0, (size_t)(text_words(p.n_bases) ? text_words(p.n_bases) : 1) * sizeof(u64), s);
    if (e != hipSuccess)
        return e;
    if (a.format == TEXT_FORMAT_FASTA)
        reads_pack_launch<TEXT_FORMAT_FASTA>(a, p, s);
    else if (a.format == TEXT_FORMAT_FASTQ)
        reads_pack_launch<TEXT_FORMAT_FASTQ>(a, p, s);
    else
        reads_pack_launch<TEXT_FORMAT_LINES>(a, p, s);
    return hipGetLastError();
}

hipError_t launch_reads_offsets(const u64 *src_record, u64 *src_offset, const u32 *rec_sc, u64 n, hipStream_t s)
{
    hipLaunchKernelGGL(reads_offsets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src_record, src_offset, rec_sc, n);
    return hipGetLastError();
}

hipError_t launch_reads_identity(u64 *src_record, u64 *src_offset, u64 n, hipStream_t s)
{
    hipLaunchKernelGGL(reads_identity_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src_record, src_offset, n);
    return hipGetLastError();
}

hipError_t launch_reads_select(const u64 *starts, const u32 *rec_amb, u64 n, u64 min_bases, u32 *flags, u64 *res2, hipStream_t s)
{
    hipLaunchKernelGGL(reads_select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, starts, rec_amb, n, min_bases, flags,
                       reinterpret_cast<unsigned long long *>(res2));
    return hipGetLastError();
}

hipError_t launch_reads_move(const u64 *starts, const u64 *src_record, const u64 *src_offset, const u32 *flags, const u32 *rank, u64 n,
                             u64 *seg_first, u32 *len32, u64 *src_record_out, u64 *src_offset_out, hipStream_t s)
{
    hipLaunchKernelGGL(reads_move_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, starts, src_record, src_offset, flags, rank,
                       n, seg_first, len32, src_record_out, src_offset_out);
    return hipGetLastError();
}

}  // namespace dnagpu
