// text_kernels.hip -- the kernels of dnagpu_table_from_text: the raw bytes of a text file -- one sequence
// per line, or FASTA -- into the packed stream, the starts and the record offsets of a resident table.  The bit arithmetic
// of one lane's 32 bytes is text_math.hpp's.
//
// The loader is a stream compaction: the result is the text's bytes with everything dropped that is no base of a sequence
// line, so a byte's place in the result is its offset minus the bytes dropped before it.  Two sweeps read the text, tile by
// tile (TEXT_TILE_BYTES per workgroup, TEXT_CHUNK bytes per lane):
//   text_sweep_kernel   counts, per tile, the bases kept and the records begun, and finds the input errors;
//   (the host scans the tile counts; one read-back: error word, records, bases, bytes consumed)
//   text_pack_kernel    packs every tile's kept bases in LDS and stores whole words, and writes the starts.
// What a byte means depends on text before it only in FASTA, where the bytes of a header line are ignored: the state a tile
// begins in (inside a header line or not, a header seen or not) comes from text_heads_kernel and a maximum scan over the
// tiles, so no lane ever walks a line.  A record without sequence is found the same way: for every header, the last header
// and the last base before it, inside the tile by the lanes, across tiles by text_finish_kernel.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "text_device.hpp"

namespace dnagpu {

// What the two sweeps make of a lane's chunk, alike: the bases kept, the records begun, and their ranks inside the tile.
struct TextLane {
    TextChunk c;
    u32 starts, headers;      // line starts; those of header lines (FASTA)
    u32 header_bytes;         // bytes of header lines (FASTA)
    u32 keep, rec;            // bases of the result; first bytes of records (LINES: line starts, FASTA: header starts)
    u32 keep_before, rec_before, keep_tile, rec_tile;     // exclusive ranks inside the tile, and the tile's totals
};
struct TextLds {
    u32 keep[TEXT_THREADS], rec[TEXT_THREADS];
    u32 wk[TEXT_THREADS / 64], wr[TEXT_THREADS / 64], wmax[TEXT_THREADS / 64];
};
// in_header_tile: the line that reaches into the tile from before is a header (FASTA)
template <bool FASTA>
__device__ __forceinline__ TextLane text_lane(const unsigned char *__restrict__ text, u64 n, u64 b, bool in_header_tile, TextLds &s)
{
    const u32 tid = threadIdx.x;
    TextLane l;
    l.c = text_load(text, n, b);
    l.starts = text_line_starts(l.c);
    l.headers = FASTA ? l.starts & l.c.gt : 0u;
    l.header_bytes = 0;
    if (FASTA) {
        // the last line start before this chunk decides what the chunk begins in: (thread + 1) << 1 | its header flag
        const u32 key = l.starts ? ((tid + 1) << 1) | ((l.headers >> text_top_bit(l.starts)) & 1) : 0u;
        const u32 before = text_block_max_before(key, s.wmax);
        const bool in_header = before ? (before & 1) != 0 : in_header_tile;
        l.header_bytes = text_header_bytes(l.starts, l.headers, in_header) & l.c.valid;
    }
    l.keep = l.c.base & ~l.header_bytes;
    l.rec = FASTA ? l.headers : l.starts;
    l.keep_tile = block_scan_value<TEXT_THREADS>((u32)__popc(l.keep), s.keep, (int)TEXT_THREADS, s.wk, (int)tid);
    l.rec_tile = block_scan_value<TEXT_THREADS>((u32)__popc(l.rec), s.rec, (int)TEXT_THREADS, s.wr, (int)tid);
    l.keep_before = s.keep[tid];
    l.rec_before = s.rec[tid];
    return l;
}

// ---- the cut of a chunk that more text follows: *cut = the greatest p with text_is_cut(p), found from the end backwards,
// TEXT_TILE_BYTES candidates at a time by one workgroup (a line or record is short beside a chunk; a chunk that holds no
// cut at all is read once, and the caller has to enlarge it anyway).
__global__ __launch_bounds__(TEXT_THREADS) void text_cut_kernel(const unsigned char *__restrict__ text, u64 n, int format,
                                                                u64 *__restrict__ cut)
{
    __shared__ unsigned long long best;
    u64 hi = n + 1;                                  // the candidates left: p < hi
    while (hi > 0) {                                 // uniform
        const u64 lo = hi > TEXT_TILE_BYTES ? hi - TEXT_TILE_BYTES : 0;
        if (threadIdx.x == 0)
            best = 0;
        __syncthreads();
        unsigned long long found = 0;                // p + 1
        for (u32 j = 0; j < TEXT_CHUNK; j++) {
            const u64 p = lo + (u64)threadIdx.x * TEXT_CHUNK + j;
            if (p < hi && text_is_cut(text, n, format, p))
                found = p + 1;
        }
        if (found)
            atomicMax(&best, found);
        __syncthreads();
        const u64 b = best;
        __syncthreads();
        if (b) {
            if (threadIdx.x == 0)
                *cut = b - 1;
            return;
        }
        hi = lo;
    }
    if (threadIdx.x == 0)
        *cut = text_no_cut(n, format);
}

// ---- FASTA, before the sweep: per tile, the last line start ((tile + 1) << 1 | it begins a header; 0: no line start) and
// the last header (offset of its '>' + 1; 0: none).  Both need no state.  *lim = the bytes of text that count.
__global__ __launch_bounds__(TEXT_THREADS) void text_heads_kernel(const unsigned char *__restrict__ text, const u64 *__restrict__ lim,
                                                                  u32 *__restrict__ last_start, u32 *__restrict__ last_header)
{
    __shared__ u32 wmax[TEXT_THREADS / 64];
    const u32 tid = threadIdx.x;
    const u64 n = *lim, b = (u64)blockIdx.x * TEXT_TILE_BYTES + (u64)tid * TEXT_CHUNK;
    const TextChunk c = text_load(text, n, b);
    const u32 starts = text_line_starts(c), headers = starts & c.gt;
    const u32 skey = starts ? ((tid + 1) << 1) | ((headers >> text_top_bit(starts)) & 1) : 0u;
    const u32 hkey = headers ? (u32)(b + text_top_bit(headers) + 1) : 0u;
    const u32 sb = text_block_max_before(skey, wmax), hb = text_block_max_before(hkey, wmax);
    if (tid == TEXT_THREADS - 1) {
        const u32 s = sb > skey ? sb : skey;
        last_start[blockIdx.x] = s ? ((blockIdx.x + 1) << 1) | (s & 1) : 0u;
        last_header[blockIdx.x] = hb > hkey ? hb : hkey;
    }
}

// out[i] = the maximum of in[0 .. i) (0 for i = 0), n <= 2^19 + 1 entries, by one workgroup of 1024 threads; in != out
__global__ __launch_bounds__(1024) void text_max_scan_kernel(const u32 *__restrict__ in, u32 *__restrict__ out, u32 n)
{
    __shared__ u32 sh[1024];
    const u32 tid = threadIdx.x, per = (n + 1023) / 1024;
    const u32 lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    u32 m = 0;
    for (u32 i = lo; i < hi; i++)
        m = m > in[i] ? m : in[i];
    sh[tid] = m;
    __syncthreads();
    for (u32 off = 1; off < 1024; off <<= 1) {
        const u32 o = tid >= off ? sh[tid - off] : 0u;
        __syncthreads();
        if (o > sh[tid])
            sh[tid] = o;
        __syncthreads();
    }
    u32 run = tid ? sh[tid - 1] : 0u;
    for (u32 i = lo; i < hi; i++) {
        const u32 v = in[i];
        out[i] = run;
        run = run > v ? run : v;
    }
}

// ---- the first sweep.  Per tile: keep_t = bases kept, rec_t = records begun; res[0] = the minimum of the error words
// (text_error_key).  FASTA: in_state[t] = the maximum of text_heads_kernel's last_start before tile t, header_before[t] that
// of last_header; and per tile, for text_finish_kernel: last_seq = the last kept base (offset + 1, 0: none),
// first_header = the first header (offset + 1), seq_before = the last kept base before that header inside the tile.
template <bool FASTA>
__global__ __launch_bounds__(TEXT_THREADS) void text_sweep_kernel(const unsigned char *__restrict__ text, const u64 *__restrict__ lim,
                                                                  const u32 *__restrict__ in_state, const u32 *__restrict__ header_before,
                                                                  u32 *__restrict__ keep_t, u32 *__restrict__ rec_t,
                                                                  u32 *__restrict__ last_seq, u32 *__restrict__ first_header,
                                                                  u32 *__restrict__ seq_before, unsigned long long *__restrict__ res)
{
    __shared__ TextLds s;
    const u32 tid = threadIdx.x, tile = blockIdx.x;
    const u64 n = *lim, tile_at = (u64)tile * TEXT_TILE_BYTES, b = tile_at + (u64)tid * TEXT_CHUNK;
    const TextLane l = text_lane<FASTA>(text, n, b, FASTA && (in_state[tile] & 1), s);
    const u32 invalid = text_invalid(l.c) & ~l.header_bytes;
    u64 err = TEXT_NO_ERROR;
    if (!FASTA) {
        const u32 empty = l.starts & text_terminators(l.c);          // a line that begins with its terminator
        const u32 m = invalid | empty;
        if (m) {
            const u32 j = (u32)__builtin_ctz(m);
            err = text_error_key(b + j, (invalid >> j) & 1 ? TEXT_ERR_CHAR : TEXT_ERR_EMPTY);
        }
    } else {
        err = text_fasta_records(l.headers, l.keep, l.keep | invalid, invalid, b, tile_at, tile, header_before[tile] != 0, s.wmax,
                                 last_seq, first_header, seq_before);
    }
    if (tid == 0) {
        keep_t[tile] = l.keep_tile;
        rec_t[tile] = l.rec_tile;
    }
    text_error_min(err, res);
}

// ---- FASTA, across tiles: the record that the first header of a tile closes, and the record the end of the text closes.
// header_before / seq_before_t: the maximum scans of last_header / last_seq.  One thread per tile.
__global__ __launch_bounds__(TEXT_THREADS) void text_finish_kernel(const u32 *__restrict__ header_before, const u32 *__restrict__ last_header,
                                                                   const u32 *__restrict__ seq_before_t, const u32 *__restrict__ last_seq,
                                                                   const u32 *__restrict__ first_header, const u32 *__restrict__ seq_before,
                                                                   u32 n_tiles, unsigned long long *__restrict__ res)
{
    const u32 t = blockIdx.x * TEXT_THREADS + threadIdx.x;
    if (t >= n_tiles)
        return;
    const u32 hb = header_before[t], qb = seq_before_t[t];
    u64 err = TEXT_NO_ERROR;
    if (first_header[t] && hb) {
        const u32 pq = seq_before[t] > qb ? seq_before[t] : qb;
        if (pq < hb)
            err = text_error_key((u64)hb - 1, TEXT_ERR_EMPTY);
    }
    if (t == n_tiles - 1) {                          // the end of the text closes the last record
        const u32 ph = last_header[t] > hb ? last_header[t] : hb, pq = last_seq[t] > qb ? last_seq[t] : qb;
        if (ph && pq < ph) {
            const u64 e = text_error_key((u64)ph - 1, TEXT_ERR_EMPTY);
            err = e < err ? e : err;
        }
    }
    if (err != TEXT_NO_ERROR)
        atomicMin(&res[0], (unsigned long long)err);
}

// ---- after an error at byte e: out2[0] = the 0-based record e belongs to (the records begun at or before it, less one:
// ~0 before the first), out2[1] = the byte.  rec_base: the scanned rec_t.  One workgroup, over e's tile.
__global__ __launch_bounds__(TEXT_THREADS) void text_rank_kernel(const unsigned char *__restrict__ text, const u64 *__restrict__ lim,
                                                                 int format, const u32 *__restrict__ rec_base, u64 e,
                                                                 u64 *__restrict__ out2)
{
    __shared__ u32 count;
    if (threadIdx.x == 0)
        count = 0;
    __syncthreads();
    const u64 tile = e / TEXT_TILE_BYTES, b = tile * TEXT_TILE_BYTES + (u64)threadIdx.x * TEXT_CHUNK;
    const TextChunk c = text_load(text, *lim, b);
    u32 rec = text_line_starts(c);
    if (format == TEXT_FORMAT_FASTA)
        rec &= c.gt;
    if (b > e)
        rec = 0;
    else if (e - b < TEXT_CHUNK - 1)
        rec &= text_low_bits((u32)(e - b) + 1);
    if (rec)
        atomicAdd(&count, (u32)__popc(rec));
    __syncthreads();
    if (threadIdx.x == 0) {
        out2[0] = (u64)rec_base[tile] + count - 1;
        out2[1] = text[e];
    }
}

// ---- the second sweep.  keep_base / rec_base: the scanned tile counts; n_bases / n_records their totals.  A tile's kept
// bases are packed in LDS at the bit its first base has in the result, and its words are stored once, whole -- but the
// first and the last word of a tile, which it may share with its neighbours, are ORed into `words` (zero before the
// launch).  starts[r] = the base record r begins at, starts[n_records] = n_bases; record_pos[r] = the offset of record
// r's first byte, for r < record_cap (null: not wanted).
template <bool FASTA>
__global__ __launch_bounds__(TEXT_THREADS) void text_pack_kernel(const unsigned char *__restrict__ text, const u64 *__restrict__ lim,
                                                                 const u32 *__restrict__ in_state, const u32 *__restrict__ keep_base,
                                                                 const u32 *__restrict__ rec_base, u64 n_bases, u64 n_records,
                                                                 u64 *__restrict__ words, u64 *__restrict__ starts,
                                                                 u64 *__restrict__ record_pos, u64 record_cap)
{
    __shared__ TextLds s;
    __shared__ unsigned long long packed[TEXT_PACKED_WORDS];
    const u32 tid = threadIdx.x, tile = blockIdx.x;
    const u64 n = *lim, b = (u64)tile * TEXT_TILE_BYTES + (u64)tid * TEXT_CHUNK;
    for (u32 i = tid; i < TEXT_PACKED_WORDS; i += TEXT_THREADS)
        packed[i] = 0;
    const TextLane l = text_lane<FASTA>(text, n, b, FASTA && (in_state[tile] & 1), s);     // (synchronises: packed is zero)
    const u64 out_at = keep_base[tile];              // the result's base this tile's first kept base becomes
    text_pack_lane(packed, out_at, l.keep_before, l.c.codes, l.keep);
    u32 rec = l.rec, r = 0;
    while (rec) {
        const u32 j = (u32)__builtin_ctz(rec);
        const u64 id = (u64)rec_base[tile] + l.rec_before + r++;
        starts[id] = out_at + l.keep_before + (u32)__popc(l.keep & text_low_bits(j));
        if (record_pos && id < record_cap)
            record_pos[id] = b + j;
        rec &= rec - 1;
    }
    if (tile == 0 && tid == 0)
        starts[n_records] = n_bases;
    __syncthreads();
    text_pack_flush(packed, out_at, l.keep_tile, words);
}

// ---------------------------------------------------------------- launchers
hipError_t launch_text_cut(const unsigned char *text, u64 n, int format, u64 *cut, hipStream_t s)
{
    hipLaunchKernelGGL(text_cut_kernel, dim3(1), dim3(TEXT_THREADS), 0, s, text, n, format, cut);
    return hipGetLastError();
}

hipError_t launch_text_heads(const unsigned char *text, const u64 *lim, u32 n_tiles, u32 *last_start, u32 *last_header, hipStream_t s)
{
    hipLaunchKernelGGL(text_heads_kernel, dim3(n_tiles), dim3(TEXT_THREADS), 0, s, text, lim, last_start, last_header);
    return hipGetLastError();
}

hipError_t launch_text_max_scan(const u32 *in, u32 *out, u32 n, hipStream_t s)
{
    hipLaunchKernelGGL(text_max_scan_kernel, dim3(1), dim3(1024), 0, s, in, out, n);
    return hipGetLastError();
}

hipError_t launch_text_sweep(const TextSweep &a, hipStream_t s)
{
    unsigned long long *res = reinterpret_cast<unsigned long long *>(a.res);
    if (a.format == TEXT_FORMAT_FASTA)
        hipLaunchKernelGGL(text_sweep_kernel<true>, dim3(a.n_tiles), dim3(TEXT_THREADS), 0, s, a.text, a.lim, a.in_state,
                           a.header_before, a.keep_t, a.rec_t, a.last_seq, a.first_header, a.seq_before, res);
    else
        hipLaunchKernelGGL(text_sweep_kernel<false>, dim3(a.n_tiles), dim3(TEXT_THREADS), 0, s, a.text, a.lim, a.in_state,
                           a.header_before, a.keep_t, a.rec_t, a.last_seq, a.first_header, a.seq_before, res);
    return hipGetLastError();
}

hipError_t launch_text_finish(const TextSweep &a, const u32 *last_header, const u32 *seq_before_t, hipStream_t s)
{
    hipLaunchKernelGGL(text_finish_kernel, dim3((a.n_tiles + TEXT_THREADS - 1) / TEXT_THREADS), dim3(TEXT_THREADS), 0, s,
                       a.header_before, last_header, seq_before_t, a.last_seq, a.first_header, a.seq_before, a.n_tiles,
                       reinterpret_cast<unsigned long long *>(a.res));
    return hipGetLastError();
}

hipError_t launch_text_rank(const unsigned char *text, const u64 *lim, int format, const u32 *rec_base, u64 e, u64 *out2, hipStream_t s)
{
    hipLaunchKernelGGL(text_rank_kernel, dim3(1), dim3(TEXT_THREADS), 0, s, text, lim, format, rec_base, e, out2);
    return hipGetLastError();
}

hipError_t launch_text_pack(const TextSweep &a, u64 n_bases, u64 n_records, u64 *words, u64 *starts, u64 *record_pos, u64 record_cap,
                            hipStream_t s)
{
    hipError_t e = hipMemsetAsync(words, 0, (size_t)(text_words(n_bases) ? text_words(n_bases) : 1) * sizeof(u64), s);
    if (e != hipSuccess)
        return e;
    if (a.format == TEXT_FORMAT_FASTA)
        hipLaunchKernelGGL(text_pack_kernel<true>, dim3(a.n_tiles), dim3(TEXT_THREADS), 0, s, a.text, a.lim, a.in_state, a.keep_t,
                           a.rec_t, n_bases, n_records, words, starts, record_pos, record_cap);
    else
        hipLaunchKernelGGL(text_pack_kernel<false>, dim3(a.n_tiles), dim3(TEXT_THREADS), 0, s, a.text, a.lim, a.in_state, a.keep_t,
                           a.rec_t, n_bases, n_records, words, starts, record_pos, record_cap);
    return hipGetLastError();
}

}  // namespace dnagpu
