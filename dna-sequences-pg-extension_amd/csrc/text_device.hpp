// text_device.hpp -- the device code that the kernels of dnagpu_table_from_text (text_kernels.hip) and of
// dnagpu_reads_from_text (reads_kernels.hip) share: the load of one lane's chunk, the maximum over the
// threads before, the closing of FASTA records inside a tile, and the packing of a tile's kept bases in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "text_math.hpp"

namespace dnagpu {

// ---- one lane's chunk: the TEXT_CHUNK bytes at byte b of the n bytes at text, as eight words.  16-byte loads where the
// chunk is whole and the address allows, bytes otherwise; no byte at or beyond text + n is read, and bytes beyond n are 0.
// Returns the bytes of the chunk that lie inside the text (b < n).
__device__ __forceinline__ u32 text_load_words(const unsigned char *__restrict__ text, u64 n, u64 b, u32 w[8])
{
    const u64 left = n - b;
    if (left >= TEXT_CHUNK && (reinterpret_cast<uintptr_t>(text + b) & 15) == 0) {
        const uint4 *p = reinterpret_cast<const uint4 *>(text + b);
        const uint4 lo = p[0], hi = p[1];
        w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w;
        w[4] = hi.x; w[5] = hi.y; w[6] = hi.z; w[7] = hi.w;
    } else {
#pragma unroll
        for (u32 q = 0; q < 8; q++) {
            u32 v = 0;
            for (u32 r = 0; r < 4; r++)
                if (q * 4 + r < left)
                    v |= (u32)text[b + q * 4 + r] << (8 * r);
            w[q] = v;
        }
    }
    return left >= TEXT_CHUNK ? TEXT_CHUNK : (u32)left;
}
// the same as a classified chunk; bytes beyond n count as no character
__device__ __forceinline__ TextChunk text_load(const unsigned char *__restrict__ text, u64 n, u64 b)
{
    TextChunk c = {};
    if (b >= n)
        return c;
    u32 w[8];
    const u32 have = text_load_words(text, n, b, w);
    c.valid = text_low_bits(have);
#pragma unroll
    for (u32 j = 0; j < TEXT_CHUNK; j++)
        text_chunk_byte(c, j, (w[j >> 2] >> (8 * (j & 3))) & 0xff);
    c.prev_nl = b == 0 || text[b - 1] == '\n';
    c.next_nl = n - b > TEXT_CHUNK && text[b + TEXT_CHUNK] == '\n';
    return c;
}

// the maximum of v over the threads before this one (0 for thread 0), by the TEXT_THREADS threads of the workgroup;
// wmax: one word of LDS per wave.  Synchronises.
__device__ __forceinline__ u32 text_block_max_before(u32 v, u32 *wmax)
{
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 inc = v;
#pragma unroll
    for (u32 off = 1; off < 64; off <<= 1) {
        const u32 o = __shfl_up(inc, off);
        if (lane >= off)
            inc = inc > o ? inc : o;
    }
    u32 ex = __shfl_up(inc, 1);
    if (lane == 0)
        ex = 0;
    if (lane == 63)
        wmax[wave] = inc;
    __syncthreads();
    for (u32 w = 0; w < wave; w++)
        ex = ex > wmax[w] ? ex : wmax[w];
    __syncthreads();
    return ex;
}

// ---- FASTA, the first sweep: the records that close inside the tile.  headers: the chunk's header starts; body: the bytes
// that make a record non-empty; seq: the bytes that must not come before the first header; invalid: the invalid characters
// of sequence lines.  Returns the lane's error word and writes, per tile, for text_finish_kernel: last_seq = the last body
// byte (offset + 1, 0: none), first_header = the first header (offset + 1), seq_before = the last body byte before that
// header inside the tile.  seen_before: a header lies before the tile.  Synchronises.
__device__ __forceinline__ u64 text_fasta_records(u32 headers, u32 body, u32 seq, u32 invalid, u64 b, u64 tile_at, u32 tile,
                                                  bool seen_before, u32 *wmax, u32 *__restrict__ last_seq,
                                                  u32 *__restrict__ first_header, u32 *__restrict__ seq_before)
{
    const u32 tid = threadIdx.x;
    u64 err = TEXT_NO_ERROR;
    // positions inside the tile + 1 (0: none): the last header and the last body byte before this chunk
    const u32 at = tid * TEXT_CHUNK + 1;
    const u32 hkey = headers ? at + text_top_bit(headers) : 0u;
    const u32 qkey = body ? at + text_top_bit(body) : 0u;
    const u32 h_before = text_block_max_before(hkey, wmax), q_before = text_block_max_before(qkey, wmax);
    const bool seen = seen_before || h_before != 0;
    if (seq) {
        const u32 j = (u32)__builtin_ctz(seq);
        if (!seen && !(headers & text_low_bits(j)))
            err = text_error_key(b + j, TEXT_ERR_ORPHAN);
    }
    if (err == TEXT_NO_ERROR && invalid)
        err = text_error_key(b + (u32)__builtin_ctz(invalid), TEXT_ERR_CHAR);
    // every header closes the record before it: empty when no body byte lies between the two headers
    u32 hs = headers;
    while (hs) {
        const u32 j = (u32)__builtin_ctz(hs);
        const u32 below = text_low_bits(j);
        const u32 ph = headers & below ? at + text_top_bit(headers & below) : h_before;
        const u32 pq = body & below ? at + text_top_bit(body & below) : q_before;
        if (ph) {
            if (pq < ph) {
                const u64 e = text_error_key(tile_at + ph - 1, TEXT_ERR_EMPTY);
                err = e < err ? e : err;
            }
        } else {                                     // the tile's first header: the record before it began in another tile
            first_header[tile] = (u32)(b + j + 1);
            seq_before[tile] = pq ? (u32)(tile_at + pq) : 0u;
        }
        hs &= hs - 1;
    }
    if (tid == TEXT_THREADS - 1) {
        const u32 q = q_before > qkey ? q_before : qkey;
        last_seq[tile] = q ? (u32)(tile_at + q) : 0u;
        if (!(h_before | hkey)) {
            first_header[tile] = 0;
            seq_before[tile] = 0;
        }
    }
    return err;
}

// the minimum of the lanes' error words into *res
__device__ __forceinline__ void text_error_min(u64 err, unsigned long long *__restrict__ res)
{
#pragma unroll
    for (u32 off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_down(err, off);
        err = o < err ? o : err;
    }
    if ((threadIdx.x & 63) == 0 && err != TEXT_NO_ERROR)
        atomicMin(res, (unsigned long long)err);
}

// ---- the second sweep: a tile's kept bases are packed in LDS at the bit its first base has in the result, and its words are
// stored once, whole -- but the first and the last word of a tile, which it may share with its neighbours, are ORed into
// `words` (zero before the launch).  packed: TEXT_PACKED_WORDS words of LDS, zero before text_pack_lane; out_at: the
// result's base the tile's first kept base becomes; keep_before / keep_tile: the lane's rank and the tile's total.
constexpr u32 TEXT_PACKED_WORDS = TEXT_TILE_BYTES / 32 + 2;
__device__ __forceinline__ void text_pack_lane(unsigned long long *packed, u64 out_at, u32 keep_before, u64 codes, u32 keep)
{
    if (!keep)
        return;
    const u64 v = text_compact(codes, keep);
    const u32 q = (u32)(out_at & 31) + keep_before, sh = 2 * (q & 31);
    atomicOr(&packed[q >> 5], (unsigned long long)(v << sh));
    if ((q & 31) + (u32)__popc(keep) > 32)
        atomicOr(&packed[(q >> 5) + 1], (unsigned long long)(v >> (64 - sh)));      // (sh > 0 here)
}
__device__ __forceinline__ void text_pack_flush(const unsigned long long *packed, u64 out_at, u32 keep_tile, u64 *__restrict__ words)
{
    const u32 n_words = ((u32)(out_at & 31) + keep_tile + 31) / 32;
    const u64 w0 = out_at >> 5;
    for (u32 i = threadIdx.x; i < n_words; i += TEXT_THREADS) {
        const unsigned long long v = packed[i];
        if (i == 0 || i == n_words - 1) {
            if (v)
                atomicOr(reinterpret_cast<unsigned long long *>(&words[w0 + i]), v);
        } else {
            words[w0 + i] = v;
        }
    }
}

}  // namespace dnagpu
