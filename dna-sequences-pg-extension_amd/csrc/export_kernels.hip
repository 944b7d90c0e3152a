// export_kernels.hip -- the text image of a resident table (dnagpu_table_to_text, dnagpu_text_image_read): the
// pass that sizes every record, the widening of the scanned sizes into record offsets, and the output-centric sweep that
// forms any byte window of the image.  The record arithmetic is export_math.hpp's.  Every kernel has a NAMED sibling
// (dnagpu_table_to_text_named) made from the same body: the headers are the strings of a names column.
#include <hip/hip_runtime.h>

#include "export_math.hpp"
#include "kernels.hpp"
#include "quals_math.hpp"

namespace dnagpu {

// ---- the plan.  One thread per sequence (grid-stride): ex32[s] = the bytes of record s that are no bases of a sequence
// line (clamped: the scan is only run once the total is known to fit 32 bits); res[0] += those, res[1] += the sequences of
// 0 bases: a block reduce, then one atomic per workgroup and word (take_segments_kernel's shape).
// NAMED (dnagpu_table_to_text_named): `numbers` is the n + 1 offsets of a names column, and the header of record s is its
// marker and the column's string s.
template <bool NAMED>
__device__ __forceinline__ void export_plan_body(const u64 *__restrict__ starts, u64 n, const u64 *__restrict__ numbers, u64 name_base,
                                                 const ExportFmt &f, u32 *__restrict__ ex32, unsigned long long *__restrict__ res)
{
    __shared__ u64 wsum[EXPORT_THREADS / 64], wemp[EXPORT_THREADS / 64];
    u64 sum = 0, emp = 0;
    for (u64 s = (u64)blockIdx.x * EXPORT_THREADS + threadIdx.x; s < n; s += (u64)gridDim.x * EXPORT_THREADS) {
        const u64 len = starts[s + 1] - starts[s];
        u32 hl;
        if constexpr (NAMED)
            hl = 1u + (u32)(numbers[s + 1] - numbers[s]);
        else
            hl = export_header_len(f, numbers ? numbers[s] : name_base + s);
        const u64 ex = export_extras(f, len, hl);
        ex32[s] = ex > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)ex;
        sum += ex;                                   // (at most 2^32 - 1 bases in all: no overflow)
        emp += len == 0;
    }
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off);
        emp += __shfl_down(emp, off);
    }
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6] = sum;
        wemp[threadIdx.x >> 6] = emp;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 total = 0, empties = 0;
#pragma unroll
        for (u32 w = 0; w < EXPORT_THREADS / 64; w++) {
            total += wsum[w];
            empties += wemp[w];
        }
        if (total)
            atomicAdd(&res[0], (unsigned long long)total);
        if (empties)
            atomicAdd(&res[1], (unsigned long long)empties);
    }
}
__global__ __launch_bounds__(EXPORT_THREADS) void export_plan_kernel(const u64 *__restrict__ starts, u64 n,
                                                                     const u64 *__restrict__ numbers, u64 name_base, ExportFmt f,
                                                                     u32 *__restrict__ ex32, unsigned long long *__restrict__ res)
{
    export_plan_body<false>(starts, n, numbers, name_base, f, ex32, res);
}
__global__ __launch_bounds__(EXPORT_THREADS) void export_plan_named_kernel(const u64 *__restrict__ starts, u64 n,
                                                                           const u64 *__restrict__ name_off, ExportFmt f,
                                                                           u32 *__restrict__ ex32, unsigned long long *__restrict__ res)
{
    export_plan_body<true>(starts, n, name_off, 0, f, ex32, res);
}

// pos[s] = starts[s] + scan[s] (the exclusive scan of the extras) for s < n, pos[n] = starts[n] + total
__global__ __launch_bounds__(EXPORT_THREADS) void export_pos_kernel(const u64 *__restrict__ starts, const u32 *__restrict__ scan, u64 n,
                                                                    u64 total, u64 *__restrict__ pos)
{
    const u64 i = (u64)blockIdx.x * EXPORT_THREADS + threadIdx.x;
    if (i < n)
        pos[i] = starts[i] + scan[i];
    else if (i == n)
        pos[i] = starts[i] + total;
}

// Index of the first entry of a[lo .. hi) that is > p (hi when there is none), a ascending; by the whole workgroup, every
// thread gets the answer (take_kernels.hip's 256-ary search).  wc: one word of LDS per wave.
__device__ __forceinline__ u64 export_block_upper_bound(const u64 *__restrict__ a, u64 lo, u64 hi, u64 p, u32 *wc)
{
    const u32 tid = threadIdx.x;
    while (hi > lo) {                                // uniform
        const u64 step = (hi - lo + EXPORT_THREADS - 1) / EXPORT_THREADS;
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
        for (u32 w = 0; w < EXPORT_THREADS / 64; w++)
            cnt += wc[w];
        __syncthreads();
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

// the last record of lo .. hi whose offset is <= p (lo's is); record i's offset is a[i - bias]
__device__ __forceinline__ u64 export_record_of(const u64 *a, u64 bias, u64 lo, u64 hi, u64 p)
{
    while (lo < hi) {
        const u64 mid = lo + (hi - lo + 1) / 2;
        if (a[mid - bias] <= p)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// 32 bits of the stream from base p0 on (16 codes); no word at or beyond n_words is read, and none that holds no base
// at or behind p0
__device__ __forceinline__ u32 export_codes(const u64 *__restrict__ words, u64 n_words, u64 n_bases, u64 p0)
{
    if (p0 >= n_bases)
        return 0;
    const u64 w = p0 >> 5;
    const unsigned sh = (unsigned)(p0 & 31) * 2;
    const u64 lo = words[w];
    const u64 hi = sh > 32 && w + 1 < n_words ? words[w + 1] : 0;
    return (u32)funnel(lo, hi, sh);
}

// the letters of four codes (8 bits): every code picks its byte of "ATCG"
__device__ __forceinline__ u32 export_letters4(u32 x)
{
    const u32 sel = (x | (x << 6) | (x << 12) | (x << 18)) & 0x03030303u;
    return __builtin_amdgcn_perm(0u, 0x47435441u, sel);
}

// What a tile knows about the body of its first record: the line and column of body offset bo0, so that a chunk of that
// record divides a small number.
struct ExportHint {
    u64 rec, bo0, q0, col0;
};

// the number of record s's name; NAMED: where its name begins in the column's bytes (what ExportRec.number then holds)
template <bool NAMED>
__device__ __forceinline__ u64 export_name_of(const ExportRead &A, const ExportNames &N, u64 s)
{
    if constexpr (NAMED)
        return N.off[s];
    else
        return A.numbers ? A.numbers[s] : A.name_base + s;
}

// sixteen bytes of a names column from byte a on, as aligned words; the column's allocation has NAMES_SLACK bytes behind
// its last byte, so the fifth word is inside it
__device__ __forceinline__ QualsBytes export_name16(const ExportNames &N, u64 a)
{
    const u32 mis = (u32)(reinterpret_cast<uintptr_t>(N.bytes + a) & 3);
    const u32 *q = reinterpret_cast<const u32 *>(N.bytes + a - mis);
    u32 d[5];
#pragma unroll
    for (u32 i = 0; i < 4; i++)
        d[i] = q[i];
    d[4] = mis ? q[4] : 0u;
    return quals_from_words(d, mis);
}

// One chunk: bytes [j0, j1) of the 16 bytes at out (16-byte aligned), the first of them byte p of the image, which lies
// in record s.  Record i's offset and first base are posA[i - bias] and startA[i - bias].
template <bool NAMED>
__device__ __forceinline__ void export_chunk(const ExportRead &A, const ExportNames &N, const u64 *posA, const u64 *startA, u64 bias,
                                             u64 s, u64 p, const ExportHint &h, u32 j0, u32 j1, unsigned char *out)
{
    const ExportFmt &f = A.fmt;
    u64 rp = posA[s - bias], st = startA[s - bias];
    ExportRec r;
    r.len = startA[s + 1 - bias] - st;
    r.header_len = export_header_from_size(f, r.len, posA[s + 1 - bias] - rp);
    r.number = 0;
    ExportCursor c = export_locate(f, r, p - rp, [&](u64 bo, u64 d, u64 *q, u64 *m) {
        const bool first = s == h.rec;
        const u64 x = first ? h.col0 + (bo - h.bo0) : bo;          // below d + the tile's bytes
        const u64 qb = first ? h.q0 : 0;
        if ((d >> 31) == 0) {
            *q = qb + (u32)x / (u32)d;
            *m = (u32)x % (u32)d;
        } else {
            const bool ge = x >= d;
            *q = qb + ge;
            *m = ge ? x - d : x;
        }
    });
    if (c.phase == 0)
        r.number = export_name_of<NAMED>(A, N, s);
    const bool whole = j0 == 0 && j1 == EXPORT_CHUNK;
    if constexpr (NAMED) {
        if (whole && c.phase == 0 && c.rem >= EXPORT_CHUNK) {       // inside one header: the name's bytes as words
            QualsBytes v = export_name16(N, r.number + (c.idx ? c.idx - 1 : 0));
            if (c.idx == 0) {                                        // the marker, then the name's first fifteen bytes
                v.hi = (v.hi << 8) | (v.lo >> 56);
                v.lo = (v.lo << 8) | (u64)(f.format == EXPORT_FASTA ? '>' : '@');
            }
            *reinterpret_cast<uint4 *>(out) = make_uint4((u32)v.lo, (u32)(v.lo >> 32), (u32)v.hi, (u32)(v.hi >> 32));
            return;
        }
    }
    if (whole && c.phase == 6 && c.rem >= EXPORT_CHUNK) {
        const u32 v = f.quality * 0x01010101u;
        *reinterpret_cast<uint4 *>(out) = make_uint4(v, v, v, v);
        return;
    }
    u32 bits = export_codes(A.words, A.n_words, A.n_bases, st + c.base);
    if (whole && c.phase == 2 && c.rem >= EXPORT_CHUNK) {           // inside one sequence line: no per-byte branch
        *reinterpret_cast<uint4 *>(out) = make_uint4(export_letters4(bits & 0xff), export_letters4((bits >> 8) & 0xff),
                                                     export_letters4((bits >> 16) & 0xff), export_letters4(bits >> 24));
        return;
    }
    if (whole && f.format != EXPORT_FASTQ && (c.phase == 2 || c.phase == 3)) {
        // One line end inside the chunk: k bases, the tb bytes of the terminator that are still to come, and bases again --
        // of the record's next line (FASTA) or of the next record (LINES; it holds a byte of the chunk, so it is among the
        // tile's).  The same 16 letters, the later ones moved up by the terminator.
        const u32 k = c.phase == 2 ? (u32)c.rem : 0;
        const u32 tb = c.phase == 2 ? f.term : (u32)c.rem;
        const u32 rest = k + tb < EXPORT_CHUNK ? EXPORT_CHUNK - k - tb : 0;
        u64 next = 0;                                // the bases that follow the terminator without another line end
        if (f.format == EXPORT_FASTA) {
            const u64 left = r.len - (c.base + k), w = export_line_bases(f, r.len);
            next = left < w ? left : w;
        } else if (rest) {
            next = startA[s + 2 - bias] - startA[s + 1 - bias];
        }
        if (rest <= next) {
            typedef unsigned __int128 u128;
            const u128 x = (u128)(export_letters4(bits & 0xff) | (u64)export_letters4((bits >> 8) & 0xff) << 32) |
                           (u128)(export_letters4((bits >> 16) & 0xff) | (u64)export_letters4(bits >> 24) << 32) << 64;
            const u128 term = tb == 2 ? 0x0A0Du : 0x0Au;                   // "\r\n", or "\n" (all of it, or its second byte)
            u128 v = term << (8 * k);
            if (k)
                v |= x & (((u128)1 << (8 * k)) - 1);
            if (rest)
                v |= (x >> (8 * k)) << (8 * (k + tb));
            *reinterpret_cast<uint4 *>(out) = make_uint4((u32)v, (u32)(v >> 32), (u32)(v >> 64), (u32)(v >> 96));
            return;
        }
    }
    u64 lo = 0, hi = 0;
#pragma unroll 1
    for (u32 j = j0; j < j1; j++) {
        while (c.rem == 0) {
            if (!export_advance(f, r, c)) {          // the next record: it holds byte j, so it exists
                s++;
                rp = posA[s - bias];
                st = startA[s - bias];
                r.len = startA[s + 1 - bias] - st;
                r.header_len = export_header_from_size(f, r.len, posA[s + 1 - bias] - rp);
                c = export_begin(f, r);
                if (c.phase == 0)
                    r.number = export_name_of<NAMED>(A, N, s);
            }
        }
        u64 b;
        if (NAMED && c.phase == 0) {
            b = c.idx == 0 ? (u64)(f.format == EXPORT_FASTA ? '>' : '@') : (u64)N.bytes[r.number + c.idx - 1];
            c.idx++;
            c.rem--;
        } else {
            b = export_emit(f, r, c, A.prefix, [&]() {
                const u32 code = bits & 3;
                bits >>= 2;
                return code;
            });
        }
        if (j < 8)
            lo |= b << (8 * j);
        else
            hi |= b << (8 * (j - 8));
    }
    if (whole) {
        *reinterpret_cast<uint4 *>(out) = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
    } else {                                         // the window's head or tail: only its own bytes
        for (u32 j = j0; j < j1; j++)
            out[j] = (unsigned char)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xff);
    }
}

template <bool NAMED>
__device__ __forceinline__ void export_tile_chunks(const ExportRead &A, const ExportNames &N, const u64 *posA, const u64 *startA,
                                                   u64 bias, u64 lo, u64 hi, const ExportHint &h, u64 v_tile, u32 a, u64 v_end)
{
    const u32 tid = threadIdx.x;
    unsigned char *dst_al = A.dst - a;
    u64 rec[EXPORT_CHUNKS_PER_THREAD];
#pragma unroll
    for (u32 k = 0; k < EXPORT_CHUNKS_PER_THREAD; k++) {             // the searches first: their loads overlap
        const u64 v = v_tile + (u64)(k * EXPORT_THREADS + tid) * EXPORT_CHUNK;
        const u64 v0 = v < a ? a : v;
        rec[k] = v0 < v_end && v + EXPORT_CHUNK > a ? export_record_of(posA, bias, lo, hi, A.first_byte + v0 - a) : lo;
    }
#pragma unroll 1
    for (u32 k = 0; k < EXPORT_CHUNKS_PER_THREAD; k++) {
        const u64 v = v_tile + (u64)(k * EXPORT_THREADS + tid) * EXPORT_CHUNK;
        if (v >= v_end || v + EXPORT_CHUNK <= a)
            continue;
        const u32 j0 = v < a ? a - (u32)v : 0;
        const u32 j1 = v_end - v < EXPORT_CHUNK ? (u32)(v_end - v) : EXPORT_CHUNK;
        export_chunk<NAMED>(A, N, posA, startA, bias, rec[k], A.first_byte + v + j0 - a, h, j0, j1, dst_al + v);
    }
}

// ---- the sweep.  With a = the destination's address mod 16, byte i of the window is "virtual" byte a + i, and a workgroup
// owns virtual bytes [blockIdx.x * EXPORT_TILE_BYTES, + EXPORT_TILE_BYTES): its chunks are 16-byte aligned in memory whatever
// the caller's pointer and first_byte are, lane t forms chunks t, t + 256, .. and stores each once, whole; only the chunks
// that hold the window's first and last byte are stored byte by byte.  The workgroup finds the records of its first and last
// byte once (take_copy_kernel's way), brings the offsets and first bases of the records between them into LDS when they are
// at most EXPORT_LDS_RECS, and every lane searches for the record of its chunk's first byte there.  count > 0.
template <bool NAMED>
__device__ __forceinline__ void export_read_body(const ExportRead &A, const ExportNames &N)
{
    __shared__ u32 wc[EXPORT_THREADS / 64], wle[EXPORT_THREADS / 64];
    __shared__ u64 s_pos[EXPORT_LDS_RECS + 1], s_start[EXPORT_LDS_RECS + 1];
    const u32 tid = threadIdx.x;
    const u64 n = A.n;
    const u32 a = (u32)(reinterpret_cast<uintptr_t>(A.dst) & 15);
    const u64 v_end = a + A.count;
    const u64 v_tile = (u64)blockIdx.x * EXPORT_TILE_BYTES;
    const u64 v_first = v_tile < a ? a : v_tile;
    const u64 v_last = (v_tile + EXPORT_TILE_BYTES < v_end ? v_tile + EXPORT_TILE_BYTES : v_end) - 1;
    const u64 p_first = A.first_byte + v_first - a, p_last = A.first_byte + v_last - a;
    // pos[0 .. ub_lo) lie at or below the tile's first byte: entry 0 is 0, entry n = the image's size is above every byte
    const u64 ub_lo = export_block_upper_bound(A.pos, 1, n, p_first, wc);
    const u64 sv = ub_lo + tid < n ? A.pos[ub_lo + tid] : ~(u64)0;
    const u32 nle = (u32)__popcll(__ballot(sv <= p_last));
    if ((tid & 63) == 0)
        wle[tid >> 6] = nle;
    __syncthreads();
    u32 n_le = 0;
#pragma unroll
    for (u32 w = 0; w < EXPORT_THREADS / 64; w++)
        n_le += wle[w];
    u64 ub_hi = ub_lo + n_le;
    if (n_le == EXPORT_THREADS && ub_hi < n)         // uniform
        ub_hi = export_block_upper_bound(A.pos, ub_hi, n, p_last, wc);
    const u64 rec_lo = ub_lo - 1, rec_hi = ub_hi - 1;

    // the first record's body at the tile's first byte: the one 64-bit division of the tile
    ExportHint h = {rec_lo, 0, 0, 0};
    if (A.fmt.format == EXPORT_FASTA) {
        const u64 rp = A.pos[rec_lo], len = A.starts[rec_lo + 1] - A.starts[rec_lo];
        const u64 body = rp + export_header_from_size(A.fmt, len, A.pos[rec_lo + 1] - rp) + A.fmt.term;
        const u64 w = export_line_bases(A.fmt, len);
        h.bo0 = p_first > body ? p_first - body : 0;
        if (w < len) {
            h.q0 = h.bo0 / (w + A.fmt.term);
            h.col0 = h.bo0 % (w + A.fmt.term);
        }
    }

    const u64 m = rec_hi - rec_lo + 1;               // the tile's records: rec_lo .. rec_hi
    if (m <= EXPORT_LDS_RECS) {                      // uniform
        for (u32 i = tid; i <= (u32)m; i += EXPORT_THREADS) {
            s_pos[i] = A.pos[rec_lo + i];
            s_start[i] = A.starts[rec_lo + i];
        }
        __syncthreads();
        export_tile_chunks<NAMED>(A, N, s_pos, s_start, rec_lo, rec_lo, rec_hi, h, v_tile, a, v_end);
    } else {
        export_tile_chunks<NAMED>(A, N, A.pos, A.starts, 0, rec_lo, rec_hi, h, v_tile, a, v_end);
    }
}
__global__ __launch_bounds__(EXPORT_THREADS) void export_read_kernel(const ExportRead A)
{
    export_read_body<false>(A, ExportNames{nullptr, nullptr});
}
// the image of dnagpu_table_to_text_named: every header is its marker and the string of N
__global__ __launch_bounds__(EXPORT_THREADS) void export_read_named_kernel(const ExportRead A, const ExportNames N)
{
    export_read_body<true>(A, N);
}

hipError_t launch_export_plan(const u64 *starts, u64 n, const u64 *numbers, u64 name_base, const ExportFmt &f, u32 *ex32,
                              unsigned long long *res2, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(res2, 0, 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess || n == 0)
        return e;
    const u64 blocks = (n + EXPORT_THREADS - 1) / EXPORT_THREADS;
    hipLaunchKernelGGL(export_plan_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(EXPORT_THREADS), 0, s, starts, n,
                       numbers, name_base, f, ex32, res2);
    return hipGetLastError();
}

hipError_t launch_export_plan_named(const u64 *starts, u64 n, const u64 *name_off, const ExportFmt &f, u32 *ex32,
                                    unsigned long long *res2, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(res2, 0, 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess || n == 0)
        return e;
    const u64 blocks = (n + EXPORT_THREADS - 1) / EXPORT_THREADS;
    hipLaunchKernelGGL(export_plan_named_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(EXPORT_THREADS), 0, s, starts, n,
                       name_off, f, ex32, res2);
    return hipGetLastError();
}

hipError_t launch_export_pos(const u64 *starts, const u32 *scan, u64 n, u64 total, u64 *pos, hipStream_t s)
{
    hipLaunchKernelGGL(export_pos_kernel, dim3((unsigned)((n + 1 + EXPORT_THREADS - 1) / EXPORT_THREADS)), dim3(EXPORT_THREADS), 0, s,
                       starts, scan, n, total, pos);
    return hipGetLastError();
}

hipError_t launch_export_read(const ExportRead &a, hipStream_t s)
{
    if (a.count == 0)
        return hipSuccess;
    const u64 v_end = (reinterpret_cast<uintptr_t>(a.dst) & 15) + a.count;
    hipLaunchKernelGGL(export_read_kernel, dim3((unsigned)((v_end + EXPORT_TILE_BYTES - 1) / EXPORT_TILE_BYTES)), dim3(EXPORT_THREADS),
                       0, s, a);
    return hipGetLastError();
}

hipError_t launch_export_read_named(const ExportRead &a, const ExportNames &names, hipStream_t s)
{
    if (a.count == 0)
        return hipSuccess;
    const u64 v_end = (reinterpret_cast<uintptr_t>(a.dst) & 15) + a.count;
    hipLaunchKernelGGL(export_read_named_kernel, dim3((unsigned)((v_end + EXPORT_TILE_BYTES - 1) / EXPORT_TILE_BYTES)),
                       dim3(EXPORT_THREADS), 0, s, a, names);
    return hipGetLastError();
}

}  // namespace dnagpu
