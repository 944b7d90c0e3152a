// export_math.hpp -- what the kernels of dnagpu_table_to_text (export_kernels.hip), its host driver (export_host.hip) and the
// host check tests/host/export_math_check.cpp share: the digits of a 64-bit number, the length of a header,
// the bytes of a record beside its bases, and the map from an offset inside a record to the byte that stands there.
//
// A record is a sequence of RUNS, and a cursor stands in one of them:
//   phase 0 header ('>' or '@', the prefix, the digits)   1 its terminator
//   phase 2 a sequence line's bases                      3 its terminator
//   phase 4 '+'    5 its terminator    6 the quality bytes    7 their terminator           (FASTQ only)
// LINES records are phases 2 3; FASTA records 0 1 (2 3)*, one (2 3) per line; FASTQ records 0 .. 7.  export_locate puts a
// cursor on any offset of a record with one division; export_emit walks on from there, byte by byte, and never looks
// at a record it has no byte of.
#pragma once
#include "kmer_device.hpp"

namespace dnagpu {

constexpr int EXPORT_LINES = 1, EXPORT_FASTA = 2, EXPORT_FASTQ = 3;     // DNAGPU_TEXT_LINES, _FASTA, _FASTQ
constexpr u32 EXPORT_PREFIX_MAX = 64;
constexpr u32 EXPORT_THREADS = 256;
constexpr u32 EXPORT_CHUNK = 16;                 // bytes one lane forms at a time: one uint4 store
constexpr u32 EXPORT_CHUNKS_PER_THREAD = 8;
constexpr u32 EXPORT_TILE_BYTES = EXPORT_THREADS * EXPORT_CHUNK * EXPORT_CHUNKS_PER_THREAD;
constexpr u32 EXPORT_LDS_RECS = 1024;            // records of a tile whose offsets are staged in LDS (32-byte records on average)

struct ExportFmt {
    int format;
    u32 term;        // bytes of a terminator: 1 "\n", 2 "\r\n"
    u64 width;       // FASTA: bases per sequence line, 0 = the whole sequence on one line
    u32 prefix_len;
    u32 quality;     // the byte of every quality line
};

// decimal digits of v, 1 .. 20
__host__ __device__ __forceinline__ u32 export_digits(u64 v)
{
    u32 d = 1;
    while (v >= 10) {
        v /= 10;
        d++;
    }
    return d;
}
// digit i (0 = the most significant) of v, which has nd digits
__host__ __device__ __forceinline__ u32 export_digit_at(u64 v, u32 nd, u32 i)
{
    for (u32 j = i + 1; j < nd; j++)
        v /= 10;
    return (u32)(v % 10);
}
// '>' or '@', the prefix, the digits; LINES records have no header
__host__ __device__ __forceinline__ u32 export_header_len(const ExportFmt &f, u64 number)
{
    return f.format == EXPORT_LINES ? 0u : 1u + f.prefix_len + export_digits(number);
}
// bases of every full sequence line of a record of len bases (FASTA), and the lines
__host__ __device__ __forceinline__ u64 export_line_bases(const ExportFmt &f, u64 len)
{
    return f.width == 0 || f.width >= len ? len : f.width;
}
__host__ __device__ __forceinline__ u64 export_lines(const ExportFmt &f, u64 len)
{
    if (len == 0)
        return 0;
    const u64 w = export_line_bases(f, len);
    return (len + w - 1) / w;
}
// bytes of a record's body: everything behind the header line
__host__ __device__ __forceinline__ u64 export_body_bytes(const ExportFmt &f, u64 len)
{
    if (f.format == EXPORT_LINES)
        return len + f.term;
    if (f.format == EXPORT_FASTA)
        return len + export_lines(f, len) * f.term;
    return 2 * len + 3 * (u64)f.term + 1;
}
// bytes of a record that are not bases of a sequence line
__host__ __device__ __forceinline__ u64 export_extras(const ExportFmt &f, u64 len, u32 header_len)
{
    const u64 head = f.format == EXPORT_LINES ? 0 : (u64)header_len + f.term;
    return head + export_body_bytes(f, len) - len;
}
// the header's length from the record's size: the kernels never need the number to find their way
__host__ __device__ __forceinline__ u32 export_header_from_size(const ExportFmt &f, u64 len, u64 record_bytes)
{
    return f.format == EXPORT_LINES ? 0u : (u32)(record_bytes - export_body_bytes(f, len) - f.term);
}

struct ExportRec {
    u64 len;         // bases
    u64 number;      // the number of its name (read only while a header's digits are formed)
    u32 header_len;
};

struct ExportCursor {
    u32 phase;
    u32 idx;         // phases 0 1 3 5 7: the byte inside the run
    u64 rem;         // bytes of the run that are left, the cursor's included
    u64 base;        // the next base of the sequence that a phase 2 forms
};

__host__ __device__ __forceinline__ u64 export_line_run(const ExportFmt &f, const ExportRec &r, u64 base)
{
    const u64 left = r.len - base;
    if (f.format != EXPORT_FASTA)
        return left;
    const u64 w = export_line_bases(f, r.len);
    return left < w ? left : w;
}

// the cursor on a record's first run (which may be empty: the walk steps over empty runs with export_advance)
__host__ __device__ __forceinline__ ExportCursor export_begin(const ExportFmt &f, const ExportRec &r)
{
    ExportCursor c;
    c.idx = 0;
    c.base = 0;
    if (f.format == EXPORT_LINES) {
        c.phase = 2;
        c.rem = r.len;
    } else {
        c.phase = 0;
        c.rem = r.header_len;
    }
    return c;
}

// the run behind the cursor's; false: the record has none
__host__ __device__ __forceinline__ bool export_advance(const ExportFmt &f, const ExportRec &r, ExportCursor &c)
{
    c.idx = 0;
    switch (c.phase) {
    case 0:
        c.phase = 1;
        c.rem = f.term;
        return true;
    case 1:
        if (f.format == EXPORT_FASTA && r.len == 0)
            return false;                        // a header with no sequence line
        c.phase = 2;
        c.rem = export_line_run(f, r, c.base);
        return true;
    case 2:
        c.phase = 3;
        c.rem = f.term;
        return true;
    case 3:
        if (f.format == EXPORT_LINES)
            return false;
        if (f.format == EXPORT_FASTA) {
            if (c.base >= r.len)
                return false;
            c.phase = 2;
            c.rem = export_line_run(f, r, c.base);
            return true;
        }
        c.phase = 4;
        c.rem = 1;
        return true;
    case 4:
        c.phase = 5;
        c.rem = f.term;
        return true;
    case 5:
        c.phase = 6;
        c.rem = r.len;
        return true;
    case 6:
        c.phase = 7;
        c.rem = f.term;
        return true;
    default:
        return false;
    }
}

__host__ __device__ __forceinline__ ExportCursor export_cursor(u32 phase, u32 idx, u64 rem, u64 base)
{
    ExportCursor c;
    c.phase = phase;
    c.idx = idx;
    c.rem = rem;
    c.base = base;
    return c;
}

// The cursor on offset off < the record's bytes.  divmod(x, d, &q, &m) divides an offset inside a FASTA body by the line
// pitch: the one division of a chunk (the kernel's works from what its tile already knows).
template <typename D>
__host__ __device__ __forceinline__ ExportCursor export_locate(const ExportFmt &f, const ExportRec &r, u64 off, D &&divmod)
{
    const u32 t = f.term;
    if (f.format != EXPORT_LINES) {
        if (off < r.header_len)
            return export_cursor(0, (u32)off, r.header_len - off, 0);
        off -= r.header_len;
        if (off < t)
            return export_cursor(1, (u32)off, t - off, 0);
        off -= t;
    }
    if (f.format == EXPORT_FASTA) {
        const u64 w = export_line_bases(f, r.len);
        u64 q = 0, col = off;
        if (w < r.len)
            divmod(off, w + t, &q, &col);
        const u64 line0 = q * w, left = r.len - line0;
        const u64 line = left < w ? left : w;
        if (col < line)
            return export_cursor(2, 0, line - col, line0 + col);
        return export_cursor(3, (u32)(col - line), t - (col - line), line0 + line);
    }
    if (off < r.len)
        return export_cursor(2, 0, r.len - off, off);
    off -= r.len;
    if (off < t)
        return export_cursor(3, (u32)off, t - off, r.len);
    if (f.format == EXPORT_LINES)
        return export_cursor(3, 0, 0, r.len);    // (not reached: off lies inside the record)
    off -= t;
    if (off < 1)
        return export_cursor(4, 0, 1, r.len);
    off -= 1;
    if (off < t)
        return export_cursor(5, (u32)off, t - off, r.len);
    off -= t;
    if (off < r.len)
        return export_cursor(6, 0, r.len - off, r.len);
    off -= r.len;
    return export_cursor(7, (u32)off, t - off, r.len);
}

__host__ __device__ __forceinline__ u32 export_letter(u32 code) { return (0x47435441u >> (8 * (code & 3))) & 0xff; }   // A T C G

// The byte under the cursor of a non-empty run, and the cursor one byte on (inside the run: rem may become 0).
// prefix: the name's prefix; next_code(): the 2-bit code of the next base of the stream.
template <typename C>
__host__ __device__ __forceinline__ u32 export_emit(const ExportFmt &f, const ExportRec &r, ExportCursor &c,
                                                    const unsigned char *prefix, C &&next_code)
{
    u32 b;
    switch (c.phase) {
    case 0:
        if (c.idx == 0)
            b = f.format == EXPORT_FASTA ? '>' : '@';
        else if (c.idx <= f.prefix_len)
            b = prefix[c.idx - 1];
        else
            b = '0' + export_digit_at(r.number, r.header_len - 1 - f.prefix_len, c.idx - 1 - f.prefix_len);
        break;
    case 2:
        b = export_letter(next_code());
        c.base++;
        break;
    case 4:
        b = '+';
        break;
    case 6:
        b = f.quality;
        break;
    default:                                     // a terminator: "\n", or "\r\n"
        b = f.term == 2 && c.idx == 0 ? '\r' : '\n';
        break;
    }
    c.idx++;
    c.rem--;
    return b;
}

}  // namespace dnagpu
