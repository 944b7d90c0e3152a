// text_math.hpp -- what the kernels of dnagpu_table_from_text (text_kernels.hip), its host driver (text_host.hip) and the host
// check tests/host/text_math_check.cpp share: the class of a byte, the bit masks of one lane's 32 bytes
// (terminators, line starts, header lines, the bases that are kept), the packing of the kept bases, the error word, the
// cut of a chunk that is followed by more text, and the size formulas.
//
// A lane owns TEXT_CHUNK = 32 consecutive bytes of the text: bit j of every mask below is byte j of the chunk, and the
// 2-bit codes of its bytes are one packed word.  A workgroup of TEXT_THREADS lanes sweeps one tile of TEXT_TILE_BYTES.
#pragma once
#include "kmer_device.hpp"

namespace dnagpu {

constexpr int TEXT_FORMAT_LINES = 1, TEXT_FORMAT_FASTA = 2;       // DNAGPU_TEXT_LINES, DNAGPU_TEXT_FASTA
constexpr u32 TEXT_THREADS = 256;
constexpr u32 TEXT_CHUNK = 32;
constexpr u32 TEXT_TILE_BYTES = TEXT_THREADS * TEXT_CHUNK;

__host__ __device__ __forceinline__ u64 text_tiles(u64 n_bytes) { return (n_bytes + TEXT_TILE_BYTES - 1) / TEXT_TILE_BYTES; }
__host__ __device__ __forceinline__ u64 text_words(u64 n_bases) { return (n_bases + 31) / 32; }

// 'A','T','C','G' -> 0,1,2,3 (dna.c:120-123); anything else -> 4
__host__ __device__ __forceinline__ u32 base_code(u32 c)
{
    u32 t = (c >> 1) & 3;                        // A=0 C=1 T=2 G=3
    u32 code = ((t & 1) << 1) | (t >> 1);        // A=0 T=1 C=2 G=3
    u32 expect = (0x47544341u >> (8 * t)) & 0xff;   // "ACTG"[t]
    return c == expect ? code : 4u;
}

// ---- the error word: (byte offset << 2) | kind, so that a 64-bit minimum keeps the error with the lowest offset (COPY
// stops at the first bad row).  No byte carries two kinds.
constexpr u64 TEXT_NO_ERROR = ~(u64)0;
constexpr u32 TEXT_ERR_EMPTY = 0;        // DNAGPU_ERR_DNA_EMPTY: an empty line (LINES), a record without sequence (FASTA)
constexpr u32 TEXT_ERR_CHAR = 1;         // DNAGPU_ERR_DNA_INVALID_CHAR
constexpr u32 TEXT_ERR_ORPHAN = 2;       // FASTA: sequence data before the first header
__host__ __device__ __forceinline__ u64 text_error_key(u64 pos, u32 kind) { return (pos << 2) | kind; }
__host__ __device__ __forceinline__ u64 text_error_pos(u64 key) { return key >> 2; }
__host__ __device__ __forceinline__ u32 text_error_kind(u64 key) { return (u32)(key & 3); }

// ---- bit masks of one chunk
__host__ __device__ __forceinline__ u32 text_low_bits(u32 j) { return j >= 32 ? ~0u : (1u << j) - 1; }      // bits [0, j)
__host__ __device__ __forceinline__ u32 text_bit_range(u32 a, u32 b) { return text_low_bits(b) & ~text_low_bits(a); }   // [a, b)
__host__ __device__ __forceinline__ u32 text_top_bit(u32 m) { return 31u - (u32)__builtin_clz(m); }         // m != 0

struct TextChunk {
    u32 valid;       // bytes of the chunk that lie inside the text
    u32 base;        // A / T / C / G
    u32 nl, cr, gt;  // '\n', '\r', '>'
    u64 codes;       // 2-bit code of every byte (0 where it is no base)
    bool prev_nl;    // the byte before the chunk is '\n', or the chunk is the text's first
    bool next_nl;    // the byte behind the chunk exists and is '\n'
};
__host__ __device__ __forceinline__ void text_chunk_byte(TextChunk &c, u32 j, u32 byte)
{
    const u32 code = base_code(byte);
    c.base |= (u32)(code < 4) << j;
    c.codes |= (u64)(code & 3) << (2 * j);
    c.nl |= (u32)(byte == '\n') << j;
    c.cr |= (u32)(byte == '\r') << j;
    c.gt |= (u32)(byte == '>') << j;
}

// A line ends at '\n'; a '\r' directly before that '\n' belongs to the terminator.
__host__ __device__ __forceinline__ u32 text_terminators(const TextChunk &c)
{
    return c.nl | (c.cr & ((c.nl >> 1) | ((u32)c.next_nl << 31)));
}
// the first byte of every line: byte 0 of the text and every byte behind a '\n'
__host__ __device__ __forceinline__ u32 text_line_starts(const TextChunk &c)
{
    return ((c.nl << 1) | (u32)c.prev_nl) & c.valid;
}
// invalid characters, were every line a sequence line: neither a base nor part of a terminator
__host__ __device__ __forceinline__ u32 text_invalid(const TextChunk &c)
{
    return c.valid & ~c.base & ~text_terminators(c);
}
// The bytes of the chunk that lie in header lines: starts = text_line_starts, headers = the starts whose byte is '>',
// in_header = whether the line that reaches into the chunk from before is a header.
__host__ __device__ __forceinline__ u32 text_header_bytes(u32 starts, u32 headers, bool in_header)
{
    u32 m = 0, from = 0;
    while (starts) {
        const u32 j = (u32)__builtin_ctz(starts);
        if (in_header)
            m |= text_bit_range(from, j);
        in_header = (headers >> j) & 1;
        from = j;
        starts &= starts - 1;
    }
    return in_header ? m | text_bit_range(from, 32) : m;
}
// the codes of the bytes in `keep`, closed up: popcount(keep) bases from bit 0 on, zero behind them
__host__ __device__ __forceinline__ u64 text_compact(u64 codes, u32 keep)
{
    if (keep == ~0u)
        return codes;
    u64 v = 0;
    u32 at = 0;
    while (keep) {                                   // run by run: a line's bases are one run
        const u32 j = (u32)__builtin_ctz(keep);
        const u32 rest = ~(keep >> j);               // (its top j bits are set: the run ends inside the word)
        const u32 run = rest ? (u32)__builtin_ctz(rest) : 32u;
        v |= ((codes >> (2 * j)) & kmer_mask((int)run)) << (2 * at);
        at += run;
        keep &= ~(text_low_bits(run) << j);
    }
    return v;
}

// ---- the cut of a chunk that more text follows (DNAGPU_TEXT_MORE): everything from the cut on is held back.
// LINES: one past the last '\n' (0: none).  FASTA: the '>' of the last header (no header: n, there is no record to hold).
// text_is_cut(p): p is a place where a record may begin -- the candidates the kernel takes the greatest of.
__host__ __device__ __forceinline__ bool text_is_cut(const unsigned char *text, u64 n, int format, u64 p)
{
    const bool line_start = p == 0 || text[p - 1] == '\n';
    if (format == TEXT_FORMAT_LINES)
        return p > 0 && p <= n && line_start;
    return p < n && line_start && text[p] == '>';
}
__host__ __device__ __forceinline__ u64 text_no_cut(u64 n, int format) { return format == TEXT_FORMAT_LINES ? 0 : n; }
inline u64 text_more_cut(const unsigned char *text, u64 n, int format)      // the host's serial form (the check's reference)
{
    for (u64 p = n + 1; p-- > 0;)
        if (text_is_cut(text, n, format, p))
            return p;
    return text_no_cut(n, format);
}

// ================================================================ dnagpu_reads_from_text
// The general entry reads the same chunks.  What it adds: FASTQ (the role of a line is its index mod 4), the IUPAC
// ambiguity letters as a class of their own, lower-case bases, and the starts of the pieces a record is cut into.
constexpr int TEXT_FORMAT_FASTQ = 3;                               // DNAGPU_TEXT_FASTQ
constexpr int READS_AMBIG_ERROR = 0, READS_AMBIG_DROP = 1, READS_AMBIG_SPLIT = 2;      // DNAGPU_AMBIG_*

// The error word of the general entry is text_error_key's with one more kind.  TEXT_ERR_ORPHAN stands for every "a record
// does not open as it must" (FASTA: data before the first header; FASTQ: no '@', no '+' -- the line's role tells which),
// so that at equal offsets it comes before TEXT_ERR_TRUNC.
constexpr u32 TEXT_ERR_TRUNC = 3;        // FASTQ without MORE: the lines are no multiple of four

// N R Y K M S W B D H V as bits of letter - 'A'
constexpr u32 READS_AMBIG_LETTERS = (1u << ('N' - 'A')) | (1u << ('R' - 'A')) | (1u << ('Y' - 'A')) | (1u << ('K' - 'A')) |
                                    (1u << ('M' - 'A')) | (1u << ('S' - 'A')) | (1u << ('W' - 'A')) | (1u << ('B' - 'A')) |
                                    (1u << ('D' - 'A')) | (1u << ('H' - 'A')) | (1u << ('V' - 'A'));
// DNAGPU_READS_FOLD_CASE: a lower-case letter counts as its upper case; every other byte is itself
__host__ __device__ __forceinline__ u32 reads_fold(u32 byte, bool fold)
{
    return fold && byte >= 'a' && byte <= 'z' ? byte - 32 : byte;
}
__host__ __device__ __forceinline__ bool reads_is_ambig(u32 byte)      // byte: folded already
{
    return byte >= 'A' && byte <= 'Z' && ((READS_AMBIG_LETTERS >> (byte - 'A')) & 1);
}

struct ReadsChunk {
    TextChunk c;     // (base and codes: after folding)
    u32 amb;         // ambiguity letters
    u32 at, plus;    // '@', '+'
};
__host__ __device__ __forceinline__ void reads_chunk_byte(ReadsChunk &r, u32 j, u32 byte, bool fold)
{
    const u32 up = reads_fold(byte, fold);
    text_chunk_byte(r.c, j, up);
    r.amb |= (u32)reads_is_ambig(up) << j;
    r.at |= (u32)(byte == '@') << j;
    r.plus |= (u32)(byte == '+') << j;
}

// FASTQ: role[q] = the bytes of the chunk that lie in lines of role q = line index mod 4 (0 '@' line, 1 sequence, 2 '+'
// line, 3 quality).  nl: the chunk's '\n' (a '\n' belongs to the line it ends); line0: the '\n' before the chunk.
__host__ __device__ __forceinline__ void reads_roles(u32 nl, u32 line0, u32 role[4])
{
    u32 from = 0, q = line0 & 3;
    role[0] = role[1] = role[2] = role[3] = 0;
    while (nl) {
        const u32 j = (u32)__builtin_ctz(nl);
        role[q] |= text_bit_range(from, j + 1);
        from = j + 1;
        q = (q + 1) & 3;
        nl &= nl - 1;
    }
    role[q] |= text_bit_range(from, 32);
}
// the k-th set bit of m, k from 1; m has at least k bits
__host__ __device__ __forceinline__ u32 text_nth_bit(u32 m, u32 k)
{
    while (--k)
        m &= m - 1;
    return (u32)__builtin_ctz(m);
}

// DNAGPU_AMBIG_SPLIT: the kept bases that begin a piece.  A base begins one iff no kept base lies between it and the last
// break at or before it; keep: the kept bases of the chunk, brk: its breaks (ambiguity letters of sequence lines and record
// openers).  Positions are 1 + the offset inside the tile, 0 = none: at that of the chunk's byte 0, pk / pb those of the
// last kept base / break before the chunk.  *undecided = the one bit that the tile cannot decide: a kept base with neither
// a kept base nor a break before it in the tile (the tiles before decide: reads_finish_kernel).
__host__ __device__ __forceinline__ u32 reads_piece_starts(u32 keep, u32 brk, u32 at, u32 pk, u32 pb, u32 *undecided)
{
    u32 cand = keep & (~(keep << 1) | brk), m = 0;   // the first base of every run of kept bases, and a base that is a break
    *undecided = 0;
    while (cand) {
        const u32 j = (u32)__builtin_ctz(cand);
        const u32 kb = keep & text_low_bits(j), bb = brk & text_low_bits(j + 1);
        const u32 k = kb ? at + text_top_bit(kb) : pk, b = bb ? at + text_top_bit(bb) : pb;
        if (!(k | b))
            *undecided = 1u << j;
        else if (k < b)
            m |= 1u << j;
        cand &= cand - 1;
    }
    return m;
}

// FASTQ: what the newline count decides.  lines: L '\n' in the text, one more line when the last byte is none.  The
// newline that ends the last whole record is number fastq_cut_newline (from 1; 0: there is no whole record): one past it
// DNAGPU_TEXT_MORE cuts, and there the truncated record begins.
__host__ __device__ __forceinline__ u64 fastq_lines(u64 newlines, bool ends_in_newline) { return newlines + (ends_in_newline ? 0 : 1); }
__host__ __device__ __forceinline__ u64 fastq_cut_newline(u64 newlines, bool ends_in_newline, bool more)
{
    return (more ? newlines : fastq_lines(newlines, ends_in_newline)) / 4 * 4;
}

}  // namespace dnagpu
