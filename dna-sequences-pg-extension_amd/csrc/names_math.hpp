// names_math.hpp -- what the kernels of the names column (names_kernels.hip), its host driver (names_host.hip) and the host
// check tests/host/names_math_check.cpp share: the sizes of a column, the bytes that end a name, the search
// for the end of a name in the masks of a text, and the words a call brings home.
//
// A names column is n strings back to back: off[0 .. n] (off[0] = 0, ascending) and off[n] bytes, none of them '\n' or '\r'.
// The name of a sequence is the header line of its source record without the marker ('>' or '@') and without the line's
// terminator; with first_word it stops before the first blank or tab.  No thread walks a line: one sweep over the text
// writes, per chunk of TEXT_CHUNK bytes, the mask of the bytes that end a name, and per tile the first of them; a suffix
// minimum over the tiles tells every tile where the next one lies; a name then ends in the masks of the tile it begins in,
// or where the suffix minimum of the next tile says.
#pragma once
#include "quals_math.hpp"
#include "text_math.hpp"

namespace dnagpu {

constexpr u32 NAMES_THREADS = 256;
constexpr u32 NAMES_NONE = 0xFFFFFFFFu;              // no name ends here (offsets are below 2^32 - 1)
constexpr u32 NAMES_GROUP_TILES = NAMES_THREADS;     // tiles whose suffix minimum one workgroup forms
constexpr u32 NAMES_SLACK = 16;                      // bytes of a column's allocation behind its last whole chunk
constexpr u64 NAMES_NO_ERROR = ~(u64)0;
enum { NAMES_R_TOTAL, NAMES_R_BAD, NAMES_R_LONE_CR, NAMES_R_WORDS };

__host__ __device__ __forceinline__ u64 names_chunks(u64 n_bytes) { return (n_bytes + TEXT_CHUNK - 1) / TEXT_CHUNK; }
__host__ __device__ __forceinline__ u64 names_groups(u64 n_tiles) { return (n_tiles + NAMES_GROUP_TILES - 1) / NAMES_GROUP_TILES; }
// bytes of the allocation behind a column of `total` bytes: whole 16-byte chunks (the copy stores chunks whole) and the
// slack that lets the named image load sixteen bytes from any byte of a name as five aligned words
__host__ __device__ __forceinline__ u64 names_alloc_bytes(u64 total) { return quals_alloc_bytes(total) + NAMES_SLACK; }

__host__ __device__ __forceinline__ bool names_forbidden(u32 byte) { return byte == '\n' || byte == '\r'; }
__host__ __device__ __forceinline__ bool names_ends_here(u32 byte, bool first_word)
{
    return byte == '\n' || (first_word && (byte == ' ' || byte == '\t'));
}

// The first byte at or behind `from` that ends a name, n when there is none.  mask(c) = the mask of chunk c; local(t) /
// after(g) = the suffix minima of launch_names_suffix_min.  Mask words are read in the tile of `from` only.
template <typename Mask, typename Local, typename After>
__host__ __device__ __forceinline__ u64 names_end_from(u64 from, u64 n, Mask &&mask, Local &&local, After &&after)
{
    if (from >= n)
        return n;
    const u64 tile = from / TEXT_TILE_BYTES, n_tiles = text_tiles(n);
    const u64 c_end = (tile + 1) * TEXT_THREADS < names_chunks(n) ? (tile + 1) * TEXT_THREADS : names_chunks(n);
    u64 c = from / TEXT_CHUNK;
    u32 m = mask(c) & ~text_low_bits((u32)(from % TEXT_CHUNK));
    while (!m && ++c < c_end)
        m = mask(c);
    if (m)
        return c * TEXT_CHUNK + (u32)__builtin_ctz(m);
    if (tile + 1 >= n_tiles)
        return n;
    const u32 a = local(tile + 1), b = after((tile + 1) / NAMES_GROUP_TILES);
    const u32 e = a < b ? a : b;
    return e == NAMES_NONE ? n : e;
}

// [start, end) of the name whose marker is the byte at p < n: the line ends at `e` = names_end_from(p + 1); a '\r' directly
// before the '\n' that ends it belongs to the terminator
template <typename Byte>
__host__ __device__ __forceinline__ u64 names_strip(u64 start, u64 e, u64 n, Byte &&byte)
{
    if (e < n && e > start && byte(e) == '\n' && byte(e - 1) == '\r')
        e--;
    return e;
}

}  // namespace dnagpu
