// Host-side check of names_math.hpp (the arithmetic the kernels of the names column and their host driver share): for texts
// whose name-ending bytes are dense, sparse (tiles and whole groups of tiles without one) or absent, the masks, the per-tile
// firsts and the two levels of the suffix minimum are built the way the kernels build them, as vectors of exactly the sizes
// the host driver allocates -- the program fails under AddressSanitizer if an entry outside them is asked for -- and
// names_end_from must agree, from sampled and from edge start offsets, with a naive walk to the next such byte; then
// names_strip on the terminators and the size formulas.
// Built and run by tests/test_read_names.py with hipcc (host code only).
#include <cstdio>
#include <vector>
#include "names_math.hpp"

using namespace dnagpu;

static int bad = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (bad < 20) {                                   \
                printf(__VA_ARGS__);                          \
                printf("  [%s:%d]\n", __FILE__, __LINE__);    \
            }                                                 \
            bad++;                                            \
        }                                                     \
    } while (0)

static u64 rng_state = 0x13198A2E03707344ull;
static u64 rng() { return rng_state = splitmix64(rng_state); }

static void check_text(const std::vector<unsigned char> &text, bool first_word, const char *what)
{
    const u64 n = text.size(), nt = text_tiles(n), ng = names_groups(nt);
    std::vector<u32> mask((size_t)names_chunks(n), 0u), first((size_t)nt, NAMES_NONE), local((size_t)nt), after((size_t)ng);
    for (u64 i = 0; i < n; i++)
        if (names_ends_here(text[(size_t)i], first_word)) {
            mask[(size_t)(i / TEXT_CHUNK)] |= 1u << (i % TEXT_CHUNK);
            u32 &f = first[(size_t)(i / TEXT_TILE_BYTES)];
            if (f == NAMES_NONE)
                f = (u32)i;
        }
    u32 carry = NAMES_NONE;                          // over the groups, from the last
    for (u64 g = ng; g-- > 0;) {
        after[(size_t)g] = carry;
        u32 m = NAMES_NONE;
        const u64 t_end = (g + 1) * NAMES_GROUP_TILES < nt ? (g + 1) * NAMES_GROUP_TILES : nt;
        for (u64 t = t_end; t-- > g * NAMES_GROUP_TILES;) {
            m = first[(size_t)t] < m ? first[(size_t)t] : m;
            local[(size_t)t] = m;
        }
        carry = m < carry ? m : carry;
    }
    std::vector<u64> next((size_t)n + 1);            // the naive answer for every start
    next[(size_t)n] = n;
    for (u64 i = n; i-- > 0;)
        next[(size_t)i] = names_ends_here(text[(size_t)i], first_word) ? i : next[(size_t)i + 1];
    const auto ask = [&](u64 from) {
        const u64 got = names_end_from(
            from, n, [&](u64 c) { return mask.at((size_t)c); }, [&](u64 t) { return local.at((size_t)t); },
            [&](u64 g) { return after.at((size_t)g); });
        const u64 want = from >= n ? n : next[(size_t)from];
        CHECK(got == want, "%s: from %llu: got %llu want %llu", what, (unsigned long long)from, (unsigned long long)got,
              (unsigned long long)want);
    };
    for (u64 t = 0; t <= nt; t++)                     // around every tile boundary
        for (u64 d = 0; d < 2 * TEXT_CHUNK + 2; d++) {
            const u64 edge = t * TEXT_TILE_BYTES;
            if (edge + d <= n + 1)
                ask(edge + d);
            if (edge >= d + 1)
                ask(edge - d - 1);
        }
    for (int i = 0; i < 100000 && n; i++)
        ask(rng() % n);
    ask(n);
    ask(n + 5);
}

int main()
{
    const u64 G = TEXT_TILE_BYTES;
    // dense: a FASTQ-like text, line ends every few dozen bytes, blanks in between
    for (u64 n : {(u64)1, (u64)31, (u64)32, (u64)33, G - 1, G, G + 1, 3 * G + 17}) {
        std::vector<unsigned char> t((size_t)n);
        for (auto &b : t) {
            const u64 r = rng() % 40;
            b = r == 0 ? '\n' : r == 1 ? ' ' : r == 2 ? '\t' : r == 3 ? '\r' : (unsigned char)('A' + r % 26);
        }
        check_text(t, false, "dense");
        check_text(t, true, "dense, first word");
    }
    // sparse: whole tiles, and whole groups of tiles, without an end; an end as the last byte of a tile and the first of the next
    {
        const u64 n = (2 * NAMES_GROUP_TILES + 5) * G + 123;
        std::vector<unsigned char> t((size_t)n, 'x');
        check_text(t, false, "no end at all");
        for (u64 at : {(u64)7, G - 1, G, 5 * G + 9, NAMES_GROUP_TILES * G - 1, NAMES_GROUP_TILES * G, (NAMES_GROUP_TILES + 3) * G + 1,
                       2 * NAMES_GROUP_TILES * G + 4 * G, n - 1})
            t[(size_t)at] = '\n';
        t[(size_t)(3 * G)] = ' ';
        check_text(t, false, "sparse");
        check_text(t, true, "sparse, first word");
    }
    // the terminator: a '\r' directly before the '\n' that ends the line belongs to it
    {
        const unsigned char s[] = "@ab\r\n@\r\n@c\n@d\r";
        const u64 n = sizeof s - 1;
        const auto byte = [&](u64 i) { return (u32)s[i]; };
        CHECK(names_strip(1, 4, n, byte) == 3, "CRLF");
        CHECK(names_strip(6, 7, n, byte) == 6, "an empty name of a CRLF file");
        CHECK(names_strip(9, 10, n, byte) == 10, "LF");
        CHECK(names_strip(12, n, n, byte) == n, "a last line without '\\n': its '\\r' stays");
        CHECK(names_strip(7, 7, n, byte) == 7, "an empty span");
    }
    CHECK(names_alloc_bytes(0) == 32 && names_alloc_bytes(1) == 32 && names_alloc_bytes(16) == 32 && names_alloc_bytes(17) == 48, "alloc");
    CHECK(names_chunks(0) == 0 && names_chunks(1) == 1 && names_chunks(32) == 1 && names_chunks(33) == 2, "chunks");
    CHECK(names_groups(1) == 1 && names_groups(NAMES_GROUP_TILES) == 1 && names_groups(NAMES_GROUP_TILES + 1) == 2, "groups");
    CHECK(names_forbidden('\n') && names_forbidden('\r') && !names_forbidden(' ') && !names_forbidden(0), "forbidden");
    if (bad) {
        printf("%d checks failed\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
