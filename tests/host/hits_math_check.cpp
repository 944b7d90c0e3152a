// Host-side check of hits_math.hpp (the index arithmetic the kernels of dnagpu_table_hits and their host driver share): C(r),
// the hits among a window's rows before r, read from the three levels the sweep leaves (tile bases, word prefixes inside a
// tile, mask words) against a naive prefix count over a random bit per stream position -- for every window offset 0..63,
// window lengths around 32, 64 and the 8192-row tile, and k in 1, 31, 32 (what decides which rows exist, and so the last
// partial word).  Built and run by tests/test_table_hits.py with hipcc (host code only: no device is touched).
#include <cstdio>
#include <vector>
#include "hits_math.hpp"

using namespace dnagpu;

static int bad = 0;
#define CHECK(cond, ...)                                                                                                          \
    do {                                                                                                                          \
        if (!(cond)) {                                                                                                            \
            if (bad < 20) {                                                                                                       \
                printf(__VA_ARGS__);                                                                                              \
                printf("  [%s:%d]\n", __FILE__, __LINE__);                                                                        \
            }                                                                                                                     \
            bad++;                                                                                                                \
        }                                                                                                                         \
    } while (0)

static u64 rng_state = 0x243F6A8885A308D3ull;
static u64 rng() { return rng_state = splitmix64(rng_state); }

static void check_window(u64 a0, u64 n, int k)
{
    // one random bit per stream position: "the k-mer at p is in the set"
    std::vector<unsigned char> hb((size_t)(a0 + n + 64));
    for (auto &b : hb)
        b = (unsigned char)(rng() & 1);
    const u64 rows = hits_stream_rows(n, k), n_mw = hits_mask_words(n), tiles = hits_tiles(n);
    CHECK(n_mw * HITS_ROWS_PER_WORD > n, "no word for C(n): a0=%llu n=%llu", (unsigned long long)a0, (unsigned long long)n);
    CHECK(tiles * HITS_TILE_WORDS >= n_mw && (tiles - 1) * HITS_TILE_WORDS < n_mw, "tiles: n=%llu", (unsigned long long)n);

    // what the sweep leaves: every thread its mask word, the prefix inside its tile, the tile's total
    std::vector<u32> mask((size_t)n_mw), word_pre((size_t)n_mw), tile_base((size_t)tiles);
    u64 valid_rows = 0;
    for (u64 w = 0; w < n_mw; w++) {
        const HitsWordAt at = hits_word_at(a0, w);
        const u32 valid = hits_word_valid(rows, w);
        valid_rows += (u64)hits_popc(valid);
        u32 m = 0;
        for (u32 j = 0; j < HITS_ROWS_PER_WORD; j++) {
            const u64 p = at.stream_word * 32 + at.fo + j;
            CHECK(p == a0 + w * 32 + j, "word_at: a0=%llu w=%llu", (unsigned long long)a0, (unsigned long long)w);
            if ((valid >> j) & 1u)
                m |= (u32)hb[(size_t)p] << j;
        }
        mask[(size_t)w] = m;
    }
    CHECK(valid_rows == rows, "valid rows %llu != %llu (n=%llu k=%d)", (unsigned long long)valid_rows, (unsigned long long)rows,
          (unsigned long long)n, k);
    u32 run = 0;
    for (u64 t = 0; t < tiles; t++) {
        tile_base[(size_t)t] = run;
        u32 in_tile = 0;
        for (u64 w = t * HITS_TILE_WORDS; w < (t + 1) * HITS_TILE_WORDS && w < n_mw; w++) {
            word_pre[(size_t)w] = in_tile;
            in_tile += hits_popc(mask[(size_t)w]);
        }
        run += in_tile;
    }

    // C(r) for every r a sequence can ask for, against the naive count
    u32 naive = 0;
    for (u64 r = 0; r <= n; r++) {
        const HitsAt at = hits_at(r);
        CHECK(at.word < n_mw && at.tile < tiles, "C(%llu) reads outside: n=%llu", (unsigned long long)r, (unsigned long long)n);
        if (at.word >= n_mw || at.tile >= tiles)
            return;
        const u32 c = hits_before(mask.data(), word_pre.data(), tile_base.data(), r);
        CHECK(c == naive, "C(%llu) = %u, expected %u (a0=%llu n=%llu k=%d)", (unsigned long long)r, c, naive, (unsigned long long)a0,
              (unsigned long long)n, k);
        if (r < rows)
            naive += hb[(size_t)(a0 + r)];
    }
    // a sequence's hits are a difference of two of them
    for (int i = 0; i < 8 && n > 0; i++) {
        const u64 s0 = rng() % n, len = rng() % (n - s0 + 1), sr = hits_seq_rows(len, k);
        u32 want = 0;
        for (u64 r = s0; r < s0 + sr; r++)
            want += hb[(size_t)(a0 + r)];
        const u32 got = sr ? hits_before(mask.data(), word_pre.data(), tile_base.data(), s0 + sr) -
                                 hits_before(mask.data(), word_pre.data(), tile_base.data(), s0)
                           : 0u;
        CHECK(got == want, "sequence [%llu, +%llu): %u hits, expected %u", (unsigned long long)s0, (unsigned long long)len, got, want);
    }
}

int main()
{
    const u64 lengths[] = {0, 1, 30, 31, 32, 33, 34, 62, 63, 64, 65, 66, 95, 96, 97, 8160, 8191, 8192, 8193, 8222, 8223, 8224, 8225,
                           16383, 16384, 16385, 20000};
    const int ks[] = {1, 31, 32};
    for (u64 a0 = 0; a0 < 64; a0++)
        for (u64 n : lengths)
            for (int k : ks)
                check_window(a0, n, k);
    check_window(12345, 70000, 21);

    // select's predicate at the corners of its two products
    CHECK(hits_selected(0, 0, 0, 0, 0, 1), "depletion keeps a sequence of no rows");
    CHECK(hits_selected(0, 0, 0, ~(u64)0, 1, 1), "0 >= 1/1 * 0");
    CHECK(!hits_selected(10, 4, 0, ~(u64)0, 1, 2) && hits_selected(10, 5, 0, ~(u64)0, 1, 2), "half");
    CHECK(!hits_selected(10, 10, 0, ~(u64)0, 3, 2) && hits_selected(0, 0, 0, ~(u64)0, 3, 2), "3/2 leaves only rows == 0");
    CHECK(hits_selected(0xFFFFFFFFu, 0xFFFFFFFFu, 1, ~(u64)0, 0xFFFFFFFFull, 0xFFFFFFFFull), "the largest products are exact");
    CHECK(!hits_selected(0xFFFFFFFFu, 0xFFFFFFFEu, 1, ~(u64)0, 0xFFFFFFFFull, 0xFFFFFFFFull), "one short of all");

    if (bad) {
        printf("%d checks failed\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
