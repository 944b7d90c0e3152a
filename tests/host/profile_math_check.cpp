// profile_math_check.cpp -- profile_math.hpp on the host against naive loops (tests/test_table_profile.py builds it plainly and
// with AddressSanitizer + UndefinedBehaviorSanitizer): the width, the rows of a sequence, class and item count around both
// limits, item -> (sequence, tile, row range) covering every row exactly once, and for every k in 1..6 and every key the
// reverse complement, the canonical test, the fold's target column and the fold as a gather.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "profile_math.hpp"

using namespace dnagpu;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

// base i of a key, and a key from its bases
static u32 base_of(u32 key, int i) { return (key >> (2 * i)) & 3u; }

static u32 naive_rc(u32 key, int k)
{
    u32 out = 0;
    for (int i = 0; i < k; i++)
        out |= (base_of(key, k - 1 - i) ^ 1u) << (2 * i);
    return out;
}

// text order under A < T < C < G: compare base by base from base 0
static int naive_cmp(u32 a, u32 b, int k)
{
    for (int i = 0; i < k; i++)
        if (base_of(a, i) != base_of(b, i))
            return base_of(a, i) < base_of(b, i) ? -1 : 1;
    return 0;
}

int main()
{
    // width
    u64 w = 4;
    for (int k = 1; k <= 6; k++, w *= 4)
        CHECK(profile_width(k) == w);
    const int none[] = {-1, 0, 7, 8, 31, 32, 33, 1 << 30};
    for (int k : none)
        CHECK(profile_width(k) == 0);

    // rows of a sequence
    for (int k = 1; k <= 6; k++)
        for (u64 len = 0; len < 80; len++) {
            u64 rows = 0;
            for (u64 p = 0; p + k <= len; p++)
                rows++;
            CHECK(profile_seq_rows(len, k) == rows);
        }
    CHECK(profile_seq_rows(0xFFFFFFFFull, 1) == 0xFFFFFFFFull && profile_seq_rows(0xFFFFFFFFull, 6) == 0xFFFFFFFAull);

    // class and items around both limits; the items of a sequence cover each of its rows exactly once
    const u64 W = PROFILE_WAVE_ROWS, T = PROFILE_TILE_ROWS;
    CHECK(W < T && T % 32 == 0);
    const u64 sizes[] = {0, 1, 2, W - 1, W, W + 1, W + 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 5 * T + 17, 0xFFFFFFFFull};
    for (u64 rows : sizes) {
        CHECK(profile_is_tiled(rows) == (rows > W));
        u64 naive_items = 0;
        if (rows > W)
            for (u64 r = 0; r < rows; r += T)
                naive_items++;
        CHECK(profile_items(rows) == naive_items);
        CHECK(profile_is_shared(rows) == (naive_items > 1));
        if (rows > 10 * T)
            continue;
        std::vector<int> seen((size_t)rows, 0);
        u64 end = 0;
        for (u64 t = 0; t < profile_items(rows); t++) {
            u64 r0, r1;
            profile_item_rows(rows, t, &r0, &r1);
            CHECK(r0 == end && r1 > r0 && r1 - r0 <= T && r1 <= rows);
            for (u64 r = r0; r < r1; r++)
                seen[(size_t)r]++;
            end = r1;
        }
        if (rows > W) {
            CHECK(end == rows);
            for (u64 r = 0; r < rows; r++)
                CHECK(seen[(size_t)r] == 1);
        }
    }
    {
        u64 r0, r1;
        profile_item_rows(0xFFFFFFFFull, profile_items(0xFFFFFFFFull) - 1, &r0, &r1);
        CHECK(r1 == 0xFFFFFFFFull && r0 < r1 && r1 - r0 <= T);
    }

    // item -> sequence over a table of mixed classes, empty sequences and runs of them, at the ends too
    const u64 seq_rows[] = {0, 0, W + 1, 0, 3, 3 * T, W, 0, 0, 2 * T + 1, T, 0, 0};
    const u64 n = sizeof seq_rows / sizeof seq_rows[0];
    std::vector<u32> off(n);
    std::vector<u64> owner, tile;                          // the naive list
    for (u64 i = 0; i < n; i++) {
        off[i] = (u32)owner.size();
        for (u64 t = 0; t < profile_items(seq_rows[i]); t++) {
            owner.push_back(i);
            tile.push_back(t);
        }
    }
    CHECK(owner.size() == 1 + 3 + 3 + 1);
    for (u32 item = 0; item < owner.size(); item++) {
        const u64 i = profile_item_seq(off.data(), n, item);
        CHECK(i == owner[item] && item - off[i] == tile[item]);
    }
    {
        const u32 one[1] = {0};
        CHECK(profile_item_seq(one, 1, 0) == 0 && profile_item_seq(one, 1, 5) == 0);
    }

    // strand arithmetic of every column
    for (int k = 1; k <= 6; k++) {
        const u32 width = (u32)profile_width(k);
        std::vector<u32> hits(width, 0);
        u32 palindromes = 0;
        for (u32 c = 0; c < width; c++) {
            const u32 rc = naive_rc(c, k);
            CHECK(profile_rc(c, k) == rc && profile_rc(rc, k) == c);
            const bool canon = naive_cmp(c, rc, k) <= 0;
            CHECK(profile_is_canonical(c, k) == canon);
            const u32 target = canon ? c : rc;
            CHECK(profile_fold_target(c, k) == target && profile_is_canonical(target, k));
            hits[target]++;
            palindromes += c == rc;
        }
        CHECK((k % 2 == 1) == (palindromes == 0));
        if (k == 2)
            CHECK(palindromes == 4);                       // AT, TA, CG, GC
        // the fold as a gather lands every forward column in exactly one canonical column
        for (u32 c = 0; c < width; c++) {
            u32 other;
            const int n_src = profile_fold_sources(c, k, &other);
            CHECK((u32)n_src == hits[c]);
            CHECK(other == naive_rc(c, k));
            if (n_src == 1)
                CHECK(other == c);
            if (n_src == 2)
                CHECK(other != c && !profile_is_canonical(other, k));
            // ... and the quad form, from the reversal of the quad's first column
            u32 other_q;
            const u32 c0 = c & ~3u;
            CHECK(profile_fold_sources_quad(c0, profile_rev_fields(c0, k), (int)(c & 3u), k, &other_q) == n_src);
            CHECK(other_q == other);
        }
    }
    printf("ok\n");
    return 0;
}
