// Host-side check of index_math.hpp (the arithmetic the kernels of the kmer-column index share with their driver): rev2 is
// an involution; ascending r is strcmp order of the decoded text under A < T < C < G; the range of a p-base prefix holds
// exactly the keys with that prefix; the prune depth and the enumeration of the concrete prefixes.  Built and run by
// tests/test_kmer_index.py with hipcc (host code only: no device is touched).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "index_math.hpp"

using namespace dnagpu;

static int bad = 0;
#define CHECK(cond, ...)                                                                                                          \
    do {                                                                                                                          \
        if (!(cond)) {                                                                                                            \
            printf(__VA_ARGS__);                                                                                                  \
            printf("  [%s:%d]\n", __FILE__, __LINE__);                                                                            \
            bad++;                                                                                                                \
        }                                                                                                                         \
    } while (0)

// text of a key with the codes renamed so that strcmp order is A < T < C < G: 'a' + code
static std::string rank_text(u64 key, int k)
{
    std::string s((size_t)k, 'a');
    for (int i = 0; i < k; i++)
        s[(size_t)i] = (char)('a' + ((key >> (2 * i)) & 3));
    return s;
}

static int iupac(char c)
{
    const char *codes = "ATCGUWSMKRYBDHVN";
    const int sets[] = {1, 2, 4, 8, 0, 3, 12, 5, 10, 9, 6, 14, 11, 7, 13, 15};
    const char *at = strchr(codes, c);
    return at ? sets[at - codes] : -1;
}

static FilterBits bits_of(const char *pattern)
{
    FilterBits fb;
    for (int q = 0; q < 4; q++)
        fb.sets[q] = 0xFFFFFFFFu;
    fb.k = (int)strlen(pattern);
    for (int i = 0; i < fb.k; i++)
        fb.sets[i >> 3] = (fb.sets[i >> 3] & ~(15u << ((i & 7) * 4))) | ((u32)iupac(pattern[i]) << ((i & 7) * 4));
    return fb;
}

int main()
{
    u64 s = 0x51ED270B;
    // rev2: an involution that moves field i to field 31 - i and keeps each field
    for (int i = 0; i < 100000; i++) {
        s = splitmix64(s);
        const u64 x = i == 0 ? 0 : i == 1 ? ~(u64)0 : s;
        CHECK(rev2(rev2(x)) == x, "rev2(rev2(%llx)) differs", (unsigned long long)x);
        if (i < 1000) {
            const u64 y = rev2(x);
            for (int f = 0; f < 32; f++)
                CHECK(((y >> (2 * (31 - f))) & 3) == ((x >> (2 * f)) & 3), "rev2(%llx): field %d", (unsigned long long)x, f);
        }
    }
    // order: ascending r == strcmp order of the text; equal r == equal keys; key_of_r inverts r_of_key; stray bits dropped
    const int ks[] = {1, 5, 31, 32};
    for (int k : ks) {
        const u64 mask = kmer_mask(k);
        std::vector<u64> keys;
        for (int i = 0; i < 4000; i++) {
            s = splitmix64(s);
            u64 x = s & mask;
            if (i % 3 == 1 && !keys.empty())          // near-copies: share a long prefix with an earlier key
                x = (keys[(size_t)(s >> 40) % keys.size()] & kmer_mask((int)(s % (u64)k))) | (x & ~kmer_mask((int)(s % (u64)k)));
            keys.push_back(x & mask);
        }
        keys.push_back(0);
        keys.push_back(mask);
        for (size_t i = 0; i + 1 < keys.size(); i++) {
            const u64 a = keys[i], b = keys[i + 1];
            const u64 ra = index_r_of_key(a, k), rb = index_r_of_key(b, k);
            const int c = rank_text(a, k).compare(rank_text(b, k));
            CHECK((ra < rb) == (c < 0) && (ra == rb) == (c == 0), "k=%d: order of %llx and %llx", k, (unsigned long long)a,
                  (unsigned long long)b);
            CHECK((ra == rb) == (a == b), "k=%d: equal r, different keys", k);
            CHECK(index_key_of_r(ra, k) == a, "k=%d: key_of_r(r_of_key(%llx))", k, (unsigned long long)a);
            CHECK(k == 32 || (ra >> (2 * k)) == 0, "k=%d: r leaves the key bits", k);
            CHECK(k == 32 || index_r_of_key(a | ((u64)1 << (2 * k)), k) == ra, "k=%d: bits above 2k change r", k);
        }
        // the range of a p-base prefix holds exactly the keys with that prefix
        std::vector<int> ps = {0, 1, k - 1, k};
        for (int p : ps) {
            if (p < 0)
                continue;
            for (int t = 0; t < 50; t++) {
                const u64 owner = keys[(size_t)t * 7 % keys.size()];
                const u64 pr = p == 0 ? 0 : index_r_of_key(owner, k) >> (2 * (k - p));
                u64 lo, hi;
                index_prefix_range(pr, p, k, &lo, &hi);
                CHECK(lo <= hi, "k=%d p=%d: empty range", k, p);
                if (p == 0)
                    CHECK(lo == 0 && hi == mask, "k=%d p=0: the range is not the whole index", k);
                for (u64 key : keys) {
                    const u64 r = index_r_of_key(key, k);
                    const bool shares = p == 0 || ((key ^ owner) & kmer_mask(p)) == 0;
                    CHECK((r >= lo && r <= hi) == shares, "k=%d p=%d: key %llx and the range of %llx", k, p,
                          (unsigned long long)key, (unsigned long long)owner);
                }
            }
        }
    }
    // prune depth
    struct Case {
        const char *pattern;
        int p;
        u32 ranges;
    };
    const Case cases[] = {
        {"ATCGC", 5, 1},                                    // `=`: p = k, one range
        {"MRKYN", 5, 64},                                   // 2 * 2 * 2 * 2 * 4
        {"NNNNNNNNNNWSNNNNNNNNN", 5, 1024},                 // opens with N's: 4^5 and no further
        {"NNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN", 5, 1024},
        {"ACUGT", 5, 0},                                    // 'U': nothing can match, no range
        {"ACTGNNNNNNN", 9, 1024},                           // `^@ 'ACTG'` at k = 11: p = l + 5
        {"AC", 2, 1},
        {"WSWSWSWSWSWS", 10, 1024},                         // 2^10
        {"BBBBBBBB", 6, 729},                               // 3^6 = 729, 3^7 = 2187
    };
    for (const Case &c : cases) {
        const FilterBits fb = bits_of(c.pattern);
        u32 R = 77;
        const int p = index_prune_depth(fb, &R);
        CHECK(p == c.p && R == c.ranges, "prune depth of %s: p = %d, %u ranges (expected %d, %u)", c.pattern, p, R, c.p, c.ranges);
        // the enumeration: strictly ascending, every prefix inside the sets, R of them
        u64 last = 0;
        for (u32 j = 0; j < R; j++) {
            const u64 pr = index_prefix_at(fb, p, j);
            CHECK(j == 0 || pr > last, "%s: prefix %u does not ascend", c.pattern, j);
            last = pr;
            for (int i = 0; i < p; i++) {
                const u32 code = (u32)(pr >> (2 * (p - 1 - i))) & 3;
                CHECK(index_set_at(fb, i) & (1u << code), "%s: prefix %u leaves the set of position %d", c.pattern, j, i);
            }
        }
        bool rest_any = true;
        for (int i = p; i < fb.k; i++)
            rest_any = rest_any && iupac(c.pattern[i]) == 15;
        CHECK(index_rest_is_any(fb, p) == rest_any, "%s: rest_is_any", c.pattern);
    }
    if (bad) {
        printf("%d failures\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
