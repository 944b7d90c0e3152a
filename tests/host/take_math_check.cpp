// Host-side check of take_math.hpp (the piece arithmetic the sweep of dnagpu_dna_gather / dnagpu_dna_take and its host driver
// share): for lists of segments -- empty, overlapping, repeated and flipped ones among them -- every output word is assembled
// from the header's pieces (take_segment_of + take_word) and compared with a naive base-by-base gather.  Segment lengths 0, 1,
// 31, 32, 33, 64, 65 at every source offset 0..63 and every output offset 0..31, random lists, segments that end exactly at
// the source's last base.  The source is a vector of exactly n_words words whose last word has ones behind its last base: the
// program fails if the header asks for a word at or beyond n_words, and no bit behind the last base may reach the output.
// Built and run by tests/test_dna_take.py with hipcc (host code only: no device is touched).
#include <cstdio>
#include <vector>
#include "take_math.hpp"

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

static u64 rng_state = 0x13198A2E03707344ull;
static u64 rng() { return rng_state = splitmix64(rng_state); }

struct Source {
    std::vector<u64> words;           // exactly ceil(n_bases / 32) of them
    u64 n_bases;
    unsigned base(u64 q) const { return (unsigned)(words[(size_t)(q >> 5)] >> (2 * (q & 31))) & 3u; }
};

static Source make_source(u64 n_bases)
{
    Source s;
    s.n_bases = n_bases;
    s.words.resize((size_t)((n_bases + 31) / 32));
    for (auto &w : s.words)
        w = rng();
    if (n_bases & 31)                 // ones behind the last base: a view's garbage (dnagpu_dna_wrap's rule)
        s.words.back() |= ~kmer_mask((int)(n_bases & 31));
    return s;
}

struct Seg {
    u64 first, len;
    uint8_t flip;
};

static void check_list(const Source &src, const std::vector<Seg> &segs, const char *what)
{
    const u64 n = segs.size();
    std::vector<u64> out_starts((size_t)n + 1), first((size_t)n);
    std::vector<uint8_t> flip((size_t)n);
    u64 total = 0;
    for (u64 i = 0; i < n; i++) {
        out_starts[(size_t)i] = total;
        first[(size_t)i] = segs[(size_t)i].first;
        flip[(size_t)i] = segs[(size_t)i].flip;
        CHECK(segs[(size_t)i].first <= src.n_bases && segs[(size_t)i].len <= src.n_bases - segs[(size_t)i].first, "%s: the list itself", what);
        total += segs[(size_t)i].len;
    }
    out_starts[(size_t)n] = total;

    // the naive gather, one base at a time
    std::vector<u64> want((size_t)take_words(total), 0);
    u64 p = 0;
    for (const Seg &g : segs)
        for (u64 j = 0; j < g.len; j++, p++) {
            const unsigned code = g.flip ? src.base(g.first + g.len - 1 - j) ^ 1u : src.base(g.first + j);
            want[(size_t)(p >> 5)] |= (u64)code << (2 * (p & 31));
        }

    const u64 n_words = src.words.size();
    bool outside = false;
    auto load = [&](u64 i) -> u64 {
        if (i >= n_words) {
            outside = true;
            return ~(u64)0;
        }
        return src.words[(size_t)i];
    };
    for (u64 w = 0; w < take_words(total); w++) {
        const u64 seg = take_segment_of(out_starts.data(), 0, n - 1, 32 * w);
        CHECK(out_starts[(size_t)seg] <= 32 * w && out_starts[(size_t)seg + 1] > 32 * w, "%s: word %llu: segment %llu does not hold its first base",
              what, (unsigned long long)w, (unsigned long long)seg);
        const u64 got = take_word(out_starts.data(), first.data(), flip.data(), total, seg, w, load);
        CHECK(got == want[(size_t)w], "%s: word %llu of %llu: %016llx, expected %016llx", what, (unsigned long long)w,
              (unsigned long long)take_words(total), (unsigned long long)got, (unsigned long long)want[(size_t)w]);
        // any earlier segment is as good a place to start the walk from
        const u64 got0 = take_word(out_starts.data(), first.data(), flip.data(), total, 0, w, load);
        CHECK(got0 == got, "%s: word %llu: the walk from segment 0 differs", what, (unsigned long long)w);
        // the sweep's LDS form: the lists from an earlier segment on, indices relative to it
        const u64 lo = seg - seg / 2, hi = seg + (n - 1 - seg) / 2;
        const u64 rel = take_segment_of(out_starts.data() + lo, 0, hi - lo, 32 * w);
        const u64 got1 = take_word(out_starts.data() + lo, first.data() + lo, flip.data() + lo, total, rel, w, load);
        CHECK(rel == seg - lo && got1 == got, "%s: word %llu: the lists from segment %llu on differ", what, (unsigned long long)w,
              (unsigned long long)lo);
    }
    CHECK(!outside, "%s: a word at or beyond n_words was asked for", what);
}

int main()
{
    const u64 lengths[] = {0, 1, 31, 32, 33, 64, 65};

    // every source offset x every output offset x every length, forward and flipped; the filler puts the probe at output
    // base d and is itself a segment (empty when d == 0), and a second probe behind it ends at a third alignment
    {
        const Source src = make_source(64 + 65 + 3);
        for (u64 s = 0; s < 64; s++)
            for (u64 d = 0; d < 32; d++)
                for (u64 len : lengths)
                    for (int f = 0; f < 2; f++) {
                        std::vector<Seg> segs = {{(s * 7 + d) % 32, d, (uint8_t)(f ^ 1)}, {s, len, (uint8_t)f}, {s + len > 40 ? s : s + 3, 40 - d, (uint8_t)f}};
                        check_list(src, segs, "alignment grid");
                    }
    }
    // segments that end exactly at the last base of a source whose last word is partial or full; the whole source; twice
    for (u64 n_bases : {1ull, 31ull, 32ull, 33ull, 64ull, 65ull, 100ull, 127ull, 128ull, 129ull})
        for (int f = 0; f < 2; f++) {
            const Source src = make_source(n_bases);
            std::vector<Seg> segs;
            for (u64 len : lengths)
                if (len <= n_bases)
                    segs.push_back({n_bases - len, len, (uint8_t)f});
            segs.push_back({0, n_bases, (uint8_t)f});
            segs.push_back({0, n_bases, (uint8_t)(f ^ 1)});
            segs.push_back({n_bases, 0, 1});
            check_list(src, segs, "ends at the last base");
        }
    // random lists: empty runs at the start, in the middle and at the end; overlaps and repeats; about half flipped
    for (int round = 0; round < 300; round++) {
        const u64 n_bases = 1 + rng() % 700;
        const Source src = make_source(n_bases);
        std::vector<Seg> segs;
        const u64 n = 1 + rng() % 80;
        for (u64 i = 0; i < n; i++) {
            const u64 kind = rng() % 8;
            u64 len = kind < 2 ? 0 : kind < 4 ? lengths[rng() % 7] : kind < 6 ? rng() % 5 : rng() % (n_bases + 1);
            if (len > n_bases)
                len = n_bases;
            const u64 first = rng() % (n_bases - len + 1);
            segs.push_back({first, len, (uint8_t)(rng() & 1)});
            if (kind == 7)
                segs.push_back(segs.back());
        }
        if (round % 3 == 0)
            segs.insert(segs.begin(), 3, Seg{rng() % (n_bases + 1), 0, 1});
        if (round % 3 == 1)
            segs.insert(segs.end(), 4, Seg{n_bases, 0, 0});
        check_list(src, segs, "random list");
    }
    // many pieces per word: 1-base segments, every other one empty
    {
        const Source src = make_source(97);
        std::vector<Seg> segs;
        for (u64 i = 0; i < 500; i++) {
            segs.push_back({rng() % 97, 1, (uint8_t)(rng() & 1)});
            segs.push_back({rng() % 98, 0, (uint8_t)(rng() & 1)});
        }
        check_list(src, segs, "one-base segments");
    }
    // all empty: no output word at all
    {
        const Source src = make_source(40);
        check_list(src, {{0, 0, 0}, {40, 0, 1}, {17, 0, 0}}, "all empty");
    }
    // the total of the validation pass: 2^32 - 1 entries of any length cannot wrap it, and one oversize length passes the limit
    CHECK(take_len_clamped(5) == 5 && take_len_clamped(~(u64)0) == ((u64)1 << 32) && take_len_clamped((u64)1 << 32) == ((u64)1 << 32),
          "take_len_clamped");
    CHECK(take_tiles(0) == 0 && take_tiles(1) == 1 && take_tiles(TAKE_TILE_WORDS) == 1 && take_tiles(TAKE_TILE_WORDS + 1) == 2, "take_tiles");

    if (bad) {
        printf("%d checks failed\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
