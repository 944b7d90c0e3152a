// seqeq_math_check.cpp -- seqeq_math.hpp on the host against base-by-base restatements (tests/test_seq_equal.py builds it
// plainly and with AddressSanitizer + UndefinedBehaviorSanitizer): the realigned word at every start alignment and length,
// read from a heap buffer of exactly n_words words; the fingerprint's independence of alignment, neighbours and junk behind
// the last base; a long sequence's fingerprint as the sum over its items; the item arithmetic against a naive loop.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "seqeq_math.hpp"

using namespace dnagpu;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

typedef std::vector<unsigned char> Bases;

static u64 rng_state = 0x5E9E9;
static u64 rnd() { return rng_state = splitmix64(rng_state); }

static Bases random_bases(u64 n)
{
    Bases b((size_t)n);
    for (u64 i = 0; i < n; i++)
        b[(size_t)i] = (unsigned char)(rnd() >> 37 & 3);
    return b;
}

// a stream of exactly ceil(n / 32) heap words: a read of word n_words is out of bounds for AddressSanitizer.  junk: the bits
// behind the last base are ones instead of zeros.
struct Stream {
    std::unique_ptr<u64[]> words;
    u64 n_words;
};
static Stream pack(const Bases &b, bool junk)
{
    Stream s;
    s.n_words = (b.size() + 31) / 32;
    s.words.reset(new u64[(size_t)s.n_words ? (size_t)s.n_words : 1]);
    for (u64 w = 0; w < s.n_words; w++)
        s.words[(size_t)w] = 0;
    for (u64 i = 0; i < b.size(); i++)
        s.words[(size_t)(i / 32)] |= (u64)b[(size_t)i] << (2 * (i % 32));
    if (junk && b.size() % 32)
        s.words[(size_t)(s.n_words - 1)] |= ~(u64)0 << (2 * (b.size() % 32));
    return s;
}

// word j of the sequence of len bases at base `start` of b, base by base
static u64 naive_word(const Bases &b, u64 start, u64 len, u64 j)
{
    u64 v = 0;
    for (u64 i = 0; i < 32 && 32 * j + i < len; i++)
        v |= (u64)b[(size_t)(start + 32 * j + i)] << (2 * i);
    return v;
}

static u64 naive_fp(const Bases &content)
{
    u64 fp = seqeq_fp_length(content.size());
    for (u64 j = 0; j < (content.size() + 31) / 32; j++)
        fp += seqeq_fp_word(naive_word(content, 0, content.size(), j), j);
    return fp;
}

int main()
{
    const u64 W = SEQEQ_WAVE_BASES, T = SEQEQ_TILE_BASES;
    CHECK(0 < W && W < T && T <= ((u64)1 << 20) && T % 32 == 0 && SEQEQ_TILE_WORDS * 32 == T);

    // ---- the item arithmetic against a naive loop; the items of a sequence cover each of its words exactly once
    const u64 sizes[] = {0, 1, 31, 32, 33, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T - 1, 3 * T, 3 * T + 1,
                         5 * T + 17, 0xFFFFFFFFull};
    for (u64 len : sizes) {
        CHECK(seqeq_words(len) == (len + 31) / 32 && seqeq_is_long(len) == (len > W));
        u64 naive_items = 0;
        if (len > W)
            for (u64 b = 0; b < len; b += T)
                naive_items++;
        CHECK(seqeq_items(len) == naive_items);
        if (len > 10 * T)
            continue;
        const u64 nw = seqeq_words(len);
        std::vector<int> seen((size_t)nw, 0);
        u64 end = 0;
        for (u64 t = 0; t < seqeq_items(len); t++) {
            u64 w0, w1;
            seqeq_item_words(len, t, &w0, &w1);
            CHECK(w0 == end && w1 > w0 && w1 - w0 <= SEQEQ_TILE_WORDS && w1 <= nw && w0 == t * (T / 32));
            for (u64 w = w0; w < w1; w++)
                seen[(size_t)w]++;
            end = w1;
        }
        if (len > W) {
            CHECK(end == nw);
            for (u64 w = 0; w < nw; w++)
                CHECK(seen[(size_t)w] == 1);
        }
    }
    {
        u64 w0, w1;
        seqeq_item_words(0xFFFFFFFFull, seqeq_items(0xFFFFFFFFull) - 1, &w0, &w1);
        CHECK(w1 == seqeq_words(0xFFFFFFFFull) && w0 < w1 && w1 - w0 <= SEQEQ_TILE_WORDS);
    }

    // ---- the realigned word: every start alignment, every length 0 .. 130 and the lengths around the class limit and
    // around 1, 2 and 3 items.  The sequence ends the stream (a tight buffer, clean or with junk behind the last base), or
    // a neighbour follows it.
    std::vector<u64> lengths;
    for (u64 len = 0; len <= 130; len++)
        lengths.push_back(len);
    for (u64 len : {W - 1, W, W + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T - 1, 3 * T, 3 * T + 1})
        lengths.push_back(len);
    for (u64 len : lengths)
        for (u64 align = 0; align < 32; align++)
            for (int form = 0; form < 3; form++) {         // tight and clean, tight with junk, a neighbour behind
                const u64 after = form == 2 ? 1 + (align * 13 + len) % 40 : 0;
                const Bases b = random_bases(align + len + after);
                const Stream s = pack(b, form == 1);
                for (u64 j = 0; j < seqeq_words(len); j++)
                    CHECK(seqeq_word(s.words.get(), s.n_words, align, len, j) == naive_word(b, align, len, j));
                Bases content(b.begin() + (size_t)align, b.begin() + (size_t)(align + len));
                CHECK(seqeq_fingerprint(s.words.get(), s.n_words, align, len) == naive_fp(content));
            }

    // ---- the fingerprint is a function of (length, bases) alone: one content at all 32 alignments, between different
    // neighbours, at the end of the stream with junk behind its last base
    for (u64 len : {(u64)0, (u64)1, (u64)31, (u64)32, (u64)33, (u64)64, (u64)100, (u64)130, W, W + 1}) {
        const Bases content = random_bases(len);
        const u64 want = naive_fp(content);
        for (u64 align = 0; align < 32; align++)
            for (int variant = 0; variant < 3; variant++) {
                Bases b = random_bases(align);             // a different filler in front every time
                b.insert(b.end(), content.begin(), content.end());
                if (variant == 0) {
                    const Bases tail = random_bases(1 + rnd() % 50);
                    b.insert(b.end(), tail.begin(), tail.end());
                }
                const Stream s = pack(b, variant == 2);
                CHECK(seqeq_fingerprint(s.words.get(), s.n_words, align, len) == want);
            }
    }

    // ---- a long sequence's items add up to the whole value, in any order
    for (u64 len : {W + 1, T, T + 1, 3 * T + 5}) {
        const u64 align = 1 + rnd() % 31;
        const Bases b = random_bases(align + len);
        const Stream s = pack(b, true);
        const u64 whole = seqeq_fingerprint(s.words.get(), s.n_words, align, len);
        u64 up = seqeq_fp_length(len), down = 0;
        for (u64 t = 0; t < seqeq_items(len); t++) {
            u64 w0, w1;
            seqeq_item_words(len, t, &w0, &w1);
            up += seqeq_fp_part(s.words.get(), s.n_words, align, len, w0, w1);
        }
        for (u64 t = seqeq_items(len); t-- > 0;) {
            u64 w0, w1;
            seqeq_item_words(len, t, &w0, &w1);
            down += seqeq_fp_part(s.words.get(), s.n_words, align, len, w0, w1);
        }
        CHECK(up == whole && down + seqeq_fp_length(len) == whole);
    }

    // ---- length is part of the identity (A is code 00: ACG, ACGA and ACGAA have the same words), and so is every base
    {
        const Bases acg = {0, 2, 3}, acga = {0, 2, 3, 0}, acgaa = {0, 2, 3, 0, 0};
        CHECK(naive_fp(acg) != naive_fp(acga) && naive_fp(acga) != naive_fp(acgaa) && naive_fp(acg) != naive_fp(acgaa));
        CHECK(naive_fp(Bases(32, 0)) != naive_fp(Bases(64, 0)) && naive_fp(Bases()) != naive_fp(Bases(1, 0)));
        Bases x = random_bases(100), y = x;
        y[99] ^= 1;
        CHECK(naive_fp(x) != naive_fp(y));
        Bases z = x;
        std::swap(z[0], z[64]);                            // the same word values cannot simply trade places
        if (z != x)
            CHECK(naive_fp(x) != naive_fp(z));
    }
    printf("ok\n");
    return 0;
}
