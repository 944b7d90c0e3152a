// Host-side check of strand_math.hpp (the arithmetic the strand kernels and the canonical add share): rc against a per-base
// loop, the one-reversal canonical test against the comparison of the two texts, the palindromes, the 32-base corner keys,
// word_revcomp, and the source words of dna_revcomp_kernel against a per-base model that also watches which words are read.
// Built and run by tests/test_strand.py with hipcc (host code only: no device is touched).
#include <cstdio>
#include <string>
#include <vector>
#include "strand_math.hpp"

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

static u64 rc_loop(u64 key, int k)
{
    u64 out = 0;
    for (int i = 0; i < k; i++)
        out |= (((key >> (2 * (k - 1 - i))) & 3) ^ 1) << (2 * i);
    return out;
}

// text with the codes renamed so that strcmp order is A < T < C < G
static std::string rank_text(u64 key, int k)
{
    std::string s((size_t)k, 'a');
    for (int i = 0; i < k; i++)
        s[(size_t)i] = (char)('a' + ((key >> (2 * i)) & 3));
    return s;
}

static void check_key(u64 x, int k)
{
    const u64 mask = kmer_mask(k), key = x & mask, M = STRAND_COMPLEMENT & mask;
    const u64 rc = rc_loop(key, k);
    CHECK(kmer_revcomp(x, k) == rc, "k=%d: rc(%llx)", k, (unsigned long long)x);
    CHECK(kmer_revcomp(rc, k) == key, "k=%d: rc(rc(%llx))", k, (unsigned long long)x);
    // the identity the canonical test rests on: the index rank of rc(key) is key ^ M
    CHECK(index_r_of_key(rc, k) == (key ^ M), "k=%d: rank of rc(%llx)", k, (unsigned long long)x);
    const int c = rank_text(key, k).compare(rank_text(rc, k));
    CHECK(kmer_is_canonical(x, k) == (c <= 0), "k=%d: is_canonical(%llx)", k, (unsigned long long)x);
    CHECK((index_r_of_key(key, k) <= (key ^ M)) == (c <= 0), "k=%d: r <= key ^ M for %llx", k, (unsigned long long)x);
    bool flipped = false;
    const u64 can = kmer_canonical(x, k, &flipped);
    CHECK(can == (c <= 0 ? key : rc), "k=%d: canonical(%llx)", k, (unsigned long long)x);
    CHECK(flipped == (can != key), "k=%d: flipped(%llx)", k, (unsigned long long)x);
    CHECK(kmer_canonical(x, k) == can && kmer_canonical(rc, k) == can, "k=%d: canonical of either strand of %llx", k,
          (unsigned long long)x);
    CHECK(kmer_is_canonical(can, k), "k=%d: canonical(%llx) is not canonical", k, (unsigned long long)x);
}

// bases [first, first + count) of words reverse-complemented by the kernel's per-word arithmetic; touched[w] = word w read
static std::vector<u64> revcomp_words(const std::vector<u64> &words, u64 first, u64 count, std::vector<int> &touched)
{
    std::vector<u64> out((size_t)((count + 31) / 32));
    for (u64 j = 0; j < out.size(); j++) {
        const RevcompSource s = revcomp_source(first, count, j);
        touched[(size_t)s.word] = 1;
        const u64 lo = words[(size_t)s.word];
        u64 hi = 0;
        if (s.two_words) {
            touched[(size_t)s.word + 1] = 1;
            hi = words[(size_t)s.word + 1];
        }
        const u64 w = (lo >> s.shift) | ((hi << 1) << (63u - s.shift));      // funnel of kmer_device.hpp
        out[(size_t)j] = revcomp_finish(w, s.nb);
    }
    return out;
}

int main()
{
    u64 s = 0x57A4D;
    const int ks[] = {1, 2, 5, 16, 31, 32};
    for (int k : ks) {
        const u64 mask = kmer_mask(k);
        for (int i = 0; i < 20000; i++) {
            s = splitmix64(s);
            check_key(s, k);                            // (bits above 2k set: they must not matter)
            check_key(s & mask, k);
        }
        check_key(0, k);
        check_key(mask, k);
        check_key(STRAND_COMPLEMENT & mask, k);
        check_key(~STRAND_COMPLEMENT & mask, k);
    }
    // palindromes: key == rc(key) only at even k; 4^(k/2) of them
    for (int k = 1; k <= 6; k++) {
        u64 n = 0, canon = 0;
        for (u64 key = 0; key <= kmer_mask(k); key++) {
            check_key(key, k);
            n += kmer_revcomp(key, k) == key;
            canon += kmer_is_canonical(key, k);
        }
        const u64 all = kmer_mask(k) + 1, want = (k & 1) ? 0 : (u64)1 << k;
        CHECK(n == want, "k=%d: %llu palindromes, expected %llu", k, (unsigned long long)n, (unsigned long long)want);
        CHECK(canon == (all + want) / 2, "k=%d: %llu canonical keys", k, (unsigned long long)canon);
    }
    {
        u64 n4 = 0, n5 = 0;
        for (u64 key = 0; key < 256; key++)
            n4 += kmer_revcomp(key, 4) == key;
        for (u64 key = 0; key < 1024; key++)
            n5 += kmer_revcomp(key, 5) == key;
        CHECK(n4 == 16 && n5 == 0, "palindromes at k = 4, 5: %llu, %llu", (unsigned long long)n4, (unsigned long long)n5);
    }
    // the 32-base corners: G x 32 folds into C x 32, T x 32 into A x 32 (key 0), which stays
    const u64 A32 = 0, T32 = STRAND_COMPLEMENT, C32 = ~STRAND_COMPLEMENT, G32 = ~(u64)0;
    CHECK(kmer_revcomp(G32, 32) == C32 && kmer_canonical(G32, 32) == C32 && !kmer_is_canonical(G32, 32), "G x 32");
    CHECK(kmer_canonical(C32, 32) == C32 && kmer_is_canonical(C32, 32), "C x 32");
    CHECK(kmer_revcomp(T32, 32) == A32 && kmer_canonical(T32, 32) == A32 && !kmer_is_canonical(T32, 32), "T x 32");
    CHECK(kmer_canonical(A32, 32) == A32 && kmer_is_canonical(A32, 32), "A x 32");
    // the worked example: ATCGA / TCGAT -> ATCGA, CGATC / GATCG -> CGATC (A=0 T=1 C=2 G=3, base 0 in the low field)
    auto enc = [](const char *t) {
        u64 key = 0;
        for (int i = 0; t[i]; i++)
            key |= (u64)(t[i] == 'A' ? 0 : t[i] == 'T' ? 1 : t[i] == 'C' ? 2 : 3) << (2 * i);
        return key;
    };
    CHECK(kmer_revcomp(enc("ATCGA"), 5) == enc("TCGAT") && kmer_canonical(enc("TCGAT"), 5) == enc("ATCGA"), "ATCGA");
    CHECK(kmer_revcomp(enc("CGATC"), 5) == enc("GATCG") && kmer_canonical(enc("GATCG"), 5) == enc("CGATC"), "CGATC");
    CHECK(kmer_canonical(enc("CGACG"), 5) == enc("CGACG") && kmer_canonical(enc("TCGAC"), 5) == enc("TCGAC"), "CGACG, TCGAC");
    // word_revcomp
    for (int i = 0; i < 1000; i++) {
        s = splitmix64(s);
        CHECK(word_revcomp(s) == rc_loop(s, 32) && word_revcomp(word_revcomp(s)) == s, "word_revcomp(%llx)", (unsigned long long)s);
    }
    // the windows of dna_revcomp_kernel: every base, the zero tail, and no word outside [first / 32, ceil((first + count) / 32))
    std::vector<u64> words(140);
    for (u64 &w : words)
        w = s = splitmix64(s);
    const u64 n_bases = 32 * words.size();
    auto base = [&](u64 i) { return (words[(size_t)(i >> 5)] >> (2 * (i & 31))) & 3; };
    const u64 firsts[] = {0, 1, 5, 31, 32, 33, 63, 64, 100};
    const u64 counts[] = {1, 2, 31, 32, 33, 63, 64, 65, 70, 95, 96, 97, 1000, 4095, 4096, 4097};
    for (u64 first : firsts)
        for (u64 count : counts) {
            if (first + count > n_bases)
                continue;
            std::vector<int> touched(words.size(), 0);
            const std::vector<u64> out = revcomp_words(words, first, count, touched);
            for (u64 j = 0; j < 32 * out.size(); j++) {
                const u64 got = (out[(size_t)(j >> 5)] >> (2 * (j & 31))) & 3;
                const u64 want = j < count ? base(first + count - 1 - j) ^ 1 : 0;
                CHECK(got == want, "revcomp first=%llu count=%llu: base %llu", (unsigned long long)first,
                      (unsigned long long)count, (unsigned long long)j);
            }
            for (u64 w = 0; w < words.size(); w++)
                CHECK(!touched[(size_t)w] || (w >= first / 32 && w < (first + count + 31) / 32),
                      "revcomp first=%llu count=%llu reads word %llu", (unsigned long long)first, (unsigned long long)count,
                      (unsigned long long)w);
        }
    if (bad) {
        printf("%d failures\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
