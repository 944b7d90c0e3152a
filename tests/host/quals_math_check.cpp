// Host-side check of quals_math.hpp (the byte arithmetic the kernels of the quality column and their host driver share): for
// lists of segments -- empty, overlapping, repeated and flipped ones among them -- every 16-byte chunk of the output is
// assembled from the header's pieces (take_segment_of + quals_chunk) and compared with a naive byte-by-byte gather, once
// with every piece formed byte by byte and once with whole pieces formed from aligned 32-bit words the way the copy kernel
// forms them, at every misalignment of the source.  Read lengths 1, 15, 16, 17, 31, 32, 33 and 50,000 random reads.  The
// source is a vector of exactly n bytes: the program fails if a byte or a word outside it is asked for.  Then the sixteen-byte
// helpers, the error word and the line length.  The trim: the lane functions joined as the kernels join them, for teams of 1,
// 2, 16 and 64 lanes (one tile and many), against cutadapt's two walks written as loops -- the worked example at every
// alignment, 50,000 random reads, the lengths around the limits of the paths, long reads.
// Built and run by tests/test_read_quals.py with hipcc (host code only).
#include <cstdio>
#include <cstring>
#include <vector>
#include "quals_math.hpp"
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

static u64 rng_state = 0x243F6A8885A308D3ull;
static u64 rng() { return rng_state = splitmix64(rng_state); }
static u64 formed_whole = 0;          // pieces formed from words

struct Seg {
    u64 first, len;
    uint8_t flip;
};

// base_mis: the misalignment (0 .. 3) the source's byte 0 is taken to have: the word loads of a whole piece are aligned to it
static void check_list(const std::vector<unsigned char> &src, u32 base_mis, const std::vector<Seg> &segs, const char *what)
{
    const u64 n = segs.size(), src_n = src.size();
    std::vector<u64> out_starts((size_t)n + 1), at((size_t)n);
    std::vector<uint8_t> flip((size_t)n);
    u64 total = 0;
    for (u64 i = 0; i < n; i++) {
        out_starts[(size_t)i] = total;
        at[(size_t)i] = segs[(size_t)i].first;
        flip[(size_t)i] = segs[(size_t)i].flip;
        CHECK(segs[(size_t)i].first <= src_n && segs[(size_t)i].len <= src_n - segs[(size_t)i].first, "%s: the list itself", what);
        total += segs[(size_t)i].len;
    }
    out_starts[(size_t)n] = total;
    std::vector<unsigned char> want((size_t)(quals_chunks(total) * QUALS_CHUNK), 0);
    u64 p = 0;
    for (const Seg &g : segs)
        for (u64 j = 0; j < g.len; j++, p++)
            want[(size_t)p] = g.flip ? src[(size_t)(g.first + g.len - 1 - j)] : src[(size_t)(g.first + j)];

    bool outside = false;
    auto load = [&](u64 i) -> u32 {
        if (i >= src_n) {
            outside = true;
            return 0xEE;
        }
        return src[(size_t)i];
    };
    auto never = [](u64, bool, QualsBytes *) { return false; };
    auto whole = [&](u64 a, bool f, QualsBytes *o) {           // (the copy kernel's: words aligned at the source's address)
        const u32 mis = (u32)((a + base_mis) & 3);
        if (a < mis || a - mis + (mis ? 20 : 16) > src_n)
            return false;
        u32 d[5] = {0, 0, 0, 0, 0};
        memcpy(d, src.data() + (a - mis), mis ? 20 : 16);
        const QualsBytes w = quals_from_words(d, mis);
        *o = f ? quals_reverse(w) : w;
        formed_whole++;
        return true;
    };
    for (u64 c = 0; c < quals_chunks(total); c++) {
        const u64 seg = take_segment_of(out_starts.data(), 0, n - 1, QUALS_CHUNK * c);
        const QualsBytes a = quals_chunk(out_starts.data(), at.data(), flip.data(), total, seg, c, load, never);
        const QualsBytes b = quals_chunk(out_starts.data(), at.data(), flip.data(), total, 0, c, load, whole);
        const u64 lo = seg - seg / 2, hi = seg + (n - 1 - seg) / 2;
        const u64 rel = take_segment_of(out_starts.data() + lo, 0, hi - lo, QUALS_CHUNK * c);
        const QualsBytes d = quals_chunk(out_starts.data() + lo, at.data() + lo, flip.data() + lo, total, rel, c, load, whole);
        for (u32 k = 0; k < QUALS_CHUNK; k++) {
            const u32 w = want[(size_t)(QUALS_CHUNK * c + k)];
            CHECK(quals_get(a, k) == w && quals_get(b, k) == w && quals_get(d, k) == w,
                  "%s: chunk %llu byte %u: %02x / %02x / %02x, expected %02x", what, (unsigned long long)c, k, quals_get(a, k),
                  quals_get(b, k), quals_get(d, k), w);
        }
    }
    CHECK(!outside, "%s: a byte outside the source was asked for", what);
}

static std::vector<unsigned char> make_source(u64 n)
{
    std::vector<unsigned char> s((size_t)n);
    for (auto &b : s)
        b = (unsigned char)(33 + rng() % 94);
    return s;
}

// ---- the trim: a team of L lanes over the sequence of n bases at column byte base, joined the way the kernels join their
// lanes (a scan of the lanes' sums, the first / last lane with a negative running sum, the maximum of the lanes' bests and
// the first / last lane that holds it), tile after tile with the carried state; against the two walks written as loops
struct Cut {
    i64 start, stop;
    u64 qsum, low;
};

static Cut naive_trim(const unsigned char *q, u64 n, const QualsTrimOpt &o)
{
    i64 start = 0, stop = (i64)n;
    if (o.cut_front) {
        i64 s = 0, best = 0;
        for (i64 i = 0; i < (i64)n; i++) {
            s += (i64)o.cut_front - (q[i] - 33);
            if (s < 0)
                break;
            if (s > best) {
                best = s;
                start = i + 1;
            }
        }
    }
    if (o.cut_tail) {
        i64 s = 0, best = 0;
        for (i64 i = (i64)n - 1; i >= 0; i--) {
            s += (i64)o.cut_tail - (q[i] - 33);
            if (s < 0)
                break;
            if (s > best) {
                best = s;
                stop = i;
            }
        }
    }
    if (start >= stop)
        start = stop = 0;
    Cut c = {start, stop, 0, 0};
    for (i64 i = start; i < stop; i++) {
        c.qsum += q[i] - 33;
        c.low += (u32)(q[i] - 33) < o.low_q;
    }
    return c;
}

static Cut team_trim(const std::vector<unsigned char> &col, u64 base, u64 n, const QualsTrimOpt &o, u32 L)
{
    const u64 c0 = base / QUALS_CHUNK, c_end = (base + n + QUALS_CHUNK - 1) / QUALS_CHUNK, tiles = (c_end - c0 + L - 1) / L;
    bool outside = false;
    auto load = [&](u64 c) {
        QualsBytes v = {0, 0};
        if ((c + 1) * QUALS_CHUNK > col.size())
            outside = true;
        else
            for (u32 k = 0; k < QUALS_CHUNK; k++)
                quals_put(v, k, col[(size_t)(c * QUALS_CHUNK + k)]);
        return v;
    };
    auto tile_lanes = [&](u64 t, std::vector<QualsLane> &l, std::vector<u64> &ex) {     // the lanes and the scan of their sums
        u64 tot = 0;
        l.clear();
        ex.clear();
        for (u32 r = 0; r < L; r++) {
            const u64 c = c0 + t * L + r;
            l.push_back(quals_lane(base, c < c_end ? n : 0, c, load));
            ex.push_back(tot);
            tot += quals_lane_sum(l.back());
        }
        return tot;
    };
    std::vector<QualsLane> l;
    std::vector<u64> ex;
    u64 qtot = 0;
    for (u64 t = 0; t < tiles; t++)
        qtot += tile_lanes(t, l, ex);
    i64 fv = 0, fi = -1, tv = 0, ti = (i64)n;
    if (o.cut_front) {
        u64 before = 0;
        for (u64 t = 0; t < tiles; t++) {
            const u64 tot = tile_lanes(t, l, ex);
            i64 neg = QUALS_NONE;
            for (u32 r = 0; r < L && neg == QUALS_NONE; r++)
                neg = quals_lane_front_neg(l[r], before + ex[r], o.cut_front);
            std::vector<i64> bv(L, fv), bi(L, fi);
            i64 top = fv;
            for (u32 r = 0; r < L; r++) {
                quals_lane_front_best(l[r], before + ex[r], o.cut_front, neg, &bv[r], &bi[r]);
                top = bv[r] > top ? bv[r] : top;
            }
            for (u32 r = 0; r < L; r++)
                if (bv[r] == top) {
                    fi = bi[r];
                    break;
                }
            fv = top;
            if (neg != QUALS_NONE)
                break;
            before += tot;
        }
    }
    if (o.cut_tail) {
        u64 behind = 0;
        for (u64 t = tiles; t-- > 0;) {
            const u64 tot = tile_lanes(t, l, ex), before = qtot - behind - tot;
            i64 neg = -1;
            for (u32 r = L; r-- > 0 && neg < 0;)
                neg = quals_lane_tail_neg(l[r], before + ex[r], qtot, n, o.cut_tail);
            std::vector<i64> bv(L, tv), bi(L, ti);
            i64 top = tv;
            for (u32 r = 0; r < L; r++) {
                quals_lane_tail_best(l[r], before + ex[r], qtot, n, o.cut_tail, neg, &bv[r], &bi[r]);
                top = bv[r] > top ? bv[r] : top;
            }
            for (u32 r = L; r-- > 0;)
                if (bv[r] == top) {
                    ti = bi[r];
                    break;
                }
            tv = top;
            if (neg >= 0)
                break;
            behind += tot;
        }
    }
    Cut c = {fi + 1, ti, 0, 0};
    if (c.start >= c.stop)
        c.start = c.stop = 0;
    for (u64 t = 0; t < tiles; t++) {
        tile_lanes(t, l, ex);
        for (u32 r = 0; r < L; r++)
            quals_lane_range(l[r], c.start, c.stop, o.low_q, &c.qsum, &c.low);
    }
    CHECK(!outside, "a chunk outside the column was asked for");
    return c;
}

static u64 trimmed = 0;
static void check_trim(const std::vector<unsigned char> &col, u64 base, u64 n, const QualsTrimOpt &o, const char *what)
{
    const Cut want = naive_trim(col.data() + base, n, o);
    for (u32 L : {1u, 2u, 16u, 64u}) {
        if (L < 16 && n > 200)
            continue;
        const Cut got = team_trim(col, base, n, o, L);
        CHECK(got.start == want.start && got.stop == want.stop && got.qsum == want.qsum && got.low == want.low,
              "%s: n=%llu base=%llu F=%u T=%u lanes=%u: [%lld, %lld) qsum %llu low %llu, expected [%lld, %lld) %llu %llu", what,
              (unsigned long long)n, (unsigned long long)base, o.cut_front, o.cut_tail, L, got.start, got.stop, (unsigned long long)got.qsum,
              (unsigned long long)got.low, want.start, want.stop, (unsigned long long)want.qsum, (unsigned long long)want.low);
    }
    trimmed++;
}

static void check_trims()
{
    // the worked example: 42 40 26 27 8 7 11 4 2 3 with T = 10 stops at 4
    {
        const unsigned char q[] = {42 + 33, 40 + 33, 26 + 33, 27 + 33, 8 + 33, 7 + 33, 11 + 33, 4 + 33, 2 + 33, 3 + 33};
        const QualsTrimOpt o = {0, 10, 0, 0, 0, 0, 0};
        const Cut c = naive_trim(q, 10, o);
        CHECK(c.start == 0 && c.stop == 4 && c.qsum == 135, "the worked example: [%lld, %lld)", c.start, c.stop);
        std::vector<unsigned char> col(48, '!');
        for (u64 base = 0; base < 32; base++) {
            for (u32 k = 0; k < 10; k++)
                col[(size_t)(base + k)] = q[k];
            check_trim(col, base, 10, o, "the worked example");
            for (u32 k = 0; k < 10; k++)
                col[(size_t)(base + k)] = '!';
        }
    }
    // 50,000 random reads of 1 .. 400 bases (and the edge lengths) at random alignments: values that wander around the
    // thresholds so that breaks, ties and crossing cuts all occur; then long ones that take several tiles of every team
    std::vector<unsigned char> col((size_t)1 << 16);
    const u64 edges[] = {1, 2, 15, 16, 17, 31, 32, 33, 240, 241, 242, 255, 256, 257, 1008, 1009, 1010, 1023, 1024, 1025};
    for (u64 round = 0; round < 50000 + 20 * 16; round++) {
        const u64 n = round < 50000 ? 1 + rng() % 400 : edges[(round - 50000) / 16];
        const u64 base = round < 50000 ? rng() % 64 : (round - 50000) % 16;
        const u32 mode = (u32)(rng() % 6);
        const u32 F = (u32)(rng() % 4 == 0 ? 0 : 1 + rng() % 40), T = (u32)(rng() % 4 == 0 ? 0 : 1 + rng() % 40);
        for (u64 i = 0; i < n; i++) {
            u32 v;
            if (mode == 0)
                v = (u32)(rng() % 94);
            else if (mode == 1)
                v = 41;                                              // all high
            else if (mode == 2)
                v = 2;                                               // all low
            else if (mode == 3)
                v = (u32)((F ? F : 20) + (i64)(rng() % 5) - 2);      // around the threshold: many ties
            else
                v = (i * 5 < n || i * 5 > 4 * n) ? (u32)(rng() % 12) : (u32)(25 + rng() % 16);      // bad ends
            col[(size_t)(base + i)] = (unsigned char)(33 + (v > 93 ? 93 : v));
        }
        const QualsTrimOpt o = {F, T, 0, (u32)(rng() % 45), 0, 0, 0};
        check_trim(col, base, n, o, "random read");
    }
    for (u64 round = 0; round < 40; round++) {
        const u64 n = 4000 + rng() % 9000, base = rng() % 64;
        const u64 dip = rng() % n;                                   // one place where the running sums go negative
        for (u64 i = 0; i < n; i++)
            col[(size_t)(base + i)] = (unsigned char)(33 + (i == dip ? 93 : (rng() % 3 == 0 ? 12 : 9)));
        const QualsTrimOpt o = {10, 10, 0, 10, 0, 0, 0};
        check_trim(col, base, n, o, "a long read");
    }
    // the verdicts, in their order
    {
        const QualsTrimOpt o = {0, 0, 20, 0, 1, 4, 10};
        CHECK(quals_verdict(0, 0, 0, o) == QUALS_FAIL_SHORT && quals_verdict(9, 900, 0, o) == QUALS_FAIL_SHORT &&
                  quals_verdict(10, 199, 0, o) == QUALS_FAIL_MEAN && quals_verdict(10, 200, 3, o) == QUALS_FAIL_LOW &&
                  quals_verdict(12, 240, 3, o) == QUALS_PASS && quals_verdict(10, 200, 2, o) == QUALS_PASS,
              "the verdicts");
        const QualsTrimOpt none = {0, 0, 0, 0, 0, 0, 0};
        CHECK(quals_verdict(1, 0, 1, none) == QUALS_PASS && quals_verdict(0, 0, 0, none) == QUALS_FAIL_SHORT, "the verdicts with no threshold");
    }
    CHECK(trimmed >= 50000 + 20 * 16 + 40 + 32, "only %llu reads were trimmed", (unsigned long long)trimmed);
    CHECK(QUALS_GROUP_BASES == 241 && QUALS_WAVE_BASES == 1009 && QUALS_TRIM_TILE_BASES == 4081, "the limits of the paths");
}

int main()
{
    check_trims();
    const u64 lengths[] = {0, 1, 15, 16, 17, 31, 32, 33};

    // every source offset x every output offset x every length, forward and flipped, at every misalignment of the source
    for (u32 mis = 0; mis < 4; mis++) {
        const std::vector<unsigned char> src = make_source(16 + 33 + 40);
        for (u64 s = 0; s < 16; s++)
            for (u64 d = 0; d < 16; d++)
                for (u64 len : lengths)
                    for (int f = 0; f < 2; f++) {
                        std::vector<Seg> segs = {{(s * 5 + d) % 16, d, (uint8_t)(f ^ 1)}, {s, len, (uint8_t)f}, {s + 3, 40 - d, (uint8_t)f}};
                        check_list(src, mis, segs, "alignment grid");
                    }
    }
    // segments that begin at the source's first byte and end at its last: the words of a whole piece must stay inside
    for (u64 n : {1ull, 15ull, 16ull, 17ull, 19ull, 20ull, 21ull, 32ull, 33ull, 35ull, 36ull, 48ull})
        for (u32 mis = 0; mis < 4; mis++)
            for (int f = 0; f < 2; f++) {
                const std::vector<unsigned char> src = make_source(n);
                std::vector<Seg> segs;
                for (u64 len : lengths)
                    if (len <= n) {
                        segs.push_back({n - len, len, (uint8_t)f});
                        segs.push_back({0, len, (uint8_t)f});
                    }
                segs.push_back({0, n, (uint8_t)f});
                segs.push_back({0, n, (uint8_t)(f ^ 1)});
                segs.push_back({n, 0, 1});
                check_list(src, mis, segs, "ends at the last byte");
            }
    // 50,000 random reads in lists of up to 200: empties, repeats, overlaps; about a third flipped
    u64 reads = 0;
    while (reads < 50000) {
        const u64 src_n = 1 + rng() % 3000;
        const std::vector<unsigned char> src = make_source(src_n);
        std::vector<Seg> segs;
        const u64 n = 1 + rng() % 200;
        for (u64 i = 0; i < n; i++) {
            const u64 kind = rng() % 8;
            u64 len = kind < 1 ? 0 : kind < 3 ? lengths[rng() % 8] : kind < 5 ? rng() % 5 : kind < 7 ? 100 + rng() % 100 : rng() % (src_n + 1);
            if (len > src_n)
                len = src_n;
            segs.push_back({rng() % (src_n - len + 1), len, (uint8_t)(rng() % 3 == 0)});
            if (kind == 7)
                segs.push_back(segs.back());
        }
        if (reads % 3 == 0)
            segs.insert(segs.begin(), 3, Seg{rng() % (src_n + 1), 0, 1});
        if (reads % 3 == 1)
            segs.insert(segs.end(), 4, Seg{src_n, 0, 0});
        check_list(src, (u32)(rng() & 3), segs, "random list");
        reads += segs.size();
    }
    // all empty: no chunk at all
    check_list(make_source(40), 0, {{0, 0, 0}, {40, 0, 1}, {17, 0, 0}}, "all empty");
    // (a quarter of the random reads have 100 .. 199 bytes: at least five whole chunks each, formed twice)
    CHECK(formed_whole > 50000, "only %llu pieces were formed from words", (unsigned long long)formed_whole);

    // the sixteen-byte helpers
    {
        QualsBytes v = {0, 0};
        for (u32 k = 0; k < 16; k++)
            quals_put(v, k, 0x40 + k);
        const QualsBytes r = quals_reverse(v);
        for (u32 k = 0; k < 16; k++)
            CHECK(quals_get(v, k) == 0x40 + k && quals_get(r, k) == 0x40 + 15 - k, "put / get / reverse at byte %u", k);
        CHECK(quals_swap64(0x0102030405060708ull) == 0x0807060504030201ull, "quals_swap64");
    }
    // the class, the error word, the sizes
    for (u32 b = 0; b < 256; b++)
        CHECK(quals_valid(b) == (b >= '!' && b <= '~'), "quals_valid(%u)", b);
    CHECK(quals_error_key(7, QUALS_ERR_LENGTH) < quals_error_key(7, QUALS_ERR_CHAR) &&
              quals_error_key(7, QUALS_ERR_CHAR) < quals_error_key(7, QUALS_ERR_TRUNC) &&
              quals_error_key(7, QUALS_ERR_TRUNC) < quals_error_key(8, QUALS_ERR_LENGTH) && quals_error_key(0xFFFFFFFFull, 3) < QUALS_NO_ERROR,
          "the order of the error words");
    CHECK(quals_error_pos(quals_error_key(0xFFFFFFFFull, QUALS_ERR_CHAR)) == 0xFFFFFFFFull &&
              quals_error_kind(quals_error_key(5, QUALS_ERR_TRUNC)) == QUALS_ERR_TRUNC,
          "the error word's parts");
    CHECK(quals_chunks(0) == 0 && quals_chunks(1) == 1 && quals_chunks(16) == 1 && quals_chunks(17) == 2 && quals_tiles(QUALS_TILE_BYTES) == 1 &&
              quals_tiles(QUALS_TILE_BYTES + 1) == 2 && quals_alloc_bytes(0) == 16 && quals_alloc_bytes(17) == 32,
          "the sizes");
    // the length of a line: "AC\r\n" is 2, "AC\r" at the end of the text is 3, "\r\n" is 0, "\n" is 0
    {
        const char *t = "AC\r\nAC\r";
        const auto byte = [&](u32 i) { return (u32)(unsigned char)t[i]; };
        CHECK(quals_line_len(0, 3, 7, byte) == 2 && quals_line_len(4, 7, 7, byte) == 3, "quals_line_len with a carriage return");
        const char *e = "\r\n\n";
        const auto byte2 = [&](u32 i) { return (u32)(unsigned char)e[i]; };
        CHECK(quals_line_len(0, 1, 3, byte2) == 0 && quals_line_len(2, 2, 3, byte2) == 0, "quals_line_len of empty lines");
    }

    if (bad) {
        printf("%d checks failed\n", bad);
        return 1;
    }
    printf("ok\n");
    return 0;
}
