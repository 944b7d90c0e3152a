/* row_batch_check.c -- glue/row_batch.h as a stand-alone program (tests/test_row_batch.py builds it plain and with
 * AddressSanitizer + UndefinedBehaviorSanitizer): the packed stream and the starts against a packer that moves one base at a
 * time, every row cut back out of the stream, a cleared batch refilled, the growth of the arrays, the two tests of the add
 * policy.  Every source row is a heap buffer of exactly ceil(length / 32) words. */
#include <stdio.h>
#include <string.h>

#include "row_batch.h"

static int failures;
#define CHECK(cond, ...)                           \
    do {                                           \
        if (!(cond)) {                             \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                   \
            printf("\n");                          \
            failures++;                            \
        }                                          \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static uint64_t words_of(uint64_t n) { return (n + 31) / 32; }

/* a row of `len` bases in a buffer of exactly words_of(len) words (NULL for no base); fill < 0: random bases, else every base
 * = fill.  The bits behind the last base are SET: a row's tail must not reach the stream. */
static uint64_t *make_row(uint64_t len, int fill)
{
    const uint64_t nw = words_of(len);
    if (nw == 0)
        return NULL;
    uint64_t *w = (uint64_t *)malloc((size_t)nw * sizeof *w);
    for (uint64_t i = 0; i < nw; i++)
        w[i] = fill < 0 ? rng() : (uint64_t)fill * 0x5555555555555555ull;
    if (len & 31)
        w[nw - 1] |= ~(uint64_t)0 << (2 * (len & 31));
    return w;
}

static unsigned base_at(const uint64_t *w, uint64_t i) { return (unsigned)(w[i >> 5] >> (2 * (i & 31))) & 3u; }

/* the reference: the bases of all rows one byte each, packed one base at a time */
typedef struct Ref {
    unsigned char *bases;
    uint64_t n, cap;
    uint64_t *starts, n_seqs, cap_seqs;
} Ref;

static void ref_add(Ref *r, const uint64_t *row, uint64_t len)
{
    if (r->n + len > r->cap) {
        r->cap = 2 * (r->n + len) + 64;
        r->bases = (unsigned char *)realloc(r->bases, (size_t)r->cap);
    }
    if (r->n_seqs + 2 > r->cap_seqs) {
        r->cap_seqs = 2 * r->cap_seqs + 64;
        r->starts = (uint64_t *)realloc(r->starts, (size_t)r->cap_seqs * sizeof(uint64_t));
    }
    r->starts[0] = 0;
    for (uint64_t i = 0; i < len; i++)
        r->bases[r->n++] = (unsigned char)base_at(row, i);
    r->starts[++r->n_seqs] = r->n;
}

static void ref_free(Ref *r)
{
    free(r->bases);
    free(r->starts);
    memset(r, 0, sizeof *r);
}

/* b against r: the counters, the starts, every word of the stream (the last one with a zero tail), and every row cut out */
static void compare(const RowBatch *b, const Ref *r, const char *what)
{
    CHECK(b->n_bases == r->n && b->n_seqs == r->n_seqs, "%s: %llu bases in %llu rows, expected %llu in %llu", what,
          (unsigned long long)b->n_bases, (unsigned long long)b->n_seqs, (unsigned long long)r->n, (unsigned long long)r->n_seqs);
    if (b->n_bases != r->n || b->n_seqs != r->n_seqs)
        return;
    CHECK(b->cap_words >= words_of(b->n_bases) + 1 && b->cap_seqs >= b->n_seqs + 1, "%s: the arrays are too short", what);
    for (uint64_t s = 0; s <= r->n_seqs; s++)
        CHECK(b->starts[s] == r->starts[s], "%s: starts[%llu] = %llu, expected %llu", what, (unsigned long long)s,
              (unsigned long long)b->starts[s], (unsigned long long)r->starts[s]);
    const uint64_t nw = words_of(r->n);
    for (uint64_t w = 0; w < nw; w++) {
        uint64_t v = 0;
        for (uint64_t i = 32 * w; i < 32 * (w + 1) && i < r->n; i++)
            v |= (uint64_t)r->bases[i] << (2 * (i & 31));
        CHECK(b->words[w] == v, "%s: word %llu = %016llx, expected %016llx", what, (unsigned long long)w,
              (unsigned long long)b->words[w], (unsigned long long)v);
    }
    for (uint64_t s = 0; s < r->n_seqs; s++) {
        const uint64_t first = r->starts[s], len = r->starts[s + 1] - first, cw = words_of(len);
        uint64_t *cut = (uint64_t *)malloc((size_t)(cw ? cw : 1) * sizeof *cut);
        memset(cut, 0xEE, (size_t)(cw ? cw : 1) * sizeof *cut);
        rb_cut(b->words, first, len, cut);
        for (uint64_t w = 0; w < cw; w++) {
            uint64_t v = 0;
            for (uint64_t i = 32 * w; i < 32 * (w + 1) && i < len; i++)
                v |= (uint64_t)r->bases[first + i] << (2 * (i & 31));
            CHECK(cut[w] == v, "%s: row %llu cut, word %llu = %016llx, expected %016llx", what, (unsigned long long)s,
                  (unsigned long long)w, (unsigned long long)cut[w], (unsigned long long)v);
        }
        free(cut);
    }
}

static void add(RowBatch *b, Ref *r, uint64_t len, int fill)
{
    uint64_t *row = make_row(len, fill);
    CHECK(rb_append(b, row, len), "rb_append of %llu bases failed", (unsigned long long)len);
    ref_add(r, row, len);
    free(row);
}

static const uint64_t LENGTHS[] = {0, 1, 31, 32, 33, 63, 64, 65, 1000};
#define N_LENGTHS (sizeof LENGTHS / sizeof LENGTHS[0])

/* every length at every offset 0 .. 31 of its first base in a word: in one long batch, and as the second row of a fresh one */
static void check_offsets(int fill, const char *what)
{
    RowBatch b = {0};
    Ref r = {0};
    for (uint64_t off = 0; off < 32; off++)
        for (size_t l = 0; l < N_LENGTHS; l++) {
            add(&b, &r, (off + 32 - (b.n_bases & 31)) & 31, fill);             /* a pad row: the next one starts at `off` */
            CHECK((b.n_bases & 31) == off, "%s: the pad row missed offset %llu", what, (unsigned long long)off);
            add(&b, &r, LENGTHS[l], fill);
            RowBatch f = {0};
            Ref fr = {0};
            add(&f, &fr, off, fill);
            add(&f, &fr, LENGTHS[l], fill);
            add(&f, &fr, 7, fill);
            compare(&f, &fr, what);
            rb_free(&f);
            ref_free(&fr);
        }
    compare(&b, &r, what);
    CHECK(b.cap_words > 1024, "%s: the long batch was meant to outgrow its first allocation", what);
    rb_free(&b);
    CHECK(!b.words && !b.starts && !b.cap_words && !b.cap_seqs && !b.n_bases && !b.n_seqs, "%s: rb_free left something", what);
    ref_free(&r);
}

/* all-T rows, cleared, all-A rows: no bit of the first filling may be left */
static void check_clear(void)
{
    RowBatch b = {0};
    Ref r = {0};
    for (uint64_t off = 0; off < 32; off++)
        for (size_t l = 0; l < N_LENGTHS; l++)
            add(&b, &r, LENGTHS[l] + off, 3);
    compare(&b, &r, "all T");
    const uint64_t cap_words = b.cap_words, cap_seqs = b.cap_seqs, filled = words_of(b.n_bases);
    rb_clear(&b);
    CHECK(b.n_bases == 0 && b.n_seqs == 0 && b.cap_words == cap_words && b.cap_seqs == cap_seqs && b.words && b.starts,
          "rb_clear changed more than the counters");
    ref_free(&r);
    for (uint64_t off = 0; off < 32; off++)
        for (size_t l = 0; l < N_LENGTHS; l++)
            add(&b, &r, LENGTHS[N_LENGTHS - 1 - l] + (31 - off), 0);
    compare(&b, &r, "all A after all T");
    CHECK(words_of(b.n_bases) == filled, "the refill was meant to cover the words of the first filling");
    for (uint64_t w = 0; w < words_of(b.n_bases); w++)
        CHECK(b.words[w] == 0, "a stale bit in word %llu: %016llx", (unsigned long long)w, (unsigned long long)b.words[w]);
    rb_free(&b);
    ref_free(&r);
}

/* the arrays start at 1024 entries and double; what they held stays */
static void check_growth(void)
{
    RowBatch b = {0};
    Ref r = {0};
    add(&b, &r, 5, -1);
    CHECK(b.cap_words == 1024 && b.cap_seqs == 1024, "the first allocation has %llu words and %llu starts",
          (unsigned long long)b.cap_words, (unsigned long long)b.cap_seqs);
    add(&b, &r, 32 * 1022 - 5, -1);                      /* 1022 words + the spare word: still the first allocation */
    CHECK(b.cap_words == 1024, "1023 words needed, %llu allocated", (unsigned long long)b.cap_words);
    add(&b, &r, 32, -1);                                 /* 1023 words + the spare word */
    CHECK(b.cap_words == 1024, "1024 words needed, %llu allocated", (unsigned long long)b.cap_words);
    add(&b, &r, 1, -1);                                  /* 1024 words + the spare word: grown */
    CHECK(b.cap_words == 2048, "1025 words needed, %llu allocated", (unsigned long long)b.cap_words);
    add(&b, &r, 32 * 4000 + 3, -1);                      /* several doublings at once */
    CHECK(b.cap_words == 8192, "5025 words needed, %llu allocated", (unsigned long long)b.cap_words);
    while (b.n_seqs < 1023)                              /* (n_seqs + 2 entries are asked for) */
        add(&b, &r, 0, -1);
    CHECK(b.cap_seqs == 1024, "1024 starts needed, %llu allocated", (unsigned long long)b.cap_seqs);
    add(&b, &r, 0, -1);
    CHECK(b.cap_seqs == 2048, "1025 starts needed, %llu allocated", (unsigned long long)b.cap_seqs);
    compare(&b, &r, "growth");
    rb_free(&b);
    ref_free(&r);
}

static void check_policy(void)
{
    const uint64_t limit = 100;
    RowBatch b = {0};
    Ref r = {0};
    CHECK(!rb_spills(&b, 0, limit) && !rb_spills(&b, limit + 1, limit) && !rb_spills(&b, ~(uint64_t)0 >> 1, limit),
          "a first row spilled");
    CHECK(!rb_full(&b, limit), "an empty batch is full");
    add(&b, &r, 0, -1);                                  /* a row without a base is a row */
    CHECK(rb_spills(&b, limit + 1, limit) && !rb_spills(&b, limit, limit) && !rb_full(&b, limit), "after an empty row");
    add(&b, &r, 60, -1);
    CHECK(!rb_spills(&b, 39, limit) && !rb_spills(&b, 40, limit) && rb_spills(&b, 41, limit), "spills at 60 + 39 / 40 / 41");
    add(&b, &r, 39, -1);
    CHECK(!rb_full(&b, limit), "full at limit - 1");
    add(&b, &r, 1, -1);
    CHECK(rb_full(&b, limit), "not full at the limit");
    CHECK(!rb_spills(&b, 0, limit) && rb_spills(&b, 1, limit), "spills at the limit");
    add(&b, &r, 1, -1);
    CHECK(rb_full(&b, limit) && rb_spills(&b, 0, limit), "at limit + 1");
    compare(&b, &r, "policy");
    rb_clear(&b);
    CHECK(!rb_spills(&b, limit + 1, limit) && !rb_full(&b, limit), "a cleared batch is an empty one");
    rb_free(&b);
    ref_free(&r);
}

int main(void)
{
    check_offsets(-1, "random rows");
    check_offsets(3, "all-T rows");
    check_clear();
    check_growth();
    check_policy();
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("row_batch ok\n");
    return 0;
}
