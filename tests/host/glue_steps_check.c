/* glue_steps_check.c -- glue/glue_steps.h as a stand-alone program (tests/test_glue_steps.py builds it plain and with
 * AddressSanitizer + UndefinedBehaviorSanitizer): the column groups, the window cursor, the add policy against a counting
 * flush and against a written-out copy of the policy, the life cycle, the byte buffer and the bound normalisers. */
#include <stdio.h>

#include "glue_steps.h"

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
#define ULL(x) ((unsigned long long)(x))

/* ---- column groups: one, two and four columns past the first 1024 units and across one doubling; old contents are kept */
static void check_columns(void)
{
    for (int n = 1; n <= 4; n += n) {
        uint64_t *col[4] = {0}, cap = 0, filled = 0;
        void **const cols[4] = {(void **)&col[0], (void **)&col[1], (void **)&col[2], (void **)&col[3]};
        static const uint64_t needs[] = {0, 1, 1024, 1025, 2048, 2049};
        static const uint64_t caps[] = {0, 1024, 1024, 2048, 2048, 4096};
        for (size_t s = 0; s < sizeof needs / sizeof needs[0]; s++) {
            CHECK(gs_grow(cols, n, &cap, needs[s]), "gs_grow of %d columns to %llu failed", n, ULL(needs[s]));
            CHECK(cap == caps[s], "%d columns, %llu needed: capacity %llu, expected %llu", n, ULL(needs[s]), ULL(cap), ULL(caps[s]));
            for (int c = 0; c < n; c++) {
                for (uint64_t i = 0; i < filled; i++)
                    CHECK(col[c][i] == 1000003 * (uint64_t)c + i, "%d columns: column %d lost entry %llu", n, c, ULL(i));
                for (uint64_t i = filled; i < needs[s]; i++)
                    col[c][i] = 1000003 * (uint64_t)c + i;                 /* (every unit of the capacity asked for is writable) */
            }
            filled = needs[s];
        }
        for (int c = 0; c < 4; c++) {
            CHECK((col[c] != NULL) == (c < n), "%d columns: column %d %s", n, c, col[c] ? "was touched" : "is missing");
            free(col[c]);
        }
    }
}

/* ---- the window cursor: every row of every total served once, in order; the refills sum to the total and none is empty */
static void check_window(void)
{
    const uint64_t W = 4, totals[] = {0, 1, W - 1, W, W + 1, 2 * W + 1};
    for (size_t t = 0; t < sizeof totals / sizeof totals[0]; t++) {
        const uint64_t total = totals[t];
        GsWindow w = {0, 0, 0};
        uint64_t refills = 0, asked = 0;
        CHECK(!gs_win_has(&w), "a fresh window has a row");
        for (; w.next < total; w.next++) {
            if (!gs_win_has(&w)) {
                const uint64_t n = gs_refill(total, w.next, W);
                CHECK(n >= 1 && n <= W && n == (total - w.next < W ? total - w.next : W), "total %llu, next %llu: refill of %llu",
                      ULL(total), ULL(w.next), ULL(n));
                gs_win_filled(&w, n);
                CHECK(w.first == w.next && w.count == n, "gs_win_filled");
                refills++;
                asked += n;
            }
            CHECK(gs_win_has(&w) && gs_win_at(&w) == w.next % W && gs_win_at(&w) < w.count, "total %llu, next %llu: index %llu of %llu",
                  ULL(total), ULL(w.next), ULL(gs_win_at(&w)), ULL(w.count));
        }
        CHECK(asked == total && refills == (total + W - 1) / W, "total %llu: %llu rows in %llu refills", ULL(total), ULL(asked), ULL(refills));
        CHECK(gs_refill(total, total, W) == 0, "a refill behind the last row");
        CHECK(!gs_win_has(&w), "total %llu: row %llu, behind the last one, is in the window", ULL(total), ULL(w.next));
    }
}

/* ---- the add policy */
typedef struct Sink {
    RowBatch b;
    uint64_t log[64][2], n_log;                  /* every flush: the batch's rows and bases */
    uint64_t fail_at;                            /* the flush with this ordinal fails (and leaves the batch) */
} Sink;

static bool sink_flush(void *self)
{
    Sink *s = (Sink *)self;
    if (s->n_log == s->fail_at)
        return false;
    s->log[s->n_log][0] = s->b.n_seqs;
    s->log[s->n_log++][1] = s->b.n_bases;
    rb_clear(&s->b);
    return true;
}

/* the policy as the glue's batch_add spelled it before glue_steps.h, error texts apart */
static bool written_out_add(Sink *s, const uint64_t *bits, uint64_t length, uint64_t limit)
{
    if (rb_spills(&s->b, length, limit) && !sink_flush(s))
        return false;
    if (!rb_append(&s->b, bits, length))
        return false;
    return !rb_full(&s->b, limit) || sink_flush(s);
}

static void check_policy(void)
{
    static uint64_t bits[8];                     /* 256 bases of A */
    const uint64_t limits[] = {1, 64, 1000000};
    for (size_t l = 0; l < 3; l++) {
        const uint64_t limit = limits[l], big = limit > 200 ? 200 : limit;
        /* rows of 0, 1, limit - 1, limit and limit + 1 bases, a first row longer than the limit, later ones too */
        const uint64_t rows[] = {big + 1, 0, 1, big - 1, big, big + 1, 0, 0, big + 1, 1, 1, big, 0, big - 1, 1, 1, 0};
        const size_t n_rows = sizeof rows / sizeof rows[0];
        Sink a = {.fail_at = UINT64_MAX}, b = {.fail_at = UINT64_MAX};
        for (size_t i = 0; i < n_rows; i++) {
            const uint64_t before = a.n_log, open_rows = a.b.n_seqs, open_bases = a.b.n_bases;
            CHECK(gs_add(&a.b, bits, rows[i], limit, sink_flush, &a) == GS_ADDED, "limit %llu: row %zu refused", ULL(limit), i);
            CHECK(written_out_add(&b, bits, rows[i], limit), "limit %llu: the written-out policy refused row %zu", ULL(limit), i);
            const bool spills = open_rows > 0 && open_bases + rows[i] > limit;
            const bool fills = (spills ? 0 : open_bases) + rows[i] >= limit;
            CHECK(a.n_log - before == (uint64_t)spills + (uint64_t)fills, "limit %llu, row %zu of %llu bases on %llu: %llu flushes",
                  ULL(limit), i, ULL(rows[i]), ULL(open_bases), ULL(a.n_log - before));
            if (i == 0)
                CHECK(a.n_log == (rows[0] >= limit) && (a.n_log == 0 || a.log[0][0] == 1),
                      "limit %llu: a first row longer than the limit was not flushed alone, after itself", ULL(limit));
            if (spills && fills)                 /* a later long row: the open batch before it, itself after it */
                CHECK(a.log[before][0] == open_rows && a.log[before][1] == open_bases && a.log[before + 1][0] == 1 &&
                      a.log[before + 1][1] == rows[i], "limit %llu, row %zu: the two flushes", ULL(limit), i);
        }
        CHECK(a.n_log == b.n_log && a.b.n_seqs == b.b.n_seqs && a.b.n_bases == b.b.n_bases, "limit %llu: %llu flushes, written out %llu",
              ULL(limit), ULL(a.n_log), ULL(b.n_log));
        for (uint64_t f = 0; f < a.n_log && f < b.n_log; f++)
            CHECK(a.log[f][0] == b.log[f][0] && a.log[f][1] == b.log[f][1], "limit %llu: flush %llu differs", ULL(limit), ULL(f));
        uint64_t flushed = 0;
        for (uint64_t f = 0; f < a.n_log; f++)
            flushed += a.log[f][0];
        CHECK(flushed + a.b.n_seqs == n_rows, "limit %llu: %llu rows flushed, %llu open", ULL(limit), ULL(flushed), ULL(a.b.n_seqs));
        CHECK(limit < 1000000 ? a.n_log > 3 : a.n_log == 0, "limit %llu: %llu flushes", ULL(limit), ULL(a.n_log));
        rb_free(&a.b);
        rb_free(&b.b);
    }
    /* a failing flush stops the add: before the row (the spill) and after it (the full batch) */
    Sink s = {.fail_at = 0};
    CHECK(gs_add(&s.b, bits, 10, 64, sink_flush, &s) == GS_ADDED && s.b.n_seqs == 1, "the first row");
    CHECK(gs_add(&s.b, bits, 60, 64, sink_flush, &s) == GS_FLUSH_FAILED && s.b.n_seqs == 1 && s.b.n_bases == 10,
          "a failed spill flush let the row in");
    CHECK(gs_add(&s.b, bits, 54, 64, sink_flush, &s) == GS_FLUSH_FAILED && s.b.n_seqs == 2 && s.b.n_bases == 64,
          "a failed flush of a full batch");
    rb_free(&s.b);
}

/* ---- the life cycle */
static int last_runs;
static bool last_ok(void *self) { last_runs++; return *(bool *)self; }

static void check_life(void)
{
    for (int good = 0; good < 2; good++) {
        GsLife l = {false, false};
        bool result = good != 0;
        last_runs = 0;
        CHECK(gs_may_add(&l), "a fresh object takes no row");
        CHECK(gs_serve(&l, last_ok, &result) == result && last_runs == 1, "the first _next");
        CHECK(l.started && l.failed == !result, "after the first _next: started %d, failed %d", l.started, l.failed);
        CHECK(!gs_may_add(&l), "a row after the first _next");
        for (int i = 0; i < 3; i++)
            CHECK(gs_serve(&l, last_ok, &result) == result, "a later _next");
        CHECK(last_runs == 1, "the last step ran %d times", last_runs);
    }
    GsLife f = {false, true};                    /* failed while rows were added */
    bool yes = true;
    last_runs = 0;
    CHECK(!gs_may_add(&f) && !gs_serve(&f, last_ok, &yes) && last_runs == 0 && !f.started, "a failed object");
}

/* ---- the byte buffer */
static void check_bytes(void)
{
    static char src[4097];
    for (size_t i = 0; i < sizeof src; i++)
        src[i] = (char)(i * 7 + 1);
    const uint64_t feeds[] = {0, 1, 4095, 4096, 4097};
    for (size_t f = 0; f < 5; f++) {
        GsBytes b = {0};
        CHECK(gs_bytes_append(&b, feeds[f] ? src : NULL, feeds[f]) && b.len == feeds[f], "a feed of %llu bytes", ULL(feeds[f]));
        CHECK(b.cap == (feeds[f] == 0 ? 0 : feeds[f] <= 4096 ? 4096 : 8192), "%llu bytes: capacity %llu", ULL(feeds[f]), ULL(b.cap));
        CHECK(gs_bytes_append(&b, src, 1) && b.len == feeds[f] + 1 && b.buf[feeds[f]] == src[0], "one more byte behind %llu", ULL(feeds[f]));
        CHECK(b.cap == (feeds[f] < 4096 ? 4096 : 8192), "%llu + 1 bytes: capacity %llu", ULL(feeds[f]), ULL(b.cap));
        CHECK(feeds[f] == 0 || memcmp(b.buf, src, (size_t)feeds[f]) == 0, "%llu bytes: the contents", ULL(feeds[f]));
        const uint64_t len = b.len, part = len / 3;
        gs_bytes_drop(&b, 0);
        CHECK(b.len == len && b.buf[0] == src[0], "a drop of nothing");
        gs_bytes_drop(&b, part);
        CHECK(b.len == len - part && (part >= feeds[f] || memcmp(b.buf, src + part, (size_t)(feeds[f] - part)) == 0) &&
              b.buf[b.len - 1] == src[0], "a drop of %llu of %llu bytes", ULL(part), ULL(len));
        gs_bytes_drop(&b, b.len);
        CHECK(b.len == 0, "a drop of everything");
        CHECK(gs_bytes_append(&b, src, 2) && b.len == 2 && b.buf[1] == src[1], "a feed into the emptied buffer");
        free(b.buf);
    }
    uint64_t chunk = 1, steps = 0;
    const uint64_t max = 100;
    const uint64_t want[] = {2, 4, 8, 16, 32, 64, 100};
    while (gs_chunk_grow(&chunk, max)) {
        CHECK(steps < 7 && chunk == want[steps], "step %llu: a chunk of %llu", ULL(steps), ULL(chunk));
        steps++;
    }
    CHECK(steps == 7 && chunk == max && !gs_chunk_grow(&chunk, max) && chunk == max, "the chunk ends at %llu after %llu steps", ULL(chunk), ULL(steps));
    chunk = UINT32_MAX / 2 + 1;
    CHECK(gs_chunk_grow(&chunk, UINT32_MAX) && chunk == UINT32_MAX, "the last step to 2^32 - 1");
}

static void check_bounds(void)
{
    const int64_t in[] = {-1, 0, 1, INT64_MAX};
    const uint64_t lower1[] = {1, 1, 1, (uint64_t)INT64_MAX}, lower0[] = {0, 0, 1, (uint64_t)INT64_MAX};
    const uint64_t upper[] = {UINT64_MAX, 0, 1, (uint64_t)INT64_MAX};
    for (int i = 0; i < 4; i++) {
        CHECK(gs_lower_bound(in[i], 1) == lower1[i] && gs_lower_bound(in[i], 0) == lower0[i], "the lower bound of %lld", (long long)in[i]);
        CHECK(gs_upper_bound(in[i]) == upper[i], "the upper bound of %lld", (long long)in[i]);
    }
}

int main(void)
{
    check_columns();
    check_window();
    check_policy();
    check_life();
    check_bytes();
    check_bounds();
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("glue_steps ok\n");
    return 0;
}
