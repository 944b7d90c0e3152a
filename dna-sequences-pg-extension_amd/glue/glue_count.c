/*
 * glue_count.c -- GROUP BY kmer: count_kmers over one sequence, the count over a table of rows as an aggregate, and the join
 * of two aggregates on the k-mer.
 */
#include "glue_core.h"

/* ------------------------------------------------------------------ count_kmers */

#define CK_WINDOW ((uint64_t)1 << 21)

/* one histogram per rank (one rank unless dna_glue_set_gpus asked for more); rank order = ascending key ranges */
struct CountKmers {
    int k;
    int n_ranks, rank;                       /* rank = the histogram rows are being served from */
    dnagpu_hist *hist[CK_MAX_RANKS];
    dnagpu_ctx *hctx[CK_MAX_RANKS];
    dnagpu_ranking *ranking;                 /* count_kmers_ordered_begin: the rows come from it, the histogram is gone */
    uint64_t rank_distinct;
    GsWindow win;                            /* cursor inside hist[rank] */
    uint64_t distinct;
    uint64_t *keys, *counts;
    uint64_t total, unique;
};

/* single: one histogram on this backend's device whatever dna_glue_set_gpus asked for (count_kmers_top_begin) */
static CountKmers *ck_begin(Dna *dna, int k, bool single)
{
    uint64_t n_rows = 0;
    if (!gpu_ok(dnagpu_kmer_count(dna->length, k, &n_rows)))
        return NULL;
    CountKmers *c = (CountKmers *)glue_new(sizeof *c);
    if (!c)
        return NULL;
    c->k = k;
    bool ok;
    if (g_n_gpus > 1 && !single) {
        /* the sequence goes to the ranks as contiguous word chunks; one all-gather + per-rank owner counts */
        dnagpu_multi *m = multi();
        dnagpu_multi_dna *md = NULL;
        ok = m && gpu_ok(dnagpu_multi_dna_upload(m, dna->bit_sequence, dna->length, &md));
        if (ok) {
            c->n_ranks = g_n_gpus;
            for (int r = 0; r < c->n_ranks; r++)
                c->hctx[r] = dnagpu_multi_ctx(m, r);
            ok = gpu_ok(dnagpu_count_multi_unordered(m, md, k, 0, n_rows, c->hist));   /* GROUP BY promises no order */
            dnagpu_multi_dna_free(m, md);
        }
    } else {
        dnagpu_dna *d = device_dna(dna);
        ok = d != NULL;
        if (ok) {
            c->n_ranks = 1;
            c->hctx[0] = g_ctx;
            /* GROUP BY promises no order (test.sql:95-104): the entry point that may partition by super-k-mers */
            ok = gpu_ok(dnagpu_count_kmers_unordered(g_ctx, d, k, 0, n_rows, &c->hist[0]));
        }
    }
    for (int r = 0; ok && r < c->n_ranks; r++) {
        uint64_t t = 0, u = 0, checksum;
        ok = gpu_ok(dnagpu_hist_summary(c->hctx[r], c->hist[r], &t, &u, &checksum));
        c->total += t;
        c->unique += u;
        c->distinct += dnagpu_hist_distinct(c->hist[r]);
    }
    if (!ok) {
        count_kmers_end(c);
        return NULL;
    }
    c->rank = 0;
    c->rank_distinct = dnagpu_hist_distinct(c->hist[0]);
    if (!cols_alloc(CK_WINDOW, &c->keys, &c->counts, NULL)) {
        count_kmers_end(c);
        return NULL;
    }
    return c;
}

CountKmers *count_kmers_begin(Dna *dna, int k) { return ck_begin(dna, k, false); }

static bool top_limit_ok(const char *who, int64_t limit)
{
    if (limit >= 1 && limit <= (int64_t)DNAGPU_TOP_MAX)
        return true;
    ereport_error("%s: limit must be between 1 and %u", who, (unsigned)DNAGPU_TOP_MAX);
    return false;
}

/* ... GROUP BY k.kmer ORDER BY count(*) DESC LIMIT limit (test.sql:95): the rows are chosen and sorted on the device
 * (dnagpu_hist_top) and served from the window buffers, which hold DNAGPU_TOP_MAX rows */
CountKmers *count_kmers_top_begin(Dna *dna, int k, int64_t limit)
{
    if (!top_limit_ok("count_kmers_top", limit))
        return NULL;
    CountKmers *c = ck_begin(dna, k, true);
    if (!c)
        return NULL;
    uint64_t n = 0;
    if (!gpu_ok(dnagpu_hist_top(c->hctx[0], c->hist[0], (uint64_t)limit, c->keys, c->counts, &n, 0))) {
        count_kmers_end(c);
        return NULL;
    }
    c->rank_distinct = n;                        /* _next serves rows [0, n) of the one window */
    gs_win_filled(&c->win, n);
    return c;
}

/* ... GROUP BY k.kmer ORDER BY count(*) [DESC] with no LIMIT: every group ranked on the device (dnagpu_hist_rank); the
 * histogram is freed, count_kmers_next reads the ranking window by window */
#define CK_RANK_WINDOW ((uint64_t)1 << 20)
CountKmers *count_kmers_ordered_begin(Dna *dna, int k, bool descending)
{
    CountKmers *c = ck_begin(dna, k, true);
    if (!c)
        return NULL;
    if (!gpu_ok(dnagpu_hist_rank(c->hctx[0], c->hist[0], descending ? DNAGPU_ORDER_COUNT_DESC : DNAGPU_ORDER_COUNT_ASC,
                                 &c->ranking))) {
        count_kmers_end(c);
        return NULL;
    }
    dnagpu_hist_free(c->hctx[0], c->hist[0]);
    c->hist[0] = NULL;
    c->rank_distinct = dnagpu_ranking_rows(c->ranking);
    return c;
}

bool count_kmers_spectrum(const CountKmers *c, int64_t *bins, int n_bins)
{
    if (!c || !bins || n_bins < 1 || (uint64_t)n_bins > DNAGPU_SPECTRUM_MAX_BINS) {
        ereport_error("count_kmers_spectrum: n_bins must be between 1 and %u", (unsigned)DNAGPU_SPECTRUM_MAX_BINS);
        return false;
    }
    uint64_t *part = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)n_bins);
    if (!part) {
        ereport_error("out of memory");
        return false;
    }
    bool ok = true;
    memset(bins, 0, sizeof(int64_t) * (size_t)n_bins);
    for (int r = 0; ok && r < c->n_ranks; r++) {     /* the ranks' groups are disjoint: their spectra add up */
        ok = gpu_ok(dnagpu_hist_spectrum(c->hctx[r], c->hist[r], (uint64_t)n_bins, part));
        for (int b = 0; ok && b < n_bins; b++)
            bins[b] += (int64_t)part[b];
    }
    free(part);
    return ok;
}

/* rows a refill of a count window asks for: a ranking is read in smaller windows */
static uint64_t ck_refill(uint64_t total, uint64_t next, bool ranking)
{
    return gs_refill(total, next, ranking ? CK_RANK_WINDOW : CK_WINDOW);
}

bool count_kmers_next(CountKmers *c, Kmer *kmer, int64_t *count)
{
    while (c->win.next >= c->rank_distinct) {        /* this rank's key range is served: on to the next one */
        if (c->rank + 1 >= c->n_ranks)
            return false;
        c->rank++;
        c->rank_distinct = dnagpu_hist_distinct(c->hist[c->rank]);
        c->win = (GsWindow){0, 0, 0};
    }
    if (!gs_win_has(&c->win)) {
        const uint64_t n = ck_refill(c->rank_distinct, c->win.next, c->ranking != NULL);
        if (!gpu_ok(c->ranking ? dnagpu_ranking_read(c->hctx[0], c->ranking, c->win.next, n, c->keys, c->counts, 0)
                               : dnagpu_hist_download(c->hctx[c->rank], c->hist[c->rank], c->win.next, n, c->keys, c->counts)))
            return false;
        gs_win_filled(&c->win, n);
    }
    kmer->length = c->k;
    kmer->bit_sequence = c->keys[gs_win_at(&c->win)];
    *count = (int64_t)c->counts[gs_win_at(&c->win)];
    c->win.next++;
    return true;
}

void count_kmers_totals(const CountKmers *c, int64_t *total, int64_t *distinct, int64_t *unique)
{
    put3(total, distinct, unique, c->total, c->distinct, c->unique);
}

void count_kmers_end(CountKmers *c)
{
    if (!c)
        return;
    for (int r = 0; r < c->n_ranks; r++)
        if (c->hist[r])
            dnagpu_hist_free(c->hctx[r], c->hist[r]);
    if (c->ranking)
        dnagpu_ranking_free(c->hctx[0], c->ranking);
    free(c->keys);
    free(c->counts);
    free(c);
}

/* ------------------------------------------------------------------ the count over a TABLE of rows as an aggregate */

struct CountKmersAgg {
    int k;
    bool canonical;                              /* count_kmers_agg_begin_canonical: the flush is dnagpu_acc_add_canonical */
    dnagpu_acc *acc;                             /* created on the first flush (the GPU context is lazy) */
    RowBatch b;                                  /* the open batch */
    GsLife life;                                 /* started: the aggregate has finished */
    uint64_t top_limit;                          /* count_kmers_agg_top: serve only the first rows of ORDER BY count(*) DESC */
    int order;                                   /* count_kmers_agg_order: 0 = none, 1 = count descending, 2 = ascending */
    dnagpu_ranking *ranking;                     /* ... every group in that order, made when the aggregate finishes */
    uint64_t serve_n;                            /* rows _next serves: distinct, or the rows of the top */
    uint64_t distinct, total, unique;
    GsWindow win;
    uint64_t *keys, *counts;
};

CountKmersAgg *count_kmers_agg_begin(int k)
{
    if (!k_ok(k))
        return NULL;
    CountKmersAgg *a = (CountKmersAgg *)glue_new(sizeof *a);
    if (a)
        a->k = k;
    return a;
}

CountKmersAgg *count_kmers_agg_begin_canonical(int k)
{
    CountKmersAgg *a = count_kmers_agg_begin(k);
    if (a)
        a->canonical = true;
    return a;
}

/* the batch so far: counted, added into the accumulator, emptied */
static bool agg_flush(void *self)
{
    CountKmersAgg *a = (CountKmersAgg *)self;
    bool ok = true;
    if (a->b.n_bases > 0) {
        dnagpu_dna *d = NULL;
        dnagpu_hist *h = NULL;
        ok = ctx() != NULL && (a->acc || gpu_ok(dnagpu_acc_create(g_ctx, a->k, &a->acc))) &&
             gpu_ok(dnagpu_dna_upload(g_ctx, a->b.words, a->b.n_bases, &d)) &&
             gpu_ok(dnagpu_count_kmers_batch(g_ctx, d, a->b.starts, a->b.n_seqs, a->k, &h)) &&
             gpu_ok(a->canonical ? dnagpu_acc_add_canonical(g_ctx, a->acc, h) : dnagpu_acc_add(g_ctx, a->acc, h));
        if (h)
            dnagpu_hist_free(g_ctx, h);
        if (d)
            dnagpu_dna_free(g_ctx, d);
    }
    rb_clear(&a->b);
    return ok;
}

bool count_kmers_agg_add(CountKmersAgg *a, const Dna *row)
{
    return stream_add(&a->life, &a->b, row, agg_flush, a, "count_kmers_agg: row added after the aggregate finished or failed");
}

/* FINALFUNC's first step: the last batch, then the totals over the accumulated groups */
static bool agg_finish(void *self)
{
    CountKmersAgg *a = (CountKmersAgg *)self;
    if (!agg_flush(a))
        return false;
    if (a->acc) {
        uint64_t t = 0, u = 0, checksum;
        if (!gpu_ok(dnagpu_acc_summary(g_ctx, a->acc, &t, &u, &checksum)))
            return false;
        a->total = t;
        a->unique = u;
        a->distinct = dnagpu_acc_distinct(a->acc);
    }
    if (!cols_alloc(CK_WINDOW, &a->keys, &a->counts, NULL))
        return false;
    a->serve_n = a->distinct;
    if (a->top_limit && a->acc) {                /* chosen and sorted on the device; the window buffers hold DNAGPU_TOP_MAX rows */
        uint64_t n = 0;
        if (!gpu_ok(dnagpu_acc_top(g_ctx, a->acc, a->top_limit, a->keys, a->counts, &n, 0)))
            return false;
        a->serve_n = n;
        gs_win_filled(&a->win, n);
    }
    return !(a->order && a->acc) ||
           gpu_ok(dnagpu_acc_rank(g_ctx, a->acc, a->order == 1 ? DNAGPU_ORDER_COUNT_DESC : DNAGPU_ORDER_COUNT_ASC, &a->ranking));
}

bool count_kmers_agg_order(CountKmersAgg *a, bool descending)
{
    if (!gs_may_add(&a->life)) {
        ereport_error("count_kmers_agg_order: called after the first row was served or the aggregate failed");
        return false;
    }
    a->order = descending ? 1 : 2;
    a->top_limit = 0;
    return true;
}

bool count_kmers_agg_top(CountKmersAgg *a, int64_t limit)
{
    if (!top_limit_ok("count_kmers_agg_top", limit))
        return false;
    if (!gs_may_add(&a->life)) {
        ereport_error("count_kmers_agg_top: called after the first row was served or the aggregate failed");
        return false;
    }
    a->top_limit = (uint64_t)limit;
    a->order = 0;
    return true;
}

bool count_kmers_agg_next(CountKmersAgg *a, Kmer *kmer, int64_t *count)
{
    if (!gs_serve(&a->life, agg_finish, a) || a->win.next >= a->serve_n)
        return false;
    if (!gs_win_has(&a->win)) {
        const uint64_t n = ck_refill(a->serve_n, a->win.next, a->ranking != NULL);
        if (!gpu_ok(a->ranking ? dnagpu_ranking_read(g_ctx, a->ranking, a->win.next, n, a->keys, a->counts, 0)
                               : dnagpu_acc_download(g_ctx, a->acc, a->win.next, n, a->keys, a->counts))) {
            a->life.failed = true;
            return false;
        }
        gs_win_filled(&a->win, n);
    }
    kmer->length = a->k;
    kmer->bit_sequence = a->keys[gs_win_at(&a->win)];
    *count = (int64_t)a->counts[gs_win_at(&a->win)];
    a->win.next++;
    return true;
}

bool count_kmers_agg_failed(const CountKmersAgg *a) { return a->life.failed; }

void count_kmers_agg_totals(const CountKmersAgg *a, int64_t *total, int64_t *distinct, int64_t *unique)
{
    put3(total, distinct, unique, a->total, a->distinct, a->unique);
}

void count_kmers_agg_end(CountKmersAgg *a)
{
    if (!a)
        return;
    if (a->ranking)
        dnagpu_ranking_free(g_ctx, a->ranking);
    if (a->acc)
        dnagpu_acc_free(g_ctx, a->acc);
    rb_free(&a->b);
    free(a->keys);
    free(a->counts);
    free(a);
}

/* the aggregate's accumulator with every row so far in it (an aggregate that saw no row gets an empty one) */
dnagpu_acc *agg_flushed_acc(CountKmersAgg *a, const char *who)
{
    if (a->life.failed) {
        ereport_error("%s: an aggregate has failed", who);
        return NULL;
    }
    if (!agg_flush(a)) {
        a->life.failed = true;
        return NULL;
    }
    if (!a->acc && (!ctx() || !gpu_ok(dnagpu_acc_create(g_ctx, a->k, &a->acc))))
        return NULL;
    return a->acc;
}

/* ------------------------------------------------------------------ the join of two aggregates on the k-mer */

#define CK_JOIN_WINDOW ((uint64_t)1 << 20)

struct CountKmersJoin {
    int k;
    bool failed;
    dnagpu_join_stats stats;
    uint64_t rows;                               /* rows _next serves */
    uint64_t *dev[3];                            /* keys, count_left, count_right: the whole result, on the device */
    uint64_t *win[3];                            /* the window being served, on the host */
    GsWindow at;
};

CountKmersJoin *count_kmers_join_begin(CountKmersAgg *left, CountKmersAgg *right, char kind)
{
    const int kd = kind == 'i' ? DNAGPU_JOIN_INNER : kind == 'a' ? DNAGPU_JOIN_ANTI : kind == 'l' ? DNAGPU_JOIN_LEFT : -1;
    if (kd < 0) {
        ereport_error("count_kmers_join: unknown kind '%c' (expected 'i', 'a' or 'l')", kind);
        return NULL;
    }
    if (!left || !right) {
        ereport_error("count_kmers_join: an aggregate is missing");
        return NULL;
    }
    if (left->k != right->k) {
        ereport_error("count_kmers_join: the two sides count kmers of different lengths (%d and %d)", left->k, right->k);
        return NULL;
    }
    dnagpu_acc *la = agg_flushed_acc(left, "count_kmers_join");
    dnagpu_acc *ra = la ? agg_flushed_acc(right, "count_kmers_join") : NULL;
    if (!la || !ra)
        return NULL;
    CountKmersJoin *j = (CountKmersJoin *)glue_new(sizeof *j);
    if (!j)
        return NULL;
    j->k = left->k;
    /* the statistics size the device buffers; the second call fills them */
    uint64_t n = 0;
    bool ok = gpu_ok(dnagpu_acc_join(g_ctx, la, ra, kd, NULL, NULL, NULL, 0, &n, &j->stats, 0));
    if (ok && n > 0) {
        for (int i = 0; ok && i < 3; i++) {
            void *d = NULL;
            ok = gpu_ok(dnagpu_buffer_alloc(g_ctx, n * sizeof(uint64_t), &d));
            j->dev[i] = (uint64_t *)d;
            if (ok) {
                const uint64_t w = n < CK_JOIN_WINDOW ? n : CK_JOIN_WINDOW;
                j->win[i] = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)w);
                if (!j->win[i]) {
                    ereport_error("out of memory");
                    ok = false;
                }
            }
        }
        uint64_t got = 0;
        ok = ok && gpu_ok(dnagpu_acc_join(g_ctx, la, ra, kd, j->dev[0], j->dev[1], j->dev[2], n, &got, NULL, 1));
        if (ok && got != n) {
            ereport_error("count_kmers_join: %llu rows, then %llu", (unsigned long long)n, (unsigned long long)got);
            ok = false;
        }
    }
    if (!ok) {
        count_kmers_join_end(j);
        return NULL;
    }
    j->rows = n;
    return j;
}

bool count_kmers_join_next(CountKmersJoin *j, Kmer *kmer, int64_t *count_left, int64_t *count_right)
{
    if (j->failed || j->at.next >= j->rows)
        return false;
    if (!gs_win_has(&j->at)) {
        const uint64_t n = gs_refill(j->rows, j->at.next, CK_JOIN_WINDOW);
        for (int i = 0; i < 3; i++)
            if (!gpu_ok(dnagpu_buffer_download(g_ctx, j->dev[i] + j->at.next, n * sizeof(uint64_t), j->win[i]))) {
                j->failed = true;
                return false;
            }
        gs_win_filled(&j->at, n);
    }
    const uint64_t at = gs_win_at(&j->at);
    kmer->length = j->k;
    kmer->bit_sequence = j->win[0][at];
    *count_left = (int64_t)j->win[1][at];
    *count_right = (int64_t)j->win[2][at];
    j->at.next++;
    return true;
}

bool count_kmers_join_failed(const CountKmersJoin *j) { return j->failed; }

void count_kmers_join_stats(const CountKmersJoin *j, int64_t *rows, int64_t *sum_left, int64_t *sum_right, int64_t *sum_min)
{
    put3(rows, sum_left, sum_right, j->stats.rows, j->stats.sum_left, j->stats.sum_right);
    if (sum_min) *sum_min = (int64_t)j->stats.sum_min;
}

void count_kmers_join_end(CountKmersJoin *j)
{
    if (!j)
        return;
    for (int i = 0; i < 3; i++) {
        if (j->dev[i])
            dnagpu_buffer_free(g_ctx, j->dev[i]);
        free(j->win[i]);
    }
    free(j);
}
