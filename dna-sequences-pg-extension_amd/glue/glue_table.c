/*
 * glue_table.c -- one answer per row of a table: its hits in a counted set (table_hits), its k-mer profile (table_profile),
 * and the rows that pass a screen on their hits (table_screen).
 */
#include "glue_core.h"

/* ------------------------------------------------------------------ per-row hits of a table in a counted set: table_hits */

struct TableHits {
    dnagpu_acc *set;                             /* the aggregate's accumulator (the aggregate outlives this object) */
    unsigned flags;
    uint64_t min_count, max_count;
    GsLife life;
    RowBatch b;                                  /* the open batch */
    uint64_t *rows, *hits, n_done, cap;          /* the answers of the rows of the batches looked up so far */
    uint64_t next;
    uint64_t tot_rows, tot_hits, tot_seqs_hit;
};

TableHits *table_hits_begin(CountKmersAgg *set, bool canonical, int64_t min_count, int64_t max_count)
{
    if (!set) {
        ereport_error("table_hits: the aggregate is missing");
        return NULL;
    }
    dnagpu_acc *acc = agg_flushed_acc(set, "table_hits");
    if (!acc)
        return NULL;
    TableHits *t = (TableHits *)glue_new(sizeof *t);
    if (!t)
        return NULL;
    t->set = acc;
    t->flags = canonical ? DNAGPU_HITS_CANONICAL : 0u;
    t->min_count = gs_lower_bound(min_count, 1);
    t->max_count = gs_upper_bound(max_count);
    return t;
}

/* the open batch: looked up on the device, its answers appended, emptied */
static bool th_flush(void *self)
{
    TableHits *t = (TableHits *)self;
    const uint64_t n = t->b.n_seqs;
    if (n == 0)
        return true;
    if (!glue_grow(COLS((void **)&t->rows, (void **)&t->hits), &t->cap, t->n_done + n))
        return false;
    bool ok = true;
    if (t->b.n_bases == 0) {                                              /* empty rows only: nothing to upload */
        memset(t->rows + t->n_done, 0, (size_t)n * sizeof(uint64_t));
        memset(t->hits + t->n_done, 0, (size_t)n * sizeof(uint64_t));
    } else {
        dnagpu_dna *d = NULL;
        dnagpu_seq_hits *h = NULL;
        uint64_t r = 0, c = 0, s = 0;
        ok = batch_upload(&t->b, &d) &&
             gpu_ok(dnagpu_table_hits(g_ctx, d, t->set, t->flags, t->min_count, t->max_count, 0, n, &h)) &&
             gpu_ok(dnagpu_seq_hits_read(g_ctx, h, 0, n, t->rows + t->n_done, t->hits + t->n_done, 0)) &&
             gpu_ok(dnagpu_seq_hits_totals(h, &r, &c, &s));
        if (ok) {
            t->tot_rows += r;
            t->tot_hits += c;
            t->tot_seqs_hit += s;
        }
        if (h)
            dnagpu_seq_hits_free(g_ctx, h);
        if (d)
            dnagpu_dna_free(g_ctx, d);
    }
    if (ok)
        t->n_done += n;
    rb_clear(&t->b);
    return ok;
}

bool table_hits_add(TableHits *t, const Dna *row)
{
    return stream_add(&t->life, &t->b, row, th_flush, t, "table_hits: row added after the first row was served or the scan failed");
}

bool table_hits_next(TableHits *t, int64_t *seq, int64_t *rows, int64_t *hits)
{
    if (!gs_serve(&t->life, th_flush, t) || t->next >= t->n_done)         /* (the first call: the last batch) */
        return false;
    const uint64_t i = t->next++;
    if (seq)
        *seq = (int64_t)i;
    if (rows)
        *rows = (int64_t)t->rows[i];
    if (hits)
        *hits = (int64_t)t->hits[i];
    return true;
}

void table_hits_totals(const TableHits *t, int64_t *rows, int64_t *hits, int64_t *seqs_hit)
{
    put3(rows, hits, seqs_hit, t->tot_rows, t->tot_hits, t->tot_seqs_hit);
}

bool table_hits_failed(const TableHits *t) { return t->life.failed; }

void table_hits_end(TableHits *t)
{
    if (!t)
        return;
    rb_free(&t->b);
    free(t->rows);
    free(t->hits);
    free(t);
}

/* ------------------------------------------------------------------ the k-mer profile of every row of a table: table_profile */

struct TableProfile {
    int k;
    unsigned flags;
    uint64_t width;                              /* 4^k */
    GsLife life;
    RowBatch b;                                  /* the open batch */
    uint64_t *rows, n_done, cap_rows;            /* the answers of the rows of the batches profiled so far */
    uint32_t *counts;                            /* n_done * width */
    uint64_t cap_counts;                         /* in 8-byte units (glue_grow's) */
    uint64_t next;
};

TableProfile *table_profile_begin(int k, bool canonical)
{
    if (!k_ok(k))
        return NULL;
    if (k > DNAGPU_PROFILE_MAX_K) {
        ereport_error("table_profile: a profile has 4^k columns and is offered for k <= %d", DNAGPU_PROFILE_MAX_K);
        return NULL;
    }
    TableProfile *t = (TableProfile *)glue_new(sizeof *t);
    if (!t)
        return NULL;
    t->k = k;
    t->flags = canonical ? DNAGPU_PROFILE_CANONICAL : 0u;
    t->width = dnagpu_profile_width(k);
    return t;
}

/* the open batch: profiled on the device, its answers appended, emptied */
static bool tp_flush(void *self)
{
    TableProfile *t = (TableProfile *)self;
    const uint64_t n = t->b.n_seqs;
    if (n == 0)
        return true;
    if (!glue_grow(COLS((void **)&t->rows), &t->cap_rows, t->n_done + n) ||
        !glue_grow(COLS((void **)&t->counts), &t->cap_counts, ((t->n_done + n) * t->width + 1) / 2))
        return false;
    uint32_t *counts = t->counts + t->n_done * t->width;
    bool ok = true;
    if (t->b.n_bases == 0) {                                              /* empty rows only: nothing to upload */
        memset(t->rows + t->n_done, 0, (size_t)n * sizeof(uint64_t));
        memset(counts, 0, (size_t)(n * t->width) * sizeof(uint32_t));
    } else {
        dnagpu_dna *d = NULL;
        ok = batch_upload(&t->b, &d) &&
             gpu_ok(dnagpu_table_profile(g_ctx, d, t->k, t->flags, 0, n, counts, t->rows + t->n_done, 0));
        if (d)
            dnagpu_dna_free(g_ctx, d);
    }
    if (ok)
        t->n_done += n;
    rb_clear(&t->b);
    return ok;
}

bool table_profile_add(TableProfile *t, const Dna *row)
{
    return stream_add(&t->life, &t->b, row, tp_flush, t, "table_profile: row added after the first row was served or the scan failed");
}

bool table_profile_next(TableProfile *t, int64_t *seq, int64_t *rows, int64_t *counts)
{
    if (!gs_serve(&t->life, tp_flush, t) || t->next >= t->n_done)         /* (the first call: the last batch) */
        return false;
    const uint64_t i = t->next++;
    if (seq)
        *seq = (int64_t)i;
    if (rows)
        *rows = (int64_t)t->rows[i];
    if (counts)
        for (uint64_t c = 0; c < t->width; c++)
            counts[c] = (int64_t)t->counts[i * t->width + c];
    return true;
}

int64_t table_profile_width(const TableProfile *t) { return (int64_t)t->width; }

bool table_profile_failed(const TableProfile *t) { return t->life.failed; }

void table_profile_end(TableProfile *t)
{
    if (!t)
        return;
    rb_free(&t->b);
    free(t->rows);
    free(t->counts);
    free(t);
}

/* ------------------------------------------------------------------ the rows of a table that pass a screen: table_screen */

_Static_assert(sizeof(Dna *) == sizeof(uint64_t), "glue_grow sizes the array of rows");

struct TableScreen {
    dnagpu_acc *set;                             /* the aggregate's accumulator (the aggregate outlives this object) */
    unsigned flags;
    uint64_t min_count, max_count, min_hits, max_hits, frac_num, frac_den;
    GsLife life;
    RowBatch b;                                  /* the open batch */
    uint64_t n_added;                            /* rows of the batches screened so far = the ordinal of the open batch's first row */
    uint64_t *seq, *rows, *hits;                 /* the passing rows of the batches screened so far ... */
    Dna **out;                                   /* ... and the rows themselves (NULL once handed out) */
    uint64_t cap, n_pass, next;
};

TableScreen *table_screen_begin(CountKmersAgg *set, bool canonical, int64_t min_count, int64_t max_count, int64_t min_hits,
                                int64_t max_hits, int64_t frac_num, int64_t frac_den)
{
    if (!set) {
        ereport_error("table_screen: the aggregate is missing");
        return NULL;
    }
    if (frac_den <= 0) {
        ereport_error("table_screen: the fraction's denominator must be positive");
        return NULL;
    }
    if (frac_den > (int64_t)UINT32_MAX || frac_num > (int64_t)UINT32_MAX) {
        ereport_error("table_screen: the terms of the fraction must be below 2^32");
        return NULL;
    }
    dnagpu_acc *acc = agg_flushed_acc(set, "table_screen");
    if (!acc)
        return NULL;
    TableScreen *t = (TableScreen *)glue_new(sizeof *t);
    if (!t)
        return NULL;
    t->set = acc;
    t->flags = canonical ? DNAGPU_HITS_CANONICAL : 0u;
    t->min_count = gs_lower_bound(min_count, 1);
    t->max_count = gs_upper_bound(max_count);
    t->min_hits = gs_lower_bound(min_hits, 0);
    t->max_hits = gs_upper_bound(max_hits);
    t->frac_num = gs_lower_bound(frac_num, 0);
    t->frac_den = (uint64_t)frac_den;
    return t;
}

static bool ts_grow(TableScreen *t, uint64_t more)
{
    return glue_grow(COLS((void **)&t->seq, (void **)&t->rows, (void **)&t->hits, (void **)&t->out), &t->cap, t->n_pass + more);
}

/* the n_out passing rows of the open batch: their ids, rows and hits from the select's device buffers (n entries apart), the
 * rows themselves from the taken table */
static bool ts_collect(TableScreen *t, const dnagpu_dna *taken, const uint64_t *dev, uint64_t n, uint64_t n_out)
{
    if (!ts_grow(t, n_out))
        return false;
    if (!gpu_ok(dnagpu_buffer_download(g_ctx, dev, n_out * 8, t->seq + t->n_pass)) ||
        !gpu_ok(dnagpu_buffer_download(g_ctx, dev + n, n_out * 8, t->rows + t->n_pass)) ||
        !gpu_ok(dnagpu_buffer_download(g_ctx, dev + 2 * n, n_out * 8, t->hits + t->n_pass)) ||
        !table_rows(taken, n_out, t->out + t->n_pass))
        return false;
    for (uint64_t i = 0; i < n_out; i++)
        t->seq[t->n_pass++] += t->n_added;                                /* the ordinal of the add call */
    return true;
}

/* the open batch: screened on the device, its passing rows appended, emptied */
static bool ts_flush(void *self)
{
    TableScreen *t = (TableScreen *)self;
    const uint64_t n = t->b.n_seqs;
    if (n == 0)
        return true;
    bool ok = true;
    if (t->b.n_bases == 0) {                                              /* empty rows only: no row, no hit, nothing to upload */
        if (t->min_hits == 0) {                                           /* (0 * den >= num * 0: the fraction asks nothing of them) */
            ok = ts_grow(t, n);
            for (uint64_t i = 0; ok && i < n; i++) {
                Dna *row = dna_cut(t->b.words, 0, 0);
                if (!row) {
                    ok = false;
                    break;
                }
                t->seq[t->n_pass] = t->n_added + i;
                t->rows[t->n_pass] = t->hits[t->n_pass] = 0;
                t->out[t->n_pass++] = row;
            }
        }
    } else {
        dnagpu_dna *d = NULL, *taken = NULL;
        dnagpu_seq_hits *h = NULL;
        void *dev = NULL;
        uint64_t n_out = 0;
        ok = batch_upload(&t->b, &d) &&
             gpu_ok(dnagpu_table_hits(g_ctx, d, t->set, t->flags, t->min_count, t->max_count, 0, n, &h)) &&
             gpu_ok(dnagpu_buffer_alloc(g_ctx, 3 * 8 * n, &dev));
        uint64_t *dv = (uint64_t *)dev;
        ok = ok && gpu_ok(dnagpu_seq_hits_select(g_ctx, h, t->min_hits, t->max_hits, t->frac_num, t->frac_den, dv, dv + n, dv + 2 * n,
                                                 n, &n_out, 1));
        if (ok && n_out > 0)
            ok = gpu_ok(dnagpu_dna_take(g_ctx, d, dv, NULL, n_out, 1, &taken)) && ts_collect(t, taken, dv, n, n_out);
        if (taken)
            dnagpu_dna_free(g_ctx, taken);
        if (dev)
            dnagpu_buffer_free(g_ctx, dev);
        if (h)
            dnagpu_seq_hits_free(g_ctx, h);
        if (d)
            dnagpu_dna_free(g_ctx, d);
    }
    t->n_added += n;
    rb_clear(&t->b);
    return ok;
}

bool table_screen_add(TableScreen *t, const Dna *row)
{
    return stream_add(&t->life, &t->b, row, ts_flush, t, "table_screen: row added after the first row was served or the scan failed");
}

bool table_screen_next(TableScreen *t, int64_t *seq, int64_t *rows, int64_t *hits, Dna **row)
{
    if (!gs_serve(&t->life, ts_flush, t) || t->next >= t->n_pass)         /* (the first call: the last batch) */
        return false;
    const uint64_t i = t->next++;
    if (seq)
        *seq = (int64_t)t->seq[i];
    if (rows)
        *rows = (int64_t)t->rows[i];
    if (hits)
        *hits = (int64_t)t->hits[i];
    if (row) {
        *row = t->out[i];                                                 /* the caller's from here on */
        t->out[i] = NULL;
    }
    return true;
}

bool table_screen_failed(const TableScreen *t) { return t->life.failed; }

void table_screen_end(TableScreen *t)
{
    if (!t)
        return;
    for (uint64_t i = 0; i < t->n_pass; i++)
        dna_free(t->out[i]);
    rb_free(&t->b);
    free(t->seq);
    free(t->rows);
    free(t->hits);
    free(t->out);
    free(t);
}
