/*
 * glue_kmers.c -- the k-mers as rows: generate_kmers over one sequence and table_kmers over the rows of a table, each with
 * the WHERE forms fused into the sweep.
 */
#include "glue_core.h"

/* ------------------------------------------------------------------ generate_kmers */

#define GK_WINDOW ((uint64_t)1 << 22)     /* rows fetched from the GPU per refill (32 MiB of keys) */

struct GenerateKmers {
    Dna *dna;
    int k;
    uint64_t total;        /* max_calls, dna.c:781 */
    uint64_t *keys;        /* host window */
    GsWindow win;          /* unfiltered: win.next = call_cntr */
    /* filtered mode */
    bool filtered;
    dnagpu_filter filter;
    uint64_t scan_pos;     /* next unscanned row of generate_kmers */
    uint64_t win_count, win_used;
    bool failed;           /* an ERROR was raised: the statement is aborted */
};

GenerateKmers *generate_kmers_begin(Dna *dna, int k)
{
    uint64_t total = 0;
    if (!gpu_ok(dnagpu_kmer_count(dna->length, k, &total)))              /* dna.c:771-773 */
        return NULL;
    GenerateKmers *g = (GenerateKmers *)glue_new(sizeof *g);
    if (!g)
        return NULL;
    g->dna = dna;
    g->k = k;
    g->total = total;
    g->keys = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(total < GK_WINDOW ? (total ? total : 1) : GK_WINDOW));
    if (!g->keys) {
        free(g);
        ereport_error("out of memory");
        return NULL;
    }
    return g;
}

GenerateKmers *generate_kmers_where_begin(Dna *dna, int k, char op, const Kmer *rhs, const Qkmer *rhs_pattern)
{
    GenerateKmers *g = generate_kmers_begin(dna, k);
    if (!g)
        return NULL;
    g->filtered = true;
    if (!filter_from_op(&g->filter, op, rhs, rhs_pattern)) {
        generate_kmers_end(g);
        return NULL;
    }
    return g;
}

bool generate_kmers_next(GenerateKmers *g, Kmer *out)
{
    if (!g->filtered) {
        if (g->win.next >= g->total)
            return false;                                                 /* SRF_RETURN_DONE */
        if (!gs_win_has(&g->win)) {
            dnagpu_dna *d = device_dna(g->dna);
            const uint64_t n = gs_refill(g->total, g->win.next, GK_WINDOW);
            if (!d || !gpu_ok(dnagpu_generate_kmers(g_ctx, d, g->k, g->win.next, n, g->keys, 0))) {
                g->failed = true;
                return false;
            }
            gs_win_filled(&g->win, n);
        }
        out->length = g->k;
        out->bit_sequence = g->keys[gs_win_at(&g->win)];
        g->win.next++;
        return true;
    }
    /* filtered: refill with the next window of source rows until one has matches */
    while (g->win_used >= g->win_count) {
        if (g->scan_pos >= g->total)
            return false;
        dnagpu_dna *d = device_dna(g->dna);
        const uint64_t n = gs_refill(g->total, g->scan_pos, GK_WINDOW);
        uint64_t n_out = 0;
        if (!d || !gpu_ok(dnagpu_generate_kmers_filtered(g_ctx, d, g->k, &g->filter, g->scan_pos, n, g->keys,
                                                          NULL, GK_WINDOW, &n_out, 0))) {
            g->scan_pos = g->total;                                       /* the ERROR aborts the statement */
            g->failed = true;
            return false;
        }
        g->scan_pos += n;
        g->win_count = n_out;
        g->win_used = 0;
    }
    out->length = g->k;
    out->bit_sequence = g->keys[g->win_used++];
    return true;
}

bool generate_kmers_failed(const GenerateKmers *g) { return g->failed; }

void generate_kmers_end(GenerateKmers *g)
{
    if (!g)
        return;
    free(g->keys);
    free(g);
}

/* ------------------------------------------------------------------ the ROWS of a table: kmers_of_table */

#define TK_WINDOW ((uint64_t)1 << 20)     /* stream rows per refill: a window never holds more table rows than stream rows */

typedef struct TableBatch {
    RowBatch b;
    uint64_t first_seq;                          /* ordinal of the batch's first row in the table */
} TableBatch;

struct TableKmers {
    int k;
    bool filtered, open;                         /* open: the last batch still takes rows */
    GsLife life;
    dnagpu_filter filter;
    TableBatch *batches;
    uint64_t n_batches, cap_batches, n_rows;     /* n_rows: add calls so far */
    /* the scan */
    uint64_t cur;                                /* batch being read */
    dnagpu_dna *dev;                             /* ... resident, with its sequence set */
    uint64_t scan_pos, scan_total;               /* stream rows of the batch: next unscanned, all */
    uint64_t *keys, *seq, *pos, win_count, win_used;
};

TableKmers *table_kmers_begin(int k, char op, const Kmer *rhs, const Qkmer *rhs_pattern)
{
    if (!k_ok(k))
        return NULL;
    TableKmers *t = (TableKmers *)glue_new(sizeof *t);
    if (!t)
        return NULL;
    t->k = k;
    t->filtered = op != 0;
    if (op != 0 && !filter_from_op(&t->filter, op, rhs, rhs_pattern)) {
        free(t);
        return NULL;
    }
    return t;
}

/* (the batches are kept, not flushed: the add policy's two tests without its flushes) */
bool table_kmers_add(TableKmers *t, const Dna *row)
{
    if (!gs_may_add(&t->life)) {
        ereport_error("table_kmers: row added after the first row was served or the scan failed");
        return false;
    }
    TableBatch *b = t->open ? &t->batches[t->n_batches - 1] : NULL;
    if (b && rb_spills(&b->b, row->length, g_agg_flush_bases))                  /* a long row: a batch of its own */
        b = NULL;
    if (!b) {
        if (t->n_batches == t->cap_batches) {
            const uint64_t c = t->cap_batches ? 2 * t->cap_batches : 16;
            TableBatch *q = (TableBatch *)realloc(t->batches, (size_t)c * sizeof *q);
            if (!q) {
                ereport_error("out of memory");
                t->life.failed = true;
                return false;
            }
            t->batches = q;
            t->cap_batches = c;
        }
        b = &t->batches[t->n_batches++];
        memset(b, 0, sizeof *b);
        b->first_seq = t->n_rows;
    }
    if (!rb_append(&b->b, row->bit_sequence, row->length)) {
        ereport_error("out of memory");
        t->life.failed = true;
        return false;
    }
    t->n_rows++;
    t->open = !rb_full(&b->b, g_agg_flush_bases);
    return true;
}

static void tk_drop_device(TableKmers *t)
{
    if (t->dev)
        dnagpu_dna_free(g_ctx, t->dev);
    t->dev = NULL;
}

/* batch t->cur onto the device with its boundaries; false = ERROR */
static bool tk_open_batch(TableKmers *t)
{
    const RowBatch *b = &t->batches[t->cur].b;
    t->scan_pos = 0;
    t->scan_total = b->n_bases >= (uint64_t)t->k ? b->n_bases - (uint64_t)t->k + 1 : 0;
    if (t->scan_total == 0)
        return true;
    return batch_upload(b, &t->dev);
}

/* the first _next: the window buffers, the first batch */
static bool tk_start(void *self)
{
    TableKmers *t = (TableKmers *)self;
    if (!cols_alloc(TK_WINDOW, &t->keys, &t->seq, &t->pos))
        return false;
    return !t->n_batches || tk_open_batch(t);
}

bool table_kmers_next(TableKmers *t, int64_t *seq, int64_t *pos, Kmer *out)
{
    if (!gs_serve(&t->life, tk_start, t))
        return false;
    while (t->win_used >= t->win_count) {                                 /* the next window with rows */
        if (t->cur >= t->n_batches)
            return false;
        if (t->scan_pos >= t->scan_total) {                               /* the next batch */
            tk_drop_device(t);
            if (++t->cur >= t->n_batches)
                return false;
            if (!tk_open_batch(t)) {
                t->life.failed = true;
                return false;
            }
            continue;
        }
        const uint64_t n = gs_refill(t->scan_total, t->scan_pos, TK_WINDOW);
        uint64_t n_out = 0;
        if (!gpu_ok(dnagpu_generate_kmers_table(g_ctx, t->dev, t->k, t->filtered ? &t->filter : NULL, t->scan_pos, n, t->keys,
                                                t->seq, t->pos, TK_WINDOW, &n_out, 0))) {
            t->life.failed = true;                                        /* the ERROR aborts the statement */
            return false;
        }
        t->scan_pos += n;
        t->win_count = n_out;
        t->win_used = 0;
    }
    const uint64_t i = t->win_used++;
    if (seq)
        *seq = (int64_t)(t->batches[t->cur].first_seq + t->seq[i]);
    if (pos)
        *pos = (int64_t)t->pos[i];
    out->length = t->k;
    out->bit_sequence = t->keys[i];
    return true;
}

bool table_kmers_failed(const TableKmers *t) { return t->life.failed; }

void table_kmers_end(TableKmers *t)
{
    if (!t)
        return;
    tk_drop_device(t);
    for (uint64_t i = 0; i < t->n_batches; i++)
        rb_free(&t->batches[i].b);
    free(t->batches);
    free(t->keys);
    free(t->seq);
    free(t->pos);
    free(t);
}
