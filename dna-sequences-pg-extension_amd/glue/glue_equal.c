/*
 * glue_equal.c -- equal rows of a table: the distinct rows with their copies (table_distinct), and the rows of one table
 * that another holds (table_match).  Either side is ONE resident table.
 */
#include "glue_core.h"

/* ------------------------------------------------------------------ equal rows: table_distinct, table_match */

#define TABLE_MAX_BASES 0xFFFFFFFFull            /* one resident table: dnagpu_dna_set_sequences' limit */

/* one side of table_distinct / table_match: the rows packed back to back, ONE resident table when uploaded */
typedef struct EqSide {
    RowBatch b;
    dnagpu_dna *dev;
} EqSide;

/* (no batch is flushed: the whole side is one table, so the add policy has no part in it) */
static bool eq_side_add(GsLife *l, EqSide *s, const Dna *row, const char *who)
{
    if (!gs_may_add(l)) {
        ereport_error("%s: row added after the first row was served or the scan failed", who);
        return false;
    }
    if (row->length > TABLE_MAX_BASES - s->b.n_bases)
        ereport_error("%s: the rows hold more than 4294967295 bases (2^32 - 1), the limit of one resident table", who);
    else if (!rb_append(&s->b, row->bit_sequence, row->length))
        ereport_error("out of memory");
    else
        return true;
    l->failed = true;
    return false;
}

static void eq_side_free(EqSide *s)
{
    if (s->dev)
        dnagpu_dna_free(g_ctx, s->dev);
    rb_free(&s->b);
    s->dev = NULL;
}

struct TableDistinct {
    EqSide rows;
    GsLife life;
    uint64_t *seq, *copies, n_out, next;         /* the representatives, ascending */
};

TableDistinct *table_distinct_begin(void) { return (TableDistinct *)glue_new(sizeof(TableDistinct)); }

bool table_distinct_add(TableDistinct *t, const Dna *row) { return eq_side_add(&t->life, &t->rows, row, "table_distinct"); }

/* the whole table: classes on the device, the representatives read back */
static bool td_run(void *self)
{
    TableDistinct *t = (TableDistinct *)self;
    if (t->rows.b.n_seqs == 0)
        return true;
    dnagpu_seq_classes *c = NULL;
    uint64_t n = 0;
    bool ok = batch_upload(&t->rows.b, &t->rows.dev) && gpu_ok(dnagpu_table_classes(g_ctx, t->rows.dev, &c));
    if (ok) {
        n = dnagpu_seq_classes_distinct(c);
        ok = cols_alloc(n ? n : 1, &t->seq, &t->copies, NULL);
    }
    ok = ok && gpu_ok(dnagpu_seq_classes_select(g_ctx, c, 1, UINT64_MAX, t->seq, t->copies, n, &t->n_out, 0));
    if (ok && t->n_out != n) {
        ereport_error("table_distinct: the select returned %llu of %llu classes", (unsigned long long)t->n_out, (unsigned long long)n);
        ok = false;
    }
    if (c)
        dnagpu_seq_classes_free(g_ctx, c);
    return ok;
}

bool table_distinct_next(TableDistinct *t, int64_t *seq, int64_t *copies)
{
    if (!gs_serve(&t->life, td_run, t) || t->next >= t->n_out)
        return false;
    const uint64_t i = t->next++;
    if (seq)
        *seq = (int64_t)t->seq[i];
    if (copies)
        *copies = (int64_t)t->copies[i];
    return true;
}

bool table_distinct_failed(const TableDistinct *t) { return t->life.failed; }

void table_distinct_end(TableDistinct *t)
{
    if (!t)
        return;
    eq_side_free(&t->rows);
    free(t->seq);
    free(t->copies);
    free(t);
}

struct TableMatch {
    EqSide build, probe;
    GsLife life;
    uint64_t *match, *copies, next;              /* one entry per probe row */
};

TableMatch *table_match_begin(void) { return (TableMatch *)glue_new(sizeof(TableMatch)); }

bool table_match_add_build(TableMatch *t, const Dna *row) { return eq_side_add(&t->life, &t->build, row, "table_match"); }
bool table_match_add_probe(TableMatch *t, const Dna *row) { return eq_side_add(&t->life, &t->probe, row, "table_match"); }

static bool tm_run(void *self)
{
    TableMatch *t = (TableMatch *)self;
    const uint64_t np = t->probe.b.n_seqs;
    if (np == 0 || t->build.b.n_seqs == 0) {       /* nothing to ask, or nothing to find: no row */
        t->probe.b.n_seqs = 0;
        return true;
    }
    if (!cols_alloc(np, &t->match, &t->copies, NULL))
        return false;
    dnagpu_seq_classes *c = NULL;
    const bool ok = batch_upload(&t->build.b, &t->build.dev) && batch_upload(&t->probe.b, &t->probe.dev) &&
                    gpu_ok(dnagpu_table_classes(g_ctx, t->build.dev, &c)) &&
                    gpu_ok(dnagpu_table_match(g_ctx, c, t->probe.dev, 0, np, t->match, t->copies, NULL, 0));
    if (c)
        dnagpu_seq_classes_free(g_ctx, c);
    return ok;
}

bool table_match_next(TableMatch *t, int64_t *probe_seq, int64_t *build_seq, int64_t *copies)
{
    if (!gs_serve(&t->life, tm_run, t))
        return false;
    while (t->next < t->probe.b.n_seqs && t->match[t->next] == DNAGPU_MATCH_NONE)
        t->next++;                               /* (an inner join: a probe row without a partner gives no row) */
    if (t->next >= t->probe.b.n_seqs)
        return false;
    const uint64_t i = t->next++;
    if (probe_seq)
        *probe_seq = (int64_t)i;
    if (build_seq)
        *build_seq = (int64_t)t->match[i];
    if (copies)
        *copies = (int64_t)t->copies[i];
    return true;
}

bool table_match_failed(const TableMatch *t) { return t->life.failed; }

void table_match_end(TableMatch *t)
{
    if (!t)
        return;
    eq_side_free(&t->build);
    eq_side_free(&t->probe);
    free(t->match);
    free(t->copies);
    free(t);
}
