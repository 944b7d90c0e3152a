/*
 * glue_copy_to.c -- COPY ... TO a text file: the rows as lines, FASTA or FASTQ (copy_dna_to), FASTQ with the rows' own
 * quality lines (copy_reads_to).
 */
#include "glue_core.h"

/* ------------------------------------------------------------------ COPY ... TO a text file: copy_dna_to */

struct CopyDnaTo {
    int format;
    uint32_t line_width;
    bool crlf;
    GsLife life;                                 /* started: the COPY has finished */
    RowBatch b;                                  /* the open batch */
    uint64_t limit_bases, chunk;                 /* a batch is flushed at limit_bases; a chunk of text has at most `chunk` bytes */
    uint64_t rows_before;                        /* rows of the flushed batches: the first name of the next one */
    char **text;                                 /* the chunks of text formed and not yet served (NULL once served and freed) */
    uint64_t *text_len;
    uint64_t cap_text, n_text, next;
    /* copy_reads_to_begin: FASTQ whose quality lines are the rows' own */
    bool reads;
    char *qual;                                  /* the quality bytes of the open batch, one per base */
    uint64_t cap_qual;
    /* _add_named: the headers are the rows' own names */
    int named;                                   /* 0: no row yet, 1: every row comes with its name, 2: none does */
    char *names;                                 /* the names of the open batch, back to back */
    uint64_t *name_off;                          /* name_off[0 .. b.n_seqs]: where each begins */
    uint64_t cap_names, cap_name_off, n_name_bytes;
};

CopyDnaTo *copy_dna_to_begin(int format, uint32_t line_width, bool crlf)
{
    if (format != DNAGPU_TEXT_LINES && format != DNAGPU_TEXT_FASTA && format != DNAGPU_TEXT_FASTQ) {
        ereport_error("copy_dna_to: the format must be 1 (one sequence per line), 2 (FASTA) or 3 (FASTQ)");
        return NULL;
    }
    if (line_width && format != DNAGPU_TEXT_FASTA) {
        ereport_error("copy_dna_to: only FASTA (format 2) takes a line width");
        return NULL;
    }
    CopyDnaTo *c = (CopyDnaTo *)glue_new(sizeof *c);
    if (!c)
        return NULL;
    c->format = format;
    c->line_width = line_width;
    c->crlf = crlf;
    c->chunk = g_copy_chunk_bytes < COPY_MAX_CHUNK ? g_copy_chunk_bytes : COPY_MAX_CHUNK;
    c->limit_bases = c->chunk < ((uint64_t)1 << 30) ? 4 * c->chunk : COPY_MAX_CHUNK;      /* (packed: four bases per byte) */
    return c;
}

/* the image of the batch's table, chunk after chunk, behind the chunks that wait */
static bool copy_to_read(CopyDnaTo *c, const dnagpu_text_image *img, const dnagpu_quals *quals)
{
    const uint64_t bytes = dnagpu_text_image_bytes(img);
    for (uint64_t at = 0; at < bytes; at += c->chunk) {
        const uint64_t n = gs_refill(bytes, at, c->chunk);
        if (!glue_grow(COLS((void **)&c->text, (void **)&c->text_len), &c->cap_text, c->n_text + 1))
            return false;
        char *t = (char *)malloc((size_t)n);
        if (!t) {
            ereport_error("out of memory");
            return false;
        }
        c->text[c->n_text] = t;
        c->text_len[c->n_text++] = n;
        if (!gpu_ok(quals ? dnagpu_text_image_read_quals(g_ctx, img, quals, at, n, t, 0) : dnagpu_text_image_read(g_ctx, img, at, n, t, 0)))
            return false;
    }
    return true;
}

/* the batch so far: made resident, written out, emptied */
static bool copy_to_flush(void *self)
{
    CopyDnaTo *c = (CopyDnaTo *)self;
    bool ok = true;
    if (c->b.n_seqs > 0) {
        const dnagpu_text_out_options opt = {c->format, c->crlf ? DNAGPU_TEXT_OUT_CRLF : 0u, c->line_width, 0, NULL, c->rows_before,
                                             NULL, 0, 0, {0, 0, 0}};
        dnagpu_dna *d = NULL;
        dnagpu_text_image *img = NULL;
        dnagpu_quals *q = NULL;
        ok = batch_upload(&c->b, &d);
        if (ok && c->reads) {
            dnagpu_quals_report qrep;
            const int rc = dnagpu_quals_upload(g_ctx, c->qual, c->b.n_bases, 0, &q, &qrep);
            ok = loader_ok(rc, qrep.bad_pos, qrep.bad_record, 0, NULL);
        }
        dnagpu_names *nm = NULL;
        if (ok && c->named == 1) {
            dnagpu_names_report nrep;
            const int rc = dnagpu_names_upload(g_ctx, c->names, c->name_off, c->b.n_seqs, 0, &nm, &nrep);
            ok = loader_ok(rc, nrep.bad_pos, nrep.bad_record, 0, NULL);
        }
        ok = ok && gpu_ok(nm ? dnagpu_table_to_text_named(g_ctx, d, nm, &opt, &img) : dnagpu_table_to_text(g_ctx, d, &opt, &img)) &&
             copy_to_read(c, img, q);
        if (img)
            dnagpu_text_image_free(g_ctx, img);
        if (nm)
            dnagpu_names_free(g_ctx, nm);
        if (q)
            dnagpu_quals_free(g_ctx, q);
        if (d)
            dnagpu_dna_free(g_ctx, d);
        c->rows_before += c->b.n_seqs;
    }
    rb_clear(&c->b);
    c->n_name_bytes = 0;
    return ok;
}

/* named and unnamed rows do not mix in one handle */
static bool copy_to_kind(CopyDnaTo *c, int kind, const char *who)
{
    if (c->named && c->named != kind) {
        ereport_error("%s: rows with a name and rows without one in the same COPY", who);
        return !(c->life.failed = true);
    }
    c->named = kind;
    return true;
}

/* the name of the row that is added next, behind the names of the batch that takes the row (copy_reads_to_add's first step) */
static bool copy_to_name(CopyDnaTo *c, const Dna *row, const char *name, size_t name_len)
{
    if (rb_spills(&c->b, row->length, c->limit_bases) && !copy_to_flush(c))
        return !(c->life.failed = true);
    if (!rb_grow((void **)&c->names, &c->cap_names, (c->n_name_bytes + name_len) / 8 + 1) ||
        !rb_grow((void **)&c->name_off, &c->cap_name_off, c->b.n_seqs + 2)) {
        ereport_error("out of memory");
        return !(c->life.failed = true);
    }
    if (name_len)
        memcpy(c->names + c->n_name_bytes, name, name_len);
    c->name_off[0] = 0;
    c->n_name_bytes += name_len;
    c->name_off[c->b.n_seqs + 1] = c->n_name_bytes;
    return true;
}

/* the row into the open batch, by the add policy at limit_bases */
static bool copy_to_add(CopyDnaTo *c, const Dna *row)
{
    if (!batch_add(&c->b, row, c->limit_bases, copy_to_flush, c))
        c->life.failed = true;
    return !c->life.failed;
}

bool copy_dna_to_add(CopyDnaTo *c, const Dna *row)
{
    if (!gs_may_add(&c->life)) {
        ereport_error("copy_dna_to: a row added after the last one or after the COPY failed");
        return false;
    }
    if (!row) {
        ereport_error("copy_dna_to: the row is missing");
        return false;
    }
    return copy_to_kind(c, 2, "copy_dna_to") && copy_to_add(c, row);
}

bool copy_dna_to_add_named(CopyDnaTo *c, const Dna *row, const char *name, size_t name_len)
{
    if (!gs_may_add(&c->life) || c->reads) {
        ereport_error("copy_dna_to: a row added after the last one or after the COPY failed");
        return false;
    }
    if (c->format == DNAGPU_TEXT_LINES) {
        ereport_error("copy_dna_to: one sequence per line (format 1) has no names");
        return false;
    }
    if (!row || (name_len && !name)) {
        ereport_error("copy_dna_to: the row or its name is missing");
        return false;
    }
    return copy_to_kind(c, 1, "copy_dna_to") && copy_to_name(c, row, name, name_len) && copy_to_add(c, row);
}

CopyDnaTo *copy_reads_to_begin(bool crlf)
{
    CopyDnaTo *c = copy_dna_to_begin(DNAGPU_TEXT_FASTQ, 0, crlf);
    if (c)
        c->reads = true;
    return c;
}

static bool reads_to_add(CopyDnaTo *c, const Dna *row, const char *name, size_t name_len, bool named, const char *quality,
                         size_t quality_len)
{
    if (!gs_may_add(&c->life) || !c->reads) {
        ereport_error("copy_reads_to: a row added after the last one or after the COPY failed");
        return false;
    }
    if (!row || (quality_len && !quality) || (name_len && !name)) {
        ereport_error(named ? "copy_reads_to: the row, its name or its quality text is missing"
                            : "copy_reads_to: the row or its quality text is missing");
        return false;
    }
    if (!copy_to_kind(c, named ? 1 : 2, "copy_reads_to"))
        return false;
    if ((uint64_t)quality_len != row->length) {
        ereport_error("FASTQ quality line length differs from the sequence's");
        return !(c->life.failed = true);
    }
    if (named && !copy_to_name(c, row, name, name_len))                       /* (flushes a batch the row would spill) */
        return false;
    /* the policy's first step here, in front of it: the qualities of the open batch leave with it, the row's go behind the
     * qualities of the batch that takes the row */
    if (rb_spills(&c->b, row->length, c->limit_bases) && !copy_to_flush(c))
        return !(c->life.failed = true);
    if (!rb_grow((void **)&c->qual, &c->cap_qual, c->b.n_bases + row->length + 1)) {
        ereport_error("out of memory");
        return !(c->life.failed = true);
    }
    if (quality_len)
        memcpy(c->qual + c->b.n_bases, quality, quality_len);
    return copy_to_add(c, row);
}

bool copy_reads_to_add(CopyDnaTo *c, const Dna *row, const char *quality, size_t quality_len)
{
    return reads_to_add(c, row, NULL, 0, false, quality, quality_len);
}

bool copy_reads_to_add_named(CopyDnaTo *c, const Dna *row, const char *name, size_t name_len, const char *quality, size_t quality_len)
{
    return reads_to_add(c, row, name, name_len, true, quality, quality_len);
}

bool copy_reads_to_finish(CopyDnaTo *c) { return copy_dna_to_finish(c); }
bool copy_reads_to_next(CopyDnaTo *c, const char **bytes, size_t *n) { return copy_dna_to_next(c, bytes, n); }
bool copy_reads_to_failed(const CopyDnaTo *c) { return copy_dna_to_failed(c); }
void copy_reads_to_end(CopyDnaTo *c) { copy_dna_to_end(c); }

bool copy_dna_to_finish(CopyDnaTo *c) { return gs_serve(&c->life, copy_to_flush, c); }     /* (the last batch, once) */

bool copy_dna_to_next(CopyDnaTo *c, const char **bytes, size_t *n)
{
    if (c->life.failed || c->next >= c->n_text)
        return false;
    if (c->next > 0) {                                                        /* the chunk served before this one */
        free(c->text[c->next - 1]);
        c->text[c->next - 1] = NULL;
    }
    const uint64_t i = c->next++;
    if (bytes)
        *bytes = c->text[i];
    if (n)
        *n = (size_t)c->text_len[i];
    return true;
}

bool copy_dna_to_failed(const CopyDnaTo *c) { return c->life.failed; }

void copy_dna_to_end(CopyDnaTo *c)
{
    if (!c)
        return;
    for (uint64_t i = 0; i < c->n_text; i++)
        free(c->text[i]);
    free(c->text);
    free(c->text_len);
    free(c->qual);
    free(c->names);
    free(c->name_off);
    rb_free(&c->b);
    free(c);
}
