/*
 * glue_copy.c -- COPY ... FROM a text file: copy_dna (lines, FASTA), copy_reads (FASTQ and real FASTA, with the source map)
 * and trim_reads (FASTQ with its qualities, trimmed on the device).  The way back: glue_copy_to.c.
 */
#include "glue_core.h"

/* ------------------------------------------------------------------ COPY ... FROM a text file: copy_dna */

struct CopyDna {
    int format;
    GsLife life;                                 /* started: the last bytes have been fed */
    GsBytes in;                                  /* the bytes fed and not yet accounted for by a load */
    uint64_t chunk;
    Dna **rows;                                  /* the rows loaded and not yet served (NULL once handed out) */
    uint64_t cap_rows, n_rows, next;             /* cap_rows: of rows[] and of the per-row arrays below */
    uint64_t first_line;                         /* rows of the whole file before rows[0] */
    int64_t bad_line;                            /* after an input ERROR: the 1-based row of the whole file it belongs to, else 0 */
    /* copy_reads_begin: the load goes through dnagpu_reads_from_text, and every row knows where it came from */
    bool reads;
    int ambiguous;
    unsigned flags;
    uint64_t min_bases;
    uint64_t *src_record, *src_offset;           /* per row of rows[]: the source record of the whole file, the offset in it */
    uint64_t first_record;                       /* source records of the whole file before the buffer's first byte */
    /* trim_reads_begin: FASTQ with its qualities, trimmed and filtered on the device; every row has its quality text */
    bool trim;
    dnagpu_quals_trim_options trim_opt;
    char **qual;                                 /* per row of rows[]: malloc'd, NUL-terminated (NULL once handed out) */
    /* trim_reads_add_adapter: the passing reads of the trim are cut at their 3' adapter (none added: no such step) */
    Qkmer adapter[32];
    uint32_t n_adapters;
    dnagpu_adapters_options ad_opt;
    /* copy_reads_keep_names: every row has the name of its source record */
    bool fed, keep_names, first_word;
    char **name;                                 /* per row of rows[]: malloc'd, NUL-terminated (NULL once served) */
    uint64_t *name_len;
    char *served_name;                           /* the name of the row last returned by a _next; freed by the next one */
    uint64_t served_len;
};

CopyDna *copy_dna_begin(int format)
{
    if (format != DNAGPU_TEXT_LINES && format != DNAGPU_TEXT_FASTA) {
        ereport_error("copy_dna: the format must be 1 (one sequence per line) or 2 (FASTA)");
        return NULL;
    }
    CopyDna *c = (CopyDna *)glue_new(sizeof *c);
    if (!c)
        return NULL;
    c->format = format;
    c->chunk = g_copy_chunk_bytes < COPY_MAX_CHUNK ? g_copy_chunk_bytes : COPY_MAX_CHUNK;
    return c;
}

CopyDna *copy_reads_begin(int format, int ambiguous, unsigned flags, uint64_t min_bases)
{
    if (format != DNAGPU_TEXT_LINES && format != DNAGPU_TEXT_FASTA && format != DNAGPU_TEXT_FASTQ) {
        ereport_error("copy_reads: the format must be 1 (one sequence per line), 2 (FASTA) or 3 (FASTQ)");
        return NULL;
    }
    if (ambiguous < DNAGPU_AMBIG_ERROR || ambiguous > DNAGPU_AMBIG_SPLIT || (flags & ~DNAGPU_READS_FOLD_CASE)) {
        ereport_error("copy_reads: the ambiguity policy must be 0, 1 or 2 and the flags 0 or DNAGPU_READS_FOLD_CASE");
        return NULL;
    }
    CopyDna *c = copy_dna_begin(format == DNAGPU_TEXT_FASTQ ? DNAGPU_TEXT_LINES : format);
    if (!c)
        return NULL;
    c->format = format;
    c->reads = true;
    c->ambiguous = ambiguous;
    c->flags = flags;
    c->min_bases = min_bases;
    return c;
}

CopyDna *trim_reads_begin(int ambiguous, unsigned flags, uint32_t cut_front, uint32_t cut_tail, uint64_t min_bases, uint32_t min_mean_q,
                          uint32_t low_q, uint32_t low_num, uint32_t low_den)
{
    if (cut_front > 255 || cut_tail > 255 || min_mean_q > 255 || low_q > 255) {
        ereport_error("trim_reads: cut_front, cut_tail, min_mean_q and low_q must be at most 255");
        return NULL;
    }
    CopyDna *c = copy_reads_begin(DNAGPU_TEXT_FASTQ, ambiguous, flags, 0);
    if (!c)
        return NULL;
    c->trim = true;
    const dnagpu_quals_trim_options o = {cut_front, cut_tail, min_mean_q, low_q, low_num, low_den, min_bases, 0};
    c->trim_opt = o;
    const dnagpu_adapters_options a = {0, 1, 3, 0, min_bases, 0};
    c->ad_opt = a;
    return c;
}

/* the two calls that make a trim_reads handle cut adapters: only between the begin and the first feed */
static bool adapters_may_change(const CopyDna *c, const char *who)
{
    if (!c->trim) {
        ereport_error("%s: only a trim_reads handle cuts adapters", who);
        return false;
    }
    if (c->fed) {
        ereport_error("%s: called after the first bytes were fed", who);
        return false;
    }
    return true;
}

bool trim_reads_add_adapter(CopyDna *c, const char *adapter)
{
    if (!adapters_may_change(c, "trim_reads_add_adapter"))
        return false;
    if (c->n_adapters == 32) {
        ereport_error("trim_reads_add_adapter: a handle takes at most 32 adapters");
        return false;
    }
    if (!qkmer_in(adapter, &c->adapter[c->n_adapters]))                   /* (the letters of a qkmer, 1 .. 32 of them) */
        return false;
    c->n_adapters++;
    return true;
}

bool trim_reads_adapter_options(CopyDna *c, uint32_t err_num, uint32_t err_den, uint32_t min_overlap, unsigned flags)
{
    if (!adapters_may_change(c, "trim_reads_adapter_options"))
        return false;
    const unsigned both = DNAGPU_ADAPTERS_DISCARD_UNTRIMMED | DNAGPU_ADAPTERS_DISCARD_TRIMMED;
    if (err_den < 1 || err_num > err_den || min_overlap < 1 || min_overlap > 32 || (flags & ~both) || (flags & both) == both) {
        ereport_error("trim_reads_adapter_options: the error rate must be at most 1, min_overlap 1 .. 32, and at most one discard flag set");
        return false;
    }
    c->ad_opt.err_num = err_num;
    c->ad_opt.err_den = err_den;
    c->ad_opt.min_overlap = min_overlap;
    c->ad_opt.flags = flags;
    return true;
}

/* room for `need` rows: rows[] and the per-row arrays of the object's kind, which grow together */
static bool copy_grow(CopyDna *c, uint64_t need)
{
    void **cols[6] = {(void **)&c->rows, (void **)&c->src_record, (void **)&c->src_offset};
    int n = c->reads ? 3 : 1;
    if (c->trim)
        cols[n++] = (void **)&c->qual;
    if (c->keep_names) {
        cols[n++] = (void **)&c->name;
        cols[n++] = (void **)&c->name_len;
    }
    return glue_grow(cols, n, &c->cap_rows, need);
}

bool copy_reads_keep_names(CopyDna *c, bool first_word)
{
    if (!c->reads || (c->format != DNAGPU_TEXT_FASTA && c->format != DNAGPU_TEXT_FASTQ)) {
        ereport_error("copy_reads_keep_names: only FASTA and FASTQ (copy_reads_begin with format 2 or 3, trim_reads_begin) have names");
        return false;
    }
    if (c->fed) {
        ereport_error("copy_reads_keep_names: called after the first bytes were fed");
        return false;
    }
    c->keep_names = true;
    c->first_word = first_word;
    return true;
}

const char *copy_reads_name(const CopyDna *c, size_t *len)
{
    if (len)
        *len = c->served_name ? (size_t)c->served_len : 0;
    return c->served_name;
}

/* the m strings of nm as the names of rows at .. at + m of c (room is there): malloc'd, NUL-terminated */
static bool names_rows(CopyDna *c, const dnagpu_names *nm, uint64_t m, uint64_t at)
{
    const uint64_t total = dnagpu_names_bytes(nm);
    uint64_t *off = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(m + 1));
    char *bytes = (char *)malloc((size_t)total + 1);
    bool ok = off && bytes;
    if (!ok)
        ereport_error("out of memory");
    ok = ok && gpu_ok(dnagpu_names_offsets(g_ctx, nm, 0, m + 1, off, 0)) && gpu_ok(dnagpu_names_read(g_ctx, nm, 0, total, bytes, 0));
    for (uint64_t i = 0; i < m; i++)
        c->name[at + i] = NULL;
    for (uint64_t i = 0; ok && i < m; i++) {
        const uint64_t len = off[i + 1] - off[i];
        char *t = (char *)malloc((size_t)len + 1);
        if (!t) {
            ereport_error("out of memory");
            ok = false;
            break;
        }
        memcpy(t, bytes + off[i], (size_t)len);
        t[len] = 0;
        c->name[at + i] = t;
        c->name_len[at + i] = len;
    }
    if (!ok)
        for (uint64_t i = 0; i < m; i++) {
            free(c->name[at + i]);
            c->name[at + i] = NULL;
        }
    free(off);
    free(bytes);
    return ok;
}

/* the tail of a load: the bytes accounted for are dropped; a record longer than the chunk doubles the chunk */
static bool copy_consumed(CopyDna *c, uint64_t consumed, bool more, const char *who)
{
    gs_bytes_drop(&c->in, consumed);
    if (more && consumed == 0 && !gs_chunk_grow(&c->chunk, COPY_MAX_CHUNK)) {
        ereport_error("%s: a record is longer than 2^32 - 1 bytes", who);
        return false;
    }
    return true;
}

/* trim_reads: the table d that the loader made of the first text_bytes bytes of the buffer (rec / off: its source map, n_seqs
 * entries) with its qualities, trimmed and filtered on the device: the passing reads appended as rows with their source
 * record, the offset of their first kept base in it, and their quality text.  *appended = how many. */
static bool trim_load(CopyDna *c, const dnagpu_dna *d, uint64_t text_bytes, const uint64_t *rec, const uint64_t *off, uint64_t n_seqs,
                      const dnagpu_names *names, uint64_t *appended)
{
    dnagpu_quals *q = NULL, *tq = NULL;
    dnagpu_dna *td = NULL;
    dnagpu_quals_report qrep;
    dnagpu_quals_trim_report trep;
    uint64_t *seg = NULL, *starts = NULL;
    void *dev = NULL;
    char *text = NULL;
    bool ok = false;
    *appended = 0;
    const int rc = dnagpu_quals_from_fastq(g_ctx, c->in.buf, text_bytes, 0, d, n_seqs ? rec : NULL, n_seqs ? off : NULL, &q, &qrep);
    if (!loader_ok(rc, qrep.bad_pos, qrep.bad_record, c->first_record, &c->bad_line))
        return false;
    if (n_seqs == 0) {
        dnagpu_quals_free(g_ctx, q);
        return true;
    }
    seg = (uint64_t *)malloc(sizeof(uint64_t) * 3 * (size_t)n_seqs);
    starts = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(n_seqs + 1));
    if (!seg || !starts) {
        ereport_error("out of memory");
        goto done;
    }
    uint64_t *seg_seq = seg, *seg_first = seg + n_seqs, *seg_len = seg + 2 * n_seqs;
    uint64_t m = 0;
    if (c->n_adapters) {                                                  /* the trim's lists stay on the device: the adapters' input */
        const char *texts[32];
        dnagpu_adapters_report arep;
        for (uint32_t a = 0; a < c->n_adapters; a++)
            texts[a] = c->adapter[a].sequence;
        if (!gpu_ok(dnagpu_buffer_alloc(g_ctx, 3 * 8 * n_seqs, &dev)))
            goto done;
        uint64_t *dv = (uint64_t *)dev;
        if (!gpu_ok(dnagpu_quals_trim(g_ctx, d, q, &c->trim_opt, NULL, NULL, NULL, NULL, dv, dv + n_seqs, dv + 2 * n_seqs, n_seqs, 1, &trep)) ||
            !gpu_ok(dnagpu_dna_adapters(g_ctx, d, texts, c->n_adapters, &c->ad_opt, dv, dv + n_seqs, dv + 2 * n_seqs, trep.passed, 1, NULL,
                                        NULL, NULL, seg_seq, seg_first, seg_len, n_seqs, 0, &arep)))
            goto done;
        m = arep.passed;
    } else {
        if (!gpu_ok(dnagpu_quals_trim(g_ctx, d, q, &c->trim_opt, NULL, NULL, NULL, NULL, seg_seq, seg_first, seg_len, n_seqs, 0, &trep)))
            goto done;
        m = trep.passed;
    }
    if (!gpu_ok(dnagpu_dna_sequence_starts(g_ctx, d, 0, n_seqs + 1, starts, 0)))
        goto done;
    if (m == 0) {
        ok = true;
        goto done;
    }
    if (!gpu_ok(dnagpu_dna_gather(g_ctx, d, seg_first, seg_len, NULL, m, 0, &td)) ||
        !gpu_ok(dnagpu_quals_gather(g_ctx, q, seg_first, seg_len, NULL, m, 0, &tq)))
        goto done;
    const uint64_t kept = dnagpu_quals_bases(tq);
    text = (char *)malloc((size_t)kept + 1);
    if (!text) {
        ereport_error("out of memory");
        goto done;
    }
    if (!gpu_ok(dnagpu_quals_read(g_ctx, tq, 0, kept, text, 0)) || !copy_grow(c, c->n_rows + m) || !table_rows(td, m, c->rows + c->n_rows))
        goto done;
    uint64_t at = 0;
    for (uint64_t i = 0; i < m; i++)
        c->qual[c->n_rows + i] = NULL;
    for (uint64_t i = 0; i < m; i++) {
        const uint64_t s = seg_seq[i], len = seg_len[i];
        char *t = (char *)malloc((size_t)len + 1);
        if (!t) {
            ereport_error("out of memory");
            for (uint64_t j = 0; j < m; j++) {                            /* the rows of this load are not kept */
                dna_free(c->rows[c->n_rows + j]);
                free(c->qual[c->n_rows + j]);
            }
            goto done;
        }
        memcpy(t, text + at, (size_t)len);
        t[len] = 0;
        at += len;
        c->qual[c->n_rows + i] = t;
        c->src_record[c->n_rows + i] = c->first_record + rec[s];
        c->src_offset[c->n_rows + i] = off[s] + (seg_first[i] - starts[s]);
    }
    if (names) {                                                          /* the passing reads' own names */
        dnagpu_names *tn = NULL;
        ok = gpu_ok(dnagpu_names_take(g_ctx, names, seg_seq, m, 0, &tn)) && names_rows(c, tn, m, c->n_rows);
        if (tn)
            dnagpu_names_free(g_ctx, tn);
        if (!ok) {
            for (uint64_t j = 0; j < m; j++) {
                dna_free(c->rows[c->n_rows + j]);
                free(c->qual[c->n_rows + j]);
            }
            goto done;
        }
    }
    *appended = m;
    ok = true;
done:
    free(text);
    free(seg);
    free(starts);
    if (dev)
        dnagpu_buffer_free(g_ctx, dev);
    if (td)
        dnagpu_dna_free(g_ctx, td);
    if (tq)
        dnagpu_quals_free(g_ctx, tq);
    dnagpu_quals_free(g_ctx, q);
    return ok;
}

/* copy_load for copy_reads_begin: the same chunk through dnagpu_reads_from_text.  The source arrays are sized for reads of
 * 32 bytes and more; a chunk of shorter ones is loaded a second time with the size its report names */
static bool copy_load_reads(CopyDna *c, uint64_t n, bool more)
{
    const dnagpu_reads_options opt = {c->format, c->ambiguous, c->flags | (more ? DNAGPU_READS_MORE : 0u), 0u, c->min_bases};
    dnagpu_dna *d = NULL;
    dnagpu_reads_report rep;
    uint64_t cap = n / 32 + 1024, *rec = NULL, *off = NULL, *pos = NULL;
    for (;;) {
        const uint64_t pos_cap = c->keep_names ? cap : 0;                     /* (the records' offsets: only the names need them) */
        bool ok = cols_alloc(cap, &rec, &off, c->keep_names ? &pos : NULL);
        if (ok) {
            const int rc = dnagpu_reads_from_text(g_ctx, c->in.buf, n, 0, &opt, &d, pos, pos_cap, rec, off, cap, &rep);
            ok = loader_ok(rc, rep.bad_pos, rep.bad_record, c->first_record, &c->bad_line);
        }
        if (ok && rep.sequences <= cap && (!c->keep_names || rep.records <= cap))
            break;
        if (ok)
            dnagpu_dna_free(g_ctx, d);
        free(rec);
        free(off);
        free(pos);
        pos = NULL;
        if (!ok)
            return false;
        cap = rep.sequences > rep.records ? rep.sequences : rep.records;
    }
    dnagpu_names *names = NULL;
    if (c->keep_names) {                                                  /* the names of the same bytes */
        dnagpu_names_report nrep;
        const int rc = dnagpu_names_from_text(g_ctx, c->in.buf, more ? rep.consumed : n, 0, c->format,
                                              c->first_word ? DNAGPU_NAMES_FIRST_WORD : 0u, pos, rep.records, rec, rep.sequences, &names,
                                              &nrep);
        if (!loader_ok(rc, nrep.bad_pos, nrep.bad_record, c->first_record, &c->bad_line)) {
            dnagpu_dna_free(g_ctx, d);
            free(rec);
            free(off);
            free(pos);
            return false;
        }
    }
    if (c->next == c->n_rows)                                             /* everything served: the arrays start over */
        c->n_rows = c->next = 0;
    uint64_t added = rep.sequences;
    bool ok;
    if (c->trim) {                                                        /* the qualities of the same bytes, then the trim */
        ok = trim_load(c, d, more ? rep.consumed : n, rec, off, rep.sequences, names, &added);
    } else {
        ok = copy_grow(c, c->n_rows + rep.sequences) && (rep.sequences == 0 || table_rows(d, rep.sequences, c->rows + c->n_rows));
        if (ok && names && !names_rows(c, names, rep.sequences, c->n_rows)) {
            for (uint64_t i = 0; i < rep.sequences; i++)                      /* the rows of this load are not kept */
                dna_free(c->rows[c->n_rows + i]);
            ok = false;
        }
        for (uint64_t i = 0; ok && i < rep.sequences; i++) {
            c->src_record[c->n_rows + i] = c->first_record + rec[i];
            c->src_offset[c->n_rows + i] = off[i];
        }
    }
    if (names)
        dnagpu_names_free(g_ctx, names);
    dnagpu_dna_free(g_ctx, d);
    free(rec);
    free(off);
    free(pos);
    if (!ok)
        return false;
    c->n_rows += added;
    c->first_record += rep.records;
    return copy_consumed(c, rep.consumed, more, "copy_reads");
}

/* the first n bytes of the buffer through dnagpu_table_from_text; the rows appended, the bytes accounted for dropped */
static bool copy_load(CopyDna *c, uint64_t n, bool more)
{
    dnagpu_dna *d = NULL;
    dnagpu_text_report rep;
    if (!ctx())
        return false;
    if (c->reads)
        return copy_load_reads(c, n, more);
    const int rc = dnagpu_table_from_text(g_ctx, c->in.buf, n, 0, c->format, more ? DNAGPU_TEXT_MORE : 0u, &d, NULL, 0, &rep);
    if (!loader_ok(rc, rep.bad_pos, rep.bad_record, c->first_line + c->n_rows, &c->bad_line))   /* (the reference's message) */
        return false;
    if (c->next == c->n_rows) {                                           /* everything served: the array starts over */
        c->first_line += c->n_rows;
        c->n_rows = c->next = 0;
    }
    bool ok = copy_grow(c, c->n_rows + rep.records) && (rep.records == 0 || table_rows(d, rep.records, c->rows + c->n_rows));
    dnagpu_dna_free(g_ctx, d);
    if (!ok)
        return false;
    c->n_rows += rep.records;
    return copy_consumed(c, rep.consumed, more, "copy_dna");
}

bool copy_dna_feed(CopyDna *c, const char *bytes, size_t n, bool last)
{
    if (!gs_may_add(&c->life)) {
        ereport_error("copy_dna: bytes fed after the last ones or after the load failed");
        return false;
    }
    if (n && !bytes) {
        ereport_error("copy_dna: the bytes are missing");
        return false;
    }
    c->fed = true;
    if (!gs_bytes_append(&c->in, bytes, n)) {
        ereport_error("out of memory");
        c->life.failed = true;
        return false;
    }
    while (!c->life.failed && c->in.len >= c->chunk)
        c->life.failed = !copy_load(c, c->chunk, true);
    if (!c->life.failed && last) {
        c->life.failed = !copy_load(c, c->in.len, false);
        c->life.started = true;
    }
    return !c->life.failed;
}

bool copy_dna_next(CopyDna *c, Dna **row, int64_t *line)
{
    if (c->life.failed) {
        if (line)
            *line = c->bad_line;
        return false;
    }
    if (c->next >= c->n_rows)
        return false;
    const uint64_t i = c->next++;
    if (line)
        *line = (int64_t)(c->first_line + i + 1);
    if (row) {
        *row = c->rows[i];                                                /* the caller's from here on */
        c->rows[i] = NULL;
    }
    return true;
}

bool copy_reads_next(CopyDna *c, Dna **row, int64_t *record, int64_t *offset)
{
    if (c->life.failed || !c->reads) {
        if (record)
            *record = c->bad_line - 1;
        return false;
    }
    if (c->next >= c->n_rows)
        return false;
    const uint64_t i = c->next;
    if (record)
        *record = (int64_t)c->src_record[i];
    if (offset)
        *offset = (int64_t)c->src_offset[i];
    if (c->keep_names) {                                                  /* copy_reads_name: this row's, until the next call */
        free(c->served_name);
        c->served_name = c->name[i];
        c->served_len = c->name_len[i];
        c->name[i] = NULL;
    }
    return copy_dna_next(c, row, NULL);
}

bool trim_reads_next(CopyDna *c, Dna **row, int64_t *record, int64_t *offset, char **quality)
{
    if (c->life.failed || !c->trim) {
        if (record)
            *record = c->bad_line - 1;
        return false;
    }
    if (c->next >= c->n_rows)
        return false;
    const uint64_t i = c->next;
    if (quality)
        *quality = c->qual[i];                                            /* the caller's from here on (free) */
    else
        free(c->qual[i]);
    c->qual[i] = NULL;
    return copy_reads_next(c, row, record, offset);
}

bool copy_dna_failed(const CopyDna *c) { return c->life.failed; }

void copy_dna_end(CopyDna *c)
{
    if (!c)
        return;
    for (uint64_t i = 0; c->qual && i < c->n_rows; i++)
        free(c->qual[i]);
    free(c->qual);
    for (uint64_t i = 0; c->name && i < c->n_rows; i++)
        free(c->name[i]);
    free(c->name);
    free(c->name_len);
    free(c->served_name);
    for (uint64_t i = 0; i < c->n_rows; i++)
        dna_free(c->rows[i]);
    free(c->rows);
    free(c->src_record);
    free(c->src_offset);
    free(c->in.buf);
    free(c);
}
