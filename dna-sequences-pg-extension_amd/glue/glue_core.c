/*
 * glue_core.c -- see glue_core.h: what every feature file of the glue needs once.
 */
#include "glue_core.h"

#include <stdarg.h>

static __thread char g_msg[256];
dnagpu_ctx *g_ctx;
static int g_device;

void ereport_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
}

const char *dna_glue_errmsg(void) { return g_msg; }
void dna_glue_set_device(int device) { g_device = device; }

/* ---- the process-wide settings */
uint64_t g_agg_flush_bases = (uint64_t)1 << 30;
uint64_t g_copy_chunk_bytes = (uint64_t)64 << 20;

void dna_glue_set_agg_flush_bases(uint64_t n) { g_agg_flush_bases = n ? n : 1; }
void dna_glue_set_copy_chunk_bytes(uint64_t n) { g_copy_chunk_bytes = n ? n : 1; }

/* multi-GPU configuration of this backend: count_kmers shards over these devices (dnagpu_count_multi) */
int g_n_gpus = 1;
static int g_transport = DNAGPU_MULTI_AUTO;
static int g_gpu_list[CK_MAX_RANKS];
static dnagpu_multi *g_multi;

static void multi_shutdown(void)
{
    if (g_multi) {
        dnagpu_multi_destroy(g_multi);
        g_multi = NULL;
    }
}

void dna_glue_set_gpus(int n_gpus, const int *devices, int transport)
{
    multi_shutdown();
    g_n_gpus = n_gpus < 1 ? 1 : (n_gpus > CK_MAX_RANKS ? CK_MAX_RANKS : n_gpus);
    for (int r = 0; r < g_n_gpus; r++)
        g_gpu_list[r] = devices ? devices[r] : r;
    g_transport = transport;
}

dnagpu_multi *multi(void)
{
    if (!g_multi && !gpu_ok(dnagpu_multi_init(g_gpu_list, g_n_gpus, g_transport, &g_multi)))
        return NULL;
    return g_multi;
}

void dna_glue_shutdown(void)
{
    multi_shutdown();
    if (g_ctx) {
        dnagpu_destroy(g_ctx);
        g_ctx = NULL;
    }
}

/* ---- the GPU library: its status as the reference's message (codes 1..3) or the library's detail */
bool gpu_ok(int rc)
{
    if (rc == DNAGPU_OK)
        return true;
    if (rc <= DNAGPU_ERR_QKMER_INVALID)
        ereport_error("%s", dnagpu_strerror(rc));
    else
        ereport_error("%s: %s", dnagpu_strerror(rc), dnagpu_last_error());
    return false;
}

dnagpu_ctx *ctx(void)
{
    if (!g_ctx && !gpu_ok(dnagpu_init(g_device, &g_ctx)))
        return NULL;
    return g_ctx;
}

dnagpu_dna *device_dna(Dna *dna)
{
    if (!dna->dev) {
        dnagpu_dna *d = NULL;
        if (!ctx() || !gpu_ok(dnagpu_dna_upload(g_ctx, dna->bit_sequence, dna->length, &d)))
            return NULL;
        dna->dev = d;
    }
    return (dnagpu_dna *)dna->dev;
}

/* ---- host memory, with the ERROR */
void *glue_new(size_t size)
{
    void *p = calloc(1, size);
    if (!p)
        ereport_error("out of memory");
    return p;
}

Dna *dna_new(uint64_t length)
{
    const uint64_t n_words = (length * 2 + 63) / 64;                      /* dna.c:181-182 */
    Dna *dna = (Dna *)calloc(1, sizeof(Dna));
    uint64_t *w = (uint64_t *)calloc(n_words ? n_words : 1, sizeof(uint64_t));   /* palloc0, dna.c:186 */
    if (!dna || !w) {
        free(dna);
        free(w);
        ereport_error("out of memory");
        return NULL;
    }
    dna->length = length;
    dna->bit_sequence = w;
    return dna;
}

/* bases [first, first + len) of a packed stream as a value of its own */
Dna *dna_cut(const uint64_t *src, uint64_t first, uint64_t len)
{
    Dna *out = dna_new(len);
    if (out)
        rb_cut(src, first, len, out->bit_sequence);
    return out;
}

/* columns of n entries each (c may be NULL); after a failure the caller's _end frees what was allocated */
bool cols_alloc(uint64_t n, uint64_t **a, uint64_t **b, uint64_t **c)
{
    *a = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)n);
    *b = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)n);
    if (c)
        *c = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)n);
    if (*a && *b && (!c || *c))
        return true;
    ereport_error("out of memory");
    return false;
}

bool k_ok(int k)
{
    if (k >= 1 && k <= 32)
        return true;
    ereport_error("%s", dnagpu_strerror(DNAGPU_ERR_INVALID_K));              /* dna.c:772-773 */
    return false;
}

/* three totals, each into a pointer that may be NULL */
void put3(int64_t *a, int64_t *b, int64_t *c, uint64_t va, uint64_t vb, uint64_t vc)
{
    if (a) *a = (int64_t)va;
    if (b) *b = (int64_t)vb;
    if (c) *c = (int64_t)vc;
}

/* ---- the steps of glue_steps.h, with the ERROR */
bool glue_grow(void **const cols[], int n, uint64_t *cap, uint64_t need)
{
    if (gs_grow(cols, n, cap, need))
        return true;
    ereport_error("out of memory");
    return false;
}

bool batch_add(RowBatch *b, const Dna *row, uint64_t limit, gs_flush_fn flush, void *self)
{
    const int r = gs_add(b, row->bit_sequence, row->length, limit, flush, self);
    if (r == GS_NO_MEMORY)
        ereport_error("out of memory");
    return r == GS_ADDED;
}

/* the _add of an object whose batches end at g_agg_flush_bases; `refusal`: its text for a row that comes too late */
bool stream_add(GsLife *l, RowBatch *b, const Dna *row, gs_flush_fn flush, void *self, const char *refusal)
{
    if (!gs_may_add(l)) {
        ereport_error("%s", refusal);
        return false;
    }
    if (!batch_add(b, row, g_agg_flush_bases, flush, self))
        l->failed = true;
    return !l->failed;
}

/* the batch as a resident table with its boundaries; rows without a base make a stream of no words.  *d is the caller's to
 * free, also after an ERROR */
bool batch_upload(const RowBatch *b, dnagpu_dna **d)
{
    static const uint64_t none[1] = {0};
    return ctx() != NULL && gpu_ok(dnagpu_dna_upload(g_ctx, b->n_bases ? b->words : none, b->n_bases, d)) &&
           gpu_ok(dnagpu_dna_set_sequences(g_ctx, *d, b->starts, b->n_seqs));
}

/* the first n sequences of a resident table as values of their own: out[0 .. n), cut from one download of the stream and of
 * its starts.  On failure none of them stays allocated. */
bool table_rows(const dnagpu_dna *table, uint64_t n, Dna **out)
{
    const uint64_t total = dnagpu_dna_length(table);
    uint64_t *words = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)((total + 31) / 32 + 1));
    uint64_t *starts = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(n + 1));
    bool ok = words && starts;
    if (!ok)
        ereport_error("out of memory");
    ok = ok && gpu_ok(dnagpu_dna_download(g_ctx, table, words)) && gpu_ok(dnagpu_dna_sequence_starts(g_ctx, table, 0, n + 1, starts, 0));
    uint64_t made = 0;
    for (; ok && made < n; made++) {
        out[made] = dna_cut(words, starts[made], starts[made + 1] - starts[made]);
        if (!out[made])
            break;
    }
    if (made < n) {
        ok = false;
        while (made > 0)
            dna_free(out[--made]);
    }
    free(words);
    free(starts);
    return ok;
}

/* ---- a WHERE on the k-mer as the library's filter: op '=' / '^' (rhs) or '@' (rhs_pattern) */
bool filter_from_op(dnagpu_filter *f, char op, const Kmer *rhs, const Qkmer *rhs_pattern)
{
    memset(f, 0, sizeof *f);
    switch (op) {
    case '=':
    case '^':
        f->kind = op == '=' ? DNAGPU_FILTER_EQUALS : DNAGPU_FILTER_STARTS_WITH;
        f->length = rhs->length;
        f->bits = rhs->bit_sequence;
        return true;
    case '@':
        f->kind = DNAGPU_FILTER_CONTAINS;
        strncpy(f->pattern, rhs_pattern->sequence, sizeof f->pattern - 1);
        return true;
    }
    ereport_error("unknown operator");
    return false;
}

/* the status of a loader: an input error (bad_pos is set) is handed on with the library's message verbatim and *bad_line =
 * the 1-based record of the whole file it belongs to (0: none); every other error goes through gpu_ok */
bool loader_ok(int rc, uint64_t bad_pos, uint64_t bad_record, uint64_t records_before, int64_t *bad_line)
{
    if (rc == DNAGPU_OK || bad_pos == UINT64_MAX)
        return gpu_ok(rc);
    ereport_error("%s", dnagpu_last_error());
    if (bad_line)
        *bad_line = bad_record == UINT64_MAX ? 0 : (int64_t)(records_before + bad_record + 1);
    return false;
}

/* a column of kmer as keys of the one length k (malloc'd, at least one entry); NULL with the ERROR */
uint64_t *kmer_keys(const Kmer *column, uint64_t n, int k)
{
    for (uint64_t i = 0; i < n; i++)
        if (column[i].length != k) {
            ereport_error("kmer_index_create: the column holds kmers of %d and %d bases; an index covers one length", k,
                          (int)column[i].length);
            return NULL;
        }
    uint64_t *keys = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(n ? n : 1));
    if (!keys)
        ereport_error("out of memory");
    for (uint64_t i = 0; keys && i < n; i++)
        keys[i] = column[i].bit_sequence;
    return keys;
}
