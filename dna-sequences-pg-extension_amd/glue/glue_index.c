/*
 * glue_index.c -- the index over a stored kmer column: build, insert, delete, and the three scans.
 */
#include "glue_core.h"

struct KmerIndex {
    dnagpu_kmer_index *idx;
    int k;
};

KmerIndex *kmer_index_create(const Kmer *column, uint64_t n)
{
    const int k = n ? column[0].length : 1;          /* (an empty column: any length does, no scan finds a row) */
    uint64_t *keys = kmer_keys(column, n, k);
    KmerIndex *x = keys ? (KmerIndex *)glue_new(sizeof *x) : NULL;
    if (x) {
        x->k = k;
        if (!ctx() || !gpu_ok(dnagpu_kmer_index_build(g_ctx, keys, n, k, 0, &x->idx))) {    /* a bad length: dna.c:773 */
            free(x);
            x = NULL;
        }
    }
    free(keys);
    return x;
}

uint64_t kmer_index_rows(const KmerIndex *idx)
{
    return idx ? dnagpu_kmer_index_rows(idx->idx) : 0;
}

int64_t kmer_index_insert(KmerIndex *idx, const Kmer *rows, uint64_t n)
{
    if (!ctx())
        return -1;
    const int64_t first = (int64_t)dnagpu_kmer_index_next_row(idx->idx);
    if (n == 0)
        return first;
    /* created over an empty column: the first rows decide the length */
    const int k = first == 0 ? rows[0].length : idx->k;
    uint64_t *keys = kmer_keys(rows, n, k);
    if (!keys)
        return -1;
    bool ok = true;
    if (k != idx->k) {
        dnagpu_kmer_index *empty = NULL;
        ok = gpu_ok(dnagpu_kmer_index_build(g_ctx, NULL, 0, k, 0, &empty));     /* a bad length: dna.c:773 */
        if (ok) {
            dnagpu_kmer_index_free(g_ctx, idx->idx);
            idx->idx = empty;
            idx->k = k;
        }
    }
    ok = ok && gpu_ok(dnagpu_kmer_index_append(g_ctx, idx->idx, keys, n, 0));
    free(keys);
    return ok ? first : -1;
}

int64_t kmer_index_delete(KmerIndex *idx, const int64_t *rows, uint64_t n)
{
    if (!ctx())
        return -1;
    uint64_t gone = 0;                               /* a negative id reads as one above 2^32 - 1: ignored */
    if (!gpu_ok(dnagpu_kmer_index_delete(g_ctx, idx->idx, (const uint64_t *)rows, n, 0, &gone)))
        return -1;
    return (int64_t)gone;
}

static int cmp_i64(const void *a, const void *b)
{
    const int64_t x = *(const int64_t *)a, y = *(const int64_t *)b;
    return (x > y) - (x < y);
}

/* the rows of one index scan, sorted into heap order */
static int64_t index_scan(KmerIndex *x, char op, const Kmer *rhs, const Qkmer *pattern, int64_t **rows)
{
    dnagpu_filter f;
    filter_from_op(&f, op, rhs, pattern);
    *rows = NULL;
    uint64_t n = 0;
    if (!ctx() || !gpu_ok(dnagpu_kmer_index_scan(g_ctx, x->idx, &f, NULL, NULL, 0, &n, NULL, 0)))
        return -1;
    if (n == 0)
        return 0;
    int64_t *out = (int64_t *)malloc(sizeof(int64_t) * (size_t)n);
    if (!out) {
        ereport_error("out of memory");
        return -1;
    }
    uint64_t got = 0;
    if (!gpu_ok(dnagpu_kmer_index_scan(g_ctx, x->idx, &f, (uint64_t *)out, NULL, n, &got, NULL, 0)) || got != n) {
        free(out);
        return -1;
    }
    qsort(out, (size_t)n, sizeof *out, cmp_i64);     /* row ids are < 2^32: the same order signed or unsigned */
    *rows = out;
    return (int64_t)n;
}

int64_t kmer_index_scan_eq(KmerIndex *idx, const Kmer *rhs, int64_t **rows) { return index_scan(idx, '=', rhs, NULL, rows); }

int64_t kmer_index_scan_starts_with(KmerIndex *idx, const Kmer *prefix, int64_t **rows)
{
    return index_scan(idx, '^', prefix, NULL, rows);
}

int64_t kmer_index_scan_contains(KmerIndex *idx, const Qkmer *pattern, int64_t **rows)
{
    return index_scan(idx, '@', NULL, pattern, rows);
}

void kmer_index_end(KmerIndex *idx)
{
    if (!idx)
        return;
    if (g_ctx)
        dnagpu_kmer_index_free(g_ctx, idx->idx);
    free(idx);
}
