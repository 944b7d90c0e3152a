/*
 * row_batch.h -- the batch every streaming object of the glue (glue_*.c) collects its rows in: the rows back to back as ONE packed
 * stream (2 bits per base, base 0 at bit 0 of word 0) with the base at which every row starts.  Plain C11 without the GPU
 * library: a row is (bits, length), and tests/host/row_batch_check.c runs all of this on the host.
 */
#ifndef ROW_BATCH_H
#define ROW_BATCH_H

#include <stdbool.h>
#include <stdint.h>
#include <stdlib.h>

typedef struct RowBatch {
    uint64_t *words, n_bases, cap_words;         /* the stream; room for ceil(n_bases / 32) + 1 words */
    uint64_t *starts, n_seqs, cap_seqs;          /* starts[0 .. n_seqs]: starts[0] = 0, starts[n_seqs] = n_bases */
} RowBatch;

/* *p (8-byte units, *cap of them) holds `need` units after this: the first allocation has 1024, every later one doubles */
static inline bool rb_grow(void **p, uint64_t *cap, uint64_t need)
{
    if (need <= *cap)
        return true;
    uint64_t c = *cap ? *cap : 1024;
    while (c < need)
        c *= 2;
    void *q = realloc(*p, (size_t)c * sizeof(uint64_t));
    if (!q)
        return false;
    *p = q;
    *cap = c;
    return true;
}

/* n bases of src (packed, base 0 at bit 0) onto dst from base `at`; dst's bits from `at` on are zero and dst has room for
 * ceil((at + n) / 32) + 1 words */
static inline void append_bases(uint64_t *dst, uint64_t at, const uint64_t *src, uint64_t n)
{
    const unsigned sh = (unsigned)(at & 31) * 2;
    const uint64_t w = at >> 5, nw = (n + 31) / 32;
    for (uint64_t i = 0; i < nw; i++) {
        uint64_t v = src[i];
        if (i == nw - 1 && (n & 31))
            v &= ((uint64_t)1 << (2 * (n & 31))) - 1;                      /* nothing behind the row's last base */
        if (sh == 0) {
            dst[w + i] = v;
        } else {
            dst[w + i] |= v << sh;
            dst[w + i + 1] = v >> (64 - sh);
        }
    }
}

/* one more row behind the batch's rows: its bases onto the packed stream, its end as the next start; false = out of memory */
static inline bool rb_append(RowBatch *b, const uint64_t *bits, uint64_t length)
{
    if (!rb_grow((void **)&b->words, &b->cap_words, (b->n_bases + length + 31) / 32 + 1) ||
        !rb_grow((void **)&b->starts, &b->cap_seqs, b->n_seqs + 2))
        return false;
    b->starts[0] = 0;
    if (length)
        append_bases(b->words, b->n_bases, bits, length);
    b->n_bases += length;
    b->starts[++b->n_seqs] = b->n_bases;
    return true;
}

/* bases [first, first + len) of a packed stream into out's ceil(len / 32) words, zero behind the last base */
static inline void rb_cut(const uint64_t *src, uint64_t first, uint64_t len, uint64_t *out)
{
    const uint64_t nw = (len + 31) / 32;
    for (uint64_t j = 0; j < nw; j++) {
        const uint64_t q = first + 32 * j, nb = len - 32 * j < 32 ? len - 32 * j : 32;
        const unsigned sh = (unsigned)(q & 31) * 2;
        uint64_t v = src[q >> 5] >> sh;
        if ((q & 31) + nb > 32)                                           /* (only then: the next word holds a base of the row) */
            v |= src[(q >> 5) + 1] << (64 - sh);
        if (nb < 32)
            v &= ((uint64_t)1 << (2 * nb)) - 1;
        out[j] = v;
    }
}

/* no row, the capacity kept (append_bases' precondition holds: a stream from base 0 starts with a plain store) */
static inline void rb_clear(RowBatch *b)
{
    b->n_bases = 0;
    b->n_seqs = 0;
}

static inline void rb_free(RowBatch *b)
{
    free(b->words);
    free(b->starts);
    *b = (RowBatch){0};
}

/* The add policy's two tests against a limit in bases.  A row of `length` bases would push a batch that has rows past the
 * limit: it gets a batch of its own (a first row never spills).  The batch has reached the limit: it takes no more rows. */
static inline bool rb_spills(const RowBatch *b, uint64_t length, uint64_t limit)
{
    return b->n_seqs > 0 && b->n_bases + length > limit;
}

static inline bool rb_full(const RowBatch *b, uint64_t limit) { return b->n_bases >= limit; }

#endif
