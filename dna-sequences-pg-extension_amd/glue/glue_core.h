/*
 * glue_core.h -- what the feature files of the glue (glue_*.c) share and do not export: the error report, the lazy GPU
 * context, the process-wide settings, and the steps of glue_steps.h with their error texts.  Definitions: glue_core.c.
 */
#ifndef GLUE_CORE_H
#define GLUE_CORE_H

#include "dna_glue.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/dnagpu.h"
#include "glue_steps.h"

#define CK_MAX_RANKS 64
#define COPY_MAX_CHUNK ((uint64_t)UINT32_MAX)    /* dnagpu_table_from_text's limit for one call */

#pragma GCC visibility push(hidden)

extern dnagpu_ctx *g_ctx;                        /* one per process, created lazily (post-fork): ctx() */
extern uint64_t g_agg_flush_bases, g_copy_chunk_bytes;
extern int g_n_gpus;

void ereport_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
bool gpu_ok(int rc);                             /* status of a dnagpu call -> true, or false with the ERROR reported */
dnagpu_ctx *ctx(void);
dnagpu_multi *multi(void);                       /* the devices of dna_glue_set_gpus */
dnagpu_dna *device_dna(Dna *dna);

void *glue_new(size_t size);                     /* a zeroed object; NULL with "out of memory" */
Dna *dna_new(uint64_t length);                   /* `length` bases of A; NULL with "out of memory" */
Dna *dna_cut(const uint64_t *src, uint64_t first, uint64_t len);
bool cols_alloc(uint64_t n, uint64_t **a, uint64_t **b, uint64_t **c);
bool k_ok(int k);
void put3(int64_t *a, int64_t *b, int64_t *c, uint64_t va, uint64_t vb, uint64_t vc);

/* the columns of a group for glue_grow, with their number: glue_grow(COLS((void **)&t->rows, (void **)&t->hits), &cap, need) */
#define COLS(...) (void **[]){__VA_ARGS__}, (int)(sizeof((void **[]){__VA_ARGS__}) / sizeof(void **))
bool glue_grow(void **const cols[], int n, uint64_t *cap, uint64_t need);
bool batch_add(RowBatch *b, const Dna *row, uint64_t limit, gs_flush_fn flush, void *self);
bool stream_add(GsLife *l, RowBatch *b, const Dna *row, gs_flush_fn flush, void *self, const char *refusal);
bool batch_upload(const RowBatch *b, dnagpu_dna **d);
bool table_rows(const dnagpu_dna *table, uint64_t n, Dna **out);

bool filter_from_op(dnagpu_filter *f, char op, const Kmer *rhs, const Qkmer *rhs_pattern);
bool loader_ok(int rc, uint64_t bad_pos, uint64_t bad_record, uint64_t records_before, int64_t *bad_line);
uint64_t *kmer_keys(const Kmer *column, uint64_t n, int k);

/* glue_count.c: the aggregate's accumulator with every row so far in it */
dnagpu_acc *agg_flushed_acc(CountKmersAgg *a, const char *who);

#pragma GCC visibility pop

#endif
