/*
 * glue_steps.h -- the arithmetic and the small state machines that the streaming objects of the glue share, beside
 * row_batch.h and in its manner: plain C11 without the GPU library and without an error text (glue_core.c words the errors).
 * tests/host/glue_steps_check.c runs all of this on the host.
 */
#ifndef GLUE_STEPS_H
#define GLUE_STEPS_H

#include <string.h>

#include "row_batch.h"

/* ---- answer columns that grow together: n columns of 8-byte units under ONE capacity (rb_grow's: 1024, then doubling) */
static inline bool gs_grow(void **const cols[], int n, uint64_t *cap, uint64_t need)
{
    uint64_t grown = *cap;
    for (int i = 0; i < n; i++) {
        grown = *cap;
        if (!rb_grow(cols[i], &grown, need))
            return false;                            /* (a column grown before this one is merely longer than *cap says) */
    }
    *cap = grown;
    return true;
}

/* ---- the served window: rows [first, first + count) of `total` are on the host, row `next` is the one to serve */
typedef struct GsWindow {
    uint64_t next, first, count;
} GsWindow;

static inline bool gs_win_has(const GsWindow *w) { return w->next < w->first + w->count; }
static inline uint64_t gs_win_at(const GsWindow *w) { return w->next - w->first; }

/* rows a refill asks for: the rest from `next` on, `limit` at the most */
static inline uint64_t gs_refill(uint64_t total, uint64_t next, uint64_t limit)
{
    return total - next < limit ? total - next : limit;
}

static inline void gs_win_filled(GsWindow *w, uint64_t n)
{
    w->first = w->next;
    w->count = n;
}

/* ---- the add policy: a row that would push a batch with rows past `limit` gets a batch of its own (the open one is flushed
 * first), the row goes behind the batch's rows, and a batch that has reached the limit is flushed.  flush(self) empties the
 * batch. */
typedef bool (*gs_flush_fn)(void *self);
enum { GS_ADDED, GS_FLUSH_FAILED, GS_NO_MEMORY };

static inline int gs_add(RowBatch *b, const uint64_t *bits, uint64_t length, uint64_t limit, gs_flush_fn flush, void *self)
{
    if (rb_spills(b, length, limit) && !flush(self))
        return GS_FLUSH_FAILED;
    if (!rb_append(b, bits, length))
        return GS_NO_MEMORY;
    return !rb_full(b, limit) || flush(self) ? GS_ADDED : GS_FLUSH_FAILED;
}

/* ---- the life cycle: rows are taken until the first _next (a writer: its _finish), which runs the last step once */
typedef struct GsLife {
    bool started, failed;                        /* started: the last step has been run, no row is taken any more */
} GsLife;

static inline bool gs_may_add(const GsLife *l) { return !l->started && !l->failed; }

/* at the top of every _next: false = the object has failed (now, in its last step, or before) */
static inline bool gs_serve(GsLife *l, gs_flush_fn last, void *self)
{
    if (!l->failed && !l->started) {
        l->started = true;
        l->failed = !last(self);
    }
    return !l->failed;
}

/* ---- the bytes fed to a loader and not yet accounted for */
typedef struct GsBytes {
    char *buf;
    uint64_t len, cap;
} GsBytes;

static inline bool gs_bytes_append(GsBytes *b, const char *bytes, uint64_t n)
{
    if (b->len + n > b->cap) {
        uint64_t cap = b->cap ? b->cap : 4096;
        while (cap < b->len + n)
            cap *= 2;
        char *grown = (char *)realloc(b->buf, (size_t)cap);
        if (!grown)
            return false;
        b->buf = grown;
        b->cap = cap;
    }
    if (n)
        memcpy(b->buf + b->len, bytes, (size_t)n);
    b->len += n;
    return true;
}

static inline void gs_bytes_drop(GsBytes *b, uint64_t consumed)
{
    if (consumed && b->len > consumed)
        memmove(b->buf, b->buf + consumed, (size_t)(b->len - consumed));
    b->len -= consumed;
}

/* a record did not fit into *chunk bytes: twice as many, `max` at the most; false = it is at `max` already */
static inline bool gs_chunk_grow(uint64_t *chunk, uint64_t max)
{
    if (*chunk >= max)
        return false;
    *chunk = *chunk > max / 2 ? max : 2 * *chunk;
    return true;
}

/* ---- bounds as SQL passes them: a lower bound of at least `floor`; an upper bound where a negative value is none */
static inline uint64_t gs_lower_bound(int64_t v, uint64_t floor) { return v > 0 ? (uint64_t)v : floor; }
static inline uint64_t gs_upper_bound(int64_t v) { return v < 0 ? UINT64_MAX : (uint64_t)v; }

#endif
