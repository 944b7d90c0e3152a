// index_host.hip -- the index over a stored kmer column (include/dnagpu.h: dnagpu_kmer_index_*): what the
// reference answers with CREATE INDEX ... USING spgist (kmer_sequence spgist_kmer_ops) and index scans of `=`, `^@` and `@>`
// (dna--1.0.sql:304-314, test.sql:156-270).  Build = a stable LSD radix sort of (r, row) pairs, r the base-reversed key
// (index_math.hpp); scan = the ranges of up to DNAGPU_INDEX_MAX_RANGES concrete prefixes plus a test of the positions
// behind them; append = the same sort of the batch, then one stable merge with the index; delete = a bitmap of the listed
// row ids, then one stable compaction (index_kernels.hip).  An update builds new arrays that take over when it succeeds.
#include "host_common.hpp"
#include "index_math.hpp"

using namespace dnagpu;

static_assert(DNAGPU_INDEX_MAX_RANGES == INDEX_MAX_RANGES, "the header's limit is the kernels'");

struct dnagpu_kmer_index {
    u64 *r = nullptr;         // n base-reversed keys, ascending (pool memory)
    u32 *row = nullptr;       // n row ids; ascending among equal keys
    u64 n = 0;                // entries now
    u64 next_row = 0;         // rows ever given (the build's n + every append's m): the id of the next appended row
    u64 distinct = 0;
    int k = 0;
};

namespace {

// The sort of dev_keys: the n >= 1 keys in device memory (read only), key j with row id row_base + j.  *out_r / *out_row =
// the sorted pairs, buffers of `ps`; the other buffer pair has gone back to the pool.  Every pass is labelled `mark`.
int sort_keys(dnagpu_ctx *ctx, PoolScope &ps, const u64 *dev_keys, u64 n, int k, u32 row_base, const char *mark, u64 **out_r,
              u32 **out_row)
{
    u64 *r[2] = {nullptr, nullptr};
    u32 *row[2] = {nullptr, nullptr};
    for (int b = 0; b < 2; b++) {
        RC_TRY(ps.alloc((size_t)n, &r[b]));
        RC_TRY(ps.alloc((size_t)n, &row[b]));
    }
    const int passes = (2 * k + 7) / 8;                  // the bits above 2k are zero: the last digit may be partial
    int cur = 0;
    RC_TRY(lsd_sort_pairs(ctx, IndexSortSrc{dev_keys, nullptr, nullptr, k, row_base}, n, passes, r, row, mark, &cur));
    ps.free_now(r[1 - cur]);
    ps.free_now(row[1 - cur]);
    *out_r = r[cur];
    *out_row = row[cur];
    return DNAGPU_OK;
}

// *out = the distinct keys of the sorted r[0 .. n), n >= 1; waits
int count_distinct(dnagpu_ctx *ctx, PoolScope &ps, const u64 *r, u64 n, u64 *out)
{
    u64 *distinct = nullptr;
    RC_TRY(ps.alloc((size_t)1, &distinct));
    HIP_TRY(hipMemsetAsync(distinct, 0, 8, ctx->stream));
    HIP_TRY(launch_index_distinct(r, n, distinct, ctx->stream));
    prof_mark(ctx, "end");
    RC_TRY(read_back(ctx, out, distinct, 8));
    ps.free_now(distinct);
    return DNAGPU_OK;
}

// idx takes the arrays (buffers of `ps`, or null with n == 0) over and returns its own to the pool: the hand-over of a
// build, an append and a delete, after which nothing can fail
void adopt(dnagpu_ctx *ctx, PoolScope &ps, dnagpu_kmer_index *idx, u64 *r, u32 *row, u64 n, u64 distinct)
{
    ps.release(r);
    ps.release(row);
    pool_free(ctx, idx->r);
    pool_free(ctx, idx->row);
    idx->r = r;
    idx->row = row;
    idx->n = n;
    idx->distinct = distinct;
}

// dev_keys: the n >= 1 keys of the column in device memory (read only)
int build_core(dnagpu_ctx *ctx, const u64 *dev_keys, u64 n, int k, dnagpu_kmer_index *idx)
{
    PoolScope ps(ctx);
    u64 *r = nullptr, distinct = 0;
    u32 *row = nullptr;
    prof_begin(ctx);
    RC_TRY(sort_keys(ctx, ps, dev_keys, n, k, 0, "index_pass", &r, &row));
    prof_mark(ctx, "index_distinct");
    RC_TRY(count_distinct(ctx, ps, r, n, &distinct));
    prof_end(ctx);
    adopt(ctx, ps, idx, r, row, n, distinct);
    idx->next_row = n;
    return DNAGPU_OK;
}

// dev_keys: the m >= 1 keys of the batch in device memory (read only); next_row + m <= 2^32 - 1
int append_core(dnagpu_ctx *ctx, const u64 *dev_keys, u64 m, dnagpu_kmer_index *idx)
{
    PoolScope ps(ctx);
    u64 *br = nullptr, *nr = nullptr, distinct = 0;
    u32 *brow = nullptr, *nrow = nullptr;
    prof_begin(ctx);
    RC_TRY(sort_keys(ctx, ps, dev_keys, m, idx->k, (u32)idx->next_row, "index_batch_sort", &br, &brow));
    const u64 total = idx->n + m;
    if (idx->n == 0) {                                   // nothing to merge with: the sorted batch is the index
        nr = br;
        nrow = brow;
    } else {
        u32 *part = nullptr;
        RC_TRY(ps.alloc((size_t)total, &nr));
        RC_TRY(ps.alloc((size_t)total, &nrow));
        RC_TRY(ps.alloc((size_t)index_sort_tiles(total) + 1, &part));
        prof_mark(ctx, "index_merge");
        HIP_TRY(launch_index_merge_partition(idx->r, idx->n, br, m, part, ctx->stream));
        HIP_TRY(launch_index_merge(idx->r, idx->row, idx->n, br, brow, m, part, nr, nrow, ctx->stream));
    }
    prof_mark(ctx, "index_distinct");
    RC_TRY(count_distinct(ctx, ps, nr, total, &distinct));
    prof_end(ctx);
    adopt(ctx, ps, idx, nr, nrow, total, distinct);
    idx->next_row += m;
    return DNAGPU_OK;
}

// dev_ids: the m >= 1 listed row ids in device memory (read only); the index has n >= 1 entries
int delete_core(dnagpu_ctx *ctx, const u64 *dev_ids, u64 m, dnagpu_kmer_index *idx, u64 *n_deleted)
{
    PoolScope ps(ctx);
    const u64 n = idx->n, words = index_bitmap_words(idx->next_row);
    const u32 nt = index_sort_tiles(n);
    u32 *bitmap = nullptr, *tiles = nullptr;
    RC_TRY(ps.alloc((size_t)words, &bitmap));
    prof_begin(ctx);
    prof_mark(ctx, "index_mark");
    HIP_TRY(hipMemsetAsync(bitmap, 0, words * 4, ctx->stream));
    HIP_TRY(launch_index_mark(dev_ids, m, idx->next_row, bitmap, ctx->stream));
    prof_mark(ctx, "index_compact");
    u32 kept = 0;
    RC_TRY(select_tiles(ctx, ps, nt, [&](u32 *t) { return launch_index_compact_count(idx->row, n, bitmap, t, ctx->stream); },
                        &tiles, &kept));
    if (kept > n)
        return DNAGPU_ERR_INTERNAL;
    if (kept == n || kept == 0) {                        // nothing listed is in the index / nothing is left of it
        prof_mark(ctx, "end");
        prof_end(ctx);
        if (kept == 0)
            adopt(ctx, ps, idx, nullptr, nullptr, 0, 0);
        *n_deleted = n - kept;
        return DNAGPU_OK;
    }
    u64 *nr = nullptr, distinct = 0;
    u32 *nrow = nullptr;
    RC_TRY(ps.alloc((size_t)kept, &nr));
    RC_TRY(ps.alloc((size_t)kept, &nrow));
    HIP_TRY(launch_index_compact_write(idx->r, idx->row, n, bitmap, tiles, nr, nrow, kept, ctx->stream));
    prof_mark(ctx, "index_distinct");
    RC_TRY(count_distinct(ctx, ps, nr, kept, &distinct));
    prof_end(ctx);
    adopt(ctx, ps, idx, nr, nrow, kept, distinct);
    *n_deleted = n - kept;
    return DNAGPU_OK;
}

// the residual test: positions p .. k-1 of fb as deny planes (filter_match)
FilterDev residual_of(const FilterBits &fb, int p)
{
    FilterDev fd;
    memset(&fd, 0, sizeof fd);
    fd.use_planes = 1;
    for (int i = p; i < fb.k; i++) {
        const u32 set = index_set_at(fb, i);
        for (int c = 0; c < 4; c++)
            if (!(set & (1u << c)))
                fd.deny[c] |= (u64)1 << (2 * i);
    }
    return fd;
}

int scan_core(dnagpu_ctx *ctx, const dnagpu_kmer_index *idx, const FilterBits &fb, u64 *out_rows, u64 *out_keys, u64 cap,
              u64 *n_out, u64 *visited, int out_on_device)
{
    u32 R = 0;
    const int p = index_prune_depth(fb, &R);
    if (R == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    u32 *off = nullptr, *beg = nullptr;
    u64 *cand = nullptr;
    RC_TRY(ps.alloc((size_t)R + 1, &off));
    RC_TRY(ps.alloc((size_t)R, &beg));
    RC_TRY(ps.alloc((size_t)1, &cand));                  // the candidates
    prof_begin(ctx);
    prof_mark(ctx, "index_ranges");
    HIP_TRY(launch_index_ranges(idx->r, idx->n, fb, p, R, off, beg, cand, ctx->stream));
    u64 C = 0;
    RC_TRY(read_back(ctx, &C, cand, 8));
    if (visited)
        *visited = C;
    if (C == 0)
        return DNAGPU_OK;
    IndexScanArgs a{idx->r, idx->row, off, beg, R, (u32)C, idx->k, index_rest_is_any(fb, p) ? 0 : 1, residual_of(fb, p)};
    u64 total = C;
    u32 *tiles = nullptr;
    prof_mark(ctx, "index_count");
    if (a.test) {
        u32 t32 = 0;
        RC_TRY(select_tiles(ctx, ps, index_scan_tiles(C), [&](u32 *t) { return launch_index_sweep_count(a, t, ctx->stream); },
                            &tiles, &t32));
        total = t32;
    }
    *n_out = total;
    const u64 nwrite = std::min(total, cap);
    if (nwrite == 0 || (!out_rows && !out_keys)) {
        prof_mark(ctx, "end");
        prof_end(ctx);
        return DNAGPU_OK;
    }
    prof_mark(ctx, "index_write");
    OutCols<2> o;
    RC_TRY(o.init(ctx, ps, {out_rows, out_keys}, nwrite, out_on_device));
    HIP_TRY(launch_index_sweep_write(a, tiles, o.dev(0), o.dev(1), nwrite, ctx->stream));
    prof_mark(ctx, "end");
    const int rc = o.finish();
    prof_end(ctx);
    return rc;
}

}  // namespace

extern "C" int dnagpu_kmer_index_build(dnagpu_ctx *ctx, const uint64_t *keys, uint64_t n, int k, int on_device,
                                       dnagpu_kmer_index **out)
{
    return guarded([&]() -> int {
    if (out)
        *out = nullptr;
    if (k < 1 || k > 32)
        return DNAGPU_ERR_INVALID_K;
    if (!ctx || !out || (n && !keys))
        return DNAGPU_ERR_BAD_ARG;
    if (n > 0xFFFFFFFFull)                           // row ids are 32-bit; refused before any device work
        return DNAGPU_ERR_TOO_LARGE;
    std::unique_ptr<dnagpu_kmer_index> idx(new dnagpu_kmer_index());
    idx->k = k;
    if (n == 0) {                                    // a valid index of 0 rows that holds no device memory
        *out = idx.release();
        return DNAGPU_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    const u64 *dev_keys = nullptr;
    RC_TRY(device_list(ctx, ps, keys, n, on_device, &dev_keys));
    RC_TRY(build_core(ctx, dev_keys, n, k, idx.get()));
    *out = idx.release();
    return DNAGPU_OK;
    });
}

extern "C" uint64_t dnagpu_kmer_index_rows(const dnagpu_kmer_index *idx) { return idx ? idx->n : 0; }
extern "C" uint64_t dnagpu_kmer_index_distinct(const dnagpu_kmer_index *idx) { return idx ? idx->distinct : 0; }
extern "C" int dnagpu_kmer_index_k(const dnagpu_kmer_index *idx) { return idx ? idx->k : 0; }

extern "C" uint64_t dnagpu_kmer_index_next_row(const dnagpu_kmer_index *idx) { return idx ? idx->next_row : 0; }

extern "C" int dnagpu_kmer_index_append(dnagpu_ctx *ctx, dnagpu_kmer_index *idx, const uint64_t *keys, uint64_t m, int on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !idx || (m && !keys))
        return DNAGPU_ERR_BAD_ARG;
    if (m > 0xFFFFFFFFull || idx->next_row + m > 0xFFFFFFFFull)      // row ids are 32-bit; refused before any device work
        return DNAGPU_ERR_TOO_LARGE;
    if (m == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    const u64 *dev_keys = nullptr;
    RC_TRY(device_list(ctx, ps, keys, m, on_device, &dev_keys));
    return append_core(ctx, dev_keys, m, idx);
    });
}

extern "C" int dnagpu_kmer_index_delete(dnagpu_ctx *ctx, dnagpu_kmer_index *idx, const uint64_t *rows, uint64_t m, int on_device,
                                        uint64_t *n_deleted)
{
    return guarded([&]() -> int {
    if (n_deleted)
        *n_deleted = 0;
    if (!ctx || !idx || (m && !rows))
        return DNAGPU_ERR_BAD_ARG;
    if (m > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    if (m == 0 || idx->n == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    const u64 *dev_ids = nullptr;
    RC_TRY(device_list(ctx, ps, rows, m, on_device, &dev_ids));
    u64 gone = 0;
    RC_TRY(delete_core(ctx, dev_ids, m, idx, &gone));
    if (n_deleted)
        *n_deleted = gone;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_kmer_index_scan(dnagpu_ctx *ctx, const dnagpu_kmer_index *idx, const dnagpu_filter *filter,
                                      uint64_t *out_rows, uint64_t *out_keys, uint64_t cap, uint64_t *n_out, uint64_t *visited,
                                      int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !idx || !n_out || !filter)
        return DNAGPU_ERR_BAD_ARG;
    FilterBits fb;
    bool none = false;
    int op_error = DNAGPU_OK;
    RC_TRY(build_filter_bits(filter, idx->k, &fb, &none, &op_error));     // a malformed filter is always an error
    *n_out = 0;
    if (visited)
        *visited = 0;
    if (idx->n == 0)
        return DNAGPU_OK;
    RC_TRY(op_error);                                // the operator's own ERROR: only when a row reaches it
    if (none)
        return DNAGPU_OK;
    return scan_core(ctx, idx, fb, out_rows, out_keys, cap, n_out, visited, out_on_device);
    });
}

extern "C" int dnagpu_kmer_index_lookup(dnagpu_ctx *ctx, const dnagpu_kmer_index *idx, const uint64_t *keys, uint64_t m,
                                        uint64_t *out_first, uint64_t *out_count, int on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !idx || (m && (!keys || !out_first || !out_count)))
        return DNAGPU_ERR_BAD_ARG;
    if (m > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    if (m == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    const u64 *dq = nullptr;
    OutCols<2> o;
    RC_TRY(device_list(ctx, ps, keys, m, on_device, &dq));
    RC_TRY(o.init(ctx, ps, {out_first, out_count}, m, on_device));
    HIP_TRY(launch_index_lookup(idx->r, idx->n, idx->k, dq, m, o.dev(0), o.dev(1), ctx->stream));
    return o.finish();
    });
}

extern "C" int dnagpu_kmer_index_read(dnagpu_ctx *ctx, const dnagpu_kmer_index *idx, uint64_t first, uint64_t count,
                                      uint64_t *out_rows, uint64_t *out_keys, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !idx)
        return DNAGPU_ERR_BAD_ARG;
    if (first > idx->n || count > idx->n - first)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0 || (!out_rows && !out_keys))
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    OutCols<2> o;
    RC_TRY(o.init(ctx, ps, {out_rows, out_keys}, count, out_on_device));
    HIP_TRY(launch_index_read(idx->r, idx->row, idx->k, first, count, o.dev(0), o.dev(1), ctx->stream));
    return o.finish();
    });
}

extern "C" void dnagpu_kmer_index_free(dnagpu_ctx *ctx, dnagpu_kmer_index *idx)
{
    if (!idx)
        return;
    if (ctx) {
        pool_free(ctx, idx->r);
        pool_free(ctx, idx->row);
    }
    delete idx;
}
