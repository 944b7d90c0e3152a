// index_host.hip -- the index over a stored kmer column (include/dnagpu.h: dnagpu_kmer_index_*): what the
// reference answers with CREATE INDEX ... USING spgist (kmer_sequence spgist_kmer_ops) and index scans of `=`, `^@` and `@>`
// (dna--1.0.sql:304-314, test.sql:156-270).  Build = a stable LSD radix sort of (r, row) pairs, r the base-reversed key
// (index_math.hpp); scan = the ranges of up to DNAGPU_INDEX_MAX_RANGES concrete prefixes plus a test of the positions
// behind them (index_kernels.hip).
#include "host_common.hpp"
#include "index_math.hpp"

using namespace dnagpu;

static_assert(DNAGPU_INDEX_MAX_RANGES == INDEX_MAX_RANGES, "the header's limit is the kernels'");

struct dnagpu_kmer_index {
    u64 *r = nullptr;         // n base-reversed keys, ascending (pool memory)
    u32 *row = nullptr;       // n positions in the caller's column; ascending among equal keys
    u64 n = 0;
    u64 distinct = 0;
    int k = 0;
};

namespace {

// dev_keys: the n >= 1 keys of the column in device memory (read only)
int build_core(dnagpu_ctx *ctx, const u64 *dev_keys, u64 n, int k, dnagpu_kmer_index *idx)
{
    PoolScope ps(ctx);
    u64 *r[2] = {nullptr, nullptr};
    u32 *row[2] = {nullptr, nullptr};
    for (int b = 0; b < 2; b++) {
        RC_TRY(ps.alloc((size_t)n, &r[b]));
        RC_TRY(ps.alloc((size_t)n, &row[b]));
    }
    const u64 n_hist = (u64)256 * index_sort_tiles(n);
    u32 *hist = nullptr, *scan_tmp = nullptr, *small = nullptr;
    RC_TRY(ps.alloc((size_t)n_hist, &hist));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n_hist), &scan_tmp));
    RC_TRY(ps.alloc((size_t)4, &small));                 // [0]: digits that occur; [2..3]: the distinct keys
    const int passes = (2 * k + 7) / 8;                  // the bits above 2k are zero: the last digit may be partial
    IndexSortSrc src{dev_keys, nullptr, nullptr, k};
    int cur = -1;                                        // the buffer pair that holds the pairs (-1: still the caller's keys)
    prof_begin(ctx);
    for (int p = 0; p < passes; p++) {
        prof_mark(ctx, "index_pass");
        HIP_TRY(launch_index_hist(src, n, 8 * p, hist, ctx->stream));
        HIP_TRY(launch_scan_u32(hist, hist, n_hist, scan_tmp, nullptr, ctx->stream));
        HIP_TRY(launch_index_digit_bins(hist, n, small, ctx->stream));
        u32 bins = 0;
        RC_TRY(read_back(ctx, &bins, small, 4));
        // one digit only: the scatter would copy the tile order.  (The last pass still runs if nothing has formed the
        // pairs yet: a column of one key.)
        if (bins <= 1 && !(p == passes - 1 && cur < 0))
            continue;
        const int dst = cur == 0 ? 1 : 0;
        HIP_TRY(launch_index_scatter(src, n, 8 * p, hist, r[dst], row[dst], ctx->stream));
        src = IndexSortSrc{nullptr, r[dst], row[dst], k};
        cur = dst;
    }
    prof_mark(ctx, "index_distinct");
    u64 *distinct = reinterpret_cast<u64 *>(small + 2);
    HIP_TRY(hipMemsetAsync(distinct, 0, 8, ctx->stream));
    HIP_TRY(launch_index_distinct(r[cur], n, distinct, ctx->stream));
    prof_mark(ctx, "end");
    RC_TRY(read_back(ctx, &idx->distinct, distinct, 8));
    prof_end(ctx);
    ps.release(r[cur]);
    ps.release(row[cur]);
    idx->r = r[cur];
    idx->row = row[cur];
    idx->n = n;
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

// `count` device words of two arrays to the caller's (host) arrays; waits
int copy_out(dnagpu_ctx *ctx, u64 count, const u64 *da, const u64 *db, u64 *a, u64 *b)
{
    if (a)
        HIP_TRY(hipMemcpyAsync(a, da, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (b)
        HIP_TRY(hipMemcpyAsync(b, db, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
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
    u64 *small = nullptr;
    RC_TRY(ps.alloc((size_t)R + 1, &off));
    RC_TRY(ps.alloc((size_t)R, &beg));
    RC_TRY(ps.alloc((size_t)2, &small));                 // [0]: the candidates; [1]: the matches
    prof_begin(ctx);
    prof_mark(ctx, "index_ranges");
    HIP_TRY(launch_index_ranges(idx->r, idx->n, fb, p, R, off, beg, small, ctx->stream));
    u64 C = 0;
    RC_TRY(read_back(ctx, &C, small, 8));
    if (visited)
        *visited = C;
    if (C == 0)
        return DNAGPU_OK;
    IndexScanArgs a{idx->r, idx->row, off, beg, R, (u32)C, idx->k, index_rest_is_any(fb, p) ? 0 : 1, residual_of(fb, p)};
    u64 total = C;
    u32 *tiles = nullptr;
    prof_mark(ctx, "index_count");
    if (a.test) {
        const u32 nt = index_scan_tiles(C);
        u32 *scan_tmp = nullptr;
        RC_TRY(ps.alloc((size_t)nt, &tiles));
        RC_TRY(ps.alloc((size_t)scan_tmp_words(nt), &scan_tmp));
        HIP_TRY(launch_index_sweep_count(a, tiles, ctx->stream));
        u32 *sum = reinterpret_cast<u32 *>(small + 1);
        HIP_TRY(launch_scan_u32(tiles, tiles, nt, scan_tmp, sum, ctx->stream));
        u32 t32 = 0;
        RC_TRY(read_back(ctx, &t32, sum, 4));
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
    if (out_on_device) {
        HIP_TRY(launch_index_sweep_write(a, tiles, out_rows, out_keys, nwrite, ctx->stream));
        prof_mark(ctx, "end");
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        prof_end(ctx);
        return DNAGPU_OK;
    }
    u64 *dr = nullptr, *dk = nullptr;
    if (out_rows)
        RC_TRY(ps.alloc((size_t)nwrite, &dr));
    if (out_keys)
        RC_TRY(ps.alloc((size_t)nwrite, &dk));
    HIP_TRY(launch_index_sweep_write(a, tiles, dr, dk, nwrite, ctx->stream));
    prof_mark(ctx, "end");
    const int rc = copy_out(ctx, nwrite, dr, dk, out_rows, out_keys);
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
    const u64 *dev_keys = keys;
    if (!on_device) {
        u64 *up = nullptr;
        RC_TRY(ps.alloc((size_t)n, &up));
        HIP_TRY(hipMemcpyAsync(up, keys, n * 8, hipMemcpyHostToDevice, ctx->stream));
        dev_keys = up;
    }
    RC_TRY(build_core(ctx, dev_keys, n, k, idx.get()));
    *out = idx.release();
    return DNAGPU_OK;
    });
}

extern "C" uint64_t dnagpu_kmer_index_rows(const dnagpu_kmer_index *idx) { return idx ? idx->n : 0; }
extern "C" uint64_t dnagpu_kmer_index_distinct(const dnagpu_kmer_index *idx) { return idx ? idx->distinct : 0; }
extern "C" int dnagpu_kmer_index_k(const dnagpu_kmer_index *idx) { return idx ? idx->k : 0; }

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
    if (on_device) {
        HIP_TRY(launch_index_lookup(idx->r, idx->n, idx->k, keys, m, out_first, out_count, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return DNAGPU_OK;
    }
    PoolScope ps(ctx);
    u64 *dq = nullptr, *df = nullptr, *dc = nullptr;
    RC_TRY(ps.alloc((size_t)m, &dq));
    RC_TRY(ps.alloc((size_t)m, &df));
    RC_TRY(ps.alloc((size_t)m, &dc));
    HIP_TRY(hipMemcpyAsync(dq, keys, m * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_index_lookup(idx->r, idx->n, idx->k, dq, m, df, dc, ctx->stream));
    return copy_out(ctx, m, df, dc, out_first, out_count);
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
    if (out_on_device) {
        HIP_TRY(launch_index_read(idx->r, idx->row, idx->k, first, count, out_rows, out_keys, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return DNAGPU_OK;
    }
    PoolScope ps(ctx);
    u64 *dr = nullptr, *dk = nullptr;
    if (out_rows)
        RC_TRY(ps.alloc((size_t)count, &dr));
    if (out_keys)
        RC_TRY(ps.alloc((size_t)count, &dk));
    HIP_TRY(launch_index_read(idx->r, idx->row, idx->k, first, count, dr, dk, ctx->stream));
    return copy_out(ctx, count, dr, dk, out_rows, out_keys);
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
