// hits_host.hip -- dnagpu_table_hits and the dnagpu_seq_hits object of include/dnagpu.h: per-sequence hits of a table's k-mers
// in a counted set (hits_kernels.hip).  The argument rules, the window's size limit, the sweep / scan / gather
// of the build, and the hand-out of the two arrays (read) and of the sequences that pass a threshold (select).
#include "host_common.hpp"
#include "hits_math.hpp"

using namespace dnagpu;

namespace {

bool has_table(const dnagpu_acc *a)
{
    return a->distinct != 0 && a->t.pbits != 0 && a->t.table && a->t.occ;
}

int hits_build(dnagpu_ctx *ctx, const dnagpu_dna *dna, const dnagpu_acc *set, bool canonical, u64 lo, u64 hi, dnagpu_seq_hits *h)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    // the window's two ends (one 16-byte copy) and, behind them, the three totals
    u64 *small = nullptr;
    RC_TRY(ps.alloc(5, &small));
    HIP_TRY(launch_hits_bounds(dna->seq_starts, h->first, h->n, small, st));
    u64 ends[2] = {0, 0};
    RC_TRY(read_back(ctx, ends, small, sizeof ends));
    const u64 a0 = ends[0], n = ends[1] - ends[0];
    if (n > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;               // (dnagpu_generate_kmers_table's per-call rule: the u32 arrays stay exact)
    unsigned long long *totals = reinterpret_cast<unsigned long long *>(small + 2);
    HIP_TRY(hipMemsetAsync(totals, 0, 3 * 8, st));
    u32 *rows = nullptr, *hits = nullptr;
    RC_TRY(ps.alloc((size_t)h->n, &rows));
    RC_TRY(ps.alloc((size_t)h->n, &hits));

    // the sweep, unless no row can hit: no table, no count in [lo, hi], no stream row of k bases
    u32 *mask = nullptr, *word_pre = nullptr, *tile = nullptr, *scan_tmp = nullptr;
    if (has_table(set) && lo <= hi && hits_stream_rows(n, h->k) != 0) {
        const u64 n_mw = hits_mask_words(n), tiles = hits_tiles(n);
        RC_TRY(ps.alloc((size_t)n_mw, &mask));
        RC_TRY(ps.alloc((size_t)n_mw, &word_pre));
        RC_TRY(ps.alloc((size_t)tiles, &tile));
        RC_TRY(ps.alloc((size_t)scan_tmp_words(tiles), &scan_tmp));
        const HitsWindow w = {dna->words, dna->n_words, dna->seq_marks, dna->n_mark_words, a0, n, h->k, canonical ? 1 : 0};
        const HitsSet s = {set->t.table, set->t.occ, set->t.pbits, lo, hi, small};     // (small[0 .. 1]: the window's ends)
        HIP_TRY(launch_hits_sweep(w, s, mask, word_pre, tile, st));
        HIP_TRY(launch_scan_u32(tile, tile, tiles, scan_tmp, nullptr, st));
    }
    HIP_TRY(launch_hits_gather(dna->seq_starts + h->first, h->n, a0, h->k, mask, word_pre, tile, rows, hits, totals, st));
    u64 t3[3] = {0, 0, 0};
    RC_TRY(read_back(ctx, t3, totals, sizeof t3));   // (waits for the stream: the object is complete)
    h->tot_rows = t3[0];
    h->tot_hits = t3[1];
    h->tot_seqs_hit = t3[2];
    ps.release(rows);
    ps.release(hits);
    h->rows = rows;
    h->hits = hits;
    return DNAGPU_OK;                                // (the scratch arrays go back to the pool here)
}

}  // namespace

extern "C" int dnagpu_table_hits(dnagpu_ctx *ctx, const dnagpu_dna *dna, const dnagpu_acc *set, unsigned flags, uint64_t min_count,
                                 uint64_t max_count, uint64_t seq_first, uint64_t seq_count, dnagpu_seq_hits **out)
{
    return guarded([&]() -> int {
    if (flags > DNAGPU_HITS_CANONICAL)
        return DNAGPU_ERR_BAD_ARG;                   // (the range before the missing object)
    if (!ctx || !dna || !set || !out)
        return DNAGPU_ERR_BAD_ARG;
    *out = nullptr;
    if (table_without_set(dna))
        return DNAGPU_ERR_BAD_ARG;
    if (seq_first > dna->n_seqs || seq_count > dna->n_seqs - seq_first)
        return DNAGPU_ERR_BAD_ARG;
    std::unique_ptr<dnagpu_seq_hits> h(new dnagpu_seq_hits());
    h->n = seq_count;
    h->first = seq_first;
    h->k = set->k;
    if (seq_count != 0) {
        if (seq_count > U32_MAX64)
            return DNAGPU_ERR_TOO_LARGE;             // (more sequences than bases allows: all but 2^32 - 1 of them are empty)
        RC_TRY(hits_build(ctx, dna, set, (flags & DNAGPU_HITS_CANONICAL) != 0, min_count ? min_count : 1, max_count, h.get()));
    }
    *out = h.release();
    return DNAGPU_OK;
    });
}

extern "C" uint64_t dnagpu_seq_hits_sequences(const dnagpu_seq_hits *h) { return h ? h->n : 0; }
extern "C" uint64_t dnagpu_seq_hits_first(const dnagpu_seq_hits *h) { return h ? h->first : 0; }
extern "C" int dnagpu_seq_hits_k(const dnagpu_seq_hits *h) { return h ? h->k : 0; }
extern "C" const uint32_t *dnagpu_seq_hits_device_rows(const dnagpu_seq_hits *h) { return h ? h->rows : nullptr; }
extern "C" const uint32_t *dnagpu_seq_hits_device_hits(const dnagpu_seq_hits *h) { return h ? h->hits : nullptr; }

extern "C" int dnagpu_seq_hits_totals(const dnagpu_seq_hits *h, uint64_t *rows, uint64_t *hits, uint64_t *seqs_hit)
{
    if (!h)
        return DNAGPU_ERR_BAD_ARG;
    if (rows)
        *rows = h->tot_rows;
    if (hits)
        *hits = h->tot_hits;
    if (seqs_hit)
        *seqs_hit = h->tot_seqs_hit;
    return DNAGPU_OK;
}

extern "C" int dnagpu_seq_hits_read(dnagpu_ctx *ctx, const dnagpu_seq_hits *h, uint64_t first, uint64_t count, uint64_t *out_rows,
                                    uint64_t *out_hits, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !h)
        return DNAGPU_ERR_BAD_ARG;
    if (first > h->n || count > h->n - first)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0 || (!out_rows && !out_hits))
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    RC_TRY(widen_out(ctx, ps, h->rows + first, count, out_rows, out_on_device));
    RC_TRY(widen_out(ctx, ps, h->hits + first, count, out_hits, out_on_device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_seq_hits_select(dnagpu_ctx *ctx, const dnagpu_seq_hits *h, uint64_t min_hits, uint64_t max_hits,
                                      uint64_t frac_num, uint64_t frac_den, uint64_t *out_seq, uint64_t *out_rows,
                                      uint64_t *out_hits, uint64_t cap, uint64_t *n_out, int out_on_device)
{
    return guarded([&]() -> int {
    if (frac_den == 0 || frac_den > U32_MAX64 || frac_num > U32_MAX64)
        return DNAGPU_ERR_BAD_ARG;                   // (the range before the missing object; the products stay exact in 64 bits)
    if (!ctx || !h || !n_out)
        return DNAGPU_ERR_BAD_ARG;
    *n_out = 0;
    if (h->n == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    const HitsPredicate p = {min_hits, max_hits, frac_num, frac_den};
    u32 *tiles = nullptr, total = 0;
    RC_TRY(select_tiles(ctx, ps, hits_select_tiles(h->n),
                        [&](u32 *t) { return launch_hits_select_count(h->rows, h->hits, h->n, p, t, st); }, &tiles, &total));
    *n_out = total;
    const u64 n_write = std::min<u64>(total, cap);
    if (n_write == 0 || (!out_seq && !out_rows && !out_hits))
        return DNAGPU_OK;
    OutCols<3> o;
    RC_TRY(o.init(ctx, ps, {out_seq, out_rows, out_hits}, n_write, out_on_device));
    HIP_TRY(launch_hits_select_write(h->rows, h->hits, h->n, p, tiles, h->first, o.dev(0), o.dev(1), o.dev(2), n_write, st));
    return o.finish();
    });
}

extern "C" void dnagpu_seq_hits_free(dnagpu_ctx *ctx, dnagpu_seq_hits *h)
{
    if (!h)
        return;
    if (ctx) {
        pool_free(ctx, h->rows);
        pool_free(ctx, h->hits);
    }
    delete h;
}
