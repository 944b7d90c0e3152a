// profile_host.hip -- dnagpu_table_profile of include/dnagpu.h: the k-mer profile of every sequence of a window of a table
// (profile_kernels.hip).  The argument rules, the plan / scan of the items, the two counting kernels, and the
// staged copy of the host form.
#include "host_common.hpp"
#include "profile_math.hpp"

using namespace dnagpu;

namespace {

int profile_run(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, bool canonical, u64 seq_first, u64 n, u32 *out_counts,
                u64 *out_rows, bool out_on_device)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    const u64 cells = n * profile_width(k);                // (n < 2^32, W <= 2^12)
    u32 *counts = out_counts;
    u64 *rows = out_rows;
    if (!out_on_device) {                                  // every buffer first: an error leaves the outputs untouched
        RC_TRY(ps.alloc((size_t)cells, &counts));
        if (out_rows)
            RC_TRY(ps.alloc((size_t)n, &rows));
    }
    u32 *items = nullptr, *scan_tmp = nullptr;
    RC_TRY(ps.alloc((size_t)n + 1, &items));               // (the last word: the total)
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n), &scan_tmp));

    const u64 *starts = dna->seq_starts + seq_first;
    HIP_TRY(launch_profile_plan(starts, n, k, rows, items, st));
    HIP_TRY(launch_scan_u32(items, items, n, scan_tmp, items + n, st));   // (not scan_total: the wave kernel is queued before the wait)
    HIP_TRY(launch_profile_wave(dna->words, dna->n_words, starts, n, k, canonical ? 1 : 0, counts, st));
    u32 n_items = 0;
    RC_TRY(read_back(ctx, &n_items, items + n, sizeof n_items));
    HIP_TRY(launch_profile_tile(dna->words, dna->n_words, starts, n, items, n_items, k, canonical ? 1 : 0, counts, st));
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(out_counts, counts, (size_t)cells * 4, hipMemcpyDeviceToHost, st));
        if (out_rows)
            HIP_TRY(hipMemcpyAsync(out_rows, rows, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return DNAGPU_OK;                                      // (the scratch and staging arrays go back to the pool here)
}

}  // namespace

extern "C" uint64_t dnagpu_profile_width(int k) { return profile_width(k); }

extern "C" int dnagpu_profile_geometry(uint64_t *wave_rows, uint64_t *tile_rows)
{
    if (wave_rows)
        *wave_rows = PROFILE_WAVE_ROWS;
    if (tile_rows)
        *tile_rows = PROFILE_TILE_ROWS;
    return DNAGPU_OK;
}

extern "C" int dnagpu_table_profile(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, unsigned flags, uint64_t seq_first,
                                    uint64_t seq_count, uint32_t *out_counts, uint64_t *out_rows, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !dna)
        return DNAGPU_ERR_BAD_ARG;
    if (flags > DNAGPU_PROFILE_CANONICAL)
        return DNAGPU_ERR_BAD_ARG;
    if (k < 1 || k > 32)
        return DNAGPU_ERR_INVALID_K;
    if (k > DNAGPU_PROFILE_MAX_K) {
        set_err("a dense profile has 4^k columns and is offered for k <= %d; k = %d needs a sparse (id, kmer, count) result",
                DNAGPU_PROFILE_MAX_K, k);
        return DNAGPU_ERR_TOO_LARGE;
    }
    if (seq_first > dna->n_seqs || seq_count > dna->n_seqs - seq_first)
        return DNAGPU_ERR_BAD_ARG;
    if (seq_count > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;                       // (more sequences than bases allows: all but 2^32 - 1 are empty)
    if (table_without_set(dna))
        return DNAGPU_ERR_BAD_ARG;
    if (seq_count == 0)
        return DNAGPU_OK;
    if (!out_counts)
        return DNAGPU_ERR_BAD_ARG;
    return profile_run(ctx, dna, k, (flags & DNAGPU_PROFILE_CANONICAL) != 0, seq_first, seq_count, out_counts, out_rows,
                       out_on_device != 0);
    });
}
