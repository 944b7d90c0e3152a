// host_steps.hip -- the host-side steps that several features of the C-ABI drive the same way (declared in host_common.hpp,
// "host_steps.hip"): the LSD pair sort of the index and of the equal sequences, the scan that hands its total back, the
// hand-out of u64 columns to host or device memory, the widening of a u32 array.  No kernel of its own.
#include "host_common.hpp"

namespace dnagpu {

int lsd_sort_pairs(dnagpu_ctx *ctx, IndexSortSrc src, u64 n, int passes, u64 *const key[2], u32 *const val[2], const char *mark,
                   int *sorted)
{
    PoolScope ps(ctx);
    const u64 n_hist = (u64)256 * index_sort_tiles(n);
    u32 *hist = nullptr, *scan_tmp = nullptr, *bins_dev = nullptr;
    RC_TRY(ps.alloc((size_t)n_hist, &hist));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n_hist), &scan_tmp));
    RC_TRY(ps.alloc((size_t)2, &bins_dev));              // [0]: digits that occur
    int cur = src.keys ? -1 : 0;                         // the buffer pair that holds the pairs (-1: still the caller's keys)
    for (int p = 0; p < passes; p++) {
        if (mark)
            prof_mark(ctx, mark);
        HIP_TRY(launch_index_hist(src, n, 8 * p, hist, ctx->stream));
        HIP_TRY(launch_scan_u32(hist, hist, n_hist, scan_tmp, nullptr, ctx->stream));
        HIP_TRY(launch_index_digit_bins(hist, n, bins_dev, ctx->stream));
        u32 bins = 0;
        RC_TRY(read_back(ctx, &bins, bins_dev, 4));
        // one digit only: the scatter would copy the tile order.  (The last pass still runs if nothing has formed the
        // pairs yet: a column of one key.)
        if (bins <= 1 && !(p == passes - 1 && cur < 0))
            continue;
        const int dst = cur == 0 ? 1 : 0;
        HIP_TRY(launch_index_scatter(src, n, 8 * p, hist, key[dst], val[dst], ctx->stream));
        src = IndexSortSrc{nullptr, key[dst], val[dst], src.k, 0};
        cur = dst;
    }
    *sorted = cur;
    return DNAGPU_OK;
}

int scan_total(dnagpu_ctx *ctx, u32 *arr, u64 n, u32 *scan_tmp, u32 *total)
{
    HIP_TRY(launch_scan_u32(arr, arr, n, scan_tmp, arr + n, ctx->stream));
    return read_back(ctx, total, arr + n, sizeof *total);
}

int copy_cols(dnagpu_ctx *ctx, const ColCopy *cols, int n_cols, u64 n, int out_on_device)
{
    const hipMemcpyKind kind = out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    for (int i = 0; i < n_cols; i++)
        if (n && cols[i].out)
            HIP_TRY(hipMemcpyAsync(cols[i].out, cols[i].dev, (size_t)n * 8, kind, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
}

int widen_out(dnagpu_ctx *ctx, PoolScope &ps, const u32 *src, u64 n, u64 *out, int out_on_device)
{
    if (!out)
        return DNAGPU_OK;
    if (out_on_device) {
        HIP_TRY(launch_hits_widen(src, out, n, ctx->stream));
        return DNAGPU_OK;
    }
    u64 *stage = nullptr;
    RC_TRY(ps.alloc((size_t)n, &stage));
    HIP_TRY(launch_hits_widen(src, stage, n, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, stage, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    return DNAGPU_OK;
}

}  // namespace dnagpu
