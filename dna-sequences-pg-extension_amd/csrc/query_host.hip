// query_host.hip -- the read-only queries over counted groups of include/dnagpu.h: dnagpu_hist_* / dnagpu_acc_* spectrum,
// select and top (query_kernels.hip).  Every query runs over a GroupSet -- the parts of a histogram, or
// the accumulator's table -- and leaves it as it is.
#include "host_common.hpp"

using namespace dnagpu;

namespace {

struct GroupSet {
    std::vector<QHistSrc> hist;       // the parts of a histogram that hold slots
    bool is_acc = false;
    QAccSrc acc{};
    u64 distinct = 0;

    template <typename F>
    hipError_t each(F &&f) const
    {
        if (is_acc)
            return f(acc);
        for (const QHistSrc &h : hist) {
            const hipError_t e = f(h);
            if (e != hipSuccess)
                return e;
        }
        return hipSuccess;
    }
};

GroupSet groups_of(const dnagpu_hist *h)
{
    GroupSet g;
    g.distinct = h->n_distinct;
    const dnagpu_hist *const one[1] = {h};
    const dnagpu_hist *const *parts = h->parts.empty() ? one : h->parts.data();
    const size_t n_parts = h->parts.empty() ? 1 : h->parts.size();
    for (size_t i = 0; i < n_parts; i++) {
        const dnagpu_hist *p = parts[i];
        const u64 n = p->extent ? p->extent : p->n_distinct;
        if (n && p->keys && p->counts)
            g.hist.push_back(QHistSrc{p->keys, p->counts, n});
    }
    return g;
}

GroupSet groups_of(const dnagpu_acc *a)
{
    GroupSet g;
    g.is_acc = true;
    g.distinct = a->distinct;
    if (a->distinct)
        g.acc = QAccSrc{a->t.table, a->t.occ, ((u64)1 << a->t.pbits) * ACC_SLOTS};
    return g;
}

int spectrum_core(dnagpu_ctx *ctx, const GroupSet &g, u64 n_bins, u64 *bins)
{
    if (g.distinct == 0) {
        memset(bins, 0, (size_t)n_bins * 8);
        return DNAGPU_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    QDigit a{};
    a.spectrum = 1;
    a.n_bins = n_bins;
    a.lds_bins = (u32)std::min<u64>(std::max<u64>(n_bins, 4), Q_LDS_BINS);
    const u64 words = std::max<u64>(n_bins, a.lds_bins);
    u64 *dev = nullptr;
    RC_TRY(ps.alloc((size_t)words, &dev));
    HIP_TRY(hipMemsetAsync(dev, 0, (size_t)words * 8, ctx->stream));
    HIP_TRY(g.each([&](const auto &s) { return launch_query_digits(s, a, dev, nullptr, ctx->stream); }));
    return read_back(ctx, bins, dev, (size_t)n_bins * 8);
}

// appends the groups with lo <= count <= hi behind *cursor
int select_into(dnagpu_ctx *ctx, const GroupSet &g, u64 lo, u64 hi, u64 *dk, u64 *dc, u64 cap, u64 *cursor)
{
    HIP_TRY(g.each([&](const auto &s) { return launch_query_select(s, lo, hi, dk, dc, cap, cursor, ctx->stream); }));
    return DNAGPU_OK;
}

// rows [0, n) of two device arrays to the caller's (host, or device) arrays; waits for the stream
int hand_out(dnagpu_ctx *ctx, u64 n, const u64 *dk, const u64 *dc, u64 *out_keys, u64 *out_counts, int out_on_device)
{
    const hipMemcpyKind kind = out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (n && out_keys)
        HIP_TRY(hipMemcpyAsync(out_keys, dk, (size_t)n * 8, kind, ctx->stream));
    if (n && out_counts)
        HIP_TRY(hipMemcpyAsync(out_counts, dc, (size_t)n * 8, kind, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
}

int select_core(dnagpu_ctx *ctx, const GroupSet &g, u64 lo, u64 hi, u64 *out_keys, u64 *out_counts, u64 cap, u64 *n_out,
                int out_on_device)
{
    *n_out = 0;
    lo = std::max<u64>(lo, 1);
    if (lo > hi || g.distinct == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    u64 *cursor = nullptr;
    RC_TRY(ps.alloc(1, &cursor));
    HIP_TRY(hipMemsetAsync(cursor, 0, 8, ctx->stream));
    u64 *dk = out_keys, *dc = out_counts;
    if (!out_on_device) {                            // host outputs: staged in pool buffers (no more rows than there are groups)
        cap = std::min(cap, g.distinct);
        dk = dc = nullptr;
        if (cap && out_keys)
            RC_TRY(ps.alloc((size_t)cap, &dk));
        if (cap && out_counts)
            RC_TRY(ps.alloc((size_t)cap, &dc));
    }
    RC_TRY(select_into(ctx, g, lo, hi, dk, dc, cap, cursor));
    u64 total = 0;
    RC_TRY(read_back(ctx, &total, cursor, 8));       // (waits for the stream: device outputs are complete)
    *n_out = total;
    if (!out_on_device)
        RC_TRY(hand_out(ctx, std::min(total, cap), dk, dc, out_keys, out_counts, 0));
    return DNAGPU_OK;
}

// The count T of the n-th group in count-descending order (1 <= n <= distinct) and *n_above = the groups with a count above
// T: an MSD radix select over 11-bit digits of the count.  The first pass takes the lowest digit of every group and the
// largest count: counts below Q_DIGITS (the typical input) are settled by it; else the digits are walked from the largest
// count's top digit down, each pass restricted to the prefix the passes before it chose, one read-back per pass.
int top_threshold(dnagpu_ctx *ctx, PoolScope &ps, const GroupSet &g, u64 n, u64 *T, u64 *n_above)
{
    u64 *dev = nullptr;
    RC_TRY(ps.alloc(Q_DIGITS + 1, &dev));            // (the last word: the largest count)
    std::vector<u64> bins(Q_DIGITS + 1);
    auto pass = [&](const QDigit &a) -> int {
        HIP_TRY(hipMemsetAsync(dev, 0, (Q_DIGITS + 1) * 8, ctx->stream));
        HIP_TRY(g.each([&](const auto &s) { return launch_query_digits(s, a, dev, dev + Q_DIGITS, ctx->stream); }));
        return read_back(ctx, bins.data(), dev, (Q_DIGITS + 1) * 8);
    };
    // the bin that holds the r-th group from the top; r becomes its rank inside the bin, *n_above grows by the bins above
    auto walk = [&](u64 &r, u64 *bin) -> int {
        u64 above = 0;
        for (int b = Q_DIGITS - 1; b >= 0; b--) {
            if (above + bins[b] >= r) {
                *bin = (u64)b;
                r -= above;
                *n_above += above;
                return DNAGPU_OK;
            }
            above += bins[b];
        }
        set_err("top: the digit histogram holds %llu groups, %llu wanted", (unsigned long long)above, (unsigned long long)r);
        return DNAGPU_ERR_INTERNAL;
    };
    QDigit a{};
    a.lds_bins = Q_DIGITS;
    a.want_max = 1;
    RC_TRY(pass(a));
    const u64 max_count = bins[Q_DIGITS];
    u64 r = n, prefix = 0;
    *n_above = 0;
    if (max_count < (u64)Q_DIGITS) {
        RC_TRY(walk(r, &prefix));
        *T = prefix;
        return DNAGPU_OK;
    }
    const int top = (63 - __builtin_clzll((unsigned long long)max_count)) / 11;
    a.want_max = 0;
    for (int j = top; j >= 0; j--) {
        a.shift = 11 * j;
        a.has_prefix = j != top;
        a.prefix_shift = a.has_prefix ? 11 * (j + 1) : 0;
        a.prefix = prefix;
        RC_TRY(pass(a));
        u64 d = 0;
        RC_TRY(walk(r, &d));
        prefix = prefix << 11 | d;
    }
    *T = prefix;
    return DNAGPU_OK;
}

int top_core(dnagpu_ctx *ctx, const GroupSet &g, u64 n, u64 *out_keys, u64 *out_counts, u64 *n_out, int out_on_device)
{
    *n_out = 0;
    const u64 rows = std::min(n, g.distinct);
    if (rows == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    u64 m = 2;                                       // the sort's network: a power of two; the padding rows sort last
    while (m < rows)
        m <<= 1;
    u64 *sk = nullptr, *sc = nullptr, *cursor = nullptr;
    RC_TRY(ps.alloc((size_t)m, &sk));
    RC_TRY(ps.alloc((size_t)m, &sc));
    RC_TRY(ps.alloc(1, &cursor));
    HIP_TRY(hipMemsetAsync(sk, 0xFF, (size_t)m * 8, ctx->stream));
    HIP_TRY(hipMemsetAsync(sc, 0, (size_t)m * 8, ctx->stream));      // (count 0: behind every group)
    HIP_TRY(hipMemsetAsync(cursor, 0, 8, ctx->stream));
    if (rows == g.distinct) {                        // every group: the whole ORDER BY count(*) DESC
        RC_TRY(select_into(ctx, g, 1, ~(u64)0, sk, sc, rows, cursor));
    } else {
        u64 T = 0, n_above = 0;
        RC_TRY(top_threshold(ctx, ps, g, rows, &T, &n_above));
        if (n_above)                                 // (so T < the largest count: T + 1 does not wrap)
            RC_TRY(select_into(ctx, g, T + 1, ~(u64)0, sk, sc, rows, cursor));
        RC_TRY(select_into(ctx, g, T, T, sk, sc, rows, cursor));     // the ties, as far as there are places left
    }
    HIP_TRY(launch_query_sort(sk, sc, (u32)m, ctx->stream));
    RC_TRY(hand_out(ctx, rows, sk, sc, out_keys, out_counts, out_on_device));
    *n_out = rows;
    return DNAGPU_OK;
}

// the argument rules the six entry points share; the range of a size comes first (dnagpu_acc_create's order), so that it
// is told apart from a missing object
template <typename Obj>
int check_spectrum(dnagpu_ctx *ctx, const Obj *o, u64 n_bins, const u64 *bins)
{
    if (n_bins < 1 || n_bins > DNAGPU_SPECTRUM_MAX_BINS || !ctx || !o || !bins)
        return DNAGPU_ERR_BAD_ARG;
    return DNAGPU_OK;
}
template <typename Obj>
int check_top(dnagpu_ctx *ctx, const Obj *o, u64 n, const u64 *n_out)
{
    if (n > DNAGPU_TOP_MAX)
        return DNAGPU_ERR_TOO_LARGE;
    if (!ctx || !o || !n_out)
        return DNAGPU_ERR_BAD_ARG;
    return DNAGPU_OK;
}

}  // namespace

extern "C" int dnagpu_hist_spectrum(dnagpu_ctx *ctx, const dnagpu_hist *h, uint64_t n_bins, uint64_t *bins)
{
    return guarded([&]() -> int {
    RC_TRY(check_spectrum(ctx, h, n_bins, bins));
    return spectrum_core(ctx, groups_of(h), n_bins, bins);
    });
}

extern "C" int dnagpu_acc_spectrum(dnagpu_ctx *ctx, const dnagpu_acc *acc, uint64_t n_bins, uint64_t *bins)
{
    return guarded([&]() -> int {
    RC_TRY(check_spectrum(ctx, acc, n_bins, bins));
    return spectrum_core(ctx, groups_of(acc), n_bins, bins);
    });
}

extern "C" int dnagpu_hist_select(dnagpu_ctx *ctx, const dnagpu_hist *h, uint64_t min_count, uint64_t max_count,
                                  uint64_t *out_keys, uint64_t *out_counts, uint64_t cap, uint64_t *n_out, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !h || !n_out)
        return DNAGPU_ERR_BAD_ARG;
    return select_core(ctx, groups_of(h), min_count, max_count, out_keys, out_counts, cap, n_out, out_on_device);
    });
}

extern "C" int dnagpu_acc_select(dnagpu_ctx *ctx, const dnagpu_acc *acc, uint64_t min_count, uint64_t max_count,
                                 uint64_t *out_keys, uint64_t *out_counts, uint64_t cap, uint64_t *n_out, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !acc || !n_out)
        return DNAGPU_ERR_BAD_ARG;
    return select_core(ctx, groups_of(acc), min_count, max_count, out_keys, out_counts, cap, n_out, out_on_device);
    });
}

extern "C" int dnagpu_hist_top(dnagpu_ctx *ctx, const dnagpu_hist *h, uint64_t n, uint64_t *out_keys, uint64_t *out_counts,
                               uint64_t *n_out, int out_on_device)
{
    return guarded([&]() -> int {
    RC_TRY(check_top(ctx, h, n, n_out));
    return top_core(ctx, groups_of(h), n, out_keys, out_counts, n_out, out_on_device);
    });
}

extern "C" int dnagpu_acc_top(dnagpu_ctx *ctx, const dnagpu_acc *acc, uint64_t n, uint64_t *out_keys, uint64_t *out_counts,
                              uint64_t *n_out, int out_on_device)
{
    return guarded([&]() -> int {
    RC_TRY(check_top(ctx, acc, n, n_out));
    return top_core(ctx, groups_of(acc), n, out_keys, out_counts, n_out, out_on_device);
    });
}
