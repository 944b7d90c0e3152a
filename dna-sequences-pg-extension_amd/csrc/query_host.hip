// query_host.hip -- the read-only queries over counted groups of include/dnagpu.h: dnagpu_hist_* / dnagpu_acc_* spectrum,
// select, top and rank (query_kernels.hip).  Every query runs over a GroupSet -- the parts of a histogram, or
// the accumulator's table -- and leaves it as it is.
#include "host_common.hpp"

using namespace dnagpu;

// every group in count order: two dense pool arrays of `rows` words each (none when rows == 0)
struct dnagpu_ranking {
    u64 rows = 0;
    int order = DNAGPU_ORDER_COUNT_DESC;
    u64 *keys = nullptr;
    u64 *counts = nullptr;
};

namespace {

struct GroupSet {
    std::vector<QHistSrc> hist;       // the parts of a histogram that hold slots
    bool is_acc = false;
    QAccSrc acc{};
    bool is_dense = false;            // dense rows (the tail of a ranking)
    QDenseSrc dense{};
    u64 distinct = 0;

    template <typename F>
    hipError_t each(F &&f) const
    {
        if (is_acc)
            return f(acc);
        if (is_dense)
            return f(dense);
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
    if (!out_on_device)                              // host outputs: staged in pool buffers (no more rows than there are groups)
        cap = std::min(cap, g.distinct);
    OutCols<2> o;
    RC_TRY(o.init(ctx, ps, {out_keys, out_counts}, cap, out_on_device));
    RC_TRY(select_into(ctx, g, lo, hi, o.dev(0), o.dev(1), cap, cursor));
    u64 total = 0;
    RC_TRY(read_back(ctx, &total, cursor, 8));       // (waits for the stream: device outputs are complete)
    *n_out = total;
    if (!out_on_device)
        RC_TRY(o.finish(std::min(total, cap)));
    return DNAGPU_OK;
}

// The count T of the n-th group in count-descending order (1 <= n <= distinct) and *n_above = the groups with a count above
// T: an MSD radix select over 11-bit digits of the count.  The first pass takes the lowest digit of every group and the
// largest count: counts below Q_DIGITS (the typical input) are settled by it; else the digits are walked from the largest
// count's top digit down, each pass restricted to the prefix the passes before it chose, one read-back per pass.
// *n_equal (may be null) = the groups with count == T.
int top_threshold(dnagpu_ctx *ctx, PoolScope &ps, const GroupSet &g, u64 n, u64 *T, u64 *n_above, u64 *n_equal = nullptr)
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
        if (n_equal)
            *n_equal = bins[prefix];
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
        if (n_equal)
            *n_equal = bins[d];                      // (exact after the last pass: every digit of T is fixed)
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
    RC_TRY(copy_cols(ctx, {{sk, out_keys}, {sc, out_counts}}, rows, out_on_device));
    *n_out = rows;
    return DNAGPU_OK;
}

// ---- rank: a counting sort by count class (DESIGN.md 4.10 "Rank")
constexpr u64 RANK_CLASSES = Q_DIGITS;               // counts below it are a class each; from it on: the tail
constexpr u64 RANK_CHUNK = (u64)1 << 20;             // most rows one sort takes (launch_query_sort's network: DNAGPU_TOP_MAX)

// The n rows at tk / tc (any order) put in count-descending order in place.  Up to `chunk` rows are one sort.  More are peeled
// from the largest counts down over a copy of the rows (a dense group source): the radix select finds the count T of the
// chunk-th row still to place, the rows above T (fewer than a chunk) are selected, sorted and placed, the whole class
// count == T follows unsorted (ties are unspecified), and the peel goes on below T.  Every peel places at least a chunk of
// rows and costs a few passes over the whole copy: the cost grows with (n / chunk)^2.
int order_tail(dnagpu_ctx *ctx, PoolScope &ps, u64 *tk, u64 *tc, u64 n, u64 chunk)
{
    if (n < 2)
        return DNAGPU_OK;
    hipStream_t st = ctx->stream;
    u64 m_cap = 2;
    while (m_cap < std::min(n, chunk))
        m_cap <<= 1;
    u64 *sk = nullptr, *sc = nullptr;
    RC_TRY(ps.alloc((size_t)m_cap, &sk));
    RC_TRY(ps.alloc((size_t)m_cap, &sc));
    // rows [0, rows) of the staging arrays sorted (the padding behind them sorts last) and copied to dk / dc
    auto sort_to = [&](u64 rows, u64 *dk, u64 *dc) -> int {
        u64 m = 2;
        while (m < rows)
            m <<= 1;
        if (m > rows) {
            HIP_TRY(hipMemsetAsync(sk + rows, 0xFF, (size_t)(m - rows) * 8, st));
            HIP_TRY(hipMemsetAsync(sc + rows, 0, (size_t)(m - rows) * 8, st));
        }
        HIP_TRY(launch_query_sort(sk, sc, (u32)m, st));
        HIP_TRY(hipMemcpyAsync(dk, sk, (size_t)rows * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(dc, sc, (size_t)rows * 8, hipMemcpyDeviceToDevice, st));
        return DNAGPU_OK;
    };
    if (n <= chunk) {
        HIP_TRY(hipMemcpyAsync(sk, tk, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(sc, tc, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
        return sort_to(n, tk, tc);
    }
    u64 *xk = nullptr, *xc = nullptr, *cursor = nullptr;
    RC_TRY(ps.alloc((size_t)n, &xk));
    RC_TRY(ps.alloc((size_t)n, &xc));
    RC_TRY(ps.alloc(1, &cursor));
    HIP_TRY(hipMemcpyAsync(xk, tk, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(xc, tc, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    GroupSet d;
    d.is_dense = true;
    d.dense = QDenseSrc{xk, xc, n};
    d.distinct = n;
    u64 done = 0, hi = ~(u64)0;                      // rows placed = the rows with a count above hi
    while (done < n) {
        const u64 rem = n - done;
        HIP_TRY(hipMemsetAsync(cursor, 0, 8, st));
        if (rem <= chunk) {
            RC_TRY(select_into(ctx, d, 1, hi, sk, sc, rem, cursor));
            RC_TRY(sort_to(rem, tk + done, tc + done));
            break;
        }
        u64 T = 0, n_above = 0, n_equal = 0;
        RC_TRY(top_threshold(ctx, ps, d, done + chunk, &T, &n_above, &n_equal));
        if (T == 0 || T > hi || n_above < done || n_above - done >= chunk || n_equal > n - n_above ||
            n_above + n_equal < done + chunk) {
            set_err("rank: peel at %llu of %llu rows: T = %llu, %llu above, %llu equal", (unsigned long long)done,
                    (unsigned long long)n, (unsigned long long)T, (unsigned long long)n_above, (unsigned long long)n_equal);
            return DNAGPU_ERR_INTERNAL;
        }
        if (n_above > done) {                        // (so T < hi: T + 1 does not wrap)
            RC_TRY(select_into(ctx, d, T + 1, hi, sk, sc, n_above - done, cursor));
            RC_TRY(sort_to(n_above - done, tk + done, tc + done));
            HIP_TRY(hipMemsetAsync(cursor, 0, 8, st));
        }
        RC_TRY(select_into(ctx, d, T, T, tk + n_above, tc + n_above, n_equal, cursor));
        done = n_above + n_equal;
        hi = T - 1;
    }
    return DNAGPU_OK;
}

int rank_core(dnagpu_ctx *ctx, const GroupSet &g, int order, dnagpu_ranking **out)
{
    std::unique_ptr<dnagpu_ranking> r(new dnagpu_ranking());
    r->order = order;
    if (g.distinct == 0) {
        *out = r.release();
        return DNAGPU_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const bool small = (ctx->debug_flags & DNAGPU_DEBUG_RANK_SMALL) != 0;
    const u64 C = small ? 4 : RANK_CLASSES, chunk = small ? 2048 : RANK_CHUNK;
    // sizes: bins[c - 1] = the groups of class c < C, bins[C - 1] = the tail
    std::vector<u64> bins((size_t)C);
    RC_TRY(spectrum_core(ctx, g, C, bins.data()));
    u64 rows = 0;
    for (u64 b : bins)
        rows += b;
    if (rows != g.distinct) {
        set_err("rank: %llu groups in the classes, %llu counted", (unsigned long long)rows, (unsigned long long)g.distinct);
        return DNAGPU_ERR_INTERNAL;
    }
    // every class's first row: DESC = the tail, then classes C - 1 .. 1; ASC = the mirror image
    std::vector<u64> first((size_t)C + 1, 0), ends((size_t)C + 1, 0);
    u64 at = 0;
    for (u64 i = 0; i < C; i++) {
        const u64 cls = order == DNAGPU_ORDER_COUNT_DESC ? C - i : i + 1;
        first[cls] = at;
        at += bins[cls - 1];
        ends[cls] = at;
    }
    PoolScope ps(ctx);
    u64 *rk = nullptr, *rc = nullptr, *cursors = nullptr;
    RC_TRY(ps.alloc((size_t)rows, &rk));
    RC_TRY(ps.alloc((size_t)rows, &rc));
    RC_TRY(ps.alloc((size_t)C + 1, &cursors));
    HIP_TRY(hipMemcpyAsync(cursors, first.data(), (size_t)(C + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (g.is_acc)
        HIP_TRY(launch_query_rank_scatter(g.acc, (u32)C, cursors, rk, rc, rows, ctx->stream));
    for (const QHistSrc &h : g.hist)                 // (several parts go on from the same cursors)
        HIP_TRY(launch_query_rank_scatter(h, (u32)C, cursors, rk, rc, rows, ctx->stream));
    std::vector<u64> got((size_t)C + 1);
    RC_TRY(read_back(ctx, got.data(), cursors, (size_t)(C + 1) * 8));
    for (u64 cls = 1; cls <= C; cls++)
        if (got[cls] != ends[cls]) {
            set_err("rank: class %llu took %llu rows, its size is %llu", (unsigned long long)cls,
                    (unsigned long long)(got[cls] - first[cls]), (unsigned long long)bins[cls - 1]);
            return DNAGPU_ERR_INTERNAL;
        }
    const u64 n_tail = bins[C - 1];
    RC_TRY(order_tail(ctx, ps, rk + first[C], rc + first[C], n_tail, chunk));
    if (order == DNAGPU_ORDER_COUNT_ASC)             // (the tail is in place, largest first: turned round)
        HIP_TRY(launch_query_reverse(rk + first[C], rc + first[C], n_tail, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ps.release(rk);
    ps.release(rc);
    r->rows = rows;
    r->keys = rk;
    r->counts = rc;
    *out = r.release();
    return DNAGPU_OK;
}

// the order's range comes first, as a size's does below
template <typename Obj>
int rank_entry(dnagpu_ctx *ctx, const Obj *o, int order, dnagpu_ranking **out)
{
    if (out)
        *out = nullptr;
    if (order != DNAGPU_ORDER_COUNT_DESC && order != DNAGPU_ORDER_COUNT_ASC)
        return DNAGPU_ERR_BAD_ARG;
    if (!ctx || !o || !out)
        return DNAGPU_ERR_BAD_ARG;
    return rank_core(ctx, groups_of(o), order, out);
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

extern "C" int dnagpu_hist_rank(dnagpu_ctx *ctx, const dnagpu_hist *h, int order, dnagpu_ranking **out)
{
    return guarded([&]() -> int { return rank_entry(ctx, h, order, out); });
}

extern "C" int dnagpu_acc_rank(dnagpu_ctx *ctx, const dnagpu_acc *acc, int order, dnagpu_ranking **out)
{
    return guarded([&]() -> int { return rank_entry(ctx, acc, order, out); });
}

extern "C" uint64_t dnagpu_ranking_rows(const dnagpu_ranking *r) { return r ? r->rows : 0; }
extern "C" int dnagpu_ranking_order(const dnagpu_ranking *r) { return r ? r->order : DNAGPU_ORDER_COUNT_DESC; }
extern "C" const uint64_t *dnagpu_ranking_device_keys(const dnagpu_ranking *r) { return r ? r->keys : nullptr; }
extern "C" const uint64_t *dnagpu_ranking_device_counts(const dnagpu_ranking *r) { return r ? r->counts : nullptr; }

extern "C" int dnagpu_ranking_read(dnagpu_ctx *ctx, const dnagpu_ranking *r, uint64_t first, uint64_t count, uint64_t *out_keys,
                                   uint64_t *out_counts, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !r)
        return DNAGPU_ERR_BAD_ARG;
    if (first > r->rows || count > r->rows - first)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0 || (!out_keys && !out_counts))
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    return copy_cols(ctx, {{r->keys + first, out_keys}, {r->counts + first, out_counts}}, count, out_on_device);
    });
}

extern "C" void dnagpu_ranking_free(dnagpu_ctx *ctx, dnagpu_ranking *r)
{
    if (!r)
        return;
    if (ctx) {
        pool_free(ctx, r->keys);
        pool_free(ctx, r->counts);
    }
    delete r;
}
