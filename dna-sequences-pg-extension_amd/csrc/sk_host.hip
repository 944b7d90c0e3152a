// sk_host.hip -- the host driver of the super-k-mer ("record") engine: geometry, level 0, levels 1-2, the tail that
// counts the final buckets, and the entry points of the record exchange.  Host side only.
// A count fills one SkParts stage by stage: level 0 (sk_level0, or the slab sweep: sk_slab_*), levels 1-2 (sk_levels12: the
// sk_l1_* stages, sk_heavy_take, sk_level2; behind a slab sweep sk_levels012_slab runs them, level 1 beside the sweep where
// that pays: sk_l01_piped) and the tail (count_sk_tail: the sk_tail_* stages over one SkTail).
#include "host_common.hpp"

using namespace dnagpu;

// ---- super-k-mer engine (sk_device.hpp, sk_*_kernels.hip): the partition passes move 16-byte records of ~9 k-mers
// instead of 8-byte keys, and a final bucket is counted from its records in an LDS hash table: no key of it is
// ever written to HBM.

// Planned k-mers per final bucket: ~770 quads of four k-mers -- 1024 (sk_count's threads: the buckets with copies) is
// 4 sigma above, so next to no bucket takes the expansion path (A/B on one box, 3 Gbase: 2700 18.7 - 18.8 ms, 2500 18.2,
// 2300 18.1 - 18.4).
constexpr u64 SK_LEAF_MEAN = 2500;
// A mid bucket of more than SK_MID_LIMIT k-mers (planned: 16 x SK_LEAF_MEAN) is "heavy" and leaves the record path for the
// expansion; below that it is regrouped like the others, and its long final buckets (thousands to millions of copies of a
// few k-mers) are what sk_count_big is for.
constexpr u64 SK_MID_LIMIT = (u64)1 << 27;
// A mid bucket of more than SK_MID_RECORDS records is heavy too: it is regrouped by ONE workgroup, tile after tile,
// twice, and beyond eight tiles the chunked split (sk_heavy_take), many workgroups per bucket, is faster -- 249 Mbase of
// a tiled 1000-base motif: sk_regroup 0.64 ms at 2^19, sk_heavy_split 0.31 at 2^16.
#ifndef SK_MID_RECORDS_LOG2
#define SK_MID_RECORDS_LOG2 16
#endif
constexpr u32 SK_MID_RECORDS = 1u << SK_MID_RECORDS_LOG2;
// Final buckets beyond SK_BIG_LIMIT k-mers are expanded without trying sk_count_big.
constexpr u64 SK_BIG_LIMIT = 0xFFFFFFFFull;
// Level 1 splits a coarse bucket 512 ways, not 1024: a tile of 8192 records then leaves in runs of 16 records (256
// bytes) instead of 8 -- sk_scatter1 3.6 - 3.9 instead of 4.9 - 5.2 ms at 3 Gbase (A/B on one box) -- and level 0 takes
// the bit over (136 coarse buckets at 3 Gbase: its 16-byte stores still combine in L2, 2.2 MB of open lines per XCD).
constexpr int SK_B1_MAX = 9;
// From this many rows level 0 runs without its histogram sweep (sk_slab_begin).  Measured, slabs vs the exact pair:
// 249 Mbase 2.16 vs 2.12 ms, 1 Gbase 8.31 vs 8.42, 3 Gbase 21.8 vs 22.4.
constexpr u64 SK_SLAB_MIN_ROWS = (u64)1 << 29;

// ---- small helpers
// pool memory for at least one element: max(n, 1) * per elements (an empty list still gets a valid pointer)
template <typename T>
static int alloc1(PoolScope &ps, size_t n, T **out, size_t per = 1)
{
    return ps.alloc(std::max<size_t>(n, 1) * per, out);
}

// The length of a chunk of a chunked level over x rows or records: ~`target` chunks of whole tiles, four tiles at least.
static u32 sk_chunk_len(u64 x, u64 target = 4096, u64 tile = 8192)
{
    const u64 len = std::max<u64>(4 * tile, (x + target - 1) / target);
    return (u32)((len + tile - 1) / tile * tile);
}

// exclusive scans in[a] -> out[a] at a time (launch_scan_u32_multi): the sum of in[a] goes to totals[a]
static ScanSet scan_set(std::initializer_list<u32 *> in, std::initializer_list<u32 *> out, u32 *totals, u32 *tmp)
{
    ScanSet ss;
    memset(&ss, 0, sizeof ss);
    for (size_t a = 0; a < in.size(); a++) {
        ss.in[a] = in.begin()[a];
        ss.out[a] = out.begin()[a];
        ss.total[a] = totals + a;
    }
    ss.tmp = tmp;
    return ss;
}

struct SkLevel {                                 // what one forced partition level leaves behind
    Node *next;
    u32 n_next;
    u32 *hist, *tot;
    Chunk *chunks;
    u32 n_chunks;
};

// plan (forced split on `bits` bits) + chunk list + histogram tables of one level over `cur`
static int sk_level_begin(dnagpu_ctx *ctx, PoolScope &ps, Node *cur, u32 n_nodes, int bits, u32 chunk_len, SkLevel *lv)
{
    hipStream_t st = ctx->stream;
    u32 *outc = nullptr, *nch = nullptr, *scan_tmp = nullptr;
    LevelCounters *ctr = nullptr;
    RC_TRY(ps.alloc(n_nodes, &outc));
    RC_TRY(ps.alloc(n_nodes, &nch));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n_nodes), &scan_tmp));
    RC_TRY(ps.alloc(1, &ctr));
    HIP_TRY(launch_plan_level(cur, n_nodes, -bits, chunk_len, outc, nch, scan_tmp, ctr, st));
    LevelCounters hc;
    RC_TRY(read_back(ctx, &hc, ctr, sizeof hc));
    lv->n_next = hc.n_next;
    lv->n_chunks = hc.n_chunks;
    RC_TRY(alloc1(ps, hc.n_chunks, &lv->chunks));
    RC_TRY(alloc1(ps, hc.n_chunks, &lv->hist, ROW_STRIDE));
    RC_TRY(alloc1(ps, hc.n_chunks, &lv->tot, ROW_STRIDE));
    RC_TRY(alloc1(ps, hc.n_next, &lv->next));
    HIP_TRY(launch_fill_chunks(cur, n_nodes, chunk_len, outc, nch, cur, lv->chunks, st));
    // (outc / nch / scan_tmp / ctr go back to the pool when the scope ends: later users queue behind this stream)
    return DNAGPU_OK;
}

// Heavy mid buckets (more than SK_MID_LIMIT k-mers or SK_MID_RECORDS records: the minimizers of repeats) that were taken
// out of the record path as a whole, for the tail's expansion.
struct SkHeavy {
    Node *nodes = nullptr;      // device, n entries: start / len in records, child_base = k-mers (if counted)
    u32 n = 0;
    bool counted = true;        // child_base holds the bucket's k-mers (checked against its expansion)
    void *recs = nullptr;       // the record buffer they live in
    u64 total = 0;              // k-mers of all
};

// The state of one record count, filled stage by stage; all device memory is pool memory of the count's one PoolScope.
struct SkParts {
    // ---- inputs
    SkGeom g;
    int k = 0;
    u64 n_expected = 0;         // the k-mers the records must hold (0 = not known: records received from other ranks)
    // ---- level 0 (sk_level0, sk_slab_begin, or count_sk_received for records that arrive)
    void *rec0 = nullptr;       // the records, coarse bucket after coarse bucket
    u64 rec0_cap = 0;           // the records rec0 has room for
    u64 n_recs = 0;             // records (after the slab sweep: slots, NULL records included)
    Node *coarse = nullptr;     // the 2^r0bits coarse nodes (device; start / len in records, in digit order)
    u32 n_coarse = 0;
    std::vector<u32> lens;      // their record counts on the host; empty = not known: level 1 then takes its exact route
    // ---- levels 1-2 (sk_levels12)
    void *recs = nullptr;       // the record buffer holding the final buckets
    Node *fin = nullptr;        // their nodes: start / len in records, child_base = k-mers
    u32 n_fin = 0;
    SkHeavy heavy;
    u64 n_kmers = 0;            // the k-mers found
};

SkGeom dnagpu::sk_geometry(const dnagpu_ctx *ctx, u64 n, int k)
{
    SkGeom g;
    // short windows make short runs ((k - m + 2) / 2 k-mers per record on random sequence): the buckets shrink with them
    // so that a bucket's records (~450) still fit sk_count's 512-record stage
    const u64 leaf_mean = std::min<u64>(SK_LEAF_MEAN, 225 * (u64)(k - sk_minimizer_len(k) + 2));
    const u64 n_final = std::max<u64>(n / leaf_mean, 16);
    const u64 n_mid = (n_final + 15) / 16;
    g.b1 = 1;
    while (g.b1 < SK_B1_MAX && ((u64)1 << g.b1) < n_mid)
        g.b1++;
    g.c0n = (u32)std::min<u64>((n_mid + ((u64)1 << g.b1) - 1) >> g.b1, (u64)sk_max_c0());
    g.r0bits = 1;
    while ((1u << g.r0bits) < g.c0n)
        g.r0bits++;
    // (the forced engine of the tests calls a bucket heavy at three times the mean, so that short sequences take that path too)
    g.mid_limit = (ctx->debug_flags & DNAGPU_DEBUG_FORCE_SUPERKMER) ? 3 * (n / ((u64)g.c0n << g.b1) + 1) : SK_MID_LIMIT;
    return g;
}

// Are the coarse buckets even?  lens[i] = the records of bucket i.  Even: the largest bucket holds at most `tol` times the
// mean of the non-empty ones, plus 64 records (big * used <= tol * total + 64 * used; no records at all are even).
// span_out (optional): the slots a speculative level 1 needs for these buckets (sk_spec_span with b1 bits).
static bool sk_even(const u32 *lens, u32 n, double tol, int b1 = 0, u64 *span_out = nullptr)
{
    u64 tot = 0, big = 0, used = 0, span = 0;
    for (u32 i = 0; i < n; i++) {
        tot += lens[i];
        big = std::max<u64>(big, lens[i]);
        used += lens[i] ? 1 : 0;
        if (span_out)
            span += sk_spec_span(lens[i], b1);
    }
    if (span_out)
        *span_out = span;
    return (double)big * (double)used <= tol * (double)tot + 64.0 * (double)used;
}

// What both front ends of level 0 start with: the root node over n rows (*cur_out, device), chunks of whole tiles so that
// the rows make ~chunk_target of them (*chunk_rows_out), and the plan of the forced split on r0bits bits (*l0).
static int sk_level0_begin(dnagpu_ctx *ctx, PoolScope &ps, u64 n, int r0bits, u64 chunk_target, Node **cur_out, u32 *chunk_rows_out,
                           SkLevel *l0)
{
    Node root;
    memset(&root, 0, sizeof root);
    root.len = (u32)n;
    root.meta = 32;                              // "remaining bits" of the bucket digits: r0bits + b1 <= 20 of them are split on
    Node *cur = nullptr;
    RC_TRY(ps.alloc(1, &cur));
    HIP_TRY(poke(cur, &root, sizeof root, ctx->stream));
    const u32 chunk_rows = sk_chunk_len(n, chunk_target, (u64)sk_tile_rows());
    prof_mark(ctx, "sk_plan0");
    RC_TRY(sk_level_begin(ctx, ps, cur, 1, r0bits, chunk_rows, l0));
    *cur_out = cur;
    *chunk_rows_out = chunk_rows;
    return DNAGPU_OK;
}

// Level 0, the exact pair (histogram sweep, scatter sweep): the rows of the packed sequence -> records in the coarse
// buckets of p.g.  Fills the level-0 part of p; p.lens = the buckets' exact record counts.
// room_for_level1: rec0 is made large enough for the regions of a level 1 without its histogram (sk_l1_route).
static int sk_level0(dnagpu_ctx *ctx, PoolScope &ps, SkParts &p, const SkRows &rows, bool room_for_level1)
{
    hipStream_t st = ctx->stream;
    const dnagpu_dna *dna = rows.dna;
    const int k = p.k, b1 = p.g.b1, r0bits = p.g.r0bits;
    const u32 c0n = p.g.c0n;
    Node *cur = nullptr;
    u32 chunk_rows = 0;
    SkLevel l0;
    RC_TRY(sk_level0_begin(ctx, ps, rows.n, r0bits, 4096, &cur, &chunk_rows, &l0));
    prof_mark(ctx, "sk_hist0");
    HIP_TRY(launch_sk_level0(false, l0.chunks, l0.n_chunks, dna->words, dna->n_words, rows.first, k, c0n, (u32)b1, (u32)r0bits,
                             l0.hist, nullptr, nullptr, st, nullptr, rows.marks, rows.n_mark_words));
    prof_mark(ctx, "sk_prefix0");
    HIP_TRY(launch_level_prefix(cur, l0.chunks, l0.n_chunks, 1, chunk_rows, l0.hist, l0.tot, st));
    HIP_TRY(launch_level_children(cur, 1, l0.tot, l0.next, nullptr, nullptr, nullptr, 0, st));
    std::vector<Node> kids(l0.n_next);
    RC_TRY(read_back(ctx, kids.data(), l0.next, (size_t)l0.n_next * sizeof(Node)));
    std::vector<u32> &lens = p.lens;
    lens.resize(kids.size());
    u64 n_recs = 0;
    for (size_t i = 0; i < kids.size(); i++) {
        lens[i] = kids[i].len;
        n_recs += kids[i].len;
    }
    if (n_recs > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    void *rec0 = nullptr;
    u64 cap = std::max<u64>(n_recs, 1);
    if (room_for_level1) {
        u64 span = 0;
        const bool even = sk_even(lens.data(), (u32)lens.size(), 1.02, b1, &span);
        if (span <= 0xFFFFFFFFull)
            cap = std::max(cap, span);
        // uneven coarse buckets (repeats): level 1's regions will come from a sampled histogram (sk_l1_route), ~20 % of
        // slack on an ordinary mid bucket: room for a third more than the records
        if ((ctx->debug_flags & DNAGPU_DEBUG_SAMPLE1) || !even) {
            const u64 roomy = n_recs + n_recs / 3 + ((u64)lens.size() << b1) * 136;
            if (roomy <= 0xFFFFFFFFull)
                cap = std::max(cap, roomy);
        }
    }
    RC_TRY(pool_alloc(ctx, (size_t)cap * 16, &rec0));
    ps.ptrs.push_back(rec0);
    prof_mark(ctx, "sk_scatter0");
    HIP_TRY(launch_sk_level0(true, l0.chunks, l0.n_chunks, dna->words, dna->n_words, rows.first, k, c0n, (u32)b1, (u32)r0bits,
                             l0.hist, l0.tot, rec0, st, nullptr, rows.marks, rows.n_mark_words));
    p.rec0 = rec0;
    p.rec0_cap = cap;
    p.coarse = l0.next;
    p.n_coarse = l0.n_next;
    p.n_recs = n_recs;
    return DNAGPU_OK;
}

// Level 0 WITHOUT its histogram sweep (the window minima are computed once): a histogram over 1/64 of the rows (chunks of
// four tiles, evenly spaced) gives every coarse bucket's share of a chunk's records; every chunk then reserves that share
// + 1/32 + six standard deviations + 24 slots in the bucket's region (one returning add per digit and chunk) and fills
// them as the exact sweep fills its histogram ranges; what it does not use becomes NULL records, which level 1 skips
// (~10 % of the slots at 3 Gbase).
// Every chunk adds cap[d] to digit d's cursor, whatever it finds, so after the first c chunks of the chunk list the records
// of digit d are the slots [start[d], start[d] + c cap[d]) of its region -- known on the host before anything runs, with
// no read-back.  The sweep may therefore run in several launches over consecutive ranges of its chunks (sk_slab_piece),
// all on the one slab table, and level 1 can start on a piece's records while the next piece is cut (sk_l01_piped).
//
// A PIPELINED sweep has SK_L0_PIECES pieces of 512 chunks each: two workgroups of sk_scatter0 per CU (half of what fits)
// leave the registers and the LDS for one workgroup of sk_scatter1 beside them -- the only mix of the two that fits a CU; a
// full set of 1024 leaves no room, and level 1 then only starts as the sweep drains.  At half its waves, and with a
// neighbour, a piece runs at ~2/3 of the sweep's rate: at 3 Gbase level 0 takes 5.9 ms instead of 4.2, and hides 2.3 of
// level 1's 3.25 ms (a kernel trace: pieces of 1.15, 1.57, 1.57, 1.56 ms, level 1 beside the last three 1.53 - 1.55 ms
// each, its last piece 0.86 ms alone).  Measured on one box (ms per step, two runs each; before: 17.83 / 17.84): 1024 chunks
// in 2 pieces 17.56 / 17.57, 2048 in 4 17.27 / 17.30, 3072 in 6 17.36 / 17.48 (shorter chunks: more slack per slab, more
// NULL records), 2048 in 2 -- full sets -- 17.97 / 17.99, 1024 in 1 17.88 / 18.02.
// It pays from SK_PIPE_MIN_ROWS rows of ONE sequence only.  The unpipelined sweep costs 1.07 ms per Grow at 0.6 and 1.2 Gbase
// but 1.25 at 2 and 1.4 at 3 Gbase (more coarse buckets: more open lines per workgroup), the pieces ~2.0 at every size:
// levels 0 + 1 side by side against one after the other, one box, 0.6 Gbase 1.49 vs 1.31 ms, 1.2 Gbase 2.71 vs 2.57,
// 2 Gbase 4.83 vs 4.71, 3 Gbase 6.86 vs 7.46.  A table of 150-base reads (1.5 Gbase) lost more, 3.55 vs 3.11: tables are
// not pipelined.  (DNAGPU_DEBUG_SLAB0 / _SLAB0_OVERFLOW pipeline every length, tables too: the tests.)
#ifndef SK_L0_PIECES_N
#define SK_L0_PIECES_N 4
#endif
constexpr u32 SK_L0_PIECES = SK_L0_PIECES_N;
constexpr u64 SK_PIPE_MIN_ROWS = (u64)5 << 29;
// The chunks of a sweep.  Unpipelined: 1024, one resident set of workgroups -- a chunk's share of a bucket is then ~2,400
// records at 3 Gbase, and the six standard deviations of slack it needs are 12 % of them (with the exact pair's 4096 chunks
// they would be 25 %).  Pipelined: SK_L0_PIECES half sets (17 %).
constexpr u64 SK_SLAB_CHUNKS = 1024, SK_SLAB_CHUNKS_PIPED = 512 * SK_L0_PIECES;

// The side stream of a call, from its first launch there until the main stream has been made to wait for it, or the host
// has waited for it (joined): a return before that -- an error -- waits for it on the host, since the scope's pool memory
// goes back on return.
struct SideWork {
    hipStream_t s, main;
    bool joined = false;
    SideWork(hipStream_t side, hipStream_t main_stream) : s(side), main(main_stream) {}
    ~SideWork()
    {
        if (!joined) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamSynchronize(main);
        }
    }
};
// The events of ctx->sync_ev (side_stream): one per piece of a pipelined level 0, one for the join behind them, and one
// that orders the side stream behind the main one where the host reads something back beside the main stream's work.
constexpr size_t SK_EV_JOIN = SK_L0_PIECES, SK_EV_POST = SK_L0_PIECES + 1, SK_EVENTS = SK_L0_PIECES + 2;

// The side stream behind everything queued on the main stream so far: a read-back posted there now travels while the
// main stream goes on, and the host waits for the side stream alone (never for the main one, which is busy by then).
static int side_behind_main(dnagpu_ctx *ctx)
{
    RC_TRY(side_stream(ctx, SK_EVENTS));
    HIP_TRY(hipEventRecord(ctx->sync_ev[SK_EV_POST], ctx->stream));
    HIP_TRY(hipStreamWaitEvent(ctx->stream2, ctx->sync_ev[SK_EV_POST], 0));
    return DNAGPU_OK;
}

struct SkSlab {                     // a slab sweep that is ready to run (sk_slab_begin)
    SkLevel l0;                     // l0.chunks: the chunks of rows
    u32 *slab = nullptr;            // the slab table (see sk_scatter0_kernel)
    std::vector<u32> cap;           // per digit: the slots a chunk reserves
    u64 span = 0;                   // the slots of all regions
    bool pipe = false;              // chunked for SK_L0_PIECES pieces with level 1 beside them
};

// the chunks [*a, *b) of piece i of a pipelined sweep over n_chunks chunks: the first pieces take ceil(n_chunks / pieces) each
static void sk_piece_range(u32 n_chunks, u32 i, u32 *a, u32 *b)
{
    const u32 per = (n_chunks + SK_L0_PIECES - 1) / SK_L0_PIECES;
    *a = std::min(n_chunks, i * per);
    *b = std::min(n_chunks, (i + 1) * per);
}

// The sample, the slab table, the regions and their buffer (sl.pipe, set by the caller, decides the chunks).  *ok = false (nothing usable produced: the caller runs the exact
// pair) when the sampled buckets are uneven (repeats) or the regions pass 2^32 slots.  Else the level-0 part of p is
// filled as the sweep will leave it if no chunk runs out of slots (sk_slab_status): the coarse nodes cover their whole
// regions (p.lens[d] slots, NULL records included), p.n_recs / p.rec0_cap are slots, and rec0 belongs to ps.
static int sk_slab_begin(dnagpu_ctx *ctx, PoolScope &ps, SkParts &p, const SkRows &rows, SkSlab &sl, bool *ok)
{
    hipStream_t st = ctx->stream;
    const dnagpu_dna *dna = rows.dna;
    const SkGeom &g = p.g;
    const int k = p.k;
    const u64 first = rows.first, n = rows.n;
    *ok = false;
    const u32 r0n = 1u << g.r0bits;
    const u64 tile = (u64)sk_tile_rows();
    Node *cur = nullptr;
    u32 chunk_rows = 0;
    SkLevel &l0 = sl.l0;
    RC_TRY(sk_level0_begin(ctx, ps, n, g.r0bits, sl.pipe ? SK_SLAB_CHUNKS_PIPED : SK_SLAB_CHUNKS, &cur, &chunk_rows, &l0));
    if (l0.n_chunks == 0)
        return DNAGPU_OK;
    // ---- the sample
    const u64 samp_len = 4 * tile, samp_stride = 64 * samp_len;
    const u32 n_samp = (u32)((n + samp_stride - 1) / samp_stride);
    u64 sampled = 0;
    for (u32 i = 0; i < n_samp; i++)
        sampled += std::min<u64>(samp_len, n - (u64)i * samp_stride);
    Chunk *samp = nullptr;
    u32 *est = nullptr;
    Node *nodes = nullptr;
    RC_TRY(ps.alloc((size_t)n_samp, &samp));
    RC_TRY(ps.alloc((size_t)sk_max_c0(), &est));
    RC_TRY(ps.alloc((size_t)sk_slab_words(), &sl.slab));
    RC_TRY(ps.alloc((size_t)r0n, &nodes));
    prof_mark(ctx, "sk_sample0");
    HIP_TRY(hipMemsetAsync(est, 0, (size_t)sk_max_c0() * sizeof(u32), st));
    HIP_TRY(launch_sk_sample_chunks(samp, n_samp, (u32)samp_stride, (u32)samp_len, (u32)n, st));
    HIP_TRY(launch_sk_level0(false, samp, n_samp, dna->words, dna->n_words, first, k, g.c0n, (u32)g.b1, (u32)g.r0bits, nullptr, nullptr,
                             nullptr, st, est, rows.marks, rows.n_mark_words));
    HIP_TRY(launch_sk_slab_init(est, (u32)g.r0bits, chunk_rows, (u32)sampled, l0.n_chunks, sl.slab, nodes, st));
    std::vector<u32> h_est(r0n);
    RC_TRY(read_back(ctx, h_est.data(), est, (size_t)r0n * sizeof(u32)));
    // even buckets?  (a repeated stretch sends its records to the few buckets of its minimizers: see sk_l1_route)
    u64 tot = 0, span = 0, span1 = 0;
    std::vector<u32> lens(r0n, 0);
    sl.cap.assign(r0n, 0);
    for (u32 d = 0; d < r0n; d++) {
        tot += h_est[d];
        sl.cap[d] = sk_slab_cap(h_est[d], chunk_rows, sampled);
        const u64 len = (u64)sl.cap[d] * l0.n_chunks;
        span += len;
        if (len > 0xFFFFFFFFull)
            return DNAGPU_OK;
        lens[d] = (u32)len;
        span1 += sk_spec_span((u32)len, g.b1);
    }
    if (tot == 0 || !sk_even(h_est.data(), r0n, 1.05) || span > 0xFFFFFFFFull)
        return DNAGPU_OK;
    const u64 cap = std::max<u64>(span, span1 <= 0xFFFFFFFFull ? span1 : 0);
    void *rec0 = nullptr;
    RC_TRY(pool_alloc(ctx, (size_t)std::max<u64>(cap, 1) * 16, &rec0));
    ps.ptrs.push_back(rec0);
    sl.span = span;
    p.lens.swap(lens);
    p.rec0 = rec0;
    p.rec0_cap = cap;
    p.coarse = nodes;
    p.n_coarse = r0n;
    p.n_recs = span;
    *ok = true;
    return DNAGPU_OK;
}

// the chunks [a, b) of the sweep, on the main stream
static int sk_slab_piece(dnagpu_ctx *ctx, const SkParts &p, const SkRows &rows, const SkSlab &sl, u32 a, u32 b)
{
    const dnagpu_dna *dna = rows.dna;
    const SkGeom &g = p.g;
    const hipError_t e = launch_sk_level0(true, sl.l0.chunks + a, b - a, dna->words, dna->n_words, rows.first, p.k, g.c0n, (u32)g.b1,
                                          (u32)g.r0bits, nullptr, nullptr, p.rec0, ctx->stream, sl.slab, rows.marks, rows.n_mark_words);
    if (e != hipSuccess) {
        set_err("sk_scatter0 (slabs): %s", hipGetErrorString(e));
        return DNAGPU_ERR_HIP;
    }
    return DNAGPU_OK;
}

// the sweep's verdict from its two status words (after the LAST piece): false when a chunk ran out of slots, or the test
// flag says so
static bool sk_slab_ok(const dnagpu_ctx *ctx, const SkSlab &sl, const u32 status[2])
{
    return !status[0] && status[1] == (u32)sl.span && !(ctx->debug_flags & DNAGPU_DEBUG_SLAB0_OVERFLOW);
}

// A sweep that is not to be used after all (a chunk ran out of slots): the level-0 part of p is as it was before
// sk_slab_begin, and rec0 is free again for the exact pair (ordered behind the sweep on the main stream).
static void sk_slab_give_up(PoolScope &ps, SkParts &p)
{
    ps.free_now(p.rec0);
    p.rec0 = nullptr;
    p.rec0_cap = p.n_recs = 0;
    p.coarse = nullptr;
    p.n_coarse = 0;
    p.lens.clear();
}

// ---------------------------------------------------------------- levels 1 and 2

// The plan of level 1 (records of every coarse bucket -> 2^b1 mid buckets; k-mers per mid bucket on the way) and what its
// stages share.
struct SkL1 {
    SkLevel lv;                     // lv.next = the mid buckets' nodes
    u32 chunk_recs = 0;
    u32 *kcount = nullptr;          // k-mers per mid bucket
    u32 *d_lens = nullptr;          // records per mid bucket (+ the speculative sweep's three status words)
    u32 *gcur = nullptr;            // the mid buckets' cursors: tiles reserve their slots there
    std::vector<u32> kc, rcn;       // kcount and d_lens on the host (sk_l1_lens_to_host)
    u64 span = 0;                   // the slots of all regions of a speculative sweep
    u32 *rstart = nullptr, *rcapv = nullptr;     // SpeculativeSampled: the regions' starts and capacities
    u32 *sp = nullptr;              // Speculative: first region and slots per region of every coarse node (sk_l1_spec_begin)
    void *rec1 = nullptr;           // level 1's output buffer: the speculative sweep allocates it, else the exact scatter
    bool rec1_kept = false;         // p.heavy lives in rec1 (sk_heavy_take with DNAGPU_DEBUG_HEAVY_EXPAND): level 2 does not free it
    // level 2 launched behind the device-side gate, before the host had level 1's verdict (sk_l2_early)
    u32 *gate = nullptr;            // the gate word
    Node *fn_early = nullptr;       // the final buckets' nodes of that launch
    bool early_open = false;        // the gate was 0: the regroup ran, sk_level2 only takes fn_early over
};

// Which way level 1 goes.  With the coarse buckets' record counts on the host (p.lens) and room in rec0 (p.rec0_cap),
// level 1 runs WITHOUT its histogram where the regions fit (see sk_spec_span): mid buckets are regions of len / 2^b1 +
// 12.5 % + 72 slots, the sweep reserves slots from cursors and counts the k-mers per mid bucket itself; a region that
// overflows (repeats) sends the level through the exact stages all the same (histogram, prefix, scatter).
enum class SkL1Route {
    Exact,                  // histogram, prefix, scatter
    Speculative,            // regions sized from their coarse bucket
    SpeculativeSampled,     // regions sized from a sampled histogram (uneven coarse buckets)
};

static int sk_l1_plan(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, SkL1 &l1)
{
    hipStream_t st = ctx->stream;
    l1.chunk_recs = sk_chunk_len(p.n_recs);
    prof_mark(ctx, "sk_plan1");
    RC_TRY(sk_level_begin(ctx, ps, p.coarse, p.n_coarse, p.g.b1, l1.chunk_recs, &l1.lv));
    const u32 n_mid = l1.lv.n_next;
    RC_TRY(alloc1(ps, n_mid, &l1.kcount));
    HIP_TRY(hipMemsetAsync(l1.kcount, 0, (size_t)std::max<u32>(n_mid, 1) * sizeof(u32), st));
    RC_TRY(ps.alloc((size_t)n_mid + 4, &l1.d_lens));
    RC_TRY(alloc1(ps, l1.lv.n_chunks, &l1.gcur, ROW_STRIDE));
    l1.kc.resize(n_mid);
    l1.rcn.resize((size_t)n_mid + 4);
    return DNAGPU_OK;
}

// mid-bucket k-mer and record counts to the host (the list is short), with `extra` words behind the record counts; in
// the same wait, two more device words (more -> more_host) where the caller has some: level 0's status
// sk_l1_lens_fit: the lists go through the pinned mailbox.  Then they may travel on another stream than the main one
// (`on`: the caller has ordered it behind what writes them) and only that stream is waited for; `gate` (one more word ->
// *gate_host) travels with them.
static bool sk_l1_lens_fit(const SkL1 &l1, u32 extra)
{
    return 2 * (size_t)l1.lv.n_next * sizeof(u32) + ((size_t)extra + 3) * sizeof(u32) <= MAILBOX_BYTES - 8;
}

static int sk_l1_lens_to_host(dnagpu_ctx *ctx, SkL1 &l1, u32 extra, const u32 *more = nullptr, u32 *more_host = nullptr,
                              hipStream_t on = nullptr, const u32 *gate = nullptr, u32 *gate_host = nullptr)
{
    hipStream_t st = on ? on : ctx->stream;
    const size_t nb = (size_t)l1.lv.n_next * sizeof(u32), nb2 = nb + (size_t)extra * sizeof(u32), nb3 = more ? 2 * sizeof(u32) : 0;
    if (sk_l1_lens_fit(l1, extra)) {    // the lists through the pinned mailbox, one wait (its last word is read_back's flag)
        char *mb = reinterpret_cast<char *>(ctx->mailbox);
        HIP_TRY(hipMemcpyAsync(mb, l1.kcount, nb, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(mb + nb, l1.d_lens, nb2, hipMemcpyDeviceToHost, st));
        if (more)
            HIP_TRY(hipMemcpyAsync(mb + nb + nb2, more, nb3, hipMemcpyDeviceToHost, st));
        if (gate)
            HIP_TRY(hipMemcpyAsync(mb + nb + nb2 + nb3, gate, sizeof(u32), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        memcpy(l1.kc.data(), mb, nb);
        memcpy(l1.rcn.data(), mb + nb, nb2);
        if (more)
            memcpy(more_host, mb + nb + nb2, nb3);
        if (gate)
            memcpy(gate_host, mb + nb + nb2 + nb3, sizeof(u32));
    } else if (on || gate) {
        set_err("sk_l1_lens_to_host: lists too long for the mailbox on a side stream");
        return DNAGPU_ERR_INTERNAL;
    } else {
        HIP_TRY(hipMemcpyAsync(l1.kc.data(), l1.kcount, nb, hipMemcpyDeviceToHost, st));
        RC_TRY(read_back(ctx, l1.rcn.data(), l1.d_lens, nb2));
        if (more)
            RC_TRY(read_back(ctx, more_host, more, nb3));
    }
    return DNAGPU_OK;
}

// The route decision, taken once.  Speculative: the regions must fit both record buffers (level 2 writes a mid bucket's
// final buckets back into its range of rec0).
// Repeats show at the coarse level already: a repeated stretch sends its records to the few buckets of its minimizers
// (half a sequence of one tiled 1000-base motif doubles ~110 of 136 coarse buckets; random sequence fills them to within
// 0.3 %).  Uneven coarse buckets (2 % over the mean of the non-empty ones) do not pay for a speculative sweep that will
// overflow: their regions come from a SAMPLED histogram -- one piece of 1024 records in every eight of a coarse bucket's,
// read once (an eighth of the records: ~0.15 ms at 3 Gbase against the exact histogram's 1.0 - 1.3) -- estimate + five
// standard deviations + 128 slots per mid bucket, so that a heavy mid bucket gets a region of its size.  One more wait
// for the host (the regions' total decides the buffer); a region that overflows all the same (bursts the sample missed)
// falls back to the exact level like every speculative sweep.  Regions that do not fit rec0: Exact.
// The part of the route decision that needs no record: can level 1 be speculative at all (*any_spec), and if so, are the
// coarse buckets even, so that the regions follow from their sizes alone (*plain; l1.span = their slots)?  That is known
// from p.lens -- after a slab sweep the sizes of the coarse REGIONS, so before the first row has been cut.
static void sk_l1_route_plain(const dnagpu_ctx *ctx, const SkParts &p, SkL1 &l1, bool *any_spec, bool *plain)
{
    *any_spec = *plain = false;
    if (p.lens.empty() || (ctx->debug_flags & DNAGPU_DEBUG_NO_SPEC1) || p.n_coarse > (u32)sk_max_c0() || l1.lv.n_chunks == 0)
        return;
    u64 span = 0;
    const bool even = sk_even(p.lens.data(), p.n_coarse, 1.02, p.g.b1, &span);
    if (even && !(ctx->debug_flags & DNAGPU_DEBUG_SAMPLE1)) {
        if (span <= p.rec0_cap && span <= 0xFFFFFFFFull) {
            l1.span = span;
            *any_spec = *plain = true;
        }
        return;
    }
    *any_spec = true;
}

static int sk_l1_route(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, SkL1 &l1, SkL1Route *route)
{
    hipStream_t st = ctx->stream;
    const u32 n_coarse = p.n_coarse, n_mid = l1.lv.n_next;
    const u32 *host_lens = p.lens.data();
    *route = SkL1Route::Exact;
    bool any_spec = false, plain = false;
    sk_l1_route_plain(ctx, p, l1, &any_spec, &plain);
    if (plain)
        *route = SkL1Route::Speculative;
    if (!any_spec || plain)
        return DNAGPU_OK;
    std::vector<Chunk> samp;
    const u32 slen = sk_sample1_len(), sstep = slen * sk_sample1_every();
    for (u32 i = 0; i < n_coarse; i++)
        for (u64 off = 0; off < host_lens[i]; off += sstep) {
            Chunk c;
            c.node = i;
            c.off = (u32)off;
            c.len = (u32)std::min<u64>(slen, host_lens[i] - off);
            c.pad = 0;
            samp.push_back(c);
        }
    Chunk *d_samp = nullptr;
    u32 *est = nullptr, *stmp = nullptr, *tot1 = nullptr;
    RC_TRY(alloc1(ps, samp.size(), &d_samp));
    RC_TRY(ps.alloc((size_t)n_mid, &est));
    RC_TRY(ps.alloc((size_t)n_mid, &l1.rcapv));
    RC_TRY(ps.alloc((size_t)n_mid, &l1.rstart));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n_mid), &stmp));
    RC_TRY(ps.alloc(1, &tot1));
    prof_mark(ctx, "sk_sample1");
    if (!samp.empty())
        HIP_TRY(hipMemcpyAsync(d_samp, samp.data(), samp.size() * sizeof(Chunk), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_sk_sampled_regions(p.coarse, d_samp, (u32)samp.size(), p.rec0, n_mid, est, l1.rcapv, l1.rstart, stmp, tot1, st));
    u32 total = 0;
    RC_TRY(read_back(ctx, &total, tot1, sizeof total));      // (also: samp has been consumed)
    // (the scan's total wraps past 2^32: regions that large are out of reach of 32-bit slots anyway -- the check below
    // compares against rec0's room, which is below 2^32)
    u64 chk = 0;
    for (u32 i = 0; i < n_coarse; i++)
        chk += host_lens[i];
    if ((u64)total >= chk && (u64)total <= p.rec0_cap) {
        l1.span = total;
        *route = SkL1Route::SpeculativeSampled;
    }
    return DNAGPU_OK;
}

// The speculative sweep: no histogram.  *moved = the records are in l1.rec1 and l1.kc / l1.rcn hold the mid buckets'
// counts; false = a region overflowed (or the test flag says so): kcount is zeroed again and the exact stages run, into
// the same rec1.
// Its three steps: the regions, their cursors and the output buffer (sk_l1_spec_begin); the sweep, which may come in
// several launches over disjoint ranges of records -- they reserve from the same cursors and add to the same k-mer
// counts; the mid nodes and the verdict (sk_l1_spec_end; l0_status: see sk_l1_lens_to_host).
static int sk_l1_spec_begin(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, SkL1 &l1, SkL1Route route)
{
    const bool sampled = route == SkL1Route::SpeculativeSampled;
    RC_TRY(ps.alloc((size_t)2 * p.n_coarse, &l1.sp));
    u32 *status = l1.d_lens + l1.lv.n_next;       // [0] slots of all regions, [1] past 2^32, [2] overflow
    prof_mark(ctx, "sk_spec1");
    HIP_TRY(launch_sk_spec_regions(p.coarse, p.n_coarse, l1.sp, status, l1.gcur, ctx->stream, sampled ? l1.rstart : nullptr));
    RC_TRY(pool_alloc(ctx, (size_t)std::max<u64>(std::max(p.n_recs, l1.span), 1) * 16, &l1.rec1));
    ps.ptrs.push_back(l1.rec1);
    return DNAGPU_OK;
}

// The records of a mid bucket from which the census calls it heavy (the forced engine of the tests: never by its records)
static u32 sk_mid_rec_limit(unsigned debug_flags) { return (debug_flags & DNAGPU_DEBUG_FORCE_SUPERKMER) ? 0xFFFFFFFFu : SK_MID_RECORDS; }

// LEVEL 2 BEHIND A GATE.  Between the speculative sweep and level 2 the host reads the mid buckets' counts and decides --
// 0.2 ms at 3 Gbase in which the device ran 9 us of kernels.  On random sequence the decision is always the same: the
// sweep stands, no mid bucket is heavy or longer than a tile, and sk_regroup<false> over all of them is level 2.  So a
// one-workgroup kernel takes that decision on the device (one word: launch_sk_l1_gate), the regroup is queued right
// behind it and does nothing unless the word is 0, and the lists travel to the host on the side stream meanwhile.  The
// host recomputes the word from what it read (sk_gate_host) -- a difference is an error, never a second or a missing
// regroup -- and goes on as before; with the word 0 sk_level2 finds its work done (l1.early_open).
// The gate must be on the device: the regroup writes into rec0, which the exact level 1 that follows an overflow reads.
// Not launched early: under the debug flags that force a fall-back or the older heavy path (those paths stay as they
// were), with lists too long for the mailbox (the wait would be the main stream's), and after a level 1 with SAMPLED
// regions: uneven coarse buckets are repeats, their heavy and long mid buckets shut the gate, and a shut gate is not free
// -- the gate kernel, 75 K workgroups that return at once, the host's second pass over the lists: 3 Gbase with a tiled
// 1000-base motif, sk_scatter1's phase 2.87 - 2.95 ms before and 3.02 - 3.06 with the early launch, one box.
// (DNAGPU_DEBUG_EARLY_L2 launches early there too: the tests of the gate's verdict on such buckets.)
static bool sk_l2_early_allowed(const dnagpu_ctx *ctx, const SkL1 &l1, bool sampled)
{
    return !(ctx->debug_flags & (DNAGPU_DEBUG_SPEC1_OVERFLOW | DNAGPU_DEBUG_SLAB0_OVERFLOW | DNAGPU_DEBUG_HEAVY_EXPAND)) &&
           (!sampled || (ctx->debug_flags & DNAGPU_DEBUG_EARLY_L2)) && l1.lv.n_next > 0 && sk_l1_lens_fit(l1, 3);
}

static SkGateIn sk_gate_in(const dnagpu_ctx *ctx, const SkParts &p, const SkL1 &l1, bool sampled, const u32 *lens, const u32 *kcount,
                           const u32 *status1, const u32 *status0, u32 span0)
{
    SkGateIn gi;
    memset(&gi, 0, sizeof gi);
    gi.lens = lens;
    gi.kcount = kcount;
    gi.n_mid = l1.lv.n_next;
    gi.status1 = status1;
    gi.span1 = (u32)l1.span;
    gi.sampled = sampled ? 1u : 0u;
    gi.status0 = status0;
    gi.span0 = span0;
    gi.mid_limit = p.g.mid_limit;
    gi.n_expected = p.n_expected;
    gi.rec_limit = sk_mid_rec_limit(ctx->debug_flags);
    gi.tile = (u32)sk_regroup_tile();
    return gi;
}

// the gate word from the host's copies of what the gate kernel read (gi's pointers are host memory)
static u32 sk_gate_host(const SkGateIn &gi)
{
    u32 g = sk_gate_status(gi.status1, gi.span1, gi.sampled, gi.status0, gi.span0);
    u64 run = 0;
    for (u32 i = 0; i < gi.n_mid; i++) {
        run += gi.kcount[i];
        g |= sk_gate_bucket(gi.lens[i], gi.kcount[i], gi.mid_limit, gi.rec_limit, gi.tile);
    }
    if ((gi.n_expected != 0 && run != gi.n_expected) || run > 0xFFFFFFFFull)
        g |= SK_GATE_KMERS;
    return g;
}

// (span0: the slots level 0's slab status must report, with l0_status)
static int sk_l1_spec_end(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, SkL1 &l1, SkL1Route route, bool *moved,
                          const u32 *l0_status = nullptr, u32 *l0_status_host = nullptr, u32 span0 = 0)
{
    hipStream_t st = ctx->stream;
    const bool sampled = route == SkL1Route::SpeculativeSampled;
    const u32 n_mid = l1.lv.n_next;
    u32 *const rstart = sampled ? l1.rstart : nullptr, *const rcapv = sampled ? l1.rcapv : nullptr;
    u32 *status = l1.d_lens + n_mid;
    HIP_TRY(launch_sk_spec_nodes(p.coarse, p.n_coarse, l1.sp, l1.gcur, l1.lv.next, status + 2, st, rstart, rcapv));
    HIP_TRY(launch_sk_node_lens(l1.lv.next, n_mid, l1.d_lens, st));
    const bool early = sk_l2_early_allowed(ctx, l1, sampled);
    if (early) {
        RC_TRY(ps.alloc(1, &l1.gate));
        RC_TRY(ps.alloc((size_t)n_mid * 16, &l1.fn_early));
        HIP_TRY(launch_sk_l1_gate(sk_gate_in(ctx, p, l1, sampled, l1.d_lens, l1.kcount, status, l0_status, span0), l1.gate, st));
        RC_TRY(side_behind_main(ctx));
        SideWork side(ctx->stream2, st);
        const size_t mark_at = ctx->ev_names.size();
        prof_mark(ctx, "sk_regroup");
        HIP_TRY(launch_sk_regroup(l1.lv.next, n_mid, l1.rec1, p.rec0, l1.fn_early, false, st, l1.gate));
        u32 gate_dev = 0;
        RC_TRY(sk_l1_lens_to_host(ctx, l1, 3, l0_status, l0_status_host, side.s, l1.gate, &gate_dev));
        side.joined = true;                      // (the host has waited for the side stream)
        const u32 *stw = l1.rcn.data() + n_mid;
        const u32 gate_host =
            sk_gate_host(sk_gate_in(ctx, p, l1, sampled, l1.rcn.data(), l1.kc.data(), stw, l0_status ? l0_status_host : nullptr, span0));
        if (gate_host != gate_dev) {
            set_err("super-k-mer level 2: the device's gate word is %u, the host's verdict %u", gate_dev, gate_host);
            return DNAGPU_ERR_INTERNAL;
        }
        l1.early_open = gate_dev == 0;
        if (!l1.early_open) {                    // the launch did nothing: its phase belongs to the one before it
            if (ctx->ev_names.size() > mark_at && mark_at > 0)
                ctx->ev_names[mark_at] = ctx->ev_names[mark_at - 1];
            ps.free_now(l1.fn_early);
            l1.fn_early = nullptr;
        }
    } else {
        RC_TRY(sk_l1_lens_to_host(ctx, l1, 3, l0_status, l0_status_host));
    }
    const u32 *stw = l1.rcn.data() + n_mid;
    *moved = !((!sampled && stw[0] != (u32)l1.span) || (!sampled && stw[1]) || stw[2] ||
               (ctx->debug_flags & DNAGPU_DEBUG_SPEC1_OVERFLOW));
    if (!*moved)
        HIP_TRY(hipMemsetAsync(l1.kcount, 0, (size_t)std::max<u32>(n_mid, 1) * sizeof(u32), st));
    return DNAGPU_OK;
}

static int sk_l1_speculative(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, SkL1 &l1, SkL1Route route, bool *moved)
{
    const bool sampled = route == SkL1Route::SpeculativeSampled;
    RC_TRY(sk_l1_spec_begin(ctx, ps, p, l1, route));
    prof_mark(ctx, "sk_scatter1");
    HIP_TRY(launch_sk_scatter1_spec(p.coarse, l1.lv.chunks, l1.lv.n_chunks, p.rec0, l1.rec1, l1.gcur, l1.sp, l1.kcount,
                                    l1.d_lens + l1.lv.n_next + 2, ctx->stream, sampled ? l1.rstart : nullptr,
                                    sampled ? l1.rcapv : nullptr));
    return sk_l1_spec_end(ctx, ps, p, l1, route, moved);
}

// The exact histogram: the mid buckets' nodes from its prefix, and their k-mer and record counts on the host before any
// record moves (the census decides on them).
static int sk_l1_histogram(dnagpu_ctx *ctx, const SkParts &p, SkL1 &l1)
{
    hipStream_t st = ctx->stream;
    const SkLevel &lv = l1.lv;
    prof_mark(ctx, "sk_hist1");
    HIP_TRY(launch_sk_hist1(p.coarse, lv.chunks, lv.n_chunks, p.rec0, lv.hist, l1.kcount, st));
    prof_mark(ctx, "sk_prefix1");
    HIP_TRY(launch_level_prefix(p.coarse, lv.chunks, lv.n_chunks, p.n_coarse, l1.chunk_recs, lv.hist, lv.tot, st, p.n_coarse));
    HIP_TRY(launch_level_children(p.coarse, p.n_coarse, lv.tot, lv.next, nullptr, nullptr, nullptr, 0, st));
    HIP_TRY(launch_sk_node_lens(lv.next, lv.n_next, l1.d_lens, st));
    return sk_l1_lens_to_host(ctx, l1, 0);
}

// The census of the mid buckets, on the host: p.n_kmers = the k-mers found (checked against p.n_expected where that is
// known), *heavy_idx = the heavy ones, p.heavy.total = their k-mers.
// Heavy: too many k-mers, or too many records for the one workgroup that regroups a mid bucket (its tiles are serial).
// DNAGPU_SK_SKEWED leaves levels 1-2 from here, in two cases only: with DNAGPU_DEBUG_HEAVY_EXPAND (the older path, kept
// for the tests: heavy mid buckets are expanded as a whole, and a set that is mostly heavy is cheaper through the tree from
// scratch -- count_core -- or as one key node per coarse bucket -- count_sk_received; rec0 is still what it was: level 1
// only reads it), or with more heavy mid buckets than the chunked split plans for (32768: not reachable with 2^32 rows, a
// guard).
static int sk_l1_census(unsigned debug_flags, const SkL1 &l1, SkParts &p, std::vector<u32> *heavy_idx)
{
    const std::vector<u32> &kc = l1.kc, &rcn = l1.rcn;
    const u32 n_mid = l1.lv.n_next;
    const u64 mid_limit = p.g.mid_limit;
    const bool forced = (debug_flags & DNAGPU_DEBUG_FORCE_SUPERKMER) != 0;
    auto is_heavy = [&](u32 i) { return kc[i] > mid_limit || (!forced && rcn[i] > SK_MID_RECORDS); };
    u64 run = 0;
    bool any_heavy = false;
    for (u32 i = 0; i < n_mid; i++) {
        run += kc[i];
        any_heavy = any_heavy || is_heavy(i);
    }
    if (p.n_expected != 0 && run != p.n_expected) {
        set_err("super-k-mer partition lost rows: %llu of %llu", (unsigned long long)run, (unsigned long long)p.n_expected);
        return DNAGPU_ERR_INTERNAL;
    }
    if (run > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    p.n_kmers = run;
    if (!any_heavy)
        return DNAGPU_OK;
    for (u32 i = 0; i < n_mid; i++)
        if (is_heavy(i)) {
            heavy_idx->push_back(i);
            p.heavy.total += kc[i];
        }
    if (((debug_flags & DNAGPU_DEBUG_HEAVY_EXPAND) && p.heavy.total * 2 > run) || heavy_idx->size() > 32768)
        return DNAGPU_SK_SKEWED;
    return DNAGPU_OK;
}

// The exact scatter (rec0 -> rec1), where the speculative sweep did not move the records.
static int sk_l1_scatter(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, SkL1 &l1)
{
    hipStream_t st = ctx->stream;
    const SkLevel &lv = l1.lv;
    if (!l1.rec1) {
        RC_TRY(pool_alloc(ctx, (size_t)std::max<u64>(p.n_recs, 1) * 16, &l1.rec1));
        ps.ptrs.push_back(l1.rec1);
    }
    prof_mark(ctx, "sk_scatter1");
    // the mid buckets' cursors start at their exact bases (the prefix of the histogram); tiles reserve their slots there
    HIP_TRY(hipMemcpyAsync(l1.gcur, lv.tot, (size_t)std::max<u32>(lv.n_chunks, 1) * ROW_STRIDE * sizeof(u32), hipMemcpyDeviceToDevice,
                           st));
    HIP_TRY(launch_sk_scatter1(p.coarse, lv.chunks, lv.n_chunks, p.rec0, l1.rec1, lv.hist, lv.tot, st, false, l1.gcur));
    return DNAGPU_OK;
}

struct SkSplit {                    // the heavy mid buckets split by d2: lv.next = their children, kcount = the children's k-mers
    SkLevel lv = {};
    u32 *kcount = nullptr;
};

// The heavy mid buckets leave the list of level 1 (empty nodes stay behind): one workgroup could not regroup them in
// time.  They are split by d2 with the CHUNKED level kernels instead (many workgroups per bucket: plan, histogram, prefix,
// children, scatter rec1 -> rec0 into the range the bucket would have been regrouped into); their sixteen children join
// the final buckets (*split), where sk_count_big takes the long ones slice by slice.
// DNAGPU_DEBUG_HEAVY_EXPAND (tests): they go to the tail's expansion as whole mid buckets instead (p.heavy; rec1 stays).
static int sk_heavy_take(dnagpu_ctx *ctx, PoolScope &ps, SkParts &p, SkL1 &l1, const std::vector<u32> &heavy_idx, SkSplit *split)
{
    hipStream_t st = ctx->stream;
    const u32 nh = (u32)heavy_idx.size();
    u32 *d_idx = nullptr;
    Node *hnodes = nullptr;
    RC_TRY(ps.alloc((size_t)nh, &d_idx));
    RC_TRY(ps.alloc((size_t)nh, &hnodes));
    HIP_TRY(hipMemcpyAsync(d_idx, heavy_idx.data(), (size_t)nh * sizeof(u32), hipMemcpyHostToDevice, st));
    HIP_TRY(launch_sk_take_heavy(l1.lv.next, d_idx, nh, l1.kcount, hnodes, st));
    HIP_TRY(hipStreamSynchronize(st));           // (heavy_idx is a host vector)
    if (ctx->debug_flags & DNAGPU_DEBUG_HEAVY_EXPAND) {
        p.heavy.nodes = hnodes;
        p.heavy.n = nh;
        p.heavy.recs = l1.rec1;
        l1.rec1_kept = true;
        return DNAGPU_OK;
    }
    u64 hrecs = 0;
    for (u32 i : heavy_idx)
        hrecs += l1.rcn[i];
    const u32 chunk_h = sk_chunk_len(hrecs);
    SkLevel &lh = split->lv;
    prof_mark(ctx, "sk_heavy_split");
    RC_TRY(sk_level_begin(ctx, ps, hnodes, nh, 4, chunk_h, &lh));
    RC_TRY(alloc1(ps, lh.n_next, &split->kcount));
    HIP_TRY(hipMemsetAsync(split->kcount, 0, (size_t)std::max<u32>(lh.n_next, 1) * sizeof(u32), st));
    HIP_TRY(launch_sk_hist1(hnodes, lh.chunks, lh.n_chunks, l1.rec1, lh.hist, split->kcount, st, true));
    HIP_TRY(launch_level_prefix(hnodes, lh.chunks, lh.n_chunks, nh, chunk_h, lh.hist, lh.tot, st, nh));
    HIP_TRY(launch_level_children(hnodes, nh, lh.tot, lh.next, nullptr, nullptr, nullptr, 0, st));
    HIP_TRY(launch_sk_scatter1(hnodes, lh.chunks, lh.n_chunks, l1.rec1, p.rec0, lh.hist, lh.tot, st, true));
    p.heavy.total = 0;                           // (nothing is left for the expansion of mid buckets)
    return DNAGPU_OK;
}

// Level 2: every mid bucket regrouped by d2 (rec1 -> rec0): 16 final buckets each, the children of the split heavy
// buckets behind them.  Fills p.recs / p.fin / p.n_fin; rec1 goes back to the pool unless p.heavy lives in it.
// The phase "sk_regroup" is marked once per regroup that did work: here, or where it was launched early.
static int sk_level2(dnagpu_ctx *ctx, PoolScope &ps, SkParts &p, SkL1 &l1, const SkSplit &split)
{
    hipStream_t st = ctx->stream;
    const u32 n_mid = l1.lv.n_next, n_split = split.lv.n_next;
    Node *fn = l1.fn_early;
    if (l1.early_open) {                         // (sk_l1_spec_end: the regroup ran behind its gate, and it was all of level 2)
        if (n_split) {
            set_err("super-k-mer level 2: heavy mid buckets behind an open gate");
            return DNAGPU_ERR_INTERNAL;
        }
    } else {
        RC_TRY(ps.alloc((size_t)n_mid * 16 + n_split, &fn));
        prof_mark(ctx, "sk_regroup");
        bool any_long = false;                   // (mid buckets of more than one regroup tile: repeats)
        for (u32 i = 0; i < n_mid && !any_long; i++)
            any_long = l1.rcn[i] > (u32)sk_regroup_tile();
        HIP_TRY(launch_sk_regroup(l1.lv.next, n_mid, l1.rec1, p.rec0, fn, any_long, st));
        if (n_split)
            HIP_TRY(launch_sk_heavy_finals(split.lv.next, n_split, split.kcount, fn + (size_t)n_mid * 16, st));
    }
    if (!l1.rec1_kept)
        ps.free_now(l1.rec1);
    p.recs = p.rec0;
    p.fin = fn;
    p.n_fin = n_mid * 16 + n_split;
    return DNAGPU_OK;
}

// Levels 1 and 2 over the coarse nodes of p (records of rec0, which this takes over).  On success the levels-1-2 part of
// p is filled: the final buckets, and the heavy mid buckets that were taken out of the record path as a whole (p.heavy:
// only with DNAGPU_DEBUG_HEAVY_EXPAND).  DNAGPU_SK_SKEWED (sk_l1_census): p.n_kmers is set, nothing has moved.
// sk_levels12_planned: the same with level 1 planned already (sk_l1_plan); sk_levels12_rest: what follows the speculative
// sweep (moved: it has left the records in l1.rec1).
static int sk_levels12_rest(dnagpu_ctx *ctx, PoolScope &ps, SkParts &p, SkL1 &l1, bool moved)
{
    if (!moved)
        RC_TRY(sk_l1_histogram(ctx, p, l1));
    std::vector<u32> heavy_idx;
    RC_TRY(sk_l1_census(ctx->debug_flags, l1, p, &heavy_idx));
    if (!moved)
        RC_TRY(sk_l1_scatter(ctx, ps, p, l1));
    SkSplit split;
    if (!heavy_idx.empty())
        RC_TRY(sk_heavy_take(ctx, ps, p, l1, heavy_idx, &split));
    return sk_level2(ctx, ps, p, l1, split);
}

static int sk_levels12_planned(dnagpu_ctx *ctx, PoolScope &ps, SkParts &p, SkL1 &l1)
{
    SkL1Route route;
    RC_TRY(sk_l1_route(ctx, ps, p, l1, &route));
    bool moved = false;
    if (route != SkL1Route::Exact)
        RC_TRY(sk_l1_speculative(ctx, ps, p, l1, route, &moved));
    return sk_levels12_rest(ctx, ps, p, l1, moved);
}

static int sk_levels12(dnagpu_ctx *ctx, PoolScope &ps, SkParts &p)
{
    SkL1 l1;
    RC_TRY(sk_l1_plan(ctx, ps, p, l1));
    return sk_levels12_planned(ctx, ps, p, l1);
}

// ---------------------------------------------------------------- levels 0 and 1 side by side

// Level 0 (slab sweep) and the plain speculative level 1, piece by piece: sk_scatter0 uses under a third of the memory
// bandwidth and sk_scatter1 little of the vector units, so piece i of level 1 runs on the side stream while piece i + 1
// of level 0 is cut on the main stream.  Level 1 is planned over the whole regions BEFORE the sweep (its regions, cursors
// and k-mer counts are those of the unpipelined level); piece i's launch gets nodes of its own -- node d = the slots
// that the chunks of level-0 piece i reserve in region d (see SK_L0_PIECES), with the planned node's split, child_base and
// chunk_base, i.e. the same regions, cursors and counters -- and chunks over them, built on the host WHILE the first
// piece of level 0 runs (the planned nodes come back on the side stream, the lists go up on it).  The main stream
// waits for the side stream behind the last piece; level 0's status comes back with level 1's lens (one wait).
// *slab_ok: the sweep is usable (else everything level 1 did here is dropped with it: sk_slab_give_up, and rec1 is free
// again); *moved: as sk_l1_speculative.
static int sk_l01_piped(dnagpu_ctx *ctx, PoolScope &ps, SkParts &p, const SkRows &rows, const SkSlab &sl, SkL1 &l1, bool *slab_ok,
                        bool *moved)
{
    hipStream_t st = ctx->stream;
    const u32 n_coarse = p.n_coarse, chunk_recs = l1.chunk_recs;
    RC_TRY(side_stream(ctx, SK_EVENTS));
    RC_TRY(sk_l1_spec_begin(ctx, ps, p, l1, SkL1Route::Speculative));
    std::vector<Node> planned(n_coarse), pn;
    std::vector<Chunk> pc;
    // The first piece of level 0 needs nothing of level 1's launch lists: it is cut while the planned nodes travel to the
    // host on the side stream, the host builds the lists, and they travel back there (the level-1 launches follow them
    // on that stream).
    const size_t planned_bytes = (size_t)n_coarse * sizeof(Node);
    if (planned_bytes > MAILBOX_BYTES - 8) {
        set_err("sk_l01_piped: %u coarse nodes do not fit the mailbox", n_coarse);
        return DNAGPU_ERR_INTERNAL;
    }
    // (their device copies are allocated before anything runs beside the main stream: what the pool does to a fresh block
    // under its debug flags is queued on the main stream.  The chunks: as if every node were split.)
    size_t pc_room = 0;
    for (u32 i = 0; i < SK_L0_PIECES; i++) {
        u32 a = 0, b = 0;
        sk_piece_range(sl.l0.n_chunks, i, &a, &b);
        for (u32 d = 0; d < n_coarse; d++)
            pc_room += ((size_t)sl.cap[d] * (b - a) + chunk_recs - 1) / chunk_recs;
    }
    Node *d_pn = nullptr;
    Chunk *d_pc = nullptr;
    RC_TRY(alloc1(ps, (size_t)SK_L0_PIECES * n_coarse, &d_pn));
    RC_TRY(alloc1(ps, pc_room, &d_pc));
    RC_TRY(side_behind_main(ctx));
    SideWork side(ctx->stream2, st);             // (pn / pc are host vectors: an early way out waits for their copies too)
    prof_mark(ctx, "sk_scatter0");
    {
        u32 a = 0, b = 0;
        sk_piece_range(sl.l0.n_chunks, 0, &a, &b);
        RC_TRY(sk_slab_piece(ctx, p, rows, sl, a, b));
        HIP_TRY(hipEventRecord(ctx->sync_ev[0], st));
    }
    HIP_TRY(hipMemcpyAsync(ctx->mailbox, p.coarse, planned_bytes, hipMemcpyDeviceToHost, side.s));
    HIP_TRY(hipStreamSynchronize(side.s));
    memcpy(planned.data(), ctx->mailbox, planned_bytes);
    u32 first_chunk[SK_L0_PIECES + 1];
    for (u32 i = 0; i < SK_L0_PIECES; i++) {
        u32 a = 0, b = 0;
        sk_piece_range(sl.l0.n_chunks, i, &a, &b);
        first_chunk[i] = (u32)pc.size();
        for (u32 d = 0; d < n_coarse; d++) {
            Node nd = planned[d];
            nd.start += sl.cap[d] * a;
            nd.len = sl.cap[d] * (b - a);
            pn.push_back(nd);
            for (u32 off = 0; nd.split && off < nd.len; off += chunk_recs) {
                Chunk c;
                c.node = d;
                c.off = off;
                c.len = std::min(chunk_recs, nd.len - off);
                c.pad = 0;
                pc.push_back(c);
            }
        }
    }
    first_chunk[SK_L0_PIECES] = (u32)pc.size();
    if (pc.size() > pc_room) {
        set_err("sk_l01_piped: %zu chunks planned, room for %zu", pc.size(), pc_room);
        return DNAGPU_ERR_INTERNAL;
    }
    HIP_TRY(hipMemcpyAsync(d_pn, pn.data(), pn.size() * sizeof(Node), hipMemcpyHostToDevice, side.s));
    if (!pc.empty())
        HIP_TRY(hipMemcpyAsync(d_pc, pc.data(), pc.size() * sizeof(Chunk), hipMemcpyHostToDevice, side.s));
    u32 *status1 = l1.d_lens + l1.lv.n_next;
    for (u32 i = 0; i < SK_L0_PIECES; i++) {
        if (i > 0) {                             // (piece 0 is on its way)
            u32 a = 0, b = 0;
            sk_piece_range(sl.l0.n_chunks, i, &a, &b);
            RC_TRY(sk_slab_piece(ctx, p, rows, sl, a, b));
            HIP_TRY(hipEventRecord(ctx->sync_ev[i], st));
        }
        HIP_TRY(hipStreamWaitEvent(side.s, ctx->sync_ev[i], 0));
        HIP_TRY(launch_sk_scatter1_spec(d_pn + (size_t)i * n_coarse, d_pc + first_chunk[i], first_chunk[i + 1] - first_chunk[i], p.rec0,
                                        l1.rec1, l1.gcur, l1.sp, l1.kcount, status1 + 2, side.s, nullptr, nullptr));
    }
    prof_mark(ctx, "sk_scatter1");                // (from here: what of level 1 the sweep did not hide)
    HIP_TRY(hipEventRecord(ctx->sync_ev[SK_EV_JOIN], side.s));
    HIP_TRY(hipStreamWaitEvent(st, ctx->sync_ev[SK_EV_JOIN], 0));
    side.joined = true;
    u32 status0[2] = {1, 0};
    RC_TRY(sk_l1_spec_end(ctx, ps, p, l1, SkL1Route::Speculative, moved, sl.slab + 18 * (size_t)sk_max_c0(), status0, (u32)sl.span));
    *slab_ok = sk_slab_ok(ctx, sl, status0);
    if (!*slab_ok) {
        ps.free_now(l1.rec1);
        l1.rec1 = nullptr;
        *moved = false;
    }
    return DNAGPU_OK;
}

// Level 0 as a slab sweep and levels 1-2 behind it.  *done = false: the slabs gave up (sk_slab_begin, or a chunk ran out of
// slots) and p is as it was -- the caller runs the exact pair and sk_levels12 over the whole sequence; nothing of what
// level 1 did here is kept.  Level 1 is planned before the sweep; where the sweep is long enough for it to pay (see
// SK_PIPE_MIN_ROWS) and level 1's route is the plain speculative one (even regions, no DNAGPU_DEBUG_NO_SPEC1 / _SAMPLE1),
// the two levels run side by side (sk_l01_piped), else one after the other.
static int sk_levels012_slab(dnagpu_ctx *ctx, PoolScope &ps, SkParts &p, const SkRows &rows, bool *done)
{
    *done = false;
    SkSlab sl;
    sl.pipe = (ctx->debug_flags & (DNAGPU_DEBUG_SLAB0 | DNAGPU_DEBUG_SLAB0_OVERFLOW)) || (!rows.marks && rows.n >= SK_PIPE_MIN_ROWS);
    bool ok = false;
    RC_TRY(sk_slab_begin(ctx, ps, p, rows, sl, &ok));
    if (!ok)
        return DNAGPU_OK;
    SkL1 l1;
    RC_TRY(sk_l1_plan(ctx, ps, p, l1));
    bool any_spec = false, plain = false, moved = false;
    sk_l1_route_plain(ctx, p, l1, &any_spec, &plain);
    const bool piped = sl.pipe && plain;
    if (piped) {
        RC_TRY(sk_l01_piped(ctx, ps, p, rows, sl, l1, &ok, &moved));
    } else {
        prof_mark(ctx, "sk_scatter0");
        RC_TRY(sk_slab_piece(ctx, p, rows, sl, 0, sl.l0.n_chunks));
        u32 status0[2] = {1, 0};
        RC_TRY(read_back(ctx, status0, sl.slab + 18 * (size_t)sk_max_c0(), sizeof status0));
        ok = sk_slab_ok(ctx, sl, status0);
    }
    if (!ok) {
        sk_slab_give_up(ps, p);
        return DNAGPU_OK;
    }
    *done = true;
    return piped ? sk_levels12_rest(ctx, ps, p, l1, moved) : sk_levels12_planned(ctx, ps, p, l1);
}

// ---------------------------------------------------------------- the tail: counting the final buckets

// What the stages of count_sk_tail share, in the order in which they fill it.
struct SkTail {
    // ---- sk_tail_select: flags (then their scans) per final bucket, and the lists of the small buckets (at most
    // sk_count_cap() k-mers: sk_count's) and the big ones
    u32 *f_small = nullptr, *f_big = nullptr, *k_range = nullptr, *f_over = nullptr;
    u32 *f_over3 = nullptr, *p_over3 = nullptr, *k_over3 = nullptr;   // the buckets of class "over": flags, their scan, their k-mers (scanned)
    u32 n_over3 = 0, over_keys3 = 0;              // (with no big bucket they are the over buckets: sk_tail_select_over)
    u32 *scan_tmp = nullptr, *totals = nullptr;   // (six scans at a time; eight totals)
    u32 *list_small = nullptr, *off_small = nullptr, *list_big = nullptr, *off_big = nullptr;
    u32 n_small = 0, n_big = 0, big_kmers = 0;
    u64 small_keys = 0;         // the output slots of the small and big buckets: one per k-mer, in bucket order
    u64 out_cap = 0;
    // ---- sk_tail_outputs
    u64 *cursor = nullptr;      // [0] next free output slot of the leaves behind the buckets' ranges; [1] buckets whose
                                // expansion disagrees with the partition's count; [2] groups sk_count and sk_count_big wrote
    u64 *ok = nullptr;          // the groups' keys
    u32 *oc = nullptr;          // and counts
    u64 *seg_off_fin = nullptr; // the directory of the final buckets (the tree's nodes get theirs in sk_tail_leaves)
    u32 *seg_cnt_fin = nullptr;
    u32 *big_status = nullptr;
    // ---- sk_tail_select_over: the oversize final buckets
    Node *over_nodes = nullptr;
    u32 n_over = 0;
    u64 over_keys = 0;
    // ---- sk_tail_tree
    TreeResult tr = {};
    // ---- sk_tail_leaves: the directory of everything
    u64 *seg_off = nullptr;
    u32 *seg_cnt = nullptr;
    u32 n_segs = 0;
};

// Selection of the small buckets (sk_count) and the big ones (sk_count_big).  n = the k-mers of all.
static int sk_tail_select(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, u64 n, SkTail &t)
{
    hipStream_t st = ctx->stream;
    const u32 n_fin = p.n_fin;
    prof_mark(ctx, "sk_select");
    RC_TRY(ps.alloc((size_t)n_fin, &t.f_small));
    RC_TRY(ps.alloc((size_t)n_fin, &t.f_big));
    RC_TRY(ps.alloc((size_t)n_fin, &t.k_range));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n_fin) * SCAN_SET_MAX, &t.scan_tmp));     // (six scans at a time: launch_scan_u32_multi)
    RC_TRY(ps.alloc(8, &t.totals));
    RC_TRY(ps.alloc((size_t)n_fin, &t.list_small));
    RC_TRY(ps.alloc((size_t)n_fin, &t.off_small));
    RC_TRY(ps.alloc((size_t)n_fin, &t.f_over));     // (first: the k-mers of the big buckets, summed)
    RC_TRY(ps.alloc((size_t)n_fin, &t.f_over3));
    RC_TRY(ps.alloc((size_t)n_fin, &t.p_over3));
    RC_TRY(ps.alloc((size_t)n_fin, &t.k_over3));
    HIP_TRY(launch_sk_select_flags(p.fin, n_fin, (u32)sk_count_cap(), (u32)SK_BIG_LIMIT, t.f_small, t.f_big, t.k_range, t.f_over,
                                   t.f_over3, t.k_over3, st));
    // the over buckets of class 3 in the same sweep and the same wait: with no big bucket (uniform sequence, most inputs)
    // that is the whole second selection.  (Their flags stay as they are, the scan goes to p_over3: sk_over_list reads both.)
    HIP_TRY(launch_scan_u32_multi(scan_set({t.f_small, t.f_big, t.k_range, t.f_over, t.f_over3, t.k_over3},
                                           {t.f_small, t.f_big, t.k_range, t.f_over, t.p_over3, t.k_over3}, t.totals, t.scan_tmp),
                                  6, n_fin, st));
    u32 ht[6] = {0, 0, 0, 0, 0, 0};
    RC_TRY(read_back(ctx, ht, t.totals, sizeof ht));
    t.n_small = ht[0];
    t.n_big = ht[1];
    t.small_keys = ht[2];
    t.big_kmers = ht[3];
    t.n_over3 = ht[4];
    t.over_keys3 = ht[5];
    // a big bucket that sk_count_big gives up on is counted again through the expansion: its groups land behind the
    // ranges while its own range stays padding, so the arrays hold up to n + the big buckets' k-mers
    t.out_cap = n + t.big_kmers;
    RC_TRY(alloc1(ps, t.n_big, &t.list_big));
    RC_TRY(alloc1(ps, t.n_big, &t.off_big));
    HIP_TRY(launch_sk_select_lists(p.fin, n_fin, (u32)sk_count_cap(), (u32)SK_BIG_LIMIT, t.f_small, t.f_big, t.k_range, t.list_small,
                                   t.off_small, t.list_big, t.off_big, st));
    return DNAGPU_OK;
}

// Output arrays and the segment directory of the final buckets (the nodes of the oversize buckets' tree come behind them)
static int sk_tail_outputs(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, SkTail &t)
{
    hipStream_t st = ctx->stream;
    const u32 n_fin = p.n_fin;
    RC_TRY(ps.alloc(3, &t.cursor));
    RC_TRY(ps.alloc((size_t)t.out_cap, &t.ok));
    RC_TRY(ps.alloc((size_t)t.out_cap, &t.oc));
    const u64 init[3] = {t.small_keys, 0, 0};
    HIP_TRY(poke(t.cursor, init, sizeof init, st));
    RC_TRY(alloc1(ps, n_fin, &t.seg_off_fin));
    RC_TRY(alloc1(ps, n_fin, &t.seg_cnt_fin));
    HIP_TRY(hipMemsetAsync(t.seg_cnt_fin, 0, (size_t)n_fin * sizeof(u32), st));     // empty and expanded buckets: no groups of their own
    HIP_TRY(hipMemsetAsync(t.seg_off_fin, 0, (size_t)n_fin * sizeof(u64), st));
    RC_TRY(alloc1(ps, t.n_big, &t.big_status));
    return DNAGPU_OK;
}

// Long buckets of few distinct keys (repeats): one table per bucket; what outgrows it joins the expansion (big_status).
// Work items: slices of the buckets' records; a bucket of several slices gets a partial area per slice.
static int sk_tail_count_big(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, SkTail &t)
{
    hipStream_t st = ctx->stream;
    const u32 n_big = t.n_big;
    prof_mark(ctx, "sk_count_big");
    u32 *nsl = nullptr, *sfirst = nullptr, *mfirst = nullptr, *sl_bucket = nullptr, *sl_idx = nullptr, *part_n = nullptr, *part_cnts = nullptr;
    u64 *part_keys = nullptr;
    RC_TRY(ps.alloc((size_t)n_big, &nsl));
    RC_TRY(ps.alloc((size_t)n_big, &sfirst));
    RC_TRY(ps.alloc((size_t)n_big, &mfirst));
    HIP_TRY(launch_sk_big_slices(p.fin, t.list_big, n_big, nsl, mfirst, st));
    HIP_TRY(launch_scan_u32(nsl, sfirst, n_big, t.scan_tmp, t.totals + 6, st));
    HIP_TRY(launch_scan_u32(mfirst, mfirst, n_big, t.scan_tmp, t.totals + 7, st));
    u32 hs[2] = {0, 0};
    RC_TRY(read_back(ctx, hs, t.totals + 6, sizeof hs));
    const u32 n_slices = hs[0], n_part = hs[1];
    RC_TRY(alloc1(ps, n_slices, &sl_bucket));
    RC_TRY(alloc1(ps, n_slices, &sl_idx));
    RC_TRY(alloc1(ps, n_part, &part_n));
    RC_TRY(alloc1(ps, n_part, &part_keys, sk_big_partial_slots()));
    RC_TRY(alloc1(ps, n_part, &part_cnts, sk_big_partial_slots()));
    HIP_TRY(launch_sk_big_slice_fill(nsl, sfirst, n_big, sl_bucket, sl_idx, st));
    HIP_TRY(launch_sk_count_big(p.fin, t.list_big, t.off_big, nsl, mfirst, sl_bucket, sl_idx, n_slices, n_big, p.recs, p.k, t.cursor + 2,
                                t.seg_off_fin, t.seg_cnt_fin, t.ok, t.oc, t.big_status, part_keys, part_cnts, part_n, n_part > 0, st));
    return DNAGPU_OK;
}

// Selection of the buckets left over: too many k-mers for sk_count, and not (or not successfully) sk_count_big's
static int sk_tail_select_over(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, SkTail &t)
{
    hipStream_t st = ctx->stream;
    const u32 n_fin = p.n_fin;
    u32 *f_over_raw = nullptr, *k_over = nullptr, *over_kbase = nullptr;
    prof_mark(ctx, "sk_select_over");
    if (t.n_big == 0) {                          // no big bucket: class 3 is all of it, and sk_tail_select has scanned it
        t.n_over = t.n_over3;
        t.over_keys = t.over_keys3;
        RC_TRY(alloc1(ps, t.n_over, &t.over_nodes));
        RC_TRY(alloc1(ps, t.n_over, &over_kbase));
        HIP_TRY(launch_sk_over_list(p.fin, n_fin, t.f_over3, t.p_over3, t.k_over3, t.over_nodes, over_kbase, st));
        return DNAGPU_OK;
    }
    RC_TRY(ps.alloc((size_t)n_fin, &f_over_raw));
    RC_TRY(ps.alloc((size_t)n_fin, &k_over));
    HIP_TRY(launch_sk_over_flags(p.fin, n_fin, (u32)sk_count_cap(), (u32)SK_BIG_LIMIT, t.f_big, t.big_status, f_over_raw, k_over, st));
    // (the flags stay as they are, their scan goes to f_over: sk_over_list reads both)
    HIP_TRY(launch_scan_u32_multi(scan_set({f_over_raw, k_over}, {t.f_over, k_over}, t.totals + 4, t.scan_tmp), 2, n_fin, st));
    u32 ho[2] = {0, 0};
    RC_TRY(read_back(ctx, ho, t.totals + 4, sizeof ho));
    t.n_over = ho[0];
    t.over_keys = ho[1];
    RC_TRY(alloc1(ps, t.n_over, &t.over_nodes));
    RC_TRY(alloc1(ps, t.n_over, &over_kbase));
    HIP_TRY(launch_sk_over_list(p.fin, n_fin, f_over_raw, t.f_over, k_over, t.over_nodes, over_kbase, st));
    return DNAGPU_OK;
}

// The expansion of n buckets (start / len in records of `recs`, child_base = k-mers) to keys: their records are
// expanded in slices by many waves at once, into kbuf from key_base on, in list order; every bucket becomes one key node
// (knodes[0 .. n)).  check_kmers: a bucket whose keys are not child_base many is counted in t.cursor[1].
static int sk_tail_expand(dnagpu_ctx *ctx, PoolScope &ps, const SkTail &t, int k, const Node *buckets, u32 n, const void *recs,
                          u32 key_base, bool check_kmers, u64 *kbuf, Node *knodes)
{
    hipStream_t st = ctx->stream;
    u32 *sfirst = nullptr, *stmp = nullptr, *stot = nullptr;
    RC_TRY(ps.alloc((size_t)n, &sfirst));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n), &stmp));
    RC_TRY(ps.alloc(2, &stot));
    HIP_TRY(launch_sk_slice_count(buckets, n, sfirst, st));
    HIP_TRY(launch_scan_u32(sfirst, sfirst, n, stmp, stot, st));
    u32 n_slices = 0;
    RC_TRY(read_back(ctx, &n_slices, stot, 4));
    u32 *d_r0 = nullptr, *d_nr = nullptr, *d_ko = nullptr, *ktmp = nullptr;
    RC_TRY(alloc1(ps, n_slices, &d_r0));
    RC_TRY(alloc1(ps, n_slices, &d_nr));
    RC_TRY(alloc1(ps, n_slices, &d_ko));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(std::max<u32>(n_slices, 1)), &ktmp));
    HIP_TRY(launch_sk_slice_fill(buckets, n, sfirst, d_r0, d_nr, st));
    HIP_TRY(launch_sk_slice_kmers(recs, d_r0, d_nr, n_slices, d_ko, st));
    HIP_TRY(launch_scan_u32(d_ko, d_ko, n_slices, ktmp, stot + 1, st));
    HIP_TRY(launch_sk_slice_nodes(buckets, n, sfirst, d_ko, n_slices, stot + 1, key_base, k, check_kmers, knodes, t.cursor + 1, st));
    HIP_TRY(launch_sk_expand_flat(recs, d_r0, d_nr, d_ko, key_base, n_slices, k, kbuf, st));
    return DNAGPU_OK;
}

// Oversize final buckets (the tail of the size distribution, moderate repeats) and heavy mid buckets (the minimizers of
// long repeats): keys, then the ordinary levels with their skew paths (t.tr).  The key ranges and key nodes: the oversize
// final buckets in list order, the heavy buckets behind them.
static int sk_tail_tree(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, SkTail &t)
{
    const SkHeavy &heavy = p.heavy;
    if (t.n_over + heavy.n > 0) {
        const u64 tree_keys = t.over_keys + heavy.total;
        if (tree_keys > 0xFFFFFFFFull)
            return DNAGPU_ERR_TOO_LARGE;
        const u32 n_tree = t.n_over + heavy.n;
        u64 *kbuf = nullptr;
        Node *knodes = nullptr;
        RC_TRY(ps.alloc((size_t)tree_keys, &kbuf));
        RC_TRY(ps.alloc((size_t)n_tree, &knodes));
        prof_mark(ctx, "sk_expand_flat");
        if (t.n_over)
            RC_TRY(sk_tail_expand(ctx, ps, t, p.k, t.over_nodes, t.n_over, p.recs, 0, true, kbuf, knodes));
        if (heavy.n)
            RC_TRY(sk_tail_expand(ctx, ps, t, p.k, heavy.nodes, heavy.n, heavy.recs, (u32)t.over_keys, heavy.counted, kbuf,
                                  knodes + t.n_over));
        RC_TRY(run_tree(ctx, ps, nullptr, 0, tree_keys, p.k, kbuf, 0, &t.tr, 0, 0, true, 0, ~0u, 0, knodes, n_tree, 2));
    }
#ifdef DNAGPU_STAMPS
    fprintf(stderr, "[sk select] n_fin %u small %u big %u (k-mers of big %u) over %u (keys %llu) heavy %u (keys %llu) tree nodes %u tiny %u small %u big %u\n",
            p.n_fin, t.n_small, t.n_big, t.big_kmers, t.n_over, (unsigned long long)t.over_keys, heavy.n,
            (unsigned long long)heavy.total, t.tr.n_nodes, t.tr.n_tiny, t.tr.n_small, t.tr.n_big);
#endif
    return DNAGPU_OK;
}

// The directory of everything (final buckets, then the tree's nodes) and the tree's leaves, counted behind the buckets' ranges
static int sk_tail_leaves(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, SkTail &t)
{
    hipStream_t st = ctx->stream;
    const u32 n_fin = p.n_fin;
    const TreeResult &tr = t.tr;
    t.n_segs = n_fin + tr.n_nodes;
    RC_TRY(ps.alloc((size_t)t.n_segs, &t.seg_off));
    RC_TRY(ps.alloc((size_t)t.n_segs, &t.seg_cnt));
    HIP_TRY(hipMemcpyAsync(t.seg_cnt, t.seg_cnt_fin, (size_t)n_fin * sizeof(u32), hipMemcpyDeviceToDevice, st));   // (sk_count_big's entries)
    HIP_TRY(hipMemcpyAsync(t.seg_off, t.seg_off_fin, (size_t)n_fin * sizeof(u64), hipMemcpyDeviceToDevice, st));
    if (tr.n_nodes > 0) {
        u32 *flags = nullptr, *ltmp = nullptr, *cls_list = nullptr;
        RC_TRY(ps.alloc((size_t)tr.n_nodes + 1, &flags));
        RC_TRY(ps.alloc((size_t)scan_tmp_words(tr.n_nodes), &ltmp));
        RC_TRY(ps.alloc((size_t)tr.n_nodes, &cls_list));
        prof_mark(ctx, "leaves");
        HIP_TRY(launch_leaves(tr.nodes, tr.n_nodes, tr.n_tiny, tr.n_small, tr.n_big, tr.buf0, tr.buf1, t.cursor, t.seg_off + n_fin,
                              t.seg_cnt + n_fin, t.ok, t.oc, flags, ltmp, cls_list, st, true, t.small_keys));
        HIP_TRY(launch_sk_unmix(t.ok, t.small_keys, t.cursor, tr.n_keys, p.k, st));      // (sk_expand_flat wrote key_mix(key))
    }
    return DNAGPU_OK;
}

// The small buckets, counted from their records
static int sk_tail_count(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, SkTail &t)
{
    hipStream_t st = ctx->stream;
    prof_mark(ctx, "sk_count");
    u32 *left = nullptr;
    RC_TRY(ps.alloc((size_t)2 * t.n_small + 1, &left));
    HIP_TRY(launch_sk_count(p.fin, t.list_small, t.off_small, t.n_small, p.recs, p.k, t.cursor + 2, t.seg_off, t.seg_cnt, t.ok, t.oc, left,
                            st));
#ifdef DNAGPU_STAMPS
    {
        u32 nl = 0;
        RC_TRY(read_back(ctx, &nl, left + 2 * (size_t)t.n_small, 4));
        fprintf(stderr, "[sk count] %u small buckets, %u left to sk_count by sk_count_clean\n", t.n_small, nl);
    }
#endif
    return DNAGPU_OK;
}

// The final read-back: the counters are checked against each other and h takes the groups over
static int sk_tail_finish(dnagpu_ctx *ctx, PoolScope &ps, const SkTail &t, u64 n, dnagpu_hist *h)
{
    prof_mark(ctx, "end");
    u64 fin_ctr[3] = {0, 0, 0};
    RC_TRY(read_back(ctx, fin_ctr, t.cursor, 24));
    const u64 extent = fin_ctr[0];
    const u64 total_groups = fin_ctr[2] + (extent - t.small_keys);
    if (fin_ctr[1] != 0) {
        set_err("super-k-mer count: %llu buckets whose records expand to a different number of k-mers than the partition counted",
                (unsigned long long)fin_ctr[1]);
        return DNAGPU_ERR_INTERNAL;
    }
    if (extent > t.out_cap) {
        set_err("super-k-mer count: %llu output slots used, %llu allocated", (unsigned long long)extent, (unsigned long long)t.out_cap);
        return DNAGPU_ERR_INTERNAL;
    }
    if (total_groups > n) {
        set_err("super-k-mer count: %llu groups for %llu rows", (unsigned long long)total_groups, (unsigned long long)n);
        return DNAGPU_ERR_INTERNAL;
    }
    h->total = n;
    hist_adopt(ps, h, t.ok, t.oc, t.seg_off, t.seg_cnt, t.n_segs, total_groups, false, extent);
    return DNAGPU_OK;
}

// The tail of the count over the partition of p: final buckets of at most sk_count_cap() k-mers are counted from their
// records (sk_count), long ones of few distinct keys by sk_count_big, the others and p.heavy expanded to keys and counted
// by the ordinary levels.  n = the k-mers of all.  Fills h on success.
static int count_sk_tail(dnagpu_ctx *ctx, PoolScope &ps, const SkParts &p, u64 n, dnagpu_hist *h)
{
    SkTail t;
    RC_TRY(sk_tail_select(ctx, ps, p, n, t));
    RC_TRY(sk_tail_outputs(ctx, ps, p, t));
    if (t.n_big)
        RC_TRY(sk_tail_count_big(ctx, ps, p, t));
    RC_TRY(sk_tail_select_over(ctx, ps, p, t));
    RC_TRY(sk_tail_tree(ctx, ps, p, t));
    RC_TRY(sk_tail_leaves(ctx, ps, p, t));
    RC_TRY(sk_tail_count(ctx, ps, p, t));
    return sk_tail_finish(ctx, ps, t, n, h);
}

// The whole count of rows of a sequence: level 0 (the slab sweep from SK_SLAB_MIN_ROWS rows, with levels 1-2 behind or
// beside it: sk_levels012_slab; else -- or where the slabs give up -- the exact pair and sk_levels12), the tail.
int dnagpu::count_sk(dnagpu_ctx *ctx, const SkRows &rows, int k, dnagpu_hist *h, u64 n_kmers_expected)
{
    PoolScope ps(ctx);
    SkParts p;
    p.g = sk_geometry(ctx, std::max<u64>(n_kmers_expected, 1), k);
    p.k = k;
    p.n_expected = n_kmers_expected;
    bool done = false;
    const unsigned dbg = ctx->debug_flags;
    if (!(dbg & DNAGPU_DEBUG_NO_SLAB0) && (rows.n >= SK_SLAB_MIN_ROWS || (dbg & (DNAGPU_DEBUG_SLAB0 | DNAGPU_DEBUG_SLAB0_OVERFLOW))))
        RC_TRY(sk_levels012_slab(ctx, ps, p, rows, &done));
    if (!done) {
        RC_TRY(sk_level0(ctx, ps, p, rows, true));
        RC_TRY(sk_levels12(ctx, ps, p));
    }
    return count_sk_tail(ctx, ps, p, n_kmers_expected, h);
}

u64 dnagpu::sk_received_cap(const std::vector<u64> &blen, u32 n_coarse, const SkGeom &g)
{
    u64 n_recs = 0, span = 0;
    for (u32 d = 0; d < n_coarse; d++) {
        n_recs += blen[d];
        span += sk_spec_span((u32)std::min<u64>(blen[d], 0xFFFFFFFFull), g.b1);
    }
    return span <= 0xFFFFFFFFull ? std::max(n_recs, span) : n_recs;
}

int dnagpu::count_sk_received(dnagpu_ctx *ctx, void *rec0, const std::vector<u64> &boff, const std::vector<u64> &blen, const SkGeom &g,
                              int k, dnagpu_hist *h, u64 rec0_cap)
{
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    ps.ptrs.push_back(rec0);
    SkParts p;
    p.g = g;
    p.k = k;
    p.rec0 = rec0;
    p.rec0_cap = rec0_cap;
    p.n_coarse = 1u << g.r0bits;
    p.n_recs = boff[p.n_coarse];
    p.lens.resize(p.n_coarse);
    std::vector<Node> hn(p.n_coarse);
    for (u32 d = 0; d < p.n_coarse; d++) {
        memset(&hn[d], 0, sizeof(Node));
        hn[d].start = (u32)boff[d];
        hn[d].len = p.lens[d] = (u32)blen[d];
        hn[d].meta = (u32)(32 - g.r0bits);       // (what level_children leaves a child of the 32-"bit" root)
    }
    RC_TRY(ps.alloc((size_t)p.n_coarse, &p.coarse));
    HIP_TRY(hipMemcpyAsync(p.coarse, hn.data(), (size_t)p.n_coarse * sizeof(Node), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));           // (hn, and the caller's pieces, are free again)
    int rc = sk_levels12(ctx, ps, p);
    if (rc == DNAGPU_SK_SKEWED) {
        // every coarse bucket as one "heavy" bucket: keys, then the ordinary levels (sk_levels12 has not moved anything yet)
        p.heavy = SkHeavy();
        p.heavy.nodes = p.coarse;
        p.heavy.n = p.n_coarse;
        p.heavy.recs = rec0;
        p.heavy.total = p.n_kmers;
        p.heavy.counted = false;
        p.n_fin = 0;
        rc = DNAGPU_OK;
    }
    RC_TRY(rc);
    return count_sk_tail(ctx, ps, p, p.n_kmers, h);
}

// Records that arrive from elsewhere (the multi-GPU exchange: every rank cuts the records of its own chunk and ships each
// coarse bucket to its owner): pieces[i] = piece_len[i] records of coarse bucket piece_bucket[i], device memory.  The
// pieces are copied bucket by bucket into one buffer (equal k-mers share the bucket, so its pieces must form ONE node),
// then levels 1-2 and the counting as in count_sk.  A skewed set (more than half the k-mers in heavy mid buckets)
// cannot fall back to the sequence here: all of it is expanded to keys for the ordinary levels instead.
static int count_sk_records(dnagpu_ctx *ctx, const void *const *pieces, const u64 *piece_len, const u32 *piece_bucket, u32 n_pieces,
                            int k, u64 global_rows, dnagpu_hist *h)
{
    hipStream_t st = ctx->stream;
    const SkGeom g = sk_geometry(ctx, global_rows, k);
    const u32 n_coarse = 1u << g.r0bits;
    std::vector<u64> blen(n_coarse, 0), boff(n_coarse + 1, 0);
    for (u32 i = 0; i < n_pieces; i++) {
        if (piece_bucket[i] >= g.c0n || (piece_len[i] && !pieces[i]))
            return DNAGPU_ERR_BAD_ARG;
        blen[piece_bucket[i]] += piece_len[i];
    }
    for (u32 d = 0; d < n_coarse; d++)
        boff[d + 1] = boff[d] + blen[d];
    const u64 n_recs = boff[n_coarse];
    if (n_recs > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    if (n_recs == 0) {
        h->total = 0;
        return DNAGPU_OK;
    }
    void *rec0 = nullptr;
    const u64 cap0 = sk_received_cap(blen, n_coarse, g);    // (room for the regions of a level 1 without its histogram)
    RC_TRY(pool_alloc(ctx, (size_t)cap0 * 16, &rec0));
    std::vector<u64> fill(boff.begin(), boff.end() - 1);
    for (u32 i = 0; i < n_pieces; i++)
        if (piece_len[i]) {
            const hipError_t e = hipMemcpyAsync(static_cast<char *>(rec0) + fill[piece_bucket[i]] * 16, pieces[i], (size_t)piece_len[i] * 16,
                                                hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) {
                pool_free(ctx, rec0);
                set_err("record pieces: %s", hipGetErrorString(e));
                return DNAGPU_ERR_HIP;
            }
            fill[piece_bucket[i]] += piece_len[i];
        }
    return count_sk_received(ctx, rec0, boff, blen, g, k, h, cap0);
}

// ---- the two halves of the unordered count, for a count whose rows live on several GPUs: records of a rank's own rows,
// grouped by coarse bucket (to be shipped to the buckets' owners), and the count of the records a rank has received
extern "C" int dnagpu_sk_buckets(const dnagpu_ctx *ctx, uint64_t global_rows, int k)
{
    if (!ctx || k < sk_min_k() || k > 32 || global_rows == 0 || global_rows > 0xFFFFFFFFull)
        return 0;
    return (int)sk_geometry(ctx, global_rows, k).c0n;
}

extern "C" int dnagpu_sk_records(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, uint64_t first, uint64_t count,
                                 uint64_t global_rows, dnagpu_records **out)
{
    return guarded([&]() -> int {
    if (!ctx || !dna || !out || k < sk_min_k() || k > 32 || global_rows < count || global_rows == 0 || global_rows > 0xFFFFFFFFull)
        return DNAGPU_ERR_BAD_ARG;
    RC_TRY(check_range(dna, k, first, count));
    HIP_TRY(hipSetDevice(ctx->device));
    const SkGeom g = sk_geometry(ctx, global_rows, k);
    std::unique_ptr<dnagpu_records> r(new (std::nothrow) dnagpu_records());
    if (!r)
        return DNAGPU_ERR_OOM;
    r->off.assign((size_t)g.c0n + 1, 0);
    if (count > 0) {
        PoolScope ps(ctx);
        SkParts p;
        p.g = g;
        p.k = k;
        prof_begin(ctx);
        const int rc = sk_level0(ctx, ps, p, SkRows{dna, first, count, nullptr, 0}, false);
        prof_mark(ctx, "end");
        prof_end(ctx);
        RC_TRY(rc);
        for (u32 d = 0; d < g.c0n; d++)
            r->off[d + 1] = r->off[d] + (d < p.lens.size() ? p.lens[d] : 0);
        const hipError_t se = hipStreamSynchronize(ctx->stream);
        if (r->off[g.c0n] != p.n_recs || se != hipSuccess) {
            set_err("super-k-mer level 0: %llu records in the buckets, %llu counted (%s)", (unsigned long long)r->off[g.c0n],
                    (unsigned long long)p.n_recs, hipGetErrorString(se));
            return se != hipSuccess ? DNAGPU_ERR_HIP : DNAGPU_ERR_INTERNAL;
        }
        ps.release(p.rec0);
        r->recs = p.rec0;
    }
    *out = r.release();
    return DNAGPU_OK;
    });
}

extern "C" uint32_t dnagpu_records_buckets(const dnagpu_records *r) { return r ? (uint32_t)(r->off.size() - 1) : 0; }
extern "C" int dnagpu_records_offsets(const dnagpu_records *r, uint64_t *offsets)
{
    if (!r || !offsets)
        return DNAGPU_ERR_BAD_ARG;
    for (size_t i = 0; i < r->off.size(); i++)
        offsets[i] = r->off[i];
    return DNAGPU_OK;
}
extern "C" void *dnagpu_records_device(const dnagpu_records *r) { return r ? r->recs : nullptr; }
extern "C" void dnagpu_records_free(dnagpu_ctx *ctx, dnagpu_records *r)
{
    if (!r)
        return;
    if (ctx)
        pool_free(ctx, r->recs);
    delete r;
}

extern "C" int dnagpu_count_records(dnagpu_ctx *ctx, const void *const *pieces, const uint64_t *piece_len,
                                    const uint32_t *piece_bucket, uint32_t n_pieces, int k, uint64_t global_rows, dnagpu_hist **out)
{
    return guarded([&]() -> int {
    if (!ctx || !out || (n_pieces && (!pieces || !piece_len || !piece_bucket)) || k < sk_min_k() || k > 32 || global_rows == 0 ||
        global_rows > 0xFFFFFFFFull)
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    HistPtr h = hist_new(0, false);
    if (!h)
        return DNAGPU_ERR_OOM;
    prof_begin(ctx);
    const int rc = count_sk_records(ctx, pieces, piece_len, piece_bucket, n_pieces, k, global_rows, h.get());
    prof_end(ctx);
    RC_TRY(rc);
    *out = h.release();
    return DNAGPU_OK;
    });
}
