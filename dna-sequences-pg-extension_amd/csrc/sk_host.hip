// sk_host.hip -- the host driver of the super-k-mer ("record") engine: geometry, level 0, levels 1-2, the tail that
// counts the final buckets, and the entry points of the record exchange.  Host side only.
#include "host_common.hpp"

using namespace dnagpu;

// ---- super-k-mer engine (superkmer_kernels.hip): the partition passes move 16-byte records of ~9 k-mers
// instead of 8-byte keys, and a final bucket is counted from its records in an LDS hash table: no key of it is
// ever written to HBM.
constexpr u64 SK_LEAF_MEAN = 2500;               // planned k-mers per final bucket: ~770 quads of four k-mers -- 1024 (sk_count's threads: the buckets with copies) is 4 sigma above, so next to no bucket takes the expansion path (A/B on one box, 3 Gbase: 2700 18.7 - 18.8 ms, 2500 18.2, 2300 18.1 - 18.4)
// A mid bucket of more than SK_MID_LIMIT k-mers (planned: 16 x SK_LEAF_MEAN) is "heavy" and leaves the record path for the
// expansion; below that it is regrouped like the others, and its long final buckets (thousands to millions of copies of a
// few k-mers) are what sk_count_big is for.  Final buckets beyond SK_BIG_LIMIT k-mers are expanded without trying.
constexpr u64 SK_MID_LIMIT = (u64)1 << 27;
// (a mid bucket is regrouped by ONE workgroup, tile after tile, twice: beyond eight tiles the chunked split below, many
// workgroups per bucket, is faster -- 249 Mbase of a tiled 1000-base motif: sk_regroup 0.64 ms at 2^19, sk_heavy_split 0.31 at 2^16)
#ifndef SK_MID_RECORDS_LOG2
#define SK_MID_RECORDS_LOG2 16
#endif
constexpr u32 SK_MID_RECORDS = 1u << SK_MID_RECORDS_LOG2;
constexpr u64 SK_BIG_LIMIT = 0xFFFFFFFFull;
// Level 1 splits a coarse bucket 512 ways, not 1024: a tile of 8192 records then leaves in runs of 16 records (256
// bytes) instead of 8 -- sk_scatter1 3.6 - 3.9 instead of 4.9 - 5.2 ms at 3 Gbase (A/B on one box) -- and level 0 takes
// the bit over (136 coarse buckets at 3 Gbase: its 16-byte stores still combine in L2, 2.2 MB of open lines per XCD).
constexpr int SK_B1_MAX = 9;

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
    RC_TRY(ps.alloc(std::max<u32>(hc.n_chunks, 1), &lv->chunks));
    RC_TRY(ps.alloc((size_t)std::max<u32>(hc.n_chunks, 1) * ROW_STRIDE, &lv->hist));
    RC_TRY(ps.alloc((size_t)std::max<u32>(hc.n_chunks, 1) * ROW_STRIDE, &lv->tot));
    RC_TRY(ps.alloc(std::max<u32>(hc.n_next, 1), &lv->next));
    HIP_TRY(launch_fill_chunks(cur, n_nodes, chunk_len, outc, nch, cur, lv->chunks, st));
    // (outc / nch / scan_tmp / ctr go back to the pool when the scope ends: later users queue behind this stream)
    return DNAGPU_OK;
}

// The three partition levels.  On success: *recs = the record buffer holding the final buckets, *fin / *n_fin =
// their nodes (start / len in records, child_base = k-mers), all pool memory of `ps`.
// Heavy mid buckets (more than SK_MID_LIMIT k-mers: the minimizers of repeats) are taken out of the record path: their
// nodes come back in *heavy (device copies, start / len in records of *heavy_recs), their k-mer counts in heavy_kc.
struct SkHeavy {
    Node *nodes = nullptr;      // device, n entries: start / len in records, child_base = k-mers (if counted)
    u32 n = 0;
    bool counted = true;        // child_base holds the bucket's k-mers (checked against its expansion)
    void *recs = nullptr;       // the record buffer they live in
    u64 total = 0;              // k-mers of all
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

// What both front ends of level 0 start with: the root node over n rows (*cur, device), chunks of whole tiles so that
// the rows make ~chunk_target of them (*chunk_rows), and the plan of the forced split on r0bits bits (*l0).
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
    const u64 tile = (u64)sk_tile_rows();
    u64 chunk_rows = std::max<u64>(4 * tile, (n + chunk_target - 1) / chunk_target);
    chunk_rows = (chunk_rows + tile - 1) / tile * tile;
    prof_mark(ctx, "sk_plan0");
    RC_TRY(sk_level_begin(ctx, ps, cur, 1, r0bits, (u32)chunk_rows, l0));
    *cur_out = cur;
    *chunk_rows_out = (u32)chunk_rows;
    return DNAGPU_OK;
}

// Level 0: the rows of the packed sequence -> records in the coarse buckets of geometry g.
// *rec0 = the record buffer (pool memory of ps), *coarse / *n_coarse = the 2^r0bits coarse nodes (device; start / len in
// records, in digit order), lens = their record counts on the host.
// (rec0_cap != null: the buffer is made large enough for the regions of a speculative level 1 -- sk_levels12 -- and
// *rec0_cap = the records it holds)
static int sk_level0(dnagpu_ctx *ctx, PoolScope &ps, const SkRows &rows, int k, const SkGeom &g, void **rec0_out, Node **coarse,
                     u32 *n_coarse, std::vector<u32> *lens_out, u64 *n_recs_out, u64 *rec0_cap = nullptr)
{
    hipStream_t st = ctx->stream;
    const dnagpu_dna *dna = rows.dna;
    const int b1 = g.b1, r0bits = g.r0bits;
    const u32 c0n = g.c0n;
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
    std::vector<u32> &lens = *lens_out;
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
    if (rec0_cap) {
        u64 span = 0;
        const bool even = sk_even(lens.data(), (u32)lens.size(), 1.02, b1, &span);
        if (span <= 0xFFFFFFFFull)
            cap = std::max(cap, span);
        // uneven coarse buckets (repeats): level 1's regions will come from a sampled histogram (sk_levels12), ~20 % of slack
        // on an ordinary mid bucket: room for a third more than the records
        if ((ctx->debug_flags & DNAGPU_DEBUG_SAMPLE1) || !even) {
            const u64 roomy = n_recs + n_recs / 3 + ((u64)lens.size() << b1) * 136;
            if (roomy <= 0xFFFFFFFFull)
                cap = std::max(cap, roomy);
        }
        *rec0_cap = cap;
    }
    RC_TRY(pool_alloc(ctx, (size_t)cap * 16, &rec0));
    ps.ptrs.push_back(rec0);
    prof_mark(ctx, "sk_scatter0");
    HIP_TRY(launch_sk_level0(true, l0.chunks, l0.n_chunks, dna->words, dna->n_words, rows.first, k, c0n, (u32)b1, (u32)r0bits,
                             l0.hist, l0.tot, rec0, st, nullptr, rows.marks, rows.n_mark_words));
    *rec0_out = rec0;
    *coarse = l0.next;
    *n_coarse = l0.n_next;
    *n_recs_out = n_recs;
    return DNAGPU_OK;
}

// Levels 1 and 2 over coarse nodes (records of rec0, which this takes over).  n = the k-mers the records must hold
// (0 = not known: records received from other ranks).  On success *n_kmers = the k-mers found.
// Level 0 WITHOUT its histogram sweep (the window minima are computed once): a histogram over 1/64 of the rows (chunks of
// four tiles, evenly spaced) gives every coarse bucket's share of a chunk's records; every chunk then reserves that share
// + 1/32 + six standard deviations + 24 slots in the bucket's region (one returning add per digit and chunk) and fills
// them as the exact sweep fills its histogram ranges; what it does not use becomes NULL records, which level 1 skips
// (~10 % of the slots at 3 Gbase).  *ok = false (nothing usable produced: the caller runs the exact pair) when the sampled
// buckets are uneven (repeats), when the regions pass 2^32 slots, or when a chunk ran out of slots.  On success the coarse
// nodes cover their whole regions (lens[d] slots, NULL records included) and *n_recs / *rec0_cap are slots.
constexpr u64 SK_SLAB_MIN_ROWS = (u64)1 << 29;     // (measured: 249 Mbase 2.16 vs 2.12 ms, 1 Gbase 8.31 vs 8.42, 3 Gbase 21.8 vs 22.4)
static int sk_level0_slab(dnagpu_ctx *ctx, PoolScope &ps, const SkRows &rows, int k, const SkGeom &g, void **rec0_out, Node **coarse,
                          u32 *n_coarse, std::vector<u32> *lens, u64 *n_recs, u64 *rec0_cap, bool *ok)
{
    hipStream_t st = ctx->stream;
    const dnagpu_dna *dna = rows.dna;
    const u64 first = rows.first, n = rows.n;
    *ok = false;
    const u32 r0n = 1u << g.r0bits;
    const u64 tile = (u64)sk_tile_rows();
    // (1024 chunks = one resident set of workgroups: a chunk's share of a bucket is then ~2,400 records, and the six
    // standard deviations of slack it needs are 12 % of them -- with the exact pair's 4096 chunks they would be 25 %)
    Node *cur = nullptr;
    u32 chunk_rows = 0;
    SkLevel l0;
    RC_TRY(sk_level0_begin(ctx, ps, n, g.r0bits, 1024, &cur, &chunk_rows, &l0));
    if (l0.n_chunks == 0)
        return DNAGPU_OK;
    // ---- the sample
    const u64 samp_len = 4 * tile, samp_stride = 64 * samp_len;
    const u32 n_samp = (u32)((n + samp_stride - 1) / samp_stride);
    u64 sampled = 0;
    for (u32 i = 0; i < n_samp; i++)
        sampled += std::min<u64>(samp_len, n - (u64)i * samp_stride);
    Chunk *samp = nullptr;
    u32 *est = nullptr, *slab = nullptr;
    Node *nodes = nullptr;
    RC_TRY(ps.alloc((size_t)n_samp, &samp));
    RC_TRY(ps.alloc((size_t)sk_max_c0(), &est));
    RC_TRY(ps.alloc((size_t)sk_slab_words(), &slab));
    RC_TRY(ps.alloc((size_t)r0n, &nodes));
    prof_mark(ctx, "sk_sample0");
    HIP_TRY(hipMemsetAsync(est, 0, (size_t)sk_max_c0() * sizeof(u32), st));
    HIP_TRY(launch_sk_sample_chunks(samp, n_samp, (u32)samp_stride, (u32)samp_len, (u32)n, st));
    HIP_TRY(launch_sk_level0(false, samp, n_samp, dna->words, dna->n_words, first, k, g.c0n, (u32)g.b1, (u32)g.r0bits, nullptr, nullptr,
                             nullptr, st, est, rows.marks, rows.n_mark_words));
    HIP_TRY(launch_sk_slab_init(est, (u32)g.r0bits, chunk_rows, (u32)sampled, l0.n_chunks, slab, nodes, st));
    std::vector<u32> h_est(r0n);
    RC_TRY(read_back(ctx, h_est.data(), est, (size_t)r0n * sizeof(u32)));
    // even buckets?  (a repeated stretch sends its records to the few buckets of its minimizers: see sk_levels12)
    u64 tot = 0, span = 0, span1 = 0;
    lens->assign(r0n, 0);
    for (u32 d = 0; d < r0n; d++) {
        tot += h_est[d];
        const u64 len = (u64)sk_slab_cap(h_est[d], chunk_rows, sampled) * l0.n_chunks;
        span += len;
        if (len > 0xFFFFFFFFull)
            return DNAGPU_OK;
        (*lens)[d] = (u32)len;
        span1 += sk_spec_span((u32)len, g.b1);
    }
    if (tot == 0 || !sk_even(h_est.data(), r0n, 1.05) || span > 0xFFFFFFFFull)
        return DNAGPU_OK;
    const u64 cap = std::max<u64>(span, span1 <= 0xFFFFFFFFull ? span1 : 0);
    void *rec0 = nullptr;
    RC_TRY(pool_alloc(ctx, (size_t)std::max<u64>(cap, 1) * 16, &rec0));
    prof_mark(ctx, "sk_scatter0");
    const hipError_t e = launch_sk_level0(true, l0.chunks, l0.n_chunks, dna->words, dna->n_words, first, k, g.c0n, (u32)g.b1,
                                          (u32)g.r0bits, nullptr, nullptr, rec0, st, slab, rows.marks, rows.n_mark_words);
    u32 status[2] = {1, 0};
    int rc = e == hipSuccess ? read_back(ctx, status, slab + 18 * (size_t)sk_max_c0(), sizeof status) : DNAGPU_ERR_HIP;
    if (rc != DNAGPU_OK || status[0] || status[1] != (u32)span || (ctx->debug_flags & DNAGPU_DEBUG_SLAB0_OVERFLOW)) {
        pool_free(ctx, rec0);                      // (ordered behind the sweep on this stream)
        if (e != hipSuccess)
            set_err("sk_scatter0 (slabs): %s", hipGetErrorString(e));
        return rc;
    }
    ps.ptrs.push_back(rec0);
    *rec0_out = rec0;
    *coarse = nodes;
    *n_coarse = r0n;
    *n_recs = span;
    *rec0_cap = cap;
    *ok = true;
    return DNAGPU_OK;
}

// host_lens / rec0_cap (optional): the coarse nodes' record counts on the host and the records rec0 has room for -- with
// both, level 1 runs WITHOUT its histogram where the regions fit (see sk_spec_span): mid buckets are regions of len / 2^b1
// + 12.5 % + 72 slots, the sweep reserves slots from cursors and counts the k-mers per mid bucket itself; a region that
// overflows (repeats) sends the level through the exact path (histogram, prefix, sweep).
static int sk_levels12(dnagpu_ctx *ctx, PoolScope &ps, const SkGeom &g, Node *coarse, u32 n_coarse, void *rec0, u64 n_recs, u64 n,
                       void **recs, Node **fin, u32 *n_fin, SkHeavy *heavy, u64 *n_kmers, const u32 *host_lens = nullptr,
                       u64 rec0_cap = 0)
{
    hipStream_t st = ctx->stream;
    const int b1 = g.b1;
    const u64 mid_limit = g.mid_limit;
    void *rec1 = nullptr;

    // ---- level 1: records of every coarse bucket -> 2^b1 mid buckets; k-mers per mid bucket on the way
    u64 chunk_recs = std::max<u64>(4 * 8192, (n_recs + 4095) / 4096);
    chunk_recs = (chunk_recs + 8191) / 8192 * 8192;
    prof_mark(ctx, "sk_plan1");
    SkLevel l1;
    RC_TRY(sk_level_begin(ctx, ps, coarse, n_coarse, b1, (u32)chunk_recs, &l1));
    u32 *kcount = nullptr;
    RC_TRY(ps.alloc(std::max<u32>(l1.n_next, 1), &kcount));
    HIP_TRY(hipMemsetAsync(kcount, 0, (size_t)std::max<u32>(l1.n_next, 1) * sizeof(u32), st));
    u32 *d_lens = nullptr;
    RC_TRY(ps.alloc((size_t)l1.n_next + 4, &d_lens));      // (+ the speculative sweep's three status words)
    u32 *gcur = nullptr;
    RC_TRY(ps.alloc((size_t)std::max<u32>(l1.n_chunks, 1) * ROW_STRIDE, &gcur));
    std::vector<u32> kc(l1.n_next), rcn((size_t)l1.n_next + 4);
    // mid-bucket k-mer and record counts to the host (the list is short), with `extra` words behind the record counts
    auto lens_to_host = [&](u32 extra) -> int {
        const size_t nb = (size_t)l1.n_next * sizeof(u32), nb2 = nb + (size_t)extra * sizeof(u32);
        if (nb + nb2 <= MAILBOX_BYTES - 8) {      // both lists through the pinned mailbox, one wait (its last word is read_back's flag)
            char *mb = reinterpret_cast<char *>(ctx->mailbox);
            HIP_TRY(hipMemcpyAsync(mb, kcount, nb, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(mb + nb, d_lens, nb2, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            memcpy(kc.data(), mb, nb);
            memcpy(rcn.data(), mb + nb, nb2);
        } else {
            HIP_TRY(hipMemcpyAsync(kc.data(), kcount, nb, hipMemcpyDeviceToHost, st));
            RC_TRY(read_back(ctx, rcn.data(), d_lens, nb2));
        }
        return DNAGPU_OK;
    };
    // ---- speculative: no histogram.  The regions must fit both record buffers (level 2 writes a mid bucket's final
    // buckets back into its range of rec0).
    u64 span = 0;
    bool even = true;
    if (host_lens) {
        // Repeats show at the coarse level already: a repeated stretch sends its records to the few buckets of its minimizers
        // (half a sequence of one tiled 1000-base motif doubles ~110 of 136 coarse buckets; random sequence fills them to
        // within 0.3 %).  Uneven coarse buckets (2 % over the mean of the non-empty ones) take the exact level at once,
        // instead of paying for a speculative sweep that will overflow.
        even = sk_even(host_lens, n_coarse, 1.02, b1, &span);
    }
    const bool can_spec = host_lens && !(ctx->debug_flags & DNAGPU_DEBUG_NO_SPEC1) && n_coarse <= (u32)sk_max_c0() && l1.n_chunks > 0;
    const bool force_sample = (ctx->debug_flags & DNAGPU_DEBUG_SAMPLE1) != 0;
    bool spec = can_spec && even && !force_sample && span <= rec0_cap && span <= 0xFFFFFFFFull;
    // ---- uneven coarse buckets (repeats): the regions from a SAMPLED histogram -- one piece of 1024 records in every eight
    // of a coarse bucket's, read once (an eighth of the records: ~0.15 ms at 3 Gbase against the exact histogram's 1.0 - 1.3)
    // -- estimate + five standard deviations + 128 slots per mid bucket, so that a heavy mid bucket gets a region of its
    // size.  One more wait for the host (the regions' total decides the buffer); a region that overflows all the same
    // (bursts the sample missed) falls back to the exact level like every speculative sweep.
    u32 *rstart = nullptr, *rcapv = nullptr;
    bool sampled = false;
    if (can_spec && (!even || force_sample) && !spec) {
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
        RC_TRY(ps.alloc(std::max<size_t>(samp.size(), 1), &d_samp));
        RC_TRY(ps.alloc((size_t)l1.n_next, &est));
        RC_TRY(ps.alloc((size_t)l1.n_next, &rcapv));
        RC_TRY(ps.alloc((size_t)l1.n_next, &rstart));
        RC_TRY(ps.alloc((size_t)scan_tmp_words(l1.n_next), &stmp));
        RC_TRY(ps.alloc(1, &tot1));
        prof_mark(ctx, "sk_sample1");
        if (!samp.empty())
            HIP_TRY(hipMemcpyAsync(d_samp, samp.data(), samp.size() * sizeof(Chunk), hipMemcpyHostToDevice, st));
        HIP_TRY(launch_sk_sampled_regions(coarse, d_samp, (u32)samp.size(), rec0, l1.n_next, est, rcapv, rstart, stmp, tot1, st));
        u32 total = 0;
        RC_TRY(read_back(ctx, &total, tot1, sizeof total));      // (also: samp has been consumed)
        // (the scan's total wraps past 2^32: regions that large are out of reach of 32-bit slots anyway -- the check below
        // compares against rec0's room, which is below 2^32)
        u64 chk = 0;
        for (u32 i = 0; i < n_coarse; i++)
            chk += host_lens[i];
        if ((u64)total >= chk && (u64)total <= rec0_cap) {
            span = total;
            spec = sampled = true;
        }
    }
    bool moved = false;
    if (spec) {
        u32 *sp = nullptr;
        RC_TRY(ps.alloc((size_t)2 * n_coarse, &sp));
        u32 *status = d_lens + l1.n_next;         // [0] slots of all regions, [1] past 2^32, [2] overflow
        prof_mark(ctx, "sk_spec1");
        HIP_TRY(launch_sk_spec_regions(coarse, n_coarse, sp, status, gcur, st, sampled ? rstart : nullptr));
        RC_TRY(pool_alloc(ctx, (size_t)std::max<u64>(std::max(n_recs, span), 1) * 16, &rec1));
        ps.ptrs.push_back(rec1);
        prof_mark(ctx, "sk_scatter1");
        HIP_TRY(launch_sk_scatter1_spec(coarse, l1.chunks, l1.n_chunks, rec0, rec1, gcur, sp, kcount, status + 2, st,
                                        sampled ? rstart : nullptr, sampled ? rcapv : nullptr));
        HIP_TRY(launch_sk_spec_nodes(coarse, n_coarse, sp, gcur, l1.next, status + 2, st, sampled ? rstart : nullptr,
                                     sampled ? rcapv : nullptr));
        HIP_TRY(launch_sk_node_lens(l1.next, l1.n_next, d_lens, st));
        RC_TRY(lens_to_host(3));
        const u32 *stw = rcn.data() + l1.n_next;
        if ((!sampled && stw[0] != (u32)span) || (!sampled && stw[1]) || stw[2] || (ctx->debug_flags & DNAGPU_DEBUG_SPEC1_OVERFLOW)) {
            spec = false;                          // (a region overflowed, or the test flag says so: the exact level, into the same rec1)
            HIP_TRY(hipMemsetAsync(kcount, 0, (size_t)std::max<u32>(l1.n_next, 1) * sizeof(u32), st));
        } else {
            moved = true;
        }
    }
    if (!spec) {
        prof_mark(ctx, "sk_hist1");
        HIP_TRY(launch_sk_hist1(coarse, l1.chunks, l1.n_chunks, rec0, l1.hist, kcount, st));
        prof_mark(ctx, "sk_prefix1");
        HIP_TRY(launch_level_prefix(coarse, l1.chunks, l1.n_chunks, n_coarse, (u32)chunk_recs, l1.hist, l1.tot, st, n_coarse));
        HIP_TRY(launch_level_children(coarse, n_coarse, l1.tot, l1.next, nullptr, nullptr, nullptr, 0, st));
        // ---- skew check on the k-mers per mid bucket, before their records move
        HIP_TRY(launch_sk_node_lens(l1.next, l1.n_next, d_lens, st));
        RC_TRY(lens_to_host(0));
    }
    // heavy: too many k-mers, or too many records for the one workgroup that regroups a mid bucket (its tiles are serial)
    const bool forced = (ctx->debug_flags & DNAGPU_DEBUG_FORCE_SUPERKMER) != 0;
    auto is_heavy = [&](u32 i) { return kc[i] > mid_limit || (!forced && rcn[i] > SK_MID_RECORDS); };
    u64 run = 0, heaviest = 0;
    for (u32 i = 0; i < l1.n_next; i++) {
        run += kc[i];
        if (is_heavy(i))
            heaviest = std::max<u64>(heaviest, std::max<u64>(kc[i], mid_limit + 1));
    }
    if (n != 0 && run != n) {
        set_err("super-k-mer partition lost rows: %llu of %llu", (unsigned long long)run, (unsigned long long)n);
        return DNAGPU_ERR_INTERNAL;
    }
    if (run > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    *n_kmers = run;
    std::vector<u32> heavy_idx;
    if (heaviest > mid_limit) {
        for (u32 i = 0; i < l1.n_next; i++)
            if (is_heavy(i)) {
                heavy_idx.push_back(i);
                heavy->total += kc[i];
            }
        // DNAGPU_SK_SKEWED leaves this function in two cases only: with DNAGPU_DEBUG_HEAVY_EXPAND (the older path, kept for
        // the tests: heavy mid buckets are expanded as a whole, and a set that is mostly heavy is cheaper through the tree
        // from scratch -- count_core -- or as one key node per coarse bucket -- count_sk_received; rec0 is still what it
        // was: level 1 only reads it), or with more heavy mid buckets than the chunked split below plans for (32768: not
        // reachable with 2^32 rows, a guard).
        if (((ctx->debug_flags & DNAGPU_DEBUG_HEAVY_EXPAND) && heavy->total * 2 > run) || heavy_idx.size() > 32768)
            return DNAGPU_SK_SKEWED;
    }

    if (!moved) {
        if (!rec1) {
            RC_TRY(pool_alloc(ctx, (size_t)std::max<u64>(n_recs, 1) * 16, &rec1));
            ps.ptrs.push_back(rec1);
        }
        prof_mark(ctx, "sk_scatter1");
        // the mid buckets' cursors start at their exact bases (the prefix of the histogram); tiles reserve their slots there
        HIP_TRY(hipMemcpyAsync(gcur, l1.tot, (size_t)std::max<u32>(l1.n_chunks, 1) * ROW_STRIDE * sizeof(u32), hipMemcpyDeviceToDevice, st));
        HIP_TRY(launch_sk_scatter1(coarse, l1.chunks, l1.n_chunks, rec0, rec1, l1.hist, l1.tot, st, false, gcur));
    }

    const u32 nh = (u32)heavy_idx.size();
    const bool heavy_expand = (ctx->debug_flags & DNAGPU_DEBUG_HEAVY_EXPAND) != 0;
    SkLevel lh;
    memset(&lh, 0, sizeof lh);
    u32 *kcount2 = nullptr;
    Node *hnodes = nullptr;
    if (nh) {
        // the heavy buckets leave the list here (empty nodes stay behind): one workgroup could not regroup them in time
        u32 *d_idx = nullptr;
        RC_TRY(ps.alloc((size_t)nh, &d_idx));
        RC_TRY(ps.alloc((size_t)nh, &hnodes));
        HIP_TRY(hipMemcpyAsync(d_idx, heavy_idx.data(), (size_t)nh * sizeof(u32), hipMemcpyHostToDevice, st));
        HIP_TRY(launch_sk_take_heavy(l1.next, d_idx, nh, kcount, hnodes, st));
        HIP_TRY(hipStreamSynchronize(st));       // (heavy_idx is a host vector)
        if (heavy_expand) {                      // (tests: the expansion of whole mid buckets)
            heavy->nodes = hnodes;
            heavy->n = nh;
            heavy->recs = rec1;
        } else {
            // They are split by d2 with the CHUNKED level kernels instead (many workgroups per bucket: plan, histogram,
            // prefix, children, scatter rec1 -> rec0 into the range the bucket would have been regrouped into); their
            // sixteen children join the final buckets, where sk_count_big takes the long ones slice by slice.
            u64 hrecs = 0;
            for (u32 i : heavy_idx)
                hrecs += rcn[i];
            u64 chunk_h = std::max<u64>(4 * 8192, (hrecs + 4095) / 4096);
            chunk_h = (chunk_h + 8191) / 8192 * 8192;
            prof_mark(ctx, "sk_heavy_split");
            RC_TRY(sk_level_begin(ctx, ps, hnodes, nh, 4, (u32)chunk_h, &lh));
            RC_TRY(ps.alloc(std::max<u32>(lh.n_next, 1), &kcount2));
            HIP_TRY(hipMemsetAsync(kcount2, 0, (size_t)std::max<u32>(lh.n_next, 1) * sizeof(u32), st));
            HIP_TRY(launch_sk_hist1(hnodes, lh.chunks, lh.n_chunks, rec1, lh.hist, kcount2, st, true));
            HIP_TRY(launch_level_prefix(hnodes, lh.chunks, lh.n_chunks, nh, (u32)chunk_h, lh.hist, lh.tot, st, nh));
            HIP_TRY(launch_level_children(hnodes, nh, lh.tot, lh.next, nullptr, nullptr, nullptr, 0, st));
            HIP_TRY(launch_sk_scatter1(hnodes, lh.chunks, lh.n_chunks, rec1, rec0, lh.hist, lh.tot, st, true));
            heavy->total = 0;                    // (nothing is left for the expansion of mid buckets)
        }
    }
    // ---- level 2: every mid bucket regrouped by d2 (rec1 -> rec0): 16 final buckets each
    Node *fn = nullptr;
    RC_TRY(ps.alloc((size_t)l1.n_next * 16 + lh.n_next, &fn));
    prof_mark(ctx, "sk_regroup");
    bool any_long = false;                       // (mid buckets of more than one regroup tile: repeats)
    for (u32 i = 0; i < l1.n_next && !any_long; i++)
        any_long = rcn[i] > (u32)sk_regroup_tile();
    HIP_TRY(launch_sk_regroup(l1.next, l1.n_next, rec1, rec0, fn, any_long, st));
    if (lh.n_next)
        HIP_TRY(launch_sk_heavy_finals(lh.next, lh.n_next, kcount2, fn + (size_t)l1.n_next * 16, st));
    if (nh == 0 || !heavy_expand)
        ps.free_now(rec1);
    *recs = rec0;
    *fin = fn;
    *n_fin = l1.n_next * 16 + lh.n_next;
    return DNAGPU_OK;
}

// The whole count: partition, then final buckets of at most sk_count_cap() k-mers are counted from their records
// (sk_count), the others expanded to keys and counted by the ordinary levels.  Fills h on success.
static int count_sk_tail(dnagpu_ctx *ctx, PoolScope &ps, void *recs, Node *fin, u32 n_fin, const SkHeavy &heavy, u64 n, int k,
                         dnagpu_hist *h)
{
    hipStream_t st = ctx->stream;
    const u32 n_heavy = heavy.n;
    prof_mark(ctx, "sk_select");
    const u32 cap = (u32)sk_count_cap();
    const u32 big_limit = (u32)SK_BIG_LIMIT;
    u32 *f_small = nullptr, *f_big = nullptr, *f_over = nullptr, *f_over_raw = nullptr, *k_over = nullptr, *k_range = nullptr,
        *scan_tmp = nullptr, *totals = nullptr, *list_small = nullptr, *off_small = nullptr, *list_big = nullptr, *off_big = nullptr;
    RC_TRY(ps.alloc((size_t)n_fin, &f_small));
    RC_TRY(ps.alloc((size_t)n_fin, &f_big));
    RC_TRY(ps.alloc((size_t)n_fin, &k_range));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n_fin) * 4, &scan_tmp));      // (four scans at a time: launch_scan_u32_multi)
    RC_TRY(ps.alloc(8, &totals));
    RC_TRY(ps.alloc((size_t)n_fin, &list_small));
    RC_TRY(ps.alloc((size_t)n_fin, &off_small));
    RC_TRY(ps.alloc((size_t)n_fin, &f_over));       // (first: the k-mers of the big buckets, summed)
    HIP_TRY(launch_sk_select_flags(fin, n_fin, cap, big_limit, f_small, f_big, k_range, f_over, st));
    {
        ScanSet ss;
        u32 *arr[4] = {f_small, f_big, k_range, f_over};
        for (int a = 0; a < 4; a++) {
            ss.in[a] = arr[a];
            ss.out[a] = arr[a];
            ss.total[a] = totals + a;
        }
        ss.tmp = scan_tmp;
        HIP_TRY(launch_scan_u32_multi(ss, 4, n_fin, st));
    }
    u32 ht[4] = {0, 0, 0, 0};
    RC_TRY(read_back(ctx, ht, totals, sizeof ht));
    const u32 n_small = ht[0], n_big = ht[1];
    const u64 small_keys = ht[2];                // the output slots of the small and big buckets: one per k-mer, in bucket order
    // a big bucket that sk_count_big gives up on is counted again through the expansion: its groups land behind the
    // ranges while its own range stays padding, so the arrays hold up to n + the big buckets' k-mers
    const u64 out_cap = n + ht[3];
    RC_TRY(ps.alloc((size_t)std::max<u32>(n_big, 1), &list_big));
    RC_TRY(ps.alloc((size_t)std::max<u32>(n_big, 1), &off_big));
    HIP_TRY(launch_sk_select_lists(fin, n_fin, cap, big_limit, f_small, f_big, k_range, list_small, off_small, list_big, off_big, st));

    // output arrays and the segment directory: final buckets first, the nodes of the oversize buckets' tree behind them
    u64 *cursor = nullptr, *ok = nullptr;
    u32 *oc = nullptr;
    // [0] next free output slot of the leaves behind the buckets' ranges; [1] buckets whose expansion disagrees with the
    // partition's count; [2] groups sk_count and sk_count_big wrote
    RC_TRY(ps.alloc(3, &cursor));
    RC_TRY(ps.alloc((size_t)out_cap, &ok));
    RC_TRY(ps.alloc((size_t)out_cap, &oc));
    {
        const u64 init[3] = {small_keys, 0, 0};
        HIP_TRY(poke(cursor, init, sizeof init, st));
    }
    u64 *seg_off = nullptr;
    u32 *seg_cnt = nullptr;
    // (the directory of the final buckets; the tree's nodes get a second one behind it once their number is known)
    u64 *seg_off_fin = nullptr;
    u32 *seg_cnt_fin = nullptr;
    RC_TRY(ps.alloc((size_t)std::max<u32>(n_fin, 1), &seg_off_fin));
    RC_TRY(ps.alloc((size_t)std::max<u32>(n_fin, 1), &seg_cnt_fin));
    HIP_TRY(hipMemsetAsync(seg_cnt_fin, 0, (size_t)n_fin * sizeof(u32), st));     // empty and expanded buckets: no groups of their own
    HIP_TRY(hipMemsetAsync(seg_off_fin, 0, (size_t)n_fin * sizeof(u64), st));
    // ---- long buckets of few distinct keys (repeats): one table per bucket; what outgrows it joins the expansion below
    u32 *big_status = nullptr;
    RC_TRY(ps.alloc((size_t)std::max<u32>(n_big, 1), &big_status));
    if (n_big) {
        prof_mark(ctx, "sk_count_big");
        // work items: slices of the buckets' records; a bucket of several slices gets a partial area per slice
        u32 *nsl = nullptr, *sfirst = nullptr, *mfirst = nullptr, *sl_bucket = nullptr, *sl_idx = nullptr, *part_n = nullptr, *part_cnts = nullptr;
        u64 *part_keys = nullptr;
        RC_TRY(ps.alloc((size_t)n_big, &nsl));
        RC_TRY(ps.alloc((size_t)n_big, &sfirst));
        RC_TRY(ps.alloc((size_t)n_big, &mfirst));
        HIP_TRY(launch_sk_big_slices(fin, list_big, n_big, nsl, mfirst, st));
        HIP_TRY(launch_scan_u32(nsl, sfirst, n_big, scan_tmp, totals + 6, st));
        HIP_TRY(launch_scan_u32(mfirst, mfirst, n_big, scan_tmp, totals + 7, st));
        u32 hs[2] = {0, 0};
        RC_TRY(read_back(ctx, hs, totals + 6, sizeof hs));
        const u32 n_slices = hs[0], n_part = hs[1];
        RC_TRY(ps.alloc((size_t)std::max<u32>(n_slices, 1), &sl_bucket));
        RC_TRY(ps.alloc((size_t)std::max<u32>(n_slices, 1), &sl_idx));
        RC_TRY(ps.alloc((size_t)std::max<u32>(n_part, 1), &part_n));
        RC_TRY(ps.alloc((size_t)std::max<u32>(n_part, 1) * sk_big_partial_slots(), &part_keys));
        RC_TRY(ps.alloc((size_t)std::max<u32>(n_part, 1) * sk_big_partial_slots(), &part_cnts));
        HIP_TRY(launch_sk_big_slice_fill(nsl, sfirst, n_big, sl_bucket, sl_idx, st));
        HIP_TRY(launch_sk_count_big(fin, list_big, off_big, nsl, mfirst, sl_bucket, sl_idx, n_slices, n_big, recs, k, cursor + 2,
                                    seg_off_fin, seg_cnt_fin, ok, oc, big_status, part_keys, part_cnts, part_n, n_part > 0, st));
    }
    prof_mark(ctx, "sk_select_over");
    RC_TRY(ps.alloc((size_t)n_fin, &f_over_raw));
    RC_TRY(ps.alloc((size_t)n_fin, &k_over));
    HIP_TRY(launch_sk_over_flags(fin, n_fin, cap, big_limit, f_big, big_status, f_over_raw, k_over, st));
    {
        ScanSet ss;
        memset(&ss, 0, sizeof ss);
        ss.in[0] = f_over_raw;
        ss.out[0] = f_over;
        ss.total[0] = totals + 4;
        ss.in[1] = k_over;
        ss.out[1] = k_over;
        ss.total[1] = totals + 5;
        ss.tmp = scan_tmp;
        HIP_TRY(launch_scan_u32_multi(ss, 2, n_fin, st));
    }
    u32 ho[2] = {0, 0};
    RC_TRY(read_back(ctx, ho, totals + 4, sizeof ho));
    const u32 n_over = ho[0];
    const u64 over_keys = ho[1];
    Node *over_nodes = nullptr;
    u32 *over_kbase = nullptr;
    RC_TRY(ps.alloc((size_t)std::max<u32>(n_over, 1), &over_nodes));
    RC_TRY(ps.alloc((size_t)std::max<u32>(n_over, 1), &over_kbase));
    HIP_TRY(launch_sk_over_list(fin, n_fin, f_over_raw, f_over, k_over, over_nodes, over_kbase, st));
    TreeResult tr;
    memset(&tr, 0, sizeof tr);
    if (n_over + n_heavy > 0) {
        // oversize final buckets (the tail of the size distribution, moderate repeats) and heavy mid buckets (the
        // minimizers of long repeats): keys, then the ordinary levels with their skew paths.  Every such bucket becomes
        // one key node; its records are expanded in slices by many waves at once.
        const u64 tree_keys = over_keys + heavy.total;
        if (tree_keys > 0xFFFFFFFFull)
            return DNAGPU_ERR_TOO_LARGE;
        const u32 n_tree = n_over + n_heavy;
        u64 *kbuf = nullptr;
        Node *knodes = nullptr;
        RC_TRY(ps.alloc((size_t)tree_keys, &kbuf));
        RC_TRY(ps.alloc((size_t)n_tree, &knodes));
        prof_mark(ctx, "sk_expand_flat");
        // the final buckets live in `recs`, the heavy mid buckets in heavy.recs -> two slice lists; the key ranges: the
        // oversize final buckets in list order, the heavy buckets behind them
        for (int part = 0; part < 2; part++) {
            const u32 nb = part == 0 ? n_over : n_heavy;
            if (nb == 0)
                continue;
            const void *rbuf = part == 0 ? recs : heavy.recs;
            const Node *bk = part == 0 ? over_nodes : heavy.nodes;     // (start / len in records, child_base = k-mers)
            u32 *sfirst = nullptr, *stmp = nullptr, *stot = nullptr;
            RC_TRY(ps.alloc((size_t)nb, &sfirst));
            RC_TRY(ps.alloc((size_t)scan_tmp_words(nb), &stmp));
            RC_TRY(ps.alloc(2, &stot));
            HIP_TRY(launch_sk_slice_count(bk, nb, sfirst, st));
            HIP_TRY(launch_scan_u32(sfirst, sfirst, nb, stmp, stot, st));
            u32 n_slices = 0;
            RC_TRY(read_back(ctx, &n_slices, stot, 4));
            u32 *d_r0 = nullptr, *d_nr = nullptr, *d_ko = nullptr, *ktmp = nullptr;
            RC_TRY(ps.alloc((size_t)std::max<u32>(n_slices, 1), &d_r0));
            RC_TRY(ps.alloc((size_t)std::max<u32>(n_slices, 1), &d_nr));
            RC_TRY(ps.alloc((size_t)std::max<u32>(n_slices, 1), &d_ko));
            RC_TRY(ps.alloc((size_t)scan_tmp_words(std::max<u32>(n_slices, 1)), &ktmp));
            HIP_TRY(launch_sk_slice_fill(bk, nb, sfirst, d_r0, d_nr, st));
            HIP_TRY(launch_sk_slice_kmers(rbuf, d_r0, d_nr, n_slices, d_ko, st));
            HIP_TRY(launch_scan_u32(d_ko, d_ko, n_slices, ktmp, stot + 1, st));
            const u32 key_base = part == 0 ? 0u : (u32)over_keys;
            HIP_TRY(launch_sk_slice_nodes(bk, nb, sfirst, d_ko, n_slices, stot + 1, key_base, k, part == 0 || heavy.counted,
                                          knodes + (part == 0 ? 0 : n_over), cursor + 1, st));
            HIP_TRY(launch_sk_expand_flat(rbuf, d_r0, d_nr, d_ko, key_base, n_slices, k, kbuf, st));
        }
        RC_TRY(run_tree(ctx, ps, nullptr, 0, tree_keys, k, kbuf, 0, &tr, 0, 0, true, 0, ~0u, 0, knodes, n_tree, 2));
    }
#ifdef DNAGPU_STAMPS
    fprintf(stderr, "[sk select] n_fin %u small %u big %u (k-mers of big %u) over %u (keys %llu) heavy %u (keys %llu) tree nodes %u tiny %u small %u big %u\n",
            n_fin, n_small, n_big, ht[3], n_over, (unsigned long long)over_keys, n_heavy, (unsigned long long)heavy.total, tr.n_nodes,
            tr.n_tiny, tr.n_small, tr.n_big);
#endif
    const u32 n_segs = n_fin + tr.n_nodes;
    RC_TRY(ps.alloc((size_t)n_segs, &seg_off));
    RC_TRY(ps.alloc((size_t)n_segs, &seg_cnt));
    HIP_TRY(hipMemcpyAsync(seg_cnt, seg_cnt_fin, (size_t)n_fin * sizeof(u32), hipMemcpyDeviceToDevice, st));   // (sk_count_big's entries)
    HIP_TRY(hipMemcpyAsync(seg_off, seg_off_fin, (size_t)n_fin * sizeof(u64), hipMemcpyDeviceToDevice, st));
    if (tr.n_nodes > 0) {
        u32 *flags = nullptr, *ltmp = nullptr, *cls_list = nullptr;
        RC_TRY(ps.alloc((size_t)tr.n_nodes + 1, &flags));
        RC_TRY(ps.alloc((size_t)scan_tmp_words(tr.n_nodes), &ltmp));
        RC_TRY(ps.alloc((size_t)tr.n_nodes, &cls_list));
        prof_mark(ctx, "leaves");
        HIP_TRY(launch_leaves(tr.nodes, tr.n_nodes, tr.n_tiny, tr.n_small, tr.n_big, tr.buf0, tr.buf1, cursor, seg_off + n_fin,
                              seg_cnt + n_fin, ok, oc, flags, ltmp, cls_list, st, true, small_keys));
        HIP_TRY(launch_sk_unmix(ok, small_keys, cursor, tr.n_keys, k, st));      // (sk_expand_flat wrote key_mix(key))
    }
    prof_mark(ctx, "sk_count");
    u32 *left = nullptr;
    RC_TRY(ps.alloc((size_t)2 * n_small + 1, &left));
    HIP_TRY(launch_sk_count(fin, list_small, off_small, n_small, recs, k, cursor + 2, seg_off, seg_cnt, ok, oc, left, st));
#ifdef DNAGPU_STAMPS
    {
        u32 nl = 0;
        RC_TRY(read_back(ctx, &nl, left + 2 * (size_t)n_small, 4));
        fprintf(stderr, "[sk count] %u small buckets, %u left to sk_count by sk_count_clean\n", n_small, nl);
    }
#endif
    prof_mark(ctx, "end");
    u64 fin_ctr[3] = {0, 0, 0};
    RC_TRY(read_back(ctx, fin_ctr, cursor, 24));
    const u64 extent = fin_ctr[0];
    const u64 total_groups = fin_ctr[2] + (extent - small_keys);
    if (fin_ctr[1] != 0) {
        set_err("super-k-mer count: %llu buckets whose records expand to a different number of k-mers than the partition counted",
                (unsigned long long)fin_ctr[1]);
        return DNAGPU_ERR_INTERNAL;
    }
    if (extent > out_cap) {
        set_err("super-k-mer count: %llu output slots used, %llu allocated", (unsigned long long)extent, (unsigned long long)out_cap);
        return DNAGPU_ERR_INTERNAL;
    }
    if (total_groups > n) {
        set_err("super-k-mer count: %llu groups for %llu rows", (unsigned long long)total_groups, (unsigned long long)n);
        return DNAGPU_ERR_INTERNAL;
    }
    h->total = n;
    hist_adopt(ps, h, ok, oc, seg_off, seg_cnt, n_segs, total_groups, false, extent);
    return DNAGPU_OK;
}

int dnagpu::count_sk(dnagpu_ctx *ctx, const SkRows &rows, int k, dnagpu_hist *h, u64 n_kmers_expected)
{
    PoolScope ps(ctx);
    const SkGeom g = sk_geometry(ctx, std::max<u64>(n_kmers_expected, 1), k);
    void *rec0 = nullptr, *recs = nullptr;
    Node *coarse = nullptr, *fin = nullptr;
    u32 n_coarse = 0, n_fin = 0;
    u64 n_recs = 0, n_kmers = 0;
    SkHeavy heavy;
    u64 rec0_cap = 0;
    std::vector<u32> lens;
    bool slabs = false;
    const unsigned dbg = ctx->debug_flags;
    if (!(dbg & DNAGPU_DEBUG_NO_SLAB0) && (rows.n >= SK_SLAB_MIN_ROWS || (dbg & (DNAGPU_DEBUG_SLAB0 | DNAGPU_DEBUG_SLAB0_OVERFLOW))))
        RC_TRY(sk_level0_slab(ctx, ps, rows, k, g, &rec0, &coarse, &n_coarse, &lens, &n_recs, &rec0_cap, &slabs));
    if (!slabs)
        RC_TRY(sk_level0(ctx, ps, rows, k, g, &rec0, &coarse, &n_coarse, &lens, &n_recs, &rec0_cap));
    RC_TRY(sk_levels12(ctx, ps, g, coarse, n_coarse, rec0, n_recs, n_kmers_expected, &recs, &fin, &n_fin, &heavy, &n_kmers,
                       lens.size() == n_coarse ? lens.data() : nullptr, rec0_cap));
    return count_sk_tail(ctx, ps, recs, fin, n_fin, heavy, n_kmers_expected, k, h);
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
    const u32 n_coarse = 1u << g.r0bits;
    const u64 n_recs = boff[n_coarse];
    std::vector<Node> hn(n_coarse);
    for (u32 d = 0; d < n_coarse; d++) {
        memset(&hn[d], 0, sizeof(Node));
        hn[d].start = (u32)boff[d];
        hn[d].len = (u32)blen[d];
        hn[d].meta = (u32)(32 - g.r0bits);       // (what level_children leaves a child of the 32-"bit" root)
    }
    Node *coarse = nullptr;
    RC_TRY(ps.alloc((size_t)n_coarse, &coarse));
    HIP_TRY(hipMemcpyAsync(coarse, hn.data(), (size_t)n_coarse * sizeof(Node), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));           // (hn, and the caller's pieces, are free again)
    void *recs = nullptr;
    Node *fin = nullptr;
    u32 n_fin = 0;
    u64 n_kmers = 0;
    SkHeavy heavy;
    std::vector<u32> lens(n_coarse);
    for (u32 d = 0; d < n_coarse; d++)
        lens[d] = (u32)blen[d];
    int rc = sk_levels12(ctx, ps, g, coarse, n_coarse, rec0, n_recs, 0, &recs, &fin, &n_fin, &heavy, &n_kmers, lens.data(), rec0_cap);
    if (rc == DNAGPU_SK_SKEWED) {
        // every coarse bucket as one "heavy" bucket: keys, then the ordinary levels (sk_levels12 has not moved anything yet)
        heavy = SkHeavy();
        heavy.nodes = coarse;
        heavy.n = n_coarse;
        heavy.recs = rec0;
        heavy.total = n_kmers;
        heavy.counted = false;
        n_fin = 0;
        rc = DNAGPU_OK;
    }
    RC_TRY(rc);
    return count_sk_tail(ctx, ps, recs, fin, n_fin, heavy, n_kmers, k, h);
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
        void *rec0 = nullptr;
        Node *coarse = nullptr;
        u32 n_coarse = 0;
        u64 n_recs = 0;
        std::vector<u32> lens;
        prof_begin(ctx);
        const int rc = sk_level0(ctx, ps, SkRows{dna, first, count, nullptr, 0}, k, g, &rec0, &coarse, &n_coarse, &lens, &n_recs);
        prof_mark(ctx, "end");
        prof_end(ctx);
        RC_TRY(rc);
        for (u32 d = 0; d < g.c0n; d++)
            r->off[d + 1] = r->off[d] + (d < lens.size() ? lens[d] : 0);
        const hipError_t se = hipStreamSynchronize(ctx->stream);
        if (r->off[g.c0n] != n_recs || se != hipSuccess) {
            set_err("super-k-mer level 0: %llu records in the buckets, %llu counted (%s)", (unsigned long long)r->off[g.c0n],
                    (unsigned long long)n_recs, hipGetErrorString(se));
            return se != hipSuccess ? DNAGPU_ERR_HIP : DNAGPU_ERR_INTERNAL;
        }
        ps.release(rec0);
        r->recs = rec0;
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
