// count_host.hip -- GROUP BY kmer, count(*): the level loop of the tree, the dense count, the choice of engine
// (count_core) and the entry points over it, the counts over a table of sequences.  Host side only.
#include "host_common.hpp"

using namespace dnagpu;

// GROUP BY kmer, count(*): the level loop
static const char *const LEVEL_HIST_NAMES[] = {"level0_hist", "level1_hist", "level2_hist", "level3_hist", "levelN_hist"};
static const char *const LEVEL_PREFIX_NAMES[] = {"level0_prefix", "level1_prefix", "level2_prefix", "level3_prefix", "levelN_prefix"};
static const char *const LEVEL_SCATTER_NAMES[] = {"level0_scatter", "level1_scatter", "level2_scatter", "level3_scatter", "levelN_scatter"};
static const char *const LEVEL_PLAN_NAMES[] = {"level0_plan", "level1_plan", "level2_plan", "level3_plan", "levelN_plan"};

int dnagpu::run_tree(dnagpu_ctx *ctx, PoolScope &ps, const dnagpu_dna *dna, u64 first, u64 n, int k, u64 *keys_in, int force_bits,
                     TreeResult *res, int fixed_bits, u64 fixed_prefix, bool single_level, u32 flt_lo, u32 flt_span, u32 flt_tb,
                     Node *init_nodes, u32 init_n, int start_level)
{
    hipStream_t st = ctx->stream;
    u64 *buf0 = keys_in, *buf1 = nullptr;
    Node root;
    memset(&root, 0, sizeof root);
    root.start = 0;
    root.len = (u32)n;
    root.meta = (u32)(2 * k - fixed_bits);      // bits every key is known to share are not split on
    root.prefix = fixed_prefix;
    bool src_dna = false;
    u64 n_keys = n;
    if (dna) {
        if (n <= (u64)LEAF_CAP && force_bits == 0) {
            RC_TRY(ps.alloc((size_t)n, &buf0));
            HIP_TRY(launch_extract(dna->words, dna->n_words, first, n, k, buf0, st));
        } else {
            src_dna = true;                 // buffer 0 is allocated once level 0 knows how many keys it keeps
            root.meta |= NODE_BUF;          // children of the dna root go to buffer 0
        }
    }
    Node *cur = init_nodes;
    u32 n_nodes = init_nodes ? init_n : 1u, n_big = 0, n_small = 0, n_tiny = 0;
    if (!init_nodes) {
        RC_TRY(ps.alloc(1, &cur));
        static_assert(sizeof(Node) == 32, "a node travels as one kernel argument");
        HIP_TRY(poke(cur, &root, sizeof root, st));
    }
    u32 n_nonempty = 1;           // nodes of the current level that uniform data would fill (all, or an owner's share)

    static u64 chunk_target = 0;                 // chunks per level (work units of the hist/scatter kernels)
    if (chunk_target == 0) {
        const char *e = diag_env("DNAGPU_CHUNKS");       // experiment switch: diagnostic build (make STAMPS=1) only
        chunk_target = e ? (u64)atoll(e) : 4096;
        if (chunk_target < 256)
            chunk_target = 256;
    }
    u32 chunk_len = (u32)std::max<u64>(4 * (u64)scatter_tile_keys(), (n + chunk_target - 1) / chunk_target);
    chunk_len = (chunk_len + scatter_tile_keys() - 1) / scatter_tile_keys() * scatter_tile_keys();

    for (int level = start_level;; level++) {
        const int li = std::min(level, 4);
        prof_mark(ctx, LEVEL_PLAN_NAMES[li]);
        u32 *outc = nullptr, *nch = nullptr, *scan_tmp = nullptr;
        LevelCounters *ctr = nullptr;
        RC_TRY(ps.alloc(n_nodes, &outc));
        RC_TRY(ps.alloc(n_nodes, &nch));
        RC_TRY(ps.alloc((size_t)scan_tmp_words(n_nodes), &scan_tmp));
        RC_TRY(ps.alloc(1, &ctr));
        HIP_TRY(launch_plan_level(cur, n_nodes, (force_bits > 0 && level == 0) ? -force_bits : level, chunk_len, outc, nch,
                                  scan_tmp, ctr, st, init_nodes ? start_level + 1 : 2));
        LevelCounters hc;
        RC_TRY(read_back(ctx, &hc, ctr, sizeof hc));
        if (hc.n_split == 0) {
            n_big = hc.n_big;                    // every node of the final list was planned (and counted) here
            n_small = hc.n_small;
            n_tiny = hc.n_tiny;
            ps.free_now(outc);
            ps.free_now(nch);
            ps.free_now(scan_tmp);
            ps.free_now(ctr);
            break;
        }
        u32 n_nonempty_next = 0;
        Chunk *chunks = nullptr;
        u32 *hist = nullptr, *tot = nullptr;
        Node *next = nullptr;
        RC_TRY(ps.alloc(hc.n_chunks, &chunks));
        RC_TRY(ps.alloc((size_t)hc.n_chunks * ROW_STRIDE, &hist));
        RC_TRY(ps.alloc((size_t)hc.n_chunks * ROW_STRIDE, &tot));
        RC_TRY(ps.alloc(hc.n_next, &next));
        // key-source levels: level_hist also finds, per node, how many low key bits vary (see level_children)
        // (levels 0-1: only for nodes a quarter or more above the level's mean size -- none in uniform data, whose
        // level-1 histogram then costs 4.05 instead of 4.3 ms at 3 Gbase; deeper: every node)
        const u32 stat_min_len = level >= 2 ? 0u : (u32)std::min<u64>((n_keys / n_nonempty + 1) * 5 / 4, 0xffffffffull);
        u32 *vary = nullptr;
        if (!src_dna && !(force_bits > 0 && level == 0)) {
            RC_TRY(ps.alloc((size_t)n_nodes * NODE_STAT_WORDS, &vary));
            HIP_TRY(hipMemsetAsync(vary, 0, (size_t)n_nodes * NODE_STAT_WORDS * sizeof(u32), st));
        }
        HIP_TRY(launch_fill_chunks(cur, n_nodes, chunk_len, outc, nch, cur, chunks, st));
        prof_mark(ctx, LEVEL_HIST_NAMES[li]);
        HIP_TRY(launch_level_hist(cur, chunks, hc.n_chunks, src_dna, dna ? dna->words : nullptr,
                                  dna ? dna->n_words : 0, first, k, buf0, buf1, hist, src_dna ? flt_lo : 0u,
                                  src_dna ? flt_span : ~0u, src_dna ? flt_tb : 0u, vary, level >= 2 ? 1 : 0, stat_min_len, st));
        prof_mark(ctx, LEVEL_PREFIX_NAMES[li]);
        HIP_TRY(launch_level_prefix(cur, chunks, hc.n_chunks, hc.n_split, chunk_len, hist, tot, st, n_nodes));
        HIP_TRY(launch_level_children(cur, n_nodes, tot, next, vary, buf0, buf1, stat_min_len, st));
        if (src_dna) {
            // the dna root's children say how many keys survive the owner filter
            std::vector<Node> kids(hc.n_next);
            RC_TRY(read_back(ctx, kids.data(), next, (size_t)hc.n_next * sizeof(Node)));
            n_keys = 0;
            for (const Node &c : kids)
                n_keys += c.len;
            if (flt_span != ~0u && flt_span > 0 && flt_span < hc.n_next)
                n_nonempty_next = flt_span;       // an owner's digits: the other children are empty by construction
            RC_TRY(ps.alloc((size_t)std::max<u64>(n_keys, 1), &buf0));
        }
        if (hc.n_scatter) {
            if (!src_dna && !buf1)
                RC_TRY(ps.alloc((size_t)std::max<u64>(n_keys, 1), &buf1));
            prof_mark(ctx, LEVEL_SCATTER_NAMES[li]);
            HIP_TRY(launch_level_scatter(cur, chunks, hc.n_chunks, src_dna, dna ? dna->words : nullptr,
                                         dna ? dna->n_words : 0, first, k, buf0, buf1, hist, tot,
                                         src_dna ? flt_lo : 0u, src_dna ? flt_span : ~0u, src_dna ? flt_tb : 0u, hc.max_bits, st));
            if (vary)                   // nodes dominated by one key: three-way split around it (returns at once if none)
                HIP_TRY(launch_peel_scatter(cur, n_nodes, chunks, hc.n_chunks, next, buf0, buf1, vary, st));
        }
        ps.free_now(outc);
        ps.free_now(nch);
        ps.free_now(scan_tmp);
        ps.free_now(ctr);
        ps.free_now(chunks);
        ps.free_now(hist);
        ps.free_now(tot);
        if (vary)
            ps.free_now(vary);
        ps.free_now(cur);
        cur = next;
        n_nodes = hc.n_next;
        n_nonempty = n_nonempty_next ? n_nonempty_next : (n_nodes ? n_nodes : 1u);
        src_dna = false;
        if (force_bits > 0 && single_level)
            break;
    }
    res->nodes = cur;
    res->n_nodes = n_nodes;
    res->n_big = n_big;
    res->n_small = n_small;
    res->n_tiny = n_tiny;
    res->n_keys = n_keys;
    res->buf0 = buf0;
    res->buf1 = buf1;
    return DNAGPU_OK;
}

bool dnagpu::dense_pays(u64 n, int k)
{
    return 2 * k <= dense_max_bits() && n > (u64)LEAF_CAP && n >= ((u64)(2 * k > 16 ? 64 : 4) << (2 * k));
}

// any_order: the caller does not need ascending keys across the whole result (dnagpu_count_kmers_unordered): long
// k-mers of long sequences then go through the super-k-mer engine
constexpr u64 SK_MIN_ROWS = (u64)1 << 25;
// the engine pays once the runs are long enough (mean (k - 13) / 2 k-mers per record) and the sequence is: measured at
// 1 Gbase, tree vs this engine: k = 23 13.4 vs 13.1 ms, 24 13.2 vs 12.4, 25 13.2 vs 12.0, 27 13.2 vs 11.5, 29 13.0 vs 10.8;
// k = 31: 16 Mbase 0.63 vs 0.63 ms, 64 Mbase 1.32 vs 1.11, 250 Mbase 3.70 vs 3.21, 3 Gbase 42.0 vs 30.5
// k = 21 and 22 (13-base minimizers: runs of 5 - 5.5 k-mers; the multi-GPU record exchange uses the engine from k = 21
// whatever the size) gain less, and lose on the longest sequences, where the tree's passes run at their best
// (tools/engine_probe.py, tree vs records: k = 21 0.93 vs 0.91 ms at 50 Mbase, 1.64 vs 1.58 at 100 Mbase, 3.53 vs 3.34 at
// 250 Mbase, 13.1 vs 13.2 at 1 Gbase, 42.2 vs 44.7 at 3 Gbase; k = 22 0.90 vs 0.86, 1.62 vs 1.50, 3.52 vs 3.12, 13.1 vs 12.2,
// 42.1 vs 43.4; k = 23 1.62 vs 1.43, 13.0 vs 11.7, 42.1 vs 36.8): they take the engine up to 2^29 (k = 21) and 2^31 (k = 22) rows
constexpr int SK_MIN_K = 23;
static bool sk_is_default(u64 n, int k)
{
    if (n < SK_MIN_ROWS)
        return false;
    if (k >= SK_MIN_K)
        return true;
    // (k = 20: 12-base minimizers keep the final buckets even up to ~2^28 rows)
    return (k == 22 && n <= ((u64)1 << 31)) || (k == 21 && n <= ((u64)1 << 29)) || (k == 20 && n <= ((u64)1 << 28));
}

// short k-mers: the histogram is a table of at most 262,144 counters filled straight from the
// packed sequence (no key is ever written); one segment, keys ascending
static int count_dense(dnagpu_ctx *ctx, const dnagpu_dna *dna, u64 first, u64 n, int k, dnagpu_hist *h)
{
    PoolScope ps(ctx);
    const int bits = 2 * k;
    const size_t n_bins = (size_t)1 << bits;
    u32 *table = nullptr, *oc = nullptr;
    u64 *ok = nullptr, *n_out = nullptr;
    RC_TRY(ps.alloc(n_bins, &table));
    RC_TRY(ps.alloc(n_bins, &ok));
    RC_TRY(ps.alloc(n_bins, &oc));
    RC_TRY(ps.alloc(1, &n_out));
    prof_mark(ctx, "dense_count");
    HIP_TRY(launch_dense_count(dna->words, dna->n_words, first, n, bits, table, ok, oc, n_out, ctx->stream));
    prof_mark(ctx, "end");
    u64 D = 0;
    HIP_TRY(hipMemcpyAsync(&D, n_out, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    h->total = n;
    return hist_adopt_one_segment(ctx, ps, h, ok, oc, D, true);
}

// sharded count: the digits of level 0 (obits of them) that `owner` of n_owners owns = [*d_lo, *d_lo + *span); *tb != 0:
// the range is the digits whose top *tb bits equal the owner's
static void owner_range(int k, int owner, int n_owners, int *obits_out, u32 *d_lo_out, u32 *span_out, u32 *tb_out)
{
    const int obits = std::min(2 * k, MAX_SPLIT_BITS);
    const u32 R = 1u << obits;
    const u32 d_lo = (u32)(((u64)owner * R + n_owners - 1) / n_owners);
    const u32 d_hi = (u32)(((u64)(owner + 1) * R + n_owners - 1) / n_owners);
    const u32 span = d_hi > d_lo ? d_hi - d_lo : 0u;
    // aligned power-of-two range (every power-of-two GPU count): the kernels test top bits only
    u32 tb = 0;
    if (span && (span & (span - 1)) == 0 && d_lo % span == 0 && span < R) {
        int lg = 0;
        while ((1u << lg) < span)
            lg++;
        tb = (u32)(obits - lg);
    }
    *obits_out = obits;
    *d_lo_out = d_lo;
    *span_out = span;
    *tb_out = tb;
}

// the level loop (run_tree), then the leaves: segments in ascending key order
static int count_tree(dnagpu_ctx *ctx, const dnagpu_dna *dna, u64 first, u64 n, int k, u64 *keys_in, dnagpu_hist *h, int fixed_bits,
                      u64 fixed_prefix, int owner, int n_owners)
{
    PoolScope ps(ctx);
    TreeResult tr;
    if (n_owners > 1) {
        // sharded count: level 0 is forced onto the owner digits and keeps only this owner's keys
        int obits = 0;
        u32 d_lo = 0, span = 0, tb = 0;
        owner_range(k, owner, n_owners, &obits, &d_lo, &span, &tb);
        RC_TRY(run_tree(ctx, ps, dna, first, n, k, keys_in, obits, &tr, 0, 0, false, d_lo, span, tb));
    } else {
        RC_TRY(run_tree(ctx, ps, dna, first, n, k, keys_in, 0, &tr, fixed_bits, fixed_prefix));
    }
    u64 *cursor = nullptr, *seg_off = nullptr, *ok = nullptr;
    u32 *seg_cnt = nullptr, *oc = nullptr;
    // a k-mer of k bases has at most 4^k distinct values
    u64 cap = std::max<u64>(tr.n_keys, 1);
    if (k < 16)
        cap = std::min<u64>(cap, (u64)1 << (2 * k));
    RC_TRY(ps.alloc(1, &cursor));
    RC_TRY(ps.alloc(tr.n_nodes, &seg_off));
    RC_TRY(ps.alloc(tr.n_nodes, &seg_cnt));
    RC_TRY(ps.alloc((size_t)cap, &ok));
    RC_TRY(ps.alloc((size_t)cap, &oc));
    u32 *flags = nullptr, *scan_tmp = nullptr, *cls_list = nullptr;
    if (tr.n_tiny != tr.n_nodes && tr.n_small != tr.n_nodes && tr.n_big != tr.n_nodes) {
        // a mixed node list: single-key / empty nodes are emitted in bulk, each leaf class gets an index list
        RC_TRY(ps.alloc((size_t)tr.n_nodes + 1, &flags));
        RC_TRY(ps.alloc((size_t)scan_tmp_words(tr.n_nodes), &scan_tmp));
        RC_TRY(ps.alloc((size_t)tr.n_nodes, &cls_list));
    }
    prof_mark(ctx, "leaves");
    HIP_TRY(hipMemsetAsync(cursor, 0, 8, ctx->stream));
    HIP_TRY(launch_leaves(tr.nodes, tr.n_nodes, tr.n_tiny, tr.n_small, tr.n_big, tr.buf0, tr.buf1, cursor, seg_off, seg_cnt, ok, oc,
                          flags, scan_tmp, cls_list, ctx->stream, false));
    prof_mark(ctx, "end");
    HIP_TRY(hipMemcpyAsync(ctx->mailbox, cursor, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const u64 total_groups = ctx->mailbox[0];
    if (total_groups > cap) {
        set_err("leaves: %llu groups exceed the output capacity %llu", (unsigned long long)total_groups, (unsigned long long)cap);
        return DNAGPU_ERR_INTERNAL;
    }
    h->total = tr.n_keys;                   // rows counted (an owner filter keeps only this owner's rows)
    hist_adopt(ps, h, ok, oc, seg_off, seg_cnt, tr.n_nodes, total_groups, true, 0);
    return DNAGPU_OK;
}

// Decides which engine counts -- the records (any_order, see above), the dense table or the tree -- and pairs prof_begin /
// prof_end around it.
static int count_core(dnagpu_ctx *ctx, const dnagpu_dna *dna, u64 first, u64 n, int k, u64 *keys_in,
                      dnagpu_hist **out, int fixed_bits = 0, u64 fixed_prefix = 0, int owner = 0, int n_owners = 1,
                      bool any_order = false)
{
    if (n > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    HistPtr h = hist_new(n);
    if (!h)
        return DNAGPU_ERR_OOM;
    if (n == 0) {
        *out = h.release();
        return DNAGPU_OK;
    }
    const bool whole = dna && fixed_bits == 0 && n_owners == 1;      // (every row of a sequence range, no owner filter)
    const bool force_sk = (ctx->debug_flags & DNAGPU_DEBUG_FORCE_SUPERKMER) && k >= sk_min_k() && n >= 64;
    int rc = DNAGPU_SK_SKEWED;
    if (any_order && whole && (sk_is_default(n, k) || force_sk)) {
        prof_begin(ctx);
        rc = count_sk(ctx, SkRows{dna, first, n, nullptr, 0}, k, h.get(), n);
        prof_end(ctx);
    }
    if (rc == DNAGPU_SK_SKEWED) {                // (or: a bucket too heavy for the engine: the ordinary tree from scratch)
        prof_begin(ctx);
        rc = whole && dense_pays(n, k) ? count_dense(ctx, dna, first, n, k, h.get())
                                       : count_tree(ctx, dna, first, n, k, keys_in, h.get(), fixed_bits, fixed_prefix, owner, n_owners);
        prof_end(ctx);
    }
    RC_TRY(rc);
    *out = h.release();
    return DNAGPU_OK;
}

// the histogram a count hands out carries the k it was counted with (dnagpu_hist_merge compares them)
static int with_k(int rc, dnagpu_hist **out, int k)
{
    if (rc == DNAGPU_OK && out && *out)
        (*out)->k = k;
    return rc;
}

extern "C" int dnagpu_count_kmers(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, uint64_t first,
                                  uint64_t count, dnagpu_hist **out)
{
    return with_k(guarded([&]() -> int {
    if (!ctx || !dna || !out)
        return DNAGPU_ERR_BAD_ARG;
    RC_TRY(check_range(dna, k, first, count));
    HIP_TRY(hipSetDevice(ctx->device));
    return count_core(ctx, dna, first, count, k, nullptr, out);
    }), out, k);
}

extern "C" int dnagpu_count_kmers_unordered(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, uint64_t first,
                                            uint64_t count, dnagpu_hist **out)
{
    return with_k(guarded([&]() -> int {
    if (!ctx || !dna || !out)
        return DNAGPU_ERR_BAD_ARG;
    RC_TRY(check_range(dna, k, first, count));
    HIP_TRY(hipSetDevice(ctx->device));
    return count_core(ctx, dna, first, count, k, nullptr, out, 0, 0, 0, 1, true);
    }), out, k);
}

// ---- GROUP BY kmer, count(*) FROM a table of sequences, LATERAL generate_kmers(sequence, k) (test.sql:140-150)
// the rows of a table: every sequence's own generate_kmers rows (none for a sequence shorter than k); BAD_ARG unless the
// starts are ascending from 0 to the stream's length
static int table_rows_host(const dnagpu_dna *dna, const uint64_t *seq_starts, uint64_t n_seqs, int k, u64 *rows_out)
{
    u64 rows = 0;
    for (u64 i = 0; i < n_seqs; i++) {
        if (seq_starts[i + 1] < seq_starts[i])
            return DNAGPU_ERR_BAD_ARG;
        const u64 len = seq_starts[i + 1] - seq_starts[i];
        if (len >= (u64)k)
            rows += len - (u64)k + 1;
    }
    if (n_seqs && (seq_starts[0] != 0 || seq_starts[n_seqs] != dna->n_bases))
        return DNAGPU_ERR_BAD_ARG;
    if (n_seqs == 0 && dna->n_bases != 0)
        return DNAGPU_ERR_BAD_ARG;
    *rows_out = rows;
    return DNAGPU_OK;
}

// the count over a table whose marks are in device memory (the caller's PoolScope or the dna's own)
static int count_table(dnagpu_ctx *ctx, const dnagpu_dna *dna, const u32 *marks, u64 n_mark_words, u64 rows, int k, dnagpu_hist **out)
{
    PoolScope ps(ctx);
    hipStream_t st = ctx->stream;
    const u64 n_windows = dna->n_bases - (u64)k + 1;   // (rows > 0: some sequence has k bases)
    // ---- long k-mers of long tables: the super-k-mer engine, its level 0 blind to the rows across sequence starts
    const bool force_sk = (ctx->debug_flags & DNAGPU_DEBUG_FORCE_SUPERKMER) && k >= sk_min_k() && rows >= 64;
    if (sk_is_default(rows, k) || force_sk) {
        HistPtr h = hist_new(rows);
        if (!h)
            return DNAGPU_ERR_OOM;
        prof_begin(ctx);
        const int rc = count_sk(ctx, SkRows{dna, 0, n_windows, marks, n_mark_words}, k, h.get(), rows);
        prof_end(ctx);
        if (rc == DNAGPU_OK) {
            *out = h.release();
            return DNAGPU_OK;
        }
        if (rc != DNAGPU_SK_SKEWED)
            return rc;                             // (else: the keys below)
    }
    // ---- every other case: the keys of the table's rows, compacted, then the ordinary count over keys
    u64 *keys = nullptr;
    unsigned long long *cursor = nullptr;
    RC_TRY(ps.alloc((size_t)rows, &keys));
    RC_TRY(ps.alloc(1, &cursor));
    HIP_TRY(launch_batch_keys(dna->words, dna->n_words, marks, n_mark_words, n_windows, k, keys,
                              cursor, st));
    u64 got = 0;
    RC_TRY(read_back(ctx, &got, cursor, 8));
    if (got != rows) {
        set_err("table count: %llu rows kept, %llu expected", (unsigned long long)got, (unsigned long long)rows);
        return DNAGPU_ERR_INTERNAL;
    }
    return count_core(ctx, nullptr, 0, rows, k, keys, out);
}

extern "C" int dnagpu_count_kmers_batch(dnagpu_ctx *ctx, const dnagpu_dna *dna, const uint64_t *seq_starts, uint64_t n_seqs,
                                        int k, dnagpu_hist **out)
{
    return with_k(guarded([&]() -> int {
    if (!ctx || !dna || !out || (n_seqs && !seq_starts))
        return DNAGPU_ERR_BAD_ARG;
    if (k < 1 || k > 32)
        return DNAGPU_ERR_INVALID_K;               // dna.c:771-773, raised by the first row's generate_kmers call
    *out = nullptr;
    u64 rows = 0;
    RC_TRY(table_rows_host(dna, seq_starts, n_seqs, k, &rows));
    if (rows > 0xFFFFFFFFull || dna->n_bases > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0)
        return count_core(ctx, nullptr, 0, 0, k, nullptr, out);
    if (n_seqs == 1)                               // one sequence: the plain count
        return count_core(ctx, dna, 0, rows, k, nullptr, out, 0, 0, 0, 1, true);
    PoolScope ps(ctx);
    // ---- the marks: one bit per base, set where a sequence starts
    u64 n_mark_words = 0, *d_starts = nullptr;
    u32 *marks = nullptr;
    RC_TRY(starts_and_marks(ctx, ps, seq_starts, n_seqs, dna->n_bases, &d_starts, &marks, &n_mark_words));
    return count_table(ctx, dna, marks, n_mark_words, rows, k, out);
    }), out, k);
}

// The table's boundaries made resident: validated, uploaded, and the marks built ONCE; dnagpu_count_kmers_table then counts
// it for any k with nothing crossing the bus (at 10^7 reads the starts are 80 MB: 5.8 ms of a 14.4 ms call).
extern "C" int dnagpu_dna_set_sequences(dnagpu_ctx *ctx, dnagpu_dna *dna, const uint64_t *seq_starts, uint64_t n_seqs)
{
    return guarded([&]() -> int {
    if (!ctx || !dna || (n_seqs && !seq_starts))
        return DNAGPU_ERR_BAD_ARG;
    u64 rows1 = 0;
    RC_TRY(table_rows_host(dna, seq_starts, n_seqs, 1, &rows1));
    if (dna->n_bases > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    HIP_TRY(hipSetDevice(ctx->device));
    if (dna->seq_starts)
        pool_free(ctx, dna->seq_starts);
    if (dna->seq_marks)
        pool_free(ctx, dna->seq_marks);
    dna->seq_starts = nullptr;
    dna->seq_marks = nullptr;
    dna->n_seqs = dna->n_mark_words = 0;
    if (n_seqs == 0)
        return DNAGPU_OK;                          // (an empty table over an empty stream: nothing to keep)
    PoolScope ps(ctx);
    u64 n_mark_words = 0, *ds = nullptr;
    u32 *dm = nullptr;
    RC_TRY(starts_and_marks(ctx, ps, seq_starts, n_seqs, dna->n_bases, &ds, &dm, &n_mark_words));
    ps.release(ds);
    ps.release(dm);
    dna->seq_starts = ds;
    dna->seq_marks = dm;
    dna->n_seqs = n_seqs;
    dna->n_mark_words = n_mark_words;
    return DNAGPU_OK;
    });
}

extern "C" uint64_t dnagpu_dna_sequences(const dnagpu_dna *dna) { return dna ? dna->n_seqs : 0; }

extern "C" int dnagpu_count_kmers_table(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, dnagpu_hist **out)
{
    return with_k(guarded([&]() -> int {
    if (!ctx || !dna || !out)
        return DNAGPU_ERR_BAD_ARG;
    if (k < 1 || k > 32)
        return DNAGPU_ERR_INVALID_K;
    *out = nullptr;
    if (table_without_set(dna))
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    u64 rows = 0;
    if (dna->n_seqs) {
        PoolScope ps(ctx);
        u64 *d_rows = nullptr;
        RC_TRY(ps.alloc(1, &d_rows));
        HIP_TRY(launch_batch_rows(dna->seq_starts, dna->n_seqs, k, d_rows, ctx->stream));
        RC_TRY(read_back(ctx, &rows, d_rows, 8));
    }
    if (rows > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    if (rows == 0)
        return count_core(ctx, nullptr, 0, 0, k, nullptr, out);
    if (dna->n_seqs == 1)
        return count_core(ctx, dna, 0, rows, k, nullptr, out, 0, 0, 0, 1, true);
    return count_table(ctx, dna, dna->seq_marks, dna->n_mark_words, rows, k, out);
    }), out, k);
}

extern "C" int dnagpu_count_kmers_owned(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, uint64_t first,
                                        uint64_t count, int owner, int n_owners, dnagpu_hist **out)
{
    return with_k(guarded([&]() -> int {
    if (!ctx || !dna || !out || n_owners < 1 || owner < 0 || owner >= n_owners)
        return DNAGPU_ERR_BAD_ARG;
    RC_TRY(check_range(dna, k, first, count));
    HIP_TRY(hipSetDevice(ctx->device));
    return count_core(ctx, dna, first, count, k, nullptr, out, 0, 0, owner, n_owners);
    }), out, k);
}

extern "C" int dnagpu_count_keys(dnagpu_ctx *ctx, uint64_t *dev_keys, uint64_t n, int k, dnagpu_hist **out)
{
    return with_k(guarded([&]() -> int {
    if (!ctx || !out || (n && !dev_keys))
        return DNAGPU_ERR_BAD_ARG;
    if (k <= 0 || k > 32)
        return DNAGPU_ERR_INVALID_K;
    HIP_TRY(hipSetDevice(ctx->device));
    return count_core(ctx, nullptr, 0, n, k, dev_keys, out);
    }), out, k);
}

extern "C" int dnagpu_count_keys_in_range(dnagpu_ctx *ctx, uint64_t *dev_keys, uint64_t n, int k,
                                          uint64_t key_min, uint64_t key_max, dnagpu_hist **out)
{
    return with_k(guarded([&]() -> int {
    if (!ctx || !out || (n && !dev_keys) || key_min > key_max)
        return DNAGPU_ERR_BAD_ARG;
    if (k <= 0 || k > 32)
        return DNAGPU_ERR_INVALID_K;
    HIP_TRY(hipSetDevice(ctx->device));
    // number of leading bits (of the 2k key bits) that key_min and key_max share
    const int nbits = 2 * k;
    u64 diff = (key_min ^ key_max) & kmer_mask(k);
    int free_bits = 0;
    while (free_bits < nbits && (diff >> free_bits) != 0)
        free_bits++;
    const int fixed = nbits - free_bits;
    const u64 prefix = free_bits >= 64 ? 0 : ((key_min & kmer_mask(k)) >> free_bits) << free_bits;
    // a single possible key (fixed == 2k) still runs through the generic path: rem = 0 leaf
    return count_core(ctx, nullptr, 0, n, k, dev_keys, out, fixed, prefix);
    }), out, k);
}
