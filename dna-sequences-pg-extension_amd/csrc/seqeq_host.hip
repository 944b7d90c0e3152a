// seqeq_host.hip -- equal sequences of include/dnagpu.h: dnagpu_dna_equals, dnagpu_table_classes with the dnagpu_seq_classes
// object (read, select, members), dnagpu_table_match and dnagpu_seq_equal_geometry (seqeq_kernels.hip).  The
// argument rules and one function per stage: the fingerprint sweep, the sort (the index's LSD passes), the verify rounds,
// the class sizes, the match.
#include "host_common.hpp"
#include "seqeq_math.hpp"

using namespace dnagpu;

namespace {

SeqTable table_of(const dnagpu_dna *d, u64 seq_first) { return SeqTable{d->words, d->n_words, d->seq_starts + seq_first}; }

// Stage 1: fp[0 .. n) = the fingerprints of the n >= 1 sequences of t; ids (may be null) = 0 .. n - 1.  items (n + 1 words)
// and scan_tmp (scan_tmp_words(n)) are the caller's scratch.  *n_items = the items of the long sequences.  Waits.
int fingerprints(dnagpu_ctx *ctx, const SeqTable &t, u64 n, u64 *fp, u32 *ids, u32 *items, u32 *scan_tmp, u32 *n_items)
{
    hipStream_t st = ctx->stream;
    HIP_TRY(launch_seqeq_fp_short(t, n, fp, ids, items, st));
    RC_TRY(scan_total(ctx, items, n, scan_tmp, n_items));
    HIP_TRY(launch_seqeq_fp_long(t, n, items, *n_items, fp, st));
    if (ctx->debug_flags & DNAGPU_DEBUG_WEAK_FINGERPRINT)
        HIP_TRY(launch_seqeq_weaken(fp, n, st));
    return DNAGPU_OK;
}

// (fingerprint, id) lists: pair[0] and pair[1] are the ping-pong of stage 2, the stable LSD sort by all eight digits of fp
// (lsd_sort_pairs)
struct Pair {
    u64 *fp;
    u32 *id;
};

// the scratch of the verify rounds, n entries each
struct RoundBufs {
    u32 *head, *run, *slot, *hidx, *eq, *pre, *items, *scan_tmp, *total;
};

// Stage 3, one round over list[0 .. m): the equal entries are settled (rep, copies of the heads), the others move to `next`.
// *left = how many moved.  Waits (one 4-byte read-back, two when the table has long sequences).
int verify_round(dnagpu_ctx *ctx, const SeqTable &t, const Pair &list, u64 m, bool has_long, const RoundBufs &b, u32 *rep,
                 u32 *copies, const Pair &next, u64 *left)
{
    hipStream_t st = ctx->stream;
    HIP_TRY(launch_seqeq_head_flags(list.fp, m, b.head, st));
    HIP_TRY(launch_scan_u32(b.head, b.run, m, b.scan_tmp, nullptr, st));
    HIP_TRY(launch_seqeq_head_slots(b.head, b.run, m, b.slot, st));
    HIP_TRY(launch_seqeq_verify(t, list.id, m, b.head, b.run, b.slot, b.hidx, b.eq, b.items, st));
    if (has_long) {
        u32 n_items = 0;
        RC_TRY(scan_total(ctx, b.items, m, b.scan_tmp, &n_items));   // (items has a word behind every list: n + 1)
        HIP_TRY(launch_seqeq_pair_items(t, list.id, t, list.id, b.hidx, m, b.items, n_items, b.eq, st));
    }
    HIP_TRY(launch_scan_u32(b.eq, b.pre, m, b.scan_tmp, b.total, st));
    u32 settled = 0;
    RC_TRY(read_back(ctx, &settled, b.total, 4));
    *left = m - settled;
    HIP_TRY(launch_seqeq_apply(list.fp, list.id, m, b.hidx, b.eq, b.pre, rep, copies, next.fp, next.id, *left, st));
    return DNAGPU_OK;
}

int classes_build(dnagpu_ctx *ctx, const dnagpu_dna *table, dnagpu_seq_classes *c)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    const u64 n = c->n;
    const SeqTable t = table_of(table, 0);
    Pair pair[3] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    for (int i = 0; i < 2; i++) {
        RC_TRY(ps.alloc((size_t)n, &pair[i].fp));
        RC_TRY(ps.alloc((size_t)n, &pair[i].id));
    }
    u32 *rep = nullptr, *copies = nullptr;
    RC_TRY(ps.alloc((size_t)n, &rep));
    RC_TRY(ps.alloc((size_t)n, &copies));
    RoundBufs b{};
    RC_TRY(ps.alloc((size_t)n, &b.head));
    RC_TRY(ps.alloc((size_t)n, &b.run));
    RC_TRY(ps.alloc((size_t)n, &b.slot));
    RC_TRY(ps.alloc((size_t)n, &b.hidx));
    RC_TRY(ps.alloc((size_t)n, &b.eq));
    RC_TRY(ps.alloc((size_t)n, &b.pre));
    RC_TRY(ps.alloc((size_t)n + 1, &b.items));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n), &b.scan_tmp));
    RC_TRY(ps.alloc((size_t)2, &b.total));
    u64 *distinct_dev = nullptr;
    RC_TRY(ps.alloc((size_t)1, &distinct_dev));

    prof_begin(ctx);
    prof_mark(ctx, "seqeq_fingerprint");
    u32 n_items = 0;
    RC_TRY(fingerprints(ctx, t, n, pair[0].fp, pair[0].id, b.items, b.scan_tmp, &n_items));
    prof_mark(ctx, "seqeq_sort");
    int kept = 0;
    u64 *const fps[2] = {pair[0].fp, pair[1].fp};
    u32 *const ids[2] = {pair[0].id, pair[1].id};
    RC_TRY(lsd_sort_pairs(ctx, IndexSortSrc{nullptr, fps[0], ids[0], 32, 0}, n, 8, fps, ids, nullptr, &kept));

    // the rounds: the sorted list stays (the match walks it); the leftovers alternate between the other pair and a third
    prof_mark(ctx, "seqeq_verify");
    int cur = kept, spare = 1 - kept;
    u64 left = n;
    u32 rounds = 0;
    while (left > 0) {
        const u64 m = left;
        RC_TRY(verify_round(ctx, t, pair[cur], m, n_items != 0, b, rep, copies, pair[spare], &left));
        rounds++;
        const int was = cur;
        cur = spare;
        spare = was == kept ? 2 : was;
        if (left > 0 && !pair[spare].fp) {
            RC_TRY(ps.alloc((size_t)left, &pair[2].fp));   // (later lists are no longer than this one)
            RC_TRY(ps.alloc((size_t)left, &pair[2].id));
        }
    }
    prof_mark(ctx, "seqeq_copies");
    HIP_TRY(hipMemsetAsync(distinct_dev, 0, 8, st));
    HIP_TRY(launch_seqeq_spread(rep, copies, n, distinct_dev, st));
    prof_mark(ctx, "end");
    u64 distinct = 0;
    RC_TRY(read_back(ctx, &distinct, distinct_dev, 8));    // (waits for the stream: the object is complete)
    prof_end(ctx);
    for (void *p : {(void *)rep, (void *)copies, (void *)pair[kept].fp, (void *)pair[kept].id})
        ps.release(p);
    c->rep = rep;
    c->copies = copies;
    c->sfp = pair[kept].fp;
    c->sid = pair[kept].id;
    c->distinct = distinct;
    c->rounds = rounds;
    return DNAGPU_OK;                                      // (the scratch arrays go back to the pool here)
}

// the two selects: count, scan, write
int select_run(dnagpu_ctx *ctx, const dnagpu_seq_classes *c, const SeqSelect &q, u64 *out_seq, u64 *out_copies, u64 cap, u64 *n_out,
               int out_on_device)
{
    *n_out = 0;
    if (c->n == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    u32 *tiles = nullptr, total = 0;
    RC_TRY(select_tiles(ctx, ps, seqeq_select_tiles(c->n),
                        [&](u32 *t) { return launch_seqeq_select_count(c->rep, c->copies, c->n, q, t, st); }, &tiles, &total));
    *n_out = total;
    const u64 n_write = std::min<u64>(total, cap);
    if (n_write == 0 || (!out_seq && !out_copies))
        return DNAGPU_OK;
    OutCols<2> o;
    RC_TRY(o.init(ctx, ps, {out_seq, out_copies}, n_write, out_on_device));
    HIP_TRY(launch_seqeq_select_write(c->rep, c->copies, c->n, q, tiles, o.dev(0), o.dev(1), n_write, st));
    return o.finish();
}

// Stage 5: the np >= 1 sequences from seq_first of probe against the built side
int match_run(dnagpu_ctx *ctx, const dnagpu_seq_classes *c, const dnagpu_dna *probe, u64 seq_first, u64 np, u64 *out_match,
              u64 *out_copies, u64 *n_matched, int out_on_device)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    // every buffer first: an error leaves the outputs untouched
    u64 *dev[2] = {out_match, out_copies}, *outs[2] = {out_match, out_copies};
    if (!out_on_device)
        for (int i = 0; i < 2; i++)
            if (outs[i])
                RC_TRY(ps.alloc((size_t)np, &dev[i]));
    u64 *counter = nullptr;
    RC_TRY(ps.alloc((size_t)1, &counter));
    u32 *match32 = nullptr;
    if (c->n != 0) {
        u64 *pfp = nullptr;
        u32 *items = nullptr, *off = nullptr, *scan_tmp = nullptr, *cur = nullptr, *flag = nullptr;
        RC_TRY(ps.alloc((size_t)np, &pfp));
        RC_TRY(ps.alloc((size_t)np + 1, &items));
        RC_TRY(ps.alloc((size_t)np + 1, &off));
        RC_TRY(ps.alloc((size_t)scan_tmp_words(np), &scan_tmp));
        RC_TRY(ps.alloc((size_t)np, &cur));
        RC_TRY(ps.alloc((size_t)np, &flag));
        RC_TRY(ps.alloc((size_t)np, &match32));
        const SeqTable pt = table_of(probe, seq_first), bt = table_of(c->table, 0);
        u32 n_items = 0;
        RC_TRY(fingerprints(ctx, pt, np, pfp, nullptr, items, scan_tmp, &n_items));
        const bool has_long = n_items != 0;
        HIP_TRY(launch_seqeq_match_walk(pt, np, pfp, bt, c->sfp, c->sid, c->n, c->rep, 1, cur, flag, items, match32, st));
        while (has_long) {                                 // probes parked on a long candidate: items, then the walk goes on
            HIP_TRY(launch_scan_u32(items, off, np, scan_tmp, off + np, st));   // (items stays: it marks the parked probes)
            RC_TRY(read_back(ctx, &n_items, off + np, 4));
            if (n_items == 0)
                break;
            HIP_TRY(launch_seqeq_pair_items(pt, nullptr, bt, c->sid, cur, np, off, n_items, flag, st));
            HIP_TRY(launch_seqeq_match_walk(pt, np, pfp, bt, c->sfp, c->sid, c->n, c->rep, 0, cur, flag, items, match32, st));
        }
    }
    HIP_TRY(hipMemsetAsync(counter, 0, 8, st));
    HIP_TRY(launch_seqeq_match_out(match32, c->copies, np, dev[0], dev[1], counter, st));
    if (!out_on_device)
        for (int i = 0; i < 2; i++)
            if (outs[i])
                HIP_TRY(hipMemcpyAsync(outs[i], dev[i], (size_t)np * 8, hipMemcpyDeviceToHost, st));
    u64 matched = 0;
    RC_TRY(read_back(ctx, &matched, counter, 8));          // (waits for the stream)
    if (n_matched)
        *n_matched = matched;
    return DNAGPU_OK;
}

}  // namespace

extern "C" int dnagpu_seq_equal_geometry(uint64_t *wave_bases, uint64_t *tile_bases)
{
    if (wave_bases)
        *wave_bases = SEQEQ_WAVE_BASES;
    if (tile_bases)
        *tile_bases = SEQEQ_TILE_BASES;
    return DNAGPU_OK;
}

extern "C" int dnagpu_dna_equals(dnagpu_ctx *ctx, const dnagpu_dna *a, const dnagpu_dna *b, int *equal)
{
    return guarded([&]() -> int {
    if (!ctx || !a || !b || !equal)
        return DNAGPU_ERR_BAD_ARG;
    if (a->n_bases != b->n_bases) {
        *equal = 0;
        return DNAGPU_OK;
    }
    if (a == b || a->n_bases == 0) {
        *equal = 1;
        return DNAGPU_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    u32 *flag = nullptr;
    RC_TRY(ps.alloc((size_t)2, &flag));
    HIP_TRY(hipMemsetAsync(flag, 1, 4, ctx->stream));
    HIP_TRY(launch_seqeq_whole(a->words, a->n_words, b->words, b->n_words, a->n_bases, flag, ctx->stream));
    u32 f = 0;
    RC_TRY(read_back(ctx, &f, flag, 4));
    *equal = f != 0;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_table_classes(dnagpu_ctx *ctx, const dnagpu_dna *table, dnagpu_seq_classes **out)
{
    return guarded([&]() -> int {
    if (!ctx || !table || !out)
        return DNAGPU_ERR_BAD_ARG;
    if (table_without_set(table))
        return DNAGPU_ERR_BAD_ARG;
    if (table->n_seqs > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;                       // (32-bit ids, and all-ones is "no match")
    std::unique_ptr<dnagpu_seq_classes> c(new dnagpu_seq_classes());
    c->table = table;
    c->n = table->n_seqs;
    if (c->n != 0)
        RC_TRY(classes_build(ctx, table, c.get()));
    *out = c.release();
    return DNAGPU_OK;
    });
}

extern "C" uint64_t dnagpu_seq_classes_sequences(const dnagpu_seq_classes *c) { return c ? c->n : 0; }
extern "C" uint64_t dnagpu_seq_classes_distinct(const dnagpu_seq_classes *c) { return c ? c->distinct : 0; }
extern "C" uint32_t dnagpu_seq_classes_rounds(const dnagpu_seq_classes *c) { return c ? c->rounds : 0; }

extern "C" int dnagpu_seq_classes_read(dnagpu_ctx *ctx, const dnagpu_seq_classes *c, uint64_t first, uint64_t count,
                                       uint64_t *out_rep, uint64_t *out_copies, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !c)
        return DNAGPU_ERR_BAD_ARG;
    if (first > c->n || count > c->n - first)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0 || (!out_rep && !out_copies))
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    RC_TRY(widen_out(ctx, ps, c->rep + first, count, out_rep, out_on_device));
    RC_TRY(widen_out(ctx, ps, c->copies + first, count, out_copies, out_on_device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_seq_classes_select(dnagpu_ctx *ctx, const dnagpu_seq_classes *c, uint64_t min_copies, uint64_t max_copies,
                                         uint64_t *out_seq, uint64_t *out_copies, uint64_t cap, uint64_t *n_out, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !c || !n_out)
        return DNAGPU_ERR_BAD_ARG;
    const SeqSelect q = {0, 0, min_copies ? min_copies : 1, max_copies};
    return select_run(ctx, c, q, out_seq, out_copies, cap, n_out, out_on_device);
    });
}

extern "C" int dnagpu_seq_classes_members(dnagpu_ctx *ctx, const dnagpu_seq_classes *c, uint64_t seq, uint64_t *out_seq,
                                          uint64_t cap, uint64_t *n_out, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !c || !n_out)
        return DNAGPU_ERR_BAD_ARG;
    if (seq >= c->n)
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    u32 target = 0;
    RC_TRY(read_back(ctx, &target, c->rep + seq, 4));      // (the class is named by its representative)
    const SeqSelect q = {1, target, 0, 0};
    return select_run(ctx, c, q, out_seq, nullptr, cap, n_out, out_on_device);
    });
}

extern "C" int dnagpu_table_match(dnagpu_ctx *ctx, const dnagpu_seq_classes *build, const dnagpu_dna *probe, uint64_t seq_first,
                                  uint64_t seq_count, uint64_t *out_match, uint64_t *out_copies, uint64_t *n_matched,
                                  int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !build || !probe)
        return DNAGPU_ERR_BAD_ARG;
    if (seq_first > probe->n_seqs || seq_count > probe->n_seqs - seq_first)
        return DNAGPU_ERR_BAD_ARG;
    if (seq_count > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;                       // (part of the window rule, as in dnagpu_table_profile)
    if (table_without_set(probe))
        return DNAGPU_ERR_BAD_ARG;
    if (seq_count == 0) {
        if (n_matched)
            *n_matched = 0;
        return DNAGPU_OK;
    }
    if (!out_match && !out_copies && !n_matched)
        return DNAGPU_ERR_BAD_ARG;
    return match_run(ctx, build, probe, seq_first, seq_count, out_match, out_copies, n_matched, out_on_device);
    });
}

extern "C" void dnagpu_seq_classes_free(dnagpu_ctx *ctx, dnagpu_seq_classes *c)
{
    if (!c)
        return;
    if (ctx) {
        pool_free(ctx, c->rep);
        pool_free(ctx, c->copies);
        pool_free(ctx, c->sfp);
        pool_free(ctx, c->sid);
    }
    delete c;
}
