// join_host.hip -- dnagpu_acc_join of include/dnagpu.h: the hash join of two accumulators (join_kernels.hip; DESIGN.md
// 4.13).  The argument rules, the empty sides, the choice between the two paths, and the hand-out of the rows.
#include "host_common.hpp"

using namespace dnagpu;

static_assert(DNAGPU_JOIN_INNER == JOIN_KIND_INNER && DNAGPU_JOIN_ANTI == JOIN_KIND_ANTI && DNAGPU_JOIN_LEFT == JOIN_KIND_LEFT,
              "the kernels' kinds are the header's");
static_assert(sizeof(dnagpu_join_stats) == JOIN_RES_WORDS * 8, "dnagpu_join_stats is the kernels' result words");

namespace {

// A result that goes to host arrays is staged in pool buffers of at most this many rows each: left's partitions are joined in
// chunks of JOIN_CHUNK_PARTS (a partition gives at most ACC_SLOTS rows), each chunk copied out before the next is queued.
constexpr u64 JOIN_CHUNK_PARTS = 256;
constexpr u64 JOIN_CHUNK_ROWS = JOIN_CHUNK_PARTS * ACC_SLOTS;

// The path, from the partition bits alone (s: left, t: right; t == 0: right holds no table).  The partition path moves
// 2 * 2^max(s, t) * 64 KB whatever the sizes; the direct path moves left once plus one or two 64-byte sectors per group at a
// random-access rate.  The byte estimate put the crossover at t - s >= 4; measured (tools/join_probe.py,
// profiles/join_probe.log) the partition path wins up to t - s = 1 (0.33 against 0.38 ms at s = 12) and
// the direct path from t - s = 2 on (0.42 against 0.56 ms at s = 12; 0.09 against 0.92 ms at t - s = 6).
bool join_takes_direct(int s, int t)
{
    return t == 0 || t - s >= 2;
}

bool has_table(const dnagpu_acc *a)
{
    return a->distinct != 0 && a->t.pbits != 0 && a->t.table && a->t.occ;
}

int join_core(dnagpu_ctx *ctx, const dnagpu_acc *left, const dnagpu_acc *right, int kind, u64 *out_keys, u64 *out_left,
              u64 *out_right, u64 cap, u64 *n_out, dnagpu_join_stats *stats, int out_on_device)
{
    *n_out = 0;
    if (stats)
        *stats = dnagpu_join_stats{};
    if (!has_table(left))
        return DNAGPU_OK;                            // no left group, no row
    const bool right_has = has_table(right);
    if (!right_has && kind == DNAGPU_JOIN_INNER)
        return DNAGPU_OK;                            // nothing can match
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    unsigned long long *res = nullptr;
    RC_TRY(ps.alloc(JOIN_RES_WORDS, &res));
    HIP_TRY(hipMemsetAsync(res, 0, JOIN_RES_WORDS * 8, st));

    JoinArgs a{};
    a.l_table = left->t.table;
    a.l_occ = left->t.occ;
    a.s = left->t.pbits;
    if (right_has) {
        a.r_table = right->t.table;
        a.r_occ = right->t.occ;
        a.t = right->t.pbits;
    }
    a.kind = kind;
    a.res = res;
    bool direct = join_takes_direct(a.s, a.t);
    if (ctx->debug_flags & DNAGPU_DEBUG_JOIN_PARTITION)
        direct = false;
    else if (ctx->debug_flags & DNAGPU_DEBUG_JOIN_DIRECT)
        direct = true;
    auto launch = [&](u64 p_lo, u64 n_parts) {
        return direct ? launch_join_direct(a, p_lo, n_parts, st) : launch_join_partition(a, p_lo, n_parts, st);
    };
    const u64 P = (u64)1 << a.s;
    u64 r[JOIN_RES_WORDS] = {0, 0, 0, 0, 0, 0};
    const bool want_rows = cap != 0 && (out_keys || out_left || out_right);
    if (!want_rows || out_on_device) {               // one launch: statistics only, or straight into the caller's device arrays
        if (want_rows) {
            a.out_keys = out_keys;
            a.out_left = out_left;
            a.out_right = out_right;
            a.cap = cap;
        }
        HIP_TRY(launch(0, P));
        RC_TRY(read_back(ctx, r, res, sizeof r));    // (waits for the stream: device outputs are complete)
    } else {                                         // host outputs: staged, chunk by chunk (no more rows than left has groups)
        cap = std::min(cap, left->distinct);
        const size_t stage = (size_t)std::min(cap, JOIN_CHUNK_ROWS);
        if (out_keys)
            RC_TRY(ps.alloc(stage, &a.out_keys));
        if (out_left)
            RC_TRY(ps.alloc(stage, &a.out_left));
        if (out_right)
            RC_TRY(ps.alloc(stage, &a.out_right));
        a.cap = cap;
        u64 done = 0;                                // rows of the chunks before this one
        for (u64 p_lo = 0; p_lo < P;) {
            // (once cap rows are out, the rest only counts: one launch)
            const u64 n_parts = done >= cap ? P - p_lo : std::min(JOIN_CHUNK_PARTS, P - p_lo);
            a.out_base = done;
            HIP_TRY(launch(p_lo, n_parts));
            RC_TRY(read_back(ctx, r, res, sizeof r));
            const u64 hi = std::min(r[0], cap);
            if (hi > done) {
                const size_t bytes = (size_t)(hi - done) * 8;
                if (out_keys)
                    HIP_TRY(hipMemcpyAsync(out_keys + done, a.out_keys, bytes, hipMemcpyDeviceToHost, st));
                if (out_left)
                    HIP_TRY(hipMemcpyAsync(out_left + done, a.out_left, bytes, hipMemcpyDeviceToHost, st));
                if (out_right)
                    HIP_TRY(hipMemcpyAsync(out_right + done, a.out_right, bytes, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
            }
            done = r[0];
            p_lo += n_parts;
        }
    }
    *n_out = r[0];
    if (stats) {
        stats->rows = r[0];
        stats->sum_left = r[1];
        stats->sum_right = r[2];
        stats->sum_min = r[3];
        stats->checksum_left = r[4];
        stats->checksum_right = r[5];
    }
    return DNAGPU_OK;
}

}  // namespace

extern "C" int dnagpu_acc_join(dnagpu_ctx *ctx, const dnagpu_acc *left, const dnagpu_acc *right, int kind, uint64_t *out_keys,
                               uint64_t *out_left, uint64_t *out_right, uint64_t cap, uint64_t *n_out, dnagpu_join_stats *stats,
                               int out_on_device)
{
    return guarded([&]() -> int {
    if (kind < DNAGPU_JOIN_INNER || kind > DNAGPU_JOIN_LEFT)
        return DNAGPU_ERR_BAD_ARG;                   // (the range before the missing object)
    if (!ctx || !left || !right || !n_out)
        return DNAGPU_ERR_BAD_ARG;
    if (left->k != right->k)
        return DNAGPU_ERR_BAD_ARG;                   // (keys of different k: equal values would be different k-mers)
    return join_core(ctx, left, right, kind, out_keys, out_left, out_right, cap, n_out, stats, out_on_device);
    });
}

extern "C" uint64_t dnagpu_acc_partitions(const dnagpu_acc *acc)
{
    return acc && acc->t.pbits ? (uint64_t)1 << acc->t.pbits : 0;
}
