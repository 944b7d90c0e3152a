// take_host.hip -- dnagpu_dna_gather, dnagpu_dna_take and dnagpu_dna_sequence_starts of include/dnagpu.h: segments of a packed
// stream, or sequences of a resident table by id, gathered into a new resident table on the device (take_kernels.hip;
// DESIGN.md 4.16).  The argument rules, the one internal form of the two entry points, and the hand-over of the result.
#include "host_common.hpp"
#include "take_math.hpp"

using namespace dnagpu;

namespace {

int gather_core(dnagpu_ctx *ctx, const dnagpu_dna *src, const TakeLists &in, dnagpu_dna **out)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    NewTable t(ctx);
    if (in.n == 0)
        return t.empty(out);
    prof_begin(ctx);
    TakePlan plan = {};
    RC_TRY(take_plan(ctx, t.ps, in, src->seq_starts, src->n_seqs, src->n_bases, "take_lists", &plan));
    RC_TRY(t.alloc(in.n, plan.total, plan.starts));  // (the plan's starts are the result's)
    RC_TRY(plan.queue_starts(ctx));
    prof_mark(ctx, "take_marks");
    RC_TRY(t.queue_marks(st));
    prof_mark(ctx, "take_copy");
    HIP_TRY(launch_take_copy(src->words, plan.seg_first, plan.flip, plan.starts, in.n, plan.total, t.h->words, st));
    prof_mark(ctx, "end");
    HIP_TRY(hipStreamSynchronize(st));
    prof_end(ctx);
    t.hand_over(out);
    return DNAGPU_OK;                                // (the lists' copies and the scratch go back to the pool here)
}

}  // namespace

extern "C" int dnagpu_dna_gather(dnagpu_ctx *ctx, const dnagpu_dna *src, const uint64_t *seg_first, const uint64_t *seg_len,
                                 const uint8_t *seg_flip, uint64_t n_segs, int on_device, dnagpu_dna **out)
{
    return guarded([&]() -> int {
    if (!ctx || !src || !out || (n_segs && (!seg_first || !seg_len)))
        return DNAGPU_ERR_BAD_ARG;
    if (n_segs > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    const TakeLists in = {nullptr, seg_first, seg_len, seg_flip, n_segs, on_device};
    return gather_core(ctx, src, in, out);
    });
}

extern "C" int dnagpu_dna_take(dnagpu_ctx *ctx, const dnagpu_dna *table, const uint64_t *seq_ids, const uint8_t *seq_flip,
                               uint64_t n_ids, int on_device, dnagpu_dna **out)
{
    return guarded([&]() -> int {
    if (!ctx || !table || !out || (n_ids && !seq_ids))
        return DNAGPU_ERR_BAD_ARG;
    if (table_without_set(table))
        return DNAGPU_ERR_BAD_ARG;
    if (n_ids > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    if (n_ids && table->n_seqs == 0) {               // an empty stream without a set: a table of no sequence
        set_err("take: a sequence id is not below the table's 0 sequences");
        return DNAGPU_ERR_BAD_ARG;
    }
    const TakeLists in = {seq_ids, nullptr, nullptr, seq_flip, n_ids, on_device};
    return gather_core(ctx, table, in, out);
    });
}

extern "C" int dnagpu_dna_sequence_starts(dnagpu_ctx *ctx, const dnagpu_dna *dna, uint64_t first, uint64_t count,
                                          uint64_t *out_starts, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !dna || (count && !out_starts))
        return DNAGPU_ERR_BAD_ARG;
    const u64 entries = dna->n_seqs ? dna->n_seqs + 1 : 0;
    if (first > entries || count > entries - first)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(out_starts, dna->seq_starts + first, (size_t)count * 8,
                           out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}
