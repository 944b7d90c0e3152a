// take_host.hip -- dnagpu_dna_gather, dnagpu_dna_take and dnagpu_dna_sequence_starts of include/dnagpu.h: segments of a packed
// stream, or sequences of a resident table by id, gathered into a new resident table on the device (take_kernels.hip;
// DESIGN.md 4.16).  The argument rules, the one internal form of the two entry points, and the hand-over of the result.
#include "host_common.hpp"
#include "take_math.hpp"

using namespace dnagpu;

namespace {

// The two faces of the call.  ids != nullptr: take (segment i = sequence ids[i] of src's set); else gather (first / len).
// All three lists are host memory, or device memory when on_device.
struct TakeLists {
    const u64 *ids;
    const u64 *first, *len;
    const uint8_t *flip;              // may be null
    u64 n;
    int on_device;
};

int gather_core(dnagpu_ctx *ctx, const dnagpu_dna *src, const TakeLists &in, dnagpu_dna **out)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    const u64 n = in.n;
    std::unique_ptr<dnagpu_dna> h(new dnagpu_dna{nullptr, 0, 0, true});
    if (n == 0) {                                    // 0 bases, no set: what dnagpu_dna_upload makes of 0 bases
        RC_TRY(ps.alloc(1, &h->words));
        ps.release(h->words);
        *out = h.release();
        return DNAGPU_OK;
    }
    // ---- the segment list on the device, validated and summed in one pass; flag and total come back together
    prof_begin(ctx);
    prof_mark(ctx, "take_lists");
    const u64 *ids = nullptr, *first = nullptr, *len = nullptr;
    const uint8_t *flip = nullptr;
    RC_TRY(device_list(ctx, ps, in.ids, n, in.on_device, &ids));
    RC_TRY(device_list(ctx, ps, in.first, n, in.on_device, &first));
    RC_TRY(device_list(ctx, ps, in.len, n, in.on_device, &len));
    RC_TRY(device_list(ctx, ps, in.flip, n, in.on_device, &flip));
    u64 *seg_first = nullptr;
    u32 *len32 = nullptr;
    unsigned long long *res = nullptr;
    if (ids)
        RC_TRY(ps.alloc((size_t)n, &seg_first));
    RC_TRY(ps.alloc((size_t)n, &len32));
    RC_TRY(ps.alloc(2, &res));
    prof_mark(ctx, "take_segments");
    HIP_TRY(launch_take_segments(ids, src->seq_starts, src->n_seqs, first, len, src->n_bases, n, seg_first, len32, res, st));
    u64 got[2] = {0, 0};
    RC_TRY(read_back(ctx, got, res, sizeof got));    // (waits for the stream: the caller's host lists have been read)
    if (got[1]) {
        set_err(ids ? "take: a sequence id is not below the table's %llu sequences"
                    : "gather: a segment leaves the stream of %llu bases",
                (unsigned long long)(ids ? src->n_seqs : src->n_bases));
        return DNAGPU_ERR_BAD_ARG;
    }
    const u64 total = got[0];
    if (total > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;                 // (dnagpu_dna_set_sequences' limit for a resident table)

    // ---- the result: starts, marks, and the stream; nothing of it is assumed zero
    const u64 nw = words_for(total), n_mark_words = total / 32 + 3;
    u32 *scan_tmp = nullptr;
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n), &scan_tmp));
    RC_TRY(ps.alloc((size_t)n + 1, &h->seq_starts));
    RC_TRY(ps.alloc((size_t)n_mark_words, &h->seq_marks));
    RC_TRY(ps.alloc((size_t)std::max<u64>(nw, 1), &h->words));
    prof_mark(ctx, "take_starts");
    HIP_TRY(launch_scan_u32(len32, len32, n, scan_tmp, nullptr, st));
    HIP_TRY(launch_take_starts(len32, n, total, h->seq_starts, st));
    prof_mark(ctx, "take_marks");
    HIP_TRY(launch_batch_marks(h->seq_starts, n, h->seq_marks, n_mark_words, st));
    prof_mark(ctx, "take_copy");
    HIP_TRY(launch_take_copy(src->words, ids ? seg_first : first, flip, h->seq_starts, n, total, h->words, st));
    prof_mark(ctx, "end");
    HIP_TRY(hipStreamSynchronize(st));
    prof_end(ctx);
    ps.release(h->seq_starts);
    ps.release(h->seq_marks);
    ps.release(h->words);
    h->n_words = nw;
    h->n_bases = total;
    h->n_seqs = n;
    h->n_mark_words = n_mark_words;
    *out = h.release();
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
    if (table->n_seqs == 0 && table->n_bases != 0)
        return DNAGPU_ERR_BAD_ARG;                   // (no dnagpu_dna_set_sequences before)
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
