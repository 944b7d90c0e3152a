// table_steps.hip -- the host-side steps that the calls which make a resident table, or a column beside one, drive the same
// way (declared in host_common.hpp, "table_steps.hip"): the hand-over of a new table, the starts and marks of a caller's
// boundaries, the segment plan of take / gather, the FASTA tile state and the input-error report of the text loaders.  No
// kernel of its own.
#include "host_common.hpp"
#include "text_math.hpp"

namespace dnagpu {

int NewTable::empty(dnagpu_dna **out)
{
    h.reset(new dnagpu_dna{nullptr, 0, 0, true});
    RC_TRY(ps.alloc(1, &h->words));
    ps.release(h->words);
    *out = h.release();
    return DNAGPU_OK;
}

int NewTable::alloc(u64 n_seqs, u64 n_bases, u64 *starts, u64 *words)
{
    h.reset(new dnagpu_dna{words, words_for(n_bases), n_bases, true});
    h->seq_starts = starts;
    h->n_seqs = n_seqs;
    h->n_mark_words = table_mark_words(n_bases);
    if (!starts)
        RC_TRY(ps.alloc((size_t)n_seqs + 1, &h->seq_starts));
    RC_TRY(ps.alloc((size_t)h->n_mark_words, &h->seq_marks));
    if (!words)
        RC_TRY(ps.alloc((size_t)std::max<u64>(h->n_words, 1), &h->words));
    return DNAGPU_OK;
}

int NewTable::queue_marks(hipStream_t st)
{
    HIP_TRY(launch_batch_marks(h->seq_starts, h->n_seqs, h->seq_marks, h->n_mark_words, st));
    return DNAGPU_OK;
}

void NewTable::hand_over(dnagpu_dna **out)
{
    ps.release(h->seq_starts);
    ps.release(h->seq_marks);
    ps.release(h->words);
    *out = h.release();
}

int starts_and_marks(dnagpu_ctx *ctx, PoolScope &ps, const u64 *host_starts, u64 n_seqs, u64 n_bases, u64 **starts, u32 **marks,
                     u64 *n_mark_words)
{
    *n_mark_words = table_mark_words(n_bases);
    RC_TRY(ps.alloc((size_t)n_seqs + 1, starts));
    RC_TRY(ps.alloc((size_t)*n_mark_words, marks));
    HIP_TRY(hipMemcpyAsync(*starts, host_starts, (size_t)(n_seqs + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_batch_marks(*starts, n_seqs, *marks, *n_mark_words, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
}

int take_plan(dnagpu_ctx *ctx, PoolScope &ps, const TakeLists &in, const u64 *seq_starts, u64 n_seqs, u64 stream_bases,
              const char *lists_mark, TakePlan *plan)
{
    hipStream_t st = ctx->stream;
    const u64 n = in.n;
    // ---- the segment list on the device, validated and summed in one pass; flag and total come back together
    prof_mark(ctx, lists_mark);
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
    HIP_TRY(launch_take_segments(ids, seq_starts, n_seqs, first, len, stream_bases, n, seg_first, len32, res, st));
    u64 got[2] = {0, 0};
    RC_TRY(read_back(ctx, got, res, sizeof got));    // (waits for the stream: the caller's host lists have been read)
    if (got[1]) {
        set_err(ids ? "take: a sequence id is not below the table's %llu sequences"
                    : "gather: a segment leaves the stream of %llu bases",
                (unsigned long long)(ids ? n_seqs : stream_bases));
        return DNAGPU_ERR_BAD_ARG;
    }
    if (got[0] > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;                 // (dnagpu_dna_set_sequences' limit for a resident table)
    u32 *scan_tmp = nullptr;
    u64 *starts = nullptr;
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n), &scan_tmp));
    RC_TRY(ps.alloc((size_t)n + 1, &starts));
    *plan = TakePlan{ids ? seg_first : first, flip, starts, got[0], len32, scan_tmp, n};
    return DNAGPU_OK;
}

int TakePlan::queue_starts(dnagpu_ctx *ctx) const
{
    prof_mark(ctx, "take_starts");
    HIP_TRY(launch_scan_u32(len32, len32, n, scan_tmp, nullptr, ctx->stream));
    HIP_TRY(launch_take_starts(len32, n, total, starts, ctx->stream));
    return DNAGPU_OK;
}

int FastaTiles::before_sweep(dnagpu_ctx *ctx, PoolScope &ps)
{
    const u32 nt = sw.n_tiles;
    u32 *last_start = nullptr, *in_state = nullptr, *header_before = nullptr;
    RC_TRY(ps.alloc((size_t)nt, &last_start));
    RC_TRY(ps.alloc((size_t)nt, &last_header));
    RC_TRY(ps.alloc((size_t)nt, &in_state));
    RC_TRY(ps.alloc((size_t)nt, &header_before));
    RC_TRY(ps.alloc((size_t)nt, &sw.last_seq));
    RC_TRY(ps.alloc((size_t)nt, &sw.first_header));
    RC_TRY(ps.alloc((size_t)nt, &sw.seq_before));
    RC_TRY(ps.alloc((size_t)nt, &seq_before_t));
    prof_mark(ctx, "text_heads");
    HIP_TRY(launch_text_heads(sw.text, sw.lim, nt, last_start, last_header, ctx->stream));
    HIP_TRY(launch_text_max_scan(last_start, in_state, nt, ctx->stream));
    HIP_TRY(launch_text_max_scan(last_header, header_before, nt, ctx->stream));
    sw.in_state = in_state;
    sw.header_before = header_before;
    return DNAGPU_OK;
}

int FastaTiles::after_sweep(hipStream_t st) const
{
    HIP_TRY(launch_text_max_scan(sw.last_seq, seq_before_t, sw.n_tiles, st));
    HIP_TRY(launch_text_finish(sw, last_header, seq_before_t, st));
    return DNAGPU_OK;
}

int text_error_rank(dnagpu_ctx *ctx, PoolScope &ps, const TextErrorIn &in, u64 pos, u64 who[3])
{
    u64 *dev = nullptr;
    RC_TRY(ps.alloc(3, &dev));
    if (in.format == TEXT_FORMAT_FASTQ)
        HIP_TRY(launch_reads_fastq_rank(in.text, in.n, in.nl_base, pos, dev, ctx->stream));
    else
        HIP_TRY(launch_text_rank(in.text, in.lim, in.format, in.rec_t, pos, dev, ctx->stream));     // (writes two words)
    return read_back(ctx, who, dev, 3 * sizeof(u64));
}

int text_error_find(dnagpu_ctx *ctx, PoolScope &ps, const TextErrorIn &in, u64 word, TextBad *bad)
{
    const u32 kind = text_error_kind(word);
    u64 who[3] = {0, 0, 0};
    RC_TRY(text_error_rank(ctx, ps, in, text_error_pos(word), who));
    *bad = TextBad{text_error_pos(word), who[0], kind == TEXT_ERR_CHAR ? (char)who[1] : (char)0, DNAGPU_ERR_BAD_ARG};
    if (kind == TEXT_ERR_CHAR) {
        set_err("Invalid character in DNA sequence: %c", (char)who[1]);
        bad->code = DNAGPU_ERR_DNA_INVALID_CHAR;
    } else if (kind == TEXT_ERR_EMPTY) {
        set_err("DNA sequence cannot be empty");
        bad->code = DNAGPU_ERR_DNA_EMPTY;
    } else if (in.format != TEXT_FORMAT_FASTQ) {
        set_err("sequence data before the first header");
    } else if (kind == TEXT_ERR_TRUNC) {
        set_err("truncated FASTQ record");
    } else if (who[2] == 0) {
        set_err("FASTQ record does not begin with '@'");
    } else {
        set_err("FASTQ separator line does not begin with '+'");
    }
    return DNAGPU_OK;
}

}  // namespace dnagpu
