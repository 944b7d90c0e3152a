// quals_host.hip -- the dnagpu_quals_* calls of include/dnagpu.h: the quality column of a resident table, one Phred+33 byte per
// base beside the packed stream (quals_kernels.hip).  The argument rules, the order of the stages, the
// read-backs, the reports and the hand-over of the result.  (dnagpu_text_image_read_quals is in export_host.hip, beside the
// image it reads.)
#include "host_common.hpp"
#include "quals_math.hpp"
#include "text_math.hpp"

using namespace dnagpu;

namespace {

// a column of n bytes that nothing has written yet, owned by ps until the caller releases its bytes
int column_new(PoolScope &ps, u64 n, std::unique_ptr<dnagpu_quals> *out)
{
    std::unique_ptr<dnagpu_quals> q(new dnagpu_quals);
    RC_TRY(ps.alloc((size_t)quals_alloc_bytes(n), &q->bytes));
    q->n = n;
    *out = std::move(q);
    return DNAGPU_OK;
}

int bad_character(u64 pos, char c, u64 record, dnagpu_quals_report *report)
{
    if (report) {
        report->bad_pos = pos;
        report->bad_record = record;
        report->bad_char = c;
    }
    set_err("invalid FASTQ quality character");
    return DNAGPU_ERR_BAD_ARG;
}

int upload(dnagpu_ctx *ctx, const char *bytes, u64 n, int on_device, dnagpu_quals **out, dnagpu_quals_report *report)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    std::unique_ptr<dnagpu_quals> q;
    RC_TRY(column_new(ps, n, &q));
    if (n) {
        unsigned long long *res = nullptr;
        RC_TRY(ps.alloc(1, &res));
        const u64 none = QUALS_NO_ERROR;
        HIP_TRY(poke(res, &none, sizeof none, st));
        HIP_TRY(hipMemcpyAsync(q->bytes, bytes, (size_t)n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        HIP_TRY(launch_quals_validate(q->bytes, n, res, st));
        u64 got = 0;
        RC_TRY(read_back(ctx, &got, res, sizeof got));           // (waits for the stream: a host array has been read)
        if (got != QUALS_NO_ERROR) {
            const u64 pos = quals_error_pos(got);
            u64 word = 0;                                        // (the copy is kept whole on error: the byte is read from it)
            RC_TRY(read_back(ctx, &word, q->bytes + (pos & ~(u64)7), sizeof word));
            return bad_character(pos, (char)(word >> (8 * (pos & 7))), ~(u64)0, report);
        }
    } else {
        HIP_TRY(hipStreamSynchronize(st));
    }
    ps.release(q->bytes);
    *out = q.release();
    return DNAGPU_OK;
}

// the words of res that the load brings home
enum { Q_ERROR, Q_RECORDS, Q_BAD_SOURCE, Q_NEWLINES, Q_WORDS };

int from_fastq(dnagpu_ctx *ctx, const char *text, u64 n, int text_on_device, const dnagpu_dna *table, const u64 *src_record,
               const u64 *src_offset, dnagpu_quals **out, dnagpu_quals_report *report)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    std::unique_ptr<dnagpu_quals> q;
    const u64 n_seqs = table->n_seqs, total = table->n_bases;
    if (n == 0) {                                    // no record: the column of a table of no base
        if (total) {
            set_err("quals_from_fastq: a sequence's source is not among the text's 0 records");
            return DNAGPU_ERR_BAD_ARG;
        }
        RC_TRY(column_new(ps, 0, &q));
        ps.release(q->bytes);
        *out = q.release();
        return DNAGPU_OK;
    }
    prof_begin(ctx);
    prof_mark(ctx, "quals_stage");
    const unsigned char *dtext = nullptr;
    RC_TRY(device_list(ctx, ps, reinterpret_cast<const unsigned char *>(text), n, text_on_device, &dtext));
    const u64 *drec = nullptr, *doff = nullptr;
    if (n_seqs) {
        RC_TRY(device_list(ctx, ps, src_record, n_seqs, text_on_device, &drec));
        RC_TRY(device_list(ctx, ps, src_offset, n_seqs, text_on_device, &doff));
    }
    // ---- every line's index: the '\n' per tile and their scan; the truncated record comes from the same counts
    const u32 nt = (u32)text_tiles(n);
    u64 *res = nullptr;
    u32 *nl_t = nullptr, *nl_base = nullptr, *scan_tmp = nullptr;
    RC_TRY(ps.alloc(Q_WORDS, &res));
    RC_TRY(ps.alloc((size_t)nt, &nl_t));
    RC_TRY(ps.alloc((size_t)nt, &nl_base));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(nt), &scan_tmp));
    const u64 res0[Q_WORDS] = {QUALS_NO_ERROR, 0, 0, 0};
    HIP_TRY(poke(res, res0, sizeof res0, st));
    prof_mark(ctx, "quals_newlines");
    HIP_TRY(launch_reads_newlines(dtext, n, nt, nl_t, st));
    u32 *newlines = reinterpret_cast<u32 *>(res + Q_NEWLINES);
    HIP_TRY(launch_scan_u32(nl_t, nl_base, nt, scan_tmp, newlines, st));
    HIP_TRY(launch_reads_fastq_cut(dtext, n, nt, nl_t, nl_base, newlines, false, res + Q_RECORDS, res, st));    // (the error word only)
    u64 got[Q_WORDS] = {};
    RC_TRY(read_back(ctx, got, res, sizeof got));    // (waits for the stream)
    const u64 records_cap = (got[Q_NEWLINES] + 1) / 4;           // (the lines are the '\n', and one more without a last '\n')

    // ---- the lines of every record, their lengths, the source of every sequence
    u32 *rec = nullptr;
    u64 *src_at = nullptr;
    RC_TRY(ps.alloc((size_t)std::max<u64>(records_cap, 1) * QUALS_REC_WORDS, &rec));
    RC_TRY(ps.alloc((size_t)std::max<u64>(n_seqs, 1), &src_at));
    unsigned long long *ures = reinterpret_cast<unsigned long long *>(res);
    prof_mark(ctx, "quals_lines");
    HIP_TRY(launch_quals_lines(dtext, n, nt, nl_base, newlines, rec, ures, st));
    HIP_TRY(launch_quals_lengths(dtext, n, newlines, rec, records_cap, ures, st));
    HIP_TRY(launch_quals_sources(dtext, n, newlines, rec, table->seq_starts, n_seqs, drec, doff, src_at, ures, st));
    RC_TRY(read_back(ctx, got, res, sizeof got));
    if (report)
        report->records = got[Q_RECORDS];
    if (got[Q_ERROR] != QUALS_NO_ERROR) {
        const u64 pos = quals_error_pos(got[Q_ERROR]);
        const u32 kind = quals_error_kind(got[Q_ERROR]);
        u64 hwho[3] = {0, 0, 0};
        RC_TRY(text_error_rank(ctx, ps, TextErrorIn{dtext, n, nullptr, TEXT_FORMAT_FASTQ, nullptr, nl_base}, pos, hwho));
        if (kind == QUALS_ERR_CHAR)
            return bad_character(pos, (char)hwho[1], hwho[0], report);
        if (report) {
            report->bad_pos = pos;
            report->bad_record = hwho[0];
        }
        set_err(kind == QUALS_ERR_TRUNC ? "truncated FASTQ record" : "FASTQ quality line length differs from the sequence's");
        return DNAGPU_ERR_BAD_ARG;
    }
    if (got[Q_BAD_SOURCE]) {
        set_err("quals_from_fastq: a sequence's source is not among the text's %llu records, or leaves its quality line",
                (unsigned long long)got[Q_RECORDS]);
        return DNAGPU_ERR_BAD_ARG;
    }

    // ---- the column
    RC_TRY(column_new(ps, total, &q));
    prof_mark(ctx, "quals_copy");
    HIP_TRY(launch_quals_copy(dtext, n, src_at, nullptr, table->seq_starts, n_seqs, total, q->bytes, st));
    prof_mark(ctx, "end");
    HIP_TRY(hipStreamSynchronize(st));
    prof_end(ctx);
    ps.release(q->bytes);
    *out = q.release();
    return DNAGPU_OK;
}

// dnagpu_dna_gather's core (take_host.hip) over bytes: ids != nullptr: segment i = sequence ids[i] of the table; else
// (first, len).  Only the column is made: the starts of the result are scratch here, the table they belong to is what
// dnagpu_dna_take / dnagpu_dna_gather return for the same lists.
int gather_core(dnagpu_ctx *ctx, const dnagpu_dna *table, const dnagpu_quals *src, const TakeLists &in, dnagpu_quals **out)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    std::unique_ptr<dnagpu_quals> q;
    if (in.n == 0) {
        RC_TRY(column_new(ps, 0, &q));
        ps.release(q->bytes);
        *out = q.release();
        return DNAGPU_OK;
    }
    prof_begin(ctx);
    TakePlan plan = {};
    RC_TRY(take_plan(ctx, ps, in, table ? table->seq_starts : nullptr, table ? table->n_seqs : 0, src->n, "quals_lists", &plan));
    RC_TRY(column_new(ps, plan.total, &q));
    RC_TRY(plan.queue_starts(ctx));
    prof_mark(ctx, "quals_copy");
    HIP_TRY(launch_quals_copy(src->bytes, src->n, plan.seg_first, plan.flip, plan.starts, in.n, plan.total, q->bytes, st));
    prof_mark(ctx, "end");
    HIP_TRY(hipStreamSynchronize(st));
    prof_end(ctx);
    ps.release(q->bytes);
    *out = q.release();
    return DNAGPU_OK;
}

}  // namespace

extern "C" int dnagpu_quals_upload(dnagpu_ctx *ctx, const char *bytes, uint64_t n, int on_device, dnagpu_quals **out,
                                   dnagpu_quals_report *report)
{
    return guarded([&]() -> int {
    report_clear(report);
    if (!ctx || !out || (n && !bytes))
        return DNAGPU_ERR_BAD_ARG;
    if (n > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;                 // (a resident table holds at most 2^32 - 1 bases)
    dnagpu_quals *made = nullptr;
    RC_TRY(upload(ctx, bytes, n, on_device, &made, report));
    *out = made;
    return DNAGPU_OK;
    });
}

extern "C" uint64_t dnagpu_quals_bases(const dnagpu_quals *q) { return q ? q->n : 0; }

extern "C" int dnagpu_quals_read(dnagpu_ctx *ctx, const dnagpu_quals *q, uint64_t first, uint64_t count, char *out, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !q || (count && !out))
        return DNAGPU_ERR_BAD_ARG;
    if (first > q->n || count > q->n - first)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(out, q->bytes + first, (size_t)count, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}

extern "C" void dnagpu_quals_free(dnagpu_ctx *ctx, dnagpu_quals *q)
{
    if (!q)
        return;
    if (ctx && q->bytes)
        pool_free(ctx, q->bytes);
    delete q;
}

extern "C" int dnagpu_quals_from_fastq(dnagpu_ctx *ctx, const char *text, uint64_t n_bytes, int text_on_device, const dnagpu_dna *table,
                                       const uint64_t *src_record, const uint64_t *src_offset, dnagpu_quals **out,
                                       dnagpu_quals_report *report)
{
    return guarded([&]() -> int {
    report_clear(report);
    if (!ctx || !table || !out || (n_bytes && !text))
        return DNAGPU_ERR_BAD_ARG;
    if ((src_record == nullptr) != (src_offset == nullptr))
        return DNAGPU_ERR_BAD_ARG;
    if (table_without_set(table))
        return DNAGPU_ERR_BAD_ARG;
    if (n_bytes > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    dnagpu_quals *made = nullptr;
    RC_TRY(from_fastq(ctx, text, n_bytes, text_on_device, table, src_record, src_offset, &made, report));
    *out = made;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_quals_gather(dnagpu_ctx *ctx, const dnagpu_quals *src, const uint64_t *seg_first, const uint64_t *seg_len,
                                   const uint8_t *seg_flip, uint64_t n_segs, int on_device, dnagpu_quals **out)
{
    return guarded([&]() -> int {
    if (!ctx || !src || !out || (n_segs && (!seg_first || !seg_len)))
        return DNAGPU_ERR_BAD_ARG;
    if (n_segs > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    const TakeLists in = {nullptr, seg_first, seg_len, seg_flip, n_segs, on_device};
    return gather_core(ctx, nullptr, src, in, out);
    });
}

extern "C" int dnagpu_quals_take(dnagpu_ctx *ctx, const dnagpu_dna *table, const dnagpu_quals *quals, const uint64_t *seq_ids,
                                 const uint8_t *seq_flip, uint64_t n_ids, int on_device, dnagpu_quals **out)
{
    return guarded([&]() -> int {
    if (!ctx || !table || !quals || !out || (n_ids && !seq_ids))
        return DNAGPU_ERR_BAD_ARG;
    if (table_without_set(table))
        return DNAGPU_ERR_BAD_ARG;
    if (table->n_bases != quals->n)
        return DNAGPU_ERR_BAD_ARG;                   // (not this table's column)
    if (n_ids > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    if (n_ids && table->n_seqs == 0) {               // an empty stream without a set: a table of no sequence
        set_err("take: a sequence id is not below the table's 0 sequences");
        return DNAGPU_ERR_BAD_ARG;
    }
    const TakeLists in = {seq_ids, nullptr, nullptr, seq_flip, n_ids, on_device};
    return gather_core(ctx, table, quals, in, out);
    });
}

namespace {

struct TrimCaller {
    u64 *first, *len, *qsum, *low;       // per sequence; any may be null
    u64 *seg_seq, *seg_first, *seg_len;  // seg_cap entries each; any may be null
    u64 seg_cap;
    int on_device;
};

enum { T_PASSED, T_KEPT, T_FRONT, T_TAIL, T_SHORT, T_MEAN, T_LOW, T_WORDS };

int trim(dnagpu_ctx *ctx, const dnagpu_dna *table, const dnagpu_quals *quals, const QualsTrimOpt &o, const TrimCaller &c,
         dnagpu_quals_trim_report *report)
{
    const u64 n = table->n_seqs;
    if (report) {
        report->sequences = n;
        report->bases_in = table->n_bases;
    }
    if (n == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    prof_begin(ctx);
    prof_mark(ctx, "quals_trim");
    // ---- the four per-sequence columns: the verdicts read them all, so those the caller does not want are scratch
    OutCols<4> cols;
    RC_TRY(cols.init(ctx, ps, {c.first, c.len, c.qsum, c.low}, n, c.on_device));
    u64 *col[4];
    for (int i = 0; i < 4; i++) {
        col[i] = cols.dev(i);
        if (!col[i])
            RC_TRY(ps.alloc((size_t)n, &col[i]));
    }
    u32 *lists = nullptr, *counts = nullptr, *flags = nullptr, *rank = nullptr, *scan_tmp = nullptr;
    unsigned long long *res = nullptr;
    RC_TRY(ps.alloc((size_t)2 * n, &lists));
    RC_TRY(ps.alloc(2, &counts));
    RC_TRY(ps.alloc((size_t)n, &flags));
    RC_TRY(ps.alloc((size_t)n, &rank));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n), &scan_tmp));
    RC_TRY(ps.alloc(T_WORDS, &res));
    HIP_TRY(launch_quals_trim(quals->bytes, table->seq_starts, n, o, col[0], col[1], col[2], col[3], lists, counts, st));
    prof_mark(ctx, "quals_verdict");
    HIP_TRY(launch_quals_verdict(table->seq_starts, n, o, col[0], col[1], col[2], col[3], flags, res, st));
    // ---- the passing sequences, in table order
    const u64 cap = std::min(c.seg_cap, n);
    OutCols<3> segs;
    RC_TRY(segs.init(ctx, ps, {c.seg_seq, c.seg_first, c.seg_len}, cap, c.on_device));
    if (cap) {
        prof_mark(ctx, "quals_segments");
        HIP_TRY(launch_scan_u32(flags, rank, n, scan_tmp, nullptr, st));
        HIP_TRY(launch_quals_segments(flags, rank, col[0], col[1], n, cap, segs.dev(0), segs.dev(1), segs.dev(2), st));
    }
    prof_mark(ctx, "end");
    u64 got[T_WORDS] = {};
    RC_TRY(read_back(ctx, got, res, sizeof got));    // (the one read-back: the report; waits for the stream)
    prof_end(ctx);
    RC_TRY(cols.finish());
    RC_TRY(segs.finish(std::min(got[T_PASSED], cap)));
    if (report) {
        report->passed = got[T_PASSED];
        report->bases_kept = got[T_KEPT];
        report->cut_front = got[T_FRONT];
        report->cut_tail = got[T_TAIL];
        report->failed_short = got[T_SHORT];
        report->failed_mean = got[T_MEAN];
        report->failed_low = got[T_LOW];
    }
    return DNAGPU_OK;
}

}  // namespace

extern "C" int dnagpu_quals_trim(dnagpu_ctx *ctx, const dnagpu_dna *table, const dnagpu_quals *quals, const dnagpu_quals_trim_options *opt,
                                 uint64_t *out_first, uint64_t *out_len, uint64_t *out_qsum, uint64_t *out_low, uint64_t *seg_seq,
                                 uint64_t *seg_first, uint64_t *seg_len, uint64_t seg_cap, int out_on_device,
                                 dnagpu_quals_trim_report *report)
{
    return guarded([&]() -> int {
    if (report)
        memset(report, 0, sizeof *report);
    if (!ctx || !table || !quals || !opt)
        return DNAGPU_ERR_BAD_ARG;
    if (opt->cut_front > QUALS_MAX_THRESHOLD || opt->cut_tail > QUALS_MAX_THRESHOLD || opt->min_mean_q > QUALS_MAX_THRESHOLD ||
        opt->low_q > QUALS_MAX_THRESHOLD || opt->reserved)
        return DNAGPU_ERR_BAD_ARG;
    if (table_without_set(table))
        return DNAGPU_ERR_BAD_ARG;
    if (table->n_bases != quals->n)
        return DNAGPU_ERR_BAD_ARG;                   // (not this table's column)
    if (table->n_seqs > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    const QualsTrimOpt o = {opt->cut_front, opt->cut_tail, opt->min_mean_q, opt->low_q, opt->low_num, opt->low_den, opt->min_bases};
    const TrimCaller c = {out_first, out_len, out_qsum, out_low, seg_seq, seg_first, seg_len, seg_cap, out_on_device};
    return trim(ctx, table, quals, o, c, report);
    });
}

extern "C" int dnagpu_quals_geometry(uint64_t *group_bases, uint64_t *wave_bases, uint64_t *tile_bases)
{
    if (!group_bases || !wave_bases || !tile_bases)
        return DNAGPU_ERR_BAD_ARG;
    *group_bases = QUALS_GROUP_BASES;
    *wave_bases = QUALS_WAVE_BASES;
    *tile_bases = QUALS_TRIM_TILE_BASES;
    return DNAGPU_OK;
}

extern "C" int dnagpu_quals_copy_geometry(uint64_t *chunk_bytes, uint64_t *tile_bytes, uint64_t *lds_segments)
{
    if (!chunk_bytes || !tile_bytes || !lds_segments)
        return DNAGPU_ERR_BAD_ARG;
    *chunk_bytes = QUALS_CHUNK;
    *tile_bytes = QUALS_TILE_BYTES;
    *lds_segments = QUALS_LDS_SEGS;
    return DNAGPU_OK;
}
