// text_host.hip -- dnagpu_table_from_text and dnagpu_text_geometry of include/dnagpu.h: the raw bytes of a text file of
// sequences (one per line, or FASTA) into a resident table, on the device (text_kernels.hip).  The argument
// rules, the order of the stages, the one read-back, the report and the hand-over of the result.
#include "host_common.hpp"
#include "text_math.hpp"

using namespace dnagpu;

namespace {

void report_clear(dnagpu_text_report *r)
{
    if (!r)
        return;
    memset(r, 0, sizeof *r);
    r->bad_pos = ~(u64)0;
    r->bad_record = ~(u64)0;
}

// a valid dna of 0 bases with no set: what dnagpu_dna_take makes of no segment
int empty_table(PoolScope &ps, dnagpu_dna **out)
{
    std::unique_ptr<dnagpu_dna> h(new dnagpu_dna{nullptr, 0, 0, true});
    RC_TRY(ps.alloc(1, &h->words));
    ps.release(h->words);
    *out = h.release();
    return DNAGPU_OK;
}

int from_text(dnagpu_ctx *ctx, const char *text, u64 n, int text_on_device, int format, bool more, dnagpu_dna **out,
              u64 *out_record_pos, u64 record_cap, dnagpu_text_report *report)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    if (n == 0)
        return empty_table(ps, out);
    const bool fasta = format == TEXT_FORMAT_FASTA;
    prof_begin(ctx);
    prof_mark(ctx, "text_stage");
    const unsigned char *dtext = reinterpret_cast<const unsigned char *>(text);
    if (!text_on_device) {
        unsigned char *stage = nullptr;
        RC_TRY(ps.alloc((size_t)n, &stage));
        HIP_TRY(hipMemcpyAsync(stage, text, (size_t)n, hipMemcpyHostToDevice, st));
        dtext = stage;
    }
    // ---- res = {error word, records, bases, bytes that count}: what the one read-back brings home
    const u32 nt = (u32)text_tiles(n);
    u64 *res = nullptr;
    RC_TRY(ps.alloc(4, &res));
    const u64 res0[4] = {TEXT_NO_ERROR, 0, 0, n};
    HIP_TRY(poke(res, res0, sizeof res0, st));
    if (more) {
        prof_mark(ctx, "text_cut");
        HIP_TRY(launch_text_cut(dtext, n, format, res + 3, st));
    }
    TextSweep a = {};
    a.text = dtext;
    a.lim = res + 3;
    a.format = format;
    a.n_tiles = nt;
    a.res = res;
    u32 *scan_tmp = nullptr, *last_header = nullptr, *seq_before_t = nullptr;
    RC_TRY(ps.alloc((size_t)nt, &a.keep_t));
    RC_TRY(ps.alloc((size_t)nt, &a.rec_t));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(nt), &scan_tmp));
    if (fasta) {                                     // the state every tile begins in
        u32 *last_start = nullptr, *in_state = nullptr, *header_before = nullptr;
        RC_TRY(ps.alloc((size_t)nt, &last_start));
        RC_TRY(ps.alloc((size_t)nt, &last_header));
        RC_TRY(ps.alloc((size_t)nt, &in_state));
        RC_TRY(ps.alloc((size_t)nt, &header_before));
        RC_TRY(ps.alloc((size_t)nt, &a.last_seq));
        RC_TRY(ps.alloc((size_t)nt, &a.first_header));
        RC_TRY(ps.alloc((size_t)nt, &a.seq_before));
        RC_TRY(ps.alloc((size_t)nt, &seq_before_t));
        prof_mark(ctx, "text_heads");
        HIP_TRY(launch_text_heads(dtext, a.lim, nt, last_start, last_header, st));
        HIP_TRY(launch_text_max_scan(last_start, in_state, nt, st));
        HIP_TRY(launch_text_max_scan(last_header, header_before, nt, st));
        a.in_state = in_state;
        a.header_before = header_before;
    }
    prof_mark(ctx, "text_sweep");
    HIP_TRY(launch_text_sweep(a, st));
    prof_mark(ctx, "text_scan");
    if (fasta) {
        HIP_TRY(launch_text_max_scan(a.last_seq, seq_before_t, nt, st));
        HIP_TRY(launch_text_finish(a, last_header, seq_before_t, st));
    }
    // (the totals are 32-bit -- n < 2^32 -- and land in the low halves of res[1] and res[2], whose high halves are zero)
    HIP_TRY(launch_scan_u32(a.rec_t, a.rec_t, nt, scan_tmp, reinterpret_cast<u32 *>(res + 1), st));
    HIP_TRY(launch_scan_u32(a.keep_t, a.keep_t, nt, scan_tmp, reinterpret_cast<u32 *>(res + 2), st));
    u64 got[4] = {0, 0, 0, 0};
    RC_TRY(read_back(ctx, got, res, sizeof got));    // (waits for the stream: a host text has been read)
    if (got[0] != TEXT_NO_ERROR) {
        const u64 pos = text_error_pos(got[0]);
        const u32 kind = text_error_kind(got[0]);
        u64 *who = nullptr, hwho[2] = {0, 0};
        RC_TRY(ps.alloc(2, &who));
        HIP_TRY(launch_text_rank(dtext, a.lim, format, a.rec_t, pos, who, st));
        RC_TRY(read_back(ctx, hwho, who, sizeof hwho));
        if (report) {
            report->bad_pos = pos;
            report->bad_record = hwho[0];
            report->bad_char = kind == TEXT_ERR_CHAR ? (char)hwho[1] : 0;
        }
        if (kind == TEXT_ERR_CHAR) {
            set_err("Invalid character in DNA sequence: %c", (char)hwho[1]);
            return DNAGPU_ERR_DNA_INVALID_CHAR;
        }
        if (kind == TEXT_ERR_EMPTY) {
            set_err("DNA sequence cannot be empty");
            return DNAGPU_ERR_DNA_EMPTY;
        }
        set_err("sequence data before the first header");
        return DNAGPU_ERR_BAD_ARG;
    }
    const u64 records = got[1], bases = got[2];
    if (report) {
        report->records = records;
        report->bases = bases;
        report->consumed = got[3];
    }
    if (records == 0)                                // (then there is no base either: every base belongs to a record)
        return empty_table(ps, out);

    // ---- the result: the stream, the starts, the marks; nothing of it is assumed zero
    std::unique_ptr<dnagpu_dna> h(new dnagpu_dna{nullptr, 0, 0, true});
    const u64 nw = text_words(bases), n_mark_words = text_mark_words(bases);
    const u64 n_pos = out_record_pos ? std::min(records, record_cap) : 0;
    u64 *pos_dev = text_on_device ? out_record_pos : nullptr;
    RC_TRY(ps.alloc((size_t)records + 1, &h->seq_starts));
    RC_TRY(ps.alloc((size_t)n_mark_words, &h->seq_marks));
    RC_TRY(ps.alloc((size_t)std::max<u64>(nw, 1), &h->words));
    if (n_pos && !text_on_device)
        RC_TRY(ps.alloc((size_t)n_pos, &pos_dev));
    prof_mark(ctx, "text_pack");
    HIP_TRY(launch_text_pack(a, bases, records, h->words, h->seq_starts, n_pos ? pos_dev : nullptr, n_pos, st));
    prof_mark(ctx, "text_marks");
    HIP_TRY(launch_batch_marks(h->seq_starts, records, h->seq_marks, n_mark_words, st));
    if (n_pos && !text_on_device)
        HIP_TRY(hipMemcpyAsync(out_record_pos, pos_dev, (size_t)n_pos * 8, hipMemcpyDeviceToHost, st));
    prof_mark(ctx, "end");
    HIP_TRY(hipStreamSynchronize(st));
    prof_end(ctx);
    ps.release(h->seq_starts);
    ps.release(h->seq_marks);
    ps.release(h->words);
    h->n_words = nw;
    h->n_bases = bases;
    h->n_seqs = records;
    h->n_mark_words = n_mark_words;
    *out = h.release();
    return DNAGPU_OK;
}

}  // namespace

extern "C" int dnagpu_table_from_text(dnagpu_ctx *ctx, const char *text, uint64_t n_bytes, int text_on_device, int format,
                                      unsigned flags, dnagpu_dna **out, uint64_t *out_record_pos, uint64_t record_cap,
                                      dnagpu_text_report *report)
{
    return guarded([&]() -> int {
    report_clear(report);
    if (!ctx || !out || (n_bytes && !text) || (record_cap && !out_record_pos))
        return DNAGPU_ERR_BAD_ARG;
    if ((format != DNAGPU_TEXT_LINES && format != DNAGPU_TEXT_FASTA) || (flags & ~DNAGPU_TEXT_MORE))
        return DNAGPU_ERR_BAD_ARG;
    if (n_bytes > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    dnagpu_dna *made = nullptr;
    RC_TRY(from_text(ctx, text, n_bytes, text_on_device, format, (flags & DNAGPU_TEXT_MORE) != 0, &made, out_record_pos, record_cap,
                     report));
    *out = made;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_text_geometry(uint64_t *tile_bytes)
{
    if (!tile_bytes)
        return DNAGPU_ERR_BAD_ARG;
    *tile_bytes = TEXT_TILE_BYTES;
    return DNAGPU_OK;
}
