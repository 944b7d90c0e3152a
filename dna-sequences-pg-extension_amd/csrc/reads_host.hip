// reads_host.hip -- dnagpu_reads_from_text of include/dnagpu.h: FASTQ and real FASTA (ambiguity letters under a policy,
// lower-case bases, a minimal length, the source of every sequence) into a resident table, on the device (reads_kernels.hip;
// DESIGN.md 4.20).  The argument rules, the order of the stages, the read-backs, the report and the hand-over of the result.
#include "host_common.hpp"
#include "text_math.hpp"

using namespace dnagpu;

namespace {

// the words of res, the block that the read-backs bring home
enum { R_ERROR, R_RECORDS, R_BASES, R_LIM, R_AMBIG, R_PIECES, R_DROPPED, R_SHORT, R_KEPT, R_KEPT_BASES, R_NEWLINES, R_WORDS };

struct Caller {
    u64 *record_pos, record_cap;
    u64 *src_record, *src_offset, seq_cap;
    int on_device;
};

int from_text(dnagpu_ctx *ctx, const char *text, u64 n, int text_on_device, const dnagpu_reads_options &opt, dnagpu_dna **out,
              const Caller &c, dnagpu_reads_report *report)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    NewTable t(ctx);
    PoolScope &ps = t.ps;
    if (n == 0)
        return t.empty(out);
    const int format = opt.format;
    const bool more = (opt.flags & DNAGPU_READS_MORE) != 0, split = opt.ambiguous == READS_AMBIG_SPLIT;
    const bool fasta = format == TEXT_FORMAT_FASTA, fastq = format == TEXT_FORMAT_FASTQ;
    prof_begin(ctx);
    prof_mark(ctx, "reads_stage");
    const unsigned char *dtext = nullptr;
    RC_TRY(device_list(ctx, ps, reinterpret_cast<const unsigned char *>(text), n, text_on_device, &dtext));
    const u32 nt = (u32)text_tiles(n);
    u64 *res = nullptr;
    RC_TRY(ps.alloc(R_WORDS, &res));
    const u64 res0[4] = {TEXT_NO_ERROR, 0, 0, n};    // (R_ERROR .. R_LIM: what one poke carries; the counters are zero)
    HIP_TRY(hipMemsetAsync(res, 0, R_WORDS * sizeof(u64), st));
    HIP_TRY(poke(res, res0, sizeof res0, st));
    ReadsSweep a = {};
    a.text = dtext;
    a.lim = res + R_LIM;
    a.format = format;
    a.ambiguous = opt.ambiguous;
    a.fold = (opt.flags & DNAGPU_READS_FOLD_CASE) != 0;
    a.n_tiles = nt;
    a.res = res;
    u32 *scan_tmp = nullptr, *nl_base = nullptr;
    RC_TRY(ps.alloc((size_t)nt, &a.keep_t));
    RC_TRY(ps.alloc((size_t)nt, &a.rec_t));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(nt), &scan_tmp));

    // ---- the state every tile begins in, and the cut
    if (fastq) {
        u32 *nl_t = nullptr;
        RC_TRY(ps.alloc((size_t)nt, &nl_t));
        RC_TRY(ps.alloc((size_t)nt, &nl_base));
        prof_mark(ctx, "reads_newlines");
        HIP_TRY(launch_reads_newlines(dtext, n, nt, nl_t, st));
        u32 *total = reinterpret_cast<u32 *>(res + R_NEWLINES);
        HIP_TRY(launch_scan_u32(nl_t, nl_base, nt, scan_tmp, total, st));
        HIP_TRY(launch_reads_fastq_cut(dtext, n, nt, nl_t, nl_base, total, more, res + R_LIM, res, st));
        a.line_base = nl_base;
    } else if (more) {
        prof_mark(ctx, "text_cut");
        HIP_TRY(launch_text_cut(dtext, n, format, res + R_LIM, st));
    }
    FastaTiles tiles;                                // FASTA: the words launch_text_finish reads
    if (fasta) {
        tiles.sw.text = dtext;
        tiles.sw.lim = a.lim;
        tiles.sw.n_tiles = nt;
        tiles.sw.res = res;
        RC_TRY(tiles.before_sweep(ctx, ps));
        a.in_state = tiles.sw.in_state;
        a.header_before = tiles.sw.header_before;
        a.last_seq = tiles.sw.last_seq;
        a.first_header = tiles.sw.first_header;
        a.seq_before = tiles.sw.seq_before;
    }
    if (split) {
        u32 *kb = nullptr, *bb = nullptr;
        RC_TRY(ps.alloc((size_t)nt, &a.piece_t));
        RC_TRY(ps.alloc((size_t)nt, &a.sc_t));
        RC_TRY(ps.alloc((size_t)nt, &a.last_keep));
        RC_TRY(ps.alloc((size_t)nt, &a.last_brk));
        RC_TRY(ps.alloc((size_t)nt, &a.undecided));
        RC_TRY(ps.alloc((size_t)nt, &kb));
        RC_TRY(ps.alloc((size_t)nt, &bb));
        a.keep_before_t = kb;
        a.brk_before_t = bb;
    }

    // ---- the first sweep and the scans
    prof_mark(ctx, "reads_sweep");
    HIP_TRY(launch_reads_sweep(a, st));
    prof_mark(ctx, "reads_scan");
    if (fasta)
        RC_TRY(tiles.after_sweep(st));
    if (split) {
        HIP_TRY(launch_text_max_scan(a.last_keep, const_cast<u32 *>(a.keep_before_t), nt, st));
        HIP_TRY(launch_text_max_scan(a.last_brk, const_cast<u32 *>(a.brk_before_t), nt, st));
        HIP_TRY(launch_reads_finish(a, st));
        HIP_TRY(launch_scan_u32(a.piece_t, a.piece_t, nt, scan_tmp, reinterpret_cast<u32 *>(res + R_PIECES), st));
        HIP_TRY(launch_scan_u32(a.sc_t, a.sc_t, nt, scan_tmp, nullptr, st));
    }
    // (the totals are 32-bit -- n < 2^32 -- and land in the low halves of their words, whose high halves are zero)
    HIP_TRY(launch_scan_u32(a.rec_t, a.rec_t, nt, scan_tmp, reinterpret_cast<u32 *>(res + R_RECORDS), st));
    HIP_TRY(launch_scan_u32(a.keep_t, a.keep_t, nt, scan_tmp, reinterpret_cast<u32 *>(res + R_BASES), st));
    u64 got[R_PIECES + 1] = {};
    RC_TRY(read_back(ctx, got, res, sizeof got));    // (waits for the stream: a host text has been read)
    if (got[R_ERROR] != TEXT_NO_ERROR)
        return text_input_error(ctx, ps, TextErrorIn{dtext, n, a.lim, format, a.rec_t, nl_base}, got[R_ERROR], report);
    const u64 records = got[R_RECORDS], all_bases = got[R_BASES], all_seqs = split ? got[R_PIECES] : records;
    if (report) {
        report->records = records;
        report->consumed = got[R_LIM];
        report->ambiguous = got[R_AMBIG];
    }
    if (records == 0)                                // (then there is no base either: every base belongs to a record)
        return t.empty(out);

    // ---- the second sweep: every sequence, before any is left out
    const bool filter = all_seqs && ((opt.ambiguous == READS_AMBIG_DROP && got[R_AMBIG]) || opt.min_bases > 1);
    const bool want_src = c.seq_cap != 0;
    const u64 n_pos = c.record_pos ? std::min(records, c.record_cap) : 0;
    OutCols<1> pos;
    u64 *src_record = nullptr, *src_offset = nullptr;
    ReadsPack p = {};
    p.n_bases = all_bases;
    p.n_seqs = all_seqs;
    p.n_records = records;
    RC_TRY(ps.alloc((size_t)all_seqs + 1, &p.starts));
    RC_TRY(ps.alloc((size_t)std::max<u64>(text_words(all_bases), 1), &p.words));
    RC_TRY(pos.init(ctx, ps, {c.record_pos}, n_pos, text_on_device));
    if (split || want_src || filter) {
        RC_TRY(ps.alloc((size_t)std::max<u64>(all_seqs, 1), &src_record));
        RC_TRY(ps.alloc((size_t)std::max<u64>(all_seqs, 1), &src_offset));
    }
    if (split)
        RC_TRY(ps.alloc((size_t)records, &p.rec_sc));
    if (filter && opt.ambiguous == READS_AMBIG_DROP) {
        RC_TRY(ps.alloc((size_t)records, &p.rec_amb));
        HIP_TRY(hipMemsetAsync(p.rec_amb, 0, (size_t)records * sizeof(u32), st));
    }
    p.record_pos = n_pos ? pos.dev(0) : nullptr;
    p.record_cap = n_pos;
    p.src_record = src_record;
    p.src_offset = src_offset;
    prof_mark(ctx, "reads_pack");
    HIP_TRY(launch_reads_pack(a, p, st));
    if (split && all_seqs)
        HIP_TRY(launch_reads_offsets(src_record, src_offset, p.rec_sc, all_seqs, st));
    else if (src_record && all_seqs)
        HIP_TRY(launch_reads_identity(src_record, src_offset, all_seqs, st));

    // ---- DROP and min_bases: the sequences that stay, gathered as dnagpu_dna_take gathers
    u64 n_seqs = all_seqs, bases = all_bases;
    u64 *starts = p.starts, *words = p.words;
    if (filter) {
        prof_mark(ctx, "reads_select");
        u32 *flags = nullptr, *rank = nullptr, *len32 = nullptr, *tmp = nullptr;
        u64 *seg_first = nullptr, *rec2 = nullptr, *off2 = nullptr;
        RC_TRY(ps.alloc((size_t)all_seqs, &flags));
        RC_TRY(ps.alloc((size_t)all_seqs, &rank));
        RC_TRY(ps.alloc((size_t)all_seqs, &len32));
        RC_TRY(ps.alloc((size_t)scan_tmp_words(all_seqs), &tmp));
        RC_TRY(ps.alloc((size_t)all_seqs, &seg_first));
        RC_TRY(ps.alloc((size_t)all_seqs, &rec2));
        RC_TRY(ps.alloc((size_t)all_seqs, &off2));
        HIP_TRY(launch_reads_select(p.starts, p.rec_amb, all_seqs, opt.min_bases, flags, res + R_DROPPED, st));
        HIP_TRY(launch_scan_u32(flags, rank, all_seqs, tmp, reinterpret_cast<u32 *>(res + R_KEPT), st));
        HIP_TRY(hipMemsetAsync(len32, 0, (size_t)all_seqs * sizeof(u32), st));
        HIP_TRY(launch_reads_move(p.starts, src_record, src_offset, flags, rank, all_seqs, seg_first, len32, rec2, off2, st));
        HIP_TRY(launch_scan_u32(len32, len32, all_seqs, tmp, reinterpret_cast<u32 *>(res + R_KEPT_BASES), st));
        u64 kept[4] = {};
        RC_TRY(read_back(ctx, kept, res + R_DROPPED, sizeof kept));
        if (report) {
            report->dropped = kept[0];
            report->short_out = kept[1];
        }
        if (kept[2] < all_seqs) {                    // (nothing left out: the packed table is the result)
            n_seqs = kept[2];
            bases = kept[3];
            src_record = rec2;
            src_offset = off2;
            if (n_seqs) {
                RC_TRY(ps.alloc((size_t)n_seqs + 1, &starts));
                RC_TRY(ps.alloc((size_t)std::max<u64>(text_words(bases), 1), &words));
                prof_mark(ctx, "reads_take");
                HIP_TRY(launch_take_starts(len32, n_seqs, bases, starts, st));
                HIP_TRY(launch_take_copy(p.words, seg_first, nullptr, starts, n_seqs, bases, words, st));
            }
        }
    }

    // ---- the caller's arrays, the marks, the hand-over.  (src_record / src_offset keep their own copies: their count is not
    // record_pos's, and copy_cols would wait for the stream a second time.)
    const u64 n_src = std::min(n_seqs, c.seq_cap);
    const hipMemcpyKind kind = text_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (n_src && c.src_record)
        HIP_TRY(hipMemcpyAsync(c.src_record, src_record, (size_t)n_src * 8, kind, st));
    if (n_src && c.src_offset)
        HIP_TRY(hipMemcpyAsync(c.src_offset, src_offset, (size_t)n_src * 8, kind, st));
    if (report) {
        report->sequences = n_seqs;
        report->bases = bases;
    }
    if (n_seqs == 0) {
        RC_TRY(pos.finish());
        prof_mark(ctx, "end");
        prof_end(ctx);
        return t.empty(out);
    }
    RC_TRY(t.alloc(n_seqs, bases, starts, words));   // (the packed or the gathered blocks are the result's)
    prof_mark(ctx, "reads_marks");
    RC_TRY(t.queue_marks(st));
    prof_mark(ctx, "end");
    RC_TRY(pos.finish());                            // (the call's one wait at the end)
    prof_end(ctx);
    t.hand_over(out);
    return DNAGPU_OK;
}

}  // namespace

extern "C" int dnagpu_reads_from_text(dnagpu_ctx *ctx, const char *text, uint64_t n_bytes, int text_on_device,
                                      const dnagpu_reads_options *opt, dnagpu_dna **out, uint64_t *out_record_pos,
                                      uint64_t record_cap, uint64_t *out_src_record, uint64_t *out_src_offset, uint64_t seq_cap,
                                      dnagpu_reads_report *report)
{
    return guarded([&]() -> int {
    report_clear(report);
    if (!ctx || !opt || !out || (n_bytes && !text))
        return DNAGPU_ERR_BAD_ARG;
    if ((record_cap && !out_record_pos) || (seq_cap && !out_src_record && !out_src_offset))
        return DNAGPU_ERR_BAD_ARG;
    if (seq_cap && (!out_src_record || !out_src_offset))
        return DNAGPU_ERR_BAD_ARG;
    if (opt->format != DNAGPU_TEXT_LINES && opt->format != DNAGPU_TEXT_FASTA && opt->format != DNAGPU_TEXT_FASTQ)
        return DNAGPU_ERR_BAD_ARG;
    if (opt->ambiguous < DNAGPU_AMBIG_ERROR || opt->ambiguous > DNAGPU_AMBIG_SPLIT ||
        (opt->flags & ~(DNAGPU_READS_MORE | DNAGPU_READS_FOLD_CASE)) || opt->reserved)
        return DNAGPU_ERR_BAD_ARG;
    if (n_bytes > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    dnagpu_dna *made = nullptr;
    const Caller c = {out_record_pos, record_cap, out_src_record, out_src_offset, seq_cap, text_on_device};
    RC_TRY(from_text(ctx, text, n_bytes, text_on_device, *opt, &made, c, report));
    *out = made;
    return DNAGPU_OK;
    });
}
