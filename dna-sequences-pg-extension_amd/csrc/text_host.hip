// text_host.hip -- dnagpu_table_from_text and dnagpu_text_geometry of include/dnagpu.h: the raw bytes of a text file of
// sequences (one per line, or FASTA) into a resident table, on the device (text_kernels.hip).  The argument
// rules, the order of the stages, the one read-back, the report and the hand-over of the result.
#include "host_common.hpp"
#include "text_math.hpp"

using namespace dnagpu;

namespace {

int from_text(dnagpu_ctx *ctx, const char *text, u64 n, int text_on_device, int format, bool more, dnagpu_dna **out,
              u64 *out_record_pos, u64 record_cap, dnagpu_text_report *report)
{
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    NewTable t(ctx);
    PoolScope &ps = t.ps;
    if (n == 0)
        return t.empty(out);
    const bool fasta = format == TEXT_FORMAT_FASTA;
    prof_begin(ctx);
    prof_mark(ctx, "text_stage");
    const unsigned char *dtext = nullptr;
    RC_TRY(device_list(ctx, ps, reinterpret_cast<const unsigned char *>(text), n, text_on_device, &dtext));
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
    FastaTiles tiles;
    TextSweep &a = tiles.sw;
    a.text = dtext;
    a.lim = res + 3;
    a.format = format;
    a.n_tiles = nt;
    a.res = res;
    u32 *scan_tmp = nullptr;
    RC_TRY(ps.alloc((size_t)nt, &a.keep_t));
    RC_TRY(ps.alloc((size_t)nt, &a.rec_t));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(nt), &scan_tmp));
    if (fasta)                                       // the state every tile begins in
        RC_TRY(tiles.before_sweep(ctx, ps));
    prof_mark(ctx, "text_sweep");
    HIP_TRY(launch_text_sweep(a, st));
    prof_mark(ctx, "text_scan");
    if (fasta)
        RC_TRY(tiles.after_sweep(st));
    // (the totals are 32-bit -- n < 2^32 -- and land in the low halves of res[1] and res[2], whose high halves are zero)
    HIP_TRY(launch_scan_u32(a.rec_t, a.rec_t, nt, scan_tmp, reinterpret_cast<u32 *>(res + 1), st));
    HIP_TRY(launch_scan_u32(a.keep_t, a.keep_t, nt, scan_tmp, reinterpret_cast<u32 *>(res + 2), st));
    u64 got[4] = {0, 0, 0, 0};
    RC_TRY(read_back(ctx, got, res, sizeof got));    // (waits for the stream: a host text has been read)
    if (got[0] != TEXT_NO_ERROR)
        return text_input_error(ctx, ps, TextErrorIn{dtext, n, a.lim, format, a.rec_t, nullptr}, got[0], report);
    const u64 records = got[1], bases = got[2];
    if (report) {
        report->records = records;
        report->bases = bases;
        report->consumed = got[3];
    }
    if (records == 0)                                // (then there is no base either: every base belongs to a record)
        return t.empty(out);

    // ---- the result: the stream, the starts, the marks; nothing of it is assumed zero
    const u64 n_pos = out_record_pos ? std::min(records, record_cap) : 0;
    OutCols<1> pos;
    RC_TRY(t.alloc(records, bases));
    RC_TRY(pos.init(ctx, ps, {out_record_pos}, n_pos, text_on_device));
    prof_mark(ctx, "text_pack");
    HIP_TRY(launch_text_pack(a, bases, records, t.h->words, t.h->seq_starts, n_pos ? pos.dev(0) : nullptr, n_pos, st));
    prof_mark(ctx, "text_marks");
    RC_TRY(t.queue_marks(st));
    prof_mark(ctx, "end");
    RC_TRY(pos.finish());                            // (the call's one wait at the end)
    prof_end(ctx);
    t.hand_over(out);
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
