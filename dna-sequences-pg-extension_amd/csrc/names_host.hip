// names_host.hip -- the dnagpu_names_* calls of include/dnagpu.h: the names column of a resident table, one string per
// sequence beside the packed stream (names_kernels.hip).  The argument rules, the order of the stages, the
// read-backs, the reports and the hand-over of the result.  (dnagpu_table_to_text_named is in export_host.hip, beside the
// image it plans.)
#include "host_common.hpp"
#include "names_math.hpp"

using namespace dnagpu;

namespace {

// A column being made: the two blocks belong to ps until hand_over
struct NewNames {
    PoolScope &ps;
    std::unique_ptr<dnagpu_names> h;
    explicit NewNames(PoolScope &scope) : ps(scope), h(new dnagpu_names) {}
    // n + 1 offsets (unless the caller has them in ps already) and the bytes of `total`; nothing is written
    int alloc(u64 n, u64 total, u64 *off = nullptr)
    {
        h->n = n;
        h->total = total;
        h->off = off;
        if (!off)
            RC_TRY(ps.alloc((size_t)n + 1, &h->off));
        return ps.alloc((size_t)names_alloc_bytes(total), &h->bytes);
    }
    void hand_over(dnagpu_names **out)               // (the caller has waited for the stream)
    {
        ps.release(h->off);
        ps.release(h->bytes);
        *out = h.release();
    }
};

// the column of no sequence: one offset, 0.  Waits.
int empty_column(dnagpu_ctx *ctx, PoolScope &ps, dnagpu_names **out)
{
    HIP_TRY(hipSetDevice(ctx->device));
    NewNames nn(ps);
    RC_TRY(nn.alloc(0, 0));
    const u64 zero = 0;
    HIP_TRY(poke(nn.h->off, &zero, sizeof zero, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    nn.hand_over(out);
    return DNAGPU_OK;
}

int bad_character(u64 pos, char c, u64 record, dnagpu_names_report *report)
{
    if (report) {
        report->bad_pos = pos;
        report->bad_record = record;
        report->bad_char = c;
    }
    set_err("invalid character in a read name");
    return DNAGPU_ERR_BAD_ARG;
}

// the lowest offset of a '\n' or '\r' in the column's bytes, NAMES_NO_ERROR when it has none.  Waits.
int first_forbidden(dnagpu_ctx *ctx, PoolScope &ps, const dnagpu_names *h, u64 *pos)
{
    unsigned long long *res = nullptr;
    RC_TRY(ps.alloc(1, &res));
    const u64 none = NAMES_NO_ERROR;
    HIP_TRY(poke(res, &none, sizeof none, ctx->stream));
    HIP_TRY(launch_names_validate(h->bytes, h->total, res, ctx->stream));
    return read_back(ctx, pos, res, sizeof *pos);
}

int upload(dnagpu_ctx *ctx, const char *bytes, const u64 *offsets, u64 n, int on_device, dnagpu_names **out,
           dnagpu_names_report *report)
{
    PoolScope ps(ctx);
    if (n == 0)
        return empty_column(ctx, ps, out);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    u64 *off = nullptr;
    unsigned long long *res = nullptr;
    RC_TRY(ps.alloc((size_t)n + 1, &off));
    RC_TRY(ps.alloc(NAMES_R_WORDS, &res));
    const u64 res0[NAMES_R_WORDS] = {0, 0, 0};
    HIP_TRY(poke(res, res0, sizeof res0, st));
    HIP_TRY(hipMemcpyAsync(off, offsets, (size_t)(n + 1) * 8, kind, st));
    HIP_TRY(launch_names_offsets_check(off, n, res, st));
    u64 got[NAMES_R_WORDS] = {};
    RC_TRY(read_back(ctx, got, res, sizeof got));    // (waits for the stream: a host array has been read)
    if (got[NAMES_R_BAD]) {
        set_err("names_upload: offsets[0] is not 0, or an offset is below the one before it");
        return DNAGPU_ERR_BAD_ARG;
    }
    const u64 total = got[NAMES_R_TOTAL];
    if (total > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    if (total && !bytes)
        return DNAGPU_ERR_BAD_ARG;
    NewNames nn(ps);
    RC_TRY(nn.alloc(n, total, off));
    if (total) {
        HIP_TRY(hipMemcpyAsync(nn.h->bytes, bytes, (size_t)total, kind, st));
        u64 pos = 0;
        RC_TRY(first_forbidden(ctx, ps, nn.h.get(), &pos));
        if (pos != NAMES_NO_ERROR) {
            u64 word = 0;                            // (the copy is kept whole on error: the byte is read from it)
            RC_TRY(read_back(ctx, &word, nn.h->bytes + (pos & ~(u64)7), sizeof word));
            return bad_character(pos, (char)(word >> (8 * (pos & 7))), ~(u64)0, report);
        }
    }
    nn.hand_over(out);
    return DNAGPU_OK;
}

struct FromText {
    const char *text;
    u64 n;
    int on_device, format;
    bool first_word;
    const u64 *record_pos;
    u64 n_records;
    const u64 *src_record;
    u64 n_seqs;
};

int from_text(dnagpu_ctx *ctx, const FromText &in, dnagpu_names **out, dnagpu_names_report *report)
{
    PoolScope ps(ctx);
    if (in.n_seqs == 0)
        return empty_column(ctx, ps, out);
    if (in.n == 0 || in.n_records == 0) {            // no byte a record could begin at
        set_err("names_from_text: a sequence's record is not among the %llu records of a text of %llu bytes",
                (unsigned long long)in.n_records, (unsigned long long)in.n);
        return DNAGPU_ERR_BAD_ARG;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    prof_begin(ctx);
    prof_mark(ctx, "names_stage");
    const u64 n = in.n, n_seqs = in.n_seqs;
    const unsigned char *dtext = nullptr;
    const u64 *dpos = nullptr, *dsrc = nullptr;
    RC_TRY(device_list(ctx, ps, reinterpret_cast<const unsigned char *>(in.text), n, in.on_device, &dtext));
    RC_TRY(device_list(ctx, ps, in.record_pos, in.n_records, in.on_device, &dpos));
    RC_TRY(device_list(ctx, ps, in.src_record, n_seqs, in.on_device, &dsrc));
    // ---- the bytes that end a name, and for every tile where the next one lies
    const u32 nt = (u32)text_tiles(n), groups = (u32)names_groups(nt);
    u32 *mask = nullptr, *tile_first = nullptr, *local = nullptr, *group_min = nullptr, *after = nullptr, *len32 = nullptr,
        *scan_tmp = nullptr;
    u64 *first = nullptr;
    unsigned long long *res = nullptr;
    RC_TRY(ps.alloc((size_t)names_chunks(n), &mask));
    RC_TRY(ps.alloc((size_t)nt, &tile_first));
    RC_TRY(ps.alloc((size_t)nt, &local));
    RC_TRY(ps.alloc((size_t)groups, &group_min));
    RC_TRY(ps.alloc((size_t)groups, &after));
    RC_TRY(ps.alloc((size_t)n_seqs, &first));
    RC_TRY(ps.alloc((size_t)n_seqs, &len32));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n_seqs), &scan_tmp));
    RC_TRY(ps.alloc(NAMES_R_WORDS, &res));
    const u64 res0[NAMES_R_WORDS] = {0, 0, 0};
    HIP_TRY(poke(res, res0, sizeof res0, st));
    prof_mark(ctx, "names_ends");
    HIP_TRY(launch_names_ends(dtext, n, nt, in.first_word, mask, tile_first, res, st));
    HIP_TRY(launch_names_suffix_min(tile_first, nt, local, group_min, after, st));
    // ---- every sequence's name: where it lies, its length, and the 64-bit sum of the lengths
    prof_mark(ctx, "names_spans");
    const NamesSpans sp = {dtext, n, nt, (u32)(in.format == DNAGPU_TEXT_FASTA ? '>' : '@'), mask, local, after, dpos, dsrc,
                           in.n_records, n_seqs, first, len32, res};
    HIP_TRY(launch_names_spans(sp, st));
    u64 got[NAMES_R_WORDS] = {};
    RC_TRY(read_back(ctx, got, res, sizeof got));    // (the one read-back of a text without a lone '\r'; waits for the stream)
    if (got[NAMES_R_BAD]) {
        set_err("names_from_text: a record_pos entry is not the offset of a '%c' inside the text, or a src_record entry is not "
                "below the %llu records", (char)sp.marker, (unsigned long long)in.n_records);
        return DNAGPU_ERR_BAD_ARG;
    }
    const u64 total = got[NAMES_R_TOTAL];
    if (total > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    // ---- the column: the offsets from the scanned lengths, the bytes through the column copy
    NewNames nn(ps);
    RC_TRY(nn.alloc(n_seqs, total));
    prof_mark(ctx, "names_offsets");
    HIP_TRY(launch_scan_u32(len32, len32, n_seqs, scan_tmp, nullptr, st));
    HIP_TRY(launch_take_starts(len32, n_seqs, total, nn.h->off, st));
    prof_mark(ctx, "names_copy");
    HIP_TRY(launch_quals_copy(dtext, n, first, nullptr, nn.h->off, n_seqs, total, nn.h->bytes, st));
    prof_mark(ctx, "end");
    if (got[NAMES_R_LONE_CR] && total) {             // a '\r' that ends no line: is it inside a name?
        u64 pos = 0;
        RC_TRY(first_forbidden(ctx, ps, nn.h.get(), &pos));
        if (pos != NAMES_NO_ERROR) {
            u64 *dev = nullptr, who[3] = {0, 0, 0};
            RC_TRY(ps.alloc(3, &dev));
            HIP_TRY(launch_names_locate(nn.h->off, n_seqs, pos, first, dsrc, dev, st));
            RC_TRY(read_back(ctx, who, dev, sizeof who));
            prof_end(ctx);
            return bad_character(who[1], '\r', who[2], report);
        }
    } else {
        HIP_TRY(hipStreamSynchronize(st));
    }
    prof_end(ctx);
    nn.hand_over(out);
    return DNAGPU_OK;
}

int take(dnagpu_ctx *ctx, const dnagpu_names *src, const u64 *ids, u64 n_ids, int on_device, dnagpu_names **out)
{
    PoolScope ps(ctx);
    if (n_ids == 0)
        return empty_column(ctx, ps, out);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    prof_begin(ctx);
    const TakeLists in = {ids, nullptr, nullptr, nullptr, n_ids, on_device};
    TakePlan plan = {};
    RC_TRY(take_plan(ctx, ps, in, src->off, src->n, src->total, "names_lists", &plan));
    NewNames nn(ps);
    RC_TRY(nn.alloc(n_ids, plan.total, plan.starts));
    RC_TRY(plan.queue_starts(ctx));
    prof_mark(ctx, "names_copy");
    HIP_TRY(launch_quals_copy(src->bytes, src->total, plan.seg_first, nullptr, plan.starts, n_ids, plan.total, nn.h->bytes, st));
    prof_mark(ctx, "end");
    HIP_TRY(hipStreamSynchronize(st));
    prof_end(ctx);
    nn.hand_over(out);
    return DNAGPU_OK;
}

// a window of a device array to the caller; waits
int read_window(dnagpu_ctx *ctx, const void *src, u64 bytes, void *out, int out_on_device)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(out, src, (size_t)bytes, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
}

}  // namespace

extern "C" int dnagpu_names_upload(dnagpu_ctx *ctx, const char *bytes, const uint64_t *offsets, uint64_t n, int on_device,
                                   dnagpu_names **out, dnagpu_names_report *report)
{
    return guarded([&]() -> int {
    report_clear(report);
    if (!ctx || !out || (n && !offsets))
        return DNAGPU_ERR_BAD_ARG;
    if (n > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    if (n && !on_device && !bytes && offsets[n] != 0)
        return DNAGPU_ERR_BAD_ARG;                   // (offsets in device memory: found after their read-back)
    dnagpu_names *made = nullptr;
    RC_TRY(upload(ctx, bytes, offsets, n, on_device, &made, report));
    *out = made;
    return DNAGPU_OK;
    });
}

extern "C" uint64_t dnagpu_names_sequences(const dnagpu_names *names) { return names ? names->n : 0; }
extern "C" uint64_t dnagpu_names_bytes(const dnagpu_names *names) { return names ? names->total : 0; }

extern "C" int dnagpu_names_offsets(dnagpu_ctx *ctx, const dnagpu_names *names, uint64_t first, uint64_t count, uint64_t *out,
                                    int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !names || (count && !out))
        return DNAGPU_ERR_BAD_ARG;
    const u64 entries = names->n + 1;
    if (first > entries || count > entries - first)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0)
        return DNAGPU_OK;
    return read_window(ctx, names->off + first, count * 8, out, out_on_device);
    });
}

extern "C" int dnagpu_names_read(dnagpu_ctx *ctx, const dnagpu_names *names, uint64_t first_byte, uint64_t count, char *out,
                                 int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !names || (count && !out))
        return DNAGPU_ERR_BAD_ARG;
    if (first_byte > names->total || count > names->total - first_byte)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0)
        return DNAGPU_OK;
    return read_window(ctx, names->bytes + first_byte, count, out, out_on_device);
    });
}

extern "C" void dnagpu_names_free(dnagpu_ctx *ctx, dnagpu_names *names)
{
    if (!names)
        return;
    if (ctx) {
        if (names->bytes)
            pool_free(ctx, names->bytes);
        if (names->off)
            pool_free(ctx, names->off);
    }
    delete names;
}

extern "C" int dnagpu_names_from_text(dnagpu_ctx *ctx, const char *text, uint64_t n_bytes, int text_on_device, int format,
                                      unsigned flags, const uint64_t *record_pos, uint64_t n_records, const uint64_t *src_record,
                                      uint64_t n_seqs, dnagpu_names **out, dnagpu_names_report *report)
{
    return guarded([&]() -> int {
    report_clear(report);
    if (!ctx || !out || (n_bytes && !text) || (n_records && !record_pos))
        return DNAGPU_ERR_BAD_ARG;
    if (format != DNAGPU_TEXT_FASTA && format != DNAGPU_TEXT_FASTQ)
        return DNAGPU_ERR_BAD_ARG;                   // (LINES has no names)
    if (flags & ~DNAGPU_NAMES_FIRST_WORD)
        return DNAGPU_ERR_BAD_ARG;
    if (!src_record && n_seqs != n_records)
        return DNAGPU_ERR_BAD_ARG;
    if (n_bytes > U32_MAX64 || n_records > U32_MAX64 || n_seqs > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    const FromText in = {text, n_bytes, text_on_device, format, (flags & DNAGPU_NAMES_FIRST_WORD) != 0, record_pos, n_records,
                         src_record, n_seqs};
    dnagpu_names *made = nullptr;
    RC_TRY(from_text(ctx, in, &made, report));
    *out = made;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_names_take(dnagpu_ctx *ctx, const dnagpu_names *names, const uint64_t *seq_ids, uint64_t n_ids, int on_device,
                                 dnagpu_names **out)
{
    return guarded([&]() -> int {
    if (!ctx || !names || !out || (n_ids && !seq_ids))
        return DNAGPU_ERR_BAD_ARG;
    if (n_ids > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;
    if (n_ids && names->n == 0) {
        set_err("take: a sequence id is not below the table's 0 sequences");
        return DNAGPU_ERR_BAD_ARG;
    }
    dnagpu_names *made = nullptr;
    RC_TRY(take(ctx, names, seq_ids, n_ids, on_device, &made));
    *out = made;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_names_geometry(uint64_t *chunk_bytes, uint64_t *tile_bytes, uint64_t *group_tiles)
{
    if (!chunk_bytes || !tile_bytes || !group_tiles)
        return DNAGPU_ERR_BAD_ARG;
    *chunk_bytes = TEXT_CHUNK;
    *tile_bytes = TEXT_TILE_BYTES;
    *group_tiles = NAMES_GROUP_TILES;
    return DNAGPU_OK;
}
