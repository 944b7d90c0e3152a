// export_host.hip -- dnagpu_table_to_text and the dnagpu_text_image_* calls of include/dnagpu.h: a resident table written out as
// text, FASTA or FASTQ on the device (export_kernels.hip).  The argument rules, the plan -- record sizes,
// their 64-bit sum, the scan, the record offsets -- and the window reads.
#include "export_math.hpp"
#include "host_common.hpp"

using namespace dnagpu;

// The plan of an image.  It BORROWS the table (its stream and starts are read by every dnagpu_text_image_read) and owns the
// record offsets, the prefix and the copy of the caller's numbers.
struct dnagpu_text_image {
    const dnagpu_dna *table = nullptr;
    ExportFmt fmt = {};
    u64 n = 0, bytes = 0, empty = 0, name_base = 0;
    u64 *pos = nullptr;                 // pool memory: n + 1 record offsets, then EXPORT_PREFIX_MAX bytes of prefix
    u64 *numbers = nullptr;             // pool memory, n entries, or null
    const dnagpu_names *names = nullptr;    // dnagpu_table_to_text_named: BORROWED like the table; the headers are its strings
    unsigned char prefix[EXPORT_PREFIX_MAX] = {};
};

namespace {

int check_options(const dnagpu_text_out_options *opt)
{
    if (opt->format < DNAGPU_TEXT_LINES || opt->format > DNAGPU_TEXT_FASTQ || (opt->flags & ~DNAGPU_TEXT_OUT_CRLF) != 0)
        return DNAGPU_ERR_BAD_ARG;
    if (opt->reserved[0] || opt->reserved[1] || opt->reserved[2])
        return DNAGPU_ERR_BAD_ARG;
    if (opt->prefix_len > EXPORT_PREFIX_MAX || (opt->prefix_len && !opt->name_prefix))
        return DNAGPU_ERR_BAD_ARG;
    for (u32 i = 0; i < opt->prefix_len; i++)
        if (opt->name_prefix[i] == '\n' || opt->name_prefix[i] == '\r') {
            set_err("table_to_text: the name prefix holds a line terminator");
            return DNAGPU_ERR_BAD_ARG;
        }
    const unsigned char q = (unsigned char)opt->quality;
    if (q != 0 && (q < 33 || q > 126))
        return DNAGPU_ERR_BAD_ARG;
    if (opt->line_width != 0 && opt->format != DNAGPU_TEXT_FASTA)
        return DNAGPU_ERR_BAD_ARG;
    return DNAGPU_OK;
}

int plan_image(dnagpu_ctx *ctx, const dnagpu_dna *table, const dnagpu_names *names, const dnagpu_text_out_options *opt,
               dnagpu_text_image *img)
{
    const u64 n = table->n_seqs;
    img->table = table;
    img->names = names;
    img->n = n;
    img->fmt.format = opt->format;
    img->fmt.term = opt->flags & DNAGPU_TEXT_OUT_CRLF ? 2 : 1;
    img->fmt.width = opt->line_width;
    const bool named = opt->format != DNAGPU_TEXT_LINES && !names;   // LINES and a names column ignore prefix, base and numbers
    img->fmt.prefix_len = named ? opt->prefix_len : 0;
    img->fmt.quality = opt->quality ? (unsigned char)opt->quality : (unsigned char)'I';
    img->name_base = named ? opt->name_base : 0;
    if (img->fmt.prefix_len)
        memcpy(img->prefix, opt->name_prefix, img->fmt.prefix_len);
    if (n == 0)
        return DNAGPU_OK;                            // an image of 0 bytes that holds no device memory
    if (n > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;                 // (every record has a terminator: the extras exceed 2^32 - 1)
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    prof_begin(ctx);
    prof_mark(ctx, "export_lists");
    const u64 *numbers = nullptr;
    if (named && opt->numbers) {                     // the image's own copy, whichever memory the caller's are in
        RC_TRY(ps.alloc((size_t)n, &img->numbers));
        HIP_TRY(hipMemcpyAsync(img->numbers, opt->numbers, (size_t)n * 8,
                               opt->numbers_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
        numbers = img->numbers;
    }
    u32 *ex32 = nullptr;
    unsigned long long *res = nullptr;
    RC_TRY(ps.alloc((size_t)n + 1, &ex32));
    RC_TRY(ps.alloc(2, &res));
    prof_mark(ctx, "export_plan");
    if (names)
        HIP_TRY(launch_export_plan_named(table->seq_starts, n, names->off, img->fmt, ex32, res, st));
    else
        HIP_TRY(launch_export_plan(table->seq_starts, n, numbers, img->name_base, img->fmt, ex32, res, st));
    u64 got[2] = {0, 0};
    RC_TRY(read_back(ctx, got, res, sizeof got));    // (waits for the stream: the caller's numbers have been read)
    if (got[0] > U32_MAX64) {
        set_err("table_to_text: %llu bytes of headers, terminators and quality lines exceed 2^32 - 1; split the table with dnagpu_dna_take",
                (unsigned long long)got[0]);
        return DNAGPU_ERR_TOO_LARGE;
    }
    u32 *scan_tmp = nullptr;
    RC_TRY(ps.alloc((size_t)scan_tmp_words(n), &scan_tmp));
    RC_TRY(ps.alloc((size_t)n + 1 + EXPORT_PREFIX_MAX / 8, &img->pos));
    prof_mark(ctx, "export_offsets");
    HIP_TRY(launch_scan_u32(ex32, ex32, n, scan_tmp, nullptr, st));
    HIP_TRY(launch_export_pos(table->seq_starts, ex32, n, got[0], img->pos, st));
    for (u32 at = 0; at < img->fmt.prefix_len; at += 32)             // (as kernel arguments: no staging copy)
        HIP_TRY(poke(reinterpret_cast<unsigned char *>(img->pos + n + 1) + at, img->prefix + at, 32, st));
    prof_mark(ctx, "end");
    HIP_TRY(hipStreamSynchronize(st));
    prof_end(ctx);
    ps.release(img->pos);
    if (img->numbers)
        ps.release(img->numbers);
    img->bytes = table->n_bases + got[0];
    img->empty = got[1];
    return DNAGPU_OK;
}

}  // namespace

extern "C" int dnagpu_table_to_text(dnagpu_ctx *ctx, const dnagpu_dna *table, const dnagpu_text_out_options *opt,
                                    dnagpu_text_image **out)
{
    return guarded([&]() -> int {
    if (!ctx || !table || !opt || !out)
        return DNAGPU_ERR_BAD_ARG;
    RC_TRY(check_options(opt));
    if (table_without_set(table))
        return DNAGPU_ERR_BAD_ARG;
    std::unique_ptr<dnagpu_text_image> img(new dnagpu_text_image);
    const int rc = plan_image(ctx, table, nullptr, opt, img.get());
    if (rc != DNAGPU_OK) {                           // (what the scope of the plan had not yet handed over is already back)
        img->pos = img->numbers = nullptr;
        return rc;
    }
    *out = img.release();
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_table_to_text_named(dnagpu_ctx *ctx, const dnagpu_dna *table, const dnagpu_names *names,
                                          const dnagpu_text_out_options *opt, dnagpu_text_image **out)
{
    return guarded([&]() -> int {
    if (!ctx || !table || !names || !opt || !out)
        return DNAGPU_ERR_BAD_ARG;
    RC_TRY(check_options(opt));
    if (opt->format == DNAGPU_TEXT_LINES)
        return DNAGPU_ERR_BAD_ARG;                   // (LINES has no names)
    if (table_without_set(table))
        return DNAGPU_ERR_BAD_ARG;
    if (names->n != table->n_seqs)
        return DNAGPU_ERR_BAD_ARG;                   // (not this table's column)
    std::unique_ptr<dnagpu_text_image> img(new dnagpu_text_image);
    const int rc = plan_image(ctx, table, names, opt, img.get());
    if (rc != DNAGPU_OK) {
        img->pos = img->numbers = nullptr;
        return rc;
    }
    *out = img.release();
    return DNAGPU_OK;
    });
}

extern "C" uint64_t dnagpu_text_image_bytes(const dnagpu_text_image *img) { return img ? img->bytes : 0; }
extern "C" uint64_t dnagpu_text_image_sequences(const dnagpu_text_image *img) { return img ? img->n : 0; }
extern "C" uint64_t dnagpu_text_image_empty(const dnagpu_text_image *img) { return img ? img->empty : 0; }

namespace {

// dnagpu_text_image_read, and with quals != null dnagpu_text_image_read_quals: the same window, then the overlay
int read_window(dnagpu_ctx *ctx, const dnagpu_text_image *img, const dnagpu_quals *quals, u64 first_byte, u64 count, char *out_text,
                int out_on_device)
{
    if (first_byte > img->bytes || count > img->bytes - first_byte)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0)
        return DNAGPU_OK;
    if (count > U32_MAX64)
        return DNAGPU_ERR_TOO_LARGE;                 // (callers page)
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    unsigned char *dt = reinterpret_cast<unsigned char *>(out_text);
    if (!out_on_device)
        RC_TRY(ps.alloc((size_t)count, &dt));
    const dnagpu_dna *t = img->table;
    const ExportRead a = {t->words, t->n_words, t->n_bases, t->seq_starts, img->pos, img->numbers,
                          reinterpret_cast<const unsigned char *>(img->pos + img->n + 1), img->n, img->name_base, img->fmt,
                          first_byte, count, dt};
    if (img->names)
        HIP_TRY(launch_export_read_named(a, ExportNames{img->names->bytes, img->names->off}, ctx->stream));
    else
        HIP_TRY(launch_export_read(a, ctx->stream));
    if (quals)
        HIP_TRY(launch_quals_overlay(quals->bytes, t->seq_starts, img->pos, img->n, img->fmt.term, first_byte, count, dt, ctx->stream));
    if (!out_on_device)
        HIP_TRY(hipMemcpyAsync(out_text, dt, count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
}

}  // namespace

extern "C" int dnagpu_text_image_read(dnagpu_ctx *ctx, const dnagpu_text_image *img, uint64_t first_byte, uint64_t count,
                                      char *out_text, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !img || (count && !out_text))
        return DNAGPU_ERR_BAD_ARG;
    return read_window(ctx, img, nullptr, first_byte, count, out_text, out_on_device);
    });
}

extern "C" int dnagpu_text_image_read_quals(dnagpu_ctx *ctx, const dnagpu_text_image *img, const dnagpu_quals *quals,
                                            uint64_t first_byte, uint64_t count, char *out_text, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !img || !quals || (count && !out_text))
        return DNAGPU_ERR_BAD_ARG;
    if (img->fmt.format != EXPORT_FASTQ || quals->n != img->table->n_bases)
        return DNAGPU_ERR_BAD_ARG;
    return read_window(ctx, img, quals, first_byte, count, out_text, out_on_device);
    });
}

extern "C" int dnagpu_text_image_record_pos(dnagpu_ctx *ctx, const dnagpu_text_image *img, uint64_t first_seq, uint64_t count,
                                            uint64_t *out_pos, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !img || (count && !out_pos))
        return DNAGPU_ERR_BAD_ARG;
    const u64 entries = img->n ? img->n + 1 : 0;     // (dnagpu_dna_sequence_starts' rule: no set, no entries)
    if (first_seq > entries || count > entries - first_seq)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(out_pos, img->pos + first_seq, (size_t)count * 8,
                           out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}

extern "C" void dnagpu_text_image_free(dnagpu_ctx *ctx, dnagpu_text_image *img)
{
    if (!img)
        return;
    if (ctx) {
        if (img->pos)
            pool_free(ctx, img->pos);
        if (img->numbers)
            pool_free(ctx, img->numbers);
    }
    delete img;
}

extern "C" int dnagpu_text_out_geometry(uint64_t *tile_bytes)
{
    if (!tile_bytes)
        return DNAGPU_ERR_BAD_ARG;
    *tile_bytes = EXPORT_TILE_BYTES;
    return DNAGPU_OK;
}
